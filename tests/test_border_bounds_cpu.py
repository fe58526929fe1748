"""CPU-side checks of finite variable bounds beside coupling GeneralConstraint rows: the Solver no longer refuses them for the
bordered path (csrc/dto_solver.cpp: general_solve_batch has a barrier for variable bounds), and still refuses inequality stage
rows there.  The problems are those of tests/test_wide_general_border_cpu.py and tests/test_general_accumulators_cpu.py with action
bounds added: bounds are layout data, so the plugins are the same."""
import numpy as np

import dto_amd
from dto_amd import problems as P
from dto_amd.model import Bound, GeneralConstraint

T = 6


def _solver(p, name, **kw):
    return dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                          general_constraint=p["general_constraint"], name=name, **kw)


def _finite_bound_sides(s):
    lo, hi = s.nlp.variable_bounds
    free = lo != hi
    return int(np.sum(np.isfinite(lo[free])) + np.sum(np.isfinite(hi[free])))


def test_24_state_product_row_with_action_bounds_takes_the_bordered_path():
    p = P.build_acrobot_padded(T=T, n=24, target=0.4, terminal="physical", general_row=(2, 5, 0.2, False, "product"), u_max=2.0)
    s = _solver(p, "acrobot24gp")
    assert _finite_bound_sides(s) == 2 * (T - 1)
    assert s.solve_unsupported is None and s.general_rows_path == "border"
    assert s._solve_nlp.num_variables == (T - 1) * 65 + 64
    # the bounds of the embedded problem: the action bounds at their embedded positions, nothing else finite but the pins
    lo, hi = s._solve_nlp.variable_bounds
    free = lo != hi
    assert int(np.sum(np.isfinite(lo[free])) + np.sum(np.isfinite(hi[free]))) == 2 * (T - 1)
    assert set(np.abs(lo[free][np.isfinite(lo[free])]).tolist()) == {2.0}


def test_inequality_stage_rows_beside_general_rows_and_bounds_are_still_refused():
    p = P.build_acrobot_padded(T=T, n=24, target=0.4, terminal="physical", general_row=(2, 5, 0.2, False, "product"),
                               stage_constraints=(0.4, -2.56, 0.1), u_max=2.0)
    s = _solver(p, "acrobot24gpc")
    assert s.solve_unsupported is not None
    assert "inequality rows" in s.solve_unsupported and "beside general rows" in s.solve_unsupported
    assert "finite variable bounds" not in s.solve_unsupported


def test_lane_path_problem_with_bounds_builds_on_the_border():
    p = P.build_pendulum(T=T, evaluate_hessian=True)
    p["bounds"] = [Bound(2, 1, action_lower=-3.0 * np.ones(1), action_upper=3.0 * np.ones(1))] * (T - 1) + [Bound(2, 0)]
    p["general_constraint"] = GeneralConstraint(lambda z, w: np.array([z[3] + z[9] - 0.3], dtype=object), 2 * T + (T - 1), 0,
                                                evaluate_hessian=True)
    s = _solver(p, "pendulum_sep", options=dto_amd.Options(general_rows="border"))
    assert s.general_rows_path == "border" and s.solve_unsupported is None
    assert _finite_bound_sides(s) == 2 * (T - 1) and s._solve_nlp.sizes.num_constraint_general == 1

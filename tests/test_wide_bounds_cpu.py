"""Per-instance variable bounds on the tile path (Solver.set_bounds_batch, include/dto.h: dto_solver_set_bounds) -- the host side:
the map from the problem's layout to the solver's for problems embedded in the 64 states, the host check of the bound pattern,
and the refusal on the lane-per-instance path.  No device work."""
import numpy as np
import pytest

from dto_amd import problems as P
from dto_amd.solver import check_bounds_pattern

T = 30


def _solver(n, stage_constraints=None, u_max=None, name=None):
    import dto_amd
    p = P.build_acrobot_padded(T=T, n=n, target=0.4, terminal="physical", stage_constraints=stage_constraints, u_max=u_max)
    return dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name=name), p


@pytest.fixture(scope="module")
def s40():
    """The 40-state model with bounds on its endpoints (tests/test_wide_gpu.py, embedded in the 64 states)."""
    return _solver(40, name="acrobot40")[0]


@pytest.fixture(scope="module")
def s40c():
    """The 40-state model whose endpoint rows pins_to_bounds restates as bounds (tests/test_wide_gpu.py)."""
    return _solver(40, stage_constraints=(0.43, -2.21, 0.08), name="acrobot40c")[0]


def _per_instance(s, B, rng):
    """Per-instance bounds of the 40-state problem: its own with new first-knot values and new finite terminal values."""
    lo, hi = s.nlp.variable_bounds
    L, U = np.tile(lo, (B, 1)), np.tile(hi, (B, 1))
    fixed = lo == hi
    V = np.where(fixed, lo + 0.1 * rng.standard_normal((B, lo.size)), 0.0)
    L[:, fixed], U[:, fixed] = V[:, fixed], V[:, fixed]
    return L, U


def test_embedded_bounds_map_to_the_solver_layout(s40):
    n, B = 40, 3
    assert s40._pad is not None and not s40._pins
    lo, hi = s40.nlp.variable_bounds
    slo, shi = s40._solve_nlp.variable_bounds
    assert np.sum(lo == hi) == n + 4                       # first knot and the four physical states of the last
    L, U = _per_instance(s40, B, np.random.default_rng(1))
    check_bounds_pattern(L, U, lo, hi)
    ML, MU = s40.bounds_to_solver_layout(L, U)
    assert ML.shape == (B, s40._solve_nlp.num_variables) == MU.shape
    zmap = np.asarray(s40._pad[0])
    assert np.array_equal(ML[:, zmap], L) and np.array_equal(MU[:, zmap], U)
    other = np.setdiff1d(np.arange(slo.size), zmap)
    assert other.size > 0
    assert np.array_equal(ML[:, other], np.tile(slo[other], (B, 1))) and np.array_equal(MU[:, other], np.tile(shi[other], (B, 1)))
    # the padding states of the first knot stay fixed at zero, the solver's pattern is kept everywhere
    assert np.all(ML[:, n:64] == 0.0) and np.all(MU[:, n:64] == 0.0)
    check_bounds_pattern(ML, MU, slo, shi)
    # bounds equal to the shared ones map to the solver's shared bounds
    SL, SU = s40.bounds_to_solver_layout(np.tile(lo, (B, 1)), np.tile(hi, (B, 1)))
    assert np.array_equal(SL, np.tile(slo, (B, 1))) and np.array_equal(SU, np.tile(shi, (B, 1)))


def test_pins_of_restated_stage_rows_are_kept(s40c):
    """pins_to_bounds fixed the 40 first-knot states (and four terminal ones) from stage rows: the problem itself has (-inf, inf)
    there, the input must too, and the solver keeps its pins; the auxiliary states of the obstacle rows keep their bounds."""
    B = 2
    assert s40c._pins is not None and len(s40c._pins) == 44
    lo, hi = s40c.nlp.variable_bounds
    slo, shi = s40c._solve_nlp.variable_bounds
    pins = np.array([p for p, _ in s40c._pins])
    assert np.all(np.isinf(lo)) and np.all(np.isinf(hi)) and np.all(slo[pins] == shi[pins])
    L, U = np.tile(lo, (B, 1)), np.tile(hi, (B, 1))
    ML, MU = s40c.bounds_to_solver_layout(L, U)
    assert np.array_equal(ML, np.tile(slo, (B, 1))) and np.array_equal(MU, np.tile(shi, (B, 1)))
    assert np.any(np.isinf(slo) & np.isfinite(shi))        # the obstacle rows' auxiliary states (<= 0) are among those kept
    # a value at a pinned variable is refused: the problem's own bounds are infinite there
    L2 = L.copy()
    L2[1, 5] = U[1, 5] = 0.0
    with pytest.raises(ValueError, match="instance 1, variable 5: not fixed|instance 1, variable 5: fixed"):
        s40c.set_bounds_batch(L2, U)


def _pattern_case(kind):
    lo = np.array([0.0, -1.0, -np.inf, -np.inf, 2.0])
    hi = np.array([0.0, 1.0, np.inf, 3.0, np.inf])
    L, U = np.tile(lo, (3, 1)), np.tile(hi, (3, 1))
    L[:, 0] = U[:, 0] = [0.5, -0.5, 1.5]                  # fixed values may differ per instance
    L[:, 1], U[:, 1] = -2.0, [0.5, 1.0, 2.0]              # so may finite bounds
    if kind == "finite_where_infinite":
        L[2, 2] = -5.0
    elif kind == "infinite_where_finite":
        U[1, 3] = np.inf
    elif kind == "unfixed_where_fixed":
        U[1, 0] = L[1, 0] + 1e-3
    elif kind == "fixed_where_unfixed":
        L[2, 1] = U[2, 1]
    elif kind == "lo_gt_hi":
        L[1, 1], U[1, 1] = 0.5, 0.25
    elif kind == "nan":
        L[2, 4] = np.nan
    return L, U, lo, hi


def test_pattern_check_accepts_the_problems_pattern_with_other_values():
    L, U, lo, hi = _pattern_case(None)
    check_bounds_pattern(L, U, lo, hi)


@pytest.mark.parametrize("kind,where,why", [
    ("finite_where_infinite", (2, 2), "finite lower bound where the problem's is infinite"),
    ("infinite_where_finite", (1, 3), "infinite upper bound where the problem's is finite"),
    ("unfixed_where_fixed", (1, 0), "not fixed"),
    ("fixed_where_unfixed", (2, 1), "fixed \\(lower == upper\\) where the problem's variable is not"),
    ("lo_gt_hi", (1, 1), "lower >= upper"),
    ("nan", (2, 4), "NaN"),
])
def test_pattern_check_names_instance_and_variable(kind, where, why):
    L, U, lo, hi = _pattern_case(kind)
    with pytest.raises(ValueError, match=f"instance {where[0]}, variable {where[1]}: {why}"):
        check_bounds_pattern(L, U, lo, hi)


def test_set_bounds_batch_checks_numpy_input_on_the_host(s40):
    B = 2
    lo, hi = s40.nlp.variable_bounds
    L, U = _per_instance(s40, B, np.random.default_rng(2))
    free = np.flatnonzero(np.isinf(lo))
    L[1, free[3]] = -1.0                                   # finite where the problem's lower bound is infinite
    with pytest.raises(ValueError, match=f"instance 1, variable {free[3]}: finite lower bound"):
        s40.set_bounds_batch(L, U)
    L, U = _per_instance(s40, B, np.random.default_rng(2))
    for bad in ((L[:, :-1], U[:, :-1]), (L[0], U[0]), (L, U[:1])):
        with pytest.raises(ValueError, match="lower and upper are"):
            s40.set_bounds_batch(*bad)
    with pytest.raises(ValueError, match="both None or both given"):
        s40.set_bounds_batch(L, None)


def test_lane_path_solver_refuses_per_instance_bounds():
    from conftest import product_solver
    s, _ = product_solver("pendulum", 6)
    lo, hi = s.nlp.variable_bounds
    with pytest.raises(ValueError, match="parameters in stage rows"):
        s.set_bounds_batch(np.tile(lo, (2, 1)), np.tile(hi, (2, 1)))
    with pytest.raises(ValueError, match="build_mpc_pendulum"):
        s.set_bounds_batch(None, None)

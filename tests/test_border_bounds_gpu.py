"""Finite variable bounds beside coupling GeneralConstraint rows on the bordered path, lane-per-instance linear solver
(csrc/dto_solver.cpp: general_solve_batch = the border_loop_* phases over a BorderLoop, bordered_step_device;
csrc/dto_border_kernels.hpp: k_border_rx, k_border_sig, k_border_stats, BorderBar, k_border_bar_stats,
k_border_trial).  The pendulum swing-up of tests/test_general_accumulators_gpu.py, T = 50: Nz = 149 is no multiple of the
wavefront, so the tail of every per-instance reduction is exercised.

References: the ORACLE's KKT report of its own restatement of the problem (oracle/sympy_models.py: build_coupled), with the limits
test_pendulum_with_a_coupling_row_and_bounds_on_the_accumulator_path uses for the same problem, and the accumulator path's
minimiser from the same guess (Options.general_rows = "auto"), within the 1e-3 in max-norm that file uses for border against
accumulators without bounds.  Measured distances on an MI355X: 2.7e-9 (inequality row), 2.1e-7 (equality row), 1.0e-8 / 1.4e-7
(upper / lower bound only), 4.1e-6 (nonlinear row) -- the limit stands as it is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, U_MAX = 50, 3.0
I15, I35 = 14 * 3, 34 * 3
U_IDX = [t * 3 + 2 for t in range(T - 1)]
PATH_DISTANCE = 1e-3

# Total of the nonlinear row sin(theta_15) + theta_35^2 = total beside |u| <= 3: the value of the expression at the solution WITH
# the bound and WITHOUT the row (NL_FREE_VALUE, checked in the test against a fresh solve) moved by 0.3.
NL_FREE_VALUE = 2.98              # measured 2.9831 (theta_15 = -0.3111, theta_35 = 1.8136)
NL_TOTAL = 2.68


def _both_paths(p, name):
    from test_general_accumulators_gpu import _solve
    sb, stb = _solve(p, name, "border", scale=0.1)
    assert stb == 1 and sb.general_rows_path == "border" and sb.solve_unsupported is None, (stb, sb.general_rows_path, sb.iterations)
    sa, sta = _solve(p, name, "auto", scale=0.1)
    assert sta == 1 and sa.general_rows_path == "accumulators", (sta, sa.general_rows_path, sa.iterations)
    d = np.max(np.abs(sb._solution - sa._solution))
    print(f"[{name}] border {sb.iterations} iterations, accumulators {sa.iterations} iterations, distance of the minimisers {d:.3e}")
    return sb, sa, d


def _report(sb, **kw):
    from test_general_accumulators_gpu import _oracle
    from test_solve_gpu import kkt_report
    rep = kkt_report(_oracle("pendulum_coupled", **kw), sb._solution, sb._duals)
    print("  ", {k: (float(v) if not isinstance(v, bool) else v) for k, v in rep.items()})
    assert rep["violation"] <= 1e-6 and rep["bound_viol"] <= 1e-12 and rep["sign_ok"], rep
    assert rep["stationarity"] <= 1e-3 and rep["compl"] <= 1e-3, rep
    return rep


@pytest.mark.parametrize("inequality", [True, False])
def test_two_sided_bounds_beside_the_coupling_row(inequality):
    """theta_15 + theta_35 (<= | =) 1 and |u| <= 3 at every knot: the bound binds (the free control peaks at 4.9) and so does the
    row (without it the sum is 1.449).  With the equality row the problem has bounds and no slack: the barrier parameter is set by
    the bounds alone."""
    from dto_amd import problems as P
    p = P.build_pendulum_coupled(T=T, total=1.0, inequality=inequality, u_max=U_MAX)
    sb, sa, d = _both_paths(p, "pendulum_coupled")
    z, lam = sb._solution, sb._duals
    _report(sb, total=1.0, u_max=U_MAX, inequality=inequality)
    u = z[U_IDX]
    assert np.max(np.abs(u)) <= U_MAX + 1e-12 and np.sum(np.abs(u) > U_MAX - 1e-2) >= 1, np.max(np.abs(u))
    assert abs(z[I15] + z[I35] - 1.0) < 1e-3 and lam[-1] > 0.1, (z[I15] + z[I35], lam[-1])
    assert d <= PATH_DISTANCE, d


def test_one_sided_bounds():
    """u <= 3 only, and u >= -3 only: each side of a bound is a barrier term of its own."""
    from dto_amd import problems as P
    from dto_amd.model import Bound
    active = []
    for side in ("upper", "lower"):
        p = P.build_pendulum_coupled(T=T, total=1.0, inequality=True)
        kw = dict(action_upper=np.array([U_MAX])) if side == "upper" else dict(action_lower=np.array([-U_MAX]))
        p["bounds"] = [Bound(2, 1, **kw)] * (T - 1) + [Bound(2, 0)]
        sb, sa, d = _both_paths(p, "pendulum_coupled")
        u = sb._solution[U_IDX]
        if side == "upper":
            assert np.max(u) <= U_MAX + 1e-12, np.max(u)
            active.append(bool(np.any(u > U_MAX - 1e-2)))
        else:
            assert np.min(u) >= -U_MAX - 1e-12, np.min(u)
            active.append(bool(np.any(u < -U_MAX + 1e-2)))
        print(f"  {side} bound only: u in [{np.min(u):.4f}, {np.max(u):.4f}], active {active[-1]}")
        assert d <= PATH_DISTANCE, (side, d)
    assert any(active), active                    # the free control peaks at 4.9 in magnitude: one side must bind


def test_a_row_only_the_border_carries_as_a_row():
    """sin(theta_15) + theta_35^2 = NL_TOTAL beside |u| <= 3, kept a row by Options(general_rows="border") ("auto" lets its
    one-knot terms ride an accumulator state: the reference minimiser)."""
    import dto_amd
    from dto_amd import problems as P
    from dto_amd.model import Bound
    # the literal: the bounded solution without the row
    pf = P.build_pendulum(T=T, evaluate_hessian=True)
    pf["bounds"] = [Bound(2, 1, action_lower=-U_MAX * np.ones(1), action_upper=U_MAX * np.ones(1))] * (T - 1) + [Bound(2, 0)]
    sf = dto_amd.Solver(pf["dynamics"], pf["objective"], pf["constraints"], pf["bounds"], evaluate_hessian=True, name="pendulum")
    xs, us = pf["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(sf, xs); dto_amd.initialize_controls(sf, [0.1 * u for u in us])
    assert dto_amd.solve(sf) == 1
    zf = sf._solution
    free = np.sin(zf[I15]) + zf[I35] ** 2
    print(f"[pendulum, |u| <= 3, no row] sin(theta_15) + theta_35^2 = {free:.4f}, peak |u| {np.max(np.abs(zf[U_IDX])):.4f}")
    assert abs(free - NL_FREE_VALUE) <= 5.1e-3 and abs(abs(NL_TOTAL - NL_FREE_VALUE) - 0.3) < 1e-12, (free, NL_FREE_VALUE, NL_TOTAL)
    p = P.build_pendulum_coupled(T=T, total=NL_TOTAL, inequality=False, nonlinear=True, u_max=U_MAX)
    sb, sa, d = _both_paths(p, "pendulum_coupled_nl")
    z, lam = sb._solution, sb._duals
    _report(sb, total=NL_TOTAL, inequality=False, nonlinear=True, u_max=U_MAX)
    assert abs(np.sin(z[I15]) + z[I35] ** 2 - NL_TOTAL) <= 1e-6 and abs(lam[-1]) > 1e-3, lam[-1]
    assert np.max(np.abs(z[U_IDX])) <= U_MAX + 1e-12
    assert d <= PATH_DISTANCE, d


def test_batch_instances_do_not_see_each_other():
    """Three guesses in one solve_batch against the same three solved alone: step lengths, barrier parameters and reductions are
    per instance."""
    import torch
    import dto_amd
    from dto_amd import problems as P
    p = P.build_pendulum_coupled(T=T, total=1.0, inequality=True, u_max=U_MAX)
    o = dto_amd.Options()
    o.general_rows = "border"
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], options=o, name="pendulum_coupled")
    assert s.general_rows_path == "border"
    B, nz = 3, s.nlp.num_variables
    Z = np.zeros((B, nz))
    for b in range(B):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s._z0

    def run(rows):
        z0 = torch.tensor(np.ascontiguousarray(Z[rows]), device="cuda")
        zo = torch.full((len(rows), nz), float("nan"), device="cuda", dtype=torch.float64)
        st, it = s.solve_batch(z0.data_ptr(), len(rows), nz, zo.data_ptr(), nz)
        torch.cuda.synchronize()
        return zo.cpu().numpy(), st, it
    zb, st, it = run([0, 1, 2])
    print(f"[batch of 3] status {st.tolist()}, iterations {it.tolist()}")
    assert np.all(st == 1), (st, it)
    for b in range(B):
        z1, st1, it1 = run([b])
        assert st1[0] == 1 and it1[0] == it[b], (b, st1, it1, it)
        assert np.max(np.abs(z1[0] - zb[b])) <= 1e-9, (b, np.max(np.abs(z1[0] - zb[b])))
        assert np.max(np.abs(zb[b][U_IDX])) <= U_MAX + 1e-12

"""Inequality rows of stage Constraints beside coupling GeneralConstraint rows on the bordered path, lane-per-instance linear solver
with the device border (csrc/dto_solver.cpp: general_solve_batch = the border_loop_* phases over a BorderLoop, bordered_step_device;
csrc/dto_border_kernels.hpp: k_border_rhsc, k_border_stats, BorderSlack,
k_border_slack_init / _stats / _update, k_border_trial).  The pendulum swing-up of tests/test_border_bounds_gpu.py, T = 50, with a
speed limit thetadot^2 - v^2 <= 0 as a stage row at EVERY knot (examples/car/car.jl:53-60 style): Nz = 149 variables and
Ns = 98 + 4 + 50 = 152 dynamics and stage rows, neither a multiple of the wavefront, so the tail of every per-instance reduction is
exercised.

References: the ORACLE's KKT report of its own restatement of the problem (built below from oracle/sympy_models.py classes) with the
limits of tests/test_border_bounds_gpu.py::_report, and the accumulator path's minimiser from the same guess within the 1e-3 in
max-norm (PATH_DISTANCE) that file uses for border against accumulators.

The thresholds that make a constraint bind are literals of the generated plugins; each is derived here from a fresh solve without
that constraint.  Measured on an MI355X: sum row 15 iterations on the border, 26 on an accumulator state, distance 1.3e-6; product
row beside the bound 20 iterations; a batch of three guesses 15 / 15 / 15, each equal to its solve alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 50
I15, I35 = 14 * 3, 34 * 3
U_IDX = [t * 3 + 2 for t in range(T - 1)]
V_IDX = [t * 3 + 1 for t in range(T)]
PATH_DISTANCE = 1e-3

# The speed limit: 0.8 x the peak |thetadot| of the swing-up without it, to two decimals.
FREE_PEAK_SPEED = 4.184           # measured 4.1841 (knot 32)
V_MAX = 3.35
# The action bound |u| <= U_MAX beside the speed limit.  With the limit and without a bound the control peaks at 5.196.  At the
# |u| <= 3 of tests/test_border_bounds_gpu.py, and at 3.5, the problem WITHOUT a general row -- the ordinary lane loop -- ran into the
# 1000-iteration limit from this guess (the speed stays above the limit: 3.376 and 3.389), so the bound was moved towards the free
# peak: at 4.0 that problem converges in 23 iterations (4.5: 22, 5.0: 18) and the bound binds.
U_MAX = 4.0
# Total of the product row theta_15 * theta_35 = total beside the speed limit and |u| <= U_MAX: the value of the product at the
# solution WITH both and WITHOUT the row (PROD_FREE_VALUE, checked in the test against a fresh solve) moved by 0.1.
PROD_FREE_VALUE = -0.49           # measured -0.4851 (theta_15 = -0.2449, theta_35 = 1.9812)
PROD_TOTAL = -0.39


def _oracle(row=None, total=1.0, u_max=None):
    from oracle import dto_oracle as O, sympy_models as S
    p = S.build("pendulum", T, evaluate_hessian=True)
    n, m = 2, 1
    x1, xT = [0.0, 0.0], [S.PI, 0.0]
    v2 = S.fl(V_MAX) ** 2
    speed = lambda x: x[1] * x[1] - v2
    con1 = S.Constraint(lambda x, u, w: [a - S.fl(b) for a, b in zip(x, x1)] + [speed(x)], n, m, indices_inequality=[3], evaluate_hessian=True)
    cont = S.Constraint(lambda x, u, w: [speed(x)], n, m, indices_inequality=[1], evaluate_hessian=True)
    conT = S.Constraint(lambda x, u, w: [a - S.fl(b) for a, b in zip(x, xT)] + [speed(x)], n, 0, indices_inequality=[3], evaluate_hessian=True)
    cons = [con1] + [cont] * (T - 2) + [conT]
    bnds = p["bounds"] if u_max is None else [S.Bound(n, m, action_lower=[-u_max], action_upper=[u_max])] * (T - 1) + [S.Bound(n, 0)]
    nz = n * T + m * (T - 1)
    tot = S.fl(total)
    gc = None
    if row == "sum<=0":
        gc = S.GeneralConstraint(lambda z, w: [z[I15] + z[I35] - tot], nz, 0, indices_inequality=[1], evaluate_hessian=False)
    elif row == "product":
        gc = S.GeneralConstraint(lambda z, w: [z[I15] * z[I35] - tot], nz, 0, evaluate_hessian=False)
    return O.NLPData(p["dynamics"], p["objective"], cons, bnds, evaluate_hessian=True, general_constraint=gc)


def _report(onlp, s):
    from test_solve_gpu import kkt_report
    rep = kkt_report(onlp, s._solution, s._duals)
    print("  ", {k: (float(v) if not isinstance(v, bool) else v) for k, v in rep.items()})
    assert rep["violation"] <= 1e-6 and rep["bound_viol"] <= 1e-12 and rep["sign_ok"], rep
    assert rep["stationarity"] <= 1e-3 and rep["compl"] <= 1e-3, rep
    return rep


def _stage_rows(onlp, s):
    """values and multipliers of the inequality stage rows at the solution (reference row order: general rows last)"""
    clo, _ = onlp.constraint_bounds
    ineq = np.isneginf(clo)
    ineq[onlp.num_dynamics + onlp.num_stage:] = False
    assert int(np.sum(ineq)) == T
    return onlp.eval_constraint(s._solution)[ineq], s._duals[ineq]


def _free(name, p):
    import dto_amd
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name=name)
    xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
    assert dto_amd.solve(s) == 1
    return s._solution


def test_speed_limit_beside_a_coupling_row_kept_on_the_border():
    """thetadot^2 <= V_MAX^2 at every knot beside theta_15 + theta_35 <= 1, the row kept on the border by Options(general_rows="border")
    ("auto" lets it ride an accumulator state through the ordinary device loop, which takes stage inequalities: the reference
    minimiser).  The limit binds (it is 0.8 x the free peak) and so does the row."""
    from dto_amd import problems as P
    from test_general_accumulators_gpu import _solve
    zf = _free("pendulum", P.build_pendulum(T=T, evaluate_hessian=True))
    peak = np.max(np.abs(zf[V_IDX]))
    print(f"[pendulum, no limit, no row] peak |thetadot| {peak:.4f} at knot {int(np.argmax(np.abs(zf[V_IDX]))) + 1}, "
          f"theta_15 + theta_35 = {zf[I15] + zf[I35]:.4f}")
    assert abs(peak - FREE_PEAK_SPEED) <= 5.1e-4 and abs(V_MAX - 0.8 * FREE_PEAK_SPEED) <= 5.1e-3, (peak, FREE_PEAK_SPEED, V_MAX)
    p = P.build_pendulum_speed_limit(T=T, v_max=V_MAX, row="sum<=0", total=1.0)
    sb, stb = _solve(p, "pendulum_speed", "border", scale=0.1)
    print(f"[speed limit + sum row] border: status {stb}, {sb.iterations} iterations")
    assert stb == 1 and sb.general_rows_path == "border" and sb.solve_unsupported is None, (stb, sb.general_rows_path, sb.iterations)
    sa, sta = _solve(p, "pendulum_speed", "auto", scale=0.1)
    assert sta == 1 and sa.general_rows_path == "accumulators", (sta, sa.general_rows_path, sa.iterations)
    d = np.max(np.abs(sb._solution - sa._solution))
    print(f"  accumulators: {sa.iterations} iterations, distance of the minimisers {d:.3e}")
    onlp = _oracle("sum<=0", 1.0)
    _report(onlp, sb)
    z, lam = sb._solution, sb._duals
    c, nu = _stage_rows(onlp, sb)
    print(f"  stage rows: max c {np.max(c):.3e}, active {int(np.sum((c > -1e-3) & (nu > 1e-3)))}, min nu {np.min(nu):.3e}, max nu {np.max(nu):.3e}; "
          f"theta_15 + theta_35 = {z[I15] + z[I35]:.6f}, its multiplier {lam[-1]:.4f}")
    assert np.sum((c > -1e-3) & (nu > 1e-3)) >= 1 and np.min(nu) >= 0.0 and lam[-1] >= 0.0
    assert abs(z[I15] + z[I35] - 1.0) < 1e-3 and lam[-1] > 1e-3, (z[I15] + z[I35], lam[-1])
    assert np.max(np.abs(z[V_IDX])) <= V_MAX + 1e-6
    assert d <= PATH_DISTANCE, d


def test_equality_and_inequality_stage_rows_bounds_and_a_border_only_row_at_once():
    """The same stage rows beside theta_15 * theta_35 = PROD_TOTAL (no sum of one-knot terms: only the border carries it) and
    |u| <= U_MAX: equality stage rows (the endpoints), inequality stage rows, bounds and the border, one barrier parameter."""
    import dto_amd
    from dto_amd import problems as P
    zf = _free("pendulum_speed", P.build_pendulum_speed_limit(T=T, v_max=V_MAX, u_max=U_MAX))
    free = zf[I15] * zf[I35]
    print(f"[speed limit, |u| <= {U_MAX}, no row] theta_15 * theta_35 = {free:.4f} ({zf[I15]:.4f}, {zf[I35]:.4f}), peak |u| {np.max(np.abs(zf[U_IDX])):.4f}, "
          f"peak |thetadot| {np.max(np.abs(zf[V_IDX])):.4f}")
    assert abs(free - PROD_FREE_VALUE) <= 5.1e-3 and abs(abs(PROD_TOTAL - PROD_FREE_VALUE) - 0.1) < 1e-12, (free, PROD_FREE_VALUE, PROD_TOTAL)
    p = P.build_pendulum_speed_limit(T=T, v_max=V_MAX, row="product", total=PROD_TOTAL, u_max=U_MAX)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], name="pendulum_speed_prod")
    assert s.general_rows_path == "border" and s.solve_unsupported is None
    xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
    st = dto_amd.solve(s)
    print(f"[speed limit + |u| <= {U_MAX} + product row] status {st}, {s.iterations} iterations")
    assert st == 1, (st, s.iterations)
    onlp = _oracle("product", PROD_TOTAL, U_MAX)
    _report(onlp, s)
    z, lam = s._solution, s._duals
    c, nu = _stage_rows(onlp, s)
    print(f"  stage rows: max c {np.max(c):.3e}, active {int(np.sum((c > -1e-3) & (nu > 1e-3)))}, min nu {np.min(nu):.3e}; "
          f"product {z[I15] * z[I35]:.6f}, its multiplier {lam[-1]:.4f}, peak |u| {np.max(np.abs(z[U_IDX])):.4f}")
    assert abs(z[I15] * z[I35] - PROD_TOTAL) <= 1e-6 and abs(lam[-1]) > 1e-3, (z[I15] * z[I35], lam[-1])
    assert np.min(nu) >= 0.0 and np.max(np.abs(z[U_IDX])) <= U_MAX + 1e-12 and np.max(np.abs(z[V_IDX])) <= V_MAX + 1e-6
    assert np.sum(np.abs(z[U_IDX]) > U_MAX - 1e-2) >= 1 and np.sum((c > -1e-3) & (nu > 1e-3)) >= 1      # both kinds of barrier bind


def _border_solver():
    import dto_amd
    from dto_amd import problems as P
    p = P.build_pendulum_speed_limit(T=T, v_max=V_MAX, row="sum<=0", total=1.0)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], options=dto_amd.Options(general_rows="border"), name="pendulum_speed")
    assert s.general_rows_path == "border"
    return s, p


def test_batch_instances_do_not_see_each_other():
    """Three guesses in one solve_batch against the same three solved alone: slacks, step lengths, barrier parameters and reductions
    are per instance."""
    import torch
    import dto_amd
    s, p = _border_solver()
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
        err = np.max(np.abs(z1[0] - zb[b]))
        assert err <= 1e-9 * max(1.0, np.max(np.abs(zb[b]))), (b, err)
        assert np.max(np.abs(zb[b][V_IDX])) <= V_MAX + 1e-6


def test_host_border_refuses_inequality_stage_rows(monkeypatch):
    import dto_amd
    from dto_amd import capi
    s, p = _border_solver()
    xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
    monkeypatch.setenv("DTO_BORDER_HOST", "1")
    with pytest.raises(capi.DtoError) as e:
        dto_amd.solve(s)
    assert e.value.code == 4 and "inequality stage rows" in str(e.value) and "device border" in str(e.value)

"""Per-instance parameters (dto_batch.params) on the bordered path (csrc/dto_solver.cpp: general_solve_batch, whose BorderLoop
keeps the batch with its params / ldp for every phase), both linear solvers.

Lane path: problems.py: build_mpc_pendulum_coupled -- the MPC pendulum of tests/test_solve_gpu.py::test_per_instance_parameters_mpc_batch
with a coupling row whose right-hand side is a parameter, theta_15 + theta_35 - w[3] <= 0 (a per-rollout budget).  A row that reads
w takes the border whatever Options.general_rows says.  Tile path: the 64-state sum row of tests/test_wide_general_border_gpu.py
on the parametric model (torque gain, weight of the state cost), checked against the oracle's PaddedAcrobot(64, 1, pair) of every
instance.

Tolerances are those of the neighbouring tests: a batch instance against its solve alone -- equal iteration counts and
1e-9 max(1, |z|); KKT steps -- 1e-8 of max |solution| against the dense solve; callbacks -- the 1e-8 relative of smoke() and
tests/test_eval_gpu.py, and for the affine row itself 1e-14 of the sum of its terms' magnitudes (three terms, two roundings).

Measured on an MI355X: lane batch 6 / 9 / 9 / 6 / 6 iterations, equal to the solves alone; step errors <= 1.1e-14 at a solution of
size 2; tile solves 141 / 96 / 60 iterations, instances 0 and 2 2.1 apart."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, B = 50, 5
I15, I35 = 14 * 3, 34 * 3

# theta_15 + theta_35 of every instance at ITS solution without the row (build_mpc_pendulum at T = 50 with the instance's x1 and
# goal, checked in the test against a fresh batch solve), to two decimals; the budgets: below it by 0.3 for instances 0, 2, 4 (the
# row binds), above it by 0.3 for instances 1, 3 (it does not)
FREE_SUMS = [0.06, 0.18, 0.52, -0.05, -0.15]          # measured 0.0564, 0.1786, 0.5152, -0.0536, -0.1471
TOTALS = [f + d for f, d in zip(FREE_SUMS, (-0.3, 0.3, -0.3, 0.3, -0.3))]


def _instances():
    rng = np.random.default_rng(11)               # (the rollouts of tests/test_solve_gpu.py)
    x1s = 0.3 * rng.standard_normal((B, 2))
    goals = np.pi * (0.5 + 0.5 * rng.random(B))
    us = [[0.1 * rng.standard_normal(1) for _ in range(T - 1)] for _ in range(B)]
    return x1s, goals, us


def _guesses(s, x1s, goals, us):
    import dto_amd
    Z = np.zeros((B, s.nlp.num_variables))
    for b in range(B):
        dto_amd.initialize_states(s, dto_amd.linear_interpolation(x1s[b], np.array([goals[b], 0.0]), T))
        dto_amd.initialize_controls(s, us[b])
        Z[b] = s._z0
    return Z


def _coupled_solver(**kw):
    import dto_amd
    from dto_amd import problems as P
    p = P.build_mpc_pendulum_coupled(T=T, **kw)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], parameters=p["parameters"], name="mpc_pendulum_coupled")
    assert s.general_rows_path == "border" and s.solve_unsupported is None and s.nlp.num_parameters == 4 * T
    return s


def _oracle(x1, goal, total):
    """the oracle's restatement of build_mpc_pendulum_coupled with one instance's parameters"""
    from oracle import dto_oracle as O, sympy_models as S
    n, m, nw = 2, 1, 4
    dt = S.Dynamics(S.pendulum_midpoint, n, n, m, num_parameter=nw, evaluate_hessian=True)
    ct = S.Cost(lambda x, u, w: S.fl(0.1) * S.dot(x, x) + S.fl(0.1) * S.dot(u, u), n, m, num_parameter=nw, evaluate_hessian=True)
    cT = S.Cost(lambda x, u, w: S.fl(0.1) * S.dot(x, x), n, 0, num_parameter=nw, evaluate_hessian=True)
    con1 = S.Constraint(lambda x, u, w: [x[0] - w[0], x[1] - w[1]], n, m, num_parameter=nw, evaluate_hessian=True)
    conT = S.Constraint(lambda x, u, w: [x[0] - w[2], x[1]], n, 0, num_parameter=nw, evaluate_hessian=True)
    nz = n * T + m * (T - 1)
    gc = S.GeneralConstraint(lambda z, w: [z[I15] + z[I35] - w[3]], nz, nw * T, indices_inequality=[1], evaluate_hessian=False)
    w = np.array([x1[0], x1[1], goal, total], dtype=float)
    return O.NLPData([dt] * (T - 1), [ct] * (T - 1) + [cT], [con1] + [S.Constraint() for _ in range(T - 2)] + [conT],
                     [S.Bound(n, m)] * (T - 1) + [S.Bound(n, 0)], evaluate_hessian=True, general_constraint=gc,
                     parameters=[w.copy() for _ in range(T)])


def test_general_row_callbacks_read_the_instance_parameters():
    """dto_eval_g_batch / dto_eval_jac_g_batch with dto_batch.params against the oracle evaluated with each instance's w: the general
    row is handed the whole flattened vector of ITS instance."""
    import ctypes as C
    import torch
    from dto_amd import capi
    s = _coupled_solver()
    n = s.nlp
    nz, nc, nj, nw = n.num_variables, n.num_constraint, n.num_jacobian, n.num_parameters
    x1s, goals, _ = _instances()
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((B, nz))
    totals = 1.0 + rng.standard_normal(B)
    W = np.stack([np.tile([x1s[b, 0], x1s[b, 1], goals[b], totals[b]], T) for b in range(B)])
    z, w = torch.tensor(Z, device="cuda"), torch.tensor(W, device="cuda")
    c = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    J = torch.full((B, nj), float("nan"), device="cuda", dtype=torch.float64)
    bt = n._batch(z.data_ptr(), B, nz, 0, w.data_ptr(), nw)
    capi.check(n._lib.dto_eval_g_batch(n._h, C.byref(bt), c.data_ptr(), nc))
    capi.check(n._lib.dto_eval_jac_g_batch(n._h, C.byref(bt), J.data_ptr(), nj))
    torch.cuda.synchronize()
    c, J = c.cpu().numpy(), J.cpu().numpy()
    for b in range(B):
        o = _oracle(x1s[b], goals[b], totals[b])
        assert o.jacobian_structure() == n.jacobian_structure()
        for got, ref in ((c[b], o.eval_constraint(Z[b])), (J[b], o.eval_constraint_jacobian(Z[b]))):
            err = np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3 * np.max(np.abs(ref))))
            assert err < 1e-8, (b, err)
        assert abs(c[b, -1] - (Z[b, I15] + Z[b, I35] - totals[b])) <= 1e-14 * (abs(Z[b, I15]) + abs(Z[b, I35]) + abs(totals[b]))


@pytest.fixture(scope="module")
def lane_batch():
    """the batch solve with per-instance x1, goal and budget, and the free sums of the same rollouts without the row"""
    import torch
    import dto_amd
    from dto_amd import problems as P
    x1s, goals, us = _instances()
    pf = P.build_mpc_pendulum(T=T)
    sf = dto_amd.Solver(pf["dynamics"], pf["objective"], pf["constraints"], pf["bounds"], evaluate_hessian=True,
                        parameters=pf["parameters"], name="mpc_pendulum")
    nz = sf.nlp.num_variables
    Z = _guesses(sf, x1s, goals, us)

    def solve(s, W):
        z0, w = torch.tensor(Z, device="cuda"), torch.tensor(W, device="cuda")
        zo = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
        st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, params_ptr=w.data_ptr(), ldp=W.shape[1])
        torch.cuda.synchronize()
        return zo.cpu().numpy(), st, it
    zf, stf, itf = solve(sf, np.stack([np.tile([x1s[b, 0], x1s[b, 1], goals[b]], T) for b in range(B)]))
    assert np.all(stf == 1), (stf, itf)
    free = zf[:, I15] + zf[:, I35]
    print(f"[mpc pendulum, T = {T}, no row] theta_15 + theta_35 = {np.round(free, 4).tolist()}, iterations {itf.tolist()}")
    s = _coupled_solver()
    W = np.stack([np.tile([x1s[b, 0], x1s[b, 1], goals[b], TOTALS[b]], T) for b in range(B)])
    zo, st, it = solve(s, W)
    print(f"[mpc pendulum + budget row, batch of {B}] status {st.tolist()}, iterations {it.tolist()}, "
          f"sums {np.round(zo[:, I15] + zo[:, I35], 6).tolist()}, budgets {TOTALS}")
    return dict(s=s, x1s=x1s, goals=goals, Z=Z, free=free, zo=zo, st=st, it=it)


def test_budgets_are_the_free_sums_moved_by_0_3(lane_batch):
    free = lane_batch["free"]
    assert np.max(np.abs(free - np.array(FREE_SUMS))) <= 5.1e-3, (free.tolist(), FREE_SUMS)


def test_every_instance_meets_its_own_endpoints_and_budget(lane_batch):
    L = lane_batch
    assert np.all(L["st"] == 1), (L["st"], L["it"])
    idx = L["s"].nlp.indices
    for b in range(B):
        z = L["zo"][b]
        xa, xb = z[np.array(idx.states[0]) - 1], z[np.array(idx.states[-1]) - 1]
        assert np.linalg.norm(xa - L["x1s"][b]) < 1e-3 and abs(xb[0] - L["goals"][b]) < 1e-3 and abs(xb[1]) < 1e-3, (b, xa, xb)
        row = z[I15] + z[I35]
        assert row <= TOTALS[b] + 1e-6, (b, row, TOTALS[b])
        if TOTALS[b] < L["free"][b]:
            assert row >= TOTALS[b] - 1e-3, (b, row, TOTALS[b])            # active: the budget is below the free sum
        else:
            assert abs(row - L["free"][b]) <= 1e-3, (b, row, L["free"][b])   # inactive: the free solution


def test_every_instance_equals_its_solve_alone_with_shared_parameters(lane_batch):
    import dto_amd
    L = lane_batch
    for b in range(B):
        sb = _coupled_solver(x1=L["x1s"][b], goal=L["goals"][b], total=TOTALS[b])
        sb._z0[:] = L["Z"][b]
        assert dto_amd.solve(sb) == 1
        assert sb.iterations == L["it"][b], (b, sb.iterations, L["it"])
        err = np.max(np.abs(sb._solution - L["zo"][b]))
        assert err <= 1e-9 * max(1.0, np.max(np.abs(L["zo"][b]))), (b, err)


def test_short_ldp_is_refused_and_nothing_is_written():
    import torch
    from dto_amd import capi
    s = _coupled_solver()
    nz, nc, nw = s.nlp.num_variables, s.nlp.num_constraint, s.nlp.num_parameters
    z0 = torch.zeros((2, nz), device="cuda", dtype=torch.float64)
    w = torch.zeros((2, nw), device="cuda", dtype=torch.float64)
    zo = torch.full((2, nz), float("nan"), device="cuda", dtype=torch.float64)
    lo = torch.full((2, nc), float("nan"), device="cuda", dtype=torch.float64)
    with pytest.raises(capi.DtoError) as e:
        s.solve_batch(z0.data_ptr(), 2, nz, zo.data_ptr(), nz, lo.data_ptr(), nc, params_ptr=w.data_ptr(), ldp=nw - 1)
    assert e.value.code == 1 and capi.STATUS_NAMES[1] == "DTO_ERR_INVALID" and "ldp < num_parameters" in str(e.value), (e.value.code, str(e.value))
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(zo))) and bool(torch.all(torch.isnan(lo)))


# ---- tile path: the 64-state sum row with per-instance (gain, weight) -----------------------------------------------------------
PAIRS = [(1.0, 1.0), (1.05, 0.95), (0.95, 1.05)]


def _tile_solver(Tn, row, **kw):
    import dto_amd
    from dto_amd import problems as P
    p = P.build_acrobot_padded(T=Tn, parameters=PAIRS[0], general_row=row, **kw)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], parameters=p["parameters"], name="acrobot_padded_par_g")
    assert s.general_rows_path == "border" and s.solve_unsupported is None and s.nlp.num_parameters == 2 * Tn
    return s, p


def test_bordered_kkt_step_on_the_tile_path_with_per_instance_parameters():
    import torch
    from oracle.padded_model import PaddedAcrobot
    from test_wide_general_border_gpu import DC, DW, STEP_ROWS, _dense_bordered, _spec
    Tn, Bn = 6, 3
    row = STEP_ROWS[0]
    s, _ = _tile_solver(Tn, row)
    nz, nc, nw = s.nlp.num_variables, s.nlp.num_constraint, s.nlp.num_parameters
    assert nc == (Tn - 1) * 64 + 1
    spec = _spec([row], 64, 1)
    rng = np.random.default_rng(41)
    Z, MU = rng.random((Bn, nz)), rng.random((Bn, nc))
    W = np.stack([np.tile(PAIRS[b], Tn) for b in range(Bn)])
    dz, dmu, dw_ = torch.tensor(Z, device="cuda"), torch.tensor(MU, device="cuda"), torch.tensor(W, device="cuda")
    dx = torch.full((Bn, nz), float("nan"), device="cuda", dtype=torch.float64)
    dl = torch.full((Bn, nc), float("nan"), device="cuda", dtype=torch.float64)
    ok = s.kkt_step_batch(dz.data_ptr(), Bn, nz, dmu.data_ptr(), nc, DW, DC, dx.data_ptr(), nz, dl.data_ptr(), nc,
                          params_ptr=dw_.data_ptr(), ldp=nw)
    torch.cuda.synchronize()
    dx, dl = dx.cpu().numpy(), dl.cpu().numpy()
    want = True
    sols = []
    for b in range(Bn):
        K, rhs = _dense_bordered(PaddedAcrobot(64, 1, PAIRS[b]), Tn, spec, Z[b], MU[b], DW, DC)
        want = want and int(np.sum(np.linalg.eigvalsh(K) < 0)) == nc
        sol = np.linalg.solve(K, rhs)
        sols.append(sol)
        scale = np.max(np.abs(sol))
        ex, el = np.max(np.abs(dx[b] - sol[:nz])), np.max(np.abs(dl[b] - sol[nz:]))
        print(f"  instance {b} (gain, weight) = {PAIRS[b]}: error {ex:.2e} / {el:.2e}, solution scale {scale:.2e}")
        assert ex <= 1e-8 * scale and el <= 1e-8 * scale, (b, ex, el, scale)
    assert bool(ok) == want, (ok, want)
    # the parameters matter at this tolerance: instance 1's step is not the step of the shared pair
    K0, rhs0 = _dense_bordered(PaddedAcrobot(64, 1, PAIRS[0]), Tn, spec, Z[1], MU[1], DW, DC)
    assert np.max(np.abs(np.linalg.solve(K0, rhs0) - sols[1])) > 1e-6 * np.max(np.abs(sols[1]))


def test_solves_on_the_tile_path_with_per_instance_parameters():
    import torch
    import dto_amd
    from oracle.padded_model import PaddedAcrobot
    from test_wide_general_border_gpu import KA, KB, SOLVE_T, TOTAL_SUM_EQ, _kkt_conditions, _spec
    Tn, Bn = SOLVE_T, 3
    row = (KA, KB, TOTAL_SUM_EQ)
    s, p = _tile_solver(Tn, row, target=0.5, terminal="physical")
    nz, nc, nw = s.nlp.num_variables, s.nlp.num_constraint, s.nlp.num_parameters
    Z = np.zeros((Bn, nz))
    for b in range(Bn):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s._z0
    W = np.stack([np.tile(PAIRS[b], Tn) for b in range(Bn)])
    z0, w = torch.tensor(Z, device="cuda"), torch.tensor(W, device="cuda")
    zo = torch.full((Bn, nz), float("nan"), device="cuda", dtype=torch.float64)
    lo = torch.full((Bn, nc), float("nan"), device="cuda", dtype=torch.float64)
    status, iters = s.solve_batch(z0.data_ptr(), Bn, nz, zo.data_ptr(), nz, lo.data_ptr(), nc, params_ptr=w.data_ptr(), ldp=nw)
    torch.cuda.synchronize()
    print(f"[64 states, sum row, per-instance (gain, weight)] status {status.tolist()}, iterations {iters.tolist()}")
    assert np.all(status == 1), (status, iters)
    zo, lam = zo.cpu().numpy(), lo.cpu().numpy()
    vlo, vhi = s.nlp.variable_bounds
    spec = _spec([row], 64, 1)
    for b in range(Bn):
        nu = _kkt_conditions(PaddedAcrobot(64, 1, PAIRS[b]), Tn, spec, zo[b], lam[b], vlo, vhi, False)
        print(f"  instance {b}: multiplier of the row {nu:.4f}")
    d = np.max(np.abs(zo[0] - zo[2]))
    print(f"  distance of instances 0 and 2: {d:.3e}")
    assert d > 1e-3, d

"""Stepwise, warm-started and shifted solves on the tile (MFMA) path -- 64-state models and the 17..63-state embedding.

include/dto.h: dto_solver_begin / iterate / run / end / stats / peek / scalar, dto_solver_begin_warm (k_wide_init_warm) and
dto_solver_shift (k_wide_shift_knots, dto_solver_shift_keep_rows) on a wide plugin, driven through the Python Solver.  Every
solution is checked as a KKT point with the ORACLE's derivatives (oracle/padded_model.py): dynamics (and pin rows) at 1e-6, the
Lagrangian stationary in every free variable at 1e-5 relative to the multipliers, bound multipliers included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TARGET = 0.5
PAIRS = [(0.8, 1.5), (1.0, 1.0), (1.3, 0.7), (1.6, 0.4)]   # per-instance (torque gain, state-cost weight)


def _solver64(T, u_max=None, parameters=None):
    import dto_amd
    from dto_amd import problems as P
    p = P.build_acrobot_padded(T=T, target=TARGET, terminal="physical", u_max=u_max, parameters=parameters)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       parameters=p["parameters"], name="acrobot_padded_par" if parameters is not None else "acrobot_padded")
    return s, p


def _guesses(s, p, B):
    import dto_amd
    Z = np.zeros((B, s._solve_nlp.num_variables))
    for b in range(B):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s.pad_batch(s._z0)
    return Z


@pytest.fixture(scope="module")
def u_free_max():
    """Largest action of the unbounded 64-state solve at T = 30: the action bounds below are set relative to it."""
    import dto_amd
    s, p = _solver64(30)
    xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
    assert dto_amd.solve(s) == 1
    return float(np.max(np.abs(np.array(dto_amd.get_trajectory(s)[1]))))


def _out(B, n):
    import torch
    return torch.full((B, max(1, n)), float("nan"), device="cuda", dtype=torch.float64)


def _shift_ref(V, k, stride, blocks, last_len, keep=None):
    """numpy restatement of dto_solver_shift on [B][n] arrays: block t <- block t + k; the blocks that enter at the end hold the
    final state (first last_len entries of the trailing short block) and repeat the last action; `keep` columns stay."""
    out = V.copy()
    for t in range(blocks):
        ts = t + k
        if ts < blocks:
            out[:, t * stride:(t + 1) * stride] = V[:, ts * stride:(ts + 1) * stride]
        else:
            out[:, t * stride:t * stride + last_len] = V[:, blocks * stride:blocks * stride + last_len]
            out[:, t * stride + last_len:(t + 1) * stride] = V[:, (blocks - 1) * stride + last_len:blocks * stride]
    if keep is not None:
        out[:, keep] = V[:, keep]
    return out


def _check_kkt64(s, T, Z, LAM, ZL, ZU, pairs=None):
    from oracle.padded_model import PaddedAcrobot, kkt_residual_blockwise
    vlo, vhi = s.nlp.variable_bounds
    free = vlo != vhi
    for b in range(Z.shape[0]):
        om = PaddedAcrobot(64, 1, pairs[b] if pairs is not None else None)
        c, r = kkt_residual_blockwise(om, T, Z[b], LAM[b])
        r = r - ZL[b] + ZU[b]
        assert np.max(np.abs(c)) <= 1e-6, (b, np.max(np.abs(c)))
        assert np.max(np.abs(r[free])) <= 1e-5 * max(1.0, np.max(np.abs(LAM[b]))), (b, np.max(np.abs(r[free])))
        assert np.all(Z[b][free] >= vlo[free]) and np.all(Z[b][free] <= vhi[free])


def test_stepwise_solve_equals_one_shot_bit_for_bit(u_free_max):
    """begin + iterate(3) + iterate(2) + run on a 64-state model with action bounds (barrier on) returns exactly what the one-shot
    dto_solve_batch returns: the same kernels, launches and host decisions, only split at outer iterations."""
    import torch
    T, B = 30, 4
    s, p = _solver64(T, u_max=1.2 * u_free_max)
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    z0 = torch.tensor(_guesses(s, p, B), device="cuda")
    zo1, mo1 = _out(B, nz), _out(B, nc)
    st1, it1 = s.solve_batch(z0.data_ptr(), B, nz, zo1.data_ptr(), nz, mo1.data_ptr(), nc)
    torch.cuda.synchronize()
    assert np.all(st1 == 1), (st1, it1)
    s.begin_batch(z0.data_ptr(), B, nz)
    assert s.hessian_mode_last() == "exact"
    s.iterate_batch(3)
    mid = s.stats_batch()
    assert np.all(mid["iterations"] == 3) and np.all(mid["status"] == 0)
    assert np.all(s.scalar_batch("iter") == 3) and np.all(s.scalar_batch("mu") > 0.0)
    s.iterate_batch(2)
    assert np.all(s.stats_batch()["iterations"] == 5) and s.repack_batch() == B
    zo2, mo2 = _out(B, nz), _out(B, nc)
    st2, it2 = s.run_batch(zo2.data_ptr(), nz, mo2.data_ptr(), nc)
    torch.cuda.synchronize()
    assert np.array_equal(st1, st2) and np.array_equal(it1, it2)
    assert np.array_equal(zo1.cpu().numpy(), zo2.cpu().numpy()) and np.array_equal(mo1.cpu().numpy(), mo2.cpu().numpy())
    stats = s.stats_batch()
    assert np.array_equal(stats["status"], st2) and np.array_equal(stats["iterations"], it2)
    assert s.repack_batch() == 0
    # the state stays after the run: end hands the same results over again
    zo3 = _out(B, nz)
    s.end_batch(zo3.data_ptr(), nz)
    torch.cuda.synchronize()
    assert np.array_equal(zo3.cpu().numpy(), zo2.cpu().numpy())
    assert np.array_equal(s.peek_batch("z"), zo2.cpu().numpy())


def test_lane_path_only_entry_points_refuse_on_the_tile_path():
    """Entry points that only have a meaning on the lane-per-instance path say so on a tile-path model instead of failing on
    missing KKT kernels."""
    from dto_amd import capi
    s, p = _solver64(3)
    with pytest.raises(capi.DtoError, match="dto_solver_begin has not been called"):
        s.iterate_batch(1)
    import torch
    nz = s._solve_nlp.num_variables
    z0 = torch.tensor(_guesses(s, p, 2), device="cuda")
    s.begin_batch(z0.data_ptr(), 2, nz)
    for call in (lambda: s.launch_op("eval"), lambda: s.footprint(), lambda: s.set_partitions(1), lambda: s.set_engine("soa"),
                 lambda: s.trace(True), lambda: s.peek_batch("slack"), lambda: s.scalar_batch("penalty")):
        with pytest.raises(capi.DtoError) as e:
            call()
        assert e.value.code == 4   # DTO_ERR_UNSUPPORTED
    s.release_state()
    with pytest.raises(capi.DtoError):
        s.stats_batch()


def test_warm_resolve_after_a_parameter_change_64_states(u_free_max):
    """Per-instance parameters change a little between two solves: the warm re-solve (dto_solver_begin_warm, multipliers, bound
    multipliers and mu kept) and a cold solve from the previous solution reach the same KKT points, the warm one in fewer
    iterations."""
    import torch
    from dto_amd import capi
    T, B = 30, 4
    s, p = _solver64(T, u_max=2.0 * u_free_max, parameters=(1.0, 1.0))
    nz, nc, nw = s._solve_nlp.num_variables, s._solve_nlp.num_constraint, s._solve_nlp.num_parameters
    z0 = torch.tensor(_guesses(s, p, B), device="cuda")
    W1 = np.array([np.tile(pr, T) for pr in PAIRS])
    pairs2 = [(g * 1.02, w * 0.98) for g, w in PAIRS]
    W2 = np.array([np.tile(pr, T) for pr in pairs2])
    w1, w2 = torch.tensor(W1, device="cuda"), torch.tensor(W2, device="cuda")
    zo, mo = _out(B, nz), _out(B, nc)
    st0, it0 = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc, params_ptr=w1.data_ptr(), ldp=nw)
    torch.cuda.synchronize()
    assert np.all(st0 == 1), (st0, it0)
    _check_kkt64(s, T, zo.cpu().numpy(), mo.cpu().numpy(), s.peek_batch("z_lower"), s.peek_batch("z_upper"), PAIRS)
    mu_end = s.stats_batch()["mu"]
    assert np.all(mu_end > 0.0)
    zprev = zo.clone()
    # warm
    s.begin_warm_batch(B, params_ptr=w2.data_ptr(), ldp=nw)
    assert np.array_equal(s.scalar_batch("mu"), mu_end)
    assert np.all(s.scalar_batch("iter") == 0) and np.all(s.scalar_batch("status") == 0)
    zw, mw = _out(B, nz), _out(B, nc)
    stw, itw = s.run_batch(zw.data_ptr(), nz, mw.data_ptr(), nc)
    torch.cuda.synchronize()
    assert np.all(stw == 1), (stw, itw)
    zw_, mw_ = zw.cpu().numpy(), mw.cpu().numpy()
    _check_kkt64(s, T, zw_, mw_, s.peek_batch("z_lower"), s.peek_batch("z_upper"), pairs2)
    # cold from the previous solution
    zc, mc = _out(B, nz), _out(B, nc)
    stc, itc = s.solve_batch(zprev.data_ptr(), B, nz, zc.data_ptr(), nz, mc.data_ptr(), nc, params_ptr=w2.data_ptr(), ldp=nw)
    torch.cuda.synchronize()
    assert np.all(stc == 1), (stc, itc)
    zc_ = zc.cpu().numpy()
    _check_kkt64(s, T, zc_, mc.cpu().numpy(), s.peek_batch("z_lower"), s.peek_batch("z_upper"), pairs2)
    assert np.max(np.abs(zw_ - zc_)) <= 1e-5
    assert np.max(np.abs(zw_ - zprev.cpu().numpy())) > 1e-4          # the parameters did move the solution
    assert int(itw.sum()) < int(itc.sum()), (itw, itc)
    with pytest.raises(capi.DtoError, match="same batch size"):
        s.begin_warm_batch(B + 1, params_ptr=w2.data_ptr(), ldp=nw)


def test_shift_on_a_native_64_state_model(u_free_max):
    """dto_solver_shift on the tile path's instance-major arrays: z, the dynamics multipliers, z_L and z_U move by two knots exactly
    as the numpy restatement moves what dto_solver_peek showed before; a warm begin + run from there converges to a KKT point."""
    import torch
    from dto_amd import capi
    T, B, k = 30, 3, 2
    s, p = _solver64(T, u_max=0.8 * u_free_max)
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    z0 = torch.tensor(_guesses(s, p, B), device="cuda")
    zo, mo = _out(B, nz), _out(B, nc)
    st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc)
    torch.cuda.synchronize()
    assert np.all(st == 1), (st, it)
    pre = {nm: s.peek_batch(nm) for nm in ("z", "multipliers", "z_lower", "z_upper")}
    assert np.array_equal(pre["z"], zo.cpu().numpy()) and np.max(pre["z_lower"]) > 0.0 and np.max(pre["z_upper"]) > 0.0
    s.shift_batch(k)
    assert np.array_equal(s.peek_batch("z"), _shift_ref(pre["z"], k, 65, T - 1, 64))
    assert np.array_equal(s.peek_batch("multipliers"), _shift_ref(pre["multipliers"], k, 64, T - 1, 0))
    assert np.array_equal(s.peek_batch("z_lower"), _shift_ref(pre["z_lower"], k, 65, T - 1, 64))
    assert np.array_equal(s.peek_batch("z_upper"), _shift_ref(pre["z_upper"], k, 65, T - 1, 64))
    s.begin_warm_batch(B)
    zw, mw = _out(B, nz), _out(B, nc)
    stw, itw = s.run_batch(zw.data_ptr(), nz, mw.data_ptr(), nc)
    torch.cuda.synchronize()
    assert np.all(stw == 1), (stw, itw)
    _check_kkt64(s, T, zw.cpu().numpy(), mw.cpu().numpy(), s.peek_batch("z_lower"), s.peek_batch("z_upper"))
    for bad in (T - 1, T):
        with pytest.raises(capi.DtoError):
            s.shift_batch(bad)


def _plant(n):
    """The model's midpoint step y = x + h f((x + y) / 2, u), solved by fixed-point iteration."""
    from dto_amd import problems as P
    res = P.acrobot_padded_midpoint(n)

    def step(x, u):
        y = np.array(x, dtype=float)
        for _ in range(200):
            y_new = np.array(y - res(y, x, np.array([u]), None), dtype=float)
            if np.max(np.abs(y_new - y)) < 1e-15:
                return y_new
            y = y_new
        return y
    return step


def test_receding_horizon_on_the_24_state_embedding():
    """MPC on problems.build_mpc_acrobot_padded (24 states; the first-knot pin rows x - w ride auxiliary states of the 64-state
    embedding): apply the first action to the plant (plus a 1e-3 disturbance), shift by one knot, warm begin with the measured
    state as the pin parameters, run -- eight steps.  Right after each shift the iterate is the previous solution moved by one knot
    (hold-last at the end) and the multipliers of the pin rows have stayed with their knot."""
    import torch
    import dto_amd
    from dto_amd import problems as P
    from oracle.padded_model import PaddedAcrobot, kkt_residual_blockwise
    T, B, n, steps = 30, 4, 24, 8
    p = P.build_mpc_acrobot_padded(T=T, n=n, target=TARGET)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       parameters=p["parameters"], name="acrobot24mpc")
    assert s.solve_unsupported is None
    nz, nc, nw = s._solve_nlp.num_variables, s._solve_nlp.num_constraint, s._solve_nlp.num_parameters
    assert nw == s.nlp.num_parameters == T * n
    stage = np.arange(n, 2 * n)                       # the pin rows: rows n .. 2n-1 of the first stage of the embedding
    om = PaddedAcrobot(n)
    vlo, vhi = s.nlp.variable_bounds
    free = vlo != vhi
    nd = (T - 1) * n
    rng = np.random.default_rng(5)
    X = 0.05 * rng.standard_normal((B, n))
    Z = np.zeros((B, nz))
    for b in range(B):
        xs, us = P.build_mpc_acrobot_padded(T=T, n=n, x1=X[b], target=TARGET)["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, us)
        Z[b] = s.pad_batch(s._z0)

    def check(zs, ms, X):
        zr, lr = s.unpad_batch(zs), s.unpad_batch(ms, multipliers=True)
        for b in range(B):
            c, r = kkt_residual_blockwise(om, T, zr[b], lr[b][:nd])
            r[:n] += lr[b][nd:nd + n]
            assert max(np.max(np.abs(c)), np.max(np.abs(zr[b][:n] - X[b]))) <= 1e-6
            assert np.max(np.abs(r[free])) <= 1e-5 * max(1.0, np.max(np.abs(lr[b]))), (b, np.max(np.abs(r[free])))
        return zr

    z0, w = torch.tensor(Z, device="cuda"), torch.tensor(np.tile(X, (1, T)), device="cuda")
    zo, mo = _out(B, nz), _out(B, nc)
    st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc, params_ptr=w.data_ptr(), ldp=nw)
    torch.cuda.synchronize()
    assert np.all(st == 1), (st, it)
    cold = float(np.mean(it))
    zs, ms = zo.cpu().numpy(), mo.cpu().numpy()
    zr = check(zs, ms, X)
    plant = _plant(n)
    warm = []
    for step in range(steps):
        X = np.array([plant(X[b], zr[b][n]) for b in range(B)]) + 1e-3 * rng.standard_normal((B, n))
        s.shift_batch(1)
        assert np.array_equal(s.peek_batch("z"), _shift_ref(zs, 1, 65, T - 1, 64))
        m_sh = s.peek_batch("multipliers")
        assert np.array_equal(m_sh[:, stage], ms[:, stage])
        assert np.array_equal(m_sh, _shift_ref(ms, 1, 64, T - 1, 0, keep=stage))
        w = torch.tensor(np.tile(X, (1, T)), device="cuda")
        s.begin_warm_batch(B, params_ptr=w.data_ptr(), ldp=nw)
        zo, mo = _out(B, nz), _out(B, nc)
        st, it = s.run_batch(zo.data_ptr(), nz, mo.data_ptr(), nc)
        torch.cuda.synchronize()
        assert np.all(st == 1), (step, st, it)
        zs, ms = zo.cpu().numpy(), mo.cpu().numpy()
        zr = check(zs, ms, X)
        warm.append(it)
    assert np.mean(warm) < 0.6 * cold, (np.array(warm), cold)

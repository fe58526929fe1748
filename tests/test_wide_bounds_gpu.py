"""Per-instance variable bounds on the tile (MFMA) path: Solver.set_bounds_batch (include/dto.h: dto_solver_set_bounds), read by
k_wide_step / k_wide_bwd / k_wide_merit and the bound kernels of the host loop through a per-instance base pointer.

Bounds equal to the shared ones reproduce the shared solve bit for bit; a native 64-state model takes a measured initial state per
instance (pinned by lower == upper) and per-instance action limits, one-shot and in a receding-horizon loop; a cold begin puts
fixed variables on their values even without a barrier.  Every solution is checked as a KKT point with the ORACLE's derivatives
(oracle/padded_model.py) and each instance's own bounds."""
import numpy as np
import pytest

from test_wide_mpc_gpu import _guesses, _out, _plant, _solver64, u_free_max  # noqa: F401  (u_free_max: module fixture)

pytestmark = pytest.mark.gpu

T = 30
N = 64


def _tile_bounds(s, B):
    lo, hi = s.nlp.variable_bounds
    return np.tile(lo, (B, 1)), np.tile(hi, (B, 1))


def _measured(s, X, lim=None):
    """The problem's bounds with instance b's first-knot state X[b] and (optionally) its action limit lim[b]."""
    L, U = _tile_bounds(s, X.shape[0])
    L[:, :N], U[:, :N] = X, X
    if lim is not None:
        lo, _ = s.nlp.variable_bounds
        act = np.array([t * (N + 1) + N for t in range(T - 1)])
        assert np.all(np.isfinite(lo[act]))
        L[:, act], U[:, act] = -lim[:, None], lim[:, None]
    return L, U


def _peek_bounds(s, B, nz):
    try:
        return s.peek_batch("z_lower"), s.peek_batch("z_upper")
    except Exception:
        return np.zeros((B, nz)), np.zeros((B, nz))   # no finite bounds besides fixed ones: no bound multipliers


def _check_kkt(Z, LAM, ZL, ZU, LO, HI):
    from oracle.padded_model import PaddedAcrobot, kkt_residual_blockwise
    om = PaddedAcrobot(N, 1, None)
    for b in range(Z.shape[0]):
        c, r = kkt_residual_blockwise(om, T, Z[b], LAM[b])
        r = r - ZL[b] + ZU[b]
        free = LO[b] != HI[b]
        assert np.max(np.abs(c)) <= 1e-6, (b, np.max(np.abs(c)))
        assert np.max(np.abs(r[free])) <= 1e-5 * max(1.0, np.max(np.abs(LAM[b]))), (b, np.max(np.abs(r[free])))
        assert np.array_equal(Z[b][~free], LO[b][~free]), b
        assert np.all(Z[b][free] >= LO[b][free]) and np.all(Z[b][free] <= HI[b][free]), b


def _solve(s, z0, B):
    import torch
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    zo, mo = _out(B, nz), _out(B, nc)
    st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc)
    torch.cuda.synchronize()
    return zo.cpu().numpy(), mo.cpu().numpy()[:, :nc], st, it


def _identity(s, p, B, to_device):
    import torch
    z0 = torch.tensor(_guesses(s, p, B), device="cuda")
    ref = _solve(s, z0, B)
    assert np.all(ref[2] == 1), ref[2:]
    L, U = _tile_bounds(s, B)
    s.set_bounds_batch(*((torch.tensor(L, device="cuda"), torch.tensor(U, device="cuda")) if to_device else (L, U)))
    got = _solve(s, z0, B)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    s.set_bounds_batch(None, None)
    again = _solve(s, z0, B)
    for a, b in zip(ref, again):
        assert np.array_equal(a, b)
    return ref


def test_identity_native_64_with_action_bounds(u_free_max):
    s, p = _solver64(T, u_max=1.2 * u_free_max)
    z, m, st, it = _identity(s, p, 4, to_device=True)
    L, U = _tile_bounds(s, 4)
    _check_kkt(z, m, s.peek_batch("z_lower"), s.peek_batch("z_upper"), L, U)


def test_identity_native_64_free():
    s, p = _solver64(T)
    lo, hi = s.nlp.variable_bounds
    assert np.all(np.isinf(lo[lo != hi]) & np.isinf(hi[lo != hi]))      # no barrier: fixed variables only
    _identity(s, p, 3, to_device=False)


def test_identity_24_state_embedding():
    import dto_amd
    from dto_amd import problems as P
    p = P.build_acrobot_padded(T=T, n=24, target=0.3, terminal="physical")
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot24")
    assert s._pad is not None
    _identity(s, p, 3, to_device=False)


def _single(X, lim):
    """A 64-state Solver whose SHARED bounds are one instance's: first knot X, action limit lim."""
    import dto_amd
    from dto_amd import problems as P
    p = P.build_acrobot_padded(T=T, target=0.5, terminal="physical", u_max=lim)
    p["bounds"][0] = P.Bound(N, 1, state_lower=X, state_upper=X, action_lower=[-lim], action_upper=[lim])
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
    return s


def test_measured_initial_states_on_a_native_64_state_model(u_free_max):
    import torch
    B = 4
    s, p = _solver64(T, u_max=2.0 * u_free_max)
    nz = s._solve_nlp.num_variables
    rng = np.random.default_rng(11)
    X = np.zeros((B, N))
    X[:, :4] = 0.1 * rng.standard_normal((B, 4))
    X[:, 4:] = 0.01 * rng.standard_normal((B, N - 4))
    lim = np.array([0.8, 0.7, 0.9, 1.5]) * u_free_max
    L, U = _measured(s, X, lim)
    Zg = _guesses(s, p, B)
    assert np.all(np.max(np.abs(Zg[:, :N] - X), axis=1) > 1e-3)           # the guesses miss the measured states
    s.set_bounds_batch(torch.tensor(L, device="cuda"), torch.tensor(U, device="cuda"))
    z, m, st, it = _solve(s, torch.tensor(Zg, device="cuda"), B)
    assert np.all(st == 1), (st, it)
    assert np.array_equal(z[:, :N], X)
    act = np.array([t * (N + 1) + N for t in range(T - 1)])
    umax = np.max(np.abs(z[:, act]), axis=1)
    assert np.all(umax <= lim), (umax, lim)
    assert np.any(umax >= lim * (1.0 - 1e-3)), (umax, lim)                 # a limit is active (to the barrier's accuracy)
    _check_kkt(z, m, s.peek_batch("z_lower"), s.peek_batch("z_upper"), L, U)
    # one workgroup owns one instance: each one is the B = 1 solve of a problem whose shared bounds are that instance's
    diffs = []
    for b in range(B):
        s1 = _single(X[b], float(lim[b]))
        z1, m1, st1, it1 = _solve(s1, torch.tensor(Zg[b:b + 1], device="cuda"), 1)
        assert st1[0] == 1 and it1[0] == it[b], (b, it1, it)
        diffs.append(float(np.max(np.abs(z1[0] - z[b]))))
        s1.close()
    print(f"[per-instance bounds] iterations {it.tolist()}, max |x_B=4 - x_B=1| per instance {diffs}")
    assert max(diffs) <= 1e-10, diffs


def test_receding_horizon_with_measured_states_on_a_native_64_state_model(u_free_max):
    """MPC on the native 64-state model: the measured state enters as the per-instance bounds of the first knot.  Each step:
    plant (midpoint step + 1e-3 disturbance), shift_batch(1), set_bounds_batch, begin_warm_batch, run_batch."""
    import torch
    B, steps = 4, 6
    s, p = _solver64(T, u_max=2.0 * u_free_max)
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    rng = np.random.default_rng(5)
    X = np.zeros((B, N))
    X[:, :4] = 0.05 * rng.standard_normal((B, 4))
    X[:, 4:] = 0.01 * rng.standard_normal((B, N - 4))
    L, U = _measured(s, X)
    s.set_bounds_batch(L, U)
    z, m, st, it = _solve(s, torch.tensor(_guesses(s, p, B), device="cuda"), B)
    assert np.all(st == 1), (st, it)
    _check_kkt(z, m, s.peek_batch("z_lower"), s.peek_batch("z_upper"), L, U)
    cold = float(np.mean(it))
    plant = _plant(N)
    warm = []
    for step in range(steps):
        X = np.array([plant(X[b], z[b][N]) for b in range(B)]) + 1e-3 * rng.standard_normal((B, N))
        s.shift_batch(1)
        L, U = _measured(s, X)
        s.set_bounds_batch(L, U)
        s.begin_warm_batch(B)
        zo, mo = _out(B, nz), _out(B, nc)
        st, it = s.run_batch(zo.data_ptr(), nz, mo.data_ptr(), nc)
        torch.cuda.synchronize()
        assert np.all(st == 1), (step, st, it)
        z, m = zo.cpu().numpy(), mo.cpu().numpy()
        assert np.array_equal(z[:, :N], X)
        _check_kkt(z, m, s.peek_batch("z_lower"), s.peek_batch("z_upper"), L, U)
        warm.append(it)
    print(f"[per-instance bounds MPC] cold {cold:.1f} iterations, warm {np.array(warm).tolist()}")
    assert np.mean(warm) < 0.6 * cold, (np.array(warm), cold)


def test_cold_begin_pins_fixed_variables_without_a_barrier():
    """No finite bounds besides the fixed variables (no barrier), guesses that miss the pins: the cold begin puts the fixed
    variables on their values, with shared and with per-instance bounds."""
    import torch
    B = 3
    s, p = _solver64(T)
    nz = s._solve_nlp.num_variables
    Zg = _guesses(s, p, B)
    Zbad = Zg.copy()
    Zbad[:, :N] += 0.05
    z, m, st, it = _solve(s, torch.tensor(Zbad, device="cuda"), B)
    assert np.all(st == 1), (st, it)
    L, U = _tile_bounds(s, B)
    _check_kkt(z, m, *_peek_bounds(s, B, nz), L, U)
    rng = np.random.default_rng(3)
    X = 0.02 * rng.standard_normal((B, N))
    L, U = _measured(s, X)
    s.set_bounds_batch(L, U)
    z, m, st, it = _solve(s, torch.tensor(Zg, device="cuda"), B)
    assert np.all(st == 1), (st, it)
    assert np.array_equal(z[:, :N], X)
    _check_kkt(z, m, *_peek_bounds(s, B, nz), L, U)


def test_errors(u_free_max):
    import torch
    from dto_amd import capi
    B = 2
    s, p = _solver64(T, u_max=2.0 * u_free_max)
    nz = s._solve_nlp.num_variables
    z0 = torch.tensor(_guesses(s, p, B), device="cuda")
    ref = _solve(s, z0, B)
    L, U = _tile_bounds(s, B)
    free = np.flatnonzero(np.isinf(L[0]))
    Lb = L.copy()
    Lb[1, free[7]] = -3.0                                  # finite where the problem's lower bound is infinite
    with pytest.raises(capi.DtoError) as e:                # device input: the device check
        s.set_bounds_batch(torch.tensor(Lb, device="cuda"), torch.tensor(U, device="cuda"))
    assert e.value.code == 1 and f"instance 1, variable {free[7]}" in str(e.value), str(e.value)
    got = _solve(s, z0, B)                                 # the shared bounds are still in force
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    # a valid setting survives a rejected one
    s.set_bounds_batch(torch.tensor(L, device="cuda"), torch.tensor(U, device="cuda"))
    Ub = U.copy()
    Ub[0, 0] = U[0, 0] + 1.0                               # a fixed variable no longer fixed
    with pytest.raises(capi.DtoError) as e:
        s.set_bounds_batch(torch.tensor(L, device="cuda"), torch.tensor(Ub, device="cuda"))
    assert e.value.code == 1 and "instance 0, variable 0" in str(e.value), str(e.value)
    got = _solve(s, z0, B)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    # a begin with another batch size
    z3 = torch.tensor(_guesses(s, p, 3), device="cuda")
    with pytest.raises(capi.DtoError) as e:
        s.begin_batch(z3.data_ptr(), 3, nz)
    assert e.value.code == 1
    s.set_bounds_batch(None, None)
    s.begin_batch(z3.data_ptr(), 3, nz)
    # the raw C call on a lane-path plugin
    from conftest import product_solver
    sl, _ = product_solver("pendulum", 6)
    n = sl._solve_nlp
    lo, hi = n.variable_bounds
    dl, dh = torch.tensor(np.tile(lo, (2, 1)), device="cuda"), torch.tensor(np.tile(hi, (2, 1)), device="cuda")
    rc = n._lib.dto_solver_set_bounds(n._h, 2, dl.data_ptr(), n.num_variables, dh.data_ptr(), n.num_variables, None)
    assert rc == 4   # DTO_ERR_UNSUPPORTED

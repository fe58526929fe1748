"""The linear solver alone on the tile path: dto_kkt_assemble / dto_kkt_factor / dto_kkt_solve on the 64-state models.

One factorisation (k_wide_step in its linear-solver mode: sigma_x / sigma_c on the diagonals, the terminal factor stored, the
negative pivots counted per instance), then any number of substitution-only solves (k_wide_fsub + k_wide_bwd) against the
stored records.  Reference everywhere: numpy's dense solve of the ORACLE's matrix (oracle/padded_model.py: dense_kkt) with
diag(sigma_x) / -diag(sigma_c) added.  Tolerance: the project's 1e-8 of max |solution| (tests/test_wide_gpu.py);
1e-6 for the unpivoted solve of an indefinite matrix (tests/test_entry_points_gpu.py).
"""
import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu


def _solver(m, T):
    if m == 1:
        return product_solver("acrobot_padded", T)[0]
    import dto_amd
    from dto_amd import problems as P
    p = P.build_acrobot_padded(T=T, m=m)
    return dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name=f"acrobot_padded_m{m}")


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _assemble_factor(s, Z, MU, dw, dc, SX=None, SC=None, W=None):
    B, nz = Z.shape
    nc = MU.shape[1]
    keep = [_dev(Z), _dev(MU)]
    kw = {}
    if SX is not None:
        keep += [_dev(SX), _dev(SC)]
        kw.update(sigma_x_ptr=keep[2].data_ptr(), ldsx=nz, sigma_c_ptr=keep[3].data_ptr(), ldsc=nc)
    if W is not None:
        keep.append(_dev(W))
        kw.update(params_ptr=keep[-1].data_ptr(), ldp=W.shape[1])
    s.kkt_assemble(keep[0].data_ptr(), B, nz, keep[1].data_ptr(), nc, dw, dc, **kw)
    return s.kkt_factor()


def _solve(s, RX, RC):
    import torch
    B, nz = RX.shape
    nc = RC.shape[1]
    dRX, dRC = _dev(RX), _dev(RC)
    oX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
    torch.cuda.synchronize()
    return oX.cpu().numpy(), oC.cpu().numpy()


def _dense(om, T, z, mu, dw, dc, sx=None, sc=None):
    from oracle.padded_model import dense_kkt
    K, rhs = dense_kkt(om, T, z, mu, dw, dc)
    nz = len(z)
    if sx is not None:
        K = K + np.diag(np.concatenate([sx, -sc]))
    return K, rhs, nz


def _check_solves(s, Ks, rng, nz, nc, tol, only=None):
    B = len(Ks)
    for _ in range(3):                                         # several right-hand sides on one factorisation
        RX, RC = rng.standard_normal((B, nz)), rng.standard_normal((B, nc))
        oX, oC = _solve(s, RX, RC)
        for b in range(B):
            if only is not None and not only[b]:
                continue
            sol = np.linalg.solve(Ks[b], np.concatenate([RX[b], RC[b]]))
            scale = np.max(np.abs(sol))
            ex, ec = np.max(np.abs(oX[b] - sol[:nz])), np.max(np.abs(oC[b] - sol[nz:]))
            print(f"  instance {b}: error {ex:.2e} / {ec:.2e}, solution scale {scale:.2e}")
            assert ex <= tol * scale and ec <= tol * scale, (b, ex, ec, scale)


@pytest.mark.parametrize("m,T,B,dw,sig", [(1, 2, 2, 2.0, True), (1, 5, 3, 2.0, True), (1, 9, 2, 30.0, True), (3, 5, 3, 2.0, True),
                                          (4, 3, 2, 30.0, True), (1, 5, 3, 2.0, False)])
def test_wide_linear_solver_matches_dense_solves(m, T, B, dw, sig):
    """The points of tests/test_wide_gpu.py's step tests (quasi-definite there; non-negative sigmas keep them so), random
    sigma_x in [0, 3) with every third entry 0 and sigma_c in [0, 0.5) (sig=False: both NULL); three right-hand sides per
    factor; then a second assemble / factor / solve with another delta_w and other multipliers (a stale record would show)."""
    from oracle.padded_model import PaddedAcrobot
    s = _solver(m, T)
    om = PaddedAcrobot(64, m)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    assert (nz, nc) == ((T - 1) * (64 + m) + 64, (T - 1) * 64) and nc == s.nlp.num_constraint
    rng = np.random.default_rng(5 + T if m == 1 else 50 + m)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    dc = 1e-5
    for dw_k, MU_k in ((dw, MU), (dw + 7.0, rng.random((B, nc)))):
        SX = SC = None
        if sig:
            SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
            SX[:, ::3] = 0.0                                   # some variables without a barrier term
        ok, neg = _assemble_factor(s, Z, MU_k, dw_k, dc, SX, SC)
        Ks = []
        for b in range(B):
            K, _, _ = _dense(om, T, Z[b], MU_k[b], dw_k, dc, None if SX is None else SX[b], None if SC is None else SC[b])
            eig = np.linalg.eigvalsh(K)
            assert (int(np.sum(eig > 0)), int(np.sum(eig < 0))) == (nz, nc), "test point must be quasi-definite; raise dw"
            Ks.append(K)
        assert np.all(neg == nc) and np.all(ok == 1), (neg, ok, nc)
        _check_solves(s, Ks, rng, nz, nc, 1e-8)


def _padded(a, ld):
    """[B][ld] with NaN in every padding entry"""
    out = np.full((a.shape[0], ld), np.nan)
    out[:, :a.shape[1]] = a
    return out


def test_wide_linear_solver_padded_leading_dimensions():
    """dto_kkt_assemble copies its five inputs row by row with the caller's leading dimensions, dto_kkt_solve reads and writes with
    four more: all nine above the row lengths and all different, NaN in every padding entry (a read one would reach the factor or
    the solution), NaN-filled outputs whose padding must stay NaN.  Bit-identical to the tight call on the same data, and within
    1e-8 of the dense solve."""
    import torch
    import dto_amd
    from dto_amd import problems as P
    from oracle.padded_model import PaddedAcrobot
    T, B, dw, dc = 4, 2, 2.0, 1e-5
    p = P.build_acrobot_padded(T=T, parameters=(1.3, 0.7))
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       parameters=p["parameters"], name="acrobot_padded_par")
    nz, nc, nw = s.nlp.num_variables, s.nlp.num_constraint, s.nlp.num_parameters
    pairs = [(0.8, 1.5), (1.6, 0.4)]
    W = np.array([np.tile(pr, T) for pr in pairs])
    assert W.shape == (B, nw)
    rng = np.random.default_rng(91)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
    SX[:, ::3] = 0.0
    RX, RC = rng.standard_normal((B, nz)), rng.standard_normal((B, nc))
    ok, neg = _assemble_factor(s, Z, MU, dw, dc, SX, SC, W)
    assert np.all(neg == nc) and np.all(ok == 1)
    tight = _solve(s, RX, RC)
    # the same system through padded arrays
    ldx, ldmu, ldsx, ldsc, ldp = nz + 3, nc + 1, nz + 8, nc + 5, nw + 1
    keep = [_dev(_padded(a, ld)) for a, ld in ((Z, ldx), (MU, ldmu), (SX, ldsx), (SC, ldsc), (W, ldp))]
    s.kkt_assemble(keep[0].data_ptr(), B, ldx, keep[1].data_ptr(), ldmu, dw, dc, sigma_x_ptr=keep[2].data_ptr(), ldsx=ldsx,
                   sigma_c_ptr=keep[3].data_ptr(), ldsc=ldsc, params_ptr=keep[4].data_ptr(), ldp=ldp)
    ok, neg = s.kkt_factor()
    assert np.all(neg == nc) and np.all(ok == 1)
    ldrx, ldrc, ldox, ldoc = nz + 5, nc + 3, nz + 7, nc + 2
    dRX, dRC = _dev(_padded(RX, ldrx)), _dev(_padded(RC, ldrc))
    oX = torch.full((B, ldox), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B, ldoc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_solve(dRX.data_ptr(), ldrx, dRC.data_ptr(), ldrc, oX.data_ptr(), ldox, oC.data_ptr(), ldoc)
    torch.cuda.synchronize()
    oX, oC = oX.cpu().numpy(), oC.cpu().numpy()
    assert np.all(np.isnan(oX[:, nz:])) and np.all(np.isnan(oC[:, nc:])), "the padding of the outputs must stay untouched"
    assert np.all(np.isfinite(tight[0])) and np.all(np.isfinite(tight[1]))
    assert np.array_equal(oX[:, :nz], tight[0]) and np.array_equal(oC[:, :nc], tight[1])
    for b in range(B):
        K = _dense(PaddedAcrobot(64, 1, pairs[b]), T, Z[b], MU[b], dw, dc, SX[b], SC[b])[0]
        eig = np.linalg.eigvalsh(K)
        assert (int(np.sum(eig > 0)), int(np.sum(eig < 0))) == (nz, nc), "test point must be quasi-definite; raise dw"
        sol = np.linalg.solve(K, np.concatenate([RX[b], RC[b]]))
        scale = np.max(np.abs(sol))
        ex, ec = np.max(np.abs(oX[b, :nz] - sol[:nz])), np.max(np.abs(oC[b, :nc] - sol[nz:]))
        print(f"  instance {b}: error {ex:.2e} / {ec:.2e}, solution scale {scale:.2e}")
        assert ex <= 1e-8 * scale and ec <= 1e-8 * scale, (b, ex, ec, scale)


def test_wide_linear_solver_agrees_with_the_newton_step():
    """sigmas NULL and the right-hand side of the Newton system (-[grad L; c], what dense_kkt returns): dto_kkt_solve must give
    the step of dto_kkt_step_batch at the same point, 1e-8 of the solution scale."""
    import torch
    from oracle.padded_model import PaddedAcrobot, dense_kkt
    T, B, dw, dc = 4, 2, 2.0, 1e-5
    s = _solver(1, T)
    om = PaddedAcrobot(64)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(404)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    R = np.array([dense_kkt(om, T, Z[b], MU[b], dw, dc)[1] for b in range(B)])
    ok, neg = _assemble_factor(s, Z, MU, dw, dc)
    assert np.all(ok == 1) and np.all(neg == nc)
    oX, oC = _solve(s, R[:, :nz], R[:, nz:])
    dZ, dMU = _dev(Z), _dev(MU)
    dx = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    dl = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    assert s.kkt_step_batch(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc, dx.data_ptr(), nz, dl.data_ptr(), nc)
    torch.cuda.synchronize()
    dx, dl = dx.cpu().numpy(), dl.cpu().numpy()
    for b in range(B):
        scale = max(np.max(np.abs(dx[b])), np.max(np.abs(dl[b])))
        ex, ec = np.max(np.abs(oX[b] - dx[b])), np.max(np.abs(oC[b] - dl[b]))
        print(f"  instance {b}: solve - step {ex:.2e} / {ec:.2e}, scale {scale:.2e}")
        assert ex <= 1e-8 * scale and ec <= 1e-8 * scale, (b, ex, ec, scale)


INDEFINITE_SEED = 99   # chosen with the oracle alone: all four matrices have min |eig| > 1e-6 (see the assertion on `usable`)


def test_wide_linear_solver_indefinite_matrix():
    """delta_w = 0 with multipliers of order 10 (the point family of test_wide_inertia_flag_matches_eigenvalues): the single attempt is
    swept to the end, the pivot count is the matrix's inertia (Sylvester), inertia_ok says whether it is (n, m, 0), and the solve
    is K^-1 rhs although the inertia is wrong -- 1e-6 of the solution scale, the bar of the lane path's test for unpivoted
    indefinite solves."""
    from oracle.padded_model import PaddedAcrobot
    T, B, dc = 4, 4, 1e-5
    s = _solver(1, T)
    om = PaddedAcrobot(64)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(INDEFINITE_SEED)
    Z = rng.random((B, nz))
    MU = 40.0 * (rng.random((B, nc)) - 0.5)
    Ks, want_neg, usable = [], [], []
    for b in range(B):
        K, _, _ = _dense(om, T, Z[b], MU[b], 0.0, dc)
        eig = np.linalg.eigvalsh(K)
        Ks.append(K)
        want_neg.append(int(np.sum(eig < 0)))
        usable.append(bool(np.min(np.abs(eig)) > 1e-6))
    assert sum(usable) >= 3, ("vacuous: pick another seed", usable)
    ok, neg = _assemble_factor(s, Z, MU, 0.0, dc)
    print(f"  negative pivots {neg.tolist()}, eigenvalues {want_neg}, constraints {nc}, inertia_ok {ok.tolist()}")
    for b in range(B):
        if usable[b]:
            assert neg[b] == want_neg[b], (b, neg[b], want_neg[b])
            assert bool(ok[b]) == (want_neg[b] == nc), (b, ok[b], want_neg[b], nc)
    _check_solves(s, Ks, rng, nz, nc, 1e-6, only=usable)


def test_wide_linear_solver_per_instance_parameters():
    """dto_batch.params on dto_kkt_assemble: every instance factorises the matrix of its own (gain, weight) pair."""
    import dto_amd
    from dto_amd import problems as P
    from oracle.padded_model import PaddedAcrobot
    T, B, dw, dc = 3, 2, 2.0, 1e-5
    p = P.build_acrobot_padded(T=T, parameters=(1.3, 0.7))
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       parameters=p["parameters"], name="acrobot_padded_par")
    nz, nc, nw = s.nlp.num_variables, s.nlp.num_constraint, s.nlp.num_parameters
    assert nw == 2 * T
    pairs = [(0.8, 1.5), (1.6, 0.4)]
    W = np.array([np.tile(pr, T) for pr in pairs])
    rng = np.random.default_rng(78)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
    SX[:, ::3] = 0.0
    ok, neg = _assemble_factor(s, Z, MU, dw, dc, SX, SC, W)
    Ks = [_dense(PaddedAcrobot(64, 1, pairs[b]), T, Z[b], MU[b], dw, dc, SX[b], SC[b])[0] for b in range(B)]
    for K in Ks:
        eig = np.linalg.eigvalsh(K)
        assert (int(np.sum(eig > 0)), int(np.sum(eig < 0))) == (nz, nc)
    assert np.max(np.abs(Ks[0] - _dense(PaddedAcrobot(64, 1, pairs[1]), T, Z[0], MU[0], dw, dc, SX[0], SC[0])[0])) > 1e-3   # the parameters matter
    assert np.all(neg == nc) and np.all(ok == 1)
    _check_solves(s, Ks, rng, nz, nc, 1e-8)


def test_wide_linear_solver_misuse_and_shared_factor_storage():
    """The state machine (factor needs assemble, solve needs factor), the factor storage shared with dto_kkt_step_batch (a step
    in between invalidates the stored factor: the next solve is refused instead of reading a foreign record), and the step itself
    untouched by a complete assemble / factor / solve sequence in the same process (bit-identical output)."""
    import torch
    import dto_amd
    from dto_amd import capi, problems as P
    T, B, dw, dc = 3, 2, 2.0, 1e-5
    p = P.build_acrobot_padded(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(12)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    RX, RC = rng.standard_normal((B, nz)), rng.standard_normal((B, nc))
    dZ, dMU = _dev(Z), _dev(MU)
    s._B = B
    with pytest.raises(capi.DtoError, match="dto_kkt_assemble has not been called"):
        s.kkt_factor()
    with pytest.raises(capi.DtoError, match="dto_kkt_assemble has not been called"):
        _solve(s, RX, RC)

    def step():
        dx = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
        dl = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
        assert s.kkt_step_batch(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc, dx.data_ptr(), nz, dl.data_ptr(), nc)
        torch.cuda.synchronize()
        return dx.cpu().numpy(), dl.cpu().numpy()
    before = step()
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc)
    with pytest.raises(capi.DtoError, match="dto_kkt_factor has not been called"):
        _solve(s, RX, RC)
    s.kkt_factor()
    first = _solve(s, RX, RC)
    assert np.all(np.isfinite(first[0])) and np.all(np.isfinite(first[1]))
    after = step()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the step wrote its own records over the factor
    with pytest.raises(capi.DtoError, match="dto_kkt_factor has not been called"):
        _solve(s, RX, RC)
    # factor again (the assembled system is still there): the same solution as before, bit for bit
    s.kkt_factor()
    again = _solve(s, RX, RC)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])

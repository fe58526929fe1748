"""dto_kkt_lbfgs_border on the tile path: the compact limited-memory BFGS matrix
    B = sigma I - W M^-1 W',  W = [sigma S, Y],  M = [[sigma S'S, L], [L', -D]]   (L, D: strictly lower part / diagonal of S'Y)
as a border of 2 m rows on a first-order factorisation (dto_kkt_assemble_first_order with sigma on the x-diagonal), so that
dto_kkt_border_solve with rhs_b = 0 returns K^-1 r for K = [[diag + B, J'], [J, -diag(sigma_c) - delta_c I]].

Reference: numpy on oracle/padded_model.py (dense_derivatives gives J); the compact matrices are the dozen lines of _compact below.
Bar: the project's 1e-8 of the largest entry of the reference solution (tests/test_wide_border_gpu.py).
64 states, B = 3, m = 6, npairs = (6, 3, 0), sigma = (0.7, 1.3, 1.0), at T = 4 and T = 9.  S is standard normal, Y = 0.3 S + 0.05 noise;
SEED was chosen on the CPU so that M is regular and diag + B positive definite for every instance (asserted before any launch)."""
import ctypes

import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu

B, M, DW, DC = 3, 6, 2.0, 1e-5
NPAIRS, SIGMA = (6, 3, 0), (0.7, 1.3, 1.0)
SEED = 0
_CASES = {}


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _compact(S, Y, sg):
    """(M, W) of the pairs in the rows of S and Y, oldest first"""
    SY = S @ Y.T
    L, D = np.tril(SY, -1), np.diag(np.diag(SY))
    return np.block([[sg * (S @ S.T), L], [L.T, -D]]), np.hstack([sg * S.T, Y.T])


def _inertia_rule(Mm, Cm):
    """the rule of dto_kkt_lbfgs_border: as many negative eigenvalues in the Schur complement as in M, none numerically zero"""
    def signs(A):
        e = np.linalg.eigvalsh(0.5 * (A + A.T))
        return int(np.sum(e < 0)), bool(np.any(np.abs(e) <= 1e-13 * np.max(np.abs(A))))
    (nm, tm), (ns, ts) = signs(Mm), signs(Cm)
    return int(nm == ns and not tm and not ts)


def _case(T):
    """Point, diagonals, history, the dense matrices and the reference flags: computed once per T, shared, never changed."""
    if T not in _CASES:
        from oracle.padded_model import PaddedAcrobot, dense_derivatives
        model = PaddedAcrobot(64, 1)
        nz, nc = (T - 1) * 65 + 64, (T - 1) * 64
        rng = np.random.default_rng(SEED * 100 + T)
        Z = rng.random((B, nz))
        SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
        SX[:, ::3] = 0.0
        S = rng.standard_normal((B, M, nz))
        Y = 0.3 * S + 0.05 * rng.standard_normal((B, M, nz))
        R = rng.standard_normal((B, nz + nc))
        Ks, K0s, want_ok = [], [], []
        for b in range(B):
            _, _, _, J, _ = dense_derivatives(model, T, Z[b], np.zeros(nc))
            K0 = np.block([[np.diag(DW + SX[b] + SIGMA[b]), J.T], [J, -np.diag(DC + SC[b])]])
            K0s.append(K0)
            k = NPAIRS[b]
            if k == 0:
                Ks.append(K0.copy()); want_ok.append(1)
                continue
            Mm, W = _compact(S[b, :k], Y[b, :k], SIGMA[b])
            assert np.linalg.cond(Mm) < 1e6, ("M must be regular: pick another SEED", T, b)
            Bc = SIGMA[b] * np.eye(nz) - W @ np.linalg.solve(Mm, W.T)
            assert np.min(np.linalg.eigvalsh(Bc + np.diag(DW + SX[b]))) > 0.0, ("diag + B must be positive definite: pick another SEED", T, b)
            K = K0.copy()
            K[:nz, :nz] += Bc - SIGMA[b] * np.eye(nz)
            Ks.append(K)
            U = np.vstack([W, np.zeros((nc, 2 * k))])
            want_ok.append(_inertia_rule(Mm, Mm - U.T @ np.linalg.solve(K0, U)))
        for a in (Z, SX, SC, S, Y, R, *Ks, *K0s):
            a.setflags(write=False)
        _CASES[T] = dict(nz=nz, nc=nc, Z=Z, SX=SX, SC=SC, S=S, Y=Y, R=R, Ks=Ks, K0s=K0s, want_ok=want_ok)
    return _CASES[T]


def _factor(s, c):
    """first-order system with sigma beside the other diagonal terms, factorised"""
    nz, nc = c["nz"], c["nc"]
    keep = [_dev(c["Z"]), _dev(c["SX"] + np.array(SIGMA)[:, None]), _dev(c["SC"])]
    s.kkt_assemble_first_order(keep[0].data_ptr(), B, nz, DW, DC, sigma_x_ptr=keep[1].data_ptr(), ldsx=nz, sigma_c_ptr=keep[2].data_ptr(), ldsc=nc)
    ok, neg = s.kkt_factor()
    assert np.all(ok == 1) and np.all(neg == nc), (ok, neg)


def _border(s, c, Y=None, npairs=NPAIRS):
    dS, dY = _dev(c["S"].reshape(B * M, -1)), _dev((c["Y"] if Y is None else Y).reshape(B * M, -1))
    return s.kkt_lbfgs_border(M, dS.data_ptr(), c["nz"], dY.data_ptr(), c["nz"], SIGMA, npairs=npairs)


def _border_solve(s, c):
    import torch
    nz, nc = c["nz"], c["nc"]
    rx, rc, rb = _dev(c["R"][:, :nz]), _dev(c["R"][:, nz:]), _dev(np.zeros((B, 2 * M)))
    sx = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    sc = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    sb = torch.full((B, 2 * M), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_border_solve(rx.data_ptr(), nz, rc.data_ptr(), nc, rb.data_ptr(), 2 * M, sx.data_ptr(), nz, sc.data_ptr(), nc, sb.data_ptr(), 2 * M)
    torch.cuda.synchronize()
    return np.concatenate([sx.cpu().numpy(), sc.cpu().numpy()], axis=1), sb.cpu().numpy()


def _plain_solve(s, c):
    import torch
    nz, nc = c["nz"], c["nc"]
    rx, rc = _dev(c["R"][:, :nz]), _dev(c["R"][:, nz:])
    sx = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    sc = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_solve(rx.data_ptr(), nz, rc.data_ptr(), nc, sx.data_ptr(), nz, sc.data_ptr(), nc)
    torch.cuda.synchronize()
    return np.concatenate([sx.cpu().numpy(), sc.cpu().numpy()], axis=1)


@pytest.mark.parametrize("T", [4, 9])
def test_border_solve_equals_the_dense_compact_solve(T):
    s, c = product_solver("acrobot_padded", T)[0], _case(T)
    _factor(s, c)
    ok, singular = _border(s, c)
    X, _ = _border_solve(s, c)
    assert np.all(singular == 0), singular
    for b in range(B):
        ref = np.linalg.solve(c["Ks"][b], c["R"][b])
        err = float(np.max(np.abs(X[b] - ref))) / float(np.max(np.abs(ref)))
        plain = float(np.max(np.abs(np.linalg.solve(c["K0s"][b], c["R"][b]) - ref))) / float(np.max(np.abs(ref)))
        print(f"  T={T} instance {b} ({NPAIRS[b]} pairs): max|x - dense| / max|x| = {err:.2e}   (K0 alone is {plain:.2e} away)")
        assert np.all(np.isfinite(X[b])) and err <= 1e-8, (T, b, err)
        if NPAIRS[b] > 0:
            assert plain > 1e-3, "the low-rank part must matter at this point"
    assert list(ok) == c["want_ok"], (list(ok), c["want_ok"])
    # the instance without pairs: exactly the plain solve against the same records
    assert np.array_equal(X[2], _plain_solve(s, c)[2])
    # run-to-run bit identity, the border formed again from the same history
    ok2, singular2 = _border(s, c)
    X2, Yb2 = _border_solve(s, c)
    assert np.array_equal(X, X2) and np.array_equal(ok, ok2) and np.array_equal(singular, singular2)


@pytest.mark.parametrize("T", [4, 9])
def test_a_pair_without_curvature_clears_the_flags_of_its_instance_only(T):
    s, c = product_solver("acrobot_padded", T)[0], _case(T)
    _factor(s, c)
    _border(s, c)
    X, _ = _border_solve(s, c)
    Ybad = np.array(c["Y"])
    Ybad[1, 1] = 0.0                                   # y = 0 in pair 1 of instance 1: a zero row in M and in the Schur complement
    ok, singular = _border(s, c, Y=Ybad)
    Xb, _ = _border_solve(s, c)
    assert ok[1] == 0 and singular[1] == 1, (ok, singular)
    assert ok[0] == c["want_ok"][0] and ok[2] == c["want_ok"][2] and singular[0] == 0 and singular[2] == 0
    assert np.all(np.isnan(Xb[1]))
    assert np.array_equal(X[0], Xb[0]) and np.array_equal(X[2], Xb[2])


NEG_SEED = 500   # chosen on the CPU: see the assertions on `want` and `regular` below


def test_a_regular_schur_complement_of_the_wrong_inertia_clears_the_flag():
    """inertia_ok = 0 from the COUNT, not from a zero eigenvalue: instance 0 gets six pairs in the nullspace of J with negative
    curvature (Y = -0.3 S + noise) on a nearly bare diagonal (delta_w = 1e-3, no sigma_x beside sigma), so that K = K0 - U M^-1 U'
    is indefinite on that nullspace -- M is positive definite there and the Schur complement has six negative eigenvalues, both
    far from singular.  Instance 1 keeps three of the ordinary pairs (flag 1), instance 2 has none (flag 1)."""
    from oracle.padded_model import PaddedAcrobot, dense_derivatives
    T, dw = 4, 1e-3
    s, c = product_solver("acrobot_padded", T)[0], _case(T)
    nz, nc = c["nz"], c["nc"]
    rng = np.random.default_rng(NEG_SEED)
    S, Y = np.array(c["S"]), np.array(c["Y"])
    _, _, _, J0, _ = dense_derivatives(PaddedAcrobot(64, 1), T, c["Z"][0], np.zeros(nc))
    null = np.linalg.svd(J0)[2][nc:]                    # rows: an orthonormal basis of the nullspace of J at instance 0
    S[0] = rng.standard_normal((M, null.shape[0])) @ null
    Y[0] = -0.3 * S[0] + 0.05 * rng.standard_normal((M, nz))
    want, regular = [], []
    for b in range(B):
        k = NPAIRS[b]
        if k == 0:
            want.append(1); regular.append(True)
            continue
        _, _, _, J, _ = dense_derivatives(PaddedAcrobot(64, 1), T, c["Z"][b], np.zeros(nc))
        K0 = np.block([[np.diag(np.full(nz, dw + SIGMA[b])), J.T], [J, -DC * np.eye(nc)]])
        Mm, W = _compact(S[b, :k], Y[b, :k], SIGMA[b])
        U = np.vstack([W, np.zeros((nc, 2 * k))])
        Cm = Mm - U.T @ np.linalg.solve(K0, U)
        want.append(_inertia_rule(Mm, Cm))
        regular.append(all(np.min(np.abs(np.linalg.eigvalsh(0.5 * (A + A.T)))) > 1e-3 * np.max(np.abs(A)) for A in (Mm, Cm)))
    assert want == [0, 1, 1] and all(regular), ("pick another NEG_SEED", want, regular)
    keep = [_dev(c["Z"]), _dev(np.tile(np.array(SIGMA)[:, None], (1, nz)))]
    s.kkt_assemble_first_order(keep[0].data_ptr(), B, nz, dw, DC, sigma_x_ptr=keep[1].data_ptr(), ldsx=nz)
    ok0, neg = s.kkt_factor()
    assert np.all(ok0 == 1) and np.all(neg == nc), (ok0, neg)       # K0 itself has the right inertia
    dS, dY = _dev(S.reshape(B * M, -1)), _dev(Y.reshape(B * M, -1))
    ok, singular = s.kkt_lbfgs_border(M, dS.data_ptr(), nz, dY.data_ptr(), nz, SIGMA, npairs=NPAIRS)
    print(f"  inertia_ok {list(ok)} (numpy rule {want}), singular {list(singular)}")
    assert list(ok) == want and np.all(singular == 0), (list(ok), want, singular)


def test_error_table_and_refused_calls_write_nothing():
    import dto_amd
    from dto_amd import capi, problems as P
    T = 4
    s, c = product_solver("acrobot_padded", T)[0], _case(T)
    nz = c["nz"]
    _factor(s, c)
    _border(s, c)
    X, _ = _border_solve(s, c)
    dS, dY = _dev(c["S"].reshape(B * M, -1)), _dev(c["Y"].reshape(B * M, -1))
    sp, yp = dS.data_ptr(), dY.data_ptr()

    def refused(code, text, m, s_ptr, lds, y_ptr, ldy):
        with pytest.raises(capi.DtoError) as e:
            s.kkt_lbfgs_border(m, s_ptr, lds, y_ptr, ldy, SIGMA)
        assert e.value.code == code and text in str(e.value), (code, text, str(e.value))
    refused(1, "m < 1", 0, sp, nz, yp, nz)
    refused(4, "one panel", 9, sp, nz, yp, nz)
    refused(1, "null argument", M, 0, nz, yp, nz)
    refused(1, "null argument", M, sp, nz, 0, nz)
    refused(1, "leading dimension", M, sp, nz - 1, yp, nz)
    refused(1, "leading dimension", M, sp, nz, yp, nz - 1)
    lib, h = s._solve_nlp._lib, s._solve_nlp._h
    rc = lib.dto_kkt_lbfgs_border(h, M, sp, nz, yp, nz, None, None, None, None, None)     # sigma is required
    assert rc == 1 and b"null argument" in lib.dto_last_error()
    # refused calls write nothing: the border of before still solves, bit for bit
    X2, _ = _border_solve(s, c)
    assert np.array_equal(X, X2)
    # no factor: assembled but not factorised, and not assembled at all (a fresh handle)
    keep = [_dev(c["Z"])]
    s.kkt_assemble_first_order(keep[0].data_ptr(), B, nz, DW, DC)
    refused(1, "dto_kkt_factor has not been called", M, sp, nz, yp, nz)
    p = P.build_acrobot_padded(T=T)
    fresh = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
    sig = (ctypes.c_double * B)(*SIGMA)
    rc = fresh._solve_nlp._lib.dto_kkt_lbfgs_border(fresh._solve_nlp._h, M, sp, nz, yp, nz, None, sig, None, None, None)
    assert rc == 1 and b"dto_kkt_assemble has not been called" in lib.dto_last_error()
    # lane-per-instance path
    lane, _ = product_solver("pendulum", 6)
    rc = lane._solve_nlp._lib.dto_kkt_lbfgs_border(lane._solve_nlp._h, M, sp, nz, yp, nz, None, sig, None, None, None)
    assert rc == 4 and b"tile path only" in lib.dto_last_error()

"""dto_kkt_lbfgs_border_rows on the tile path: the compact limited-memory BFGS matrix AND nr rows of the caller's in one border of
2 m + nr <= 16 rows on a first-order factorisation,
    [ K0  U   G' ] [ v ]   [ r ]      U' = [sigma S; Y],  M the compact matrix,  G the rows,  C their nr x nr block
    [ U'  M   0  ] [ w ] = [ 0 ]      <=>  [K G'; G C] [v; y] = [r; t],  K = K0 - U M^-1 U' = first-order system + B,
    [ G   0   C  ] [ y ]   [ t ]           B = sigma I - W M^-1 W'
Reference: numpy on oracle/padded_model.py (dense_derivatives gives J, H is dropped) and the dozen lines of _compact below.
Bar: the project's 1e-8 of the largest entry of the reference solution (tests/test_wide_border_gpu.py); for
the product, 1e-8 of the largest entry of |A| |solution|.
64 states, B = 3, m = 6, npairs = (6, 3, 0), sigma = (0.7, 1.3, 1.0), delta_w = 0.8, delta_c = 1e-6, at T = 4 and T = 9.  The rows:
  nr = 1   one dense random row, with a constraint side (g_c, 0.2 x standard normal), C = -0.5 (1 + b).  Such a row is no
           constraint row of K: at T = 9 its constraint side turns the eigenvalue it adds to the Schur complement positive (+26, +0.72
           and +28 beside entries of some hundreds -- a regular matrix with the wrong COUNT, flags 0), at T = 4 it does not (flags 1);
           the numpy rule says which, the solve is checked either way
  nr = 4   the sum row and the product row of tests/test_wide_general_border_gpu.py (at T = 9 its knots (2, 5) and (3, 6), at T = 4,
           which has no knot 5, the knots (1, 3) and (2, 4)) and two dense random rows, no g_c, C = -diag(0, 0.3, 1e-6, 0.7)
S is standard normal, Y = 0.3 S + 0.05 noise: the history of tests/test_wide_lbfgs_border_gpu.py."""
import ctypes

import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu

B, M, DW, DC = 3, 6, 0.8, 1e-6
NPAIRS, SIGMA = (6, 3, 0), (0.7, 1.3, 1.0)
D4 = (0.0, 0.3, 1e-6, 0.7)
ROWS = {4: [(1, 3, 0.2, False), (2, 4, 0.1, True)], 9: [(2, 5, 0.2, False), (3, 6, 0.1, True)]}
_CASES = {}


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _compact(S, Y, sg):
    """(M, W) of the pairs in the rows of S and Y, oldest first"""
    SY = S @ Y.T
    L, D = np.tril(SY, -1), np.diag(np.diag(SY))
    return np.block([[sg * (S @ S.T), L], [L.T, -D]]), np.hstack([sg * S.T, Y.T])


def _signs(A):
    e = np.linalg.eigvalsh(0.5 * (A + A.T))
    return int(np.sum(e < 0)), bool(np.any(np.abs(e) <= 1e-13 * np.max(np.abs(A))))


def _inertia_rule(Mm, Sc, nr):
    """the rule of dto_kkt_lbfgs_border_rows: neg(M) + nr negative eigenvalues in the Schur complement, none numerically zero in either"""
    (nm, tm), (ns, ts) = (_signs(Mm) if Mm.size else (0, False)), _signs(Sc)
    return int(nm + nr == ns and not tm and not ts)


def _rows(T, nr, Z, rng, nz, nc):
    """G [B][nr][nz + nc] at the points Z and C [B][nr][nr]"""
    G, Cb = np.zeros((B, nr, nz + nc)), np.zeros((B, nr, nr))
    for b in range(B):
        if nr == 1:
            G[b, 0] = rng.standard_normal(nz + nc)
            G[b, 0, nz:] *= 0.2
            Cb[b] = -0.5 * (1 + b)
            continue
        for j, (ka, kb, _, prod) in enumerate(ROWS[T]):
            ia, ib = (ka - 1) * 65, (kb - 1) * 65                      # q1 of the two knots
            G[b, j, ia] += Z[b, ib] if prod else 1.0
            G[b, j, ib] += Z[b, ia] if prod else 1.0
        G[b, 2:, :nz] = rng.standard_normal((2, nz))
        Cb[b] = -np.diag(D4)
    return G, Cb


def _case(T, nr, bad_pair=False):
    """Point, history, rows, the dense matrices, the reference solutions and flags: computed once per case, shared, never changed."""
    key = (T, nr, bad_pair)
    if key not in _CASES:
        from oracle.padded_model import PaddedAcrobot, dense_derivatives
        model = PaddedAcrobot(64, 1)
        nz, nc = (T - 1) * 65 + 64, (T - 1) * 64
        rng = np.random.default_rng(1000 + T)                          # (the same point and history for every nr of one T)
        Z = rng.random((B, nz))
        S = rng.standard_normal((B, M, nz))
        Y = 0.3 * S + 0.05 * rng.standard_normal((B, M, nz))
        if bad_pair:
            Y[1, 1] = 0.0                                              # pair 1 of instance 1 has no curvature: a zero row in M
        R = rng.standard_normal((B, nz + nc))
        G, Cb = _rows(T, nr, Z, np.random.default_rng(2000 + 10 * T + nr), nz, nc)
        Rb = np.zeros((B, 2 * M + nr))
        Rb[:, 2 * M:] = np.random.default_rng(3000 + 10 * T + nr).standard_normal((B, nr))
        As, sols, want_ok = [], [], []
        for b in range(B):
            _, _, _, J, _ = dense_derivatives(model, T, Z[b], np.zeros(nc))
            K0 = np.block([[(DW + SIGMA[b]) * np.eye(nz), J.T], [J, -DC * np.eye(nc)]])
            k = NPAIRS[b]
            Mm, W = _compact(S[b, :k], Y[b, :k], SIGMA[b]) if k else (np.zeros((0, 0)), np.zeros((nz, 0)))
            U = np.vstack([W, np.zeros((nc, 2 * k))])
            Ub = np.hstack([U, G[b].T])                                # the whole border, (nz + nc) x (2 k + nr)
            Cfull = np.block([[Mm, np.zeros((2 * k, nr))], [np.zeros((nr, 2 * k)), Cb[b]]])
            want_ok.append(_inertia_rule(Mm, Cfull - Ub.T @ np.linalg.solve(K0, Ub), nr))
            A = np.block([[K0, Ub], [Ub.T, Cfull]])
            As.append(A)
            if bad_pair and b == 1:
                sols.append(None)
                continue
            assert np.linalg.cond(Mm) < 1e6 if k else True, ("M must be regular: pick another seed", T, b)
            sol = np.linalg.solve(A, np.concatenate([R[b], np.zeros(2 * k), Rb[b, 2 * M:]]))
            # the same from the eliminated form: K = first-order system + B, bordered by the rows alone
            K = K0.copy()
            if k:
                K[:nz, :nz] -= W @ np.linalg.solve(Mm, W.T)
            el = np.linalg.solve(np.block([[K, G[b].T], [G[b], Cb[b]]]), np.concatenate([R[b], Rb[b, 2 * M:]]))
            assert np.max(np.abs(el[:nz + nc] - sol[:nz + nc])) <= 1e-9 * np.max(np.abs(sol)), "the two dense forms agree"
            if k:
                assert np.max(np.abs(sol[nz + nc:nz + nc + 2 * k] + np.linalg.solve(Mm, U.T @ sol[:nz + nc]))) <= 1e-9 * np.max(np.abs(sol))
            sols.append(sol)
        for a in (Z, S, Y, R, G, Cb, Rb):
            a.setflags(write=False)
        _CASES[key] = dict(T=T, nr=nr, nz=nz, nc=nc, Z=Z, S=S, Y=Y, R=R, G=G, Cb=Cb, Rb=Rb, As=As, sols=sols, want_ok=want_ok)
    return _CASES[key]


def _factor(s, c):
    """first-order system with delta_w and sigma on the x-diagonal, factorised"""
    nz, nc = c["nz"], c["nc"]
    keep = [_dev(c["Z"]), _dev(np.tile(np.array(SIGMA)[:, None], (1, nz)))]
    s.kkt_assemble_first_order(keep[0].data_ptr(), B, nz, DW, DC, sigma_x_ptr=keep[1].data_ptr(), ldsx=nz)
    ok, neg = s.kkt_factor()
    assert np.all(ok == 1) and np.all(neg == nc), (ok, neg)


def _border(s, c):
    nz, nc, nr = c["nz"], c["nc"], c["nr"]
    dS, dY = _dev(c["S"].reshape(B * M, -1)), _dev(c["Y"].reshape(B * M, -1))
    gx, cb = _dev(c["G"][:, :, :nz].reshape(B * nr, nz)), _dev(c["Cb"].reshape(B, nr * nr))
    gc = _dev(c["G"][:, :, nz:].reshape(B * nr, nc)) if nr == 1 else None
    return s.kkt_lbfgs_border_rows(M, dS.data_ptr(), nz, dY.data_ptr(), nz, SIGMA, nr, gx.data_ptr(), nz, cb.data_ptr(), nr * nr,
                                   gc_ptr=gc.data_ptr() if gc is not None else 0, ldgc=nc if gc is not None else 0, npairs=NPAIRS)


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float64)


def _border_solve(s, c, nb):
    import torch
    nz, nc = c["nz"], c["nc"]
    rx, rc, rb = _dev(c["R"][:, :nz]), _dev(c["R"][:, nz:]), _dev(c["Rb"][:, :nb] if nb == 2 * M else c["Rb"])
    sx, sc, sb = _nan(B, nz), _nan(B, nc), _nan(B, nb)
    s.kkt_border_solve(rx.data_ptr(), nz, rc.data_ptr(), nc, rb.data_ptr(), nb, sx.data_ptr(), nz, sc.data_ptr(), nc, sb.data_ptr(), nb)
    torch.cuda.synchronize()
    return np.concatenate([sx.cpu().numpy(), sc.cpu().numpy()], axis=1), sb.cpu().numpy()


def _expand(c, b, sol):
    """reference [v; w; y] of instance b in the device's layout of sol_b: the k pairs of an instance in the first k entries of
    the S block and of the Y block, zeros for the pairs it does not have"""
    n, k, nr = c["nz"] + c["nc"], NPAIRS[b], c["nr"]
    w = np.zeros(2 * M + nr)
    w[:k], w[M:M + k], w[2 * M:] = sol[n:n + k], sol[n + k:n + 2 * k], sol[n + 2 * k:]
    return sol[:n], w


@pytest.mark.parametrize("T,nr", [(4, 1), (4, 4), (9, 1), (9, 4)])
def test_bordered_solve_and_product_equal_the_dense_ones(T, nr):
    import torch
    s, c = product_solver("acrobot_padded", T)[0], _case(T, nr)
    nz, nc, nb = c["nz"], c["nc"], 2 * M + nr
    _factor(s, c)
    ok, singular = _border(s, c)
    X, Yb = _border_solve(s, c, nb)
    print(f"  T={T} nr={nr}: inertia_ok {list(ok)} (numpy rule {c['want_ok']}), singular {list(singular)}")
    assert np.all(singular == 0), singular
    assert list(ok) == c["want_ok"], (list(ok), c["want_ok"])
    # the product of the solution with the bordered matrix gives the right-hand side back
    vx, vc, vb = _dev(X[:, :nz]), _dev(X[:, nz:]), _dev(Yb)
    ox, oc, ob = _nan(B, nz), _nan(B, nc), _nan(B, nb)
    s.kkt_border_multiply(vx.data_ptr(), nz, vc.data_ptr(), nc, vb.data_ptr(), nb, ox.data_ptr(), nz, oc.data_ptr(), nc, ob.data_ptr(), nb)
    torch.cuda.synchronize()
    P_, Pb = np.concatenate([ox.cpu().numpy(), oc.cpu().numpy()], axis=1), ob.cpu().numpy()
    for b in range(B):
        v, w = _expand(c, b, c["sols"][b])
        scale = max(float(np.max(np.abs(v))), float(np.max(np.abs(w))))
        ev, ew = float(np.max(np.abs(X[b] - v))), float(np.max(np.abs(Yb[b] - w)))
        k = NPAIRS[b]
        bound = 1e-8 * float(np.max(np.abs(c["As"][b]) @ np.abs(c["sols"][b])))
        res = max(float(np.max(np.abs(P_[b] - c["R"][b]))), float(np.max(np.abs(Pb[b] - c["Rb"][b]))))
        print(f"    instance {b} ({k} pairs): |x - dense| {ev:.2e}, |sol_b - dense| {ew:.2e} (rows {np.max(np.abs(Yb[b, 2 * M:] - w[2 * M:])):.2e}), "
              f"scale {scale:.2e}; product residual {res:.2e} (bound {bound:.2e})")
        assert np.all(np.isfinite(X[b])) and np.all(np.isfinite(Yb[b]))
        assert ev <= 1e-8 * scale and ew <= 1e-8 * scale, (T, nr, b, ev, ew, scale)
        assert res <= bound, (T, nr, b, res, bound)
    # two runs, the border formed again from the same arrays: identical bits
    ok2, singular2 = _border(s, c)
    X2, Yb2 = _border_solve(s, c, nb)
    assert np.array_equal(X, X2) and np.array_equal(Yb, Yb2) and np.array_equal(ok, ok2) and np.array_equal(singular, singular2)


@pytest.mark.parametrize("T", [4, 9])
def test_a_pair_without_curvature_clears_the_flag_of_its_instance_only(T):
    nr = 4
    s, good, bad = product_solver("acrobot_padded", T)[0], _case(T, nr), _case(T, nr, bad_pair=True)
    _factor(s, good)
    _border(s, good)
    X, Yb = _border_solve(s, good, 2 * M + nr)
    ok, singular = _border(s, bad)
    Xb, Ybb = _border_solve(s, bad, 2 * M + nr)
    print(f"  inertia_ok {list(ok)} (numpy rule {bad['want_ok']}), singular {list(singular)}")
    assert bad["want_ok"][1] == 0 and list(ok) == bad["want_ok"], (list(ok), bad["want_ok"])
    assert bad["want_ok"][0] == good["want_ok"][0] and bad["want_ok"][2] == good["want_ok"][2]
    assert singular[1] == 1 and singular[0] == 0 and singular[2] == 0
    assert np.all(np.isnan(Xb[1]))
    assert np.array_equal(X[0], Xb[0]) and np.array_equal(X[2], Xb[2]) and np.array_equal(Yb[0], Ybb[0]) and np.array_equal(Yb[2], Ybb[2])


@pytest.mark.parametrize("T", [4, 9])
def test_no_rows_is_kkt_lbfgs_border_bit_for_bit(T):
    s, c = product_solver("acrobot_padded", T)[0], _case(T, 1)
    nz = c["nz"]
    _factor(s, c)
    dS, dY = _dev(c["S"].reshape(B * M, -1)), _dev(c["Y"].reshape(B * M, -1))
    ok0, sing0 = s.kkt_lbfgs_border(M, dS.data_ptr(), nz, dY.data_ptr(), nz, SIGMA, npairs=NPAIRS)
    X0, Y0 = _border_solve(s, c, 2 * M)
    _border(s, c)                                                        # (a border with a row in between)
    ok1, sing1 = s.kkt_lbfgs_border_rows(M, dS.data_ptr(), nz, dY.data_ptr(), nz, SIGMA, 0, 0, 0, 0, 0, npairs=NPAIRS)
    X1, Y1 = _border_solve(s, c, 2 * M)
    assert np.all(np.isfinite(X0)) and np.array_equal(X0, X1) and np.array_equal(Y0, Y1)
    assert np.array_equal(ok0, ok1) and np.array_equal(sing0, sing1)


def test_error_table_and_refused_calls_write_nothing():
    import torch
    from dto_amd import capi
    T, nr = 4, 4
    s, c = product_solver("acrobot_padded", T)[0], _case(T, nr)
    nz, nc = c["nz"], c["nc"]
    _factor(s, c)
    _border(s, c)
    X, Yb = _border_solve(s, c, 2 * M + nr)
    dS, dY = _dev(c["S"].reshape(B * M, -1)), _dev(c["Y"].reshape(B * M, -1))
    g5 = _nan(B * 5, nz)                                                 # never read: every call below is refused
    c5, gc5 = _nan(B, 25), _nan(B * 5, nc)
    sp, yp, gp, cp, gcp = (a.data_ptr() for a in (dS, dY, g5, c5, gc5))
    lib, h = s._solve_nlp._lib, s._solve_nlp._h
    sig = (ctypes.c_double * B)(*SIGMA)

    def refused(code, text, m=M, nr_=4, s_=sp, lds=nz, y_=yp, ldy=nz, gx=gp, ldgx=nz, gc=None, ldgc=0, cc=cp, ldc=16):
        okv, sgv = (ctypes.c_int32 * B)(*([-7] * B)), (ctypes.c_int32 * B)(*([-7] * B))
        rc = lib.dto_kkt_lbfgs_border_rows(h, m, s_, lds, y_, ldy, None, sig, nr_, gx, ldgx, gc, ldgc, cc, ldc, okv, sgv, None)
        msg = lib.dto_last_error().decode()
        assert rc == code and text in msg, (rc, code, text, msg)
        assert list(okv) == [-7] * B and list(sgv) == [-7] * B
    refused(4, "one panel", nr_=5, ldc=25)                               # 2 * 6 + 5 > 16
    refused(4, "one panel", m=7, nr_=3, ldc=9)
    refused(1, "nr < 0", nr_=-1)
    refused(1, "null argument", gx=None)
    refused(1, "null argument", cc=None)
    refused(1, "null argument", s_=None)
    refused(1, "leading dimension", ldgx=nz - 1)
    refused(1, "leading dimension", ldc=15)
    refused(1, "leading dimension", gc=gcp, ldgc=nc - 1)
    refused(1, "leading dimension", lds=nz - 1)
    refused(1, "m < 1", m=0)
    with pytest.raises(capi.DtoError) as e:                              # ... and through the wrapper
        s.kkt_lbfgs_border_rows(M, sp, nz, yp, nz, SIGMA, 5, gp, nz, cp, 25)
    assert e.value.code == 4 and "one panel" in str(e.value)
    # nothing was written or launched: the inputs pre-filled with NaN are as they were, and the border of before still solves, bit for bit
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(g5))) and bool(torch.all(torch.isnan(c5))) and bool(torch.all(torch.isnan(gc5)))
    X2, Yb2 = _border_solve(s, c, 2 * M + nr)
    assert np.array_equal(X, X2) and np.array_equal(Yb, Yb2)
    # lane-per-instance path
    lane, _ = product_solver("pendulum", 6)
    rc = lane._solve_nlp._lib.dto_kkt_lbfgs_border_rows(lane._solve_nlp._h, M, sp, nz, yp, nz, None, sig, 4, gp, nz, None, 0, cp, 16, None, None, None)
    assert rc == 4 and b"tile path only" in lib.dto_last_error()

"""Bordered solves against the stored factor on the tile path: dto_kkt_border_factor / dto_kkt_border_solve.

    [ K   G' ] [ v ]   [ r ]        G: nb x N border rows (nb <= 16), C: nb x nb of which the symmetric part is used
    [ G   C  ] [ y ] = [ s ]

dto_kkt_border_factor: Y = K^-1 G' (one panel through the stored records), P = G Y' on the f64 matrix cores (k_border_gram),
S = sym(C) - sym(P), its pivoted LU and the two flags (k_border_schur); dto_kkt_border_solve: v0 = K^-1 r, y = S^-1 (s - Y r)
(k_border_rhs), v = v0 - Y' y (k_border_sub).

Reference everywhere: numpy's dense solve of the ORACLE's bordered matrix [[K, G'], [G, (C + C')/2]], K from
oracle/padded_model.py: dense_kkt (embedded_dense_kkt for the 24-state problem) plus the sigmas, with the models and helpers of
tests/test_wide_linear_solver_gpu.py / test_wide_multi_solve_gpu.py.  Bar: the project's 1e-8 of max |solution| per instance,
over v and y together.  The systems (delta_w = 2 or 30, the sigmas of the existing tests, G standard normal) have cond2(K) of
1e1 .. 5e2, cond2 of the bordered matrix <= 6e2 and cond2(S) <= 8; a float64 Schur route in numpy agrees with the dense solve to
9e-16 .. 6e-15 there (tests/test_kkt_border_cpu.py restates that route), so the reference sits seven orders inside the bar.
Every test asserts cond2(bordered) <= 1e4 and prints its worst error; DESIGN.md section 4.3 holds the table of the MI355X run.
"""
import os

import numpy as np
import pytest

from test_wide_linear_solver_gpu import _assemble_factor, _dense, _dev, _solve
from test_wide_multi_solve_gpu import _quasi_definite_system, _solve_multi

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _border_factor(s, G, C, nz, nc, use_gc, lds=None):
    """G [B][nb][nz + nc] (the constraint part is not passed when use_gc is False), C [B][nb][nb] or None.  Padding of the inputs
    is NaN; the device copies are overwritten with NaN once the call has returned (it has consumed them)."""
    import torch
    B, nb, _ = G.shape
    ldgx, ldgc, ldc = lds or (nz, nc, nb * nb)
    hx, hc, hC = np.full((B * nb, ldgx), np.nan), np.full((B * nb, ldgc), np.nan), np.full((B, ldc), np.nan)
    hx[:, :nz], hc[:, :nc] = G[:, :, :nz].reshape(B * nb, nz), G[:, :, nz:].reshape(B * nb, nc)   # row b * nb + j
    if C is not None:
        hC[:, :nb * nb] = C.reshape(B, nb * nb)
    dx, dc, dC = _dev(hx), _dev(hc), _dev(hC)
    flags = s.kkt_border_factor(nb, dx.data_ptr(), ldgx, dc.data_ptr() if use_gc else 0, ldgc if use_gc else 0,
                                dC.data_ptr() if C is not None else 0, ldc if C is not None else 0)
    for t in (dx, dc, dC):
        t.fill_(NAN)
    torch.cuda.synchronize()
    return flags


def _border_solve(s, R, Sb, nz, nc, lds=None):
    """R [B][nz + nc], Sb [B][nb] -> [B][nz + nc + nb].  Inputs padded with NaN, outputs NaN everywhere before the call: every
    entry of a solution must have been written, no padding entry may have been."""
    import torch
    B, nb = Sb.shape
    ldrx, ldrc, ldrb, ldsx, ldsc, ldsb = lds or (nz, nc, nb, nz, nc, nb)
    hx, hc, hb = np.full((B, ldrx), np.nan), np.full((B, ldrc), np.nan), np.full((B, ldrb), np.nan)
    hx[:, :nz], hc[:, :nc], hb[:, :nb] = R[:, :nz], R[:, nz:], Sb
    dx, dc, db = _dev(hx), _dev(hc), _dev(hb)
    oX, oC, oB = (torch.full((B, ld), NAN, device="cuda", dtype=torch.float64) for ld in (ldsx, ldsc, ldsb))
    s.kkt_border_solve(dx.data_ptr(), ldrx, dc.data_ptr(), ldrc, db.data_ptr(), ldrb, oX.data_ptr(), ldsx, oC.data_ptr(), ldsc,
                       oB.data_ptr(), ldsb)
    torch.cuda.synchronize()
    oX, oC, oB = oX.cpu().numpy(), oC.cpu().numpy(), oB.cpu().numpy()
    assert np.all(np.isnan(oX[:, nz:])) and np.all(np.isnan(oC[:, nc:])) and np.all(np.isnan(oB[:, nb:])), "output padding was written"
    return np.concatenate([oX[:, :nz], oC[:, :nc], oB[:, :nb]], axis=1)


def _border(rng, B, nb, nz, nc, use_gc, ckind):
    G = rng.standard_normal((B, nb, nz + nc))
    if not use_gc:
        G[:, :, nz:] = 0.0
    if ckind == "negdiag":
        C = np.stack([-np.diag(1e-5 + rng.random(nb)) for _ in range(B)])
    elif ckind == "symmetric":
        C = rng.standard_normal((B, nb, nb))
        C = 0.5 * (C + C.transpose(0, 2, 1))
    elif ckind == "nonsymmetric":
        C = rng.standard_normal((B, nb, nb))
        assert not np.allclose(C, C.transpose(0, 2, 1))
    else:
        C = None
    return G, C


def _bordered(K, G, C):
    nb = G.shape[0]
    Cs = np.zeros((nb, nb)) if C is None else 0.5 * (C + C.T)
    M = np.block([[K, G.T], [G, Cs]])
    cond = np.linalg.cond(M)
    assert cond <= 1e4, ("the reference must be well conditioned", cond)
    return M


def _schur_eigs(K, G, C):
    nb = G.shape[0]
    S = (np.zeros((nb, nb)) if C is None else 0.5 * (C + C.T)) - G @ np.linalg.solve(K, G.T)
    return np.linalg.eigvalsh(0.5 * (S + S.T))


def _check_solves(s, Ms, rng, nz, nc, nb, n=3, lds=None, only=None):
    B, worst, last = len(Ms), 0.0, None
    for _ in range(n):
        R, Sb = rng.standard_normal((B, nz + nc)), rng.standard_normal((B, nb))
        last = (R, Sb, _border_solve(s, R, Sb, nz, nc, lds))
        for b in range(B):
            if only is not None and not only[b]:
                continue
            ref = np.linalg.solve(Ms[b], np.concatenate([R[b], Sb[b]]))
            err = float(np.max(np.abs(last[2][b] - ref)) / np.max(np.abs(ref)))
            worst = max(worst, err)
            assert np.all(np.isfinite(last[2][b])) and err <= 1e-8, (b, err)
    return worst, last


#        m, T, B, delta_w, nb, g_c,   C
CASES = [(1, 2, 2, 2.0, 1, False, "negdiag"),
         (1, 4, 2, 2.0, 5, False, "negdiag"),
         (1, 4, 2, 2.0, 16, True, "negdiag"),
         (3, 3, 2, 2.0, 12, False, "symmetric"),
         (1, 5, 2, 2.0, 16, False, None),
         (4, 3, 1, 30.0, 7, True, "nonsymmetric")]


@pytest.mark.parametrize("m,T,B,dw,nb,use_gc,ckind", CASES)
def test_border_solves_match_dense_solves(m, T, B, dw, nb, use_gc, ckind):
    """Three bordered right-hand sides per border, then a second dto_kkt_border_factor with another G and C on the same
    dto_kkt_factor (a stale Y or LU would show).  The flags against the oracle's Schur complement: negdef = every eigenvalue of
    S below zero, singular = 0."""
    s, Ks, rng, nz, nc = _quasi_definite_system(m, T, B, dw, 5 + T if m == 1 else 50 + m)
    worst = 0.0
    for rnd in range(2):
        G, C = _border(rng, B, nb, nz, nc, use_gc, ckind)
        negdef, singular = _border_factor(s, G, C, nz, nc, use_gc)
        Ms = [_bordered(Ks[b], G[b], None if C is None else C[b]) for b in range(B)]
        for b in range(B):
            eig = _schur_eigs(Ks[b], G[b], None if C is None else C[b])
            assert np.min(np.abs(eig)) > 1e-3, ("the sign pattern must be decidable", eig)
            assert negdef[b] == int(np.all(eig < 0)) and singular[b] == 0, (b, negdef, singular, eig)
        worst = max(worst, _check_solves(s, Ms, rng, nz, nc, nb)[0])
    print(f"  m={m} T={T} B={B} nb={nb} g_c={use_gc} C={ckind}: worst error / solution scale {worst:.2e}")


def test_border_flags_follow_the_schur_complement():
    """g_c = 0 and C <= 0 on a quasi-definite K: S = C - G_x (K^-1)_xx G_x' is negative definite, flag 1; with a random g_c the
    (K^-1)_cc block, which is negative definite, makes S positive definite here, flag 0.  Compared with the oracle's eigenvalues."""
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, 2, 2.0, 9)
    seen = set()
    for use_gc in (False, True):
        G, C = _border(rng, 2, 5, nz, nc, use_gc, "negdiag")
        negdef, singular = _border_factor(s, G, C, nz, nc, use_gc)
        for b in range(2):
            eig = _schur_eigs(Ks[b], G[b], C[b])
            print(f"  g_c={use_gc} instance {b}: eig(S) {eig.min():.3g} .. {eig.max():.3g}, negdef {negdef[b]}")
            assert np.min(np.abs(eig)) > 1e-3
            assert negdef[b] == int(np.all(eig < 0)) and singular[b] == 0
            seen.add(int(negdef[b]))
    assert seen == {0, 1}, "both signs must occur"


def test_border_singular_schur_complement():
    """Instance 0: border row 1 is zero and C = 0, so row and column 1 of S are exactly zero (Y_1 = K^-1 0 = 0): the second pivot is
    an exact zero.  schur_singular = 1 and NaN in every entry of its three solution arrays; instance 1 is not affected."""
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, 2, 2.0, 9)
    nb = 2
    G, _ = _border(rng, 2, nb, nz, nc, True, None)
    G[0, 1] = 0.0
    C = np.zeros((2, nb, nb))
    C[1] = -np.diag(1e-5 + rng.random(nb))
    negdef, singular = _border_factor(s, G, C, nz, nc, True)
    assert singular.tolist() == [1, 0] and negdef[0] == 0, (singular, negdef)
    M1 = _bordered(Ks[1], G[1], C[1])
    for _ in range(3):
        R, Sb = rng.standard_normal((2, nz + nc)), rng.standard_normal((2, nb))
        sol = _border_solve(s, R, Sb, nz, nc)
        assert np.all(np.isnan(sol[0])), "a singular instance returns NaN in every entry"
        ref = np.linalg.solve(M1, np.concatenate([R[1], Sb[1]]))
        err = float(np.max(np.abs(sol[1] - ref)) / np.max(np.abs(ref)))
        print(f"  instance 1 next to a singular one: error {err:.2e}")
        assert err <= 1e-8


def test_border_lu_exchanges_rows():
    """C = 60 x a random matrix and g_c = 0: S is indefinite with its largest entries off the diagonal, so the LU of S exchanges
    rows (the borders of the other tests are diagonally dominant and never do)."""
    s, Ks, _, nz, nc = _quasi_definite_system(1, 4, 2, 2.0, 9)
    from test_kkt_border_cpu import schur_factor
    nb, rng = 6, np.random.default_rng(107)
    G, _ = _border(rng, 2, nb, nz, nc, False, None)
    C = 60.0 * rng.standard_normal((2, nb, nb))
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(2)]
    for b in range(2):
        piv = schur_factor(Ks[b], G[b], C[b])[2]
        assert any(p != k for k, p in enumerate(piv)), "the case is there for the row exchanges"
    negdef, singular = _border_factor(s, G, C, nz, nc, False)
    assert negdef.tolist() == [0, 0] and singular.tolist() == [0, 0]
    worst, _ = _check_solves(s, Ms, rng, nz, nc, nb)
    print(f"  worst error / solution scale {worst:.2e}")


def test_border_gram_chunking():
    """DTO_BORDER_GRAM_CHUNK = 64 (rounded up to the slab of 128: four chunks of the 451 entries of a row, the last one 67 long),
    a value above N (one chunk) and the default: all within the bar, two runs with one setting bit-identical."""
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, 2, 2.0, 9)
    nb = 16
    assert nz + nc == 451
    G, C = _border(rng, 2, nb, nz, nc, True, "negdiag")
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(2)]
    R, Sb = rng.standard_normal((2, nz + nc)), rng.standard_normal((2, nb))
    saved = os.environ.pop("DTO_BORDER_GRAM_CHUNK", None)
    try:
        for setting in ("64", "100000", None):
            if setting is not None:
                os.environ["DTO_BORDER_GRAM_CHUNK"] = setting
            runs = []
            for _ in range(2):
                _border_factor(s, G, C, nz, nc, True)
                runs.append(_border_solve(s, R, Sb, nz, nc))
            os.environ.pop("DTO_BORDER_GRAM_CHUNK", None)
            assert np.array_equal(runs[0], runs[1]), setting
            for b in range(2):
                ref = np.linalg.solve(Ms[b], np.concatenate([R[b], Sb[b]]))
                err = float(np.max(np.abs(runs[0][b] - ref)) / np.max(np.abs(ref)))
                print(f"  chunk {setting}: instance {b} error {err:.2e}")
                assert err <= 1e-8, (setting, b, err)
    finally:
        if saved is not None:
            os.environ["DTO_BORDER_GRAM_CHUNK"] = saved


def test_border_padded_leading_dimensions():
    """All nine leading dimensions above their row lengths and all different, NaN in every input padding entry, outputs
    pre-filled with NaN: bit for bit the tight call, output padding still NaN (checked by _border_solve)."""
    s, Ks, rng, nz, nc = _quasi_definite_system(3, 3, 2, 2.0, 53)
    nb = 12
    G, C = _border(rng, 2, nb, nz, nc, True, "nonsymmetric")
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(2)]
    R, Sb = rng.standard_normal((2, nz + nc)), rng.standard_normal((2, nb))
    f0 = _border_factor(s, G, C, nz, nc, True)
    tight = _border_solve(s, R, Sb, nz, nc)
    f1 = _border_factor(s, G, C, nz, nc, True, lds=(nz + 5, nc + 3, nb * nb + 7))
    wide = _border_solve(s, R, Sb, nz, nc, lds=(nz + 1, nc + 2, nb + 4, nz + 6, nc + 9, nb + 11))
    assert np.array_equal(f0[0], f1[0]) and np.array_equal(f0[1], f1[1])
    assert np.all(np.isfinite(tight)) and np.array_equal(tight, wide)
    for b in range(2):
        ref = np.linalg.solve(Ms[b], np.concatenate([R[b], Sb[b]]))
        err = float(np.max(np.abs(wide[b] - ref)) / np.max(np.abs(ref)))
        print(f"  instance {b}: error {err:.2e}")
        assert err <= 1e-8


def test_border_calls_interleave_with_the_other_stored_factor_calls():
    """dto_kkt_solve, dto_kkt_solve_multi(3), dto_kkt_multiply and dto_kkt_solve_refined(2) before the border calls and between
    them: bit-identical every time, and the border solves stay within the bar."""
    from test_wide_kmul_gpu import _multiply
    from test_wide_refined_solve_gpu import _refined
    B, nb = 2, 5
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, B, 2.0, 21)
    R = rng.standard_normal((B, nz + nc))
    MX, MC = rng.standard_normal((B, 3, nz)), rng.standard_normal((B, 3, nc))

    def others():
        a = _solve(s, np.ascontiguousarray(R[:, :nz]), np.ascontiguousarray(R[:, nz:]))
        b_ = _solve_multi(s, MX, MC)
        return [a[0], a[1], b_[0], b_[1], _multiply(s, R, nz, nc), _refined(s, R, nz, nc, 2)]
    before = others()
    G, C = _border(rng, B, nb, nz, nc, True, "symmetric")
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(B)]
    _border_factor(s, G, C, nz, nc, True)
    between = others()
    w1, _ = _check_solves(s, Ms, rng, nz, nc, nb, n=1)
    middle = others()
    w2, _ = _check_solves(s, Ms, rng, nz, nc, nb, n=2)
    after = others()
    for other in (between, middle, after):
        for x, y in zip(before, other):
            assert np.all(np.isfinite(x)) and np.array_equal(x, y)
    print(f"  worst border error {max(w1, w2):.2e}")


def test_border_per_instance_parameters():
    """The per-instance (gain, weight) pairs of test_wide_multi_solve_per_instance_parameters."""
    import dto_amd
    from dto_amd import problems as P
    from oracle.padded_model import PaddedAcrobot
    T, B, dw, dc, nb = 3, 2, 2.0, 1e-5, 4
    p = P.build_acrobot_padded(T=T, parameters=(1.3, 0.7))
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       parameters=p["parameters"], name="acrobot_padded_par")
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    pairs = [(0.8, 1.5), (1.6, 0.4)]
    W = np.array([np.tile(pr, T) for pr in pairs])
    rng = np.random.default_rng(78)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
    SX[:, ::3] = 0.0
    ok, neg = _assemble_factor(s, Z, MU, dw, dc, SX, SC, W)
    assert np.all(neg == nc) and np.all(ok == 1)
    Ks = [_dense(PaddedAcrobot(64, 1, pairs[b]), T, Z[b], MU[b], dw, dc, SX[b], SC[b])[0] for b in range(B)]
    G, C = _border(rng, B, nb, nz, nc, False, "negdiag")
    _border_factor(s, G, C, nz, nc, False)
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(B)]
    worst, _ = _check_solves(s, Ms, rng, nz, nc, nb)
    print(f"  worst error / solution scale {worst:.2e}")


def test_border_on_an_embedded_problem():
    """The 24-state problem with stage rows of tests/test_wide_embedded_linear_gpu.py (T = 5) in the solver's layout, nb = 3,
    against embedded_dense_kkt."""
    import test_wide_embedded_linear_gpu as E
    s, c = E._solver("rows5"), E._system("rows5")
    nz, nc, nb = c["nz"], c["nc"], 3
    E._assemble(s, c)
    E._factor(s, nc)
    rng = np.random.default_rng(61)
    G, C = _border(rng, E.B, nb, nz, nc, True, "symmetric")
    _, singular = _border_factor(s, G, C, nz, nc, True)
    assert not np.any(singular)
    Ms = [_bordered(c["Ks"][b], G[b], C[b]) for b in range(E.B)]
    worst, _ = _check_solves(s, Ms, rng, nz, nc, nb)
    print(f"  rows5, delta_w = {c['dw']}: worst error / solution scale {worst:.2e}")


def test_border_misuse():
    """The state machine of include/dto.h call by call: error code, message fragment, and outputs that are still all NaN."""
    import torch
    import dto_amd
    from dto_amd import capi, problems as P
    T, B, dw, dc, nb = 3, 2, 2.0, 1e-5, 2
    p = P.build_acrobot_padded(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(12)
    dZ, dMU = _dev(rng.random((B, nz))), _dev(rng.random((B, nc)))
    dGX, dGC = _dev(rng.standard_normal((B * nb, nz))), _dev(rng.standard_normal((B * nb, nc)))
    dCC = _dev(-np.tile(np.eye(nb).reshape(1, nb * nb), (B, 1)))
    dRX, dRC, dRB = _dev(rng.standard_normal((B, nz))), _dev(rng.standard_normal((B, nc))), _dev(rng.standard_normal((B, nb)))
    oX, oC, oB = (torch.full((B, n), NAN, device="cuda", dtype=torch.float64) for n in (nz, nc, nb))
    lib, h = s._solve_nlp._lib, s._solve_nlp._h
    s._B = B
    INVALID, UNSUPPORTED = 1, 4

    def untouched():
        torch.cuda.synchronize()
        assert bool(torch.isnan(oX).all()) and bool(torch.isnan(oC).all()) and bool(torch.isnan(oB).all()), "a refused call wrote"

    def factor(n=nb, ldgx=nz, ldgc=nc, ldc=nb * nb, gx=None):
        return lib.dto_kkt_border_factor(h, n, dGX.data_ptr() if gx is None else gx, ldgx, dGC.data_ptr(), ldgc, dCC.data_ptr(), ldc,
                                         None, None, None)

    def solve(ldrx=nz, ldrc=nc, ldrb=nb, ldsx=nz, ldsc=nc, ldsb=nb, rb=None, sb=None):
        return lib.dto_kkt_border_solve(h, dRX.data_ptr(), ldrx, dRC.data_ptr(), ldrc, dRB.data_ptr() if rb is None else rb, ldrb,
                                        oX.data_ptr(), ldsx, oC.data_ptr(), ldsc, oB.data_ptr() if sb is None else sb, ldsb, None)

    def refused(rc, code, text):
        assert rc == code, (rc, code, lib.dto_last_error())
        assert text in lib.dto_last_error().decode(), (text, lib.dto_last_error())
        untouched()
    refused(solve(), INVALID, "dto_kkt_border_factor has not been called")
    refused(factor(), INVALID, "dto_kkt_assemble has not been called")
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc)
    refused(factor(), INVALID, "dto_kkt_factor has not been called")
    refused(solve(), INVALID, "dto_kkt_border_factor has not been called")
    s.kkt_factor()
    refused(solve(), INVALID, "dto_kkt_border_factor has not been called")
    refused(factor(n=0), INVALID, "nb < 1")
    refused(factor(n=17), UNSUPPORTED, "16 border rows")
    for kw in (dict(ldgx=nz - 1), dict(ldgc=nc - 1), dict(ldc=nb * nb - 1)):
        refused(factor(**kw), INVALID, "leading dimension too small")
    refused(factor(gx=0), INVALID, "null argument")
    refused(solve(), INVALID, "dto_kkt_border_factor has not been called")      # the refused calls left no border behind
    assert factor() == 0
    for kw in (dict(ldrx=nz - 1), dict(ldrc=nc - 1), dict(ldrb=nb - 1), dict(ldsx=nz - 1), dict(ldsc=nc - 1), dict(ldsb=nb - 1)):
        refused(solve(**kw), INVALID, "leading dimension too small")
    for kw in (dict(rb=0), dict(sb=0)):
        refused(solve(**kw), INVALID, "null argument")
    with pytest.raises(ValueError, match="overlap"):
        s.kkt_border_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, dRB.data_ptr(), nb, dRX.data_ptr(), nz, oC.data_ptr(), nc, oB.data_ptr(), nb)
    # a new factorisation, a new system and a call that takes the factor storage each invalidate the border
    s.kkt_factor()
    refused(solve(), INVALID, "dto_kkt_border_factor has not been called")
    assert factor() == 0
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc)
    refused(solve(), INVALID, "dto_kkt_border_factor has not been called")
    s.kkt_factor()
    assert factor() == 0
    dx = torch.full((B, nz), NAN, device="cuda", dtype=torch.float64)
    dl = torch.full((B, nc), NAN, device="cuda", dtype=torch.float64)
    assert s.kkt_step_batch(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc, dx.data_ptr(), nz, dl.data_ptr(), nc)
    refused(solve(), INVALID, "dto_kkt_border_factor has not been called")
    refused(factor(), INVALID, "dto_kkt_step_batch / the solver has used the factor storage since")
    s.kkt_factor()
    assert factor() == 0 and solve() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(oX).all()) and bool(torch.isfinite(oC).all()) and bool(torch.isfinite(oB).all())

"""The bordered matrix as an operator and refined bordered solves on the tile path: dto_kkt_border_multiply /
dto_kkt_border_solve_refined.

    M = [ K   G' ]      K as dto_kkt_multiply applies it (k_wide_kmul), G the panel kept by dto_kkt_border_factor,
        [ G  sym(C) ]   sym(C) = (C + C')/2; the border part is one pass over G (k_border_mul) plus k_border_mul_fin

dto_kkt_border_solve_refined: dto_kkt_border_solve, then passes of (rho, sigma) = (r, s) - M (v, y), a bordered solve of the
residual, the update; resid = max |(r, s) - M (v, y)| of what is returned.

Reference everywhere: the ORACLE's dense bordered matrix (oracle/padded_model.py: dense_kkt / embedded_dense_kkt plus the sigmas,
the helpers of tests/test_wide_border_gpu.py), products, residuals and magnitudes in np.longdouble on the host.

Bars.  Product: max |out - M v| <= 1e-8 max |M v| per instance (the project's bar); the componentwise figure
max_i |out - M v|_i / (|M||v|)_i is printed.  Symmetry: |u'(Mv) - v'(Mu)| <= (q + 1) 2^-53 |u|'|M||v|, the bound of a dot product
of length q in any summation order.  Refined solves, on passes = 2: omega = max_i |rhs - M sol|_i / (|M||sol| + |rhs|)_i <=
(q + 1) 2^-53 with q the largest number of nonzeros in a row of M, counted on M itself (border rows are dense in G, so q is at most
N + nb: 5e-14 at N = 451) -- the limiting componentwise backward error of fixed-precision refinement with working-precision residuals
(Skeel 1980; Higham, Accuracy and Stability of Numerical Algorithms, Theorem 12.3), the bar of
tests/test_wide_refined_solve_gpu.py, whose margin covers the last-bit differences between the generated derivative code and the
oracle's entries -- and forward error <= 1e-8 of max |solution| per instance.  Every bordered reference matrix is asserted to have
cond2 <= 1e4.  The tests print their figures before they assert; DESIGN.md section 4.3 holds the table of the first MI355X run.
"""
import os

import numpy as np
import pytest

from test_wide_border_gpu import CASES, _border, _border_factor, _border_solve, _bordered
from test_wide_linear_solver_gpu import _dev
from test_wide_multi_solve_gpu import _quasi_definite_system

pytestmark = pytest.mark.gpu

LD = np.longdouble
NAN = float("nan")
EPS_BAR = 2.0 ** -53


def _padded(a, ld):
    out = np.full((a.shape[0], ld), np.nan)
    out[:, :a.shape[1]] = a
    return out


def _outputs(B, lds):
    import torch
    return [torch.full((B, ld), NAN, device="cuda", dtype=torch.float64) for ld in lds]


def _collect(outs, lens):
    """The three output arrays on the host, their padding checked (it must still be NaN), as one [B][nz + nc + nb] array."""
    import torch
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h, n in zip(host, lens):
        assert np.all(np.isnan(h[:, n:])), "output padding was written"
    return np.concatenate([h[:, :n] for h, n in zip(host, lens)], axis=1)


def _border_multiply(s, V, nz, nc, lds=None):
    """V [B][nz + nc + nb] -> M V, same shape.  Inputs padded with NaN, outputs NaN everywhere before the call."""
    B, nb = V.shape[0], V.shape[1] - nz - nc
    ldvx, ldvc, ldvb, ldox, ldoc, ldob = lds or (nz, nc, nb, nz, nc, nb)
    dx, dc, db = _dev(_padded(V[:, :nz], ldvx)), _dev(_padded(V[:, nz:nz + nc], ldvc)), _dev(_padded(V[:, nz + nc:], ldvb))
    outs = _outputs(B, (ldox, ldoc, ldob))
    s.kkt_border_multiply(dx.data_ptr(), ldvx, dc.data_ptr(), ldvc, db.data_ptr(), ldvb, outs[0].data_ptr(), ldox, outs[1].data_ptr(), ldoc,
                          outs[2].data_ptr(), ldob)
    return _collect(outs, (nz, nc, nb))


def _border_refined(s, R, nz, nc, passes, resid=False, lds=None):
    """R [B][nz + nc + nb] -> the refined solution, same shape (and resid [B])."""
    import torch
    B, nb = R.shape[0], R.shape[1] - nz - nc
    ldrx, ldrc, ldrb, ldsx, ldsc, ldsb = lds or (nz, nc, nb, nz, nc, nb)
    dx, dc, db = _dev(_padded(R[:, :nz], ldrx)), _dev(_padded(R[:, nz:nz + nc], ldrc)), _dev(_padded(R[:, nz + nc:], ldrb))
    outs = _outputs(B, (ldsx, ldsc, ldsb))
    rs = torch.full((B,), NAN, device="cuda", dtype=torch.float64)
    s.kkt_border_solve_refined(dx.data_ptr(), ldrx, dc.data_ptr(), ldrc, db.data_ptr(), ldrb, outs[0].data_ptr(), ldsx, outs[1].data_ptr(),
                               ldsc, outs[2].data_ptr(), ldsb, passes, resid_ptr=rs.data_ptr() if resid else 0)
    sol = _collect(outs, (nz, nc, nb))
    return (sol, rs.cpu().numpy()) if resid else sol


def _q(M):
    return int(np.max(np.sum(M != 0.0, axis=1)))


def _check_product(out, Ms, V, what):
    worst = 0.0
    for b, M in enumerate(Ms):
        ML, vL = M.astype(LD), V[b].astype(LD)
        ref, mag = ML @ vL, np.abs(ML) @ np.abs(vL)
        assert np.all(np.isfinite(out[b])), (what, b)
        err = np.abs(out[b].astype(LD) - ref)
        nrm = float(np.max(err)) / float(np.max(np.abs(ref)))
        pos = mag > 0                                       # (rows with an empty product: covered by the norm-wise bar alone)
        cw = float(np.max(err[pos] / mag[pos]))
        worst = max(worst, cw)
        print(f"  {what} instance {b}: max|out - Mv| / max|Mv| = {nrm:.2e}, componentwise max |out - Mv|_i / (|M||v|)_i = {cw:.2e}")
        assert nrm <= 1e-8, (what, b, nrm)
    return worst


def _omega(M, sol, rhs):
    ML, xL, rL = M.astype(LD), sol.astype(LD), rhs.astype(LD)
    return float(np.max(np.abs(rL - ML @ xL) / (np.abs(ML) @ np.abs(xL) + np.abs(rL))))


def _dense_solution(M, rhs):
    """numpy's LU plus one refinement step with the residual in np.longdouble."""
    x = np.linalg.solve(M, rhs)
    return x + np.linalg.solve(M, (rhs.astype(LD) - M.astype(LD) @ x.astype(LD)).astype(np.float64))


def _check_refined(sols, Ms, R, what, only=None):
    """sols: {passes: [B][n]}; every figure printed, omega and the forward error asserted on the largest number of passes."""
    last = max(sols)
    for b, M in enumerate(Ms):
        if only is not None and not only[b]:
            continue
        bar, ref = (_q(M) + 1) * EPS_BAR, _dense_solution(M, R[b])
        om = {k: _omega(M, v[b], R[b]) for k, v in sols.items()}
        fe = {k: float(np.max(np.abs(v[b] - ref)) / np.max(np.abs(ref))) for k, v in sols.items()}
        print(f"  {what} instance {b}: q = {_q(M)}, bar {bar:.2e}, omega " + " / ".join(f"passes {k}: {om[k]:.2e}" for k in sorted(om)) +
              ", forward error " + " / ".join(f"{fe[k]:.2e}" for k in sorted(fe)))
        assert np.all(np.isfinite(sols[last][b])), (what, b)
        assert om[last] <= bar, (what, b, om, bar)
        assert fe[last] <= 1e-8, (what, b, fe)


@pytest.mark.parametrize("m,T,B,dw,nb,use_gc,ckind", CASES)
def test_border_product_matches_the_oracle(m, T, B, dw, nb, use_gc, ckind):
    """Random vectors and columns of M (a unit vector at an x_t entry, at a lam_t entry, at a border entry: a wrong block shows as a
    wrong column), the symmetry of the operator, and a non-symmetric C against its symmetric part (bit for bit: the halves are
    exact)."""
    s, Ks, rng, nz, nc = _quasi_definite_system(m, T, B, dw, 5 + T if m == 1 else 50 + m)
    N = nz + nc
    G, C = _border(rng, B, nb, nz, nc, use_gc, ckind)
    _border_factor(s, G, C, nz, nc, use_gc)
    Ms = [_bordered(Ks[b], G[b], None if C is None else C[b]) for b in range(B)]
    t = (T - 1) // 2
    worst = 0.0
    U, V = rng.standard_normal((B, N + nb)), rng.standard_normal((B, N + nb))
    MU_, MV = _border_multiply(s, U, nz, nc), _border_multiply(s, V, nz, nc)
    worst = max(worst, _check_product(MV, Ms, V, "random"))
    for what, i in (("unit x_t", t * (64 + m) + 5), ("unit lam_t", nz + t * 64 + 2), ("unit border", N + nb - 1)):
        E = np.zeros((B, N + nb))
        E[:, i] = 1.0
        worst = max(worst, _check_product(_border_multiply(s, E, nz, nc), Ms, E, what))
    for b, M in enumerate(Ms):
        lhs = abs(float(U[b].astype(LD) @ MV[b].astype(LD) - V[b].astype(LD) @ MU_[b].astype(LD)))
        bound = (_q(M) + 1) * EPS_BAR * float(np.abs(U[b]).astype(LD) @ (np.abs(M).astype(LD) @ np.abs(V[b]).astype(LD)))
        print(f"  instance {b}: q = {_q(M)}, |u'Mv - v'Mu| = {lhs:.2e}, bound {bound:.2e}")
        assert lhs <= bound, (b, lhs, bound)
    if ckind == "nonsymmetric":
        _border_factor(s, G, 0.5 * (C + C.transpose(0, 2, 1)), nz, nc, use_gc)
        assert np.array_equal(MV, _border_multiply(s, V, nz, nc)), "a non-symmetric C must give what its symmetric part gives"
    print(f"  m={m} T={T} B={B} nb={nb} g_c={use_gc} C={ckind}: worst componentwise figure {worst:.2e}")


def test_border_refined_zero_passes_is_the_border_solve():
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, 2, 2.0, 9)
    nb = 5
    G, C = _border(rng, 2, nb, nz, nc, True, "symmetric")
    _border_factor(s, G, C, nz, nc, True)
    R = rng.standard_normal((2, nz + nc + nb))
    plain = _border_solve(s, R[:, :nz + nc], R[:, nz + nc:], nz, nc)
    assert np.all(np.isfinite(plain)) and np.array_equal(plain, _border_refined(s, R, nz, nc, 0))


@pytest.mark.parametrize("m,T,seed,nb,use_gc,ckind", [(1, 4, 9, 16, True, "negdiag"), (3, 3, 53, 12, False, "symmetric")])
def test_border_refined_backward_and_forward_error(m, T, seed, nb, use_gc, ckind):
    s, Ks, rng, nz, nc = _quasi_definite_system(m, T, 2, 2.0, seed)
    G, C = _border(rng, 2, nb, nz, nc, use_gc, ckind)
    _border_factor(s, G, C, nz, nc, use_gc)
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(2)]
    R = rng.standard_normal((2, nz + nc + nb))
    _check_refined({k: _border_refined(s, R, nz, nc, k) for k in (0, 1, 2)}, Ms, R, f"(m, T) = ({m}, {T}), nb = {nb}")


def _indefinite():
    """The indefinite family of tests/test_wide_refined_solve_gpu.py (delta_w = 0: the single factorisation attempt runs to the end
    with a wrong inertia, K^-1 is the unpivoted one) with a border of five rows."""
    import test_wide_refined_solve_gpu as W
    c = W._system("indefinite")
    s = W._solver(c["m"], c["T"])
    nz, nc, B, nb = c["nz"], c["nc"], c["B"], 5
    assert all(c["usable"]), ("every instance must be used", c["usable"])
    ok, neg = W._assemble_factor(s, c)
    print(f"  indefinite: inertia_ok {ok.tolist()}, negative pivots {neg.tolist()} of {nc}")
    assert any(int(n) != nc for n in neg), "the family must hold a factorisation of wrong inertia"
    rng = np.random.default_rng(171)
    G, C = _border(rng, B, nb, nz, nc, True, "symmetric")
    _, singular = _border_factor(s, G, C, nz, nc, True)
    assert not np.any(singular)
    Ms = [_bordered(c["Ks"][b], G[b], C[b]) for b in range(B)]      # (asserts cond2 <= 1e4)
    return s, Ms, rng, nz, nc, nb, B


def test_border_refined_on_the_indefinite_family():
    s, Ms, rng, nz, nc, nb, B = _indefinite()
    R = rng.standard_normal((B, nz + nc + nb))
    _check_refined({k: _border_refined(s, R, nz, nc, k) for k in (0, 1, 2)}, Ms, R, "indefinite, nb = 5")


def test_border_refined_residual_norm():
    """resid against dto_kkt_border_multiply and the same subtraction on the host (bit for bit) and against the oracle's
    residual; asking for it does not change the solution."""
    s, Ms, rng, nz, nc, nb, B = _indefinite()
    R = rng.standard_normal((B, nz + nc + nb))
    for passes in (0, 2):
        sol, rs = _border_refined(s, R, nz, nc, passes, resid=True)
        assert np.array_equal(sol, _border_refined(s, R, nz, nc, passes)), "asking for the norm must not change the solution"
        mine = np.max(np.abs(R - _border_multiply(s, sol, nz, nc)), axis=1)
        print(f"  passes {passes}: resid {rs.tolist()}")
        assert np.array_equal(rs, mine), (passes, rs, mine)
        for b in range(B):
            host = float(np.max(np.abs(R[b].astype(LD) - Ms[b].astype(LD) @ sol[b].astype(LD))))
            assert abs(rs[b] - host) <= 1e-8 * np.max(np.abs(R[b])), (passes, b, rs[b], host)


def test_border_product_and_refined_chunking():
    """DTO_BORDER_GRAM_CHUNK = 64 at factor time (rounded up to the slab of 128: four chunks of the 451 entries of a row, the last
    one 67 long), a value above N (one chunk) and the default: the product and the refined solve use the chunks of the factor
    call, stay within the bars, and two runs with one setting are bit-identical."""
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, 2, 2.0, 9)
    nb = 16
    assert nz + nc == 451
    G, C = _border(rng, 2, nb, nz, nc, True, "negdiag")
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(2)]
    V, R = rng.standard_normal((2, nz + nc + nb)), rng.standard_normal((2, nz + nc + nb))
    saved = os.environ.pop("DTO_BORDER_GRAM_CHUNK", None)
    try:
        for setting in ("64", "100000", None):
            if setting is not None:
                os.environ["DTO_BORDER_GRAM_CHUNK"] = setting
            runs = []
            for _ in range(2):
                _border_factor(s, G, C, nz, nc, True)
                os.environ.pop("DTO_BORDER_GRAM_CHUNK", None)      # the later calls use what the factor call used
                runs.append((_border_multiply(s, V, nz, nc), _border_refined(s, R, nz, nc, 2)))
                if setting is not None:
                    os.environ["DTO_BORDER_GRAM_CHUNK"] = setting
            os.environ.pop("DTO_BORDER_GRAM_CHUNK", None)
            assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), setting
            _check_product(runs[0][0], Ms, V, f"chunk {setting}")
            _check_refined({2: runs[0][1]}, Ms, R, f"chunk {setting}")
    finally:
        if saved is not None:
            os.environ["DTO_BORDER_GRAM_CHUNK"] = saved


def test_border_product_and_refined_padded_leading_dimensions():
    """The six leading dimensions of the product and the six of the refined solve all above their row lengths and all twelve
    different (the border was factorised from padded arrays too), NaN in every input padding entry, outputs pre-filled with NaN:
    bit for bit the tight calls, output padding still NaN (checked by _collect)."""
    s, Ks, rng, nz, nc = _quasi_definite_system(3, 3, 2, 2.0, 53)
    nb = 12
    G, C = _border(rng, 2, nb, nz, nc, True, "nonsymmetric")
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(2)]
    V, R = rng.standard_normal((2, nz + nc + nb)), rng.standard_normal((2, nz + nc + nb))
    _border_factor(s, G, C, nz, nc, True, lds=(nz + 5, nc + 3, nb * nb + 7))
    tight = _border_multiply(s, V, nz, nc), _border_refined(s, R, nz, nc, 2, resid=True)
    wide = (_border_multiply(s, V, nz, nc, lds=(nz + 1, nc + 2, nb + 3, nz + 4, nc + 5, nb + 6)),
            _border_refined(s, R, nz, nc, 2, resid=True, lds=(nz + 7, nc + 8, nb + 9, nz + 10, nc + 11, nb + 12)))
    assert np.all(np.isfinite(tight[0])) and np.array_equal(tight[0], wide[0])
    assert np.all(np.isfinite(tight[1][0])) and np.array_equal(tight[1][0], wide[1][0]) and np.array_equal(tight[1][1], wide[1][1])
    _check_product(wide[0], Ms, V, "padded")
    _check_refined({2: wide[1][0]}, Ms, R, "padded")


def test_border_refined_singular_instance():
    """The zero-row case of tests/test_wide_border_gpu.py: instance 0 has a singular Schur complement -- NaN in every entry of its
    refined solution and in its resid, instance 1 within the bars; the product needs no S and stays finite for both."""
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, 2, 2.0, 9)
    nb = 2
    G, _ = _border(rng, 2, nb, nz, nc, True, None)
    G[0, 1] = 0.0
    C = np.zeros((2, nb, nb))
    C[1] = -np.diag(1e-5 + rng.random(nb))
    negdef, singular = _border_factor(s, G, C, nz, nc, True)
    assert singular.tolist() == [1, 0], singular
    Ms = [np.block([[Ks[0], G[0].T], [G[0], C[0]]]), _bordered(Ks[1], G[1], C[1])]
    R, V = rng.standard_normal((2, nz + nc + nb)), rng.standard_normal((2, nz + nc + nb))
    for passes in (0, 2):
        sol, rs = _border_refined(s, R, nz, nc, passes, resid=True)
        assert np.all(np.isnan(sol[0])) and np.isnan(rs[0]), "a singular instance returns NaN in every entry and in resid"
        assert np.isfinite(rs[1])
        if passes == 2:
            _check_refined({2: sol}, Ms, R, "next to a singular instance", only=[False, True])
    _check_product(_border_multiply(s, V, nz, nc), Ms, V, "with a singular Schur complement in instance 0")


def test_border_product_and_refined_interleave_with_the_other_stored_factor_calls():
    """dto_kkt_solve, dto_kkt_solve_multi(3), dto_kkt_multiply, dto_kkt_solve_refined(2) and a plain dto_kkt_border_solve before,
    between and after product and refined calls: bit-identical every time."""
    from test_wide_kmul_gpu import _multiply
    from test_wide_linear_solver_gpu import _solve
    from test_wide_multi_solve_gpu import _solve_multi
    from test_wide_refined_solve_gpu import _refined
    B, nb = 2, 5
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, B, 2.0, 21)
    R = rng.standard_normal((B, nz + nc))
    MX, MC = rng.standard_normal((B, 3, nz)), rng.standard_normal((B, 3, nc))
    RB = rng.standard_normal((B, nz + nc + nb))
    G, C = _border(rng, B, nb, nz, nc, True, "symmetric")
    Ms = [_bordered(Ks[b], G[b], C[b]) for b in range(B)]
    _border_factor(s, G, C, nz, nc, True)

    def others():
        a = _solve(s, np.ascontiguousarray(R[:, :nz]), np.ascontiguousarray(R[:, nz:]))
        b_ = _solve_multi(s, MX, MC)
        return [a[0], a[1], b_[0], b_[1], _multiply(s, R, nz, nc), _refined(s, R, nz, nc, 2),
                _border_solve(s, RB[:, :nz + nc], RB[:, nz + nc:], nz, nc)]
    before = others()
    p1 = _border_multiply(s, RB, nz, nc)
    between = others()
    r1 = _border_refined(s, RB, nz, nc, 2, resid=True)
    middle = others()
    p2, r2 = _border_multiply(s, RB, nz, nc), _border_refined(s, RB, nz, nc, 2, resid=True)
    after = others()
    for other in (between, middle, after):
        for x, y in zip(before, other):
            assert np.all(np.isfinite(x)) and np.array_equal(x, y)
    assert np.array_equal(p1, p2) and np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    _check_product(p1, Ms, RB, "interleaved")
    _check_refined({2: r1[0]}, Ms, RB, "interleaved")


def test_border_product_and_refined_on_an_embedded_problem():
    """The 24-state problem with stage rows of tests/test_wide_embedded_linear_gpu.py (T = 5) in the solver's layout, nb = 3,
    against embedded_dense_kkt."""
    import test_wide_embedded_linear_gpu as E
    s, c = E._solver("rows5"), E._system("rows5")
    nz, nc, nb = c["nz"], c["nc"], 3
    E._assemble(s, c)
    E._factor(s, nc)
    rng = np.random.default_rng(62)
    G, C = _border(rng, E.B, nb, nz, nc, True, "symmetric")
    _, singular = _border_factor(s, G, C, nz, nc, True)
    assert not np.any(singular)
    Ms = [_bordered(c["Ks"][b], G[b], C[b]) for b in range(E.B)]
    V, R = rng.standard_normal((E.B, nz + nc + nb)), rng.standard_normal((E.B, nz + nc + nb))
    _check_product(_border_multiply(s, V, nz, nc), Ms, V, "rows5")
    _check_refined({k: _border_refined(s, R, nz, nc, k) for k in (0, 2)}, Ms, R, "rows5")


def test_border_product_and_refined_misuse():
    """The state machine of include/dto.h call by call: error code, message fragment, and outputs that are still all NaN."""
    import torch
    import dto_amd
    from dto_amd import problems as P
    T, B, dw, dc, nb = 3, 2, 2.0, 1e-5, 2
    p = P.build_acrobot_padded(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(13)
    dZ, dMU = _dev(rng.random((B, nz))), _dev(rng.random((B, nc)))
    dGX, dGC = _dev(rng.standard_normal((B * nb, nz))), _dev(rng.standard_normal((B * nb, nc)))
    dCC = _dev(-np.tile(np.eye(nb).reshape(1, nb * nb), (B, 1)))
    dRX, dRC, dRB = _dev(rng.standard_normal((B, nz))), _dev(rng.standard_normal((B, nc))), _dev(rng.standard_normal((B, nb)))
    oX, oC, oB = (torch.full((B, n), NAN, device="cuda", dtype=torch.float64) for n in (nz, nc, nb))
    oR = torch.full((B,), NAN, device="cuda", dtype=torch.float64)
    lib, h = s._solve_nlp._lib, s._solve_nlp._h
    s._B = B
    INVALID = 1
    FULL = dict(ldix=nz, ldic=nc, ldib=nb, ldox=nz, ldoc=nc, ldob=nb)

    def untouched():
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in (oX, oC, oB, oR)), "a refused call wrote"

    def factor():
        return lib.dto_kkt_border_factor(h, nb, dGX.data_ptr(), nz, dGC.data_ptr(), nc, dCC.data_ptr(), nb * nb, None, None, None)

    def multiply(ib=None, ob=None, **ld):
        a = dict(FULL, **ld)
        return lib.dto_kkt_border_multiply(h, dRX.data_ptr(), a["ldix"], dRC.data_ptr(), a["ldic"], dRB.data_ptr() if ib is None else ib, a["ldib"],
                                           oX.data_ptr(), a["ldox"], oC.data_ptr(), a["ldoc"], oB.data_ptr() if ob is None else ob, a["ldob"], None)

    def refined(passes=2, ib=None, ob=None, **ld):
        a = dict(FULL, **ld)
        return lib.dto_kkt_border_solve_refined(h, passes, dRX.data_ptr(), a["ldix"], dRC.data_ptr(), a["ldic"],
                                                dRB.data_ptr() if ib is None else ib, a["ldib"], oX.data_ptr(), a["ldox"], oC.data_ptr(), a["ldoc"],
                                                oB.data_ptr() if ob is None else ob, a["ldob"], oR.data_ptr(), None)

    def refused(rc, text):
        assert rc == INVALID, (rc, lib.dto_last_error())
        assert text in lib.dto_last_error().decode(), (text, lib.dto_last_error())
        untouched()

    def no_border():
        for call in (multiply, refined):
            refused(call(), "dto_kkt_border_factor has not been called")
    no_border()                                                             # before dto_kkt_assemble
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc)
    no_border()                                                             # before dto_kkt_factor
    s.kkt_factor()
    no_border()                                                             # before dto_kkt_border_factor
    assert factor() == 0
    refused(refined(passes=-1), "passes outside 0..4")
    refused(refined(passes=5), "passes outside 0..4")
    for call in (multiply, refined):
        for name, n in FULL.items():
            refused(call(**{name: n - 1}), "leading dimension too small")
        for kw in (dict(ib=0), dict(ob=0)):
            refused(call(**kw), "null argument")
    with pytest.raises(ValueError, match="overlap"):
        s.kkt_border_multiply(dRX.data_ptr(), nz, dRC.data_ptr(), nc, dRB.data_ptr(), nb, oX.data_ptr(), nz, oC.data_ptr(), nc, dRB.data_ptr(), nb)
    with pytest.raises(ValueError, match="overlap"):
        s.kkt_border_solve_refined(dRX.data_ptr(), nz, dRC.data_ptr(), nc, dRB.data_ptr(), nb, dRX.data_ptr(), nz, oC.data_ptr(), nc,
                                   oB.data_ptr(), nb, 2)
    untouched()
    # a new factorisation, a new system and a call that takes the factor storage each invalidate the border
    s.kkt_factor()
    no_border()
    assert factor() == 0
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc)
    no_border()
    s.kkt_factor()
    assert factor() == 0
    dx = torch.full((B, nz), NAN, device="cuda", dtype=torch.float64)
    dl = torch.full((B, nc), NAN, device="cuda", dtype=torch.float64)
    assert s.kkt_step_batch(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc, dx.data_ptr(), nz, dl.data_ptr(), nc)
    no_border()
    s.kkt_factor()
    assert factor() == 0 and multiply() == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in (oX, oC, oB))
    for o in (oX, oC, oB):
        o.fill_(NAN)
    assert refined() == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in (oX, oC, oB, oR))

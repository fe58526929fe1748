"""dto_kkt_solve_refined on the tile path: dto_kkt_solve plus passes of r = rhs - K sol, d = K^-1 r, sol += d against the stored
factor (k_wide_kmul for the residual, k_wide_fsub + k_wide_bwd for the correction).

Reference: the ORACLE's dense matrix (oracle/padded_model.py: dense_kkt, plus diag([sigma_x; -sigma_c])), residuals and
magnitudes in np.longdouble on the host.

Bars.  Backward error after two passes: omega = max_i |rhs - K sol|_i / (|K||sol| + |rhs|)_i <= (q + 1) 2^-53 (1.6e-14 at
q = 142, the largest number of nonzeros in a row of K): the limiting componentwise backward error of fixed-precision refinement
with working-precision residuals (Skeel 1980; Higham, Accuracy and Stability of Numerical Algorithms, Theorem 12.3).  The
reference itself -- numpy's LU plus one float64 refinement step -- gives 2.9e-16 .. 6.2e-16 on these systems, so the bar sits
about 25 times above it, which leaves room for the last-bit differences between the generated derivative code and the oracle's
entries.  Forward error after two passes: the project's 1e-8 of max |solution| for every instance, the
indefinite ones included (condition numbers <= 3.4e3 times the omega bar is 5e-11).

test_refined_backward_and_forward_error prints omega and the forward error for passes = 0 / 1 / 2 before it asserts; DESIGN.md
section 4.3 holds the table of the first MI355X run.
"""
import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu

LD = np.longdouble
INDEFINITE_SEED = 99   # the seed of tests/test_wide_linear_solver_gpu.py: all four matrices have min |eig| > 1e-6


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


_MODELS, _SYSTEMS = {}, {}


def _dense(m, T, z, mu, dw, dc, sx=None, sc=None):
    from oracle.padded_model import PaddedAcrobot, dense_kkt
    if m not in _MODELS:
        _MODELS[m] = PaddedAcrobot(64, m)
    K, _ = dense_kkt(_MODELS[m], T, z, mu, dw, dc)
    if sx is not None:
        K = K + np.diag(np.concatenate([sx, -sc]))
    return K


def _system(name):
    """The systems of the backward / forward error tests, built once: the quasi-definite points of
    tests/test_wide_linear_solver_gpu.py and its indefinite family (delta_w = 0, multipliers 40 (U - 1/2))."""
    if name not in _SYSTEMS:
        m, T, B, dw, sig, seed = {"qd_1_4": (1, 4, 2, 2.0, False, 404), "qd_3_5": (3, 5, 3, 2.0, True, 53),
                                  "qd_1_9": (1, 9, 2, 30.0, True, 14), "indefinite": (1, 4, 4, 0.0, False, INDEFINITE_SEED)}[name]
        nz, nc = (T - 1) * (64 + m) + 64, (T - 1) * 64
        rng = np.random.default_rng(seed)
        Z = rng.random((B, nz))
        MU = 40.0 * (rng.random((B, nc)) - 0.5) if name == "indefinite" else rng.random((B, nc))
        SX = SC = None
        if sig:
            SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
            SX[:, ::3] = 0.0
        dc = 1e-5
        Ks = [_dense(m, T, Z[b], MU[b], dw, dc, None if SX is None else SX[b], None if SC is None else SC[b]) for b in range(B)]
        R = rng.standard_normal((B, nz + nc))
        eigs = [np.linalg.eigvalsh(K) for K in Ks]
        usable = [bool(np.min(np.abs(e)) > 1e-6) for e in eigs]
        dense = [np.linalg.solve(Ks[b], R[b]) for b in range(B)]
        _SYSTEMS[name] = dict(m=m, T=T, B=B, dw=dw, dc=dc, nz=nz, nc=nc, Z=Z, MU=MU, SX=SX, SC=SC, Ks=Ks, R=R, eigs=eigs,
                              usable=usable, dense=dense)
    return _SYSTEMS[name]


def _assemble_factor(s, c):
    nz, nc = c["nz"], c["nc"]
    keep = [_dev(c["Z"]), _dev(c["MU"])]
    kw = {}
    if c["SX"] is not None:
        keep += [_dev(c["SX"]), _dev(c["SC"])]
        kw.update(sigma_x_ptr=keep[2].data_ptr(), ldsx=nz, sigma_c_ptr=keep[3].data_ptr(), ldsc=nc)
    s.kkt_assemble(keep[0].data_ptr(), c["B"], nz, keep[1].data_ptr(), nc, c["dw"], c["dc"], **kw)
    return s.kkt_factor()


def _refined(s, R, nz, nc, passes, resid=False):
    import torch
    B = R.shape[0]
    dRX, dRC = _dev(R[:, :nz]), _dev(R[:, nz:])
    oX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    rs = torch.full((B,), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_solve_refined(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc, passes,
                        resid_ptr=rs.data_ptr() if resid else 0)
    torch.cuda.synchronize()
    sol = np.concatenate([oX.cpu().numpy(), oC.cpu().numpy()], axis=1)
    return (sol, rs.cpu().numpy()) if resid else sol


def _plain(s, R, nz, nc):
    import torch
    B = R.shape[0]
    dRX, dRC = _dev(R[:, :nz]), _dev(R[:, nz:])
    oX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
    torch.cuda.synchronize()
    return np.concatenate([oX.cpu().numpy(), oC.cpu().numpy()], axis=1)


def _omega(K, sol, rhs):
    KL, xL, rL = K.astype(LD), sol.astype(LD), rhs.astype(LD)
    return float(np.max(np.abs(rL - KL @ xL) / (np.abs(KL) @ np.abs(xL) + np.abs(rL))))


def test_refined_zero_passes_is_the_plain_solve():
    c = _system("qd_1_4")
    s = _solver(c["m"], c["T"])
    _assemble_factor(s, c)
    a, b_ = _plain(s, c["R"], c["nz"], c["nc"]), _refined(s, c["R"], c["nz"], c["nc"], 0)
    assert np.all(np.isfinite(a)) and np.array_equal(a, b_)


@pytest.mark.parametrize("name", ["qd_1_4", "qd_3_5", "qd_1_9", "indefinite"])
def test_refined_backward_and_forward_error(name):
    """omega for passes = 0, 1, 2 (printed), the bar on passes = 2; forward error of passes = 2 against the dense solve."""
    c = _system(name)
    s = _solver(c["m"], c["T"])
    nz, nc, B = c["nz"], c["nc"], c["B"]
    if name == "indefinite":
        assert sum(c["usable"]) >= 3, ("vacuous: pick another seed", c["usable"])
        assert any(int(np.sum(e < 0)) != nc for e in c["eigs"]), "the family must hold a matrix of wrong inertia"
    ok, neg = _assemble_factor(s, c)
    print(f"  {name}: inertia_ok {ok.tolist()}, negative pivots {neg.tolist()} of {nc}")
    sols = [_refined(s, c["R"], nz, nc, k) for k in (0, 1, 2)]
    for b in range(B):
        if not c["usable"][b]:
            continue
        K = c["Ks"][b]
        q = int(np.max(np.sum(K != 0.0, axis=1)))
        om = [_omega(K, sols[k][b], c["R"][b]) for k in range(3)]
        scale = np.max(np.abs(c["dense"][b]))
        fe = [float(np.max(np.abs(sols[k][b] - c["dense"][b])) / scale) for k in range(3)]
        cond = float(np.max(np.abs(c["eigs"][b])) / np.min(np.abs(c["eigs"][b])))
        print(f"  {name} instance {b}: q = {q}, cond2 = {cond:.2e}, omega passes 0/1/2 = {om[0]:.2e} / {om[1]:.2e} / {om[2]:.2e}, "
              f"forward error 0/1/2 = {fe[0]:.2e} / {fe[1]:.2e} / {fe[2]:.2e}, bar {(q + 1) * 2.0 ** -53:.2e}")
        assert om[2] <= (q + 1) * 2.0 ** -53, (name, b, om, q)
        assert fe[2] <= 1e-8, (name, b, fe)


def test_refined_padded_leading_dimensions():
    """kkt_solve_refined(passes=2) with four different leading dimensions above the row lengths: NaN in every padding entry of the
    right-hand side, NaN-filled outputs whose padding must stay NaN (the passes read the right-hand side again and update the
    solution in place, each with the caller's strides).  Bit-identical to the tight call, within 1e-8 of the dense solve."""
    import torch
    c = _system("qd_3_5")
    s = _solver(c["m"], c["T"])
    nz, nc, B = c["nz"], c["nc"], c["B"]
    _assemble_factor(s, c)
    tight = _refined(s, c["R"], nz, nc, 2)
    ldrx, ldrc, ldsx, ldsc = nz + 5, nc + 3, nz + 7, nc + 2
    hX, hC = np.full((B, ldrx), np.nan), np.full((B, ldrc), np.nan)
    hX[:, :nz], hC[:, :nc] = c["R"][:, :nz], c["R"][:, nz:]
    dRX, dRC = _dev(hX), _dev(hC)
    oX = torch.full((B, ldsx), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B, ldsc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_solve_refined(dRX.data_ptr(), ldrx, dRC.data_ptr(), ldrc, oX.data_ptr(), ldsx, oC.data_ptr(), ldsc, 2)
    torch.cuda.synchronize()
    oX, oC = oX.cpu().numpy(), oC.cpu().numpy()
    assert np.all(np.isnan(oX[:, nz:])) and np.all(np.isnan(oC[:, nc:])), "the padding of the outputs must stay untouched"
    sol = np.concatenate([oX[:, :nz], oC[:, :nc]], axis=1)
    assert np.all(np.isfinite(tight)) and np.array_equal(sol, tight)
    for b in range(B):
        scale = np.max(np.abs(c["dense"][b]))
        fe = float(np.max(np.abs(sol[b] - c["dense"][b])) / scale)
        print(f"  instance {b}: forward error {fe:.2e}")
        assert fe <= 1e-8, (b, fe)


def test_refined_residual_norm():
    """resid = max |rhs - K sol| of the returned solution: the oracle's K on the host to 1e-8 of max |rhs|, and dto_kkt_multiply
    followed by the same subtraction on the host bit for bit."""
    import torch
    c = _system("indefinite")
    s = _solver(c["m"], c["T"])
    nz, nc, B = c["nz"], c["nc"], c["B"]
    _assemble_factor(s, c)
    for passes in (0, 2):
        sol, rs = _refined(s, c["R"], nz, nc, passes, resid=True)
        assert np.array_equal(sol, _refined(s, c["R"], nz, nc, passes)), "asking for the norm must not change the solution"
        dVX, dVC = _dev(sol[:, :nz]), _dev(sol[:, nz:])
        kX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
        kC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
        s.kkt_multiply(dVX.data_ptr(), nz, dVC.data_ptr(), nc, kX.data_ptr(), nz, kC.data_ptr(), nc)
        torch.cuda.synchronize()
        Kx = np.concatenate([kX.cpu().numpy(), kC.cpu().numpy()], axis=1)
        mine = np.max(np.abs(c["R"] - Kx), axis=1)
        print(f"  passes {passes}: resid {rs.tolist()}")
        assert np.array_equal(rs, mine), (passes, rs, mine)
        for b in range(B):
            host = float(np.max(np.abs(c["R"][b].astype(LD) - c["Ks"][b].astype(LD) @ sol[b].astype(LD))))
            assert abs(rs[b] - host) <= 1e-8 * np.max(np.abs(c["R"][b])), (passes, b, rs[b], host)


def test_refined_misuse():
    """The state machine and the argument checks of dto_kkt_solve, plus the range of passes: all DTO_ERR_INVALID (1)."""
    import torch
    import dto_amd
    from dto_amd import capi, problems as P
    T, B, dw, dc = 3, 2, 2.0, 1e-5
    p = P.build_acrobot_padded(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(12)
    dZ, dMU = _dev(rng.random((B, nz))), _dev(rng.random((B, nc)))
    R = rng.standard_normal((B, nz + nc))
    dRX, dRC = _dev(R[:, :nz]), _dev(R[:, nz:])
    oX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    lib, h = s._solve_nlp._lib, s._solve_nlp._h

    def raw(passes=1, rx=None, ldrx=nz, rc=None, ldrc=nc, sx=None, ldsx=nz, sc=None, ldsc=nc):
        ptr = lambda given, default: default.data_ptr() if given is None else given   # noqa: E731
        return lib.dto_kkt_solve_refined(h, passes, ptr(rx, dRX), ldrx, ptr(rc, dRC), ldrc, ptr(sx, oX), ldsx, ptr(sc, oC), ldsc, None, None)

    def invalid(rc, text):
        assert rc == 1, rc
        assert text in lib.dto_last_error().decode(), (text, lib.dto_last_error())
    invalid(raw(), "dto_kkt_assemble has not been called")
    with pytest.raises(capi.DtoError, match="dto_kkt_assemble has not been called"):
        s.kkt_multiply(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc)
    invalid(raw(), "dto_kkt_factor has not been called")
    s.kkt_factor()
    assert raw() == 0
    invalid(raw(passes=-1), "passes")
    invalid(raw(passes=5), "passes")
    for kw in (dict(ldrx=nz - 1), dict(ldrc=nc - 1), dict(ldsx=nz - 1), dict(ldsc=nc - 1)):
        invalid(raw(**kw), "leading dimension too small")
    for kw in (dict(rx=0), dict(rc=0), dict(sx=0), dict(sc=0)):
        invalid(raw(**kw), "null argument")
    # the same checks on the product
    assert lib.dto_kkt_multiply(h, dRX.data_ptr(), nz - 1, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc, None) == 1
    assert lib.dto_kkt_multiply(h, dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, None, nc, None) == 1
    # dto_kkt_step_batch takes the records: the refined solve is refused, the product (which needs none) still works
    dx = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    dl = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    assert s.kkt_step_batch(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc, dx.data_ptr(), nz, dl.data_ptr(), nc)
    invalid(raw(), "dto_kkt_factor has not been called")
    s.kkt_multiply(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
    torch.cuda.synchronize()
    assert np.all(np.isfinite(oX.cpu().numpy())) and np.all(np.isfinite(oC.cpu().numpy()))

"""dto_kkt_assemble_first_order on the tile path: the system of dto_kkt_assemble with W = 0,
    K0 = [[diag(sigma_x) + delta_w I, J'], [J, -diag(sigma_c) - delta_c I]],
assembled by k_wide_step's linear-solver mode and applied by k_wide_kmul with dto_wide_args.first_order set.

Reference: numpy on oracle/padded_model.py -- dense_derivatives gives J, K0 is put together here, products in np.longdouble.
Bars: the project's 1e-8 of the largest entry of the reference product (tests/test_wide_kmul_gpu.py) and, for
factor + solve, max |K0 x - r| <= 1e-8 max |r| (the 1e-8 of tests/test_wide_linear_solver_gpu.py).  B = 3; one action at T = 2, 3
and 9 (a chunk edge of k_wide_kmul: 8 stages per workgroup), three actions at T = 3; with and without sigma_x / sigma_c."""
import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu

B, DW, DC = 3, 2.0, 1e-5
LD = np.longdouble
_CASES = {}


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


def _case(m, T, sig):
    """Point, sigmas, the oracle's K0 (first order) and K (exact Hessian) per instance: computed once, shared, never changed."""
    key = (m, T, sig)
    if key not in _CASES:
        from oracle.padded_model import PaddedAcrobot, dense_derivatives
        model = PaddedAcrobot(64, m)
        nz, nc = (T - 1) * (64 + m) + 64, (T - 1) * 64
        rng = np.random.default_rng(7000 + 100 * m + 10 * T + int(sig))
        Z, MU = rng.random((B, nz)), rng.random((B, nc))
        SX = SC = None
        if sig:
            SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
            SX[:, ::3] = 0.0
        K0s, Ks = [], []
        for b in range(B):
            _, _, _, J, H = dense_derivatives(model, T, Z[b], MU[b])
            dx = DW + (SX[b] if sig else np.zeros(nz))
            dcv = DC + (SC[b] if sig else np.zeros(nc))
            K0s.append(np.block([[np.diag(dx), J.T], [J, -np.diag(dcv)]]))
            Ks.append(np.block([[H + np.diag(dx), J.T], [J, -np.diag(dcv)]]))
        for a in (Z, MU, SX, SC, *K0s, *Ks):
            if a is not None:
                a.setflags(write=False)
        _CASES[key] = dict(nz=nz, nc=nc, Z=Z, MU=MU, SX=SX, SC=SC, K0s=K0s, Ks=Ks)
    return _CASES[key]


def _sig_kw(c, keep):
    if c["SX"] is None:
        return {}
    keep += [_dev(c["SX"]), _dev(c["SC"])]
    return dict(sigma_x_ptr=keep[-2].data_ptr(), ldsx=c["nz"], sigma_c_ptr=keep[-1].data_ptr(), ldsc=c["nc"])


def _assemble_first_order(s, c, mu=None):
    keep = [_dev(c["Z"])]
    kw = _sig_kw(c, keep)
    if mu is not None:
        keep.append(_dev(mu))
        kw.update(mu_ptr=keep[-1].data_ptr(), ldmu=c["nc"])
    s.kkt_assemble_first_order(keep[0].data_ptr(), B, c["nz"], DW, DC, **kw)


def _assemble_exact(s, c):
    keep = [_dev(c["Z"]), _dev(c["MU"])]
    kw = _sig_kw(c, keep)
    s.kkt_assemble(keep[0].data_ptr(), B, c["nz"], keep[1].data_ptr(), c["nc"], DW, DC, **kw)


def _multiply(s, V, nz, nc):
    import torch
    dvx, dvc = _dev(V[:, :nz]), _dev(V[:, nz:])
    ox = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    oc = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_multiply(dvx.data_ptr(), nz, dvc.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc)
    torch.cuda.synchronize()
    return np.concatenate([ox.cpu().numpy(), oc.cpu().numpy()], axis=1)


def _check_product(out, Ks, V, what):
    for b, K in enumerate(Ks):
        ref = K.astype(LD) @ V[b].astype(LD)
        assert np.all(np.isfinite(out[b])), (what, b)
        err = float(np.max(np.abs(out[b].astype(LD) - ref))) / float(np.max(np.abs(ref)))
        print(f"  {what} instance {b}: max|out - K v| / max|K v| = {err:.2e}")
        assert err <= 1e-8, (what, b, err)


@pytest.mark.parametrize("m,T,sig", [(1, 2, True), (1, 2, False), (1, 3, True), (1, 3, False), (1, 9, True), (1, 9, False), (3, 3, True),
                                     (3, 3, False)])
def test_first_order_product_matches_the_dense_k0(m, T, sig):
    s, c = _solver(m, T), _case(m, T, sig)
    nz, nc = c["nz"], c["nc"]
    assert (nz, nc) == (s.nlp.num_variables, s.nlp.num_constraint)
    _assemble_first_order(s, c)
    rng = np.random.default_rng(50 + T + m)
    V = rng.standard_normal((B, nz + nc))
    out = _multiply(s, V, nz, nc)
    _check_product(out, c["K0s"], V, f"m={m} T={T} sigma={sig} first order")
    # the exact Hessian is NOT in it: the two oracle products differ by far more than the bar at this point
    gap = max(float(np.max(np.abs((c["Ks"][b] - c["K0s"][b]) @ V[b]))) / float(np.max(np.abs(c["K0s"][b] @ V[b]))) for b in range(B))
    assert gap > 1e-3, gap


def test_first_order_product_does_not_read_the_multipliers():
    s, c = _solver(1, 3), _case(1, 3, True)
    nz, nc = c["nz"], c["nc"]
    V = np.random.default_rng(77).standard_normal((B, nz + nc))
    outs = []
    for mu in (None, c["MU"], 5.0 - 3.0 * c["MU"], np.full((B, nc), np.nan)):
        _assemble_first_order(s, c, mu)
        outs.append(_multiply(s, V, nz, nc))
    for o in outs[1:]:
        assert np.array_equal(outs[0], o), "first-order products differ with the multipliers"


def test_first_order_factor_and_solve():
    for T in (3, 9):
        s, c = _solver(1, T), _case(1, T, True)
        nz, nc = c["nz"], c["nc"]
        _assemble_first_order(s, c)
        ok, neg = s.kkt_factor()
        assert np.all(ok == 1) and np.all(neg == nc), (ok, neg)     # diag > 0 over J: quasi-definite
        import torch
        rng = np.random.default_rng(90 + T)
        R = rng.standard_normal((B, nz + nc))
        rx, rc = _dev(R[:, :nz]), _dev(R[:, nz:])
        sx = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
        sc = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
        s.kkt_solve(rx.data_ptr(), nz, rc.data_ptr(), nc, sx.data_ptr(), nz, sc.data_ptr(), nc)
        torch.cuda.synchronize()
        X = np.concatenate([sx.cpu().numpy(), sc.cpu().numpy()], axis=1)
        for b in range(B):
            res = float(np.max(np.abs(c["K0s"][b].astype(LD) @ X[b].astype(LD) - R[b]))) / float(np.max(np.abs(R[b])))
            ref = np.linalg.solve(c["K0s"][b], R[b])
            err = float(np.max(np.abs(X[b] - ref))) / float(np.max(np.abs(ref)))
            print(f"  T={T} instance {b}: max|K0 x - r| / max|r| = {res:.2e}, max|x - dense solve| / max|x| = {err:.2e}")
            assert res <= 1e-8 and err <= 1e-8, (T, b, res, err)


def test_plain_assemble_afterwards_gives_the_exact_hessian_product_again():
    s, c = _solver(1, 3), _case(1, 3, True)
    nz, nc = c["nz"], c["nc"]
    V = np.random.default_rng(78).standard_normal((B, nz + nc))
    _assemble_exact(s, c)
    before = _multiply(s, V, nz, nc)
    _check_product(before, c["Ks"], V, "exact, before")
    _assemble_first_order(s, c)
    _check_product(_multiply(s, V, nz, nc), c["K0s"], V, "first order, between")
    _assemble_exact(s, c)
    after = _multiply(s, V, nz, nc)
    assert np.array_equal(before, after), "dto_kkt_assemble after a first-order assembly must give what it gave before"


def test_first_order_errors():
    from dto_amd import capi
    lane, _ = product_solver("pendulum", 6)
    z = _dev(np.zeros((B, lane.nlp.num_variables)))
    with pytest.raises(capi.DtoError) as e:
        lane.kkt_assemble_first_order(z.data_ptr(), B, lane.nlp.num_variables, DW, DC)
    assert e.value.code == 4 and "tile path only" in str(e.value)
    s, c = _solver(1, 3), _case(1, 3, True)
    nz, nc = c["nz"], c["nc"]
    V = np.random.default_rng(79).standard_normal((B, nz + nc))
    _assemble_exact(s, c)
    before = _multiply(s, V, nz, nc)
    dz, dsx = _dev(c["Z"]), _dev(c["SX"])
    for kw in (dict(ldx=nz - 1), dict(ldx=nz, sigma_x_ptr=dsx.data_ptr(), ldsx=nz - 1)):
        ldx = kw.pop("ldx")
        with pytest.raises(capi.DtoError) as e:
            s.kkt_assemble_first_order(dz.data_ptr(), B, ldx, DW, DC, **kw)
        assert e.value.code == 1 and "leading dimension" in str(e.value)
    # a refused call writes nothing: the assembled system is still the exact one
    assert np.array_equal(before, _multiply(s, V, nz, nc))

"""dto_kkt_border_multiply / dto_kkt_border_solve_refined on the lane-per-instance path (states <= 16): DTO_ERR_UNSUPPORTED -- no
assembled system is kept there to multiply with (dto_kkt_multiply is unsupported too, tests/test_lane_kmul_gpu.py) -- and the
border stays usable: a dto_kkt_border_solve after the two refused calls returns what it returned before them, bit for bit.
System: the acrobot T = 6 of tests/test_lane_border_gpu.py, nb = 2."""
import numpy as np
import pytest

from conftest import product_solver
from test_lane_border_gpu import B, DC, DW, T, _system

pytestmark = pytest.mark.gpu


def test_lane_path_refuses_and_keeps_its_border():
    import torch
    from dto_amd import capi
    c = _system()
    nz, nc, nb = c["nz"], c["nc"], 2
    s, _ = product_solver("acrobot", T)
    assert (s.nlp.num_variables, s.nlp.num_constraint) == (nz, nc)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")   # noqa: E731
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda", dtype=torch.float64)   # noqa: E731
    rng = np.random.default_rng(77)
    keep = [dev(c[k]) for k in ("Z", "MU", "SX", "SC")]
    s.kkt_assemble(keep[0].data_ptr(), B, nz, keep[1].data_ptr(), nc, DW, DC, keep[2].data_ptr(), nz, keep[3].data_ptr(), nc)
    ok, _ = s.kkt_factor()
    assert np.all(ok == 1)
    G = rng.standard_normal((B, nb, nz + nc))
    C = np.stack([-np.diag(1e-5 + rng.random(nb)) for _ in range(B)])
    dGX, dGC, dC = dev(G[:, :, :nz].reshape(B * nb, nz)), dev(G[:, :, nz:].reshape(B * nb, nc)), dev(C.reshape(B, nb * nb))
    _, singular = s.kkt_border_factor(nb, dGX.data_ptr(), nz, dGC.data_ptr(), nc, dC.data_ptr(), nb * nb)
    assert not np.any(singular)
    dRX, dRC, dRB = dev(rng.standard_normal((B, nz))), dev(rng.standard_normal((B, nc))), dev(rng.standard_normal((B, nb)))

    def solve():
        oX, oC, oB = nan(B, nz), nan(B, nc), nan(B, nb)
        s.kkt_border_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, dRB.data_ptr(), nb, oX.data_ptr(), nz, oC.data_ptr(), nc, oB.data_ptr(), nb)
        torch.cuda.synchronize()
        return np.concatenate([oX.cpu().numpy(), oC.cpu().numpy(), oB.cpu().numpy()], axis=1)
    before = solve()
    assert np.all(np.isfinite(before))
    oX, oC, oB, oR = nan(B, nz), nan(B, nc), nan(B, nb), nan(B)
    with pytest.raises(capi.DtoError, match="tile path only") as e:
        s.kkt_border_multiply(dRX.data_ptr(), nz, dRC.data_ptr(), nc, dRB.data_ptr(), nb, oX.data_ptr(), nz, oC.data_ptr(), nc, oB.data_ptr(), nb)
    assert e.value.code == 4   # DTO_ERR_UNSUPPORTED
    with pytest.raises(capi.DtoError, match="tile path only") as e:
        s.kkt_border_solve_refined(dRX.data_ptr(), nz, dRC.data_ptr(), nc, dRB.data_ptr(), nb, oX.data_ptr(), nz, oC.data_ptr(), nc,
                                   oB.data_ptr(), nb, 2, resid_ptr=oR.data_ptr())
    assert e.value.code == 4
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in (oX, oC, oB, oR)), "a refused call writes nothing"
    assert np.array_equal(before, solve())

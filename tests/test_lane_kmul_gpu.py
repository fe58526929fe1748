"""dto_kkt_multiply / dto_kkt_solve_refined on the lane-per-instance path (states <= 16): DTO_ERR_UNSUPPORTED -- no assembled
system or factor is kept there, refinement lives in its solver (dto_options.kkt_refinement) -- and the assembled state stays
usable: a dto_kkt_solve after the two refused calls returns what it returned before them, bit for bit."""
import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu


def test_lane_path_refuses_and_keeps_its_state():
    import torch
    from dto_amd import capi
    s, _ = product_solver("acrobot", 5)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    B = 2
    rng = np.random.default_rng(32)

    def dev(a):
        return torch.tensor(np.ascontiguousarray(a), device="cuda")
    dZ, dMU = dev(rng.random((B, nz))), dev(rng.random((B, nc)))
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, 30.0, 1e-5)
    ok, _ = s.kkt_factor()
    assert np.all(ok == 1)
    dRX, dRC = dev(rng.standard_normal((B, nz))), dev(rng.standard_normal((B, nc)))

    def solve():
        oX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
        oC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
        s.kkt_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
        torch.cuda.synchronize()
        return oX.cpu().numpy(), oC.cpu().numpy()
    before = solve()
    assert np.all(np.isfinite(before[0])) and np.all(np.isfinite(before[1]))
    oX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    with pytest.raises(capi.DtoError, match="tile path only") as e:
        s.kkt_multiply(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
    assert e.value.code == 4   # DTO_ERR_UNSUPPORTED
    with pytest.raises(capi.DtoError, match="tile path only") as e:
        s.kkt_solve_refined(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc, 2)
    assert e.value.code == 4
    torch.cuda.synchronize()
    assert np.all(np.isnan(oX.cpu().numpy())) and np.all(np.isnan(oC.cpu().numpy())), "a refused call writes nothing"
    after = solve()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])

"""dto_kkt_solve_multi on the lane-per-instance path (states <= 16): nrhs passes of the single solve -- there is no stored factor
to share -- with results bit-identical to nrhs calls of dto_kkt_solve."""
import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu


def test_lane_multi_solve_equals_single_solves_bit_for_bit():
    import torch
    s, _ = product_solver("acrobot", 5)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    B, nrhs = 2, 3
    rng = np.random.default_rng(31)

    def dev(a):
        return torch.tensor(np.ascontiguousarray(a), device="cuda")
    dZ, dMU = dev(rng.random((B, nz))), dev(rng.random((B, nc)))
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, 30.0, 1e-5)
    ok, _ = s.kkt_factor()
    assert np.all(ok == 1)
    RX, RC = rng.standard_normal((B, nrhs, nz)), rng.standard_normal((B, nrhs, nc))
    singles = []
    for r in range(nrhs):
        dRX, dRC = dev(RX[:, r]), dev(RC[:, r])
        oX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
        oC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
        s.kkt_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
        torch.cuda.synchronize()
        singles.append((oX.cpu().numpy(), oC.cpu().numpy()))
    dRX, dRC = dev(RX.reshape(B * nrhs, nz)), dev(RC.reshape(B * nrhs, nc))     # row b * nrhs + r
    oX = torch.full((B * nrhs, nz), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B * nrhs, nc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_solve_multi(nrhs, dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
    torch.cuda.synchronize()
    oX, oC = oX.cpu().numpy().reshape(B, nrhs, nz), oC.cpu().numpy().reshape(B, nrhs, nc)
    assert np.all(np.isfinite(oX)) and np.all(np.isfinite(oC))
    for r in range(nrhs):
        assert np.array_equal(oX[:, r], singles[r][0]) and np.array_equal(oC[:, r], singles[r][1]), r

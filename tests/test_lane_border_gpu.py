"""dto_kkt_border_factor / dto_kkt_border_solve on the lane-per-instance path (states <= 16): Y = K^-1 G' is nb sweeps of the
single solve and v0 one more (no factor is stored there), the border kernels are those of the tile path.

Reference: numpy's dense solve of the oracle's bordered matrix [[K, G'], [G, (C + C')/2]], K built as in
tests/test_entry_points_gpu.py (dense_blocks of the oracle, sigmas, delta_w = 30).  Bar: the project's 1e-8 of max |solution|
per instance over v and y together; cond2 of the bordered matrix is asserted <= 1e4."""
import numpy as np
import pytest

from conftest import product_solver
from test_entry_points_gpu import dense_blocks

pytestmark = pytest.mark.gpu

T, B, DW, DC = 6, 3, 30.0, 1e-6
_SYSTEM = {}


def _system():
    """Point, sigmas and the oracle's matrices: computed once, shared by the cases, never changed."""
    if not _SYSTEM:
        from oracle import dto_oracle as O, sympy_models as S
        p = S.build("acrobot", T, evaluate_hessian=True)
        onlp = O.NLPData(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True)
        nz, nc = onlp.num_variables, onlp.num_constraint
        rng = np.random.default_rng(606)
        Z, MU = rng.random((B, nz)), rng.random((B, nc))
        SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
        SX[:, ::3] = 0.0
        Ks = []
        for b in range(B):
            H, J = dense_blocks(onlp, Z[b], MU[b])
            K = np.block([[H + np.diag(SX[b]) + DW * np.eye(nz), J.T], [J, -np.diag(SC[b]) - DC * np.eye(nc)]])
            eig = np.linalg.eigvalsh(K)
            assert (int(np.sum(eig > 0)), int(np.sum(eig < 0))) == (nz, nc), "test point must be quasi-definite"
            Ks.append(K)
        for a in (Z, MU, SX, SC, *Ks):
            a.setflags(write=False)
        _SYSTEM.update(nz=nz, nc=nc, Z=Z, MU=MU, SX=SX, SC=SC, Ks=Ks)
    return _SYSTEM


@pytest.mark.parametrize("partitions", [0, 1])
@pytest.mark.parametrize("nb", [1, 5])
def test_lane_border_solves_match_dense_solves(nb, partitions):
    import torch
    c = _system()
    nz, nc, Ks = c["nz"], c["nc"], c["Ks"]
    s, _ = product_solver("acrobot", T)
    assert (s.nlp.num_variables, s.nlp.num_constraint) == (nz, nc)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")   # noqa: E731
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda", dtype=torch.float64)   # noqa: E731
    rng = np.random.default_rng(10 * nb + partitions)
    keep = [dev(c[k]) for k in ("Z", "MU", "SX", "SC")]
    s.set_partitions(partitions)
    try:
        s.kkt_assemble(keep[0].data_ptr(), B, nz, keep[1].data_ptr(), nc, DW, DC, keep[2].data_ptr(), nz, keep[3].data_ptr(), nc)
        ok, _ = s.kkt_factor()
        assert np.all(ok == 1)
        worst = 0.0
        for rnd in range(2):                                      # a second border on the same system: a stale Y or LU would show
            G = rng.standard_normal((B, nb, nz + nc))
            C = rng.standard_normal((B, nb, nb)) if rnd else np.stack([-np.diag(1e-5 + rng.random(nb)) for _ in range(B)])
            dGX, dGC, dC = dev(G[:, :, :nz].reshape(B * nb, nz)), dev(G[:, :, nz:].reshape(B * nb, nc)), dev(C.reshape(B, nb * nb))
            negdef, singular = s.kkt_border_factor(nb, dGX.data_ptr(), nz, dGC.data_ptr(), nc, dC.data_ptr(), nb * nb)
            assert not np.any(singular)
            Ms = []
            for b in range(B):
                Cs = 0.5 * (C[b] + C[b].T)
                M = np.block([[Ks[b], G[b].T], [G[b], Cs]])
                assert np.linalg.cond(M) <= 1e4
                eig = np.linalg.eigvalsh(Cs - G[b] @ np.linalg.solve(Ks[b], G[b].T))
                assert np.min(np.abs(eig)) > 1e-3 and negdef[b] == int(np.all(eig < 0)), (b, eig, negdef)
                Ms.append(M)
            for _ in range(3):
                R, Sb = rng.standard_normal((B, nz + nc)), rng.standard_normal((B, nb))
                dRX, dRC, dRB = dev(R[:, :nz]), dev(R[:, nz:]), dev(Sb)
                oX, oC, oB = nan(B, nz), nan(B, nc), nan(B, nb)
                s.kkt_border_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, dRB.data_ptr(), nb, oX.data_ptr(), nz, oC.data_ptr(), nc,
                                   oB.data_ptr(), nb)
                torch.cuda.synchronize()
                sol = np.concatenate([oX.cpu().numpy(), oC.cpu().numpy(), oB.cpu().numpy()], axis=1)
                for b in range(B):
                    ref = np.linalg.solve(Ms[b], np.concatenate([R[b], Sb[b]]))
                    err = float(np.max(np.abs(sol[b] - ref)) / np.max(np.abs(ref)))
                    worst = max(worst, err)
                    assert np.all(np.isfinite(sol[b])) and err <= 1e-8, (b, err)
        print(f"  nb={nb} partitions={partitions}: worst error / solution scale {worst:.2e}")
        # a new dto_kkt_factor invalidates the border on this path too
        from dto_amd import capi
        s.kkt_factor()
        with pytest.raises(capi.DtoError, match="dto_kkt_border_factor has not been called") as e:
            s.kkt_border_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, dRB.data_ptr(), nb, oX.data_ptr(), nz, oC.data_ptr(), nc,
                               oB.data_ptr(), nb)
        assert e.value.code == 1
    finally:
        s.set_partitions(0)

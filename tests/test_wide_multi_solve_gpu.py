"""Many right-hand sides against one stored factor on the tile path: dto_kkt_solve_multi on the 64-state models.

Right-hand side r of instance b is row b * nrhs + r of every array.  The panels travel through the stored records in blocks of
16 columns (k_wide_fsub_multi + k_wide_bwd_multi); the records are only read.  Reference everywhere: numpy's dense solve of the
ORACLE's matrix (oracle/padded_model.py: dense_kkt) with diag(sigma_x) / -diag(sigma_c) added, as in
tests/test_wide_linear_solver_gpu.py, whose models and helpers these tests use.  Tolerance: the project's 1e-8 of max |solution|
per right-hand side; 1e-6 for the unpivoted solve of an indefinite matrix.
"""
import numpy as np
import pytest

from test_wide_linear_solver_gpu import INDEFINITE_SEED, _assemble_factor, _dense, _dev, _solve, _solver

pytestmark = pytest.mark.gpu

NRHS = (1, 3, 16, 17, 33)   # below a block of columns, one block, one over, several blocks plus a tail (for 8 or 16 columns a block)


def _solve_multi(s, RX, RC, ldrx=None, ldrc=None, ldsx=None, ldsc=None):
    """RX [B][nrhs][nz], RC [B][nrhs][nc] -> solutions of the same shapes.  Padding of the inputs is NaN; the outputs start as
    NaN everywhere, every entry of every column must have been written and the padding must not."""
    import torch
    B, nrhs, nz = RX.shape
    nc = RC.shape[2]
    ldrx, ldrc, ldsx, ldsc = ldrx or nz, ldrc or nc, ldsx or nz, ldsc or nc
    hX, hC = np.full((B * nrhs, ldrx), np.nan), np.full((B * nrhs, ldrc), np.nan)
    hX[:, :nz], hC[:, :nc] = RX.reshape(B * nrhs, nz), RC.reshape(B * nrhs, nc)    # row b * nrhs + r
    dX, dC = _dev(hX), _dev(hC)
    oX = torch.full((B * nrhs, ldsx), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B * nrhs, ldsc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_solve_multi(nrhs, dX.data_ptr(), ldrx, dC.data_ptr(), ldrc, oX.data_ptr(), ldsx, oC.data_ptr(), ldsc)
    torch.cuda.synchronize()
    oX, oC = oX.cpu().numpy(), oC.cpu().numpy()
    assert np.all(np.isnan(oX[:, nz:])) and np.all(np.isnan(oC[:, nc:])), "padding of the outputs was written"
    return oX[:, :nz].reshape(B, nrhs, nz), oC[:, :nc].reshape(B, nrhs, nc)


def _check(Ks, RX, RC, oX, oC, tol, only=None):
    B, nrhs, nz = RX.shape
    for b in range(B):
        if only is not None and not only[b]:
            continue
        sol = np.linalg.solve(Ks[b], np.concatenate([RX[b], RC[b]], axis=1).T).T       # [nrhs][nz + nc]
        assert np.all(np.isfinite(oX[b])) and np.all(np.isfinite(oC[b])), (b, "an entry was not written")
        worst = 0.0
        for r in range(nrhs):
            scale = np.max(np.abs(sol[r]))
            ex, ec = np.max(np.abs(oX[b, r] - sol[r, :nz])), np.max(np.abs(oC[b, r] - sol[r, nz:]))
            worst = max(worst, ex / scale, ec / scale)
            assert ex <= tol * scale and ec <= tol * scale, (b, r, ex, ec, scale)
        print(f"  instance {b}, {nrhs} right-hand sides: worst error / solution scale {worst:.2e}")


def _quasi_definite_system(m, T, B, dw, seed):
    """Assemble + factor at a random point per instance with the quasi-definite settings of
    test_wide_linear_solver_matches_dense_solves; returns the solver, the dense matrices and the rng."""
    from oracle.padded_model import PaddedAcrobot
    s = _solver(m, T)
    om = PaddedAcrobot(64, m)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(seed)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
    SX[:, ::3] = 0.0
    ok, neg = _assemble_factor(s, Z, MU, dw, 1e-5, SX, SC)
    Ks = []
    for b in range(B):
        K, _, _ = _dense(om, T, Z[b], MU[b], dw, 1e-5, SX[b], SC[b])
        eig = np.linalg.eigvalsh(K)
        assert (int(np.sum(eig > 0)), int(np.sum(eig < 0))) == (nz, nc), "test point must be quasi-definite; raise dw"
        Ks.append(K)
    assert np.all(neg == nc) and np.all(ok == 1), (neg, ok, nc)
    return s, Ks, rng, nz, nc


@pytest.mark.parametrize("m,T,B,dw", [(1, 2, 2, 2.0), (1, 5, 3, 2.0), (3, 3, 2, 2.0), (4, 3, 2, 30.0)])
def test_wide_multi_solve_matches_dense_solves(m, T, B, dw):
    """T = 2 is one interior stage plus the terminal block.  Every column is a different random vector; the right-hand-side
    counts run through one factorisation one after the other."""
    s, Ks, rng, nz, nc = _quasi_definite_system(m, T, B, dw, 5 + T if m == 1 else 50 + m)
    for nrhs in NRHS:
        RX, RC = rng.standard_normal((B, nrhs, nz)), rng.standard_normal((B, nrhs, nc))
        oX, oC = _solve_multi(s, RX, RC)
        _check(Ks, RX, RC, oX, oC, 1e-8)


def test_wide_multi_solve_strides():
    """Leading dimensions above the row lengths, all four different; NaN in the padding of the inputs must not reach a
    solution, the padding of the outputs must stay as it was."""
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 5, 3, 2.0, 10)
    for nrhs in (3, 17):
        RX, RC = rng.standard_normal((3, nrhs, nz)), rng.standard_normal((3, nrhs, nc))
        oX, oC = _solve_multi(s, RX, RC, ldrx=nz + 5, ldrc=nc + 3, ldsx=nz + 7, ldsc=nc + 1)
        _check(Ks, RX, RC, oX, oC, 1e-8)


def test_wide_multi_solve_mixes_with_single_solves():
    """One factorisation: a single solve of column 2, a multi-solve of five columns, the single solve again, a second
    multi-solve.  All agree with the dense solve, and the two single solves are bit-identical: the multi-solve left the records
    (the right-hand-side slots that dto_kkt_solve writes included) to the single path."""
    B, nrhs = 2, 5
    s, Ks, rng, nz, nc = _quasi_definite_system(1, 4, B, 2.0, 21)
    RX, RC = rng.standard_normal((B, nrhs, nz)), rng.standard_normal((B, nrhs, nc))
    c2x, c2c = np.ascontiguousarray(RX[:, 2]), np.ascontiguousarray(RC[:, 2])
    before = _solve(s, c2x, c2c)
    first = _solve_multi(s, RX, RC)
    single = _solve(s, c2x, c2c)
    second = _solve_multi(s, RX, RC)
    _check(Ks, RX, RC, first[0], first[1], 1e-8)
    _check(Ks, RX, RC, second[0], second[1], 1e-8)
    _check(Ks, RX[:, 2:3], RC[:, 2:3], single[0][:, None, :], single[1][:, None, :], 1e-8)
    assert np.array_equal(before[0], single[0]) and np.array_equal(before[1], single[1])
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


def test_wide_multi_solve_indefinite_matrix():
    """The point family and delta_w = 0 of test_wide_linear_solver_indefinite_matrix: K^-1 rhs although the inertia is wrong,
    1e-6 of the solution scale."""
    from oracle.padded_model import PaddedAcrobot
    T, B, dc, nrhs = 4, 4, 1e-5, 3
    s = _solver(1, T)
    om = PaddedAcrobot(64)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(INDEFINITE_SEED)
    Z = rng.random((B, nz))
    MU = 40.0 * (rng.random((B, nc)) - 0.5)
    Ks, usable, wrong = [], [], []
    for b in range(B):
        K, _, _ = _dense(om, T, Z[b], MU[b], 0.0, dc)
        eig = np.linalg.eigvalsh(K)
        Ks.append(K)
        usable.append(bool(np.min(np.abs(eig)) > 1e-6))
        wrong.append(int(np.sum(eig < 0)) != nc)
    assert sum(usable) >= 3 and any(w and u for w, u in zip(wrong, usable)), ("vacuous: pick another seed", usable, wrong)
    _assemble_factor(s, Z, MU, 0.0, dc)
    RX, RC = rng.standard_normal((B, nrhs, nz)), rng.standard_normal((B, nrhs, nc))
    oX, oC = _solve_multi(s, RX, RC)
    _check(Ks, RX, RC, oX, oC, 1e-6, only=usable)


def test_wide_multi_solve_per_instance_parameters():
    """The per-instance (gain, weight) pairs of test_wide_linear_solver_per_instance_parameters, four right-hand sides."""
    import dto_amd
    from dto_amd import problems as P
    from oracle.padded_model import PaddedAcrobot
    T, B, dw, dc, nrhs = 3, 2, 2.0, 1e-5, 4
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
    Ks = [_dense(PaddedAcrobot(64, 1, pairs[b]), T, Z[b], MU[b], dw, dc, SX[b], SC[b])[0] for b in range(B)]
    for K in Ks:
        eig = np.linalg.eigvalsh(K)
        assert (int(np.sum(eig > 0)), int(np.sum(eig < 0))) == (nz, nc)
    assert np.all(neg == nc) and np.all(ok == 1)
    RX, RC = rng.standard_normal((B, nrhs, nz)), rng.standard_normal((B, nrhs, nc))
    oX, oC = _solve_multi(s, RX, RC)
    _check(Ks, RX, RC, oX, oC, 1e-8)


def test_wide_multi_solve_misuse():
    """The state machine of dto_kkt_solve holds for the multi-solve, and a refused call writes nothing."""
    import torch
    import dto_amd
    from dto_amd import capi, problems as P
    T, B, dw, dc, nrhs = 3, 2, 2.0, 1e-5, 3
    p = P.build_acrobot_padded(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(12)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    dZ, dMU = _dev(Z), _dev(MU)
    dX, dC = _dev(rng.standard_normal((B * nrhs, nz))), _dev(rng.standard_normal((B * nrhs, nc)))
    oX = torch.full((B * nrhs, nz), float("nan"), device="cuda", dtype=torch.float64)
    oC = torch.full((B * nrhs, nc), float("nan"), device="cuda", dtype=torch.float64)

    def refused(match, n=nrhs, ldrx=nz):
        with pytest.raises(capi.DtoError, match=match) as e:
            s.kkt_solve_multi(n, dX.data_ptr(), ldrx, dC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
        assert e.value.code == 1   # DTO_ERR_INVALID
        torch.cuda.synchronize()
        assert bool(torch.isnan(oX).all()) and bool(torch.isnan(oC).all()), "a refused call wrote to its outputs"

    refused("dto_kkt_assemble has not been called")
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc)
    refused("dto_kkt_factor has not been called")
    s.kkt_factor()
    refused("nrhs < 1", n=0)
    refused("leading dimension too small", ldrx=nz - 1)
    dx = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    dl = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    assert s.kkt_step_batch(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, dw, dc, dx.data_ptr(), nz, dl.data_ptr(), nc)
    refused("dto_kkt_step_batch / the solver has used the factor storage since")
    s.kkt_factor()
    s.kkt_solve_multi(nrhs, dX.data_ptr(), nz, dC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(oX).all()) and bool(torch.isfinite(oC).all())

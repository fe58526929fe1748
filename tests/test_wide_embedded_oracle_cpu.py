"""ORACLE pin: oracle/padded_model.py: embedded_dense_kkt -- the 64-state embedding of a 24-state problem restated without product
code -- against the problem's OWN dense K in the reference layout (dense_derivatives at n = 24 + PaddedStageRows), through the maps
zmap / mumap / musign that solver.py: pad_to_wide returns:

    K_emb[idx][:, idx] = D K_ref D,   idx = [zmap; nz_pad + mumap],  D = diag(1, musign),

to 1e-13 of max |K| (the two sum the same closed-form terms in a different order), and every row and column outside idx holds only
the constants of the embedding: delta_w / -delta_c on the diagonal, +1 at (row q, y_q) of every row q >= n, -1 at (row q, x_q) of
the padding rows.  tests/test_wide_embedded_linear_gpu.py uses the function as the reference of the stored-factor calls.
"""
import numpy as np
import pytest

DW, DC = 2.0, 1e-5
DISC = (0.4, -2.56, 0.1)
N = 64


def _problem(m, T, disc):
    from dto_amd import problems as P
    from dto_amd.solver import pad_to_wide
    from oracle.padded_model import PaddedAcrobot, PaddedStageRows
    par = (1.2, 0.8) if m == 2 else None
    p = P.build_acrobot_padded(T=T, n=24, m=m, target=0.4, terminal="physical", parameters=par, stage_constraints=disc)
    out = pad_to_wide(p["dynamics"], p["objective"], p["constraints"], p["bounds"], True)
    assert out is not None
    zmap, mumap, musign = out[4], out[5], out[6]
    model = PaddedAcrobot(24, m, par)
    rows = PaddedStageRows(24, m, T, p["x1"], p["xT"], *disc) if disc is not None else None
    return model, rows, zmap, mumap, musign


def _reference_k(model, rows, T, z, mu, dw, dc):
    """The problem's own K in the reference layout: [dynamics rows; stage rows] (src/data.jl:64-75)."""
    from oracle.padded_model import dense_derivatives
    nd = (T - 1) * model.n
    _, _, _, J, H = dense_derivatives(model, T, z, mu[:nd], 1.0)
    if rows is not None:
        J = np.vstack([J, rows.jacobian(z)])
        H = H + rows.hessian(z, mu[nd:])
    nz, nc = H.shape[0], J.shape[0]
    return np.block([[H + dw * np.eye(nz), J.T], [J, -dc * np.eye(nc)]])


@pytest.mark.parametrize("m,T,disc", [(1, 5, DISC), (1, 5, None), (2, 4, None)])
def test_embedded_dense_kkt_is_the_problems_own_k_under_the_maps(m, T, disc):
    from oracle.padded_model import embedded_dense_kkt
    model, rows, zmap, mumap, musign = _problem(m, T, disc)
    n = model.n
    nz_pad, nc_pad = (T - 1) * (N + m) + N, (T - 1) * N
    nz, nc = (T - 1) * (n + m) + n, (T - 1) * n + (rows.num if rows is not None else 0)
    assert len(zmap) == nz and len(mumap) == nc == len(musign)
    if rows is not None:
        assert np.all(musign[:(T - 1) * n] == 1.0) and np.all(musign[(T - 1) * n:] == -1.0)
    rng = np.random.default_rng(100 * m + T + (1 if disc else 0))
    z_pad, mu_pad = rng.random(nz_pad), rng.random(nc_pad)     # auxiliary and padding states / rows anywhere: K_emb[idx, idx] does
    K_emb = embedded_dense_kkt(model, rows, T, z_pad, mu_pad, DW, DC)   # not depend on them
    assert K_emb.shape == (nz_pad + nc_pad,) * 2 and np.array_equal(K_emb, K_emb.T)
    K_ref = _reference_k(model, rows, T, z_pad[zmap], mu_pad[mumap] * musign, DW, DC)
    idx = np.concatenate([zmap, nz_pad + mumap])
    D = np.concatenate([np.ones(nz), musign])
    got, want = K_emb[np.ix_(idx, idx)], D[:, None] * K_ref * D[None, :]
    err = np.max(np.abs(got - want)) / np.max(np.abs(K_ref))
    print(f"  m = {m}, T = {T}, stage rows {disc is not None}: max |K_emb[idx, idx] - D K_ref D| / max |K| = {err:.2e}")
    assert err <= 1e-13, err
    # outside idx: the constants of the embedding and nothing else
    QS = max(rows.rows_of[t] + (rows.rows_of[T - 1] if t == T - 2 else 0) for t in range(T - 1)) if rows is not None else 0
    E = np.diag(np.concatenate([np.full(nz_pad, DW), np.full(nc_pad, -DC)]))
    for t in range(T - 1):
        ox, oy = t * (N + m), (t + 1) * (N + m)
        for q in range(n, N):
            r = nz_pad + t * N + q
            E[r, oy + q] = E[oy + q, r] = 1.0
            if q >= n + QS:
                E[r, ox + q] = E[ox + q, r] = -1.0
    outside = np.ones(K_emb.shape, dtype=bool)
    outside[np.ix_(idx, idx)] = False
    assert np.array_equal(K_emb[outside], E[outside])
    assert len(idx) < K_emb.shape[0] and np.count_nonzero(E[outside]) > 0

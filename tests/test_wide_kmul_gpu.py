"""dto_kkt_multiply on the tile path: out = K [v_x; v_c] on the system of dto_kkt_assemble (k_wide_kmul).

Reference everywhere: the ORACLE's dense matrix (oracle/padded_model.py: dense_kkt, plus diag([sigma_x; -sigma_c])) applied in
np.longdouble on the host.  Bar: the project's 1e-8 of max |K v|; the componentwise figure
max_i |out - K v|_i / (|K| |v|)_i is printed (DESIGN.md section 4.3 records it).  Shapes: one stage, two stages, three and four
actions, a chunk edge of the kernel's grid with one stage and with three stages behind it (T = S + 1, S + 3), and three chunks
(T = 2 S + 2).  The chunk length itself (DTO_WIDE_KMUL_S, read once per process) is varied over child processes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu

S = 8                      # stages per workgroup of k_wide_kmul (csrc/dto_wide_kernels.hpp: DTO_WIDE_KMUL_S; tests/test_kkt_multiply_cpu.py
DW, DC, B = 2.0, 1e-5, 3   # checks that the two agree)
LD = np.longdouble


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


_MODELS, _CASES = {}, {}


def _oracle_model(m, parameters=None):
    from oracle.padded_model import PaddedAcrobot
    key = (m, parameters)
    if key not in _MODELS:
        _MODELS[key] = PaddedAcrobot(64, m, parameters)
    return _MODELS[key]


def _dense(m, T, z, mu, dw, dc, sx=None, sc=None, parameters=None):
    from oracle.padded_model import dense_kkt
    K, _ = dense_kkt(_oracle_model(m, parameters), T, z, mu, dw, dc)
    if sx is not None:
        K = K + np.diag(np.concatenate([sx, -sc]))
    return K


def _point(m, T, sig=True):
    """Point and sigmas of one case (no oracle matrix: the children of the chunk-length test need none)."""
    nz, nc = (T - 1) * (64 + m) + 64, (T - 1) * 64
    rng = np.random.default_rng(1000 * m + 10 * T + int(sig))
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    SX = SC = None
    if sig:
        SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
        SX[:, ::3] = 0.0
    return dict(nz=nz, nc=nc, Z=Z, MU=MU, SX=SX, SC=SC)


def _case(m, T, sig=True):
    """Point, sigmas and the oracle's matrices of one case: computed once, shared by the tests, never changed."""
    key = (m, T, sig)
    if key not in _CASES:
        c = _point(m, T, sig)
        Z, MU, SX, SC = c["Z"], c["MU"], c["SX"], c["SC"]
        Ks = [_dense(m, T, Z[b], MU[b], DW, DC, None if SX is None else SX[b], None if SC is None else SC[b]) for b in range(B)]
        for a in (Z, MU, SX, SC, *Ks):
            if a is not None:
                a.setflags(write=False)
        _CASES[key] = dict(c, Ks=Ks)
    return _CASES[key]


def _assemble(s, c):
    nz, nc = c["nz"], c["nc"]
    keep = [_dev(c["Z"]), _dev(c["MU"])]
    kw = {}
    if c["SX"] is not None:
        keep += [_dev(c["SX"]), _dev(c["SC"])]
        kw.update(sigma_x_ptr=keep[2].data_ptr(), ldsx=nz, sigma_c_ptr=keep[3].data_ptr(), ldsc=nc)
    s.kkt_assemble(keep[0].data_ptr(), c["Z"].shape[0], nz, keep[1].data_ptr(), nc, DW, DC, **kw)


def _multiply(s, V, nz, nc, lds=None):
    """V: [B][nz + nc].  lds = (ldvx, ldvc, ldox, ldoc): padded arrays, NaN in the padding and in the outputs before the call."""
    import torch
    nb = V.shape[0]
    ldvx, ldvc, ldox, ldoc = lds or (nz, nc, nz, nc)
    vx, vc = np.full((nb, ldvx), np.nan), np.full((nb, ldvc), np.nan)
    vx[:, :nz], vc[:, :nc] = V[:, :nz], V[:, nz:]
    dvx, dvc = _dev(vx), _dev(vc)
    ox = torch.full((nb, ldox), float("nan"), device="cuda", dtype=torch.float64)
    oc = torch.full((nb, ldoc), float("nan"), device="cuda", dtype=torch.float64)
    s.kkt_multiply(dvx.data_ptr(), ldvx, dvc.data_ptr(), ldvc, ox.data_ptr(), ldox, oc.data_ptr(), ldoc)
    torch.cuda.synchronize()
    ox, oc = ox.cpu().numpy(), oc.cpu().numpy()
    assert np.all(np.isnan(ox[:, nz:])) and np.all(np.isnan(oc[:, nc:])), "the padding of the outputs must stay untouched"
    return np.concatenate([ox[:, :nz], oc[:, :nc]], axis=1)


def _check(out, Ks, V, what):
    worst = 0.0
    for b, K in enumerate(Ks):
        KL, vL = K.astype(LD), V[b].astype(LD)
        ref = KL @ vL
        mag = np.abs(KL) @ np.abs(vL)
        assert np.all(np.isfinite(out[b])), (what, b)
        err = np.abs(out[b].astype(LD) - ref)
        nrm = float(np.max(err)) / float(np.max(np.abs(ref)))
        pos = mag > 0                                       # (rows with an empty product: covered by the norm-wise bar alone)
        cw = float(np.max(err[pos] / mag[pos]))
        worst = max(worst, cw)
        print(f"  {what} instance {b}: max|out - Kv| / max|Kv| = {nrm:.2e}, componentwise max |out - Kv|_i / (|K||v|)_i = {cw:.2e}")
        assert nrm <= 1e-8, (what, b, nrm)
    return worst


def _vectors(m, T, nz, nc, rng):
    """random v; then unit vectors, one per instance: an x_t, the last action of a stage, a lam_t; then an x_T component"""
    n = 64
    t = (T - 1) // 2                                        # a stage in the middle (stage 0 when T = 2)
    ix, iu, il, iT = t * (n + m) + 5, t * (n + m) + n + m - 1, nz + t * n + 2, (T - 1) * (n + m) + 3
    V0 = rng.standard_normal((B, nz + nc))
    V1 = np.zeros((B, nz + nc)); V1[0, ix] = 1.0; V1[1, iu] = 1.0; V1[2, il] = 1.0
    V2 = rng.standard_normal((B, nz + nc)); V2[0] = 0.0; V2[0, iT] = 1.0
    return [("random", V0), ("unit x_t / u_t / lam_t", V1), ("unit x_T", V2)]


@pytest.mark.parametrize("m,T,sig,padded", [(1, 2, True, False), (1, 3, True, True), (1, 3, False, False), (3, 3, True, False),
                                            (4, 3, True, False), (1, S + 1, True, False), (1, S + 3, True, False),
                                            (1, 2 * S + 2, True, False)])
def test_kkt_multiply_matches_the_oracle(m, T, sig, padded):
    """Columns and random combinations of the oracle's K: a wrong block shows as a wrong column.  sig=False: sigma_x / sigma_c
    NULL.  padded: four different leading dimensions, NaN in every padding entry -- read paddings would show as NaN in the
    product, written ones are caught in _multiply.  T = 2 S + 2: three chunks, the middle one recomputes a left edge and holds
    no terminal knot."""
    s = _solver(m, T)
    c = _case(m, T, sig)
    nz, nc = c["nz"], c["nc"]
    assert (nz, nc) == (s.nlp.num_variables, s.nlp.num_constraint)
    _assemble(s, c)                                         # no factorisation: the product needs none
    rng = np.random.default_rng(7 + T)
    lds = (nz + 3, nc + 1, nz + 8, nc + 5) if padded else None
    worst = 0.0
    for what, V in _vectors(m, T, nz, nc, rng):
        worst = max(worst, _check(_multiply(s, V, nz, nc, lds), c["Ks"], V, what))
    print(f"  m = {m}, T = {T}: worst componentwise figure {worst:.2e}")


@pytest.mark.parametrize("m", [1, 3])
def test_kkt_multiply_is_symmetric(m):
    """u'(K v) = v'(K u) needs no entry of the oracle: |u'(Kv) - v'(Ku)| <= (q + 1) 2^-53 |u|'|K||v|, the standard bound of a
    dot product of length q in any summation order (q: the largest number of nonzeros in a row of K; |K| from the oracle)."""
    T = 3
    s = _solver(m, T)
    c = _case(m, T, True)
    nz, nc = c["nz"], c["nc"]
    _assemble(s, c)
    rng = np.random.default_rng(70 + m)
    U, V = rng.standard_normal((B, nz + nc)), rng.standard_normal((B, nz + nc))
    KU, KV = _multiply(s, U, nz, nc), _multiply(s, V, nz, nc)
    for b, K in enumerate(c["Ks"]):
        q = int(np.max(np.sum(K != 0.0, axis=1)))
        lhs = abs(float(U[b].astype(LD) @ KV[b].astype(LD) - V[b].astype(LD) @ KU[b].astype(LD)))
        bound = (q + 1) * 2.0 ** -53 * float(np.abs(U[b]).astype(LD) @ (np.abs(K).astype(LD) @ np.abs(V[b]).astype(LD)))
        print(f"  m = {m} instance {b}: q = {q}, |u'Kv - v'Ku| = {lhs:.2e}, bound {bound:.2e}")
        assert lhs <= bound, (b, q, lhs, bound)


def test_kkt_multiply_is_bit_identical_run_to_run():
    T = S + 3                                               # two workgroups per instance
    s = _solver(1, T)
    c = _case(1, T, True)
    _assemble(s, c)
    V = np.random.default_rng(3).standard_normal((B, c["nz"] + c["nc"]))
    a, b_ = _multiply(s, V, c["nz"], c["nc"]), _multiply(s, V, c["nz"], c["nc"])
    assert np.array_equal(a, b_)


CHUNK_T = S + 3


def _chunk_child(out_path):
    """One process of test_kkt_multiply_is_bit_identical_for_every_chunk_length: the product of one fixed vector, saved."""
    c = _point(1, CHUNK_T, True)
    s = _solver(1, CHUNK_T)
    _assemble(s, c)
    V = np.random.default_rng(4).standard_normal((B, c["nz"] + c["nc"]))
    out = _multiply(s, V, c["nz"], c["nc"])
    assert np.all(np.isfinite(out))
    with open(out_path, "wb") as f:
        np.save(f, out)


def test_kkt_multiply_is_bit_identical_for_every_chunk_length(tmp_path):
    """k_wide_kmul writes every row once, by one thread, from the same operations whatever the chunk length is.  The length is
    read from DTO_WIDE_KMUL_S once per process, so each value gets a fresh child process, one after the other (never two children
    on the GPU at a time): 1 and 3 stages per workgroup and the default 8 on T = S + 3."""
    outs = []
    for chunk in ("1", "3", None):
        env = {k: v for k, v in os.environ.items() if k != "DTO_WIDE_KMUL_S"}
        if chunk is not None:
            env["DTO_WIDE_KMUL_S"] = chunk
        path = tmp_path / f"kv_{chunk}.bin"
        r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), str(path)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (chunk, r.returncode, r.stdout[-2000:], r.stderr[-2000:])   # (no further child after a failure)
        with open(path, "rb") as f:
            outs.append(np.load(f))
    assert outs[0].shape == (B, (CHUNK_T - 1) * 129 + 64) and np.all(np.isfinite(outs[0]))
    assert np.array_equal(outs[0], outs[2]), "1 stage per workgroup differs from the default"
    assert np.array_equal(outs[1], outs[2]), "3 stages per workgroup differ from the default"


def test_kkt_multiply_per_instance_parameters():
    """dto_batch.params of dto_kkt_assemble: B = 2 with different (gain, weight) pairs; each instance equals a B = 1 call with its
    own parameters bit for bit, and the oracle's matrix of its own pair to 1e-8."""
    import dto_amd
    from dto_amd import problems as P
    T = 3
    p = P.build_acrobot_padded(T=T, parameters=(1.3, 0.7))
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       parameters=p["parameters"], name="acrobot_padded_par")
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    pairs = [(0.8, 1.5), (1.6, 0.4)]
    W = np.array([np.tile(pr, T) for pr in pairs])
    rng = np.random.default_rng(78)
    Z, MU, V = rng.random((2, nz)), rng.random((2, nc)), rng.standard_normal((2, nz + nc))

    def run(rows):
        dZ, dMU, dW = _dev(Z[rows]), _dev(MU[rows]), _dev(W[rows])
        s.kkt_assemble(dZ.data_ptr(), len(rows), nz, dMU.data_ptr(), nc, DW, DC, params_ptr=dW.data_ptr(), ldp=W.shape[1])
        return _multiply(s, V[rows], nz, nc)
    both = run([0, 1])
    for b in range(2):
        assert np.array_equal(both[b], run([b])[0]), b
    Ks = [_dense(1, T, Z[b], MU[b], DW, DC, parameters=pairs[b]) for b in range(2)]
    _check(both, Ks, V, "parameters")
    assert np.max(np.abs(both[0] - (_dense(1, T, Z[0], MU[0], DW, DC, parameters=pairs[1]) @ V[0]))) > 1e-3   # the parameters matter


def test_kkt_multiply_leaves_the_factor_alone():
    """Multiply works after assemble without a factor; a dto_kkt_solve before and after a dto_kkt_multiply on one factorisation
    returns bit-identical results, and the product itself does not depend on whether a factor exists."""
    import torch
    T = 3
    s = _solver(1, T)
    c = _case(1, T, True)
    nz, nc = c["nz"], c["nc"]
    _assemble(s, c)
    rng = np.random.default_rng(19)
    V = rng.standard_normal((B, nz + nc))
    before_factor = _multiply(s, V, nz, nc)
    ok, neg = s.kkt_factor()
    assert np.all(ok == 1) and np.all(neg == nc)
    dRX, dRC = _dev(V[:, :nz]), _dev(V[:, nz:])

    def solve():
        oX = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
        oC = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
        s.kkt_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
        torch.cuda.synchronize()
        return np.concatenate([oX.cpu().numpy(), oC.cpu().numpy()], axis=1)
    first = solve()
    after_factor = _multiply(s, V, nz, nc)
    second = solve()
    assert np.all(np.isfinite(first)) and np.array_equal(first, second)
    assert np.array_equal(before_factor, after_factor)
    # and the two are inverse to each other: the solve is within the project's 1e-8 max|sol| of K^-1 v, so
    # K sol - v is within 1e-8 max|sol| times the largest absolute row sum of K
    back = _multiply(s, first, nz, nc)
    for i, K in enumerate(c["Ks"]):
        assert np.max(np.abs(back[i] - V[i])) <= 1e-8 * np.max(np.abs(first[i])) * np.max(np.sum(np.abs(K), axis=1)), i


if __name__ == "__main__":
    _chunk_child(sys.argv[1])

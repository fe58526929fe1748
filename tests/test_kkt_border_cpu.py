"""dto_kkt_border_factor / dto_kkt_border_solve without a GPU: the symbols and their signatures in the header, capi.py, the Julia
shim and the INTEGRATION.md listing; the device error; and the Schur route of csrc/dto_border_kernels.hpp restated in numpy, in
the order of the kernels' operations, against the dense solve of the oracle's bordered matrix."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import product_solver

import dto_amd
from dto_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"dto_kkt_border_factor": ["ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "ptr", "ptr"],
        "dto_kkt_border_solve": ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr"]}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _c_class(param):
    if "*" in param:
        return "ptr"
    t = re.sub(r"\b\w+$", "", param).replace("const", "").strip()
    return {"int64_t": "i64", "int": "i32", "int32_t": "i32", "double": "f64"}[t]


def _jl_class(t):
    t = t.strip()
    if t.startswith(("Ptr{", "Ref{")):
        return "ptr"
    return {"Int64": "i64", "Cint": "i32", "Int32": "i32", "Float64": "f64"}[t]


def _jl_types(src, name):
    out = []
    for m in re.finditer(r"ccall\(\(:%s,\s*libdto\)\s*,\s*Cint\s*,\s*\((.*?)\)\s*,\n" % name, src, flags=re.S):
        out.append([_jl_class(t) for t in re.split(r",(?![^{]*\})", m.group(1)) if t.strip()])
    return out


@pytest.mark.parametrize("name", sorted(WANT))
def test_symbol_in_header_capi_shim_and_listing(name):
    header = re.sub(r"/\*.*?\*/", " ", _read("include", "dto.h"), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S)
    assert m, f"{name} is not declared in include/dto.h"
    assert [_c_class(p.strip()) for p in m.group(1).split(",")] == WANT[name]
    fn = getattr(capi.lib(), name)                            # the shared library exports it, capi.py binds it
    cls = {ctypes.c_void_p: "ptr", capi.c_int32_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int: "i32"}
    assert [cls[t] for t in fn.argtypes] == WANT[name] and fn.restype is ctypes.c_int
    shim = _jl_types(_read("julia", "gpu_evaluator.jl"), name)
    assert shim and all(t == WANT[name] for t in shim), (name, shim)
    md = "\n\n".join(re.findall(r"```julia\n(.*?)```", _read("INTEGRATION.md"), flags=re.S))
    listing = _jl_types(md, name)
    assert listing and all(t == WANT[name] for t in listing), (name, listing)
    assert f"`{name}" in _read("README.md")
    assert int(re.search(r"#define\s+DTO_ABI_VERSION\s+(\d+)", header).group(1)) == 4      # entry points are only added


def test_python_signatures():
    fac = inspect.signature(dto_amd.Solver.kkt_border_factor).parameters
    assert list(fac) == ["self", "nb", "g_x_ptr", "ldgx", "g_c_ptr", "ldgc", "c_ptr", "ldc", "stream"]
    assert all(fac[k].default == 0 for k in ("g_c_ptr", "ldgc", "c_ptr", "ldc", "stream"))
    sol = inspect.signature(dto_amd.Solver.kkt_border_solve).parameters
    assert list(sol) == ["self", "rhs_x_ptr", "ldrx", "rhs_c_ptr", "ldrc", "rhs_b_ptr", "ldrb", "sol_x_ptr", "ldsx", "sol_c_ptr", "ldsc",
                         "sol_b_ptr", "ldsb", "stream"]
    assert sol["stream"].default == 0


def test_constants_of_the_tests_are_the_kernels():
    """tests/test_wide_border_gpu.py places its chunk cases by the slab of 128 and relies on the limit of 16 rows."""
    src = _read("directtrajectoryoptimization.jl_amd", "csrc", "dto_border_kernels.hpp")
    assert int(re.search(r"constexpr int KB_KT = (\d+);", src).group(1)) == 128
    assert int(re.search(r"constexpr int KB_MAX = (\d+);", src).group(1)) == 16
    assert int(re.search(r"constexpr int KB_CHUNK_DEFAULT = (\d+);", src).group(1)) == 2048
    # the runtime-only header is no part of a plugin's cache key: the plugins' kernels do not depend on it
    assert "dto_border_kernels.hpp" in re.search(r"fn not in \((.*?)\)", _read("directtrajectoryoptimization.jl_amd", "plugin.py")).group(1)


def test_wrappers_reject_bad_arguments_on_the_host():
    s, _ = product_solver("pendulum", 6)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    g = np.zeros((2, nz))
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_border_factor(1, g, nz)
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_border_factor(1.0, g.ctypes.data, nz)
    r = np.zeros((2, nz + nc + 1))
    with pytest.raises(ValueError, match="overlap"):
        s.kkt_border_solve(r.ctypes.data, nz, r.ctypes.data + 8, nc, r.ctypes.data + 16, 1, r.ctypes.data, nz, r.ctypes.data + 24, nc,
                           r.ctypes.data + 32, 1)


def test_calls_fail_loudly_without_a_gpu():
    n = ctypes.c_int(-1)
    capi.check(capi.lib().dto_device_count(ctypes.byref(n)))
    if n.value > 0:
        return  # on the GPU box the calls are exercised by tests/test_wide_border_gpu.py and tests/test_lane_border_gpu.py
    s, _ = product_solver("pendulum", 6)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    s._B = 2
    g, r, o = np.zeros((2, nz)), np.zeros((2, nz + nc + 1)), np.zeros((2, nz + nc + 1))
    with pytest.raises(capi.DtoError) as e:
        s.kkt_border_factor(1, g.ctypes.data, nz)
    assert e.value.code in (1, 3)   # DTO_ERR_DEVICE (there is no CPU fallback) or DTO_ERR_INVALID
    with pytest.raises(capi.DtoError) as e:
        s.kkt_border_solve(r.ctypes.data, nz, r.ctypes.data, nc, r.ctypes.data, 1, o.ctypes.data, nz, o.ctypes.data, nc, o.ctypes.data, 1)
    assert e.value.code in (1, 3)


# ---- the Schur route in the order of the kernels -------------------------------------------------------------------------------
def gram_in_kernel_order(G, Y, chunk, kt=128):
    """k_border_gram + the chunk sum of k_border_schur: per chunk, per slab, four partial sums (one per wavefront: a quarter of the
    slab each, four entries of k per matrix-core step), added in wavefront order; the chunks added in chunk order."""
    nb, N = G.shape
    chunk = (chunk + kt - 1) // kt * kt
    P = np.zeros((nb, nb))
    for k_lo in range(0, N, chunk):
        k_hi = min(N, k_lo + chunk)
        acc = np.zeros((4, nb, nb))
        for k0 in range(k_lo, k_hi, kt):
            for w in range(4):
                for kk in range(k0 + w * (kt // 4), min(k_hi, k0 + (w + 1) * (kt // 4)), 4):
                    acc[w] += G[:, kk:min(kk + 4, k_hi)] @ Y[:, kk:min(kk + 4, k_hi)].T
        P += ((acc[0] + acc[1]) + acc[2]) + acc[3]
    return P


def schur_factor(K, G, C, chunk=2048):
    """dto_kkt_border_factor: Y, the LU of S with partial pivoting (row exchanges recorded step by step), the two flags."""
    nb = G.shape[0]
    Y = np.linalg.solve(K, G.T).T
    P = gram_in_kernel_order(G, Y, chunk)
    S = (np.zeros((nb, nb)) if C is None else 0.5 * (C + C.T)) - 0.5 * (P + P.T)
    try:
        np.linalg.cholesky(-S)
        negdef = 1
    except np.linalg.LinAlgError:
        negdef = 0
    A, piv, singular = S.copy(), [], 0
    for k in range(nb):
        pv = k + int(np.argmax(np.abs(A[k:, k])))
        piv.append(pv)
        A[[k, pv]] = A[[pv, k]]
        if not abs(A[k, k]) > 0.0:
            singular = 1
            continue
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return Y, A, piv, negdef, singular


def schur_solve(K, Y, A, piv, singular, r, sb):
    """dto_kkt_border_solve: v0 = K^-1 r, t = s - Y r (G K^-1 r = Y r: K is symmetric), y = S^-1 t from the LU, v = v0 - Y' y."""
    nb = Y.shape[0]
    v0 = np.linalg.solve(K, r)
    t = sb - Y @ r
    if singular:
        y = np.full(nb, np.nan)
    else:
        for k in range(nb):                      # the exchanges moved whole rows, multipliers included: all of them first
            t[[k, piv[k]]] = t[[piv[k], k]]
        for k in range(nb):
            t[k + 1:] -= A[k + 1:, k] * t[k]
        y = t
        for k in range(nb - 1, -1, -1):
            y[k] = (y[k] - A[k, k + 1:] @ y[k + 1:]) / A[k, k]
    v = v0.copy()
    for j in range(nb):
        v -= y[j] * Y[j]
    return np.concatenate([v, y])


@pytest.fixture(scope="module")
def oracle_system():
    """The (m, T) = (1, 4) system of tests/test_wide_border_gpu.py: delta_w = 2, the sigmas of the stored-factor tests."""
    from oracle.padded_model import PaddedAcrobot, dense_kkt
    T, dw, dc = 4, 2.0, 1e-5
    nz, nc = (T - 1) * 65 + 64, (T - 1) * 64
    rng = np.random.default_rng(9)
    z, mu = rng.random(nz), rng.random(nc)
    sx, sc = rng.random(nz) * 3.0, rng.random(nc) * 0.5
    sx[::3] = 0.0
    K, _ = dense_kkt(PaddedAcrobot(64, 1), T, z, mu, dw, dc)
    K = K + np.diag(np.concatenate([sx, -sc]))
    eig = np.linalg.eigvalsh(K)
    assert (int(np.sum(eig > 0)), int(np.sum(eig < 0))) == (nz, nc)
    K.setflags(write=False)
    return K, nz, nc, rng


@pytest.mark.parametrize("nb,use_gc,ckind,chunk", [(1, False, "negdiag", 2048), (5, False, "negdiag", 2048), (16, True, "negdiag", 64),
                                                   (16, False, None, 2048), (7, True, "nonsymmetric", 128),
                                                   (6, False, "large", 2048)])
def test_schur_route_in_kernel_order_matches_the_dense_solve(oracle_system, nb, use_gc, ckind, chunk):
    """Pins the algebra where it runs without a GPU: the Y r identity, the symmetrisation of C (a non-symmetric C must give what
    its symmetric part gives), the pivoted LU with recorded exchanges, the chunked sums.  The dense solve and the route agree to a
    few 1e-15 on these systems; 1e-12 is asserted, four orders inside the 1e-8 of the GPU tests."""
    K, nz, nc, _ = oracle_system
    rng = np.random.default_rng(100 + nb)
    G = rng.standard_normal((nb, nz + nc))
    if not use_gc:
        G[:, nz:] = 0.0
    # ("large": an indefinite S whose largest entries are off the diagonal, so that the LU exchanges rows)
    C = {"negdiag": -np.diag(1e-5 + rng.random(nb)), "nonsymmetric": rng.standard_normal((nb, nb)),
         "large": 60.0 * rng.standard_normal((nb, nb)), None: None}[ckind]
    Cs = np.zeros((nb, nb)) if C is None else 0.5 * (C + C.T)
    M = np.block([[K, G.T], [G, Cs]])
    assert np.linalg.cond(M) <= 1e4
    Y, A, piv, negdef, singular = schur_factor(K, G, C, chunk)
    S = Cs - G @ np.linalg.solve(K, G.T)
    eig = np.linalg.eigvalsh(0.5 * (S + S.T))
    assert singular == 0 and negdef == int(np.all(eig < 0)) and np.min(np.abs(eig)) > 1e-3
    assert ckind != "large" or any(p != k for k, p in enumerate(piv)), "the case is there for the row exchanges"
    for _ in range(3):
        r, sb = rng.standard_normal(nz + nc), rng.standard_normal(nb)
        ref = np.linalg.solve(M, np.concatenate([r, sb]))
        got = schur_solve(K, Y, A, piv, singular, r, sb)
        err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
        print(f"  nb={nb} g_c={use_gc} C={ckind}: route against dense solve {err:.2e}, cond2 {np.linalg.cond(M):.2e}")
        assert err <= 1e-12


def test_schur_route_flags_a_zero_row(oracle_system):
    """A zero border row with C = 0: row and column of S are exactly zero, the pivot is an exact zero, the solution NaN."""
    K, nz, nc, _ = oracle_system
    rng = np.random.default_rng(7)
    G = rng.standard_normal((2, nz + nc))
    G[1] = 0.0
    Y, A, piv, negdef, singular = schur_factor(K, G, None)
    assert (negdef, singular) == (0, 1) and A[1, 1] == 0.0
    assert np.all(np.isnan(schur_solve(K, Y, A, piv, singular, rng.standard_normal(nz + nc), rng.standard_normal(2))))


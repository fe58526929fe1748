"""dto_kkt_border_multiply / dto_kkt_border_solve_refined without a GPU: the symbols and their signatures in the header, capi.py,
the Julia shim and the INTEGRATION.md listing; the host-side argument checks and the device error; and the refined Schur route
restated in numpy -- dto_kkt_border_solve (tests/test_kkt_border_cpu.py: schur_factor / schur_solve) plus passes of
(rho, sigma) = (r, s) - M (v, y) in float64, a bordered solve of the residual and the update -- on the oracle's matrix.

Bar: omega = max_i |rhs - M sol|_i / (|M||sol| + |rhs|)_i <= (q + 1) 2^-53 after two passes, q the largest number of nonzeros in a
row of the bordered matrix M = [[K, G'], [G, sym(C)]], counted on M itself (border rows are dense in G: q is at most N + nb, 5e-14
at N = 451; a diagonal C or a missing g_c only lowers the count and with it the bar): the limiting
componentwise backward error of fixed-precision refinement with working-precision residuals (Skeel 1980; Higham, Accuracy and
Stability of Numerical Algorithms, Theorem 12.3), the bar of tests/test_wide_refined_solve_gpu.py.  omega is evaluated in
np.longdouble."""
import ctypes
import inspect
import re

import numpy as np
import pytest

from conftest import product_solver
from test_kkt_border_cpu import _c_class, _jl_types, _read, oracle_system, schur_factor, schur_solve  # noqa: F401 (fixture)

import dto_amd
from dto_amd import capi

LD = np.longdouble
WANT = {"dto_kkt_border_multiply": ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr"],
        "dto_kkt_border_solve_refined": ["ptr", "i32", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64",
                                         "ptr", "ptr"]}


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
    assert _read("README.md").count(f"`{name}`") >= 2, "named in the linear-solver bullet and in the known limits"
    assert int(re.search(r"#define\s+DTO_ABI_VERSION\s+(\d+)", header).group(1)) == 4      # entry points are only added


def test_python_signatures():
    mul = inspect.signature(dto_amd.Solver.kkt_border_multiply).parameters
    assert list(mul) == ["self", "v_x_ptr", "ldvx", "v_c_ptr", "ldvc", "v_b_ptr", "ldvb", "out_x_ptr", "ldox", "out_c_ptr", "ldoc",
                         "out_b_ptr", "ldob", "stream"]
    assert mul["stream"].default == 0
    ref = inspect.signature(dto_amd.Solver.kkt_border_solve_refined).parameters
    assert list(ref) == ["self", "rhs_x_ptr", "ldrx", "rhs_c_ptr", "ldrc", "rhs_b_ptr", "ldrb", "sol_x_ptr", "ldsx", "sol_c_ptr", "ldsc",
                         "sol_b_ptr", "ldsb", "passes", "resid_ptr", "stream"]
    assert ref["resid_ptr"].default == 0 and ref["stream"].default == 0
    assert ref["passes"].default is inspect.Parameter.empty


def test_the_new_kernels_belong_to_the_runtime_library():
    src = _read("directtrajectoryoptimization.jl_amd", "csrc", "dto_border_kernels.hpp")
    for kernel in ("k_border_mul", "k_border_mul_fin"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, src), kernel
    assert "atomic" not in src.split("k_border_mul(")[1].split("static __global__")[0], "no atomic sums in the product"
    assert "asm" not in src


def test_wrappers_reject_bad_arguments_on_the_host():
    s, _ = product_solver("pendulum", 6)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    r, o = np.zeros((2, nz + nc + 1)), np.zeros((2, nz + nc + 1))
    rp, op = r.ctypes.data, o.ctypes.data
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_border_multiply(r, nz, rp + 8, nc, rp + 16, 1, op, nz, op + 8, nc, op + 16, 1)
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_border_multiply(rp, nz, rp + 8, nc, rp + 16, 1, op, nz, op + 8, nc, 1.5, 1)
    with pytest.raises(ValueError, match="overlap"):
        s.kkt_border_multiply(rp, nz, rp + 8, nc, rp + 16, 1, op, nz, op + 8, nc, rp + 16, 1)
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_border_solve_refined(rp, nz, rp + 8, nc, r, 1, op, nz, op + 8, nc, op + 16, 1, 2)
    with pytest.raises(TypeError, match="passes"):
        s.kkt_border_solve_refined(rp, nz, rp + 8, nc, rp + 16, 1, op, nz, op + 8, nc, op + 16, 1, 2.0)
    with pytest.raises(TypeError, match="passes"):
        s.kkt_border_solve_refined(rp, nz, rp + 8, nc, rp + 16, 1, op, nz, op + 8, nc, op + 16, 1, True)
    for passes in (-1, 5):
        with pytest.raises(ValueError, match=r"passes outside 0\.\.4"):
            s.kkt_border_solve_refined(rp, nz, rp + 8, nc, rp + 16, 1, op, nz, op + 8, nc, op + 16, 1, passes)
    for kw in (dict(sx=rp), dict(sc=rp + 8), dict(sb=rp + 16)):
        a = dict(sx=op, sc=op + 8, sb=op + 16)
        a.update(kw)
        with pytest.raises(ValueError, match="overlap"):
            s.kkt_border_solve_refined(rp, nz, rp + 8, nc, rp + 16, 1, a["sx"], nz, a["sc"], nc, a["sb"], 1, 2)


def test_calls_fail_loudly_without_a_gpu():
    n = ctypes.c_int(-1)
    capi.check(capi.lib().dto_device_count(ctypes.byref(n)))
    if n.value > 0:
        return  # on the GPU box the calls are exercised by tests/test_wide_border_refined_gpu.py and tests/test_lane_border_refined_gpu.py
    s, _ = product_solver("pendulum", 6)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    r, o = np.zeros((2, nz + nc + 1)), np.zeros((2, nz + nc + 1))
    rp, op = r.ctypes.data, o.ctypes.data
    with pytest.raises(capi.DtoError) as e:
        s.kkt_border_multiply(rp, nz, rp, nc, rp, 1, op, nz, op, nc, op, 1)
    assert e.value.code in (1, 3)   # DTO_ERR_DEVICE (there is no CPU fallback) or DTO_ERR_INVALID
    with pytest.raises(capi.DtoError) as e:
        s.kkt_border_solve_refined(rp, nz, rp, nc, rp, 1, op, nz, op, nc, op, 1, 2)
    assert e.value.code in (1, 3)


# ---- the refined route in numpy ----------------------------------------------------------------------------------------------
def omega(M, sol, rhs):
    ML, xL, rL = M.astype(LD), sol.astype(LD), rhs.astype(LD)
    return float(np.max(np.abs(rL - ML @ xL) / (np.abs(ML) @ np.abs(xL) + np.abs(rL))))


def refined(solve, M, rhs, passes):
    """dto_kkt_border_solve_refined: the bordered solve, then residual = rhs - M sol in float64 (M holds sym(C)), the bordered
    solve of the residual, the update."""
    sol = solve(rhs)
    for _ in range(passes):
        sol = sol + solve(rhs - M @ sol)
    return sol


def _bar(M):
    return (int(np.max(np.sum(M != 0.0, axis=1))) + 1) * 2.0 ** -53


@pytest.mark.parametrize("nb,use_gc", [(5, False), (16, True)])
def test_refined_route_reaches_the_backward_error_bar(oracle_system, nb, use_gc):
    """The exact float64 inner solve: already at 1e-15 without a pass (the feature matters where the inner solve is inexact, next
    test); the bar holds after two."""
    K, nz, nc, _ = oracle_system
    N = nz + nc
    rng = np.random.default_rng(300 + nb)
    G = rng.standard_normal((nb, N))
    if not use_gc:
        G[:, nz:] = 0.0
    C = -np.diag(1e-5 + rng.random(nb))
    M = np.block([[K, G.T], [G, 0.5 * (C + C.T)]])
    Y, A, piv, _, singular = schur_factor(K, G, C)
    assert singular == 0
    for _ in range(3):
        rhs = rng.standard_normal(N + nb)
        om = [omega(M, refined(lambda b_: schur_solve(K, Y, A, piv, singular, b_[:N].copy(), b_[N:].copy()), M, rhs, k), rhs) for k in (0, 1, 2)]
        print(f"  nb={nb} g_c={use_gc}: omega passes 0/1/2 = {om[0]:.2e} / {om[1]:.2e} / {om[2]:.2e}, bar {_bar(M):.2e}")
        assert om[2] <= _bar(M), (nb, om)


@pytest.mark.parametrize("nb,use_gc", [(5, False), (16, True)])
def test_refined_route_repairs_an_inexact_inner_solve(nb, use_gc):
    """K^-1 applied in single precision for Y, for S and for every v0 -- the stand-in for a stored factor of wrong inertia.  The
    point and the sigmas are oracle_system's (its RNG stream, seed 9); G (standard normal), C and the right-hand side are drawn
    after them on the same stream.  Pins the sign conventions, the use of sym(C) in the product and that S built from the inexact Y
    still contracts: omega > 1e-9 without a pass, within the bar after two (seen: 5e-8 .. 7e-8, 3e-15 .. 7e-15 after one pass,
    2e-16 .. 4e-16 after two, bars 2.9e-14 / 5.0e-14)."""
    from oracle.padded_model import PaddedAcrobot, dense_kkt
    T, dw, dc = 4, 2.0, 1e-5
    nz, nc = (T - 1) * 65 + 64, (T - 1) * 64
    N = nz + nc
    rng = np.random.default_rng(9)
    z, mu = rng.random(nz), rng.random(nc)
    sx, sc = rng.random(nz) * 3.0, rng.random(nc) * 0.5
    sx[::3] = 0.0
    K, _ = dense_kkt(PaddedAcrobot(64, 1), T, z, mu, dw, dc)
    K = K + np.diag(np.concatenate([sx, -sc]))
    G = rng.standard_normal((nb, N))
    if not use_gc:
        G[:, nz:] = 0.0
    C = -np.diag(1e-5 + rng.random(nb))
    Cs = 0.5 * (C + C.T)
    M = np.block([[K, G.T], [G, Cs]])
    K32 = K.astype(np.float32)

    def kinv(X):
        return np.linalg.solve(K32, X.astype(np.float32)).astype(np.float64)
    Y = kinv(G.T).T
    P = G @ Y.T
    S = Cs - 0.5 * (P + P.T)

    def solve(b_):
        r, sb = b_[:N], b_[N:]
        v0 = kinv(r)
        y = np.linalg.solve(S, sb - Y @ r)
        return np.concatenate([v0 - Y.T @ y, y])
    for _ in range(3):
        rhs = rng.standard_normal(N + nb)
        om = [omega(M, refined(solve, M, rhs, k), rhs) for k in (0, 1, 2)]
        print(f"  nb={nb} g_c={use_gc}, single-precision K^-1: omega passes 0/1/2 = {om[0]:.2e} / {om[1]:.2e} / {om[2]:.2e}, bar {_bar(M):.2e}")
        assert om[0] > 1e-9, "the inner solve must be inexact for the case to show anything"
        assert om[2] <= _bar(M), (nb, om)

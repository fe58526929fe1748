"""dto_kkt_multiply / dto_kkt_solve_refined without a GPU: the symbols and their signatures in the header, capi.py, the Julia
shim and the INTEGRATION.md listing, the host-side argument checks of the Python wrappers, and the device error."""
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
# pointer / int64 / int32 classes of the two prototypes (include/dto.h)
WANT = {"dto_kkt_multiply": ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr"],
        "dto_kkt_solve_refined": ["ptr", "i32", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "i64", "ptr", "ptr"]}


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
    cls = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int: "i32"}
    assert [cls[t] for t in fn.argtypes] == WANT[name] and fn.restype is ctypes.c_int
    shim = _jl_types(_read("julia", "gpu_evaluator.jl"), name)
    assert shim and all(t == WANT[name] for t in shim), (name, shim)
    md = "\n\n".join(re.findall(r"```julia\n(.*?)```", _read("INTEGRATION.md"), flags=re.S))
    listing = _jl_types(md, name)
    assert listing and all(t == WANT[name] for t in listing), (name, listing)
    assert f"`{name}" in _read("README.md")


def test_python_signatures():
    mul = inspect.signature(dto_amd.Solver.kkt_multiply).parameters
    assert list(mul) == ["self", "v_x_ptr", "ldvx", "v_c_ptr", "ldvc", "out_x_ptr", "ldox", "out_c_ptr", "ldoc", "stream"]
    ref = inspect.signature(dto_amd.Solver.kkt_solve_refined).parameters
    assert list(ref) == ["self", "rhs_x_ptr", "ldrx", "rhs_c_ptr", "ldrc", "sol_x_ptr", "ldsx", "sol_c_ptr", "ldsc", "passes", "resid_ptr", "stream"]
    assert ref["resid_ptr"].default == 0 and ref["stream"].default == 0 and mul["stream"].default == 0
    assert ref["passes"].default is inspect.Parameter.empty


def test_chunk_length_of_the_tests_is_the_kernel_s():
    """tests/test_wide_kmul_gpu.py places its chunk-edge cases at T = S + 1 and S + 3 for the S of the kernel."""
    src = _read("directtrajectoryoptimization.jl_amd", "csrc", "dto_wide_kernels.hpp")
    s_kernel = int(re.search(r"#define\s+DTO_WIDE_KMUL_S\s+(\d+)", src).group(1))
    s_tests = int(re.search(r"^S = (\d+)", _read("tests", "test_wide_kmul_gpu.py"), flags=re.M).group(1))
    assert s_kernel == s_tests
    assert int(re.search(r"#define\s+DTO_PLUGIN_ABI\s+(\d+)", _read("directtrajectoryoptimization.jl_amd", "csrc", "dto_model_plugin.h")).group(1)) >= 9


def test_wrappers_reject_bad_arguments_on_the_host():
    s, _ = product_solver("pendulum", 6)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rx, rc, ox, oc = np.zeros((2, nz)), np.zeros((2, nc)), np.zeros((2, nz)), np.zeros((2, nc))
    args = (rx.ctypes.data, nz, rc.ctypes.data, nc, ox.ctypes.data, nz, oc.ctypes.data, nc)
    for bad in (-1, 5, 17):
        with pytest.raises(ValueError, match="passes"):
            s.kkt_solve_refined(*args, bad)
    for bad in (1.0, "2", None, True):
        with pytest.raises(TypeError, match="passes"):
            s.kkt_solve_refined(*args, bad)
    with pytest.raises(ValueError, match="overlap"):
        s.kkt_solve_refined(rx.ctypes.data, nz, rc.ctypes.data, nc, rx.ctypes.data, nz, oc.ctypes.data, nc, 1)
    with pytest.raises(ValueError, match="overlap"):
        s.kkt_multiply(rx.ctypes.data, nz, rc.ctypes.data, nc, ox.ctypes.data, nz, rc.ctypes.data, nc)
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_multiply(rx, nz, rc.ctypes.data, nc, ox.ctypes.data, nz, oc.ctypes.data, nc)


def test_calls_fail_with_the_device_error_without_a_gpu():
    n = ctypes.c_int(-1)
    capi.check(capi.lib().dto_device_count(ctypes.byref(n)))
    if n.value > 0:
        return  # on the GPU box the calls are exercised by tests/test_wide_kmul_gpu.py, test_wide_refined_solve_gpu.py, test_lane_kmul_gpu.py
    s, _ = product_solver("pendulum", 6)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rx, rc, ox, oc = np.zeros((2, nz)), np.zeros((2, nc)), np.zeros((2, nz)), np.zeros((2, nc))
    with pytest.raises(capi.DtoError) as e:
        s.kkt_multiply(rx.ctypes.data, nz, rc.ctypes.data, nc, ox.ctypes.data, nz, oc.ctypes.data, nc)
    assert e.value.code == 3  # DTO_ERR_DEVICE: there is no CPU fallback
    with pytest.raises(capi.DtoError) as e:
        s.kkt_solve_refined(rx.ctypes.data, nz, rc.ctypes.data, nc, ox.ctypes.data, nz, oc.ctypes.data, nc, 2)
    assert e.value.code == 3

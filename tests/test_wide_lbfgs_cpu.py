"""The limited-memory mode of the tile path without a GPU: what Options(hessian_approximation="limited-memory") means on every
solver path, what is handed to the C library, the two new entry points in the header and in capi.py, and the host-side argument
checks of their wrappers.  The device side is tests/test_wide_first_order_gpu.py, test_wide_lbfgs_border_gpu.py and
test_wide_lbfgs_solve_gpu.py."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from conftest import product_solver

import dto_amd
from dto_amd import capi, problems as P
from dto_amd import solver as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _solver(p, option, name, **kw):
    return dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=p["evaluate_hessian"],
                          general_constraint=p.get("general_constraint"), parameters=p.get("parameters"),
                          options=dto_amd.Options(hessian_approximation=option, **kw), name=name)


def test_tile_path_takes_the_limited_memory_mode_without_a_notice():
    """The acceptance row: the reference's default build of a 64-state model, Ipopt's own spelling of the mode."""
    p = P.build_acrobot_padded(T=3, evaluate_hessian=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error", S.HessianModeNotice)
        s = _solver(p, "limited-memory", "acrobot_padded")
    assert s.hessian_mode == "lbfgs" and s.solve_unsupported is None
    assert s._solve_nlp.structure.wide
    assert S._c_options(s.options, lbfgs=s.hessian_mode == "lbfgs").hessian_approximation == capi.DTO_HESSIAN_LBFGS == 1
    # ... and a problem WITH Hessians, as "lbfgs" on the lane path
    s2 = _solver(P.build_acrobot_padded(T=3), "limited-memory", "acrobot_padded")
    assert s2.hessian_mode == "lbfgs" and s2.solve_unsupported is None


def test_lane_path_reads_it_as_lbfgs():
    for eh in (False, True):
        p = P.build_pendulum(T=6, evaluate_hessian=eh)
        a, b = _solver(p, "limited-memory", "pendulum"), _solver(p, "lbfgs", "pendulum")
        assert a.hessian_mode == b.hessian_mode == "lbfgs"
        assert not a._solve_nlp.structure.wide


def test_general_rows_on_the_border_are_named_in_the_error():
    p = P.build_ref_general_coupled()
    with pytest.raises(ValueError, match=r"limited-memory.*GeneralConstraint row"):
        _solver(p, "limited-memory", "ref_general_coupled", general_rows="border")


def test_user_jacobian_dynamics_give_the_error_of_lbfgs():
    p = P.build_ref_userjac()
    msgs = []
    for option in ("lbfgs", "limited-memory"):
        with pytest.raises(ValueError, match="user-provided Jacobian") as e:
            _solver(p, option, "ref_userjac")
        msgs.append(str(e.value).replace(f"'{option}'", "<mode>"))
    assert msgs[0] == msgs[1]


def test_the_other_values_keep_their_meaning():
    with pytest.raises(ValueError, match="'limited-memory'"):
        _solver(P.build_pendulum(T=6, evaluate_hessian=True), "bfgs", "pendulum")
    p = P.build_acrobot_padded(T=3, evaluate_hessian=False)
    with pytest.raises(ValueError, match="lane-per-instance"):
        _solver(p, "lbfgs", "acrobot_padded")
    assert _solver(p, "exact", "acrobot_padded").hessian_mode == "exact-from-trace"
    # ("auto" and its one-time notice are pinned by tests/test_default_mode.py)


def test_entry_points_in_header_and_capi():
    header = re.sub(r"/\*.*?\*/", " ", _read("include", "dto.h"), flags=re.S)
    want = {"dto_kkt_assemble_first_order": 3, "dto_kkt_lbfgs_border": 11}
    for name, nargs in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        fn = getattr(capi.lib(), name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    assert int(re.search(r"#define\s+DTO_ABI_VERSION\s+(\d+)", header).group(1)) == 4 == capi.DTO_ABI_VERSION
    plug = _read("directtrajectoryoptimization.jl_amd", "csrc", "dto_model_plugin.h")
    assert int(re.search(r"#define\s+DTO_PLUGIN_ABI\s+(\d+)", plug).group(1)) >= 10
    assert re.search(r"\bint\s+first_order\s*;", _read("directtrajectoryoptimization.jl_amd", "csrc", "dto_wide_kernels.hpp"))
    full = _read("include", "dto.h")
    assert "sigma_x" in full.split("The compact limited-memory BFGS matrix")[1].split("int dto_kkt_lbfgs_border(")[0], \
        "the header says who puts sigma on the diagonal"
    assert "keep their exact-Hessian state" in full, "the header states the asymmetry of the stepwise entry points"


def test_wrappers_reject_bad_arguments_on_the_host():
    s, _ = product_solver("acrobot_padded", 3)
    nz = s.nlp.num_variables
    a = np.zeros((2 * 6, nz))
    ap = a.ctypes.data
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_assemble_first_order(a, 2, nz, 1.0, 1e-8)
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_assemble_first_order(ap, 2, nz, 1.0, 1e-8, sigma_x_ptr=1.5, ldsx=nz)
    with pytest.raises(ValueError, match="positive integer"):
        s.kkt_assemble_first_order(ap, 0, nz, 1.0, 1e-8)
    s = _solver(P.build_acrobot_padded(T=3), "exact", "acrobot_padded")   # (a Solver of this test's own: _B is set by hand below)
    s._B = 2
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_lbfgs_border(6, a, nz, ap + 8, nz, (1.0, 1.0))
    with pytest.raises(TypeError, match="device pointers"):
        s.kkt_lbfgs_border(6.0, ap, nz, ap + 8, nz, (1.0, 1.0))
    with pytest.raises(ValueError, match="one entry per instance"):
        s.kkt_lbfgs_border(6, ap, nz, ap + 8, nz, (1.0, 1.0, 1.0))
    for bad in ((1.0, 0.0), (1.0, -2.0), (float("nan"), 1.0), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="positive and finite"):
            s.kkt_lbfgs_border(6, ap, nz, ap + 8, nz, bad)
    for bad in ((6, 7), (-1, 0), (1, 2, 3), (1.5, 2.0)):
        with pytest.raises(ValueError, match="npairs"):
            s.kkt_lbfgs_border(6, ap, nz, ap + 8, nz, (1.0, 1.0), npairs=bad)
    with pytest.raises(ValueError, match="two arrays"):
        s.kkt_lbfgs_border(6, ap, nz, ap, nz, (1.0, 1.0))


def test_calls_fail_loudly_without_a_gpu():
    n = ctypes.c_int(-1)
    capi.check(capi.lib().dto_device_count(ctypes.byref(n)))
    if n.value > 0:
        return  # on the GPU box the calls are exercised by the three GPU test files
    s, _ = product_solver("acrobot_padded", 3)
    nz = s.nlp.num_variables
    a = np.zeros((2 * 6, nz))
    with pytest.raises(capi.DtoError) as e:
        s.kkt_assemble_first_order(a.ctypes.data, 2, nz, 1.0, 1e-8)
    assert e.value.code in (1, 3)   # DTO_ERR_DEVICE (there is no CPU fallback) or DTO_ERR_INVALID
    s = _solver(P.build_acrobot_padded(T=3), "exact", "acrobot_padded")   # (a Solver of this test's own: _B is set by hand)
    s._B = 2
    with pytest.raises(capi.DtoError) as e:
        s.kkt_lbfgs_border(6, a.ctypes.data, nz, a.ctypes.data + 8, nz, (1.0, 1.0))
    assert e.value.code in (1, 3)

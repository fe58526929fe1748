"""The limited-memory mode of the tile path beside coupling GeneralConstraint rows, without a GPU: which problems
Options(hessian_approximation="limited-memory") takes (at most four rows left on the border), the new entry point in the header
and in capi.py, and the host-side argument checks of its wrapper.  The device side is tests/test_wide_lbfgs_rows_border_gpu.py and
tests/test_wide_lbfgs_rows_solve_gpu.py."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import dto_amd
from dto_amd import capi, problems as P
from dto_amd import solver as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEP_ROWS = [(2, 5, 0.2), (3, 6, 0.1, False, "product")]                      # the rows of tests/test_wide_general_border_gpu.py
FIVE_ROWS = [(a, b, 0.1 * (j + 1)) for j, (a, b) in enumerate([(1, 2), (1, 3), (1, 4), (1, 5), (1, 6)])]


def _solver(rows, option, name, n=64, **kw):
    p = P.build_acrobot_padded(T=6, n=n, general_row=list(rows), **({} if n == 64 else dict(target=0.4, terminal="physical")))
    return dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                          general_constraint=p["general_constraint"], name=name,
                          options=dto_amd.Options(hessian_approximation=option, **kw))


def test_up_to_four_rows_on_the_tile_border_take_the_mode():
    with warnings.catch_warnings():
        warnings.simplefilter("error", S.HessianModeNotice)
        s = _solver(STEP_ROWS, "limited-memory", "acrobot_padded_g_m1")
    assert s.hessian_mode == "lbfgs" and s.general_rows_path == "border" and s.solve_unsupported is None
    assert s._solve_nlp.structure.wide and s._solve_nlp.num_constraint == 5 * 64 + 2
    assert S._c_options(s.options, lbfgs=s.hessian_mode == "lbfgs").hessian_approximation == capi.DTO_HESSIAN_LBFGS == 1
    assert S.TILE_LBFGS_MAX_ROWS == 4


def test_a_row_of_the_embedding_takes_it_too():
    s = _solver([(2, 5, 0.2, False, "product")], "limited-memory", "acrobot24gp", n=24)
    assert s.hessian_mode == "lbfgs" and s.general_rows_path == "border" and s.solve_unsupported is None
    assert s._solve_nlp.structure.wide


def test_five_rows_name_the_limit_of_four():
    with pytest.raises(ValueError, match=r"limited-memory.*at most 4\b"):
        _solver(FIVE_ROWS, "limited-memory", "acrobot_padded_g5")
    # ... and the exact mode takes the same problem
    assert _solver(FIVE_ROWS, "exact", "acrobot_padded_g5").hessian_mode == "exact"


def test_auto_keeps_its_substitute_beside_rows():
    p = P.build_acrobot_padded(T=6, general_row=list(STEP_ROWS), evaluate_hessian=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", S.HessianModeNotice)
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=False,
                           general_constraint=p["general_constraint"], name="acrobot_padded_g_m1",
                           options=dto_amd.Options(hessian_approximation="auto"))
    assert s.hessian_mode == "exact-from-trace" and s.general_rows_path == "border"


def test_entry_point_in_header_and_capi():
    full = open(os.path.join(ROOT, "include", "dto.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", full, flags=re.S)
    m = re.search(r"\bint\s+dto_kkt_lbfgs_border_rows\s*\(([^;{]*?)\)\s*;", header, flags=re.S)
    assert m and len(m.group(1).split(",")) == 18
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["p", "m", "s", "lds", "y", "ldy", "npairs", "sigma", "nr", "g_x", "ldgx", "g_c", "ldgc", "c", "ldc", "inertia_ok",
                     "schur_singular", "stream"]
    fn = capi.lib().dto_kkt_lbfgs_border_rows
    assert len(fn.argtypes) == 18 and fn.restype is ctypes.c_int
    assert fn.argtypes[8] is ctypes.c_int64 and fn.argtypes[6] is capi.c_int32_p and fn.argtypes[7] is capi.c_double_p
    assert int(re.search(r"#define\s+DTO_ABI_VERSION\s+(\d+)", header).group(1)) == capi.DTO_ABI_VERSION
    doc = full.split("int dto_kkt_lbfgs_border(")[1].split("int dto_kkt_lbfgs_border_rows(")[0]
    assert "neg(M) + nr" in doc and "2 m + nr > 16" in doc, "the header states the inertia rule and the size of the panel"
    flat = re.sub(r"\s*\n\s*\*\s*", " ", full)                           # (a comment's line breaks)
    assert "at most four coupling rows in limited-memory mode on the tile path" in flat


def _own_solver():
    s = _solver(STEP_ROWS, "exact", "acrobot_padded_g_m1")   # (a Solver of this test's own: _B is set by hand)
    s._B = 2
    return s


def test_wrapper_rejects_bad_arguments_on_the_host():
    s = _own_solver()
    nz = s.nlp.num_variables
    a = np.zeros((2 * 6 + 2 + 1, nz))
    ap = a.ctypes.data
    rows = lambda **kw: dict(dict(m=6, s_ptr=ap, lds=nz, y_ptr=ap + 8, ldy=nz, sigma=(1.0, 1.0), nr=1, gx_ptr=ap + 16, ldgx=nz, c_ptr=ap + 24,
                                  ldc=1), **kw)
    for bad in (dict(s_ptr=a), dict(m=6.0), dict(nr=1.0), dict(gx_ptr=a), dict(c_ptr=2.5), dict(gc_ptr=a), dict(nr=True)):
        with pytest.raises(TypeError, match="device pointers"):
            s.kkt_lbfgs_border_rows(**rows(**bad))
    with pytest.raises(ValueError, match="non-negative"):
        s.kkt_lbfgs_border_rows(**rows(nr=-1))
    with pytest.raises(ValueError, match="one entry per instance"):
        s.kkt_lbfgs_border_rows(**rows(sigma=(1.0, 1.0, 1.0)))
    for bad in ((1.0, 0.0), (1.0, -2.0), (float("nan"), 1.0), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="positive and finite"):
            s.kkt_lbfgs_border_rows(**rows(sigma=bad))
    for bad in ((6, 7), (-1, 0), (1, 2, 3), (1.5, 2.0)):
        with pytest.raises(ValueError, match="npairs"):
            s.kkt_lbfgs_border_rows(**rows(npairs=bad))
    with pytest.raises(ValueError, match="two arrays"):
        s.kkt_lbfgs_border_rows(**rows(y_ptr=ap))
    for bad in (dict(gx_ptr=0), dict(c_ptr=0)):
        with pytest.raises(ValueError, match="needs the rows"):
            s.kkt_lbfgs_border_rows(**rows(**bad))


def test_call_fails_loudly_without_a_gpu():
    n = ctypes.c_int(-1)
    capi.check(capi.lib().dto_device_count(ctypes.byref(n)))
    if n.value > 0:
        return  # on the GPU box the call is exercised by tests/test_wide_lbfgs_rows_border_gpu.py
    s = _own_solver()
    nz = s.nlp.num_variables
    a = np.zeros((2 * 6 + 2, nz))
    ap = a.ctypes.data
    with pytest.raises(capi.DtoError) as e:
        s.kkt_lbfgs_border_rows(6, ap, nz, ap + 8, nz, (1.0, 1.0), 1, ap + 16, nz, ap + 24, 1)
    assert e.value.code in (1, 3)   # DTO_ERR_DEVICE (there is no CPU fallback) or DTO_ERR_INVALID

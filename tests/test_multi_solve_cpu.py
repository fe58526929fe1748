"""dto_kkt_solve_multi without a GPU: the symbol, the Python signature, the row rule of its arrays, and the device error."""
import ctypes
import inspect
import re

import numpy as np
import pytest

from conftest import product_solver

import dto_amd
from dto_amd import capi


def test_symbol_is_exported_with_its_signature():
    lib = capi.lib()
    assert hasattr(lib, "dto_kkt_solve_multi")
    assert len(lib.dto_kkt_solve_multi.argtypes) == 11 and lib.dto_kkt_solve_multi.argtypes[1] is ctypes.c_int64


def test_python_signature():
    params = list(inspect.signature(dto_amd.Solver.kkt_solve_multi).parameters)
    assert params == ["self", "nrhs", "rhs_x_ptr", "ldrx", "rhs_c_ptr", "ldrc", "sol_x_ptr", "ldsx", "sol_c_ptr", "ldsc", "stream"]
    assert inspect.signature(dto_amd.Solver.kkt_solve_multi).parameters["stream"].default == 0


def test_row_rule_matches_the_docstring_example():
    """[B][nrhs][n] flattened to [B * nrhs][n] puts right-hand side r of instance b into row b * nrhs + r; the example of the
    docstring is an instance of that rule."""
    doc = inspect.getdoc(dto_amd.Solver.kkt_solve_multi)
    assert "b * nrhs + r" in doc
    B, nrhs, n = 4, 3, 5
    a = np.arange(B * nrhs * n).reshape(B, nrhs, n)
    flat = a.reshape(B * nrhs, n)
    for b in range(B):
        for r in range(nrhs):
            assert np.array_equal(flat[b * nrhs + r], a[b, r])
    m = re.search(r"B = (\d+) and nrhs = (\d+), right-hand side (\d+) of instance (\d+)\s+is row (\d+)", doc)
    assert m, "the docstring gives an example of the row rule"
    eB, en, er, eb, erow = (int(v) for v in m.groups())
    assert eb < eB and er < en and erow == eb * en + er


def test_call_fails_with_the_device_error_without_a_gpu():
    n = ctypes.c_int(-1)
    capi.check(capi.lib().dto_device_count(ctypes.byref(n)))
    if n.value > 0:
        return  # on the GPU box the call is exercised by tests/test_wide_multi_solve_gpu.py and tests/test_lane_multi_solve_gpu.py
    s, _ = product_solver("pendulum", 6)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rx, rc, ox, oc = np.zeros((2, nz)), np.zeros((2, nc)), np.zeros((2, nz)), np.zeros((2, nc))
    with pytest.raises(capi.DtoError) as e:
        s.kkt_solve_multi(2, rx.ctypes.data, nz, rc.ctypes.data, nc, ox.ctypes.data, nz, oc.ctypes.data, nc)
    assert e.value.code == 3  # DTO_ERR_DEVICE: there is no CPU fallback

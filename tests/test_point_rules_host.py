"""The per-entry rules of a warm start from a caller's primal-dual point and of a receding-horizon shift
(csrc/dto_point_rules.hpp: warm_var, warm_slack, shift_source -- shared by k_wide_init_warm, k_wide_shift_knots and the kernels of
dto_solve_batch_warm / dto_point_shift), checked on the host, and the layout of dto_point.

tests/host/point_rules_main.cpp includes the header alone, is built for the host only and run under the address and
undefined-behaviour sanitizers; its expected values are worked out by hand from the rules stated in include/dto.h.  It calls no HIP
function and needs no GPU.
"""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_point_rules_on_the_host(tmp_path):
    exe = str(tmp_path / "point_rules_main")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "directtrajectoryoptimization.jl_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "host", "point_rules_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("point rules ok"), (r.returncode, r.stdout, r.stderr[-4000:])


def test_dto_point_has_the_c_compilers_layout(tmp_path):
    """capi.CPoint against a C99 program that includes include/dto.h: size and the offset of every field."""
    import dto_amd  # noqa: F401
    from dto_amd import capi
    names = [n for n, _ in capi.CPoint._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "dto.h"\nint main(void) {\n  printf("%zu", sizeof(dto_point));\n'
    src += "".join(f'  printf(" %zu", offsetof(dto_point, {n}));\n' for n in names)
    src += '  printf("\\n");\n  return 0;\n}\n'
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(capi.CPoint)
    assert out[1:] == [getattr(capi.CPoint, n).offset for n in names]
    assert names == ["x", "ldx", "mu", "ldmu", "zl", "ldzl", "zu", "ldzu", "slack", "ldslack", "barrier", "qn_s", "ldqs", "qn_y", "ldqy",
                     "qn_npairs", "qn_sigma"]
    lib = capi.lib()
    assert hasattr(lib, "dto_solve_batch_warm") and hasattr(lib, "dto_point_shift")

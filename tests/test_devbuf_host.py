"""DevBuf (csrc/dto_problem.hpp), the one owner of device memory in the runtime library, checked on the host.

tests/host/devbuf_main.cpp includes the header and replaces hipMalloc / hipFree / hipMemset by malloc-backed stubs that count live
allocations and can fail the next one; it is built WITHOUT the HIP runtime and run under the address and undefined-behaviour
sanitizers, so a leak, a double free or a read of a moved-from buffer ends the run with a nonzero status.  This is also the cover of
the failure paths of ensure_state / ensure_im_state (a failed set-up leaves an empty state): exhausting the memory of a GPU to reach
them is not something a test does.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_owns_frees_and_reports(tmp_path):
    exe = str(tmp_path / "devbuf_main")
    subprocess.run(["g++", "-std=c++17", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "devbuf_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "devbuf ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-4000:])

"""The step-acceptance rules that the two host-driven solver loops share (csrc/dto_host_globalization.hpp: trial acceptance, filter
ring, fallback step, termination ladder, delta_w ladder, monotone barrier update), checked on the host.

tests/host/globalization_main.cpp includes the header next to dto_kkt_kernels.hpp (the option struct and the ring size), is built
for the host only and run under the address and undefined-behaviour sanitizers; its expected values are worked out by hand from
Waechter & Biegler's Algorithm A.  It calls no HIP function and needs no GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_globalization_rules(tmp_path):
    exe = str(tmp_path / "globalization_main")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "directtrajectoryoptimization.jl_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "globalization_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("globalization ok"), (r.returncode, r.stdout, r.stderr[-4000:])

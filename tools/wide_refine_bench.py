"""Timing of the product y = K v and of the refined solve on the tile path: python tools/wide_refine_bench.py [T] [B] [reps]

dto_kkt_multiply, dto_kkt_solve, dto_kkt_solve_refined with one and with two passes, and dto_kkt_factor at one point,
alternating, HIP events on the stream, two warm-up rounds, medians of `reps` rounds with the minimum and maximum beside them
(the run-to-run spread).  One JSON line: the times, the product's traffic over its time (per instance it reads the point, the
multipliers, v and the sigmas and writes the product; the constant Jacobian table comes from the L2), the cost of a refinement
pass relative to a solve and to a factorisation, and the chunk length of the product's grid (DTO_WIDE_KMUL_S in the
environment overrides the kernel's default for this process: run once per value to compare them)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import dto_amd
from dto_amd import problems as P

T = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
assert torch.cuda.is_available(), "needs a GPU"
p = P.build_acrobot_padded(T=T)
s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
nz, nc = s.nlp.num_variables, s.nlp.num_constraint
g = torch.Generator(device="cuda"); g.manual_seed(0)
Z = torch.rand((B, nz), device="cuda", dtype=torch.float64, generator=g)
MU = torch.rand((B, nc), device="cuda", dtype=torch.float64, generator=g)
SX = torch.rand((B, nz), device="cuda", dtype=torch.float64, generator=g)
SC = torch.rand((B, nc), device="cuda", dtype=torch.float64, generator=g)
RX = torch.randn((B, nz), device="cuda", dtype=torch.float64, generator=g)
RC = torch.randn((B, nc), device="cuda", dtype=torch.float64, generator=g)
kx, kc, ox, oc = torch.empty_like(Z), torch.empty_like(MU), torch.empty_like(Z), torch.empty_like(MU)
resid = torch.empty((B,), device="cuda", dtype=torch.float64)
dw, dc = 2.0, 1e-5


def multiply():
    s.kkt_multiply(RX.data_ptr(), nz, RC.data_ptr(), nc, kx.data_ptr(), nz, kc.data_ptr(), nc)


def solve():
    s.kkt_solve(RX.data_ptr(), nz, RC.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc)


def refined(passes):
    return lambda: s.kkt_solve_refined(RX.data_ptr(), nz, RC.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc, passes)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


s.kkt_assemble(Z.data_ptr(), B, nz, MU.data_ptr(), nc, dw, dc, sigma_x_ptr=SX.data_ptr(), ldsx=nz, sigma_c_ptr=SC.data_ptr(), ldsc=nc)
entries = dict(factor=s.kkt_factor, multiply=multiply, solve=solve, refined1=refined(1), refined2=refined(2))
times = {k: [] for k in entries}
for it in range(2 + reps):
    for k, fn in entries.items():
        dt = timed(fn)
        if it >= 2:
            times[k].append(dt)
s.kkt_solve_refined(RX.data_ptr(), nz, RC.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc, 2, resid_ptr=resid.data_ptr())
torch.cuda.synchronize()
ok = bool(torch.isfinite(ox).all().item() and torch.isfinite(oc).all().item() and torch.isfinite(kx).all().item())
med = {k: float(np.median(v)) for k, v in times.items()}
out = dict(T=T, B=B, reps=reps, finite=ok, kmul_s=int(os.environ.get("DTO_WIDE_KMUL_S", "0")) or "default",
           max_resid_2_passes=float(resid.max().item()))
for k in entries:
    out[k + "_s"] = round(med[k], 6); out[k + "_min_s"] = round(min(times[k]), 6); out[k + "_max_s"] = round(max(times[k]), 6)
mul_bytes = B * 8 * (4 * nz + 4 * nc)   # reads z, v_x, sigma_x [nz], mu, v_c, sigma_c [nc]; writes out_x [nz], out_c [nc]
pass1 = med["refined1"] - med["solve"]
out.update(multiply_GB=round(mul_bytes / 1e9, 3), multiply_GBps=round(mul_bytes / med["multiply"] / 1e9, 1),
           pass_s=round(pass1, 6), pass_over_solve=round(pass1 / med["solve"], 3), pass_over_factor=round(pass1 / med["factor"], 4),
           multiply_over_solve=round(med["multiply"] / med["solve"], 3))
print(json.dumps(out))

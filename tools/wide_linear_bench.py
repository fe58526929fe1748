"""Timing of the linear solver alone on the tile path against the KKT step: python tools/wide_linear_bench.py [T] [B] [reps]

dto_kkt_step_batch (factor + solve in one sweep pair), dto_kkt_factor (factor into the stored records) and dto_kkt_solve
(substitution only: k_wide_fsub + k_wide_bwd) at the same point, alternating, HIP events on the stream, two warm-up rounds.
One JSON line: median and minimum per entry point, the solve / step ratio, and the traffic of a solve (the records are read
twice) over its time."""
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
RX = torch.randn((B, nz), device="cuda", dtype=torch.float64, generator=g)
RC = torch.randn((B, nc), device="cuda", dtype=torch.float64, generator=g)
dx, dl, ox, oc = torch.empty_like(Z), torch.empty_like(MU), torch.empty_like(Z), torch.empty_like(MU)
dw, dc = 2.0, 1e-5


def step():
    # (inertia_ok is read back: one synchronise inside the call, as in the figure of DESIGN.md section 0)
    return s.kkt_step_batch(Z.data_ptr(), B, nz, MU.data_ptr(), nc, dw, dc, dx.data_ptr(), nz, dl.data_ptr(), nc)


def solve():
    s.kkt_solve(RX.data_ptr(), nz, RC.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


s.kkt_assemble(Z.data_ptr(), B, nz, MU.data_ptr(), nc, dw, dc)
times = dict(step=[], factor=[], solve=[])
for it in range(2 + reps):
    t_step = timed(step)                 # (writes the shared records: the factor below is needed again anyway)
    t_fac = timed(s.kkt_factor)
    t_sol = [timed(solve), timed(solve)]   # two right-hand sides per factor
    if it >= 2:
        times["step"].append(t_step); times["factor"].append(t_fac); times["solve"] += t_sol
ok = bool(torch.isfinite(ox).all().item() and torch.isfinite(oc).all().item())
med = {k: float(np.median(v)) for k, v in times.items()}
rec_bytes = B * (T - 1) * 18128 * 8   # Dims<64, 1>::FAC doubles per stage and instance (csrc/dto_wide_kernels.hpp)
print(json.dumps(dict(T=T, B=B, reps=reps, finite=ok,
                      step_s=round(med["step"], 5), factor_s=round(med["factor"], 5), solve_s=round(med["solve"], 5),
                      step_min_s=round(min(times["step"]), 5), factor_min_s=round(min(times["factor"]), 5), solve_min_s=round(min(times["solve"]), 5),
                      solve_over_step=round(med["solve"] / med["step"], 4),
                      solve_read_GB=round(2 * rec_bytes / 1e9, 2), solve_GBps=round(2 * rec_bytes / med["solve"] / 1e9, 1))))

"""dto_kkt_border_factor / dto_kkt_border_solve on the tile path against what a caller had to do without them:
python tools/wide_border_bench.py [T] [B] [nb] [reps]

HIP events on the stream, two warm-up rounds, medians of `reps` rounds with the minimum and maximum beside them.  One JSON line:
  * border_factor: the whole call; multi_solve: dto_kkt_solve_multi(nb) alone on arrays of the same shape; their difference is the
    two panel copies, k_border_gram, k_border_schur and the wait for the stream -- an upper bound of the two kernels, and
    gram_GBps_at_least = (2 x nb x N doubles per instance) over that difference against the HBM peak (a kernel trace,
    rocprofv3 --kernel-trace --stats, gives the kernels alone);
  * border_solve against a plain dto_kkt_solve on the same right-hand side;
  * parent: nb + 1 dto_kkt_solve calls plus the copy of Y = K^-1 G' to the host (the Schur complement was the host's job), per
    bordered right-hand side; the border calls amortise the nb solves over every right-hand side that follows;
  * border_multiply (dto_kkt_border_multiply) against a plain dto_kkt_multiply on the same vector: their difference is k_border_mul
    + k_border_mul_fin, the one pass over the kept panel -- mul_panel_GBps_at_least = (nb x N doubles per instance) over that
    difference against the HBM peak;
  * border_refined1: dto_kkt_border_solve_refined(passes = 1); its excess over border_solve is one refinement pass (product,
    residual, bordered solve of the residual, update), reported relative to one dto_kkt_border_solve and to one dto_kkt_factor."""
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
nb = int(sys.argv[3]) if len(sys.argv) > 3 else 12
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
HBM_PEAK_GBPS = 8000.0   # MI355X
assert torch.cuda.is_available(), "needs a GPU"
p = P.build_acrobot_padded(T=T)
s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
nz, nc = s.nlp.num_variables, s.nlp.num_constraint
N = nz + nc
g = torch.Generator(device="cuda"); g.manual_seed(0)
Z = torch.rand((B, nz), device="cuda", dtype=torch.float64, generator=g)
MU = torch.rand((B, nc), device="cuda", dtype=torch.float64, generator=g)
s.kkt_assemble(Z.data_ptr(), B, nz, MU.data_ptr(), nc, 2.0, 1e-5)
ok, _ = s.kkt_factor()
assert np.all(ok == 1)
GX = torch.randn((B * nb, nz), device="cuda", dtype=torch.float64, generator=g)
GC = torch.randn((B * nb, nc), device="cuda", dtype=torch.float64, generator=g)
C = -torch.eye(nb, device="cuda", dtype=torch.float64).reshape(1, nb * nb).repeat(B, 1)
YX, YC = torch.empty_like(GX), torch.empty_like(GC)
RX = torch.randn((B, nz), device="cuda", dtype=torch.float64, generator=g)
RC = torch.randn((B, nc), device="cuda", dtype=torch.float64, generator=g)
RB = torch.randn((B, nb), device="cuda", dtype=torch.float64, generator=g)
OX, OC, OB = torch.empty_like(RX), torch.empty_like(RC), torch.empty_like(RB)
PX, PC = torch.empty_like(RX), torch.empty_like(RC)
MX, MC, MB = torch.empty_like(RX), torch.empty_like(RC), torch.empty_like(RB)
KX, KC = torch.empty_like(RX), torch.empty_like(RC)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def border_factor():
    s.kkt_border_factor(nb, GX.data_ptr(), nz, GC.data_ptr(), nc, C.data_ptr(), nb * nb)


def multi_solve():
    s.kkt_solve_multi(nb, GX.data_ptr(), nz, GC.data_ptr(), nc, YX.data_ptr(), nz, YC.data_ptr(), nc)


def border_solve():
    s.kkt_border_solve(RX.data_ptr(), nz, RC.data_ptr(), nc, RB.data_ptr(), nb, OX.data_ptr(), nz, OC.data_ptr(), nc, OB.data_ptr(), nb)


def plain_solve():
    s.kkt_solve(RX.data_ptr(), nz, RC.data_ptr(), nc, PX.data_ptr(), nz, PC.data_ptr(), nc)


def parent():
    for r in range(nb):
        s.kkt_solve(GX.data_ptr() + 8 * r * nz, nb * nz, GC.data_ptr() + 8 * r * nc, nb * nc,
                    YX.data_ptr() + 8 * r * nz, nb * nz, YC.data_ptr() + 8 * r * nc, nb * nc)
    plain_solve()
    return YX.cpu(), YC.cpu()


def border_multiply():
    s.kkt_border_multiply(RX.data_ptr(), nz, RC.data_ptr(), nc, RB.data_ptr(), nb, MX.data_ptr(), nz, MC.data_ptr(), nc, MB.data_ptr(), nb)


def plain_multiply():
    s.kkt_multiply(RX.data_ptr(), nz, RC.data_ptr(), nc, KX.data_ptr(), nz, KC.data_ptr(), nc)


def border_refined1():
    s.kkt_border_solve_refined(RX.data_ptr(), nz, RC.data_ptr(), nc, RB.data_ptr(), nb, OX.data_ptr(), nz, OC.data_ptr(), nc, OB.data_ptr(), nb, 1)


def kkt_factor():
    s.kkt_factor()
    border_factor()          # (a new factorisation invalidates the border: put it back, outside the figure -- see factor_s below)


what = dict(border_factor=border_factor, multi_solve=multi_solve, border_solve=border_solve, plain_solve=plain_solve, parent=parent,
            border_multiply=border_multiply, plain_multiply=plain_multiply, border_refined1=border_refined1,
            factor_and_border_factor=kkt_factor)
times = {k: [] for k in what}
for it in range(2 + reps):
    for k, fn in what.items():
        t = timed(fn)
        if it >= 2:
            times[k].append(t)
out = dict(T=T, B=B, nb=nb, N=N, reps=reps)
for k, v in times.items():
    out[k + "_s"] = round(float(np.median(v)), 6)
    out[k + "_min_s"] = round(min(v), 6)
    out[k + "_max_s"] = round(max(v), 6)
rest = out["border_factor_s"] - out["multi_solve_s"]
gram_bytes = 2.0 * nb * N * 8 * B
out["factor_minus_multi_s"] = round(rest, 6)
out["gram_read_GB"] = round(gram_bytes / 1e9, 3)
if rest > 0:
    out["gram_GBps_at_least"] = round(gram_bytes / rest / 1e9, 1)
    out["gram_fraction_of_hbm_peak_at_least"] = round(gram_bytes / rest / 1e9 / HBM_PEAK_GBPS, 3)
out["border_solve_over_plain_solve"] = round(out["border_solve_s"] / out["plain_solve_s"], 3)
out["parent_over_border_solve"] = round(out["parent_s"] / out["border_solve_s"], 2)
mul_rest = out["border_multiply_s"] - out["plain_multiply_s"]
panel_bytes = 1.0 * nb * N * 8 * B
out["mul_minus_plain_mul_s"] = round(mul_rest, 6)
out["mul_panel_read_GB"] = round(panel_bytes / 1e9, 3)
if mul_rest > 0:
    out["mul_panel_GBps_at_least"] = round(panel_bytes / mul_rest / 1e9, 1)
    out["mul_panel_fraction_of_hbm_peak_at_least"] = round(panel_bytes / mul_rest / 1e9 / HBM_PEAK_GBPS, 3)
out["factor_s"] = round(out["factor_and_border_factor_s"] - out["border_factor_s"], 6)
one_pass = out["border_refined1_s"] - out["border_solve_s"]
out["refine_pass_s"] = round(one_pass, 6)
out["refine_pass_over_border_solve"] = round(one_pass / out["border_solve_s"], 3)
if out["factor_s"] > 0:
    out["refine_pass_over_factor"] = round(one_pass / out["factor_s"], 3)
print(json.dumps(out), flush=True)

"""dto_kkt_solve_multi against nrhs consecutive dto_kkt_solve calls on one factorisation (tile path):
python tools/wide_multi_bench.py [T] [B] [reps] [nrhs,nrhs,...]

Both on the same stored records and the same right-hand sides (column r of the sequential run is row b * nrhs + r of the
multi-solve's arrays, passed with the leading dimension nrhs * n), HIP events on the stream, two warm-up rounds, alternating,
medians of `reps` rounds with the minimum and maximum beside them (the run-to-run spread).  One JSON line per nrhs: the two
times, their ratio, the largest difference of the two results, and the record traffic of one block of columns (the records are
read once forward and once backward) over its time."""
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
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
counts = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1, 16, 64]
BLOCK = 16   # columns per pass over the records (csrc/dto_wide_kernels.hpp: DTO_WIDE_MULTI_R)
assert torch.cuda.is_available(), "needs a GPU"
p = P.build_acrobot_padded(T=T)
s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
nz, nc = s.nlp.num_variables, s.nlp.num_constraint
g = torch.Generator(device="cuda"); g.manual_seed(0)
Z = torch.rand((B, nz), device="cuda", dtype=torch.float64, generator=g)
MU = torch.rand((B, nc), device="cuda", dtype=torch.float64, generator=g)
s.kkt_assemble(Z.data_ptr(), B, nz, MU.data_ptr(), nc, 2.0, 1e-5)
ok, _ = s.kkt_factor()
assert np.all(ok == 1)
rec_bytes = B * (T - 1) * 18128 * 8   # Dims<64, 1>::FAC doubles per stage and instance (csrc/dto_wide_kernels.hpp)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


for nrhs in counts:
    RX = torch.randn((B * nrhs, nz), device="cuda", dtype=torch.float64, generator=g)
    RC = torch.randn((B * nrhs, nc), device="cuda", dtype=torch.float64, generator=g)
    mx, mc, qx, qc = torch.empty_like(RX), torch.empty_like(RC), torch.empty_like(RX), torch.empty_like(RC)

    def multi():
        s.kkt_solve_multi(nrhs, RX.data_ptr(), nz, RC.data_ptr(), nc, mx.data_ptr(), nz, mc.data_ptr(), nc)

    def sequential():
        for r in range(nrhs):
            s.kkt_solve(RX.data_ptr() + 8 * r * nz, nrhs * nz, RC.data_ptr() + 8 * r * nc, nrhs * nc,
                        qx.data_ptr() + 8 * r * nz, nrhs * nz, qc.data_ptr() + 8 * r * nc, nrhs * nc)

    tm, tq = [], []
    for it in range(2 + reps):
        a, b = timed(multi), timed(sequential)
        if it >= 2:
            tm.append(a); tq.append(b)
    diff = max(float((mx - qx).abs().max()), float((mc - qc).abs().max()))
    scale = max(float(qx.abs().max()), float(qc.abs().max()))
    m, q = float(np.median(tm)), float(np.median(tq))
    blocks = (nrhs + BLOCK - 1) // BLOCK
    print(json.dumps(dict(T=T, B=B, nrhs=nrhs, reps=reps, multi_s=round(m, 5), multi_min_s=round(min(tm), 5), multi_max_s=round(max(tm), 5),
                          sequential_s=round(q, 5), sequential_min_s=round(min(tq), 5), sequential_max_s=round(max(tq), 5),
                          sequential_over_multi=round(q / m, 3), max_difference=diff, solution_scale=scale,
                          block_read_GB=round(2 * rec_bytes / 1e9, 2), block_GBps=round(2 * rec_bytes * blocks / m / 1e9, 1))), flush=True)
    del RX, RC, mx, mc, qx, qc

"""Limited-memory mode of the tile path: time of one outer iteration against the exact mode on the same tree, and of the compact
border alone (dto_kkt_lbfgs_border).  For the record, no claim and no threshold.

    python tools/wide_lbfgs_bench.py --T 16 --B 3 --iters 20
    python tools/wide_lbfgs_bench.py --T 2000 --B 8 --iters 10

One JSON line: ms per outer iteration of solve_batch stopped at max_iter = iters in both modes (the second of two runs, so that
allocations are paid), and ms per dto_kkt_lbfgs_border call with a full history of 6 pairs (median of `reps`)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--B", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import dto_amd
    from dto_amd import problems as P
    out = dict(T=a.T, B=a.B, iters=a.iters)
    p = P.build_acrobot_padded(T=a.T, target=0.5, terminal="physical")
    for mode in ("limited-memory", "exact"):
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                           options=dto_amd.Options(hessian_approximation=mode, max_iter=a.iters), name="acrobot_padded")
        nz, nc = s.nlp.num_variables, s.nlp.num_constraint
        Z = np.zeros((a.B, nz))
        for b in range(a.B):
            xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
            dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
            Z[b] = s._z0
        z0 = torch.tensor(Z, device="cuda")
        zo = torch.empty((a.B, nz), device="cuda", dtype=torch.float64)
        lo = torch.empty((a.B, nc), device="cuda", dtype=torch.float64)
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            status, iters = s.solve_batch(z0.data_ptr(), a.B, nz, zo.data_ptr(), nz, lo.data_ptr(), nc)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        out[mode] = dict(ms_per_iteration=1e3 * dt / max(1, int(np.max(iters))), iterations=[int(v) for v in iters],
                         mode=s.hessian_mode_last())
        if mode == "limited-memory":
            rng = np.random.default_rng(0)
            S = torch.tensor(rng.standard_normal((a.B * 6, nz)), device="cuda")
            Y = 0.3 * S + 0.05 * torch.tensor(rng.standard_normal((a.B * 6, nz)), device="cuda")
            sx = torch.full((a.B, nz), 1.0, device="cuda", dtype=torch.float64)
            s.kkt_assemble_first_order(z0.data_ptr(), a.B, nz, 1.0, 1e-8, sigma_x_ptr=sx.data_ptr(), ldsx=nz)
            s.kkt_factor()
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.kkt_lbfgs_border(6, S.data_ptr(), nz, Y.data_ptr(), nz, [1.0] * a.B)
                ts.append(1e3 * (time.perf_counter() - t0))
            out["lbfgs_border_ms"] = float(np.median(ts))
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

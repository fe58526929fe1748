"""Limited-memory mode of the tile path: time of one outer iteration against the exact mode on the same tree, and of the compact
border alone (dto_kkt_lbfgs_border / dto_kkt_lbfgs_border_rows).  For the record, no claim and no threshold.

    python tools/wide_lbfgs_bench.py --T 16 --B 3 --iters 20
    python tools/wide_lbfgs_bench.py --T 2000 --B 8 --iters 10
    python tools/wide_lbfgs_bench.py --T 16 --B 3 --iters 20 --general-row
    python tools/wide_lbfgs_bench.py --T 16 --B 3 --warm

--general-row: the same problem with one coupling GeneralConstraint row, q1[T // 3] + q1[2 T // 3] = 0.2, left on the border -- the
limited-memory mode then runs 13 border rows, the exact mode the row alone.

--warm: in place of the per-iteration figures, whole limited-memory solves to convergence through dto_solve_batch_warm -- cold from
the guesses, then warm from the converged point with x perturbed by 1e-3 (relative to max |x|), with the history in the point and
without it: ms per solve (median of `reps` after one run that pays the allocations) and the iteration counts.

One JSON line: ms per outer iteration of solve_batch stopped at max_iter = iters in both modes (after one run that pays the
allocations: the median of `reps` runs), and ms per border call with a full history of 6 pairs (median of `reps`)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def general_row(T):
    return (max(2, T // 3), 2 * T // 3, 0.2)


def build(T, mode, iters, row):
    import dto_amd
    from dto_amd import problems as P
    p = P.build_acrobot_padded(T=T, target=0.5, terminal="physical", **(dict(general_row=general_row(T)) if row else {}))
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p.get("general_constraint"), options=dto_amd.Options(hessian_approximation=mode, max_iter=iters),
                       name="acrobot_padded_g" if row else "acrobot_padded")
    return s, p


def warm_case(a):
    """cold against warm solves of the limited-memory mode (dto_solve_batch_warm), to convergence"""
    import torch
    import dto_amd
    s, p = build(a.T, "limited-memory", 1000, a.general_row)
    nz = s.nlp.num_variables
    Z = np.zeros((a.B, nz))
    for b in range(a.B):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s._z0
    z0 = torch.tensor(Z, device="cuda")

    def timed(start, end, **kw):
        ts = []
        for _ in range(1 + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            status, iters = s.solve_batch_warm(a.B, start, end, **kw)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return dict(ms_per_solve=float(np.median(ts[1:])), status=[int(v) for v in status], iterations=[int(v) for v in iters])
    first = s.new_point(a.B)
    out = dict(T=a.T, B=a.B, general_row=list(general_row(a.T)) if a.general_row else None, cold=timed(None, first, x0_ptr=z0.data_ptr(), ldx=nz))
    start = s.new_point(a.B)
    for k in ("x", "mu", "zl", "zu", "slack", "barrier", "qn_s", "qn_y"):
        getattr(start, k).copy_(getattr(first, k))
    start.qn_npairs[:], start.qn_sigma[:] = first.qn_npairs, first.qn_sigma
    rng = np.random.default_rng(0)
    start.x += 1e-3 * float(first.x.abs().max()) * torch.tensor(rng.standard_normal((a.B, nz)), device="cuda")
    end = s.new_point(a.B)
    out["warm_with_history"] = timed(start, end)
    out["cold_from_the_same_x"] = timed(None, end, x0_ptr=start.x.data_ptr(), ldx=nz)
    start.qn_s = start.qn_y = start.qn_npairs = start.qn_sigma = None
    out["warm_without_history"] = timed(start, end)
    s.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--B", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--general-row", action="store_true")
    ap.add_argument("--warm", action="store_true")
    a = ap.parse_args()
    if a.warm:
        return warm_case(a)
    import torch
    import dto_amd
    out = dict(T=a.T, B=a.B, iters=a.iters, general_row=list(general_row(a.T)) if a.general_row else None)
    for mode in ("limited-memory", "exact"):
        s, p = build(a.T, mode, a.iters, a.general_row)
        nz, nc = s.nlp.num_variables, s.nlp.num_constraint
        Z = np.zeros((a.B, nz))
        for b in range(a.B):
            xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
            dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
            Z[b] = s._z0
        z0 = torch.tensor(Z, device="cuda")
        zo = torch.empty((a.B, nz), device="cuda", dtype=torch.float64)
        lo = torch.empty((a.B, nc), device="cuda", dtype=torch.float64)
        ts = []
        for _ in range(1 + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            status, iters = s.solve_batch(z0.data_ptr(), a.B, nz, zo.data_ptr(), nz, lo.data_ptr(), nc)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0) / max(1, int(np.max(iters))))
        out[mode] = dict(ms_per_iteration=float(np.median(ts[1:])), iterations=[int(v) for v in iters], mode=s.hessian_mode_last())
        if mode == "limited-memory":
            rng = np.random.default_rng(0)
            S = torch.tensor(rng.standard_normal((a.B * 6, nz)), device="cuda")
            Y = 0.3 * S + 0.05 * torch.tensor(rng.standard_normal((a.B * 6, nz)), device="cuda")
            sx = torch.full((a.B, nz), 1.0, device="cuda", dtype=torch.float64)
            s.kkt_assemble_first_order(z0.data_ptr(), a.B, nz, 1.0, 1e-8, sigma_x_ptr=sx.data_ptr(), ldsx=nz)
            s.kkt_factor()
            ka, kb, _ = general_row(a.T)
            G = torch.zeros((a.B, nz), device="cuda", dtype=torch.float64)
            G[:, (ka - 1) * 65] = 1.0
            G[:, (kb - 1) * 65] = 1.0
            C = torch.full((a.B, 1), -1e-8, device="cuda", dtype=torch.float64)
            calls = {"lbfgs_border_ms": lambda: s.kkt_lbfgs_border(6, S.data_ptr(), nz, Y.data_ptr(), nz, [1.0] * a.B),
                     "lbfgs_border_rows_ms": lambda: s.kkt_lbfgs_border_rows(6, S.data_ptr(), nz, Y.data_ptr(), nz, [1.0] * a.B, 1, G.data_ptr(), nz,
                                                                             C.data_ptr(), 1)}
            for key, call in calls.items():
                ts = []
                for _ in range(1 + a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    ts.append(1e3 * (time.perf_counter() - t0))
                out[key] = float(np.median(ts[1:]))
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

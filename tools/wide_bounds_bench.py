"""Per-instance variable bounds on the tile path: B instances of the native 64-state model
(problems.build_acrobot_padded with action bounds) at horizon T, timed end to end (host loop included):
  shared        -- dto_solve_batch with the problem's shared bounds;
  per_instance  -- dto_solver_set_bounds with bounds equal to the shared ones in every row, then dto_solve_batch;
the two alternate (--reps rounds, after one warm-up solve of each) and must return identical results; then
  mpc_step      -- measured first-knot states as per-instance bounds: dto_solver_shift(1) + dto_solver_set_bounds +
                   dto_solver_begin_warm + dto_solver_run.
--only shared | per_instance: that mode alone (--reps solves, no warm-up), for a kernel-trace run of each under rocprofv3.
Prints one JSON line.   python tools/wide_bounds_bench.py [--B 256] [--T 200] [--reps 3] [--only MODE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dto_amd
from dto_amd import problems as P

N = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("shared", "per_instance"), default=None)
    args = ap.parse_args()
    B, T = args.B, args.T
    p = P.build_acrobot_padded(T=T, target=1.0, terminal="physical", u_max=10.0)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    Z = np.zeros((B, nz))
    for b in range(B):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s._z0
    lo, hi = s.nlp.variable_bounds
    L = torch.tensor(np.tile(lo, (B, 1)), device="cuda")
    U = torch.tensor(np.tile(hi, (B, 1)), device="cuda")
    z0 = torch.tensor(Z, device="cuda")
    zo = torch.empty((B, nz), device="cuda", dtype=torch.float64)
    mo = torch.empty((B, nc), device="cuda", dtype=torch.float64)
    res = dict(B=B, T=T, states=N)

    def solve(mode):
        if mode == "per_instance":
            s.set_bounds_batch(L, U)
        else:
            s.set_bounds_batch(None, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc)
        torch.cuda.synchronize()
        return st, it, time.perf_counter() - t0

    if args.only:
        walls = []
        for _ in range(args.reps):
            st, it, dt = solve(args.only)
            walls.append(round(dt, 4))
        res[args.only] = dict(converged=int(np.sum(st == 1)), iter_mean=float(np.mean(it)), wall_s=walls)
        print(json.dumps(res), flush=True)
        return

    out = {}
    for mode in ("shared", "per_instance"):          # warm-up: code objects, allocations of the batch state
        st, it, _ = solve(mode)
        out[mode] = (zo.cpu().numpy(), mo.cpu().numpy(), st, it)
    same = all(np.array_equal(a, b) for a, b in zip(out["shared"], out["per_instance"]))
    walls = {"shared": [], "per_instance": []}
    for r in range(args.reps):
        for mode in (("shared", "per_instance") if r % 2 == 0 else ("per_instance", "shared")):
            st, it, dt = solve(mode)
            walls[mode].append(round(dt, 4))
            same = same and np.array_equal(zo.cpu().numpy(), out["shared"][0])
    for mode in walls:
        st, it = out[mode][2], out[mode][3]
        res[mode] = dict(converged=int(np.sum(st == 1)), iter_mean=float(np.mean(it)), wall_s=walls[mode],
                         wall_median_s=float(np.median(walls[mode])))
    res["identical_results"] = bool(same)

    # one receding-horizon step with per-instance measured states, from the shared solution above
    rng = np.random.default_rng(0)
    zs = out["shared"][0]
    X = zs[:, N + 1:2 * N + 1] + 1e-3 * rng.standard_normal((B, N))   # the second knot of the solution, disturbed
    Lm, Um = np.tile(lo, (B, 1)), np.tile(hi, (B, 1))
    Lm[:, :N], Um[:, :N] = X, X
    Lm, Um = torch.tensor(Lm, device="cuda"), torch.tensor(Um, device="cuda")
    s.set_bounds_batch(None, None)
    s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.shift_batch(1)
    s.set_bounds_batch(Lm, Um)
    s.begin_warm_batch(B)
    st, it = s.run_batch(zo.data_ptr(), nz, mo.data_ptr(), nc)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pinned = bool(np.array_equal(zo.cpu().numpy()[:, :N], Lm.cpu().numpy()[:, :N]))
    res["mpc_step"] = dict(converged=int(np.sum(st == 1)), iter_mean=float(np.mean(it)), iter_max=int(np.max(it)), wall_s=round(dt, 3),
                           first_knot_pinned=pinned)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

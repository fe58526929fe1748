"""Lane border, one receding-horizon step of the MPC pendulum with a per-instance budget row (problems.py:
build_mpc_pendulum_coupled, T = 50, the five rollouts of tests/test_border_params_gpu.py): the cold solve through dto_solve_batch and
through dto_solve_batch_warm(start = NULL), then -- with --warm -- the point shifted by one knot (dto_point_shift), the measured state
(the model's own step plus a 1e-3 disturbance) in the parameters, and the re-solve warm from the point against cold from the same x.
For the record, no claim and no threshold.

    python tools/border_warm_bench.py [--warm] [--reps 5]

One JSON line: ms per solve (median of `reps` after one run that pays the allocations) and the iteration counts."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, B = 50, 5
TOTALS = [-0.24, 0.48, 0.22, 0.25, -0.45]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import dto_amd
    from dto_amd import problems as P
    p = P.build_mpc_pendulum_coupled(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], parameters=p["parameters"], name="mpc_pendulum_coupled")
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    rng = np.random.default_rng(11)
    x1s = 0.3 * rng.standard_normal((B, 2))
    goals = np.pi * (0.5 + 0.5 * rng.random(B))
    us = [[0.1 * rng.standard_normal(1) for _ in range(T - 1)] for _ in range(B)]
    Z = np.zeros((B, nz))
    for b in range(B):
        dto_amd.initialize_states(s, dto_amd.linear_interpolation(x1s[b], np.array([goals[b], 0.0]), T))
        dto_amd.initialize_controls(s, us[b])
        Z[b] = s._z0
    params = lambda X: torch.tensor(np.stack([np.tile([X[b, 0], X[b, 1], goals[b], TOTALS[b]], T) for b in range(B)]), device="cuda")

    def timed(call):
        ts = []
        for _ in range(1 + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            status, iters = call()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return dict(ms_per_solve=float(np.median(ts[1:])), status=[int(v) for v in status], iterations=[int(v) for v in iters])
    z0, w = torch.tensor(Z, device="cuda"), params(x1s)
    zo = torch.empty((B, nz), device="cuda", dtype=torch.float64)
    lo = torch.empty((B, nc), device="cuda", dtype=torch.float64)
    out = dict(T=T, B=B)
    out["solve_batch"] = timed(lambda: s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, lo.data_ptr(), nc, params_ptr=w.data_ptr(), ldp=4 * T))
    first = s.new_point(B)
    out["solve_batch_warm_cold"] = timed(lambda: s.solve_batch_warm(B, None, first, x0_ptr=z0.data_ptr(), ldx=nz, params_ptr=w.data_ptr(), ldp=4 * T))
    if a.warm:
        z = first.x.cpu().numpy()

        def plant(x, u):
            y = np.array(x, dtype=float)
            for _ in range(200):
                y_new = np.array(y - P.pendulum_midpoint(y, x, np.array([u]), None), dtype=float)
                if np.max(np.abs(y_new - y)) < 1e-15:
                    break
                y = y_new
            return y_new
        X = np.array([plant(z[b][:2], z[b][2]) for b in range(B)]) + 1e-3 * np.random.default_rng(5).standard_normal((B, 2))
        s.shift_point(first, 1)
        w1 = params(X)
        end = s.new_point(B)
        out["warm_after_shift"] = timed(lambda: s.solve_batch_warm(B, first, end, params_ptr=w1.data_ptr(), ldp=4 * T))
        out["cold_from_the_same_x"] = timed(lambda: s.solve_batch_warm(B, None, end, x0_ptr=first.x.data_ptr(), ldx=nz, params_ptr=w1.data_ptr(), ldp=4 * T))
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

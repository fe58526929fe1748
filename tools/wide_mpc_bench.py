"""Re-solve costs on the tile path: B instances of the 64-state model (problems.build_acrobot_padded with
per-instance parameters and action bounds) at horizon T, three re-solves timed end to end (host loop included):
  cold      -- dto_solve_batch from the previous solution (multipliers zero, mu = mu_init);
  warm      -- dto_solver_begin_warm after a 2 % change of every instance's parameters + dto_solver_run;
  shift     -- dto_solver_shift(1) + dto_solver_begin_warm + dto_solver_run (the receding-horizon step).
Prints one JSON line.   python tools/wide_mpc_bench.py [B] [T]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dto_amd
from dto_amd import problems as P


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    p = P.build_acrobot_padded(T=T, target=1.0, terminal="physical", parameters=(1.0, 1.0), u_max=10.0)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       parameters=p["parameters"], name="acrobot_padded_par")
    nz, nc, nw = s._solve_nlp.num_variables, s._solve_nlp.num_constraint, s._solve_nlp.num_parameters
    rng = np.random.default_rng(0)
    Z = np.zeros((B, nz))
    for b in range(B):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s._z0
    pairs = np.stack([1.0 + 0.2 * rng.standard_normal(B).clip(-2, 2), 1.0 + 0.2 * rng.standard_normal(B).clip(-2, 2)], axis=1)
    w1 = torch.tensor(np.tile(pairs, (1, T)), device="cuda")
    w2 = torch.tensor(np.tile(pairs * np.array([1.02, 0.98]), (1, T)), device="cuda")
    z0 = torch.tensor(Z, device="cuda")
    zo = torch.empty((B, nz), device="cuda", dtype=torch.float64)
    mo = torch.empty((B, nc), device="cuda", dtype=torch.float64)
    res = dict(B=B, T=T, states=64)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st, it = f()
        torch.cuda.synchronize()
        return st, it, time.perf_counter() - t0

    st, it, dt = timed(lambda: s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc, params_ptr=w1.data_ptr(), ldp=nw))
    res["first"] = dict(converged=int(np.sum(st == 1)), iter_mean=float(np.mean(it)), iter_max=int(np.max(it)), wall_s=round(dt, 3))
    zprev = zo.clone()

    def warm():
        s.begin_warm_batch(B, params_ptr=w2.data_ptr(), ldp=nw)
        return s.run_batch(zo.data_ptr(), nz, mo.data_ptr(), nc)
    st, it, dt = timed(warm)
    res["warm_param_change"] = dict(converged=int(np.sum(st == 1)), iter_mean=float(np.mean(it)), iter_max=int(np.max(it)), wall_s=round(dt, 3))

    def shift():
        s.shift_batch(1)
        s.begin_warm_batch(B, params_ptr=w2.data_ptr(), ldp=nw)
        return s.run_batch(zo.data_ptr(), nz, mo.data_ptr(), nc)
    st, it, dt = timed(shift)
    res["shift_warm"] = dict(converged=int(np.sum(st == 1)), iter_mean=float(np.mean(it)), iter_max=int(np.max(it)), wall_s=round(dt, 3))
    st, it, dt = timed(lambda: s.solve_batch(zprev.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc, params_ptr=w2.data_ptr(), ldp=nw))
    res["cold_from_previous"] = dict(converged=int(np.sum(st == 1)), iter_mean=float(np.mean(it)), iter_max=int(np.max(it)), wall_s=round(dt, 3))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

"""Coupling GeneralConstraint rows on the tile path: what one outer iteration and one bordered step cost.

    python tools/wide_general_border_bench.py [--B 3] [--T 30] [--reps 20] [--bounded]

1. solve_batch of the 64-state problem of tests/test_wide_general_border_gpu.py (q1[10] + q1[20] = total): wall time per outer
   iteration of the batch (the slowest instance's iteration count).
2. The pieces of one bordered step at the solution, through the entry points the step itself calls, HIP events around each:
   the three callbacks (Jacobian, constraints, objective gradient), dto_kkt_assemble + dto_kkt_factor,
   dto_kkt_border_factor (panel substitution, Gram product, Schur complement) and dto_kkt_border_solve.
--bounded: the same problem with the action bounds |u| <= problems.ACROBOT_PADDED_COUPLING_U_MAX["64"] of
tests/test_wide_general_border_bounds_gpu.py (the barrier of the bordered loop); part 1 only -- the pieces of part 2 are the same calls.
Numbers only, no threshold (DESIGN.md section 4.3 quotes a run)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import dto_amd
    from dto_amd import problems as P
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=3)
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bounded", action="store_true")
    a = ap.parse_args()
    T, B = a.T, a.B
    u_max = P.ACROBOT_PADDED_COUPLING_U_MAX["64"] if a.bounded else None
    p = P.build_acrobot_padded(T=T, target=0.5, terminal="physical", general_row=(10, 20, P.ACROBOT_PADDED_COUPLING_TOTALS["sum"]), u_max=u_max)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], name="acrobot_padded_g")
    n = s.nlp
    nz, nc, nnz = n.num_variables, n.num_constraint, n.num_jacobian
    Z = np.zeros((B, nz))
    for b in range(B):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s._z0
    z0 = torch.tensor(Z, device="cuda")
    zo = torch.zeros((B, nz), device="cuda", dtype=torch.float64)
    lam = torch.zeros((B, nc), device="cuda", dtype=torch.float64)
    s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, lam.data_ptr(), nc)   # (first call: allocations)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    status, iters = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, lam.data_ptr(), nc)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(f"solve_batch{f' with |u| <= {u_max}' if a.bounded else ''}: B = {B}, T = {T}, status {status.tolist()}, iterations {iters.tolist()}, {wall * 1e3:.1f} ms, "
          f"{wall * 1e3 / max(1, int(iters.max())):.2f} ms per outer iteration of the batch")
    if a.bounded:
        return

    f64 = dict(device="cuda", dtype=torch.float64)
    J, c, g = torch.zeros((B, nnz), **f64), torch.zeros((B, nc), **f64), torch.zeros((B, nz), **f64)
    ng = 1
    panel, cb = torch.zeros((B * ng, nz), **f64), torch.full((B, ng * ng), -1e-8, **f64)
    ia, ib = 9 * 65, 19 * 65
    panel[:, ia] = 1.0
    panel[:, ib] = 1.0
    rx, rc, rb = torch.randn((B, nz), **f64), torch.randn((B, nc), **f64), torch.randn((B, ng), **f64)
    ox, oc, ob = torch.zeros((B, nz), **f64), torch.zeros((B, nc), **f64), torch.zeros((B, ng), **f64)

    def callbacks():
        n.eval_constraint_jacobian_batch(zo.data_ptr(), B, nz, J.data_ptr(), nnz)
        n.eval_constraint_batch(zo.data_ptr(), B, nz, c.data_ptr(), nc)
        n.eval_objective_gradient_batch(zo.data_ptr(), B, nz, g.data_ptr(), nz)

    def factor():
        s.kkt_assemble(zo.data_ptr(), B, nz, lam.data_ptr(), nc, 1e-4, 1e-8)
        s.kkt_factor()

    def border_factor():
        s.kkt_border_factor(ng, panel.data_ptr(), nz, 0, 0, cb.data_ptr(), ng * ng)

    def border_solve():
        s.kkt_border_solve(rx.data_ptr(), nz, rc.data_ptr(), nc, rb.data_ptr(), ng, ox.data_ptr(), nz, oc.data_ptr(), nc, ob.data_ptr(), ng)

    steps = (("callbacks", callbacks), ("assemble + factor", factor), ("border factor", border_factor), ("border solve", border_solve))
    for _, fn in steps:          # warm-up (allocations of the first call)
        fn()
    torch.cuda.synchronize()
    total = 0.0
    for name, fn in steps:
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        total += med
        print(f"  {name:18s} {med:8.3f} ms (median of {a.reps})")
    print(f"  {'sum':18s} {total:8.3f} ms")


if __name__ == "__main__":
    main()

"""One SHA-256 per case over the raw bytes of what the two HOST-driven solver loops of csrc/dto_solver.cpp return -- x, multipliers,
status, iterations -- plus the per-instance status and iterations in clear (needs a GPU, a few seconds):
python tools/host_loops_digest.py

To compare two states of the host loops (wide_outer: tile path; general_solve_batch: bordered path) whose results must be
bit-identical: run it at both and diff the printouts.  Every case runs to termination (max_iter 200), B = 3, at the smallest shapes
that reach every phase: the 64-state acrobot at T = 4 with and without action bounds (barrier on / off; both end at max_iter after
200 iterations of rejected trials and fallback steps) and at T = 30 (the one without bounds converges), the reference's
GeneralConstraint problem with a coupling row as an equality and as an inequality (slack, barrier update), and the acrobot with two
coupling rows at T = 8 on the device border and on the host border (DTO_BORDER_HOST=1: the host-statistics branch).
Then one case per branch the bordered loop has grown since (lane_feature_cases, tile_border_cases), at the shapes of the tests that
own the plugins: action bounds beside a coupling row (inequality and equality), inequality stage rows with bounds and a product row,
per-instance parameters, the tile border with and without action bounds, and the limited-memory mode without rows and beside a sum
row with action bounds.
DTO_WIDE_VERBOSE=1 prints every iteration of instance 0 of the tile path (delta_w, attempts, alpha, ls_fail) to stderr."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import dto_amd
from dto_amd import problems as P

B = 3
MAX_ITER = 200


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


def report(label, s, Z, W=None):
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    z0 = torch.tensor(Z, device="cuda")
    zo = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    mo = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    kw = {}
    if W is not None:   # per-instance parameters
        w = torch.tensor(W, device="cuda")
        kw = dict(params_ptr=w.data_ptr(), ldp=W.shape[1])
    st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc, **kw)
    torch.cuda.synchronize()
    print(f"{label:34s} {digest(zo, mo, st, it)} status {st.tolist()} iterations {it.tolist()}", flush=True)


def tile_cases():
    # (at T = 4 the target is out of reach: those two end at max_iter after 200 iterations of rejected trials; T = 30 converges)
    for label, T, u_max in (("tile barrier", 4, 1.0), ("tile no-barrier", 4, None), ("tile barrier T30", 30, 1.0), ("tile no-barrier T30", 30, None)):
        p = P.build_acrobot_padded(T=T, target=0.5, terminal="physical", u_max=u_max)
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded",
                           options=dto_amd.Options(max_iter=MAX_ITER))
        Z = np.zeros((B, s.nlp.num_variables))
        for b in range(B):   # the guesses of tools/wide_outputs_digest.py: iterations
            xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
            dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
            Z[b] = s._z0
        report(label, s, s.pad_batch(Z))
        s.close()


def bordered_cases():
    opts = dict(general_rows="border", max_iter=MAX_ITER)
    for label, ineq in (("bordered ref eq", None), ("bordered ref ineq 0.05", 0.05)):
        p = P.build_ref_general_coupled(inequality=ineq)
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                           general_constraint=p["general_constraint"], options=dto_amd.Options(**opts),
                           name="ref_general_coupled" + ("" if ineq is None else "_ineq"))
        Z = np.zeros((B, s.nlp.num_variables))
        for b in range(B):   # the guess of tests/test_bordered_gpu.py, the actions five times as far out
            rng = np.random.Generator(np.random.PCG64(5 + b))
            dto_amd.initialize_states(s, dto_amd.linear_interpolation(p["x1"], p["xT"], p["T"]))
            dto_amd.initialize_controls(s, [5.0 * rng.standard_normal(1) for _ in range(p["T"] - 1)])
            Z[b] = s._z0
        report(label, s, s.pad_batch(Z))
        s.close()
    p = P.build_acrobot_coupled(T=8)
    pa = P.build_acrobot(T=8, evaluate_hessian=True)
    for label, host in (("bordered acrobot", None), ("bordered acrobot host", "1")):
        if host is not None:
            os.environ["DTO_BORDER_HOST"] = host
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                           general_constraint=p["general_constraint"], options=dto_amd.Options(**opts), name="acrobot_coupled")
        Z = np.zeros((B, s.nlp.num_variables))
        for b in range(B):   # the guess of tools/border_bench.py, the actions at their full size
            xs, us = pa["guess"](np.random.Generator(np.random.PCG64(b)))
            dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, us)
            Z[b] = s._z0
        report(label, s, s.pad_batch(Z))
        s.close()
    os.environ.pop("DTO_BORDER_HOST", None)


def guesses(s, p, scale=0.1):
    Z = np.zeros((B, s.nlp.num_variables))
    for b in range(B):   # PCG64(b), the actions scaled as the tests scale them
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [scale * u for u in us])
        Z[b] = s._z0
    return s.pad_batch(Z)


def lane_feature_cases():
    opts = dict(general_rows="border", max_iter=MAX_ITER)
    # the pendulum swing-up, T = 50, theta_15 + theta_35 (<= | =) 1 beside |u| <= 3 (tests/test_border_bounds_gpu.py)
    for label, ineq in (("lane bounds, row <= 1", True), ("lane bounds, row = 1", False)):
        p = P.build_pendulum_coupled(T=50, total=1.0, inequality=ineq, u_max=3.0)
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                           general_constraint=p["general_constraint"], options=dto_amd.Options(**opts), name="pendulum_coupled")
        report(label, s, guesses(s, p))
        s.close()
    # speed limit at every knot, |u| <= 4 and the product row (tests/test_border_stage_ineq_gpu.py)
    p = P.build_pendulum_speed_limit(T=50, v_max=3.35, row="product", total=-0.39, u_max=4.0)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], options=dto_amd.Options(**opts), name="pendulum_speed_prod")
    report("lane stage ineq, bounds, product", s, guesses(s, p))
    s.close()
    # per-instance start, goal and budget of the row (tests/test_border_params_gpu.py: its first three rollouts and budgets)
    T = 50
    p = P.build_mpc_pendulum_coupled(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], parameters=p["parameters"],
                       options=dto_amd.Options(max_iter=MAX_ITER), name="mpc_pendulum_coupled")
    rng = np.random.default_rng(11)
    x1s = 0.3 * rng.standard_normal((5, 2))
    goals = np.pi * (0.5 + 0.5 * rng.random(5))
    us = [[0.1 * rng.standard_normal(1) for _ in range(T - 1)] for _ in range(5)]
    totals = (-0.24, 0.48, 0.22)
    Z = np.zeros((B, s.nlp.num_variables))
    for b in range(B):
        dto_amd.initialize_states(s, dto_amd.linear_interpolation(x1s[b], np.array([goals[b], 0.0]), T))
        dto_amd.initialize_controls(s, us[b])
        Z[b] = s._z0
    W = np.stack([np.tile([x1s[b, 0], x1s[b, 1], goals[b], totals[b]], T) for b in range(B)])
    report("lane per-instance parameters", s, s.pad_batch(Z), W)
    s.close()


def tile_border_cases():
    # 64 states, T = 30, the sum row over knots 10 and 20 (tests/test_wide_general_border_gpu.py, ..._bounds_gpu.py, test_wide_lbfgs_*.py)
    row = (10, 20, P.ACROBOT_PADDED_COUPLING_TOTALS["sum"])
    u64 = P.ACROBOT_PADDED_COUPLING_U_MAX["64"]
    for label, u_max, lm in (("tile border, sum row", None, False), ("tile border, sum row, bounds", u64, False),
                             ("tile lbfgs, sum row, bounds", u64, True)):
        p = P.build_acrobot_padded(T=30, target=0.5, terminal="physical", general_row=row, u_max=u_max)
        o = dto_amd.Options(max_iter=MAX_ITER, **(dict(hessian_approximation="limited-memory") if lm else {}))
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                           general_constraint=p["general_constraint"], options=o, name="acrobot_padded_g")
        report(label, s, guesses(s, p))
        s.close()
    # limited-memory mode without rows, T = 16 (tests/test_wide_lbfgs_solve_gpu.py)
    p = P.build_acrobot_padded(T=16, target=0.5, terminal="physical")
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       options=dto_amd.Options(max_iter=MAX_ITER, hessian_approximation="limited-memory"), name="acrobot_padded")
    report("tile lbfgs, no rows", s, guesses(s, p))
    s.close()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    tile_cases()
    bordered_cases()
    lane_feature_cases()
    tile_border_cases()


if __name__ == "__main__":
    main()

"""One SHA-256 per case over the raw bytes of what the two HOST-driven solver loops of csrc/dto_solver.cpp return -- x, multipliers,
status, iterations -- plus the per-instance status and iterations in clear (needs a GPU, a few seconds):
python tools/host_loops_digest.py

To compare two states of the host loops (wide_outer: tile path; general_solve_batch: bordered path) whose results must be
bit-identical: run it at both and diff the printouts.  Every case runs to termination (max_iter 200), B = 3, at the smallest shapes
that reach every phase: the 64-state acrobot at T = 4 with and without action bounds (barrier on / off; both end at max_iter after
200 iterations of rejected trials and fallback steps) and at T = 30 (the one without bounds converges), the reference's
GeneralConstraint problem with a coupling row as an equality and as an inequality (slack, barrier update), and the acrobot with two
coupling rows at T = 8 on the device border and on the host border (DTO_BORDER_HOST=1: the host-statistics branch).
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


def report(label, s, Z):
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    z0 = torch.tensor(Z, device="cuda")
    zo = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    mo = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc)
    torch.cuda.synchronize()
    print(f"{label:28s} {digest(zo, mo, st, it)} status {st.tolist()} iterations {it.tolist()}", flush=True)


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


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    tile_cases()
    bordered_cases()


if __name__ == "__main__":
    main()

"""One SHA-256 per entry point of the tile path over the raw bytes of its outputs, at fixed seeds and tiny shapes (needs a GPU, a few
seconds): python tools/wide_outputs_digest.py

To compare two states of csrc/dto_wide_kernels.hpp whose results must be bit-identical: run it at both and diff the printouts.
Shapes: build_acrobot_padded(T=4), B = 3 (the smallest horizon with an interior stage, a prefetch hand-over and the terminal block)
and build_acrobot_padded(T=5, m=3), B = 2 (the triangular part of the action block); nrhs = 3 is a partial block of
dto_kkt_solve_multi, 17 one full block plus one column.  Last, three iterations on the 64-state model with action bounds
(tests/test_wide_bounds_gpu.py): the instantiations of k_wide_step / k_wide_bwd with barrier terms."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import dto_amd
from dto_amd import problems as P


def solvers():
    """(label, Solver, problem, B) of every shape; building them compiles or loads the plugins (no GPU needed for that)."""
    out = []
    for label, kw, B in (("T4", dict(T=4), 3), ("T5m3", dict(T=5, m=3), 2)):
        p = P.build_acrobot_padded(**kw)
        name = "acrobot_padded" + (f"_m{kw['m']}" if "m" in kw else "")
        out.append((label, dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name=name), p, B))
    p = P.build_acrobot_padded(T=4, target=0.5, terminal="physical", u_max=1.0)
    out.append(("T4bounded", dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                                           name="acrobot_padded"), p, 3))
    return out


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


def linear_solver_calls(label, s, B):
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    g = torch.Generator(device="cuda"); g.manual_seed(1)

    def rnd(rows, n, normal=False):
        return (torch.randn if normal else torch.rand)((rows, n), device="cuda", dtype=torch.float64, generator=g)

    def nan(rows, n):
        return torch.full((rows, n), float("nan"), device="cuda", dtype=torch.float64)

    Z, MU = rnd(B, nz), rnd(B, nc)
    dx, dl = nan(B, nz), nan(B, nc)
    ok = s.kkt_step_batch(Z.data_ptr(), B, nz, MU.data_ptr(), nc, 2.0, 1e-5, dx.data_ptr(), nz, dl.data_ptr(), nc)
    torch.cuda.synchronize()
    print(f"{label} kkt_step_batch      {digest(dx, dl, np.array([ok]))}")
    s.kkt_assemble(Z.data_ptr(), B, nz, MU.data_ptr(), nc, 2.0, 1e-5)
    print(f"{label} kkt_factor          {digest(*s.kkt_factor())}")
    for nrhs in (1, 3, 17):
        RX, RC = rnd(B * nrhs, nz, True), rnd(B * nrhs, nc, True)
        ox, oc = nan(B * nrhs, nz), nan(B * nrhs, nc)
        if nrhs == 1:
            s.kkt_solve(RX.data_ptr(), nz, RC.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc)
            torch.cuda.synchronize()
            print(f"{label} kkt_solve           {digest(ox, oc)}")
            s.kkt_multiply(RX.data_ptr(), nz, RC.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc)
            torch.cuda.synchronize()
            print(f"{label} kkt_multiply        {digest(ox, oc)}")
            s.kkt_solve_refined(RX.data_ptr(), nz, RC.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc, 1)
            torch.cuda.synchronize()
            print(f"{label} kkt_solve_refined   {digest(ox, oc)}")
        else:
            s.kkt_solve_multi(nrhs, RX.data_ptr(), nz, RC.data_ptr(), nc, ox.data_ptr(), nz, oc.data_ptr(), nc)
            torch.cuda.synchronize()
            print(f"{label} kkt_solve_multi {nrhs:2d}  {digest(ox, oc)}")


def iterations(label, s, p, B):
    Z = np.zeros((B, s.nlp.num_variables))
    for b in range(B):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s._z0
    z0 = torch.tensor(Z, device="cuda")
    s.begin_batch(z0.data_ptr(), B, Z.shape[1])
    s.iterate_batch(3)
    print(f"{label} solver_iterate x 3  {digest(s.peek_batch('z'), s.peek_batch('multipliers'), s.peek_batch('z_lower'), s.peek_batch('z_upper'))}")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    for label, s, p, B in solvers():
        if label.endswith("bounded"):
            iterations(label, s, p, B)
        else:
            linear_solver_calls(label, s, B)
        s.close()


if __name__ == "__main__":
    main()

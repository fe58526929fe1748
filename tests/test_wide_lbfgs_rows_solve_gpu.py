"""The limited-memory mode of the tile path BESIDE coupling GeneralConstraint rows: Options(hessian_approximation="limited-memory")
on the problems of tests/test_wide_general_border_gpu.py::test_solve_64_states_with_a_coupling_row -- 64 states, T = 30, B = 3, a row
over the knots 10 and 20, the totals of dto_amd/problems.py, the guesses PCG64(b) with the actions x 0.1 -- and on the 24-state
linear row kept on the border of the embedding.  dto_solve_batch / dto_solve run the host-driven bordered loop with the compact
L-BFGS matrix (history 6) and the row in ONE border of 13 rows (dto_kkt_lbfgs_border_rows); no second derivative is evaluated.

Every solution is checked as a KKT point with the ORACLE's derivatives (oracle/padded_model.py) and the closed form of the row, with
the bars of that test: violation <= 1e-6, stationarity <= 1e-5 max(1, |lambda|), the row binds.  Iteration counts are printed, not
asserted.  The equality rows ("sum", "product") have to converge from all three guesses; the inequality row and the sum row beside
action bounds are solved from the guesses listed in GUESSES below (DESIGN.md section 4.3 has the counts)."""
import numpy as np
import pytest

from test_wide_general_border_gpu import (KA, KB, SOLVE_B, SOLVE_T, TOTAL_PROD_EQ, TOTAL_SUM_EQ, TOTAL_SUM_INEQ, _kkt_conditions, _solver,
                                          _spec)
from test_wide_general_border_bounds_gpu import U64, _kkt_conditions_bounded, _u_index

pytestmark = pytest.mark.gpu

# the guesses every case is solved from: all three for the equality rows (required); the other two cases had no evidence from the CPU
# beforehand and keep the guesses that converge
GUESSES = {"sum": (0, 1, 2), "product": (0, 1, 2), "sum<=0": (0, 1, 2), "sum,bounded": (0, 1, 2)}
_REF = {}


def _row(kind):
    return {"sum": (KA, KB, TOTAL_SUM_EQ), "product": (KA, KB, TOTAL_PROD_EQ, False, "product"), "sum<=0": (KA, KB, TOTAL_SUM_INEQ, True),
            "sum,bounded": (KA, KB, TOTAL_SUM_EQ)}[kind]


def _lm_solver(kind):
    import dto_amd
    kw = dict(u_max=U64) if kind == "sum,bounded" else {}
    return _solver(SOLVE_T, [_row(kind)], name="acrobot_padded_g", target=0.5, terminal="physical",
                   options=dto_amd.Options(hessian_approximation="limited-memory"), **kw)


def _guesses(s, p, seeds):
    import dto_amd
    Z = np.zeros((len(seeds), s.nlp.num_variables))
    for k, b in enumerate(seeds):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[k] = s._z0
    return Z


def _solve_batch(s, Z):
    import torch
    nb, nz, nc = Z.shape[0], s.nlp.num_variables, s.nlp.num_constraint
    z0 = torch.tensor(Z, device="cuda")
    zo = torch.full((nb, nz), float("nan"), device="cuda", dtype=torch.float64)
    lo = torch.full((nb, nc), float("nan"), device="cuda", dtype=torch.float64)
    status, iters = s.solve_batch(z0.data_ptr(), nb, nz, zo.data_ptr(), nz, lo.data_ptr(), nc)
    torch.cuda.synchronize()
    return status, iters, zo.cpu().numpy(), lo.cpu().numpy()


def _batch(kind):
    """The batch of a case, solved once and shared (never changed)."""
    if kind not in _REF:
        s, p = _lm_solver(kind)
        assert s.hessian_mode == "lbfgs" and s.general_rows_path == "border" and s.solve_unsupported is None
        assert s.nlp.num_constraint == (SOLVE_T - 1) * 64 + 1
        status, iters, Z, LAM = _solve_batch(s, _guesses(s, p, GUESSES[kind]))
        print(f"[64 states, {kind} row, limited-memory] guesses {GUESSES[kind]}: status {status.tolist()}, iterations {iters.tolist()}")
        for a in (Z, LAM):
            a.setflags(write=False)
        _REF[kind] = dict(s=s, p=p, status=status, iters=iters, Z=Z, LAM=LAM, mode=s.hessian_mode_last())
    return _REF[kind]


@pytest.mark.parametrize("kind", ["sum", "product", "sum<=0"])
def test_solve_64_states_with_a_coupling_row_in_limited_memory_mode(kind):
    from oracle.padded_model import PaddedAcrobot
    if kind != "sum<=0":
        assert GUESSES[kind] == tuple(range(SOLVE_B)), "the equality rows converge from all three guesses"
    assert len(GUESSES[kind]) >= 1
    ref = _batch(kind)
    s = ref["s"]
    assert np.all(ref["status"] == 1), (ref["status"], ref["iters"])
    assert ref["mode"] == "lbfgs"
    vlo, vhi = s.nlp.variable_bounds
    spec = _spec([_row(kind)], 64, 1)
    for k, b in enumerate(GUESSES[kind]):
        nu = _kkt_conditions(PaddedAcrobot(64), SOLVE_T, spec, ref["Z"][k], ref["LAM"][k], vlo, vhi, kind == "sum<=0")
        print(f"  guess {b}: {ref['iters'][k]} iterations, multiplier of the row {nu:.4f}")


@pytest.mark.parametrize("kind", ["sum", "product"])
def test_each_instance_equals_its_solve_alone(kind):
    ref = _batch(kind)
    s, p = ref["s"], ref["p"]
    for k, b in enumerate(GUESSES[kind]):
        status, iters, Z, LAM = _solve_batch(s, _guesses(s, p, [b]))
        dz, dl = float(np.max(np.abs(Z[0] - ref["Z"][k]))), float(np.max(np.abs(LAM[0] - ref["LAM"][k])))
        print(f"  guess {b} alone: {iters[0]} iterations (batch: {ref['iters'][k]}), max |dz| {dz:.2e}, max |dlam| {dl:.2e}")
        assert status[0] == 1 and iters[0] == ref["iters"][k], (b, status, iters, ref["iters"])
        assert dz <= 1e-9 and dl <= 1e-9, (b, dz, dl)


def test_sum_row_beside_action_bounds_in_limited_memory_mode():
    from oracle.padded_model import PaddedAcrobot
    kind = "sum,bounded"
    assert len(GUESSES[kind]) >= 1
    ref = _batch(kind)
    s = ref["s"]
    assert np.all(ref["status"] == 1), (ref["status"], ref["iters"])
    assert ref["mode"] == "lbfgs"
    vlo, vhi = s.nlp.variable_bounds
    spec = _spec([_row(kind)], 64, 1)
    for k, b in enumerate(GUESSES[kind]):
        nu, bc = _kkt_conditions_bounded(PaddedAcrobot(64), SOLVE_T, spec, ref["Z"][k], ref["LAM"][k], vlo, vhi)
        u = ref["Z"][k][_u_index(64, SOLVE_T)]
        print(f"  guess {b}: {ref['iters'][k]} iterations, multiplier of the row {nu:.4f}, peak |u| {np.max(np.abs(u)):.6f}, "
              f"bound complementarity {bc:.2e}")
        assert np.sum(np.abs(u) > U64 - 1e-2) >= 1, np.max(np.abs(u))


def test_24_state_linear_row_on_the_border_in_limited_memory_mode():
    """The row of test_24_state_linear_row_on_the_border_when_asked, checked in the problem's own layout (24 states)."""
    import dto_amd
    from oracle.padded_model import PaddedAcrobot
    n_, T = 24, SOLVE_T
    row = (KA, KB, 0.2)
    s, p = _solver(T, [row], n=n_, name="acrobot24g", target=0.4, terminal="physical",
                   options=dto_amd.Options(general_rows="border", hessian_approximation="limited-memory"))
    assert s.hessian_mode == "lbfgs" and s.general_rows_path == "border" and s.solve_unsupported is None
    assert s._solve_nlp.num_variables == (T - 1) * 65 + 64
    xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
    assert dto_amd.solve(s) == 1, (s.status, s.iterations)
    assert s.hessian_mode_last() == "lbfgs"
    zs, ls = s._solution, s._duals
    assert zs.shape == ((T - 1) * 25 + 24,) and ls.shape == ((T - 1) * n_ + 1,)
    vlo, vhi = s.nlp.variable_bounds
    nu = _kkt_conditions(PaddedAcrobot(n_), T, _spec([row], n_, 1), zs, ls, vlo, vhi, False)
    print(f"[24 states, linear row on the border, limited-memory] {s.iterations} iterations, multiplier {nu:.4f}")

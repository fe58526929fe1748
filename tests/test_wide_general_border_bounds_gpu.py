"""Finite variable bounds beside coupling GeneralConstraint rows on the bordered path, tile linear solver (64 states, and 24
states in the 64-state embedding): csrc/dto_solver.cpp general_solve_batch (border_loop_* phases) / bordered_step_tile with the barrier terms of
csrc/dto_border_kernels.hpp (BorderBar in k_border_point, k_border_bar_stats, k_border_trial).

The problems are those of tests/test_wide_general_border_gpu.py (T = 30, B = 3, knots 10 and 20, the same guesses) with action
bounds |u| <= U.  Bounds are layout data, not literals of the generated code (plugin.Structure takes no bounds), so the plugins
are the ones of the unbounded problems.  U is a literal of dto_amd.problems beside the rows' totals: a fraction of the smallest
peak |u| of the unbounded solutions, to one decimal (0.7 for the 24-state problem; 0.8 for the 64-state one, moved from 0.7 for
the product row's convergence, see there); the tests derive the peaks again and check the literal against them.

Reference: the KKT conditions with the ORACLE's derivatives (oracle/padded_model.py: dense_derivatives), the bound multipliers
eliminated as tests/test_solve_gpu.py: kkt_report does; for the 24-state problem the ordinary tile solver's minimiser of the same
problem with the row on an accumulator state."""
import numpy as np
import pytest

from test_wide_general_border_gpu import KA, KB, SOLVE_B, SOLVE_T, TOTAL_PROD_EQ, TOTAL_SUM_EQ, _row_jacobian, _row_values, _solver, _spec

pytestmark = pytest.mark.gpu

from dto_amd.problems import ACROBOT_PADDED_COUPLING_U_MAX as _UMAX   # (beside the totals: measured peaks in the comment there)
U64, U24 = _UMAX["64"], _UMAX["24"]
PATH_DISTANCE = 1e-3                 # border against accumulators: the limit of tests/test_general_accumulators_gpu.py


def _u_index(n, T):
    return np.array([t * (n + 1) + n for t in range(T - 1)])


def _solve_batch(s, p, B):
    import torch
    import dto_amd
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    Z = np.zeros((B, nz))
    for b in range(B):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        Z[b] = s._z0
    z0 = torch.tensor(Z, device="cuda")
    zo = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    lo_ = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    status, iters = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, lo_.data_ptr(), nc)
    torch.cuda.synchronize()
    return zo.cpu().numpy(), lo_.cpu().numpy(), status, iters


@pytest.fixture(scope="module")
def peaks64():
    """peak |u| of the three solutions of the unbounded problem (test_solve_64_states_with_a_coupling_row[sum])"""
    s, p = _solver(SOLVE_T, [(KA, KB, TOTAL_SUM_EQ)], name="acrobot_padded_g", target=0.5, terminal="physical")
    zo, _, status, iters = _solve_batch(s, p, SOLVE_B)
    assert np.all(status == 1), (status, iters)
    pk = np.max(np.abs(zo[:, _u_index(64, SOLVE_T)]), axis=1)
    print(f"[64 states, sum row, no bounds] peak |u| {pk.tolist()}, iterations {iters.tolist()}")
    return pk


def _kkt_conditions_bounded(om, T, spec, z, lam, vlo, vhi):
    from oracle.padded_model import dense_derivatives
    nd = (T - 1) * om.n
    _, g, c, J, _ = dense_derivatives(om, T, z, lam[:nd], 1.0)
    row, G = _row_values(spec, z), _row_jacobian(spec, z)
    fixed = vlo == vhi
    assert np.max(np.abs(c)) <= 1e-6, np.max(np.abs(c))
    assert np.max(np.abs(z[fixed] - vlo[fixed])) < 1e-12, np.max(np.abs(z[fixed] - vlo[fixed]))
    assert max(np.max(vlo - z), np.max(z - vhi), 0.0) <= 1e-12
    r = g + J.T @ lam[:nd] + G.T @ lam[nd:]
    # the bound multipliers are not returned: z_L = max(r, 0) on a finite lower bound, z_U = max(-r, 0) on a finite upper one
    zl = np.where(np.isfinite(vlo) & ~fixed, np.maximum(r, 0.0), 0.0)
    zu = np.where(np.isfinite(vhi) & ~fixed, np.maximum(-r, 0.0), 0.0)
    stat = (r - zl + zu)[~fixed]
    assert np.max(np.abs(stat)) <= 1e-5 * max(1.0, np.max(np.abs(lam))), np.max(np.abs(stat))
    with np.errstate(invalid="ignore"):
        bc = np.maximum(np.where(zl > 0, (z - vlo) * zl, 0.0), np.where(zu > 0, (vhi - z) * zu, 0.0))
    assert np.max(bc) <= 1e-3, np.max(bc)
    nu = lam[nd]
    assert abs(nu) > 1e-3 and abs(row[0]) <= 1e-6, (nu, row)      # the row binds
    return nu, float(np.max(bc))


@pytest.mark.parametrize("kind", ["sum", "product"])
def test_solve_64_states_with_a_coupling_row_and_action_bounds(kind, peaks64):
    """A native 64-state model has no spare state for an accumulator, and no accumulator could carry the product row."""
    from oracle.padded_model import PaddedAcrobot
    # (0.8 x, not 0.7 x: at 28.4 the product row ran into the 1000-iteration limit from guess 0 -- dto_amd/problems.py)
    assert abs(U64 - 0.8 * np.min(peaks64)) <= 0.051 and U64 < np.min(peaks64), (U64, peaks64)
    row = (KA, KB, TOTAL_SUM_EQ) if kind == "sum" else (KA, KB, TOTAL_PROD_EQ, False, "product")
    s, p = _solver(SOLVE_T, [row], name="acrobot_padded_g", target=0.5, terminal="physical", u_max=U64)
    T, B = SOLVE_T, SOLVE_B
    assert s.nlp.num_variables == (T - 1) * 65 + 64 and s.general_rows_path == "border" and s.solve_unsupported is None
    zo, lam, status, iters = _solve_batch(s, p, B)
    print(f"[64 states, {kind} row, |u| <= {U64}] status {status.tolist()}, iterations {iters.tolist()}")
    assert np.all(status == 1), (status, iters)
    vlo, vhi = s.nlp.variable_bounds
    spec = _spec([row], 64, 1)
    for b in range(B):
        nu, bc = _kkt_conditions_bounded(PaddedAcrobot(64), T, spec, zo[b], lam[b], vlo, vhi)
        u = zo[b][_u_index(64, T)]
        print(f"  instance {b}: multiplier of the row {nu:.4f}, peak |u| {np.max(np.abs(u)):.6f}, bound complementarity {bc:.2e}")
        assert np.sum(np.abs(u) > U64 - 1e-2) >= 1, np.max(np.abs(u))


def test_24_states_in_the_embedding_on_both_paths():
    """The linear two-knot row beside |u| <= U24: Options.general_rows = "auto" puts it on an accumulator state of the embedding
    (the ordinary tile solver, which takes bounds), "border" keeps it a row (the bordered loop).  Same guess, same minimiser."""
    import dto_amd
    n_, T = 24, SOLVE_T
    row = (KA, KB, 0.2)

    def solve(rows, u_max):
        s, p = _solver(T, [row], n=n_, name="acrobot24g", target=0.4, terminal="physical", options=dto_amd.Options(general_rows=rows),
                       **({} if u_max is None else dict(u_max=u_max)))
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
        dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
        st = dto_amd.solve(s)
        assert st == 1 and s.solve_unsupported is None, (rows, u_max, st, s.iterations)
        return s
    free = solve("auto", None)
    peak = np.max(np.abs(free._solution[_u_index(n_, T)]))
    print(f"[24 states, linear row, no bounds] peak |u| {peak:.4f}")
    assert abs(U24 - 0.7 * peak) <= 0.051 and U24 < peak, (U24, peak)
    sa, sb = solve("auto", U24), solve("border", U24)
    assert sa.general_rows_path == "accumulators" and sb.general_rows_path == "border"
    d = np.max(np.abs(sa._solution - sb._solution))
    ub = sb._solution[_u_index(n_, T)]
    print(f"[24 states, linear row, |u| <= {U24}] accumulators {sa.iterations} iterations, border {sb.iterations} iterations, "
          f"distance of the minimisers {d:.3e}, peak |u| on the border {np.max(np.abs(ub)):.6f}")
    assert np.max(np.abs(ub)) <= U24 + 1e-12 and np.sum(np.abs(ub) > U24 - 1e-2) >= 1
    assert d <= PATH_DISTANCE, d


def test_stepwise_entry_points_and_per_instance_bounds_stay_refused():
    import torch
    from dto_amd import capi
    s, p = _solver(SOLVE_T, [(KA, KB, TOTAL_SUM_EQ)], name="acrobot_padded_g", target=0.5, terminal="physical", u_max=U64)
    nz = s.nlp.num_variables
    z0 = torch.zeros((2, nz), device="cuda", dtype=torch.float64)
    with pytest.raises(capi.DtoError) as e:
        s.begin_batch(z0.data_ptr(), 2, nz)
    assert e.value.code == 4 and "bordered path" in str(e.value)
    vlo, vhi = s.nlp.variable_bounds
    with pytest.raises(capi.DtoError) as e:
        s.set_bounds_batch(np.tile(vlo, (2, 1)), np.tile(vhi, (2, 1)))
    assert e.value.code == 4 and "bordered path" in str(e.value)

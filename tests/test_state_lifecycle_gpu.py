"""Device state of a problem handle across releases and reallocations (csrc/dto_solver.cpp: SolverState / WideState / WideKkt /
KktBorder, all of whose device memory is owned by DevBuf members).

What is pinned: a result does not depend on what the handle held before.  A batch solved again after the state was rebuilt for
another batch size, released (Solver.release_state), rebuilt for another partition count, or after a buffer that is allocated on
first use (the column state and history of the limited-memory mode, the refinement buffers, the multi-solve / refined-solve /
border workspaces of the tile path) came into being, is BIT-identical -- x, multipliers, statuses, iteration counts -- to its first
solve or to what a fresh Solver object gives for that call alone.  Models: the pendulum at T = 6 (lane path) and the 64-state
model at T = 2 / T = 5 with the systems of tests/test_wide_multi_solve_gpu.py (tile path); no plugin beyond those.
"""
import numpy as np
import pytest

from conftest import product_solver
from test_wide_border_gpu import _border_factor, _border_solve
from test_wide_linear_solver_gpu import _assemble_factor, _solve
from test_wide_multi_solve_gpu import _quasi_definite_system, _solve_multi
from test_wide_refined_solve_gpu import _refined

pytestmark = pytest.mark.gpu

T_LANE = 6


def _same(a, b):
    """Bit for bit, NaN included, over a tuple of arrays."""
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _lane_solver(**opts):
    import dto_amd
    from dto_amd import problems as P
    p = P.build_pendulum(T=T_LANE, evaluate_hessian=True)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       options=dto_amd.Options(**opts), name="pendulum")
    return s, p


@pytest.fixture(scope="module")
def guesses():
    """[70][nz] initial points: the model's own random guesses, seeded per instance; a batch of B takes the first B rows."""
    s, p = _lane_solver()
    idx = s.nlp.indices
    Z = np.zeros((70, s.nlp.num_variables))
    for b in range(70):
        xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
        for rows, values in ((idx.states, xs), (idx.actions, us)):      # (1-based indices, as initialize_states / _controls use them)
            for t, v in enumerate(values):
                Z[b, np.asarray(rows[t][:len(v)], dtype=int) - 1] = v
    Z.setflags(write=False)
    return Z


def _lane_solve(s, Z, B):
    import torch
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint       # (the pendulum is solved in its own layout: no embedding)
    z0 = torch.tensor(np.ascontiguousarray(Z[:B]), device="cuda")
    zo = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    mo = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, mo.data_ptr(), nc)
    torch.cuda.synchronize()
    return zo.cpu().numpy(), mo.cpu().numpy(), st.copy(), it.copy()


def test_lane_state_rebuilt_released_and_repartitioned(guesses):
    """B = 3, B = 70 (two tiles: the state is rebuilt), B = 3, release_state, B = 3, two partitions, back to automatic."""
    s, _ = _lane_solver()
    first = _lane_solve(s, guesses, 3)
    assert np.all(first[2] == 1), first[2]
    big = _lane_solve(s, guesses, 70)
    assert np.all(big[2][:3] == 1), big[2]
    assert _same(_lane_solve(s, guesses, 3), first), "after a larger batch"
    s.release_state()
    assert _same(_lane_solve(s, guesses, 3), first), "after release_state"
    s.set_partitions(2)
    two = _lane_solve(s, guesses, 3)
    assert s.partitions() == 2
    assert np.array_equal(two[2], first[2]), (two[2], first[2])          # another elimination order: the same outcome, not the same bits
    s.set_partitions(0)
    assert _same(_lane_solve(s, guesses, 3), first), "back at the automatic partition count"
    s.set_partitions(2)
    s.release_state()                                                   # the request outlives the state it was stored with
    assert _same(_lane_solve(s, guesses, 3), two) and s.partitions() == 2


def test_lane_lazy_buffers(guesses):
    """Limited-memory mode (history block and the column state) then exact on one handle; refinement buffers allocated on a state
    that had run without them, and again after the batch size changed.  Reference: a fresh Solver running that configuration only."""
    import dto_amd
    fresh_lbfgs = _lane_solve(_lane_solver(hessian_approximation="lbfgs")[0], guesses, 3)
    fresh_exact = _lane_solve(_lane_solver()[0], guesses, 3)
    fresh_refined = _lane_solve(_lane_solver(kkt_refinement=1)[0], guesses, 3)
    assert not _same(fresh_lbfgs[:1], fresh_exact[:1])   # (the modes do differ: the comparisons below are not vacuous)
    s, _ = _lane_solver(hessian_approximation="lbfgs")
    assert s.hessian_mode == "lbfgs"
    assert _same(_lane_solve(s, guesses, 3), fresh_lbfgs)
    assert s.hessian_mode_last() == "lbfgs"
    s.hessian_mode = "exact"                              # the mode is a field of dto_options: same plugin, same handle
    assert _same(_lane_solve(s, guesses, 3), fresh_exact), "exact after limited-memory"
    assert s.hessian_mode_last() == "exact"
    s.options = dto_amd.Options(kkt_refinement=1)
    assert _same(_lane_solve(s, guesses, 3), fresh_refined), "refinement buffers on a state that ran without them"
    _lane_solve(s, guesses, 70)
    assert _same(_lane_solve(s, guesses, 3), fresh_refined), "refinement after a change of the batch size"
    s.options = dto_amd.Options()
    assert _same(_lane_solve(s, guesses, 3), fresh_exact), "plain again"


def test_lane_solver_objects_created_and_dropped(guesses):
    """Five Solver objects, one after the other, each closed after its solve.  (Not a statement about device memory: what is free
    on a shared card is not this test's to assert.)"""
    first = None
    for _ in range(5):
        s, _p = _lane_solver()
        got = _lane_solve(s, guesses, 3)
        s.close()
        first = first or got
        assert _same(got, first)


def _fresh_tile_solver(T):
    """A new Solver object (a problem handle of its own) on the session's traced model."""
    import dto_amd
    p = product_solver("acrobot_padded", T)[1]
    return dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name="acrobot_padded")


def _tile_system(rng, B, nz, nc):
    """The quasi-definite settings of _quasi_definite_system, as data: (Z, MU, dw, dc, SX, SC)."""
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
    SX[:, ::3] = 0.0
    return Z, MU, 2.0, 1e-5, SX, SC


def test_tile_stored_factor_across_batch_sizes():
    """assemble / factor / solve at B = 2, B = 3 (every buffer grows), B = 2 again: the two B = 2 solutions agree bit for bit, and
    with the dense solve to the bar of tests/test_wide_multi_solve_gpu.py."""
    sols = []
    for B, seed in ((2, 7), (3, 8), (2, 7)):
        s, Ks, rng, nz, nc = _quasi_definite_system(1, 2, B, 2.0, seed)
        rhs = np.random.default_rng(70 + B)
        RX, RC = rhs.standard_normal((B, nz)), rhs.standard_normal((B, nc))
        oX, oC = _solve(s, RX, RC)
        for b in range(B):
            ref = np.linalg.solve(Ks[b], np.concatenate([RX[b], RC[b]]))
            assert np.max(np.abs(np.concatenate([oX[b], oC[b]]) - ref)) <= 1e-8 * np.max(np.abs(ref))
        sols.append((oX, oC))
    assert _same(sols[0], sols[2])
    assert sols[1][0].shape[0] == 3


def test_tile_workspaces_allocated_on_first_use():
    """One factorisation at T = 5, B = 3; on it: multi-solves of 3 then 17 right-hand sides, a refined solve, borders of 1 then 3
    rows with a solve each.  Every result equals what a fresh Solver gives for that call alone.  Then a solver run on the same
    handle takes the factor storage: dto_kkt_solve reports it as it always has."""
    import torch
    import dto_amd
    from dto_amd import capi
    T, B = 5, 3
    s = _fresh_tile_solver(T)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    system = _tile_system(np.random.default_rng(10), B, nz, nc)
    rng = np.random.default_rng(11)
    R = rng.standard_normal((B, nz + nc))
    multi = {n: (rng.standard_normal((B, n, nz)), rng.standard_normal((B, n, nc))) for n in (3, 17)}
    border = {nb: (rng.standard_normal((B, nb, nz + nc)), np.stack([-np.diag(1e-5 + rng.random(nb)) for _ in range(B)]),
                   rng.standard_normal((B, nb))) for nb in (1, 3)}

    def factored(solver):
        Z, MU, dw, dc, SX, SC = system
        ok, neg = _assemble_factor(solver, Z, MU, dw, dc, SX, SC)
        assert np.all(ok == 1) and np.all(neg == nc), (ok, neg)
        return solver

    def bordered(solver, nb):
        G, C, Sb = border[nb]
        negdef, singular = _border_factor(solver, G, C, nz, nc, True)
        assert np.all(singular == 0), singular
        return _border_solve(solver, R, Sb, nz, nc), negdef, singular

    calls = [("multi 3", lambda v: _solve_multi(v, *multi[3])), ("multi 17", lambda v: _solve_multi(v, *multi[17])),
             ("refined", lambda v: (_refined(v, R, nz, nc, 1),)), ("border 1", lambda v: bordered(v, 1)),
             ("border 3", lambda v: bordered(v, 3))]
    factored(s)
    for name, call in calls:
        got = call(s)
        want = call(factored(_fresh_tile_solver(T)))
        assert np.all(np.isfinite(got[0])), name
        assert _same(got, want), name
    # the solver on the same handle writes the factor storage: the stored factor and the border are gone, the assembled system is not
    s.options = dto_amd.Options(max_iter=2)
    z0 = torch.tensor(system[0], device="cuda")
    zo = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    s.begin_batch(z0.data_ptr(), B, nz)
    st, _it = s.run_batch(zo.data_ptr(), nz)
    torch.cuda.synchronize()
    assert st.shape == (B,)
    with pytest.raises(capi.DtoError, match="dto_kkt_factor has not been called") as e:
        _solve(s, R[:, :nz], R[:, nz:])
    assert e.value.code == 1                              # DTO_ERR_INVALID
    with pytest.raises(capi.DtoError, match="dto_kkt_border_factor has not been called"):
        _border_solve(s, R, border[1][2], nz, nc)
    s.kkt_factor()                                        # ... and a new factorisation of the assembled system serves again
    assert _same((_refined(s, R, nz, nc, 1),), calls[2][1](factored(_fresh_tile_solver(T))))

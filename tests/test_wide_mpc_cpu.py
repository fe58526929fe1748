"""CPU-side checks of the receding-horizon model of the tile path (problems.build_mpc_acrobot_padded): its 64-state embedding
carries the first-knot pin rows x - w as auxiliary states, and those are the rows whose multipliers dto_solver_shift keeps."""
import numpy as np

from _dag_eval import evaluate

from dto_amd import problems as P


def test_mpc_acrobot_pin_rows_ride_auxiliary_states_of_the_embedding():
    from dto_amd.solver import pad_to_wide
    from oracle.padded_model import PaddedAcrobot
    n, T = 24, 5
    rng = np.random.default_rng(3)
    x1 = 0.05 * rng.standard_normal(n)
    p = P.build_mpc_acrobot_padded(T=T, n=n, x1=x1, target=0.5)
    assert [len(w) for w in p["parameters"]] == [n] * T and np.array_equal(p["parameters"][0], x1)
    assert p["constraints"][0].num_constraint == n and all(c.num_constraint == 0 for c in p["constraints"][1:])
    bT = p["bounds"][-1]
    assert np.array_equal(bT.state_lower[:4], [0.5, 0, 0, 0]) and np.array_equal(bT.state_upper[:4], [0.5, 0, 0, 0])
    assert np.all(np.isinf(bT.state_lower[4:]))
    out = pad_to_wide(p["dynamics"], p["objective"], p["constraints"], p["bounds"], True)
    assert out is not None
    dyn, obj, cons, bnds, zmap, mumap, musign = out
    nd = (T - 1) * n
    # the stage rows of the embedding: rows n .. 2n-1 of the first stage, sign flipped -- Solver.shift_batch keeps their multipliers
    assert np.array_equal(mumap[nd:], n + np.arange(n)) and np.all(musign[nd:] == -1.0) and np.all(musign[:nd] == 1.0)
    om = PaddedAcrobot(n)
    X, U, W = rng.random((2, 64)), rng.random(1), rng.random(n)
    env = {("x", i): float(v) for i, v in enumerate(X[0])}
    env.update({("y", i): float(v) for i, v in enumerate(X[1])}); env[("u", 0)] = float(U[0])
    env.update({("w", i): float(v) for i, v in enumerate(W)})
    r = np.array(evaluate(dyn[0].evaluate_expr, env))
    assert np.max(np.abs(r[:n] - om.residual(X[0, :n], U, X[1, :n]))) < 1e-13
    assert np.max(np.abs(r[n:2 * n] - (X[1, n:2 * n] - (X[0, :n] - W)))) < 1e-14        # a_{2,j} - (x_j - w_j)
    # the auxiliary states of knot 2 are fixed at zero (equality rows); none of the other knots has a row
    assert np.all(bnds[1].state_lower[n:] == 0.0) and np.all(bnds[1].state_upper[n:] == 0.0)
    assert dyn[1] is dyn[2] and dyn[0] is not dyn[1]

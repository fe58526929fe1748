"""A GeneralConstraint row that reads parameters (problems.py: build_mpc_pendulum_coupled, theta_15 + theta_35 - w[3] <= 0): the
traced expressions and their Jacobian against the ORACLE's GeneralConstraint(f, nz, nw) (oracle/sympy_models.py), which is handed
the whole flattened parameter vector as the reference does (src/moi.jl:48,68), and the generated General::eval reads w.  Such a
row rides no accumulator state and is not folded: it stays a row of the bordered path."""
import numpy as np

import dto_amd
from dto_amd import problems as P

T = 50
NZ, NW = 2 * T + (T - 1), 4 * T


def _oracle_row():
    from oracle import sympy_models as S
    i15, i35 = 14 * 3, 34 * 3
    return S.GeneralConstraint(lambda z, w: [z[i15] + z[i35] - w[3]], NZ, NW, indices_inequality=[1], evaluate_hessian=False)


def test_parametric_general_row_matches_the_oracle():
    from _dag_eval import evaluate
    p = P.build_mpc_pendulum_coupled(T=T)
    g, og = p["general_constraint"], _oracle_row()
    assert (g.num_variables, g.num_parameter, g.num_constraint, g.num_jacobian) == (NZ, NW, 1, 2)
    assert (og.num_constraint, og.num_jacobian) == (1, 2) and g.indices_inequality == og.indices_inequality == [1]
    assert [list(v) for v in g.jacobian_sparsity] == [list(v) for v in og.jacobian_sparsity]
    rng = np.random.default_rng(3)
    for _ in range(3):
        z, w = rng.standard_normal(NZ), rng.standard_normal(NW)
        env = {("z", i): float(z[i]) for i in range(NZ)}
        env.update({("w", i): float(w[i]) for i in range(NW)})
        got = np.array(evaluate(list(g.evaluate_expr), env))
        ref = og.evaluate(list(z), list(w))
        # three terms, two roundings on either side, in whatever order: 4 ulp of the sum of their magnitudes
        tol = 4 * 2.0 ** -53 * (abs(z[14 * 3]) + abs(z[34 * 3]) + abs(w[3]) + 0.25)
        assert np.max(np.abs(got - ref)) <= tol, (got, ref)
        gj = np.array(evaluate(list(g.jacobian_expr), env))
        assert np.array_equal(gj, og.jacobian(list(z), list(w))), gj
        # the parameter the row reads is entry 3 of the flattened vector, nothing else of w
        w2 = w.copy()
        w2[3] += 0.25
        env.update({("w", 3): float(w2[3])})
        assert abs(evaluate(list(g.evaluate_expr), env)[0] - (got[0] - 0.25)) <= 2 * tol
        w3 = w + 1.0
        w3[3] = w[3]
        env.update({("w", i): float(w3[i]) for i in range(NW)})
        assert evaluate(list(g.evaluate_expr), env)[0] == got[0]


def test_generated_general_code_reads_w_and_the_row_stays_on_the_border():
    from dto_amd.plugin import generate_source
    p = P.build_mpc_pendulum_coupled(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], parameters=p["parameters"], name="mpc_pendulum_coupled")
    assert s.general_rows_path == "border" and s.solve_unsupported is None
    assert s.nlp.num_parameters == NW and s._solve_nlp.sizes.num_constraint_general == 1
    src = generate_source(s._solve_nlp.structure, "mpc_pendulum_coupled")
    general = src[src.index("struct Model::General {"):]
    general = general[:general.index("};")]
    assert "const double* w" in general and "w[3]" in general, general
    # the shared parameters reach the row through the host callbacks too (evaluated on the device: not here)
    assert p["parameters"][0][3] == 1.0

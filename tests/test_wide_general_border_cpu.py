"""CPU-side checks of coupling GeneralConstraint rows on the tile path: a 64-state structure with general rows is a solver
plugin (tile KKT kernels AND the general callbacks), the Solver sends such problems to the bordered path, and a 17 .. 63-state
problem whose row is not a sum of one-knot terms is embedded in the 64 states with the row re-indexed to the embedded layout."""
import numpy as np

from _dag_eval import evaluate

import dto_amd
from dto_amd import problems as P
from dto_amd.plugin import Structure, generate_source

T = 6


def _solver(p, name, **kw):
    return dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                          general_constraint=p["general_constraint"], name=name, **kw)


def test_64_state_structure_with_general_rows_is_a_solver_plugin():
    p = P.build_acrobot_padded(T=T, general_row=(2, 5, 0.2))
    st = Structure(p["dynamics"], p["objective"], p["constraints"], p["general_constraint"], True)
    assert st.wide and st.wide_solver
    src = generate_source(st, "acrobot_padded_g")
    assert "launch_wide<Model>" in src and "wide_info<Model>" in src
    # the general callbacks: the class k_wide_general evaluates, and the flag that instantiates it
    assert "struct Model::General {" in src and "HAS_GENERAL = true" in src and "&k_general" in src
    # stage Constraint rows still make a callbacks-only plugin (the tile kernels have no stage rows)
    pc = P.build_acrobot_padded(T=T, stage_constraints=(0.4, -2.56, 0.1))
    stc = Structure(pc["dynamics"], pc["objective"], pc["constraints"], None, True)
    assert stc.wide and not stc.wide_solver
    assert "launch_wide<Model>" not in generate_source(stc, "acrobot_padded_c")


def test_64_state_solver_takes_the_bordered_path():
    p = P.build_acrobot_padded(T=T, general_row=(2, 5, 0.2))
    s = _solver(p, "acrobot_padded_g")
    assert s.general_rows_path == "border" and s.solve_unsupported is None
    assert s._solve_nlp.num_constraint == (T - 1) * 64 + 1


def test_24_state_product_row_is_embedded_with_its_row_reindexed():
    n_, ka, kb, tot = 24, 2, 5, 0.2
    p = P.build_acrobot_padded(T=T, n=n_, target=0.4, terminal="physical", general_row=(ka, kb, tot, False, "product"))
    assert accumulate_returns_none(p)
    s = _solver(p, "acrobot24gp")
    assert s.solve_unsupported is None and s.general_rows_path == "border"
    assert s._solve_nlp.num_variables == (T - 1) * 65 + 64
    nd = (T - 1) * n_
    zmap, mumap, musign = s._pad
    assert s._solve_nlp.num_constraint == (T - 1) * 64 + 1
    # the general row: behind the embedded dynamics rows, sign +1
    assert mumap.shape == (nd + 1,) and mumap[-1] == (T - 1) * 64 and np.all(musign == 1.0)
    from dto_amd.solver import embed_general_constraint
    g = embed_general_constraint(p["general_constraint"], zmap, s._solve_nlp.num_variables)
    assert g.num_constraint == 1 and g.num_variables == (T - 1) * 65 + 64 and g.num_hessian == 0
    ia, ib = (ka - 1) * (n_ + 1), (kb - 1) * (n_ + 1)
    rng = np.random.default_rng(11)
    for _ in range(3):
        z = rng.random(s.nlp.num_variables)
        zp = s.pad_batch(z)
        env = {("z", i): float(v) for i, v in enumerate(zp)}
        assert abs(evaluate(g.evaluate_expr, env)[0] - (z[ia] * z[ib] - tot)) <= 1e-14
        jv = dict(zip((c - 1 for c in g.jacobian_sparsity[1]), evaluate(g.jacobian_expr, env)))
        assert sorted(jv) == sorted([int(zmap[ia]), int(zmap[ib])])
        assert abs(jv[int(zmap[ia])] - z[ib]) <= 1e-14 and abs(jv[int(zmap[ib])] - z[ia]) <= 1e-14
    assert set(g.jacobian_sparsity[0]) == {1}


def accumulate_returns_none(p):
    from dto_amd.solver import accumulate_general_constraint
    return accumulate_general_constraint(list(p["dynamics"]), list(p["objective"]), list(p["constraints"]), p["bounds"],
                                         p["general_constraint"], True, max_state=63) is None


def test_24_state_linear_row_stays_on_accumulators_unless_asked():
    p = P.build_acrobot_padded(T=T, n=24, target=0.4, terminal="physical", general_row=(2, 5, 0.2))
    assert not accumulate_returns_none(p)


def test_inequality_stage_rows_beside_general_rows_are_refused_with_a_reason():
    p = P.build_acrobot_padded(T=T, n=24, target=0.4, terminal="physical", general_row=(2, 5, 0.2, False, "product"),
                               stage_constraints=(0.4, -2.56, 0.1))
    s = _solver(p, "acrobot24gpc")
    assert s.solve_unsupported is not None
    assert "inequality rows" in s.solve_unsupported and "beside general rows" in s.solve_unsupported

"""Build every model plugin the tests, smoke() and bench.py use, so they travel prebuilt to the GPU box."""
from __future__ import annotations

from . import problems as P
from .plugin import Structure, build_plugin, build_plugins


def _entries():
    return [
        ("pendulum", P.build_pendulum, dict(T=6, evaluate_hessian=True)),
        ("pendulum", P.build_pendulum, dict(T=2, evaluate_hessian=True)),
        ("cartpole", P.build_cartpole, dict(T=5, evaluate_hessian=True)),
        ("acrobot", P.build_acrobot, dict(T=5, evaluate_hessian=True)),
        ("acrobot_bounds", P.build_acrobot, dict(T=4, evaluate_hessian=True, endpoint="bounds")),
        ("car", P.build_car, dict(T=6, evaluate_hessian=True)),
        ("car", P.build_car, dict(T=6, evaluate_hessian=False)),
        ("cartpole", P.build_cartpole, dict(T=5, evaluate_hessian=False)),
        ("pendulum", P.build_pendulum, dict(T=6, evaluate_hessian=False)),
        ("ref_objective", P.build_ref_objective, {}),
        ("ref_dynamics", P.build_ref_dynamics, {}),
        ("ref_constraints", P.build_ref_constraints, {}),
        ("ref_hesslag", P.build_ref_hesslag, {}),
        ("ref_general", P.build_ref_general, dict(user_jacobian=False)),
        ("ref_general", P.build_ref_general, dict(user_jacobian=True)),
        ("ref_general_coupled", P.build_ref_general_coupled, {}),
        ("acrobot_coupled", P.build_acrobot_coupled, dict(T=8)),
        ("param_pendulum", P.build_param_pendulum, dict(T=8)),
        ("ref_userjac", P.build_ref_userjac, {}),
        ("mpc_pendulum", P.build_mpc_pendulum, dict(T=5)),
        ("acrobot_padded", P.build_acrobot_padded, dict(T=3)),
        ("acrobot_padded", P.build_acrobot_padded, dict(T=2)),
        ("acrobot_padded", P.build_acrobot_padded, dict(T=3, evaluate_hessian=False)),
        ("acrobot", P.build_acrobot, dict(T=5, evaluate_hessian=False)),
    ]


def tile_border_solvers():
    """The problems of tests/test_wide_general_border_*.py: coupling GeneralConstraint rows on the tile path (64 states, and 24
    states through the embedding).  Knots, totals and names are literals of the generated code, so every problem is a plugin of
    its own; constructing the Solver builds what it loads (the callbacks plugin and, for 24 states, the embedded solver form).  Returns the
    names."""
    from .solver import Options, Solver

    def solver(name, rows, options=None, **kw):
        p = P.build_acrobot_padded(general_row=list(rows) if len(rows) > 1 else rows[0], **kw)
        Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
               general_constraint=p["general_constraint"], options=options, name=name)
        return name

    pairs = lambda count, T: [(a, b) for a in range(1, T + 1) for b in range(a + 1, T + 1)][:count]
    tot = P.ACROBOT_PADDED_COUPLING_TOTALS
    out = [solver("acrobot_padded_g", [(2, 5, 0.2)], T=6),
           solver("acrobot24gp", [(2, 5, 0.2, False, "product")], T=6, n=24, target=0.4, terminal="physical"),
           solver("acrobot24gpc", [(2, 5, 0.2, False, "product")], T=6, n=24, target=0.4, terminal="physical",
                  stage_constraints=(0.4, -2.56, 0.1))]
    for m in (1, 2):
        out.append(solver(f"acrobot_padded_g_m{m}", [(2, 5, 0.2), (3, 6, 0.1, False, "product")], T=6, m=m))
    for count in (16, 17):
        out.append(solver(f"acrobot_padded_g{count}", [(a, b, 0.1 * (j + 1)) for j, (a, b) in enumerate(pairs(count, 8))], T=8))
    # one row more than the limited-memory mode takes beside its compact matrix (tests/test_wide_lbfgs_rows_cpu.py)
    out.append(solver("acrobot_padded_g5", [(a, b, 0.1 * (j + 1)) for j, (a, b) in enumerate(pairs(5, 6))], T=6))
    # ... and the reference's default build (no Hessians) of the two-row problem: its callbacks plugin ("auto" keeps the exact substitute)
    import warnings
    from .solver import HessianModeNotice
    p0 = P.build_acrobot_padded(T=6, general_row=[(2, 5, 0.2), (3, 6, 0.1, False, "product")], evaluate_hessian=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", HessianModeNotice)
        Solver(p0["dynamics"], p0["objective"], p0["constraints"], p0["bounds"], evaluate_hessian=False,
               general_constraint=p0["general_constraint"], name="acrobot_padded_g_m1")
    out.append("acrobot_padded_g_m1")
    for row in ((10, 20, tot["sum"]), (10, 20, tot["product"], False, "product"), (10, 20, tot["sum<=0"], True)):
        out.append(solver("acrobot_padded_g", [row], T=30, target=0.5, terminal="physical"))
    out.append(solver("acrobot24gp", [(10, 20, tot["product24"], False, "product")], T=30, n=24, target=0.4, terminal="physical"))
    out.append(solver("acrobot24g", [(10, 20, 0.2)], T=30, n=24, target=0.4, terminal="physical", options=Options(general_rows="border")))
    return out


def all_structures():
    out = []
    for name, builder, kw in _entries():
        p = builder(**kw)
        out.append((name, Structure(p["dynamics"], p["objective"], p["constraints"], p.get("general_constraint"),
                                    p["evaluate_hessian"])))
        if p.get("general_constraint") is not None:
            # the solver's internal form of a stage-local general constraint (solver.py:fold_general_constraint)
            from .solver import fold_general_constraint
            folded = fold_general_constraint(p["dynamics"], p["objective"], p["constraints"], p["general_constraint"],
                                             p["evaluate_hessian"])
            if folded is not None:
                out.append((name + "_folded", Structure(p["dynamics"], p["objective"], folded[0], None, p["evaluate_hessian"])))
    return out


def build_all(verbose: bool = False):
    items = list(all_structures())
    # the solver-internal exact-Hessian clones of the evaluate_hessian=false models are compiled in the same parallel batch
    from .solver import _with_exact_hessians, fold_general_constraint
    for name, builder, kw in _entries():
        p = builder(**kw)
        if p["evaluate_hessian"] or p.get("general_constraint") is not None:
            continue
        up = _with_exact_hessians(list(p["dynamics"]), list(p["objective"]), list(p["constraints"]))
        if up is not None:
            items.append((name, Structure(up[0], up[1], up[2], None, True)))
    paths = build_plugins(items, verbose=verbose)
    # the solver-internal forms (exact-Hessian clones of evaluate_hessian=false models, solver.py:_with_exact_hessians):
    # constructing the Solver builds whatever it will load; no device is needed for that
    from .solver import Solver
    for name, builder, kw in _entries():
        p = builder(**kw)
        if p["evaluate_hessian"]:
            continue
        try:
            Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=False,
                   general_constraint=p.get("general_constraint"), parameters=p.get("parameters"), name=name)
        except Exception as e:  # a model the solver does not take (callbacks only) still has its callback plugin above
            if verbose:
                print(f"prebuild: no solver form for {name}: {e}")
    return paths

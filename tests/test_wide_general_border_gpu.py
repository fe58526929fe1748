"""Coupling GeneralConstraint rows on the tile path (64 states, and 17 .. 63 states in their 64-state embedding): the bordered
KKT step -- stored factor of the stage part, one panel substitution for the border rows, one bordered solve -- and the
host-driven filter line-search loop around it (csrc/dto_solver.cpp: bordered_step_tile, general_solve_batch).

Reference: numpy's dense solve of [H + dw I, J'; J, -dc I] with H and the dynamics rows of J from the ORACLE
(oracle/padded_model.py: dense_derivatives) and the general rows from their closed forms below (the rows are Hessian-free in the
solver: a product row contributes to J, not to H).  Tolerance of the steps: the project's 1e-8 of max |solution| (SURVEY.md
section 8, tests/test_wide_gpu.py); of the solves: the limits of the tile-path solve tests of tests/test_wide_gpu.py.

The totals of the solve tests are literals of the generated plugins (a plugin per total), so they are fixed numbers here: each
was taken from the solution WITHOUT the row (free value + 0.3 for the equality rows -- + 0.1 for the 64-state product row, see
there -- and free sum - 0.3 for the inequality row, rounded to two decimals) and the tests check that against a fresh solve
without the row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DW, DC = 0.8, 1e-6          # the values of tests/test_bordered_gpu.py

# rows of the step tests: (knot a, knot b, total, inequality, kind) -- q1[a] + q1[b] - total, or q1[a] * q1[b] - total
STEP_ROWS = [(2, 5, 0.2), (3, 6, 0.1, False, "product")]


def _spec(rows, n, m):
    return [((r[0] - 1) * (n + m), (r[1] - 1) * (n + m), float(r[2]), len(r) > 4 and r[4] == "product") for r in rows]


def _row_values(spec, z):
    return np.array([(z[ia] * z[ib] if prod else z[ia] + z[ib]) - tot for ia, ib, tot, prod in spec])


def _row_jacobian(spec, z):
    G = np.zeros((len(spec), len(z)))
    for j, (ia, ib, _, prod) in enumerate(spec):
        G[j, ia] += z[ib] if prod else 1.0
        G[j, ib] += z[ia] if prod else 1.0
    return G


def _solver(T, rows, n=64, m=1, name="acrobot_padded_g", options=None, **kw):
    import dto_amd
    from dto_amd import problems as P
    p = P.build_acrobot_padded(T=T, n=n, m=m, general_row=list(rows) if len(rows) > 1 else rows[0], **kw)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], name=name, options=options)
    return s, p


def _kkt_step(s, Z, MU, dw, dc):
    import torch
    B, nz = Z.shape
    nc = MU.shape[1]
    dz, dmu = torch.tensor(Z, device="cuda"), torch.tensor(MU, device="cuda")
    dx = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    dl = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    ok = s.kkt_step_batch(dz.data_ptr(), B, nz, dmu.data_ptr(), nc, dw, dc, dx.data_ptr(), nz, dl.data_ptr(), nc)
    torch.cuda.synchronize()
    return dx.cpu().numpy(), dl.cpu().numpy(), ok


def _dense_bordered(om, T, spec, z, mu, dw, dc):
    """K and right-hand side of the bordered Newton-KKT system, rows in the reference order [dynamics; general]"""
    from oracle.padded_model import dense_derivatives
    nd = (T - 1) * om.n
    _, g, c, J, H = dense_derivatives(om, T, z, mu[:nd], 1.0)
    Ja = np.vstack([J, _row_jacobian(spec, z)])
    ca = np.concatenate([c, _row_values(spec, z)])
    nz, nc = len(z), len(ca)
    K = np.block([[H + dw * np.eye(nz), Ja.T], [Ja, -dc * np.eye(nc)]])
    return K, -np.concatenate([g + Ja.T @ mu, ca])


def _check_step(s, om, T, spec, B, seed):
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    assert nc == (T - 1) * 64 + len(spec) and s.general_rows_path == "border" and s.solve_unsupported is None
    rng = np.random.default_rng(seed)
    Z, MU = rng.random((B, nz)), rng.random((B, nc))
    dx, dl, ok = _kkt_step(s, Z, MU, DW, DC)
    want = True
    for b in range(B):
        K, rhs = _dense_bordered(om, T, spec, Z[b], MU[b], DW, DC)
        eig = np.linalg.eigvalsh(K)
        want = want and int(np.sum(eig < 0)) == nc
        sol = np.linalg.solve(K, rhs)
        scale = np.max(np.abs(sol))
        ex, el = np.max(np.abs(dx[b] - sol[:nz])), np.max(np.abs(dl[b] - sol[nz:]))
        print(f"  instance {b}: error {ex:.2e} / {el:.2e} (general rows {np.max(np.abs(dl[b][-len(spec):] - sol[-len(spec):])):.2e}), "
              f"solution scale {scale:.2e}")
        assert ex <= 1e-8 * scale and el <= 1e-8 * scale, (b, ex, el, scale)
    assert bool(ok) == want, (ok, want)
    return Z, MU


@pytest.mark.parametrize("m", [1, 2])
def test_bordered_kkt_step_on_the_tile_path_matches_dense_solve(m):
    from oracle.padded_model import PaddedAcrobot
    T, B = 6, 3
    s, _ = _solver(T, STEP_ROWS, m=m, name=f"acrobot_padded_g_m{m}")
    om = PaddedAcrobot(64, m)
    spec = _spec(STEP_ROWS, 64, m)
    Z, MU = _check_step(s, om, T, spec, B, 21 + m)
    # a negative delta_w: wrong inertia, reported
    nc = s.nlp.num_constraint
    for b in range(B):
        K, _ = _dense_bordered(om, T, spec, Z[b], MU[b], -DW, DC)
        assert int(np.sum(np.linalg.eigvalsh(K) < 0)) != nc
    _, _, ok = _kkt_step(s, Z, MU, -DW, DC)
    assert not ok


def _pairs(count, T):
    return [(a, b) for a in range(1, T + 1) for b in range(a + 1, T + 1)][:count]


def test_sixteen_border_rows_and_the_seventeenth_refused():
    from dto_amd import capi
    from oracle.padded_model import PaddedAcrobot
    T, B = 8, 2
    rows = [(a, b, 0.1 * (j + 1)) for j, (a, b) in enumerate(_pairs(16, T))]
    s, _ = _solver(T, rows, name="acrobot_padded_g16")
    _check_step(s, PaddedAcrobot(64), T, _spec(rows, 64, 1), B, 77)
    rows17 = [(a, b, 0.1 * (j + 1)) for j, (a, b) in enumerate(_pairs(17, T))]
    s17, _ = _solver(T, rows17, name="acrobot_padded_g17")
    nz, nc = s17.nlp.num_variables, s17.nlp.num_constraint
    rng = np.random.default_rng(78)
    with pytest.raises(capi.DtoError) as e:
        _kkt_step(s17, rng.random((1, nz)), rng.random((1, nc)), DW, DC)
    assert e.value.code == 4 and "more than 16 border rows" in str(e.value)


def test_linear_solver_with_general_rows_present():
    """dto_kkt_assemble / factor / solve / multiply on a problem with general rows: K is the stage part (dimension Nz + Ns), the
    tail of every constraint-side array is neither read (NaN in the inputs) nor written (NaN stays in the outputs)."""
    import torch
    from oracle.padded_model import PaddedAcrobot, dense_kkt
    T, B = 6, 3
    s, _ = _solver(T, STEP_ROWS, name="acrobot_padded_g_m1")
    om = PaddedAcrobot(64)
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    ns = nc - 2
    rng = np.random.default_rng(31)
    Z, MU, RX, RC = rng.random((B, nz)), rng.random((B, nc)), rng.standard_normal((B, nz)), rng.standard_normal((B, nc))
    MU[:, ns:] = np.nan
    RC[:, ns:] = np.nan
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    nan = lambda n: torch.full((B, n), float("nan"), device="cuda", dtype=torch.float64)
    dZ, dMU, dRX, dRC = dev(Z), dev(MU), dev(RX), dev(RC)
    s.kkt_assemble(dZ.data_ptr(), B, nz, dMU.data_ptr(), nc, DW, DC)
    ok, neg = s.kkt_factor()
    assert np.all(neg == ns) and np.all(ok == 1), (ok, neg, ns)
    oX, oC, pX, pC = nan(nz), nan(nc), nan(nz), nan(nc)
    s.kkt_solve(dRX.data_ptr(), nz, dRC.data_ptr(), nc, oX.data_ptr(), nz, oC.data_ptr(), nc)
    s.kkt_multiply(oX.data_ptr(), nz, oC.data_ptr(), nc, pX.data_ptr(), nz, pC.data_ptr(), nc)
    torch.cuda.synchronize()
    oX, oC, pX, pC = (a.cpu().numpy() for a in (oX, oC, pX, pC))
    assert np.all(np.isnan(oC[:, ns:])) and np.all(np.isnan(pC[:, ns:]))
    for b in range(B):
        K, _ = dense_kkt(om, T, Z[b], MU[b, :ns], DW, DC)
        rhs = np.concatenate([RX[b], RC[b, :ns]])
        sol = np.linalg.solve(K, rhs)
        got = np.concatenate([oX[b], oC[b, :ns]])
        scale = np.max(np.abs(sol))
        err = np.max(np.abs(got - sol))
        # K_s sol, formed by the device, against the right-hand side: relative to the size of the terms of the product
        res = np.max(np.abs(np.concatenate([pX[b], pC[b, :ns]]) - rhs))
        bound = 1e-8 * np.max(np.abs(K) @ np.abs(sol))
        print(f"  instance {b}: error {err:.2e} (scale {scale:.2e}), residual {res:.2e} (bound {bound:.2e})")
        assert err <= 1e-8 * scale and res <= bound


# ---- solves ------------------------------------------------------------------------------------------------------------------
SOLVE_T, SOLVE_B, KA, KB = 30, 3, 10, 20
from dto_amd.problems import ACROBOT_PADDED_COUPLING_TOTALS as _TOTALS   # (shared with prebuild.py: a plugin per total)
TOTAL_SUM_EQ, TOTAL_PROD_EQ, TOTAL_SUM_INEQ, TOTAL_PROD_24 = (_TOTALS[k] for k in ("sum", "product", "sum<=0", "product24"))


def _free_solution(n, target, name):
    import dto_amd
    from dto_amd import problems as P
    p = P.build_acrobot_padded(T=SOLVE_T, n=n, target=target, terminal="physical")
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, name=name)
    xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
    assert dto_amd.solve(s) == 1
    z = s._solution
    return z[(KA - 1) * (n + 1)], z[(KB - 1) * (n + 1)]


@pytest.fixture(scope="module")
def free64():
    return _free_solution(64, 0.5, "acrobot_padded")


def _kkt_conditions(om, T, spec, z, lam, vlo, vhi, inequality):
    from oracle.padded_model import dense_derivatives
    nd = (T - 1) * om.n
    _, g, c, J, _ = dense_derivatives(om, T, z, lam[:nd], 1.0)
    row, G = _row_values(spec, z), _row_jacobian(spec, z)
    fixed = vlo == vhi
    assert np.max(np.abs(c)) <= 1e-6, np.max(np.abs(c))
    assert np.max(np.abs(z[fixed] - vlo[fixed])) < 1e-12, np.max(np.abs(z[fixed] - vlo[fixed]))
    r = g + J.T @ lam[:nd] + G.T @ lam[nd:]
    assert np.max(np.abs(r[~fixed])) <= 1e-5 * max(1.0, np.max(np.abs(lam))), np.max(np.abs(r[~fixed]))
    nu = lam[nd]
    assert abs(nu) > 1e-3, nu                                  # the row binds
    if inequality:
        assert row[0] <= 1e-6 and nu >= -1e-9 and abs(nu * row[0]) <= 1e-3, (row, nu)
    else:
        assert abs(row[0]) <= 1e-6, row
    return nu


@pytest.mark.parametrize("kind", ["sum", "product", "sum<=0"])
def test_solve_64_states_with_a_coupling_row(kind, free64):
    import torch
    from oracle.padded_model import PaddedAcrobot
    qa, qb = free64
    if kind == "sum":
        tot, free = TOTAL_SUM_EQ, qa + qb + 0.3
    elif kind == "product":
        # (+ 0.1, not + 0.3: towards the free value, because at + 0.3 -- the product would have to change sign -- the guesses of
        #  instances 0 and 2 ran into the 1000-iteration limit; instance 1 converged in 256 iterations)
        tot, free = TOTAL_PROD_EQ, qa * qb + 0.1
    else:
        tot, free = TOTAL_SUM_INEQ, qa + qb - 0.3
    assert abs(tot - free) <= 5.1e-3, (kind, tot, free)         # the literal is the free value +- 0.3, to two decimals
    row = (KA, KB, tot, kind == "sum<=0") + (("product",) if kind == "product" else ())
    s, p = _solver(SOLVE_T, [row], name="acrobot_padded_g", target=0.5, terminal="physical")
    T, B = SOLVE_T, SOLVE_B
    nz, nc = s.nlp.num_variables, s.nlp.num_constraint
    assert nc == (T - 1) * 64 + 1 and s.general_rows_path == "border"
    import dto_amd
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
    print(f"[64 states, {kind} row, total {tot}] status {status.tolist()}, iterations {iters.tolist()}")
    assert np.all(status == 1), (status, iters)
    assert s.hessian_mode_last() == "exact"
    zo, lam = zo.cpu().numpy(), lo_.cpu().numpy()
    vlo, vhi = s.nlp.variable_bounds
    spec = _spec([row], 64, 1)
    for b in range(B):
        nu = _kkt_conditions(PaddedAcrobot(64), T, spec, zo[b], lam[b], vlo, vhi, kind == "sum<=0")
        print(f"  instance {b}: multiplier of the row {nu:.4f}")


def test_stepwise_entry_points_and_per_instance_bounds_are_refused():
    import torch
    from dto_amd import capi
    row = (KA, KB, TOTAL_SUM_EQ)
    s, p = _solver(SOLVE_T, [row], name="acrobot_padded_g", target=0.5, terminal="physical")
    nz = s.nlp.num_variables
    z0 = torch.zeros((2, nz), device="cuda", dtype=torch.float64)
    with pytest.raises(capi.DtoError) as e:
        s.begin_batch(z0.data_ptr(), 2, nz)
    assert e.value.code == 4 and "bordered path" in str(e.value)
    vlo, vhi = s.nlp.variable_bounds
    with pytest.raises(capi.DtoError) as e:
        s.set_bounds_batch(np.tile(vlo, (2, 1)), np.tile(vhi, (2, 1)))
    assert e.value.code == 4 and "bordered path" in str(e.value)


def test_24_state_product_row_solved_through_the_embedding():
    import dto_amd
    from oracle.padded_model import PaddedAcrobot
    n_, T = 24, SOLVE_T
    qa, qb = _free_solution(n_, 0.4, "acrobot24")
    assert abs(TOTAL_PROD_24 - (qa * qb + 0.3)) <= 5.1e-3, (TOTAL_PROD_24, qa * qb + 0.3)
    row = (KA, KB, TOTAL_PROD_24, False, "product")
    s, p = _solver(T, [row], n=n_, name="acrobot24gp", target=0.4, terminal="physical")
    assert s.general_rows_path == "border" and s.solve_unsupported is None and s._solve_nlp.num_variables == (T - 1) * 65 + 64
    xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
    assert dto_amd.solve(s) == 1, (s.status, s.iterations)
    zs, ls = s._solution, s._duals
    nd = (T - 1) * n_
    assert zs.shape == (s.nlp.num_variables,) and ls.shape == (nd + 1,)
    vlo, vhi = s.nlp.variable_bounds
    nu = _kkt_conditions(PaddedAcrobot(n_), T, _spec([row], n_, 1), zs, ls, vlo, vhi, False)
    print(f"[24 states, product row through the embedding] {s.iterations} iterations, multiplier {nu:.4f}")


def test_24_state_linear_row_on_the_border_when_asked():
    """The linear two-knot row of tests/test_wide_gpu.py rides an accumulator state by default (checked there);
    Options(general_rows="border") keeps it a row of the embedded problem."""
    import dto_amd
    from oracle.padded_model import PaddedAcrobot
    n_, T = 24, SOLVE_T
    row = (KA, KB, 0.2)
    s, p = _solver(T, [row], n=n_, name="acrobot24g", target=0.4, terminal="physical", options=dto_amd.Options(general_rows="border"))
    assert s.general_rows_path == "border" and s.solve_unsupported is None
    xs, us = p["guess"](np.random.Generator(np.random.PCG64(0)))
    dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
    assert dto_amd.solve(s) == 1, (s.status, s.iterations)
    zs, ls = s._solution, s._duals
    assert ls.shape == ((T - 1) * n_ + 1,)
    vlo, vhi = s.nlp.variable_bounds
    nu = _kkt_conditions(PaddedAcrobot(n_), T, _spec([row], n_, 1), zs, ls, vlo, vhi, False)
    print(f"[24 states, linear row on the border] {s.iterations} iterations, multiplier {nu:.4f}")

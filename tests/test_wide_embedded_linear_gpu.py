"""The stored-factor calls of the tile path on EMBEDDED problems: dto_kkt_assemble / factor / solve / solve_multi / multiply /
solve_refined on 24-state models in the solver's layout (64 states per knot), where solver.py: pad_to_wide gives every stage kind
a Dynamics class of its own -- the first knot's rows, interior obstacle rows, the last stage with the last knot's rows as functions
of y -- plus constant rows y_q = 0 and padding rows y_q - x_q = 0.  The kernels walk such a horizon through dispatch_wk(kind[t]);
k_wide_kmul carries the y-y Hessian and V' vx + E' vl from one stage into the next, across kinds and across chunk edges.

Reference everywhere: oracle/padded_model.py: embedded_dense_kkt (pinned in tests/test_wide_embedded_oracle_cpu.py) plus
diag([sigma_x; -sigma_c]); numpy.linalg.solve for solves, np.longdouble for products and residuals.  No bounds: the linear-solver
calls ignore them, auxiliary and padding states are free variables.  Point, multipliers (those of auxiliary rows too, so the
-lam c'' term is live), sigmas and right-hand sides are random in the solver's layout; delta_w is the smaller of {2, 30} at which
every oracle matrix has inertia (nz, nc, 0).

Bars: the project's 1e-8 of max |solution| / max |K v|; for the refined solve the bars of
tests/test_wide_refined_solve_gpu.py: omega after two passes <= (q + 1) 2^-53, forward error <= 1e-8.
"""
import numpy as np
import pytest

from test_wide_kmul_gpu import _check as _check_product, _multiply
from test_wide_linear_solver_gpu import _dev, _solve
from test_wide_multi_solve_gpu import _check as _check_multi, _solve_multi
from test_wide_refined_solve_gpu import _omega, _refined

pytestmark = pytest.mark.gpu

N, NPHYS, B, DC = 64, 24, 3, 1e-5
DISC = (0.4, -2.56, 0.1)
PAR2 = (1.2, 0.8)
#        plugin name,   m, T, stage rows
CASES = {"rows5": ("acrobot24c", 1, 5, True),      # four stages: first kind, two of the middle kind, last kind
         "free5": ("acrobot24", 1, 5, False),
         "two4": ("acrobot24u2", 2, 4, False),
         "rows10": ("acrobot24c", 1, 10, True)}     # S = 8: chunk 1 of k_wide_kmul is the last-kind stage + the terminal knot

_SOLVERS, _MODELS, _SYSTEMS = {}, {}, {}


def _problem(name):
    from dto_amd import problems as P
    plugin, m, T, with_rows = CASES[name]
    return P.build_acrobot_padded(T=T, n=NPHYS, m=m, target=0.4, terminal="physical", parameters=PAR2 if m == 2 else None,
                                  stage_constraints=DISC if with_rows else None)


def _solver(name):
    import dto_amd
    if name not in _SOLVERS:
        p = _problem(name)
        _SOLVERS[name] = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                                        parameters=p["parameters"], name=CASES[name][0])
    return _SOLVERS[name]


def _oracle(name):
    from oracle.padded_model import PaddedAcrobot, PaddedStageRows
    _, m, T, with_rows = CASES[name]
    if m not in _MODELS:
        _MODELS[m] = PaddedAcrobot(NPHYS, m, PAR2 if m == 2 else None)
    x1, xT = np.zeros(NPHYS), np.zeros(NPHYS)
    xT[0] = 0.4
    return _MODELS[m], (PaddedStageRows(NPHYS, m, T, x1, xT, *DISC) if with_rows else None)


def _matrices(name, Z, MU, SX, SC, dw):
    from oracle.padded_model import embedded_dense_kkt
    model, rows = _oracle(name)
    T = CASES[name][2]
    return [embedded_dense_kkt(model, rows, T, Z[b], MU[b], dw, DC) + np.diag(np.concatenate([SX[b], -SC[b]])) for b in range(B)]


def _inertia_ok(Ks, nz, nc):
    for K in Ks:
        eig = np.linalg.eigvalsh(K)
        if (int(np.sum(eig > 0)), int(np.sum(eig < 0))) != (nz, nc):
            return False
    return True


def _system(name):
    """Point, sigmas and the oracle's matrices of one case: computed once, shared by the tests, never changed."""
    if name not in _SYSTEMS:
        _, m, T, _ = CASES[name]
        nz, nc = (T - 1) * (N + m) + N, (T - 1) * N
        rng = np.random.default_rng(sum(map(ord, name)))
        Z, MU = rng.random((B, nz)), rng.random((B, nc))
        SX, SC = rng.random((B, nz)) * 3.0, rng.random((B, nc)) * 0.5
        SX[:, ::3] = 0.0
        for dw in (2.0, 30.0):
            Ks = _matrices(name, Z, MU, SX, SC, dw)
            if _inertia_ok(Ks, nz, nc):
                break
        else:
            raise AssertionError("no delta_w of {2, 30} makes every test matrix quasi-definite")
        for a in (Z, MU, SX, SC, *Ks):
            a.setflags(write=False)
        _SYSTEMS[name] = dict(m=m, T=T, nz=nz, nc=nc, dw=dw, Z=Z, MU=MU, SX=SX, SC=SC, Ks=Ks)
    return _SYSTEMS[name]


def _assemble(s, c, dw=None, MU=None):
    nz, nc = c["nz"], c["nc"]
    assert (nz, nc) == (s._solve_nlp.num_variables, s._solve_nlp.num_constraint) and s._pad is not None
    keep = [_dev(c["Z"]), _dev(c["MU"] if MU is None else MU), _dev(c["SX"]), _dev(c["SC"])]
    s.kkt_assemble(keep[0].data_ptr(), B, nz, keep[1].data_ptr(), nc, c["dw"] if dw is None else dw, DC,
                   sigma_x_ptr=keep[2].data_ptr(), ldsx=nz, sigma_c_ptr=keep[3].data_ptr(), ldsc=nc)


def _factor(s, nc):
    ok, neg = s.kkt_factor()
    assert np.all(neg == nc) and np.all(ok == 1), (neg, ok, nc)


def _three_solves(s, Ks, rng, nz, nc):
    worst = 0.0
    for _ in range(3):
        RX, RC = rng.standard_normal((B, nz)), rng.standard_normal((B, nc))
        oX, oC = _solve(s, RX, RC)
        for b in range(B):
            sol = np.linalg.solve(Ks[b], np.concatenate([RX[b], RC[b]]))
            scale = np.max(np.abs(sol))
            ex, ec = np.max(np.abs(oX[b] - sol[:nz])), np.max(np.abs(oC[b] - sol[nz:]))
            worst = max(worst, ex / scale, ec / scale)
            print(f"  instance {b}: error {ex:.2e} / {ec:.2e}, solution scale {scale:.2e}")
            assert ex <= 1e-8 * scale and ec <= 1e-8 * scale, (b, ex, ec, scale)
    return worst


@pytest.mark.parametrize("name", ["rows5", "free5", "two4"])
def test_embedded_solve_matches_dense_solves(name):
    """Assemble, factor (negative pivots = rows, inertia flag set), three substitution-only solves; then a second assemble with
    another delta_w and other multipliers on the same handle (a stale record or a stale multiplier would show)."""
    s, c = _solver(name), _system(name)
    nz, nc = c["nz"], c["nc"]
    rng = np.random.default_rng(11)
    _assemble(s, c)
    _factor(s, nc)
    worst = _three_solves(s, c["Ks"], rng, nz, nc)
    dw2, MU2 = c["dw"] + 7.0, rng.random((B, nc))
    Ks2 = _matrices(name, c["Z"], MU2, c["SX"], c["SC"], dw2)
    assert _inertia_ok(Ks2, nz, nc), "test point must be quasi-definite"
    _assemble(s, c, dw2, MU2)
    _factor(s, nc)
    worst = max(worst, _three_solves(s, Ks2, rng, nz, nc))
    print(f"  {name}: delta_w = {c['dw']}, worst error / solution scale {worst:.2e}")


@pytest.mark.parametrize("nrhs", [3, 17])
def test_embedded_multi_solve_matches_dense_solves(nrhs):
    """Below one block of columns and one block plus a tail; four padded leading dimensions, NaN in the padding."""
    s, c = _solver("rows5"), _system("rows5")
    nz, nc = c["nz"], c["nc"]
    _assemble(s, c)
    _factor(s, nc)
    rng = np.random.default_rng(20 + nrhs)
    RX, RC = rng.standard_normal((B, nrhs, nz)), rng.standard_normal((B, nrhs, nc))
    oX, oC = _solve_multi(s, RX, RC, ldrx=nz + 5, ldrc=nc + 3, ldsx=nz + 7, ldsc=nc + 1)
    _check_multi(c["Ks"], RX, RC, oX, oC, 1e-8)


def _units(nz, nc, where):
    V = np.zeros((len(where), nz + nc))
    for b, i in enumerate(where):
        V[b, i] = 1.0
    return V


def test_embedded_product_matches_the_oracle():
    """Random vectors and columns of K on the four-stage case: an auxiliary state of the knot after x_1 (fed by the first-kind
    stage, read by a middle-kind one), an auxiliary state of the last knot fed by the rows that are functions of y, a padding
    state; the multiplier of such a row of the last stage, of a row of the first stage, of a padding row."""
    s, c = _solver("rows5"), _system("rows5")
    nz, nc, T = c["nz"], c["nc"], c["T"]
    _assemble(s, c)
    rng = np.random.default_rng(31)
    kn = N + 1                                                   # variables per knot
    aux1, auxT, pad = 1 * kn + NPHYS + 3, (T - 1) * kn + NPHYS + 1 + 2, 2 * kn + 55
    lamT, lam0, lamp = nz + (T - 2) * N + NPHYS + 1 + 2, nz + 0 * N + NPHYS + 6, nz + 2 * N + 55
    worst = 0.0
    for what, V in (("random", rng.standard_normal((B, nz + nc))),
                    ("unit aux state of knot 1 / aux state of the last knot / padding state", _units(nz, nc, (aux1, auxT, pad))),
                    ("unit multiplier of a last-knot row / first-knot row / padding row", _units(nz, nc, (lamT, lam0, lamp)))):
        for b in range(B):
            assert np.any(c["Ks"][b] @ V[b] != 0.0)
        worst = max(worst, _check_product(_multiply(s, V, nz, nc), c["Ks"], V, what))
    # the unit vectors hit what they are meant to: the last-knot rows have entries in the y block of the last stage
    K = c["Ks"][0]
    assert np.count_nonzero(K[lamT, (T - 1) * kn:(T - 1) * kn + NPHYS]) >= 1 and K[lamT, auxT] == 1.0 and K[lamp, pad] == -1.0
    print(f"  rows5: worst componentwise figure {worst:.2e}")


def test_embedded_product_chunk_edge_between_stage_kinds():
    """T = 10 with 8 stages per workgroup: chunk 1 holds the last-kind stage and the terminal knot, the left edge it recomputes for
    the carry is a middle-kind stage."""
    s, c = _solver("rows10"), _system("rows10")
    nz, nc, T = c["nz"], c["nc"], c["T"]
    assert T - 1 == 8 + 1
    _assemble(s, c)
    rng = np.random.default_rng(32)
    kn = N + 1
    x8, a8, l7 = 8 * kn + 1, 8 * kn + NPHYS, nz + 7 * N + NPHYS      # knot 8: y of stage 7 (chunk 0), x of stage 8 (chunk 1)
    worst = 0.0
    for what, V in (("random", rng.standard_normal((B, nz + nc))),
                    ("unit x / aux state of the knot on the chunk edge / multiplier of the row left of it", _units(nz, nc, (x8, a8, l7)))):
        worst = max(worst, _check_product(_multiply(s, V, nz, nc), c["Ks"], V, what))
    print(f"  rows10: worst componentwise figure {worst:.2e}")


def test_embedded_refined_backward_and_forward_error():
    """omega for passes = 0, 1, 2 (printed), the bars on passes = 2.  The reference itself (numpy's LU plus one float64
    refinement step) is checked against the omega bar first, on the host."""
    s, c = _solver("rows5"), _system("rows5")
    nz, nc = c["nz"], c["nc"]
    R = np.random.default_rng(41).standard_normal((B, nz + nc))
    dense, bars = [], []
    for b, K in enumerate(c["Ks"]):
        q = int(np.max(np.sum(K != 0.0, axis=1)))
        x = np.linalg.solve(K, R[b])
        x = x + np.linalg.solve(K, R[b] - K @ x)
        ref = _omega(K, x, R[b])
        print(f"  instance {b}: q = {q}, bar {(q + 1) * 2.0 ** -53:.2e}, omega of numpy's LU + one refinement step {ref:.2e}")
        assert ref <= (q + 1) * 2.0 ** -53, ("the reference misses the bar", b, ref)
        dense.append(x); bars.append((q + 1) * 2.0 ** -53)
    _assemble(s, c)
    _factor(s, nc)
    sols = [_refined(s, R, nz, nc, k) for k in (0, 1, 2)]
    for b, K in enumerate(c["Ks"]):
        om = [_omega(K, sols[k][b], R[b]) for k in range(3)]
        scale = np.max(np.abs(dense[b]))
        fe = [float(np.max(np.abs(sols[k][b] - dense[b])) / scale) for k in range(3)]
        print(f"  instance {b}: omega passes 0/1/2 = {om[0]:.2e} / {om[1]:.2e} / {om[2]:.2e}, "
              f"forward error 0/1/2 = {fe[0]:.2e} / {fe[1]:.2e} / {fe[2]:.2e}, bar {bars[b]:.2e}")
        assert om[2] <= bars[b], (b, om, bars[b])
        assert fe[2] <= 1e-8, (b, fe)


def test_embedded_round_trip_through_the_problem_layout():
    """The documented route: a right-hand side that is zero outside zmap / mumap, the solution mapped back with unpad_batch (stage
    rows come back with the opposite sign) equals the oracle's embedded solve at those positions."""
    s, c = _solver("rows5"), _system("rows5")
    nz, nc, T, m = c["nz"], c["nc"], c["T"], c["m"]
    # the maps from the definition of the embedding: states 0 .. 23 and the action of every knot; the dynamics rows of every
    # stage, then the stage rows knot by knot (the last knot's behind the last stage's own)
    zmap = np.concatenate([np.concatenate([t * (N + m) + np.arange(NPHYS), t * (N + m) + N + np.arange(m if t < T - 1 else 0)])
                           for t in range(T)]).astype(np.int64)
    q = [NPHYS + 1] + [1] * (T - 2) + [5]
    mumap = np.concatenate([t * N + np.arange(NPHYS) for t in range(T - 1)]
                           + [t * N + NPHYS + np.arange(q[t]) for t in range(T - 1)] + [(T - 2) * N + NPHYS + q[T - 2] + np.arange(q[T - 1])])
    musign = np.concatenate([np.ones((T - 1) * NPHYS), -np.ones(sum(q))])
    assert np.array_equal(s._pad[0], zmap) and np.array_equal(s._pad[1], mumap) and np.array_equal(s._pad[2], musign)
    rng = np.random.default_rng(51)
    RX, RC = np.zeros((B, nz)), np.zeros((B, nc))
    RX[:, zmap], RC[:, mumap] = rng.standard_normal((B, len(zmap))), rng.standard_normal((B, len(mumap)))
    _assemble(s, c)
    _factor(s, nc)
    oX, oC = _solve(s, RX, RC)
    gx, gc = s.unpad_batch(oX), s.unpad_batch(oC, multipliers=True)
    assert gx.shape == (B, s.nlp.num_variables) and gc.shape == (B, s.nlp.num_constraint)
    for b in range(B):
        sol = np.linalg.solve(c["Ks"][b], np.concatenate([RX[b], RC[b]]))
        scale = np.max(np.abs(sol))
        ex, ec = np.max(np.abs(gx[b] - sol[:nz][zmap])), np.max(np.abs(gc[b] - sol[nz:][mumap] * musign))
        print(f"  instance {b}: error {ex:.2e} / {ec:.2e}, solution scale {scale:.2e}")
        assert ex <= 1e-8 * scale and ec <= 1e-8 * scale, (b, ex, ec, scale)

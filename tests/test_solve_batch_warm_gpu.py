"""dto_solve_batch_warm: the host-driven bordered loop (csrc/dto_solver.cpp: general_solve_batch) started from a primal-dual point
the caller owns and returning the whole point -- Solver.solve_batch_warm / Solver.new_point / Point.

Problems and bars are those of the neighbouring files: the MPC pendulum with a per-instance budget row of
tests/test_border_params_gpu.py (lane border, T = 50, B = 5), the 64-state sum row of tests/test_wide_general_border_gpu.py (tile
border, T = 30, B = 3) and the 64-state limited-memory problem of tests/test_wide_lbfgs_solve_gpu.py (T = 16, B = 3).  Each cold
solve runs once per module and is shared.

What is asserted: bit equality with dto_solve_batch for start = NULL; 0 iterations and an unchanged point when a converged point
whose bounds and inequality rows are inactive is handed back (the loop tests convergence before its first step); bit equality of a
warm batch with the warm solves of its instances alone; convergence to KKT points (oracle derivatives; violation <= 1e-6, which a
converged status implies at tol = 1e-6, stationarity <= 1e-5 max(1, |lam|), complementarity <= 1e-3 = compl_inf_tol) of warm
re-solves after a shift and a new measured state.  Iteration counts, warm against cold, are printed and never asserted.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _clone(pt, rows=None):
    """a deep copy of a Point (optionally of some instances)"""
    from dto_amd import Point
    out = Point()
    for k in ("x", "mu", "zl", "zu", "slack", "barrier", "qn_s", "qn_y"):
        v = getattr(pt, k)
        if v is not None:
            setattr(out, k, (v if rows is None else v[rows]).clone().contiguous())
    for k in ("qn_npairs", "qn_sigma"):
        v = getattr(pt, k)
        if v is not None:
            setattr(out, k, np.ascontiguousarray(v if rows is None else v[rows]).copy())
    return out


def _nan_point(s, B):
    pt = s.new_point(B)
    for k in ("x", "mu", "zl", "zu", "slack", "barrier", "qn_s", "qn_y"):
        if getattr(pt, k) is not None:
            getattr(pt, k).fill_(float("nan"))
    return pt


def _cold_both(s, Z, W=None):
    """solve_batch and solve_batch_warm(start = None) from the same guesses"""
    import torch
    B, nz, nc = Z.shape[0], s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    z0 = torch.tensor(Z, device="cuda")
    kw = {}
    if W is not None:
        w = torch.tensor(W, device="cuda")
        kw = dict(params_ptr=w.data_ptr(), ldp=W.shape[1])
    zo = torch.full((B, nz), float("nan"), device="cuda", dtype=torch.float64)
    lo = torch.full((B, nc), float("nan"), device="cuda", dtype=torch.float64)
    st, it = s.solve_batch(z0.data_ptr(), B, nz, zo.data_ptr(), nz, lo.data_ptr(), nc, **kw)
    torch.cuda.synchronize()
    end = _nan_point(s, B)
    st2, it2 = s.solve_batch_warm(B, None, end, x0_ptr=z0.data_ptr(), ldx=nz, **kw)
    torch.cuda.synchronize()
    return dict(st=st, it=it, z=_np(zo), lam=_np(lo), st2=st2, it2=it2, end=end)


def _assert_cold_equal(r):
    assert np.array_equal(r["st"], r["st2"]) and np.array_equal(r["it"], r["it2"]), (r["st"], r["st2"], r["it"], r["it2"])
    assert np.array_equal(r["z"], _np(r["end"].x)) and np.array_equal(r["lam"], _np(r["end"].mu))
    for k in ("zl", "zu", "slack", "barrier"):
        assert np.all(np.isfinite(_np(getattr(r["end"], k)))), k


# ---- the three problems ------------------------------------------------------------------------------------------------------
def _lane():
    if "lane" not in _CACHE:
        import test_border_params_gpu as L
        x1s, goals, us = L._instances()
        s = L._coupled_solver()
        Z = L._guesses(s, x1s, goals, us)
        W = np.stack([np.tile([x1s[b, 0], x1s[b, 1], goals[b], L.TOTALS[b]], L.T) for b in range(L.B)])
        r = _cold_both(s, Z, W)
        print(f"[lane border, T = {L.T}, B = {L.B}] cold status {r['st'].tolist()}, iterations {r['it'].tolist()}")
        _CACHE["lane"] = dict(r, s=s, W=W, x1s=x1s, goals=goals, totals=L.TOTALS, T=L.T, B=L.B)
    return _CACHE["lane"]


def _sum64():
    if "sum64" not in _CACHE:
        import dto_amd
        import test_wide_general_border_gpu as G
        row = (G.KA, G.KB, G.TOTAL_SUM_EQ, False)
        s, p = G._solver(G.SOLVE_T, [row], name="acrobot_padded_g", target=0.5, terminal="physical")
        Z = np.zeros((G.SOLVE_B, s.nlp.num_variables))
        for b in range(G.SOLVE_B):
            xs, us = p["guess"](np.random.Generator(np.random.PCG64(b)))
            dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, [0.1 * u for u in us])
            Z[b] = s._z0
        r = _cold_both(s, Z)
        print(f"[tile border, 64 states, sum row, T = {G.SOLVE_T}] cold status {r['st'].tolist()}, iterations {r['it'].tolist()}")
        _CACHE["sum64"] = dict(r, s=s, B=G.SOLVE_B)
    return _CACHE["sum64"]


def _lbfgs64():
    if "lbfgs64" not in _CACHE:
        import test_wide_lbfgs_solve_gpu as Q
        s, p = Q._solver64()
        r = _cold_both(s, Q._guesses(s, p, range(Q.B)))
        print(f"[tile path, limited-memory, T = {Q.T}] cold status {r['st'].tolist()}, iterations {r['it'].tolist()}, "
              f"pairs {r['end'].qn_npairs.tolist()}")
        _CACHE["lbfgs64"] = dict(r, s=s, p=p, B=Q.B, T=Q.T)
    return _CACHE["lbfgs64"]


# ---- 1. cold equals dto_solve_batch ----------------------------------------------------------------------------------------------
def test_cold_start_equals_solve_batch_on_the_lane_border():
    r = _lane()
    assert np.all(r["st"] == 1), (r["st"], r["it"])
    _assert_cold_equal(r)
    e = r["end"]
    # no finite variable bound: zl = zu = 0; one inequality general row: a positive slack / multiplier pair with s nu of the order
    # of the barrier parameter (<= compl_inf_tol), zeros in the entries of the equality rows
    assert not np.any(_np(e.zl)) and not np.any(_np(e.zu))
    sl, mu, bar = _np(e.slack), _np(e.mu), _np(e.barrier)
    assert not np.any(sl[:, :-1]) and np.all(sl[:, -1] > 0) and np.all(mu[:, -1] > 0) and np.all(bar > 0)
    assert np.all(sl[:, -1] * mu[:, -1] <= 1e-3), sl[:, -1] * mu[:, -1]
    z = _np(e.x)
    row = z[:, 14 * 3] + z[:, 34 * 3] - np.array(r["totals"])
    assert np.max(np.abs(row + sl[:, -1])) <= 1e-6, row + sl[:, -1]       # c + s = 0 to the solver's tolerance


def test_cold_start_equals_solve_batch_on_the_tile_border():
    r = _sum64()
    assert np.all(r["st"] == 1), (r["st"], r["it"])
    _assert_cold_equal(r)
    e = r["end"]
    for k in ("zl", "zu", "slack", "barrier"):     # variables free or fixed, equality rows: nothing of a barrier
        assert not np.any(_np(getattr(e, k))), k
    assert r["s"].hessian_mode_last() == "exact"


def test_cold_start_equals_solve_batch_in_limited_memory_mode():
    r = _lbfgs64()
    assert np.all(r["st"] == 1), (r["st"], r["it"])
    _assert_cold_equal(r)
    e = r["end"]
    for k in ("zl", "zu", "slack", "barrier"):
        assert not np.any(_np(getattr(e, k))), k
    assert np.all((e.qn_npairs >= 1) & (e.qn_npairs <= 6)) and np.all(e.qn_sigma > 0) and np.all(np.isfinite(e.qn_sigma))
    S, Y = _np(e.qn_s), _np(e.qn_y)
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(Y))
    for b in range(r["B"]):
        k = int(e.qn_npairs[b])
        sy = np.sum(S[b, :k] * Y[b, :k], axis=1)
        assert np.all(sy > 0), (b, sy)                                 # every kept pair passed the curvature test
    assert r["s"].hessian_mode_last() == "lbfgs"


def test_bound_multipliers_come_back_with_action_bounds():
    """the bounded case of tests/test_wide_lbfgs_solve_gpu.py (|u| <= 0.9 or 0.95 of the free peak), its bars: complementarity 1e-3,
    stationarity 1e-5 with the RETURNED multipliers subtracted"""
    import torch
    import test_wide_lbfgs_solve_gpu as Q
    ref = _lbfgs64()
    T = ref["T"]
    u_idx = np.array([t * 65 + 64 for t in range(T - 1)])
    peak = float(np.max(np.abs(ref["z"][0][u_idx])))
    for frac in (0.9, 0.95):
        s, p = Q._solver64(u_max=frac * peak)
        r = _cold_both(s, Q._guesses(s, p, [0]))
        print(f"  u_max = {frac} x {peak:.4f}: status {r['st'][0]}, {r['it'][0]} iterations")
        if r["st"][0] == 1:
            break
    assert r["st"][0] == 1
    _assert_cold_equal(r)
    z, lam, zl, zu = r["z"][0], r["lam"][0], _np(r["end"].zl)[0], _np(r["end"].zu)[0]
    vlo, vhi = s.nlp.variable_bounds
    fixed = vlo == vhi
    fl, fh = np.isfinite(vlo) & ~fixed, np.isfinite(vhi) & ~fixed
    assert fl.sum() == T - 1 and fh.sum() == T - 1
    assert not np.any(zl[~fl]) and not np.any(zu[~fh]), "0 at infinite sides and fixed variables"
    assert np.all(zl[fl] > 0) and np.all(zu[fh] > 0)
    viol, rr = Q._kkt(z, lam)
    stat = rr - zl + zu
    stat[fixed] = 0.0
    compl = max(np.max((z - vlo)[fl] * zl[fl]), np.max((vhi - z)[fh] * zu[fh]))
    print(f"  violation {viol:.2e}, stationarity {np.max(np.abs(stat)):.2e}, complementarity {compl:.2e}, barrier {_np(r['end'].barrier)}")
    assert viol <= 1e-6 and np.max(np.abs(stat)) <= 1e-5 and compl <= 1e-3
    torch.cuda.synchronize()


# ---- 2. fixed point ----------------------------------------------------------------------------------------------------------------
def _hand_back(s, end, rows, W=None):
    import torch
    start = _clone(end, rows)
    B = len(rows)
    out = _nan_point(s, B)
    kw = {}
    if W is not None:
        w = torch.tensor(W[rows], device="cuda")
        kw = dict(params_ptr=w.data_ptr(), ldp=W.shape[1])
    st, it = s.solve_batch_warm(B, start, out, **kw)
    torch.cuda.synchronize()
    assert list(st) == [1] * B and list(it) == [0] * B, (st, it)
    assert np.array_equal(_np(out.x), _np(end.x)[rows]) and np.array_equal(_np(out.mu), _np(end.mu)[rows])
    return out


def test_a_converged_point_handed_back_takes_no_iteration_tile_border():
    r = _sum64()
    _hand_back(r["s"], r["end"], list(range(r["B"])))


def test_a_converged_point_handed_back_takes_no_iteration_limited_memory():
    r = _lbfgs64()
    out = _hand_back(r["s"], r["end"], list(range(r["B"])))
    assert np.array_equal(out.qn_npairs, r["end"].qn_npairs) and np.array_equal(_np(out.qn_s), _np(r["end"].qn_s))


def test_a_converged_point_handed_back_takes_no_iteration_lane_border():
    """instances 1 and 3 of the pendulum batch: their budget does not bind; slack, multiplier and barrier parameter come back too"""
    r = _lane()
    out = _hand_back(r["s"], r["end"], [1, 3], r["W"])
    assert np.array_equal(_np(out.slack), _np(r["end"].slack)[[1, 3]]) and np.array_equal(_np(out.barrier), _np(r["end"].barrier)[[1, 3]])


# ---- 5. MPC re-solve on the lane border, 3. each instance alone -------------------------------------------------------------------
def _pendulum_plant():
    from dto_amd import problems as P

    def step(x, u):
        y = np.array(x, dtype=float)
        for _ in range(200):
            y_new = np.array(y - P.pendulum_midpoint(y, x, np.array([u]), None), dtype=float)
            if np.max(np.abs(y_new - y)) < 1e-15:
                return y_new
            y = y_new
        return y
    return step


def _lane_mpc():
    """solve, shift by one knot, a new measured x1 in the parameters (plant step + 1e-3 disturbance), solve warm"""
    if "lane_mpc" not in _CACHE:
        import torch
        r = _lane()
        s, B, T = r["s"], r["B"], r["T"]
        pt = _clone(r["end"])
        s.shift_point(pt, 1)
        z = _np(r["end"].x)
        plant = _pendulum_plant()
        rng = np.random.default_rng(5)
        X = np.array([plant(z[b][:2], z[b][2]) for b in range(B)]) + 1e-3 * rng.standard_normal((B, 2))
        W = np.stack([np.tile([X[b, 0], X[b, 1], r["goals"][b], r["totals"][b]], T) for b in range(B)])
        w = torch.tensor(W, device="cuda")
        start = _clone(pt)
        end = _nan_point(s, B)
        st, it = s.solve_batch_warm(B, start, end, params_ptr=w.data_ptr(), ldp=W.shape[1])
        torch.cuda.synchronize()
        # cold from the same x, for the record
        cold = _nan_point(s, B)
        stc, itc = s.solve_batch_warm(B, None, cold, x0_ptr=pt.x.data_ptr(), ldx=pt.x.shape[1], params_ptr=w.data_ptr(), ldp=W.shape[1])
        torch.cuda.synchronize()
        print(f"[lane border MPC step] warm status {st.tolist()}, iterations {it.tolist()}; cold from the same x: {stc.tolist()}, {itc.tolist()}; "
              f"first solve {r['it'].tolist()}")
        _CACHE["lane_mpc"] = dict(start=pt, end=end, st=st, it=it, W=W, X=X)
    return _CACHE["lane_mpc"]


def test_mpc_resolve_on_the_lane_border_converges_to_kkt_points():
    import test_border_params_gpu as L
    from test_solve_gpu import kkt_report
    r, m = _lane(), _lane_mpc()
    assert np.all(m["st"] == 1), (m["st"], m["it"])
    z, lam = _np(m["end"].x), _np(m["end"].mu)
    for b in range(r["B"]):
        rep = kkt_report(L._oracle(m["X"][b], r["goals"][b], r["totals"][b]), z[b], r["s"].multipliers_to_reference(lam[b]))
        print(f"  instance {b}:", {k: (float(v) if not isinstance(v, bool) else v) for k, v in rep.items()})
        assert rep["violation"] <= 1e-6 and rep["sign_ok"] and rep["compl"] <= 1e-3, (b, rep)
        assert rep["stationarity"] <= 1e-5 * max(1.0, np.max(np.abs(lam[b]))), (b, rep)
        assert np.max(np.abs(z[b][:2] - m["X"][b])) <= 1e-6


def _lane_warm(rows):
    """the warm solve of _lane_mpc for some instances of the batch, as a batch of their own"""
    import torch
    r, m = _lane(), _lane_mpc()
    s = r["s"]
    start, end = _clone(m["start"], rows), _nan_point(s, len(rows))
    w = torch.tensor(m["W"][rows], device="cuda")
    st, it = s.solve_batch_warm(len(rows), start, end, params_ptr=w.data_ptr(), ldp=m["W"].shape[1])
    torch.cuda.synchronize()
    return st, it, {k: _np(getattr(end, k)) for k in ("x", "mu", "slack", "barrier")}


@pytest.mark.parametrize("separators", ["cyclic reduction, batch of 4", "sequential walk, batch of 5"])
def test_each_instance_equals_its_warm_solve_alone_lane_border(separators, monkeypatch):
    """Bit for bit.  On the lane path the arithmetic of an instance is decided by the size class of its batch, on purpose
    (csrc/dto_solver.cpp: fill_kkt_args, sep_cr): the separator system of the time-partitioned factorisation is solved by cyclic
    reduction in batches of at most DTO_SEP_CR_MAX_INST = 4 instances and by a walk over the separators in larger ones, so an
    instance of a batch of FIVE and its solve alone differ in their last bits -- measured here first, warm and on the cold
    dto_solve_batch of the code as it was: equal iteration counts, max |dx| 8.9e-16 .. 2.7e-15, a solve alone equal to the same
    instance in a batch of two.  The property is therefore stated inside each class: the first four rollouts (budget active for 0
    and 2, inactive for 1 and 3) as a batch of four against their solves alone with the default settings, and the batch of five
    against the solves alone with DTO_SEP_CR=0 (read at every call), which sends both through the walk."""
    r = _lane()
    if separators.startswith("sequential"):
        monkeypatch.setenv("DTO_SEP_CR", "0")
        rows = list(range(r["B"]))
    else:
        rows = [0, 1, 2, 3]
    stb, itb, batch = _lane_warm(rows)
    assert np.all(stb == 1), (stb, itb)
    worst = {}
    for j, b in enumerate(rows):
        st, it, alone = _lane_warm([b])
        assert st[0] == stb[j] and it[0] == itb[j], (b, st, it, stb, itb)
        worst[b] = {k: float(np.max(np.abs(alone[k][0] - batch[k][j]))) for k in alone}
        print(f"  {separators}: instance {b} alone against the batch: {it[0]} iterations, max |difference| {worst[b]}")
    assert all(v == 0.0 for d in worst.values() for v in d.values()), worst


def test_warm_resolve_with_the_host_border(monkeypatch):
    """DTO_BORDER_HOST=1 (read at every call).  The host border takes equality rows and free or fixed variables only, so this case
    is the pendulum with the EQUALITY coupling row of tests/test_border_bounds_gpu.py without action bounds (build_pendulum_coupled,
    T = 50, theta_15 + theta_35 = 1) in place of the budget row, whose inequality that border refuses; its initial state is no
    parameter, so the re-solve starts from the converged point with a 1e-3 perturbation of x in place of a new measured state."""
    import torch
    import dto_amd
    from dto_amd import problems as P
    from test_general_accumulators_gpu import _oracle
    from test_solve_gpu import kkt_report
    T = 50
    p = P.build_pendulum_coupled(T=T, total=1.0, inequality=False)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], options=dto_amd.Options(general_rows="border"), name="pendulum_coupled")
    assert s.general_rows_path == "border" and s.solve_unsupported is None
    rng = np.random.Generator(np.random.PCG64(5))
    dto_amd.initialize_states(s, dto_amd.linear_interpolation(p["x1"], p["xT"], T))
    dto_amd.initialize_controls(s, [0.1 * rng.standard_normal(1) for _ in range(T - 1)])
    nz = s.nlp.num_variables
    z0 = torch.tensor(np.asarray(s._z0)[None, :], device="cuda")
    monkeypatch.setenv("DTO_BORDER_HOST", "1")
    first = _nan_point(s, 1)
    st, it = s.solve_batch_warm(1, None, first, x0_ptr=z0.data_ptr(), ldx=nz)
    torch.cuda.synchronize()
    assert st[0] == 1, (st, it)
    start = _clone(first)
    start.x += 1e-3 * torch.tensor(np.random.default_rng(5).standard_normal((1, nz)), device="cuda")
    end = _nan_point(s, 1)
    st2, it2 = s.solve_batch_warm(1, start, end)
    torch.cuda.synchronize()
    print(f"[host border] cold {it[0]} iterations, warm from the perturbed point {it2[0]}")
    assert st2[0] == 1, (st2, it2)
    lam = _np(end.mu)[0]
    rep = kkt_report(_oracle("pendulum_coupled", total=1.0, inequality=False), _np(end.x)[0], s.multipliers_to_reference(lam))
    assert rep["violation"] <= 1e-6 and rep["stationarity"] <= 1e-5 * max(1.0, np.max(np.abs(lam))), rep


# ---- 6. MPC re-solve on the tile path, limited-memory; 3. each instance alone --------------------------------------------------------
def _tile_mpc():
    """build_mpc_acrobot_padded(T = 16, n = 24), limited-memory: solve, shift by one knot, the measured state (plant step + 1e-3
    disturbance) as the pin parameters, solve warm with the history in the point and without it."""
    if "tile_mpc" not in _CACHE:
        import torch
        import dto_amd
        from dto_amd import problems as P
        from test_wide_mpc_gpu import _plant, TARGET
        T, B, n = 16, 3, 24
        p = P.build_mpc_acrobot_padded(T=T, n=n, target=TARGET)
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, parameters=p["parameters"],
                           options=dto_amd.Options(hessian_approximation="limited-memory"), name="acrobot24mpc")
        assert s.solve_unsupported is None and s.hessian_mode == "lbfgs"
        nz, nw = s._solve_nlp.num_variables, s._solve_nlp.num_parameters
        rng = np.random.default_rng(5)
        X = 0.05 * rng.standard_normal((B, n))
        Z = np.zeros((B, nz))
        for b in range(B):
            xs, us = P.build_mpc_acrobot_padded(T=T, n=n, x1=X[b], target=TARGET)["guess"](np.random.Generator(np.random.PCG64(b)))
            dto_amd.initialize_states(s, xs); dto_amd.initialize_controls(s, us)
            Z[b] = s.pad_batch(s._z0)
        z0, w = torch.tensor(Z, device="cuda"), torch.tensor(np.tile(X, (1, T)), device="cuda")
        first = _nan_point(s, B)
        st, it = s.solve_batch_warm(B, None, first, x0_ptr=z0.data_ptr(), ldx=nz, params_ptr=w.data_ptr(), ldp=nw)
        torch.cuda.synchronize()
        print(f"[24 states, limited-memory, T = {T}] cold status {st.tolist()}, iterations {it.tolist()}")
        out = dict(s=s, T=T, B=B, n=n, st0=st, it0=it, X0=X, first=first)
        if np.all(st == 1):
            zr = s.unpad_batch(_np(first.x))
            plant = _plant(n)
            X1 = np.array([plant(X[b], zr[b][n]) for b in range(B)]) + 1e-3 * rng.standard_normal((B, n))
            pt = _clone(first)
            s.shift_point(pt, 1)
            W1 = np.tile(X1, (1, T))
            w1 = torch.tensor(W1, device="cuda")
            runs = {}
            for name in ("history", "no history"):
                start = _clone(pt)
                if name == "no history":
                    start.qn_s = start.qn_y = start.qn_npairs = start.qn_sigma = None
                end = _nan_point(s, B)
                st1, it1 = s.solve_batch_warm(B, start, end, params_ptr=w1.data_ptr(), ldp=nw)
                torch.cuda.synchronize()
                runs[name] = dict(start=start, end=end, st=st1, it=it1)
            cold = _nan_point(s, B)
            stc, itc = s.solve_batch_warm(B, None, cold, x0_ptr=pt.x.data_ptr(), ldx=nz, params_ptr=w1.data_ptr(), ldp=nw)
            torch.cuda.synchronize()
            print(f"[24 states, limited-memory MPC step] warm with the history {runs['history']['it'].tolist()}, without {runs['no history']['it'].tolist()}, "
                  f"cold from the same x {itc.tolist()} (status {stc.tolist()})")
            out.update(runs=runs, X1=X1, W1=W1)
        _CACHE["tile_mpc"] = out
    return _CACHE["tile_mpc"]


@pytest.mark.parametrize("history", ["history", "no history"])
def test_mpc_resolve_on_the_tile_path_in_limited_memory_mode(history):
    from oracle.padded_model import PaddedAcrobot, kkt_residual_blockwise
    m = _tile_mpc()
    assert np.all(m["st0"] == 1), ("the cold solve of build_mpc_acrobot_padded in limited-memory mode", m["st0"], m["it0"])
    s, T, n, B = m["s"], m["T"], m["n"], m["B"]
    run = m["runs"][history]
    assert np.all(run["st"] == 1), (run["st"], run["it"])
    assert s.hessian_mode_last() == "lbfgs"
    zs, ms = _np(run["end"].x), _np(run["end"].mu)
    zr, lr = s.unpad_batch(zs), s.unpad_batch(ms, multipliers=True)
    om = PaddedAcrobot(n)
    vlo, vhi = s.nlp.variable_bounds
    free = vlo != vhi
    nd = (T - 1) * n
    for b in range(B):
        c, r = kkt_residual_blockwise(om, T, zr[b], lr[b][:nd])
        r[:n] += lr[b][nd:nd + n]
        viol = max(np.max(np.abs(c)), np.max(np.abs(zr[b][:n] - m["X1"][b])))
        stat = np.max(np.abs(r[free]))
        print(f"  {history}, instance {b}: {run['it'][b]} iterations, violation {viol:.2e}, stationarity {stat:.2e}")
        assert viol <= 1e-6, (b, viol)
        assert stat <= 1e-5 * max(1.0, np.max(np.abs(lr[b]))), (b, stat)


def test_each_instance_equals_its_warm_solve_alone_limited_memory():
    import torch
    m = _tile_mpc()
    assert np.all(m["st0"] == 1), (m["st0"], m["it0"])
    s, run = m["s"], m["runs"]["history"]
    nw = m["W1"].shape[1]
    for b in range(m["B"]):
        start, end = _clone(run["start"], [b]), _nan_point(s, 1)
        w = torch.tensor(m["W1"][[b]], device="cuda")
        st, it = s.solve_batch_warm(1, start, end, params_ptr=w.data_ptr(), ldp=nw)
        torch.cuda.synchronize()
        assert st[0] == run["st"][b] and it[0] == run["it"][b], (b, st, it, run["st"], run["it"])
        for k in ("x", "mu", "qn_s", "qn_y"):
            assert np.array_equal(_np(getattr(end, k))[0], _np(getattr(run["end"], k))[b]), (b, k)
        assert end.qn_npairs[0] == run["end"].qn_npairs[b] and end.qn_sigma[0] == run["end"].qn_sigma[b]


# ---- 7. argument checks --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_written():
    import torch
    import dto_amd
    from dto_amd import capi
    r = _sum64()
    s, B = r["s"], r["B"]
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    good = _clone(r["end"])

    def refused(start, end, code, B_=B, untouched=None):
        with pytest.raises(capi.DtoError) as e:
            s.solve_batch_warm(B_, start, end)
        assert e.value.code == code, (e.value.code, str(e.value))
        torch.cuda.synchronize()
        for k in ("x", "mu", "zl", "zu", "slack", "barrier"):
            v = getattr(untouched if untouched is not None else end, k)
            if v is not None and not isinstance(v, tuple):
                assert bool(torch.all(torch.isnan(v))), k
        return str(e.value)

    INVALID, UNSUPPORTED = 1, 4
    end = _nan_point(s, B)
    short = _clone(good); short.x = (good.x.data_ptr(), nz - 1)
    refused(short, end, INVALID)                                            # a leading dimension that is too short (start)
    short = _clone(good); short.mu = (good.mu.data_ptr(), nc - 1)
    refused(short, end, INVALID)
    short = _clone(good); short.slack = (good.slack.data_ptr(), nc - 1)
    refused(short, end, INVALID)
    e2 = _nan_point(s, B); keep = e2.zl; e2.zl = (e2.zl.data_ptr(), nz - 1)
    refused(good, e2, INVALID); assert bool(torch.all(torch.isnan(keep)))   # ... and of the end point
    one = _clone(good); one.zu = None
    refused(one, end, INVALID)                                              # only one of zl / zu
    e2 = _nan_point(s, B); e2.zl = None
    refused(good, e2, INVALID)
    part = _clone(good); part.qn_s = torch.zeros((B, 6, nz), device="cuda", dtype=torch.float64)
    refused(part, end, INVALID)                                             # a partial history
    part.qn_y = part.qn_s.clone(); part.qn_sigma = np.ones(B)
    refused(part, end, INVALID)
    part.qn_npairs = np.full(B, 7, dtype=np.int32)
    refused(part, end, INVALID)                                             # more pairs than the history holds
    part.qn_npairs = np.zeros(B, dtype=np.int32); part.qn_sigma = np.zeros(B)
    refused(part, end, INVALID)
    refused(good, end, INVALID, B_=0)                                       # B < 1
    nox = _clone(good); nox.x = None
    nox_end = _nan_point(s, B)
    with pytest.raises(capi.DtoError) as e:
        s.solve_batch_warm(B, nox, nox_end)
    assert e.value.code == INVALID
    # a problem of the ordinary tile loop: refused, the message names the warm start it has
    import test_wide_lbfgs_solve_gpu as Q
    s2, _ = Q._solver64(option="exact")
    end2 = _nan_point(s2, 1)
    with pytest.raises(capi.DtoError) as e:
        s2.solve_batch_warm(1, None, end2, x0_ptr=end2.x.data_ptr(), ldx=end2.x.shape[1])
    assert e.value.code == UNSUPPORTED and "dto_solver_begin_warm" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(end2.mu))) and bool(torch.all(torch.isnan(end2.zl)))
    # and of the ordinary lane loop
    from conftest import product_solver
    s3, _ = product_solver("pendulum", 6)
    end3 = _nan_point(s3, 1)
    with pytest.raises(capi.DtoError) as e:
        s3.solve_batch_warm(1, None, end3, x0_ptr=end3.x.data_ptr(), ldx=end3.x.shape[1])
    assert e.value.code == UNSUPPORTED and "dto_solver_begin_warm" in str(e.value), str(e.value)

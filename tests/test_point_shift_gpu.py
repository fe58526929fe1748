"""dto_point_shift (Solver.shift_point): the receding-horizon shift of dto_solver_shift applied to a caller's primal-dual point,
against the numpy restatement of the index map that tests/test_wide_mpc_gpu.py keeps for dto_solver_shift (_shift_ref) -- exact
equality, since the call only moves numbers.  No solve is needed: the arrays hold random values, NaN in the padding behind every
row (ld larger than the row), which must stay NaN.

T = 5 and T = 16, knots 1, 2 and T - 2, on
  * the 2-state MPC pendulum (lane path; the multipliers of its stage rows behind the dynamics rows stay),
  * the 64-state model in the limited-memory mode (all 12 history vectors of an instance shift like x),
  * a 24-state problem embedded in 64 states with a GeneralConstraint row on the border (a general-row tail) and a keep mask
    (dto_solver_shift_keep_rows) on some dynamics rows;
then the Solver's own keep mask on the embedded MPC problem, and the refusals.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 3


def _solver(kind, T):
    import dto_amd
    from dto_amd import problems as P
    if kind == "pendulum":
        p = P.build_mpc_pendulum(T=T)
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, parameters=p["parameters"],
                           name="mpc_pendulum")
        return s, 2, 1, None
    if kind == "acrobot64":
        p = P.build_acrobot_padded(T=T, target=0.5, terminal="physical", u_max=1.0)
        s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                           options=dto_amd.Options(hessian_approximation="limited-memory"), name="acrobot_padded")
        return s, 64, 1, None
    p = P.build_acrobot_padded(T=T, n=24, target=0.4, terminal="physical", general_row=(2, 4, 0.2))
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       general_constraint=p["general_constraint"], options=dto_amd.Options(general_rows="border"), name="acrobot24g")
    assert s.general_rows_path == "border" and s._solve_nlp.num_constraint == (T - 1) * 64 + 1
    keep = np.zeros(s._solve_nlp.num_constraint, dtype=np.int32)
    keep[[1, 24, 64 + 30, (T - 2) * 64 + 63]] = 1
    return s, 64, 1, keep


def _padded(rng, shape, pad):
    """a random device tensor [..., n] that is a view of [..., n + pad] with NaN behind every row"""
    import torch
    full = torch.full(shape[:-1] + (shape[-1] + pad,), float("nan"), device="cuda", dtype=torch.float64)
    full[..., :shape[-1]] = torch.tensor(rng.standard_normal(shape), device="cuda")
    return full, full[..., :shape[-1]]


@pytest.mark.parametrize("T", [5, 16])
@pytest.mark.parametrize("kind", ["pendulum", "acrobot64", "acrobot24g"])
def test_shift_equals_the_index_map(kind, T):
    import torch
    from dto_amd import Point, capi
    from test_wide_mpc_gpu import _shift_ref
    s, nx, nu, keep = _solver(kind, T)
    n = s._solve_nlp
    nz, nc = n.num_variables, n.num_constraint
    assert nz == (T - 1) * (nx + nu) + nx and nc >= (T - 1) * nx
    if keep is not None:
        capi.check(n._lib.dto_solver_shift_keep_rows(n._h, keep.ctypes.data_as(capi.c_int32_p), nc))
    keep_cols = None if keep is None else np.flatnonzero(keep)
    hist = kind == "acrobot64"
    rng = np.random.default_rng(7)
    for knots in (1, 2, T - 2):
        fulls, pt = {}, Point()
        for k, cols, pad in (("x", nz, 3), ("mu", nc, 5), ("zl", nz, 0), ("zu", nz, 1), ("slack", nc, 2)):
            fulls[k], v = _padded(rng, (B, cols), pad)
            setattr(pt, k, v)
        pt.barrier = torch.tensor(rng.random(B), device="cuda")
        if hist:
            for k in ("qn_s", "qn_y"):
                fulls[k], v = _padded(rng, (B, 6, nz), 7)
                setattr(pt, k, v)
            pt.qn_npairs = np.array([6, 3, 0], dtype=np.int32)
            pt.qn_sigma = np.array([1.0, 2.5, 0.5])
        before = {k: v.cpu().numpy().copy() for k, v in fulls.items()}
        bar = pt.barrier.cpu().numpy().copy()
        s.shift_point(pt, knots)
        torch.cuda.synchronize()
        after = {k: v.cpu().numpy() for k, v in fulls.items()}
        for k in ("x", "zl", "zu"):
            want = before[k].copy()
            want[:, :nz] = _shift_ref(before[k][:, :nz], knots, nx + nu, T - 1, nx)
            assert np.array_equal(after[k], want, equal_nan=True), (kind, T, knots, k)
        want = before["mu"].copy()
        want[:, :(T - 1) * nx] = _shift_ref(before["mu"][:, :(T - 1) * nx], knots, nx, T - 1, 0, keep=keep_cols)
        assert np.array_equal(after["mu"], want, equal_nan=True), (kind, T, knots, "mu")
        assert np.array_equal(after["mu"][:, (T - 1) * nx:], before["mu"][:, (T - 1) * nx:], equal_nan=True)   # stage and general rows
        assert np.array_equal(after["slack"], before["slack"], equal_nan=True)
        assert np.array_equal(pt.barrier.cpu().numpy(), bar)
        if hist:
            for k in ("qn_s", "qn_y"):
                want = before[k].copy()
                for v in range(6):
                    want[:, v, :nz] = _shift_ref(before[k][:, v, :nz], knots, nx + nu, T - 1, nx)
                assert np.array_equal(after[k], want, equal_nan=True), (kind, T, knots, k)
            assert pt.qn_npairs.tolist() == [6, 3, 0] and pt.qn_sigma.tolist() == [1.0, 2.5, 0.5]
    if keep is not None:
        capi.check(n._lib.dto_solver_shift_keep_rows(n._h, None, 0))


def test_the_solver_marks_the_stage_rows_of_an_embedded_problem_and_the_refusals():
    import torch
    import dto_amd
    from dto_amd import Point, capi, problems as P
    from test_wide_mpc_gpu import _shift_ref
    T, n = 5, 24
    p = P.build_mpc_acrobot_padded(T=T, n=n)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True, parameters=p["parameters"],
                       name="acrobot24mpc")
    nz, nc = s._solve_nlp.num_variables, s._solve_nlp.num_constraint
    stage = np.sort(np.asarray(s._stage_rows))        # the pin rows, carried as dynamics rows of the first stage of the embedding
    assert len(stage) == n and stage[-1] < 64
    rng = np.random.default_rng(3)
    X, MU = rng.standard_normal((B, nz)), rng.standard_normal((B, nc))
    pt = Point(x=torch.tensor(X, device="cuda"), mu=torch.tensor(MU, device="cuda"))
    s.shift_point(pt, 1)
    torch.cuda.synchronize()
    assert np.array_equal(pt.x.cpu().numpy(), _shift_ref(X, 1, 65, T - 1, 64))
    assert np.array_equal(pt.mu.cpu().numpy(), _shift_ref(MU, 1, 64, T - 1, 0, keep=stage))
    # knots = 0 moves nothing; knots >= T - 1, a short leading dimension, one of zl / zu, a partial history, B < 1: DTO_ERR_INVALID
    x0 = pt.x.clone()
    s.shift_point(pt, 0)
    assert torch.equal(pt.x, x0)

    def refused(point, knots, code, B_=None):
        with pytest.raises(capi.DtoError) as e:
            s.shift_point(point, knots, B=B_)
        assert e.value.code == code, (e.value.code, str(e.value))
        torch.cuda.synchronize()
        assert torch.equal(pt.x, x0)
    refused(pt, T - 1, 1)
    refused(Point(x=(pt.x.data_ptr(), nz - 1)), 1, 1, B_=B)
    refused(Point(x=pt.x, mu=(pt.mu.data_ptr(), nc - 1)), 1, 1)
    refused(Point(x=pt.x, zl=torch.zeros_like(pt.x)), 1, 1)
    refused(Point(x=pt.x, qn_s=torch.zeros((B, 6, nz), device="cuda", dtype=torch.float64)), 1, 1)
    refused(pt, 1, 1, B_=0)
    # varying dimensions (the 6-knot problem of tests/test_layout.py): DTO_ERR_UNSUPPORTED
    from test_layout import varying_dimension_problem
    dyn, obj, cons, bounds = varying_dimension_problem("product")
    sv = dto_amd.Solver(dyn, obj, cons, bounds, evaluate_hessian=True, name="varydims")
    nzv = sv._solve_nlp.num_variables
    with pytest.raises(capi.DtoError) as e:
        sv.shift_point(Point(x=torch.zeros((B, nzv), device="cuda", dtype=torch.float64)), 1)
    assert e.value.code == 4, str(e.value)

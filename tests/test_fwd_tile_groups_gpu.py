"""The sequential forward sweep gives a wavefront a GROUP of adjacent tiles (csrc/dto_kkt_kernels.hpp: kkt_fwd_seq_body): the
first round of every tile with the lanes where they are, the inertia-correction rounds once for the group on its packed needing
lanes.  Every quantity of an attempt is per lane, so the solve must not change by a bit: each case runs the same iterations with
DTO_FWD_GROUP=1 (one tile per wavefront) and with groups, in one process and one build, and compares status, iteration and
factorisation counts, iterate, multipliers and step bit for bit."""
import os

import numpy as np
import pytest

from conftest import product_solver

pytestmark = pytest.mark.gpu

NAMES = ("z", "multipliers", "dz", "dmultipliers")


def _snapshot(s):
    out = {k: s.peek_batch(k) for k in NAMES}
    st = s.stats_batch()
    out.update(status=st["status"].copy(), iterations=st["iterations"].copy(), nfact=s.scalar_batch("nfact").copy())
    return out


def _assert_same(a, b, what):
    for k in ("status", "iterations", "nfact") + NAMES:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _stepwise(s, d, B, ld, group, n_iter, before=None, light=False, **begin_kw):
    """`n_iter` iterations, one iterate_batch(1) at a time, under DTO_FWD_GROUP=group: the snapshot after every iteration
    (light: the factorisation counts only)."""
    os.environ["DTO_FWD_GROUP"] = str(group)
    try:
        s.begin_batch(d.data_ptr(), B, ld, **begin_kw)
        assert s.partitions() == 1
        extra = before(s) if before else None
        snaps = []
        for _ in range(n_iter):
            s.iterate_batch(1)
            snaps.append(s.scalar_batch("nfact").copy() if light else _snapshot(s))
        return snaps, extra
    finally:
        del os.environ["DTO_FWD_GROUP"]


B_ACROBOT = 64 * 5 + 7                              # six tiles, the last one ragged
_ACROBOT21 = {}


def _acrobot21():
    """Acrobot T = 21, 327 of the bench's guesses (straight line + u ~ N(0, 1)).  At 21 stages an instance needs a second
    attempt in about one iteration of a hundred, so 327 guesses of any one seed never have more than a handful of retrying
    instances in the same iteration (24 seeds tried: 5 at most).  The batch is therefore CHOSEN from a seeded pool of 24 576 such
    guesses by what the pool does in 30 iterations at one tile per wavefront: first the instances that retry in the pool's
    busiest iteration, then those with the longest ladders, then the pool's first ones.  What an instance computes does not
    depend on its neighbours, so they do the same in the batch of the test -- which the test asserts, not assumes."""
    if not _ACROBOT21:
        import torch
        from bench import make_guesses
        s, p = product_solver("acrobot", 21)
        n_pool = 24576
        Z = make_guesses(s, p, n_pool, seed=3)
        d = torch.tensor(Z, device="cuda")
        s.set_partitions(1)
        try:
            snaps, _ = _stepwise(s, d, n_pool, Z.shape[1], 1, 30, light=True)
        finally:
            s.set_partitions(0)
        att = np.diff(np.stack([np.zeros(n_pool)] + snaps), axis=0)
        busiest = int(np.argmax(np.sum(att >= 2, axis=1)))
        first = list(np.flatnonzero(att[busiest] >= 2)[:160])
        deep = [i for i in np.argsort(-att.max(axis=0), kind="stable")[:32] if i not in first]
        rest = [i for i in range(n_pool) if i not in set(first) | set(deep)]
        order = (first + deep + rest)[:B_ACROBOT]
        print("pool: busiest iteration", busiest, "with", int(np.sum(att[busiest] >= 2)), "retrying instances; longest ladder", att.max())
        _ACROBOT21["case"] = (s, torch.tensor(Z[order], device="cuda"), Z.shape[1])
    return _ACROBOT21["case"]


def test_groups_of_two_four_and_eight_tiles_change_nothing():
    """Acrobot T = 21 (first and last stage: the out-of-line 13 x 13 end stages), 30 iterations.  Groups of 4: a partial last
    group; groups of 8: all tiles in one block, several passes per retry round."""
    s, d, ld = _acrobot21()
    s.set_partitions(1)
    try:
        ref, _ = _stepwise(s, d, B_ACROBOT, ld, 1, 30)
        # what the run exercises, from the attempts of every instance per iteration
        att = np.diff(np.stack([np.zeros(B_ACROBOT)] + [r["nfact"] for r in ref]), axis=0)
        assert att.max() >= 3, att.max()            # a ladder of at least two retries: more than one packed round
        packed = {k: max(int(np.sum(row[g0:g0 + 64 * k] >= 2)) for row in att for g0 in range(0, B_ACROBOT, 64 * k)) for k in (2, 4, 8)}
        print("attempts per iteration: max", att.max(), "largest count of retrying instances in a group:", packed)
        assert min(packed.values()) > 64, packed    # more needing lanes than a wavefront has: a second pass in the round
        for k in (2, 4, 8):
            got, _ = _stepwise(s, d, B_ACROBOT, ld, k, 30)
            for it, (a, b) in enumerate(zip(ref, got)):
                _assert_same(a, b, (k, it))
    finally:
        s.set_partitions(0)


@pytest.mark.parametrize("model,T", [("car", 51)])
def test_groups_with_variable_bounds_and_inequality_rows(model, T):
    """The BOUNDED instantiation of the stage loop: the arrays of row count Nz (bound multipliers) and Ni (slacks) per lane."""
    import torch
    import dto_amd
    s, p = product_solver(model, T)
    B = 64 * 2 + 9
    rng = np.random.Generator(np.random.PCG64(13))
    Z = np.zeros((B, s.nlp.num_variables))
    for b in range(B):
        xs, us = p["guess"](rng)
        dto_amd.initialize_states(s, xs)
        dto_amd.initialize_controls(s, us)
        Z[b] = s._z0
    d = torch.tensor(Z, device="cuda")
    s.set_partitions(1)
    try:
        ref, _ = _stepwise(s, d, B, Z.shape[1], 1, 25)
        got, _ = _stepwise(s, d, B, Z.shape[1], 2, 25)
    finally:
        s.set_partitions(0)
    assert ref[-1]["nfact"].sum() > ref[-1]["iterations"].sum()      # the inertia correction did retry
    assert s.footprint()["num_slacks"] > 0 and np.any(s.peek_batch("z_lower") != 0.0)
    for it, (a, b) in enumerate(zip(ref, got)):
        _assert_same(a, b, it)


def test_groups_with_per_instance_parameters():
    """Per-instance parameters live in SoA tiles of their own row count (Nw): the `wtile` path of the stage loop."""
    import torch
    import dto_amd
    from dto_amd import problems as P
    T, B = 30, 64 * 2 + 5
    rng = np.random.default_rng(5)
    p = P.build_mpc_pendulum(T=T)
    s = dto_amd.Solver(p["dynamics"], p["objective"], p["constraints"], p["bounds"], evaluate_hessian=True,
                       parameters=p["parameters"], name="mpc_pendulum")
    nz, nw = s.nlp.num_variables, s.nlp.num_parameters
    x1s = 0.3 * rng.standard_normal((B, 2))
    goals = np.pi * (0.5 + 0.5 * rng.random(B))
    W = np.stack([np.tile([x1s[b, 0], x1s[b, 1], goals[b]], T) for b in range(B)])
    Z = np.zeros((B, nz))
    for b in range(B):
        dto_amd.initialize_states(s, dto_amd.linear_interpolation(x1s[b], np.array([goals[b], 0.0]), T))
        dto_amd.initialize_controls(s, [rng.standard_normal(1) for _ in range(T - 1)])
        Z[b] = s._z0
    d, w = torch.tensor(Z, device="cuda"), torch.tensor(W, device="cuda")
    s.set_partitions(1)
    try:
        ref, _ = _stepwise(s, d, B, nz, 1, 20, params_ptr=w.data_ptr(), ldp=nw)
        got, _ = _stepwise(s, d, B, nz, 2, 20, params_ptr=w.data_ptr(), ldp=nw)
    finally:
        s.set_partitions(0)
    assert ref[-1]["nfact"].sum() > ref[-1]["iterations"].sum()      # the inertia correction did retry
    assert len(np.unique(ref[-1]["z"][:, :2], axis=0)) == B          # every instance starts where ITS parameters pin it
    for it, (a, b) in enumerate(zip(ref, got)):
        _assert_same(a, b, it)


def test_groups_after_a_repack():
    """The acrobot batch again: iterate until instances have finished, repack (the running ones move to the leading tiles, the
    launch covers fewer tiles), ten more iterations in groups of two."""
    s, d, ld = _acrobot21()

    def until_some_finished(s_):
        for n in range(60):
            s_.iterate_batch(5)
            running = int(np.sum(s_.scalar_batch("status") == 0))
            if running <= B_ACROBOT - 64:
                break
        left = s_.repack_batch()
        print("repack after", 5 * (n + 1), "iterations:", running, "running,", left, "after the repack")
        return n, running, left

    s.set_partitions(1)
    try:
        ref, how_ref = _stepwise(s, d, B_ACROBOT, ld, 1, 10, before=until_some_finished)
        got, how_got = _stepwise(s, d, B_ACROBOT, ld, 2, 10, before=until_some_finished)
    finally:
        s.set_partitions(0)
    assert how_ref == how_got, (how_ref, how_got)
    assert 64 < how_ref[2] <= B_ACROBOT - 64, how_ref                # at least a tile less, and still more than one tile
    assert ref[-1]["nfact"].sum() > ref[0]["nfact"].sum()            # ... that still iterate
    for it, (a, b) in enumerate(zip(ref, got)):
        _assert_same(a, b, it)


def test_groups_next_to_the_early_back_substitutions():
    """More than 1 024 tiles: dto_solver_iterate runs the back substitutions of finished tiles on a second stream next to the
    forward launch (tests/test_sequential_sweeps_gpu.py).  With groups the gate counts forward BLOCKS and a block publishes the
    tags of all its tiles: groups of four with and without the second stream, and one tile per wavefront, agree bit for bit."""
    import torch
    from bench import make_guesses
    s, p = product_solver("acrobot", 21)
    tiles = 1024 + 40
    B = tiles * 64 - 17
    Zs = make_guesses(s, p, 192, seed=4)
    Z = np.tile(Zs, (B // 192 + 1, 1))[:B]
    d = torch.tensor(Z, device="cuda")
    res = {}
    for group, overlap in ((4, "0"), (4, "1"), (1, "1")):
        os.environ["DTO_FWD_GROUP"] = str(group)
        os.environ["DTO_OVERLAP_SWEEPS"] = overlap
        try:
            s.begin_batch(d.data_ptr(), B, Z.shape[1])
            assert s.partitions() == 1
            for n in (4, 3):
                s.iterate_batch(n)
            res[group, overlap] = _snapshot(s)
        finally:
            del os.environ["DTO_FWD_GROUP"]
            del os.environ["DTO_OVERLAP_SWEEPS"]
    s.release_state()
    assert res[4, "0"]["nfact"].sum() > 7 * B
    _assert_same(res[4, "0"], res[4, "1"], "second stream")
    _assert_same(res[1, "1"], res[4, "1"], "groups of four")

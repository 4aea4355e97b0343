"""Hand-overs of held batches (gpu_batch.hip, sub_batch_load / run_ipm / HeldDynamics::adopt; ipm_kernels.hpp, k_compact_held /
k_level_held).

Slim gather: where the loop that hands its survivors over knows that every tile holds its dynamics, the gather of BAt reads the
stage slots N-1 and N of an instance and writes every slot of the sub-batch (k < N from N-1, N from N); under a current positive
Hessian verdict the gather of RSQ does the same.  The verdicts say the patterns are equal, so every output must be BIT FOR BIT what
the full copy gives; scalars `slim_dyn_copies` / `slim_hess_copies` count the hand-overs of the last solve that took the slim path.

Dense held level: options `compact_held 1`, `compact_held_min` -- a level of an all-held root compacts its survivors once half of
it has converged, and that level stays on the held entries (`level_held_launches` counts them; they are part of `fact_held_launches`
/ `rhs_held_launches` too).  The tail rule measures the survivors against the ROOT's batch at every level, so the tail takes the
same instances at the same iteration whether a level was made or not.

Recipe of tests/hold_common.py: nx = 8, nu = 3, batch 130 (two full tiles and a tile of 2 lanes), ACADOS_AMD_WPI=0, outputs x u pi
lam t iter status under numpy.array_equal, both tiers.  Survivor counts behind the factor sweep of iteration 0, 1, ... (host
simulation, tol_stat 1e-8, nothing handed over):
    SEED 47, N = 3   130 130 130 130 129 99 43 17 5 0     level at 43 (2 * 43 <= 130), tail at 17 (4 * 17 <= 130)
    SEED 47, N = 2   130 130 130 130 126 93 33 8 2 0      level at 33, tail at 8
    SEED 47, N = 1   130 130 130 128 109 54 21 6 1 0      level at 54, tail at 21
    SEED 5,  N = 3   130 130 130 130 129 100 53 21 4 0    level at 53: the first solve of the re-used level, SEED 47 (43) the second
A level of 130 instances is made for 96 slots (two tiles); both levels of the re-used case lie in its first tile, so the slots
43 .. 52 of the first solve share a tile with the 43 live lanes of the second.

Mutations (host simulation, not committed; profiles/NOTES.md): the gather taking slot N for k < N, or slot N-1 for stage N, fails
test_constant_data_takes_the_slim_gather at every horizon; the version check of the Hessian verdict dropped fails
test_setter_of_q_between_solves[...-with_a].  The status clear of k_level_held dropped fails no case, the re-used level included:
every way out of a level's loop leaves final statuses in the slots it was loaded with, so no stale RUNNING is reachable today."""
import numpy as np
import pytest

import hold_common
from hold_common import B, MID, TIERS, assert_same, clib, outputs  # noqa: F401

SEED, SEED_FIRST = 47, 5
LEVELS = {"compact_held": 1, "compact_held_min": 4}
ALONE = {"tail_max": 0}
SCALARS = ("tail_switches", "compactions", "slim_dyn_copies", "slim_hess_copies", "level_held_launches", "fact_held_launches",
           "rhs_held_launches", "hess_held_launches")


def base_data(N, seed=SEED):
    return hold_common.base_data(N, seed=seed)


def make_batch(clib, N, hold, opts=None, data=None):
    return hold_common.make_batch(clib, data if data is not None else base_data(N), N, None, dict(opts or {}, hold_dynamics=hold))


def counts(gb):
    return {f: int(gb.scalar(f)) for f in SCALARS}


def solve(clib, N, hold, opts=None, data=None, prepare=None):
    gb = make_batch(clib, N, hold, opts, data)
    if prepare is not None:
        prepare(gb)
    gb.solve()
    assert gb.kernel_name.startswith("1tpi-box<NX=8,NU=3"), gb.kernel_name
    return gb, outputs(gb, N), counts(gb)


_PLAIN = {}


def plain(clib, N):
    """the solve with holding off and the default hand-over (one tail switch): the reference of most cases, computed once per library"""
    if (id(clib), N) not in _PLAIN:
        _, out, c = solve(clib, N, 0)
        assert c["tail_switches"] == 1 and c["compactions"] == 0 and c["slim_dyn_copies"] == 0 and c["slim_hess_copies"] == 0, c
        assert c["level_held_launches"] == 0 and c["fact_held_launches"] == 0, c
        assert np.all(out["status"] == 0)
        _PLAIN[id(clib), N] = out
    return _PLAIN[id(clib), N]


def _one_ulp(N, field, idx):
    d = base_data(N)[field].copy()
    d[(MID,) + idx] = np.nextafter(d[(MID,) + idx], np.inf)
    return d


@pytest.mark.parametrize("N", [3, 2, 1])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_constant_data_takes_the_slim_gather(clib, N):
    """case 1: constant dynamics and Hessian, default tail: one tail switch, both arrays through the slim gather (at N = 1 the slot
    N-1 is slot 0 and nothing is duplicated), outputs those of hold_dynamics 0"""
    _, out, c = solve(clib, N, 1)
    print(N, c)
    assert c["tail_switches"] == 1 and c["slim_dyn_copies"] == 1 and c["slim_hess_copies"] == 1, c
    assert_same(out, plain(clib, N))
    # hold_hessian 0: no verdict is taken, and none is asked for the copy's sake
    _, out0, c0 = solve(clib, N, 1, {"hold_hessian": 0})
    assert c0["tail_switches"] == 1 and c0["slim_dyn_copies"] == 1 and c0["slim_hess_copies"] == 0 and c0["hess_held_launches"] == 0, c0
    assert_same(out0, out)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_hessian_that_differs_is_copied_in_full(clib):
    """case 2: Q of one instance differs by one ulp at stage 1 (k < N), the dynamics are constant"""
    N = 3
    q = _one_ulp(N, "Q", (5, 2))
    on = solve(clib, N, 1, prepare=lambda gb: gb.set("Q", 1, q))
    off = solve(clib, N, 0, prepare=lambda gb: gb.set("Q", 1, q))
    print(on[2])
    assert on[2]["tail_switches"] == 1 and on[2]["slim_dyn_copies"] == 1 and on[2]["slim_hess_copies"] == 0, on[2]
    assert off[2]["slim_dyn_copies"] == 0 and off[2]["slim_hess_copies"] == 0
    assert_same(on[1], off[1])


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_one_ulp_in_the_dynamics_keeps_the_full_copy(clib):
    """case 3: one ulp in one entry of A of instance MID at stage 1: a tile that must fetch, no slim copy of either array (no held
    factor launch, so no Hessian verdict either)"""
    N = 3
    a = _one_ulp(N, "A", (1, 2))
    on = solve(clib, N, 1, prepare=lambda gb: gb.set("A", 1, a))
    off = solve(clib, N, 0, prepare=lambda gb: gb.set("A", 1, a))
    assert on[2]["tail_switches"] == 1 and on[2]["slim_dyn_copies"] == 0 and on[2]["slim_hess_copies"] == 0, on[2]
    assert on[2]["fact_held_launches"] == 0
    assert_same(on[1], off[1])


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_setter_of_a_between_solves(clib):
    """case 4: set("A", 1, ...) between two solves of one object: the second hand-over copies BAt in full, and the solve leaves
    what a fresh batch with that data leaves"""
    N = 3
    a = base_data(N)["A"].copy()
    a[MID] = a[MID] * 1.01
    gb = make_batch(clib, N, 1)
    gb.solve()
    c1 = counts(gb)
    assert c1["slim_dyn_copies"] == 1 and c1["slim_hess_copies"] == 1, c1
    assert_same(outputs(gb, N), plain(clib, N))
    gb.set("A", 1, a)
    gb.solve()
    c2, second = counts(gb), outputs(gb, N)
    print(c1, c2)
    assert c2["tail_switches"] == 1 and c2["slim_dyn_copies"] == 0, c2
    _, fresh, _ = solve(clib, N, 0, prepare=lambda g: g.set("A", 1, a))
    assert_same(second, fresh)
    assert not np.array_equal(second["x", 2], plain(clib, N)["x", 2])   # (the new A was solved)


@pytest.mark.parametrize("with_a", [False, True], ids=["q_alone", "with_a"])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_setter_of_q_between_solves(clib, with_a):
    """case 5: the same with set("Q", 1, ...), Q of one instance changed: RSQ is copied in full.  q_alone: the dynamics keep their
    count, the second solve asks the detector again in front of its first held launch and the verdict in hand is negative.
    with_a: A of one instance is changed too, so no launch of the second solve is a held one, nobody asks the detector and the
    verdict in hand is the positive one of the FIRST solve, taken on older data: only its version says so"""
    N = 3
    q = base_data(N)["Q"].copy()
    q[MID] = q[MID] * 1.25
    a = _one_ulp(N, "A", (1, 2))

    def change(g):
        g.set("Q", 1, q)
        if with_a:
            g.set("A", 1, a)

    gb = make_batch(clib, N, 1)
    gb.solve()
    c1 = counts(gb)
    assert c1["slim_dyn_copies"] == 1 and c1["slim_hess_copies"] == 1, c1
    change(gb)
    gb.solve()
    c2, second = counts(gb), outputs(gb, N)
    print(c1, c2)
    assert c2["tail_switches"] == 1 and c2["slim_hess_copies"] == 0 and c2["slim_dyn_copies"] == (0 if with_a else 1), c2
    _, fresh, _ = solve(clib, N, 0, prepare=change)
    assert_same(second, fresh)
    assert not np.array_equal(second["x", 2], plain(clib, N)["x", 2])


@pytest.mark.parametrize("N", [3, 1])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_dense_level_stays_on_the_held_entries(clib, N):
    """case 6: compact_held with no tail: the survivors go from level to level, every level on the held entries"""
    _, out, c = solve(clib, N, 1, dict(LEVELS, **ALONE))
    print(N, c)
    assert c["compactions"] >= 1 and c["level_held_launches"] > 0 and c["tail_switches"] == 0, c
    assert c["slim_dyn_copies"] == c["compactions"] and c["slim_hess_copies"] == c["compactions"], c
    assert c["level_held_launches"] < c["fact_held_launches"] + c["rhs_held_launches"], c
    assert c["hess_held_launches"] == c["fact_held_launches"], c
    _, off, c0 = solve(clib, N, 0, dict(ALONE, compact_held=0))
    assert c0["compactions"] == 0 and c0["level_held_launches"] == 0, c0
    assert np.all(out["status"] == 0)
    assert_same(out, off)
    # holding off: compact_held makes no level
    _, off1, c1 = solve(clib, N, 0, dict(LEVELS, **ALONE))
    assert c1["compactions"] == 0 and c1["level_held_launches"] == 0, c1
    assert_same(off1, off)


@pytest.mark.parametrize("N", [3, 1])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_tail_below_a_dense_level(clib, N):
    """case 7: compact_held with the default tail: one level, whose tail takes the instances the root's tail would have taken, at
    the same iteration; both hand-overs are slim"""
    _, out, c = solve(clib, N, 1, LEVELS)
    print(N, c)
    assert c["compactions"] >= 1 and c["level_held_launches"] > 0 and c["tail_switches"] == 1, c
    assert c["slim_dyn_copies"] == c["compactions"] + 1 and c["slim_hess_copies"] == c["compactions"] + 1, c
    _, flat, cf = solve(clib, N, 1, {"compact_held": 0})
    assert cf["compactions"] == 0 and cf["tail_switches"] == 1 and cf["level_held_launches"] == 0, cf
    assert np.array_equal(out["iter"], flat["iter"])
    assert_same(out, flat)
    assert_same(out, plain(clib, N))


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_reused_level_with_fewer_survivors(clib):
    """case 8: two solves on one object, 53 survivors in the level of the first and 43 in that of the second (new data through the
    bulk setter): the slots 43 .. 52 of the level's first tile keep what the first solve left, and the held factor entry keeps the
    lanes behind the level's count alive to its epilogue.  Statuses all 0; outputs and iteration counts those of a fresh batch"""
    N = 3
    opts = dict(LEVELS, **ALONE)
    fresh, want, cw = solve(clib, N, 1, opts)
    gb = make_batch(clib, N, 1, opts, base_data(N, SEED_FIRST))
    gb.solve()
    c1 = counts(gb)
    assert np.all(gb.info("status") == 0) and c1["compactions"] >= 1 and c1["level_held_launches"] > 0, c1
    gb.set_bulk(fresh.get_bulk_in())
    gb.solve()
    c2, second = counts(gb), outputs(gb, N)
    print(c1, c2, cw)
    assert np.all(second["status"] == 0)
    assert c2["compactions"] == cw["compactions"] and c2["level_held_launches"] == cw["level_held_launches"], (c2, cw)
    assert np.array_equal(second["iter"], want["iter"])
    assert_same(second, want)
    _, off, _ = solve(clib, N, 0, dict(ALONE, compact_held=0))
    assert_same(second, off)

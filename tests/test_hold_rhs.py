"""The held entry of the rhs-only backward sweep (ipm_kernels_box.hpp, kh_backrhs): where EVERY 64-instance tile of the root batch
was found with the same [B A]' at every stage, both rhs-only launches of an iteration go to an entry that keeps the block in
registers -- fetched at the zero slot N and at stage N-1, reused by the stages N-2 .. 0 -- instead of kb_backrhs, which fetches it at
every stage.  The registers hold the very values the loads would have returned, so every output must be BIT FOR BIT what option
hold_dynamics = 0 gives.  The outputs cannot tell which entry ran: scalar `rhs_held_launches` counts the launches of the held one.

Recipe of tests/test_hold_dynamics.py: nx = 8, nu = 3, batch 130 (two full tiles and a tile of 2 lanes), family forced with
ACADOS_AMD_WPI=0, seeded random_lqr_batch, outputs x u pi lam t iter status under numpy.array_equal; both tiers: `hostsim` (kernel
sources under g++, one lane at a time) and `gpu` (the product library).  Horizons: N = 3 (the zero slot, the fetch at N-1, one stage
that reuses the block, stage 0), N = 2 (exactly one stage reuses) and N = 1 (none does): the shapes at which a wrong "fetch at"
condition shows."""
import os

import numpy as np
import pytest

import hold_common
from hold_common import LIB, MID, TIERS, TILES, assert_no_scratch, assert_same, built_kernel_facts, clib, outputs  # noqa: F401


def base_data(N):
    return hold_common.base_data(N, seed=41)


def make_batch(clib, N, a_stage=None, opts=None):
    return hold_common.make_batch(clib, base_data(N), N, a_stage, opts)


def solved(clib, N, hold, a_stage=None, opts=None, key=None):
    return hold_common.solved(clib, base_data(N), N, hold, a_stage, opts, key)


def held(gb):
    return int(gb.scalar("rhs_held_launches"))


@pytest.mark.parametrize("N", [3, 1, 2])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_constant_dynamics_run_the_held_entry(clib, N):
    """N = 3: slot N, the fetch at N-1, one interior stage that reuses the block and stage 0; N = 2: exactly one stage reuses; N = 1:
    none does"""
    on, out_on = solved(clib, N, 1, key="equal")
    off, out_off = solved(clib, N, 0, key="equal")
    assert int(on.scalar("tiles_invariant")) == TILES
    assert held(on) > 0
    assert held(off) == 0
    assert np.all(out_on["status"] == 0)
    assert_same(out_on, out_off)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_one_tile_that_must_fetch_keeps_the_fetching_entry(clib):
    """one entry of A of one instance of the middle tile moved by one ulp at stage 1: the entry reads no flag, so the whole launch
    fetches"""
    N = 3
    a = base_data(N)["A"].copy()
    a[MID, 1, 2] = np.nextafter(a[MID, 1, 2], np.inf)
    assert np.sum(a != base_data(N)["A"]) == 1
    on, out_on = solved(clib, N, 1, {1: a})
    off, out_off = solved(clib, N, 0, {1: a})
    assert int(on.scalar("tiles_invariant")) == TILES - 1
    assert held(on) == 0 and held(off) == 0
    assert_same(out_on, out_off)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_counter_and_choice_do_not_outlive_the_data(clib):
    N = 3
    gb = make_batch(clib, N)
    gb.solve()
    assert int(gb.scalar("tiles_invariant")) == TILES and held(gb) > 0
    a = base_data(N)["A"].copy()
    a[MID] = a[MID] * 0.75
    gb.set("A", 2, a)
    gb.solve()
    assert int(gb.scalar("tiles_invariant")) == TILES - 1
    assert held(gb) == 0
    assert_same(outputs(gb, N), solved(clib, N, 1, {2: a})[1])
    assert_same(outputs(gb, N), solved(clib, N, 0, {2: a})[1])


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_several_iterations_with_redo_launches_and_hand_overs(clib):
    """every iteration of the root level behind the one that detects launches the held entry twice (redo = 0 and redo = 1, option
    cond_pred_corr is on by default): four launches are two such iterations"""
    N = 3
    on, out_on = solved(clib, N, 1, key="equal")
    off, out_off = solved(clib, N, 0, key="equal")
    assert out_on["iter"].max() >= 3
    assert held(on) >= 4 and held(on) % 2 == 0
    assert int(on.scalar("tail_switches")) == 1 and int(off.scalar("tail_switches")) == 1
    assert_same(out_on, out_off)
    # the sub-level of a compaction has no flags: it fetches
    opts = {"compact_min": 4, "tail_max": 0}
    con, out_con = solved(clib, N, 1, opts=opts)
    coff, out_coff = solved(clib, N, 0, opts=opts)
    assert int(con.scalar("compactions")) >= 1 and int(coff.scalar("compactions")) >= 1
    assert int(con.scalar("tiles_invariant")) == TILES and held(coff) == 0
    assert_same(out_con, out_coff)


@pytest.mark.parametrize("where", ["stage_1", "every_stage"])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_nan_stays_with_its_instance(clib, where):
    """stage_1: the detector's NaN case -- the pattern differs from stage 0, the tile fetches, and with it the launch.  every_stage:
    the same NaN pattern at every stage is stage-invariant like any other pattern, the held entry carries the lane"""
    N = 3
    a = base_data(N)["A"].copy()
    a[MID, 1, 2] = np.nan
    clean = solved(clib, N, 1, key="equal")[1]
    stages = {1: a} if where == "stage_1" else {k: a for k in range(N)}
    for hold in (1, 0):
        gb, out = solved(clib, N, hold, stages)
        bad = np.flatnonzero(out["status"] != 0)
        assert bad.tolist() == [MID] and out["status"][MID] == 1, bad
        assert_same(out, clean, skip=(MID,))
        if hold:
            assert int(gb.scalar("tiles_invariant")) == (TILES - 1 if where == "stage_1" else TILES)
            assert (held(gb) == 0) if where == "stage_1" else (held(gb) > 0)
        else:
            assert held(gb) == 0


HELD = "kh_backrhs<8, 3>"


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
def test_held_entry_is_built_without_scratch():
    """the held entry of C2's shape is in the built library and stays in registers: no private segment, no spilled register -- read
    off its kernel descriptor"""
    facts = built_kernel_facts(HELD, instructions=False)
    assert facts is not None, HELD
    assert_no_scratch(facts[0])

"""The held entry of the factor sweep (ipm_kernels_box.hpp, kh_factor): where EVERY 64-instance tile of the root batch was found with the
same [B A]' at every stage, the factor launches of the root loop behind the one that detects go to an entry that fetches the block at
the zero slot N and at stage N-1 only -- A' parked in LDS, B' in LDS / registers -- and sums W W' column by column without ever storing
W.  Only the loop nest differs from kb_factor, every scalar keeps its chain of operations: every output must be BIT FOR BIT what option
hold_dynamics = 0 gives.  The outputs cannot tell which entry ran: scalar `fact_held_launches` counts the launches of the held one.

Recipe of tests/test_hold_rhs.py: nx = 8, nu = 3, batch 130 (two full tiles and a tile of 2 lanes), family forced with
ACADOS_AMD_WPI=0, seeded random_lqr_batch, outputs x u pi lam t iter status under numpy.array_equal; both tiers: `hostsim` (kernel
sources under g++, one lane at a time) and `gpu` (the product library).  Horizons: N = 3 (the zero slot, the fetch at N-1, one stage
that reuses the block, stage 0), N = 2 (exactly one stage reuses) and N = 1 (none does): the shapes at which a wrong "fetch at"
condition or a stale LDS block shows.

Launch counts.  A root loop that hands nothing over (tail_max = 0, no compaction) launches the factor sweep once per iteration and once
more for the exit test: max(iter) + 1 times.  The first of them runs in front of the detecting sweep, every later one is held:
fact_held_launches = max(iter).  With a hand-over the root loop ends early, behind its m-th factor launch: m - 1 of them are held, and
the rhs pairs of the iterations 2 .. m-1 are (two launches each, cond_pred_corr is on by default): fact_held = rhs_held / 2 + 1."""
import os

import numpy as np
import pytest

import hold_common
from hold_common import B, LIB, MID, TIERS, TILES, assert_no_scratch, assert_same, built_kernel_facts, clib, outputs  # noqa: F401

ALONE = {"tail_max": 0}  # the root loop runs to the end by itself


def base_data(N):
    return hold_common.base_data(N, seed=43)


def make_batch(clib, N, a_stage=None, opts=None):
    return hold_common.make_batch(clib, base_data(N), N, a_stage, opts)


def solved(clib, N, hold, a_stage=None, opts=None, key=None):
    return hold_common.solved(clib, base_data(N), N, hold, a_stage, opts, key)


def fheld(gb):
    return int(gb.scalar("fact_held_launches"))


def rheld(gb):
    return int(gb.scalar("rhs_held_launches"))


@pytest.mark.parametrize("N", [3, 2, 1])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_constant_dynamics_run_the_held_entry(clib, N):
    """N = 3: slot N, the fetch at N-1, one interior stage that reuses the block and stage 0; N = 2: exactly one stage reuses; N = 1:
    none does.  Every factor launch of the root loop but the first is held"""
    on, out_on = solved(clib, N, 1, opts=ALONE, key="alone")
    off, out_off = solved(clib, N, 0, opts=ALONE, key="alone")
    assert int(on.scalar("tiles_invariant")) == TILES
    assert int(on.scalar("tail_switches")) == 0 and int(on.scalar("compactions")) == 0
    assert fheld(on) > 0
    assert fheld(on) == int(out_on["iter"].max())      # max(iter) + 1 factor launches, minus the one in front of the detector
    assert fheld(off) == 0
    assert np.all(out_on["status"] == 0)
    assert_same(out_on, out_off)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_one_tile_that_must_fetch_keeps_the_fetching_entry(clib):
    """one entry of A of one instance of the middle tile moved by one ulp at stage 1: the entry reads no flag, so every launch fetches"""
    N = 3
    a = base_data(N)["A"].copy()
    a[MID, 1, 2] = np.nextafter(a[MID, 1, 2], np.inf)
    assert np.sum(a != base_data(N)["A"]) == 1
    on, out_on = solved(clib, N, 1, {1: a})
    off, out_off = solved(clib, N, 0, {1: a})
    assert int(on.scalar("tiles_invariant")) == TILES - 1
    assert fheld(on) == 0 and fheld(off) == 0
    assert_same(out_on, out_off)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_setter_between_two_solves_of_one_object(clib):
    """constant, then one stage changed, then constant again: the choice follows the data of each solve, and the block parked by an
    earlier solve is never met again"""
    N = 3
    gb = make_batch(clib, N, opts=ALONE)
    gb.solve()
    first = outputs(gb, N)
    assert int(gb.scalar("tiles_invariant")) == TILES and fheld(gb) == int(first["iter"].max()) > 0
    assert_same(first, solved(clib, N, 0, opts=ALONE, key="alone")[1])
    a = base_data(N)["A"].copy()
    a[MID] = a[MID] * 0.75
    gb.set("A", 2, a)
    gb.solve()
    assert int(gb.scalar("tiles_invariant")) == TILES - 1
    assert fheld(gb) == 0
    assert_same(outputs(gb, N), solved(clib, N, 0, {2: a}, opts=ALONE)[1])
    gb.set("A", 2, base_data(N)["A"])
    gb.solve()
    third = outputs(gb, N)
    assert int(gb.scalar("tiles_invariant")) == TILES and fheld(gb) == int(third["iter"].max()) > 0
    assert_same(third, solved(clib, N, 0, opts=ALONE, key="alone")[1])


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_hand_overs_count_the_root_level_only(clib):
    """a tail hand-over (the defaults: the last survivors continue one wave per instance) and a compaction (compact_min lowered): the
    sub-level has no flags and fetches, its factor launches are not counted"""
    N = 3
    on, out_on = solved(clib, N, 1, key="tail")
    off, out_off = solved(clib, N, 0, key="tail")
    assert int(on.scalar("tail_switches")) == 1 and int(off.scalar("tail_switches")) == 1
    assert out_on["iter"].max() >= 3
    assert fheld(on) == rheld(on) // 2 + 1 and 0 < fheld(on) < out_on["iter"].max()
    assert fheld(off) == 0
    assert_same(out_on, out_off)
    opts = {"compact_min": 4, "tail_max": 0}
    con, out_con = solved(clib, N, 1, opts=opts)
    coff, out_coff = solved(clib, N, 0, opts=opts)
    assert int(con.scalar("compactions")) >= 1 and int(coff.scalar("compactions")) >= 1
    assert int(con.scalar("tiles_invariant")) == TILES
    assert fheld(con) == rheld(con) // 2 + 1 and 0 < fheld(con) < out_con["iter"].max()
    assert fheld(coff) == 0
    assert_same(out_con, out_coff)


@pytest.mark.parametrize("where", ["stage_1", "every_stage"])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_nan_stays_with_its_instance(clib, where):
    """stage_1: the detector's NaN case -- the pattern differs from stage 0, the tile fetches, and with it every launch.  every_stage:
    the same NaN pattern at every stage is stage-invariant like any other pattern, the held entry carries the lane.  Statuses and
    every output, NaN patterns included, are the twin's"""
    N = 3
    a = base_data(N)["A"].copy()
    a[MID, 1, 2] = np.nan
    clean = solved(clib, N, 1, opts=ALONE, key="alone")[1]
    stages = {1: a} if where == "stage_1" else {k: a for k in range(N)}
    on, out_on = solved(clib, N, 1, stages, opts=ALONE)
    off, out_off = solved(clib, N, 0, stages, opts=ALONE)
    assert_same(out_on, out_off)
    bad = np.flatnonzero(out_on["status"] != 0)
    assert bad.tolist() == [MID] and out_on["status"][MID] == 1, bad
    assert_same(out_on, clean, skip=(MID,))
    assert int(on.scalar("tiles_invariant")) == (TILES - 1 if where == "stage_1" else TILES)
    assert (fheld(on) == 0) if where == "stage_1" else (fheld(on) == int(out_on["iter"].max()) > 0)
    assert fheld(off) == 0


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_statistics_rows_of_a_held_solve(clib):
    """what the factor sweep's epilogue writes into the statistics table (mu, the four residual norms, the objective: columns 6-10
    and 12) for instances of the first tile"""
    N = 3
    on = solved(clib, N, 1, opts=ALONE, key="alone")[0]
    off = solved(clib, N, 0, opts=ALONE, key="alone")[0]
    assert fheld(on) > 0 and fheld(off) == 0
    cols = [6, 7, 8, 9, 10, 12]
    for inst in (0, 31, 63):
        s_on, s_off = on.stat(inst), off.stat(inst)
        assert s_on.shape == s_off.shape and s_on.shape[0] >= 3
        assert np.array_equal(s_on[:, cols], s_off[:, cols], equal_nan=True), inst


HELD = "kh_factor<8, 3>"


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
def test_held_entry_is_built_without_scratch():
    """the held entry of C2's shape is in the built library: no private segment, no spilled register, static LDS that lets four
    single-wave blocks share a CU's 160 KB, no scratch instruction in its code (read the way tests/test_box_sweep_isa.py does)"""
    facts = built_kernel_facts(HELD)
    assert facts is not None, HELD
    md, lds_bytes, ins = facts
    if ins is None:
        pytest.skip("llvm-objdump not found")
    assert ins, HELD
    assert_no_scratch(md)
    assert lds_bytes is not None and lds_bytes <= 40960, lds_bytes
    assert not any("scratch_" in t for t in ins)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_polish_pass_keeps_the_counts_of_the_solve(clib):
    """the polish pass is a root loop of its own (iteration counter 0 against iter_max 1): its first factor launch runs in front of its
    detecting sweep, its second and last one is held, and the rhs pair between them is the detecting iteration's and fetches.  So a
    polished solve reports the plain solve's `tiles_invariant` (the scalar speaks of the solve, the pass does not overwrite it), its
    `fact_held_launches` plus one and its `rhs_held_launches`.  polish_ratio 0 selects every instance: on the device a wave without a
    running lane leaves the detecting sweep before it counts (GQP_WAVE_ANY; the host simulation treats every wave as live), and the
    pass holds only if all three tiles count"""
    N = 3
    plain = solved(clib, N, 1, opts=ALONE, key="alone")[0]
    pol = solved(clib, N, 1, opts=dict(ALONE, polish=1, polish_ratio=0.0))[0]
    print("polished", pol.scalar("polished"), "tiles", pol.scalar("tiles_invariant"), "fact held", fheld(plain), fheld(pol), "rhs held", rheld(plain), rheld(pol))
    assert int(pol.scalar("polished")) == B                 # (every tile has running lanes in the loop of the pass)
    assert int(pol.scalar("tiles_invariant")) == TILES == 3
    assert fheld(pol) == fheld(plain) + 1
    assert rheld(pol) == rheld(plain) > 0

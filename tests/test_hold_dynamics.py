"""Held dynamics of the one-instance-per-lane box sweeps (ipm_kernels_box.hpp): a 64-instance tile whose [B A]' is the same bit
pattern at every stage k = 0 .. N-1 keeps that block in registers across the stages of the two forward sweeps (kb_forward) instead
of fetching it again at every stage; kb_backrhs and kb_factor fetch it as before.  The registers hold the very values the loads would have returned, so every output must be BIT
FOR BIT what option hold_dynamics = 0 (every tile fetches at every stage: the code path of before) gives.

Shape of every test: nx = 8, nu = 3, N = 3 (stage 0, one interior stage, stage N-1 and the zero slot), batch 130 (two full tiles
and a tile of 2 lanes), family forced with ACADOS_AMD_WPI=0.  Every test exists in both tiers: `hostsim` (kernel sources under
g++, CPU, one lane at a time) and `gpu` (the product library).

What these tests guard is the direction that can hurt: a block held where it must not be (one ulp, -0.0, a setter between two solves, a
NaN, a hand-over).  They cannot see whether a consumer holds at all -- `tiles_invariant` is summed on the host from the detector's
counters, and a kernel that fetched at every stage regardless would give the same outputs and the same scalar.  That the loads are gone
is a measurement: HBM bytes per launch in profiles/r08_v1_pmc_traffic.json against profiles/r08_parent_pmc_traffic.json."""
import os

import numpy as np
import pytest

import hold_common
from hold_common import B, LIB, MID, TIERS, assert_no_scratch, assert_same, built_kernel_facts, clib  # noqa: F401
from oracle.oracle import OracleQp, default_opts

N = 3
ZR, ZC = 3, 6            # entry of A that is +0.0 in every instance of the base batch


def base_data():
    return hold_common.base_data(N, seed=41, zero_entry=(ZR, ZC))


def make_batch(clib, a_stage=None, opts=None):
    return hold_common.make_batch(clib, base_data(), N, a_stage, opts)


def outputs(gb):
    return hold_common.outputs(gb, N)


def solved(clib, hold, a_stage=None, opts=None, key=None):
    return hold_common.solved(clib, base_data(), N, hold, a_stage, opts, key)


def altered(stage, r, c, value):
    """{stage: A of the whole batch} with entry (r, c) of instance MID replaced"""
    a = base_data()["A"].copy()
    a[MID, r, c] = value
    return {stage: a}


_ORACLE = {}


def oracle(i):
    if i not in _ORACLE:
        from acados_amd.generators import lqr_instance_qp
        o = OracleQp(lqr_instance_qp(base_data(), i, N))
        assert o.solve(default_opts(tol_stat=1e-8)) == 0
        _ORACLE[i] = o
    return _ORACLE[i]


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_all_stages_equal(clib):
    on, out_on = solved(clib, 1, key="equal")
    off, out_off = solved(clib, 0, key="equal")
    assert int(on.scalar("tiles_invariant")) == 3
    assert np.all(out_on["status"] == 0)
    assert_same(out_on, out_off)
    for i in (0, MID, B - 1):
        o = oracle(i)
        for k in range(N + 1):
            assert np.allclose(out_on["x", k][i], o.get(k, "x"), atol=1e-9), (i, k)
            if k < N:
                assert np.allclose(out_on["u", k][i], o.get(k, "u"), atol=1e-9), (i, k)
        assert out_on["iter"][i] == o.iter


VARIANTS = {
    "ulp_at_last_stage": lambda: altered(N - 1, 1, 2, np.nextafter(base_data()["A"][MID, 1, 2], np.inf)),
    "ulp_at_stage_1": lambda: altered(1, 1, 2, np.nextafter(base_data()["A"][MID, 1, 2], np.inf)),
    "minus_zero": lambda: altered(1, ZR, ZC, -0.0),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_one_instance_of_the_middle_tile_differs(clib, variant):
    """what a compare with a tolerance, a skipped last stage or a floating-point `==` get wrong"""
    a_stage = VARIANTS[variant]()
    (k, a), = a_stage.items()
    if variant == "minus_zero":
        assert a[MID, ZR, ZC] == 0.0 and np.signbit(a[MID, ZR, ZC]) and not np.signbit(base_data()["A"][MID, ZR, ZC])
    else:
        assert np.sum(a != base_data()["A"]) == 1
    on, out_on = solved(clib, 1, a_stage)
    off, out_off = solved(clib, 0, a_stage)
    assert int(on.scalar("tiles_invariant")) == 2
    assert_same(out_on, out_off)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_flags_do_not_outlive_the_data(clib):
    gb = make_batch(clib)
    gb.solve()
    assert int(gb.scalar("tiles_invariant")) == 3
    a = base_data()["A"].copy()
    a[MID] = a[MID] * 0.75
    gb.set("A", 2, a)
    gb.solve()
    assert int(gb.scalar("tiles_invariant")) == 2
    fresh, out_fresh = solved(clib, 1, {2: a})
    assert_same(outputs(gb), out_fresh)
    # ... and nothing is held outside a solve: the same again with holding off from the start
    assert_same(out_fresh, solved(clib, 0, {2: a})[1])


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_nan_stays_with_its_instance(clib):
    """DESIGN 1, instance isolation: the instance with the NaN ends with status 1, every other one bit for bit as without it"""
    a = base_data()["A"].copy()
    a[MID, 1, 2] = np.nan
    clean = solved(clib, 1, key="equal")[1]
    for hold in (1, 0):
        gb, out = solved(clib, hold, {1: a})
        bad = np.flatnonzero(out["status"] != 0)
        assert bad.tolist() == [MID] and out["status"][MID] == 1, bad
        assert_same(out, clean, skip=(MID,))
        if hold:
            assert int(gb.scalar("tiles_invariant")) == 2


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_hand_over_to_the_tail_with_held_dynamics(clib):
    on, out_on = solved(clib, 1, key="equal")
    off, out_off = solved(clib, 0, key="equal")
    assert int(on.scalar("tail_switches")) == 1 and int(off.scalar("tail_switches")) == 1
    assert int(on.scalar("tiles_invariant")) == 3
    assert_same(out_on, out_off)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_compaction_with_held_dynamics(clib):
    opts = {"compact_min": 4, "tail_max": 0}
    on, out_on = solved(clib, 1, opts=opts)
    off, out_off = solved(clib, 0, opts=opts)
    assert int(on.scalar("compactions")) >= 1 and int(off.scalar("compactions")) >= 1
    assert int(on.scalar("tiles_invariant")) == 3
    assert_same(out_on, out_off)


LIGHT = ("kb_forward<8, 3, false, false>", "kb_forward<8, 3, false, true>", "kb_backrhs<8, 3, false>")


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
def test_light_sweeps_hold_the_block_without_scratch():
    """the three light sweeps of C2 -- the two forward sweeps hold [B A]' (88 doubles more, live across the stage loop) -- stay in
    registers: no private segment, no spilled register -- read off the kernel descriptors of the built library (the same three kernels and fields as
    test_box_sweep_isa.py::test_c2_sweeps_stay_in_registers_and_fit_four_per_cu; kept here so that this file states the whole contract)"""
    for k in LIGHT:
        facts = built_kernel_facts(k, instructions=False)
        assert facts is not None, k
        assert_no_scratch(facts[0])

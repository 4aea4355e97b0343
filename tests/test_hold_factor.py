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
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
NX, NU, B = 8, 3, 130
TILES = (B + 63) // 64
MID = 64 + 17            # an instance of the middle tile
FIELDS = ("x", "u", "pi", "lam", "t")
ALONE = {"tail_max": 0}  # the root loop runs to the end by itself


@pytest.fixture
def clib(request, monkeypatch):
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")   # one instance per lane whatever the batch size
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


_BASE = {}


def base_data(N):
    """the batch with the same A, B at every stage (computed once per horizon, never changed: callers copy what they alter)"""
    if N not in _BASE:
        from acados_amd.generators import random_lqr_batch
        _BASE[N] = random_lqr_batch(N=N, nx=NX, nu=NU, batch=B, seed=43)
    return _BASE[N]


def make_batch(clib, N, a_stage=None, opts=None):
    """a_stage: {stage: A of the whole batch at that stage} on top of the base batch"""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims
    gb = OcpQpGpuBatch(lqr_dims(N, NX, NU), B, _clib=clib)
    fill_lqr_batch(gb, base_data(N), N)
    for k, a in (a_stage or {}).items():
        gb.set("A", k, a)
    gb.opts_set("tol_stat", 1e-8)
    for f, v in (opts or {}).items():
        gb.opts_set(f, v)
    return gb


def outputs(gb, N):
    out = {"iter": gb.info("iter").copy(), "status": gb.info("status").copy()}
    for k in range(N + 1):
        for f in FIELDS:
            if (f == "pi" or f == "u") and k == N:
                continue
            out[f, k] = np.array(gb.get(f, k), copy=True)
    return out


_SOLVED = {}


def solved(clib, N, hold, a_stage=None, opts=None, key=None):
    """(batch, outputs) of one solve; runs named by `key` are computed once per library and shared between the tests"""
    ck = (id(clib), N, hold, key)
    if key is not None and ck in _SOLVED:
        return _SOLVED[ck]
    gb = make_batch(clib, N, a_stage, dict(opts or {}, hold_dynamics=hold))
    gb.solve()
    assert gb.kernel_name.startswith("1tpi-box<NX=8,NU=3"), gb.kernel_name
    res = (gb, outputs(gb, N))
    if key is not None:
        _SOLVED[ck] = res
    return res


def assert_same(a, b, skip=()):
    assert a.keys() == b.keys()
    keep = np.array([i not in skip for i in range(B)])
    for key in a:
        assert np.array_equal(a[key][keep], b[key][keep], equal_nan=True), key


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


LIB = os.path.join(ROOT, "acados_amd", "csrc", "libacados_amd_qp.so")
HELD = "kh_factor<8, 3>"


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
def test_held_entry_is_built_without_scratch():
    """the held entry of C2's shape is in the built library: no private segment, no spilled register, static LDS that lets four
    single-wave blocks share a CU's 160 KB, no scratch instruction in its code (read the way tests/test_box_sweep_isa.py does)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    if not isa_lint.READELF or not isa_lint.OBJDUMP:
        pytest.skip("llvm-readelf / llvm-objdump not found")
    found = {}
    for co in isa_lint.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
            tmp = f.name
        try:
            meta = isa_lint.metadata(tmp)
            notes = subprocess.run([isa_lint.READELF, "--notes", tmp], capture_output=True, text=True).stdout
            dis = isa_lint.kernels(subprocess.run([isa_lint.OBJDUMP, "-d", tmp], capture_output=True, text=True).stdout)
        finally:
            os.unlink(tmp)
        # static LDS per kernel: .group_segment_fixed_size precedes .name / .symbol inside a kernel's metadata entry
        lds, cur = {}, None
        for ln in notes.splitlines():
            m = re.match(r"\s*-?\s*\.(group_segment_fixed_size|symbol):\s*(\S+)", ln)
            if m and m.group(1) == "group_segment_fixed_size":
                cur = int(m.group(2))
            elif m and cur is not None:
                lds[m.group(2).strip("'\"").replace(".kd", "")] = cur
                cur = None
        names = isa_lint.demangle(list(meta))
        for sym, md in meta.items():
            if "gqp::" + HELD + "(" in names[sym]:
                found[HELD] = (md, lds.get(sym), dis.get(sym, []))
    assert set(found) == {HELD}, sorted(found)
    md, lds_bytes, ins = found[HELD]
    assert ins, HELD
    assert int(md.get("private_segment_fixed_size", 0)) == 0, md
    assert int(md.get("vgpr_spill_count", 0)) == 0 and int(md.get("sgpr_spill_count", 0)) == 0, md
    assert lds_bytes is not None and lds_bytes <= 40960, lds_bytes
    assert not any("scratch_" in t for t in ins)

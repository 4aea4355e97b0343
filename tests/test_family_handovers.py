"""Tail and level hand-overs on every kernel family, on data where every stage and every instance differs; both tiers.

tests/test_family_stage_edges.py keeps each family alone (tail_max 0).  A default solve of a one-instance-per-lane batch ends through a
hand-over: the survivors are gathered into a sub-batch of another family (gpu_batch.hip: run_ipm -> compact_into -> sub_batch_create /
sub_batch_load, copy_level with k_compact_tile / k_compact_copy / k_compact_scalars, the amask copy), finished there with that
family's own finalize, and scattered back (compact_back / sub_batch_store, k_stat_merge).  A compaction level (compact_min) and the
dense live list of the sixteen-lanes families (k_active_perm) are the other two ways a loop changes which instance sits in which
slot.  The hand-over copies whole stage-indexed arrays by element count and trusts that parent and child agree on every stage
offset, padded dim, activity-word count and row order: on the generators' data (one block over the horizon) an error there moves
equal bits to equal bits, here it moves a wrong block to a wrong instance.

Data: the rows' generators, perturbed stage-wise (stagewise_common.make_batch), and ONE random structure with a shared slack, a masked
side, an equality-flagged x0 and general rows whose instances differ in q and r.  Batch composition is chosen with the oracle alone
(stagewise_common.HANDOVER_SEEDS) and asserted here on the oracle's iteration counts c before any sweep runs: an instance with count c
leaves the loop at the factor sweep of iteration c, so #{c > j} instances are alive when run_ipm applies its rules at iteration j.

Tail cases (HANDOVERS: one per lane row x tail family; N = 2, 9; B = 65, 130: three tiles, the last one partial):
  early    tail_div 1, tail_max B - 1: the first finished instance triggers the switch, the sorted list has holes
  late     tail_div 1, tail_max 1: exactly one survivor, placed at lane 0, 63, 64 and B - 1 by reordering the instances
  default  the library's tail_max 12288, tail_div 4, at B = 65
Asserted: solve() == 0; tail_switches == 1, compactions == 0; the parent's and the tail's kernel name (the tail reads the very
switches of family_switches() that the stand-alone rows of FAMILIES pin with their scalars: ACADOS_AMD_W16T_GEN=0 is the register-row
factor sweep there); the independent residual kernel <= 2e-8; EVERY instance against the oracle's solve of its own read-back QP (box
rows: x u pi lam at 1e-8, rows with general rows or slacks: x u pi lam sl su t at 1e-7); iteration counts and statuses equal to the
oracle's and to those of the same batch solved with tail_max 0; the instances that had finished before the switch agree with that
run bit for bit in the output blob.

Level cases (every row of FAMILIES but the single-launch row and ric0; compact_min 2, tail_max 0; N = 2, 9; the row's ragged batch and
the next size, HANDOVER_BATCHES): against the same batch with compact_min 1 << 30 -- compactions >= 1 against 0 and every output bit
equal (output blob, status iter res_stat res_eq res_ineq res_comp mu); per-instance arithmetic does not depend on the slot.  The
sixteen-lanes rows run with solve_max 0 (the whole solve in one launch never enters a level) and additionally with
ACADOS_AMD_W16_PERM = 0 and = 1, with and without the level: four runs, equal bits.  No family breaks bit identity.

Combined: compact_min 4 with the default tail on 1tpi-gen and 1tpi-pipe/xbox: the level, not the root, hands over.

Tail families as the parent commit reports them: the box rows land on w16-box<NX,NU> of the parent's padded dims (wpi-box with
ACADOS_AMD_W16=0), chain24 on w16r-gen<NX=24,NU=3,NG=4> (wpi-gen with ACADOS_AMD_W16G=0), the structure row on wpi-gen.

Grid.  gpu tier: everything.  hostsim tier: the late case at ONE lane position (64); the early case at N = 9 with B = 65 only; the
hand-overs marked slow (a second per instance and sweep in a simulated w16r-gen<24,3,4> tail) run N = 2 there and their early pattern
on the device only; the level cases of the sixteen-lanes rows (four runs each) run N = 2 there, the slow ones at B = 5 only; the
combined case runs N = 2 there.

Measured worst deviation from the oracle (printed per case), host simulation / MI355X: box rows 1.9e-14 / 2.0e-14, rows with general
rows and slacks 3.5e-9 / 7.0e-9."""
import numpy as np
import pytest

from conftest import compare_with_oracle
from stagewise_common import (FAMILIES, HANDOVER_BATCHES, HANDOVERS, KKT_TOL, LONG, ROWS, TIERS, check_family, make_batch, oracle_counts,
                              oracle_solve, structure_cases)

INFO = ("status", "iter", "res_stat", "res_eq", "res_ineq", "res_comp", "mu")
TAIL_DEFAULTS = (12288, 4)          # tail_max, tail_div of a fresh batch (gpu_batch.hip)


@pytest.fixture
def clib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


def _param(tier, *args):
    return pytest.param(tier.values[0], *args, id="-".join(str(a) for a in args) + "-" + tier.id, marks=tier.marks)


def _outputs(gb):
    out = {f: gb.info(f).copy() for f in INFO}
    out["blob"] = gb.get_bulk()
    return out


def _assert_same_bits(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key]), (what, key)


def _survivors(c, j):
    return int(np.sum(c > j))


def _switch(c, B, tail_max, tail_div):
    """(j, n): the first iteration j at which the tail rule of run_ipm holds for the n = #{c > j} survivors; None: it never does"""
    for j in range(int(c.max())):
        n = _survivors(c, j)
        if 1 <= n <= tail_max and tail_div * n <= B:
            return j, n
    return None


def _against_oracle(gb, blob, row, c, what):
    """every instance against the oracle's solve of its own read-back QP, iteration counts and statuses the oracle's"""
    N, B = gb.N, gb.n_batch
    nrm = gb.res_compute()
    assert np.all(np.isfinite(nrm)) and nrm.max() <= KKT_TOL, nrm.max()
    gen = ROWS[row].get("gen")
    fields = ("x", "u", "pi", "lam") + (("sl", "su", "t") if gen else ())
    sol = {(f, k): gb.get(f, k) for k in range(N + 1) for f in fields if not (f == "pi" and k == N)}
    it, st = gb.info("iter"), gb.info("status")
    assert np.all(st == 0), st
    assert np.array_equal(it, c), (it, c)
    worst = 0.0
    for i in range(B):
        qp, o = oracle_solve(gb, blob, i)
        worst = max(worst, compare_with_oracle(lambda k, f: sol[(f, k)][i], o, qp, 1e-7 if gen else 1e-8, fields=fields))
    print(f"{what}: iterations {sorted(set(it.tolist()))}, worst deviation from the oracle {worst:.2e}")
    return worst


# ---- tail cases -------------------------------------------------------------------------------------------------------------------
def _tail_grid():
    out = []
    for ho, h in HANDOVERS.items():
        for tier in TIERS:
            host = tier.id == "hostsim"
            for N in (2, LONG):
                if host and N == LONG and (h.get("slow") or ROWS[h["row"]].get("slow")):
                    continue
                for B in HANDOVER_BATCHES[64]:
                    if not (host and (h.get("slow") or (N == LONG and B > 65))):
                        out.append(_param(tier, ho, N, B, "early", -1))
                    for lane in ((64,) if host else (0, 63, 64, B - 1)):
                        out.append(_param(tier, ho, N, B, "late", lane))
                out.append(_param(tier, ho, N, HANDOVER_BATCHES[64][0], "default", -1))
    return out


@pytest.mark.parametrize("clib,ho,N,B,pattern,lane", _tail_grid(), indirect=["clib"])
def test_tail_handover(clib, monkeypatch, ho, N, B, pattern, lane):
    h = HANDOVERS[ho]
    row = h["row"]
    for k, v in h["env"].items():
        monkeypatch.setenv(k, v)
    ref = make_batch(clib, monkeypatch, row, N, B, handover=True)        # tail_max 0: the whole solve on the lane family
    blob = ref.get_bulk_in()
    c = oracle_counts(ref, blob)
    assert len(set(c.tolist())) >= 3, c
    if row == "1tpi-gen/struct":
        assert structure_cases(ref.to_qp(0)) == {"general", "shared", "one-sided", "x0"}
    if pattern == "late":
        slow = np.flatnonzero(c == c.max())
        assert slow.size == 1, slow                                      # the maximum is attained by exactly one instance ...
        order = np.arange(B)
        order[[lane, slow[0]]] = order[[slow[0], lane]]                  # ... which goes to `lane`
        blob, c = np.ascontiguousarray(blob[order]), c[order]
        ref.set_bulk(blob)
        assert np.array_equal(ref.get_bulk_in(), blob) and int(np.argmax(c)) == lane
    tail_max, tail_div = {"early": (B - 1, 1), "late": (1, 1), "default": TAIL_DEFAULTS}[pattern]
    sw = _switch(c, B, tail_max, tail_div)
    assert sw is not None, c
    j, n = sw
    if pattern == "early":
        assert j == c.min() and n == int(np.sum(c > c.min())) and n >= 2, (j, n)         # the first finished instance triggers it
    elif pattern == "late":
        assert n == 1
    else:
        assert 4 * n <= B
    done = c <= j                                                          # finished before the switch: nothing may touch them
    assert done.any() and not done.all()

    gb = make_batch(clib, monkeypatch, row, N, B, handover=True)
    gb.set_bulk(blob)
    gb.opts_set("tail_max", tail_max)
    gb.opts_set("tail_div", tail_div)
    assert gb.tail_kernel_name == ""                                      # no tail before the first hand-over
    bad = gb.solve()
    check_family(gb, row)
    assert bad == 0, (ho, gb.info("status"), gb.info("iter"))
    assert int(gb.scalar("tail_switches")) == 1 and int(gb.scalar("compactions")) == 0
    name = gb.tail_kernel_name
    assert name.startswith(h["tail"][0]) and all(s in name for s in h["tail"][1:]), (ho, name)
    _against_oracle(gb, blob, row, c, f"{ho} N={N} B={B} {pattern} lane {lane} ({n} of {B} handed to {name} at iteration {j})")

    assert ref.solve() == 0
    check_family(ref, row)
    assert int(ref.scalar("tail_switches")) == 0 and ref.tail_kernel_name == ""
    got, want = _outputs(gb), _outputs(ref)
    for f in ("iter", "status"):
        assert np.array_equal(got[f], want[f]), f
    for key in got:
        assert np.array_equal(got[key][done], want[key][done]), (ho, key, "an instance that had finished before the switch moved")


# ---- level cases ------------------------------------------------------------------------------------------------------------------
LEVEL_ROWS = [row for row in FAMILIES if row not in ("w16-box/kx_solve", "ric0")]


def _level_grid():
    out = []
    for row in LEVEL_ROWS:
        r = FAMILIES[row]
        for tier in TIERS:
            for N in (2, LONG):
                if tier.id == "hostsim" and N == LONG and r["unit"] == 4:
                    continue
                for B in HANDOVER_BATCHES[r["unit"]]:
                    if not (tier.id == "hostsim" and r.get("slow") and B > HANDOVER_BATCHES[4][0]):
                        out.append(_param(tier, row, N, B))
    return out


@pytest.mark.parametrize("clib,row,N,B", _level_grid(), indirect=["clib"])
def test_compaction_level_is_bit_identical(clib, monkeypatch, row, N, B):
    w16 = FAMILIES[row]["unit"] == 4
    runs = {}
    for perm in (("0", "1") if w16 else (None,)):
        if perm is not None:
            monkeypatch.setenv("ACADOS_AMD_W16_PERM", perm)
        for compact_min in (1 << 30, 2):
            gb = make_batch(clib, monkeypatch, row, N, B, handover=True)
            gb.opts_set("compact_min", compact_min)
            if w16:
                gb.opts_set("solve_max", 0)
            if not runs:
                c = oracle_counts(gb, gb.get_bulk_in())
                assert len(set(c.tolist())) >= 3, c
                assert any(1 <= _survivors(c, j) <= B // 2 for j in range(int(c.max()))), c
            bad = gb.solve()
            check_family(gb, row)
            assert bad == 0, (row, gb.info("status"), gb.info("iter"))
            assert int(gb.scalar("tail_switches")) == 0
            levels = int(gb.scalar("compactions"))
            assert levels >= 1 if compact_min == 2 else levels == 0, (row, perm, compact_min, levels)
            runs[(perm, compact_min)] = _outputs(gb)
    first = next(iter(runs))
    assert np.array_equal(runs[first]["iter"], c), (runs[first]["iter"], c)
    for key, out in runs.items():
        _assert_same_bits(runs[first], out, (row, key))
    print(f"{row} N={N} B={B}: iterations {sorted(set(c.tolist()))}, {len(runs)} runs bit-identical")


# ---- a tail below a level -----------------------------------------------------------------------------------------------------------
def _combined_grid():
    return [_param(tier, row, N) for row in ("1tpi-gen", "1tpi-pipe/xbox") for tier in TIERS for N in (2, LONG)
            if not (tier.id == "hostsim" and N == LONG)]


@pytest.mark.parametrize("clib,row,N", _combined_grid(), indirect=["clib"])
def test_tail_below_a_compaction_level_on_stagewise_data(clib, monkeypatch, row, N):
    """compact_min 4 with the default tail, B = 130: at most 65 survivors go on in a level, and that level, not the root, hands its
    last (at most 32) to the tail"""
    B = HANDOVER_BATCHES[64][1]
    gb = make_batch(clib, monkeypatch, row, N, B, handover=True)
    blob = gb.get_bulk_in()
    c = oracle_counts(gb, blob)
    level = next((j for j in range(int(c.max())) if 1 <= _survivors(c, j) <= B // 2), None)
    assert level is not None and 4 * _survivors(c, level) > B, c        # the level is entered before the tail rule holds
    assert _switch(c, B, *TAIL_DEFAULTS) is not None, c
    gb.opts_set("compact_min", 4)
    gb.opts_set("tail_max", TAIL_DEFAULTS[0])
    gb.opts_set("tail_div", TAIL_DEFAULTS[1])
    bad = gb.solve()
    check_family(gb, row)
    assert bad == 0, (row, gb.info("status"), gb.info("iter"))
    assert int(gb.scalar("compactions")) >= 1 and int(gb.scalar("tail_switches")) == 1
    assert gb.tail_kernel_name.startswith("w16r-gen<NX=24,NU=3,NG=4>" if row == "1tpi-gen" else "w16-box<NX=4,NU=1>"), gb.tail_kernel_name
    _against_oracle(gb, blob, row, c, f"{row} N={N} B={B} level + tail ({gb.tail_kernel_name})")

"""Held Hessian and verdicts kept across solves (gpu_batch.hip, HeldDynamics; ipm_kernels_box.hpp, kh_factor / k_hess_invariant).

Held Hessian: where every tile of the root batch holds its dynamics, the held factor entry exists and the packed Hessian RSQ of every
instance is bit for bit the same at the stages 0 .. N-1, the held factor launches read the copy of stage N-1 at every stage k < N
(GqpOpts::hold bit 2; option `hold_hessian`, default 1).  The loads return the same 64-bit patterns, so every output must be BIT FOR
BIT what `hold_dynamics 0` gives on the same data.  The outputs cannot tell which copy was read: scalar `hess_held_launches` counts
the launches with the bit, `hess_detector_runs` the runs of the detector in a solve (it runs once per version of the data, not per
solve).

Verdicts kept: a solve of a batch whose matrices no setter has touched since the last count starts from that count -- no detecting
sweep, and iteration 1 runs the held entries too.  A root loop that hands nothing over (tail_max = 0) launches the factor sweep
max(iter) + 1 times and the rhs sweep twice per iteration: a solve that detects holds max(iter) and 2 (max(iter) - 1) of them
(tests/test_hold_factor.py), a solve that starts from a kept count holds all max(iter) + 1 and 2 max(iter).

Recipe of tests/hold_common.py: nx = 8, nu = 3, batch 130 (two full tiles and a tile of 2 lanes), ACADOS_AMD_WPI=0, outputs x u pi
lam t iter status under numpy.array_equal, both tiers.  Horizons N = 3 (stage N keeps its own copy, N-1 is the copy read, the stages
1 and 0 are redirected), N = 2 (one stage is redirected) and N = 1 (none is: the detector compares nothing and the bit changes no
address)."""
import ctypes as C

import numpy as np
import pytest

import hold_common
from hold_common import B, MID, TIERS, TILES, assert_same, clib, outputs  # noqa: F401

ALONE = {"tail_max": 0}  # the root loop runs to the end by itself
VEC_FIELDS = ("b", "q", "r", "lbu", "ubu", "lbx", "lbx#value", "ubx", "lbu_mask", "ubu_mask", "lbx_mask", "ubx_mask")


def base_data(N):
    return hold_common.base_data(N, seed=47)


def make_batch(clib, N, hold, opts=None, data=None):
    return hold_common.make_batch(clib, data if data is not None else base_data(N), N, None, dict(opts or {}, hold_dynamics=hold))


def counts(gb):
    return {f: int(gb.scalar(f)) for f in ("tiles_invariant", "fact_held_launches", "rhs_held_launches", "hess_held_launches", "hess_detector_runs", "detecting_sweeps")}


def run_pair(clib, N, steps, opts=None, data=None):
    """the same sequence of steps (callables on a batch, each followed by a solve) on a batch with holding on and on its twin with
    hold_dynamics 0; the outputs of every solve must be equal.  Returns per solve (counts of the batch that holds, its outputs)"""
    on, off = make_batch(clib, N, 1, opts, data), make_batch(clib, N, 0, opts, data)
    res = []
    for step in steps:
        for gb in (on, off):
            if step is not None:
                step(gb)
            gb.solve()
        out_on, out_off = outputs(on, N), outputs(off, N)
        c_off = counts(off)
        assert c_off["fact_held_launches"] == 0 and c_off["rhs_held_launches"] == 0 and c_off["hess_held_launches"] == 0, c_off
        assert c_off["hess_detector_runs"] == 0 and c_off["detecting_sweeps"] == 0, c_off
        assert_same(out_on, out_off)
        res.append((counts(on), out_on))
    assert on.kernel_name.startswith("1tpi-box<NX=8,NU=3"), on.kernel_name
    return res


def detecting(c, out):
    """the counts of a root loop that detects and hands nothing over"""
    it = int(out["iter"].max())
    return c["tiles_invariant"] == TILES and c["fact_held_launches"] == it > 0 and c["rhs_held_launches"] == 2 * (it - 1) and c["detecting_sweeps"] == 1


def kept(c, out):
    """... and of one that starts from a kept count"""
    it = int(out["iter"].max())
    return c["tiles_invariant"] == TILES and c["fact_held_launches"] == it + 1 and c["rhs_held_launches"] == 2 * it > 0 and c["detecting_sweeps"] == 0


@pytest.mark.parametrize("N", [3, 2, 1])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_constant_data_reads_one_copy(clib, N):
    """every held factor launch carries the bit: the verdict is taken in front of the first of them"""
    (c, out), = run_pair(clib, N, [None], ALONE)
    print(N, c)
    assert np.all(out["status"] == 0)
    assert detecting(c, out), c
    assert c["hess_held_launches"] == c["fact_held_launches"] and c["hess_detector_runs"] == 1, c
    # option off: the held entry runs, every stage reads its own copy, the detector is not asked
    (c0, out0), = run_pair(clib, N, [None], dict(ALONE, hold_hessian=0))
    assert detecting(c0, out0) and c0["hess_held_launches"] == 0 and c0["hess_detector_runs"] == 0, c0
    assert_same(out, out0)


def _one_ulp(field, idx):
    def change(N):
        d = {k: v.copy() for k, v in base_data(N).items()}
        d[field][(MID,) + idx] = np.nextafter(d[field][(MID,) + idx], np.inf)
        assert np.sum(d[field] != base_data(N)[field]) == 1
        return None, d[field]
    return change


def _minus_zero(N):
    """an entry of S that is +0.0 in every instance and at every stage, made -0.0 in one instance at stage 1"""
    d = {k: v.copy() for k, v in base_data(N).items()}
    d["S"][:, 1, 4] = 0.0
    s1 = d["S"].copy()
    s1[MID, 1, 4] = -0.0
    assert np.array_equal(s1, d["S"]) and np.signbit(s1[MID, 1, 4]) and not np.signbit(d["S"][MID, 1, 4])
    return d, s1


# (lower triangle of Q and R: what the batch stores; S is nu x nx)
CHANGES = {"Q": ("Q", _one_ulp("Q", (5, 2))), "Q_diagonal": ("Q", _one_ulp("Q", (7, 7))), "R": ("R", _one_ulp("R", (2, 0))),
           "S": ("S", _one_ulp("S", (2, 7))), "minus_zero": ("S", _minus_zero)}


@pytest.mark.parametrize("what", list(CHANGES))
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_one_pattern_that_differs_keeps_every_copy(clib, what):
    """one ulp in one entry at stage 1 of one instance of the middle tile (N = 3: stage 1 is interior, and N - 1 = 2 is the last
    stage the detector reads), or +0.0 made -0.0: no launch reads one copy, the dynamics stay held"""
    N = 3
    field, change = CHANGES[what]
    data, at_stage_1 = change(N)
    (c, out), = run_pair(clib, N, [lambda gb: gb.set(field, 1, at_stage_1)], ALONE, data)
    print(what, c)
    assert detecting(c, out), c
    assert c["hess_held_launches"] == 0 and c["hess_detector_runs"] == 1, c


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_last_compared_stage(clib):
    """the same at stage N-1, the last one the detector compares, and at stage N, which it must not compare (Q of stage N is the
    terminal weight: any value there leaves the verdict positive, and the held launch must read stage N's own copy)"""
    N = 3
    q = base_data(N)["Q"].copy()
    q[MID, 3, 3] = np.nextafter(q[MID, 3, 3], np.inf)
    (c, out), = run_pair(clib, N, [lambda gb: gb.set("Q", N - 1, q)], ALONE)
    assert detecting(c, out) and c["hess_held_launches"] == 0, c
    qn = base_data(N)["Q"] * 1.5
    (c, out), = run_pair(clib, N, [lambda gb: gb.set("Q", N, qn)], ALONE)
    assert detecting(c, out) and c["hess_held_launches"] == c["fact_held_launches"], c


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_setter_between_solves_of_one_object(clib):
    """Q changed at stage 2, then restored: the verdict follows each time, and each change costs one run of the detector"""
    N = 3
    q = base_data(N)["Q"].copy()
    q[MID] = q[MID] * 1.25
    res = run_pair(clib, N, [None, lambda gb: gb.set("Q", 2, q), lambda gb: gb.set("Q", 2, base_data(N)["Q"]), None], ALONE)
    (c1, o1), (c2, o2), (c3, o3), (c4, o4) = res
    print(c1, c2, c3, c4)
    assert detecting(c1, o1) and c1["hess_held_launches"] == c1["fact_held_launches"] and c1["hess_detector_runs"] == 1
    # (a setter of Q leaves the count of the dynamics standing)
    assert kept(c2, o2) and c2["hess_held_launches"] == 0 and c2["hess_detector_runs"] == 1, c2
    assert kept(c3, o3) and c3["hess_held_launches"] == c3["fact_held_launches"] and c3["hess_detector_runs"] == 1, c3
    assert kept(c4, o4) and c4["hess_held_launches"] == c4["fact_held_launches"] and c4["hess_detector_runs"] == 0, c4
    assert_same(o1, o3)
    assert_same(o1, o4)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _vector_blob(gb, N, blob, scale_q):
    """the vector part of the input blob `blob`, q of stage 1 scaled"""
    vec = np.zeros((B, gb.bulk_len(2)))
    for k in range(N + 1):
        for f in VEC_FIELDS:
            vo, vl = gb.bulk_offset(2, f, k)
            if vo < 0 or vl == 0:
                continue
            io, il = gb.bulk_offset(0, f, k)
            assert il == vl, (f, k)
            vec[:, vo:vo + vl] = blob[:, io:io + il] * (scale_q if (f, k) == ("q", 1) else 1.0)
    return vec


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_bulk_setters(clib):
    """set_bulk_vec between two solves keeps both verdicts (no detecting sweep, no detector run); set_bulk of changed matrices
    detects both again, set_bulk of the matrices as they were too (a blob with matrices is new data whatever it holds)"""
    N = 3

    def vec_only(gb):
        blob = gb.get_bulk_in()
        assert gb._L.ocp_qp_gpu_batch_set_bulk_vec(gb._h, _vp(_vector_blob(gb, N, blob, 1.5)), 0) == 0

    def bulk_changed(gb):
        blob = gb.get_bulk_in()
        o, l = gb.bulk_offset(0, "Q", 1)
        blob[MID, o + 2 * hold_common.NX + 2] *= 1.0 + 2.0 ** -40   # Q[2, 2] of stage 1, one instance
        gb.set_bulk(blob)

    def bulk_restored(gb):
        blob = gb.get_bulk_in()
        o0, l = gb.bulk_offset(0, "Q", 0)
        o1, _ = gb.bulk_offset(0, "Q", 1)
        blob[:, o1:o1 + l] = blob[:, o0:o0 + l]
        gb.set_bulk(blob)

    (c1, o1), (c2, o2), (c3, o3), (c4, o4) = run_pair(clib, N, [None, vec_only, bulk_changed, bulk_restored], ALONE)
    print(c1, c2, c3, c4)
    assert detecting(c1, o1) and c1["hess_detector_runs"] == 1 and c1["hess_held_launches"] == c1["fact_held_launches"]
    assert kept(c2, o2) and c2["hess_detector_runs"] == 0 and c2["hess_held_launches"] == c2["fact_held_launches"], c2
    assert not np.array_equal(o1["x", 2], o2["x", 2])           # (the new q was solved)
    assert detecting(c3, o3) and c3["hess_detector_runs"] == 1 and c3["hess_held_launches"] == 0, c3
    assert detecting(c4, o4) and c4["hess_detector_runs"] == 1 and c4["hess_held_launches"] == c4["fact_held_launches"], c4
    assert_same(o2, o4)


@pytest.mark.parametrize("N", [3, 2, 1])
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_second_solve_of_unchanged_data_holds_from_the_first_launch(clib, N):
    """every factor and rhs launch of the root loop of the second solve is a held one; set("A") with the very same values is a
    write all the same: the third solve detects again.  Results equal in all three"""
    a = base_data(N)["A"]
    (c1, o1), (c2, o2), (c3, o3) = run_pair(clib, N, [None, None, lambda gb: gb.set("A", 0, a)], ALONE)
    print(c1, c2, c3)
    assert detecting(c1, o1), c1
    assert kept(c2, o2), c2
    assert c2["hess_held_launches"] == c2["fact_held_launches"] and c2["hess_detector_runs"] == 0, c2
    assert detecting(c3, o3), c3
    assert c3["hess_held_launches"] == c3["fact_held_launches"] and c3["hess_detector_runs"] == 0, c3   # (A is not the Hessian)
    assert_same(o1, o2)
    assert_same(o1, o3)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_time_varying_dynamics_pay_nothing_and_keep_their_count(clib):
    """one tile that must fetch: no held launch, the detector of the Hessian is never asked; the partial count is kept too (every
    instance was running when it was taken)"""
    N = 3
    a = base_data(N)["A"].copy()
    a[MID, 1, 2] = np.nextafter(a[MID, 1, 2], np.inf)
    (c1, o1), (c2, o2) = run_pair(clib, N, [lambda gb: gb.set("A", 1, a), None], ALONE)
    for c, d in ((c1, 1), (c2, 0)):
        assert c["tiles_invariant"] == TILES - 1 and c["fact_held_launches"] == 0 and c["rhs_held_launches"] == 0 and c["detecting_sweeps"] == d, c
        assert c["hess_held_launches"] == 0 and c["hess_detector_runs"] == 0, c
    assert_same(o1, o2)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_nan_stays_with_its_instance(clib):
    """a NaN in Q of one instance at one stage: its pattern differs from stage 0's, every stage reads its own copy; status 1 for
    that instance, every neighbour bit for bit as without it"""
    N = 3
    q = base_data(N)["Q"].copy()
    q[MID, 4, 4] = np.nan
    (c, out), = run_pair(clib, N, [lambda gb: gb.set("Q", 1, q)], ALONE)
    (_, clean), = run_pair(clib, N, [None], ALONE)
    bad = np.flatnonzero(out["status"] != 0)
    assert bad.tolist() == [MID] and out["status"][MID] == 1, bad
    assert_same(out, clean, skip=(MID,))
    assert c["tiles_invariant"] == TILES and c["fact_held_launches"] > 0 and c["hess_held_launches"] == 0, c


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_hand_overs_count_the_root_level_only(clib):
    """a tail hand-over (the defaults) and a compaction: the sub-level takes no part, in the first solve and in one that starts from
    a kept count (m factor launches of the root loop: m - 1 held and m - 2 rhs pairs when it detects, m and m - 1 pairs when not)"""
    N = 3
    for opts, scalar in (({}, "tail_switches"), ({"compact_min": 4, "tail_max": 0}, "compactions")):
        on = make_batch(clib, N, 1, opts)
        on.solve()
        first, c1 = outputs(on, N), counts(on)
        assert int(on.scalar(scalar)) >= 1
        on.solve()
        second, c2 = outputs(on, N), counts(on)
        assert int(on.scalar(scalar)) >= 1
        print(scalar, c1, c2)
        off = make_batch(clib, N, 0, opts)
        off.solve()
        assert_same(first, outputs(off, N))
        assert_same(second, first)
        assert first["iter"].max() >= 3
        assert c1["fact_held_launches"] == c1["rhs_held_launches"] // 2 + 1 and 0 < c1["fact_held_launches"] < first["iter"].max(), c1
        assert c2["fact_held_launches"] == c2["rhs_held_launches"] // 2 + 1 == c1["fact_held_launches"] + 1, c2
        for c in (c1, c2):
            assert c["tiles_invariant"] == TILES and c["hess_held_launches"] == c["fact_held_launches"], c
        assert c1["hess_detector_runs"] == 1 and c2["hess_detector_runs"] == 0


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_polish_pass_detects_for_itself(clib):
    """the polish pass is a root loop of its own and keeps detecting: in a solve that starts from a kept count it adds one held
    factor launch and no held rhs launch, as it does in a solve that detects (tests/test_hold_factor.py)"""
    N = 3
    plain = make_batch(clib, N, 1, ALONE)
    pol = make_batch(clib, N, 1, dict(ALONE, polish=1, polish_ratio=0.0))
    for gb in (plain, pol):
        gb.solve()
        gb.solve()
    cp, cq = counts(plain), counts(pol)
    print(cp, cq)
    assert int(pol.scalar("polished")) == B
    assert kept(cp, outputs(plain, N)), cp
    assert cq["fact_held_launches"] == cp["fact_held_launches"] + 1 and cq["rhs_held_launches"] == cp["rhs_held_launches"], cq
    assert cq["tiles_invariant"] == TILES and cq["detecting_sweeps"] == 0
    assert cq["hess_held_launches"] == cq["fact_held_launches"], cq

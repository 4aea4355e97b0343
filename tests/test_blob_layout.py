"""The blob entries of the C ABI (include/acados_amd/ocp_qp_gpu_batch.h; gpu_batch.hip, "bulk pack / unpack"), on both tiers.

Layout: the segment table of every blob kind -- input, output, vector part (_bulk_offset with output 0 / 1 / 2), seeds and
directions (_sens_bulk_offset with output 0 / 1) -- is rebuilt here from the rule of the header and the stage dimensions the
batch reports (_get_dims), and every (offset, length) and every length per instance is compared with it: stage-major, the
documented field order, fields of length 0 at a stage skipped.  The "lbx#value" segment follows EVERY lbx of non-zero length,
hence every equality-flagged one (the header names only those): its entries refer to something only where the row is
equality-flagged, and the segment tables of the acados-side adapter (integration/ocp_qp_gpu_segments.h) count on it at
every such stage.

Entries no other test calls directly, on 70 instances (one full tile of 64 and a ragged one) of the slack-and-equality structure
pendulum_slack with random data per instance: _set_bulk_vec, _set_bulk_out / _get_bulk, _sens_set_bulk / _sens_get_bulk
against the per-field seeds, is_device = 1 read-backs, and the time_pack bookkeeping of the four ways a blob comes in."""
import ctypes as C

import numpy as np
import pytest

from conftest import INPUT_ONLY, load_qp

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]

MASKS = ("lbu_mask", "ubu_mask", "lbx_mask", "ubx_mask", "lg_mask", "ug_mask", "lls_mask", "lus_mask")
MATRICES = ("A", "B", "Q", "S", "R", "C", "D", "Zl", "Zu")
IN_FIELDS = ("A", "B", "b", "Q", "S", "R", "q", "r", "lbu", "ubu", "lbx", "ubx", "lg", "ug", "C", "D", "Zl", "Zu", "zl", "zu",
             "lls", "lus") + MASKS
OUT_FIELDS = ("u", "x", "sl", "su", "pi", "lam", "t")
VEC_FIELDS = tuple(f for f in IN_FIELDS if f not in MATRICES)
SEED_FIELDS = ("r", "q", "zl", "zu", "b", "lbu", "lbx", "lg", "ubu", "ubx", "ug", "lls", "lus")
B = 70


@pytest.fixture
def clib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dims(gb):
    """the stage dimensions as the batch itself reports them"""
    one = np.zeros(1, dtype=np.int32)
    assert gb._L.ocp_qp_gpu_batch_get_dims(gb._h, b"N", one.ctypes.data_as(C.POINTER(C.c_int))) >= 0
    d = {"N": int(one[0])}
    for f in ("nx", "nu", "nbx", "nbu", "ng", "ns", "nbxe"):
        v = np.zeros(d["N"] + 1, dtype=np.int32)
        gb._L.ocp_qp_gpu_batch_get_dims(gb._h, f.encode(), v.ctypes.data_as(C.POINTER(C.c_int)))
        d[f] = [int(x) for x in v]
    return d


def _field_len(d, f, k):
    """doubles of field f at stage k (acados' shapes; dynamics and pi live at the stages 0 .. N-1)"""
    nx, nu, nbx, nbu, ng, ns = (d[n][k] for n in ("nx", "nu", "nbx", "nbu", "ng", "ns"))
    nx1 = d["nx"][k + 1] if k < d["N"] else 0
    if f.endswith("_mask"):
        f = f[:-5]
    return {"A": nx1 * nx, "B": nx1 * nu, "b": nx1, "Q": nx * nx, "S": nu * nx, "R": nu * nu, "q": nx, "r": nu,
            "lbu": nbu, "ubu": nbu, "lbx": nbx, "ubx": nbx, "lg": ng, "ug": ng, "C": ng * nx, "D": ng * nu,
            "Zl": ns, "Zu": ns, "zl": ns, "zu": ns, "lls": ns, "lus": ns,
            "u": nu, "x": nx, "sl": ns, "su": ns, "pi": nx1, "lam": 2 * (nbx + nbu + ng + ns), "t": 2 * (nbx + nbu + ng + ns)}[f]


def _expected(d, fields, prefix="", value_segment=False):
    """{(name, stage): (offset, length)} and the doubles per instance"""
    segs, off = {}, 0
    for k in range(d["N"] + 1):
        for f in fields:
            n = _field_len(d, f, k)
            if n == 0:
                continue
            segs[(prefix + f, k)] = (off, n)
            off += n
            if value_segment and f == "lbx":
                segs[("lbx#value", k)] = (off, n)
                off += n
    return segs, off


def _offset(gb, fn, output, name, k):
    n = C.c_int(-7)
    off = fn(gb._h, output, name.encode(), k, C.byref(n))
    return int(off), int(n.value)


def _structures():
    from acados_amd.generators import lqr_instance_qp, mass_spring_qp, random_lqr_batch
    out = [(p, lambda p=p: load_qp(p)) for p in INPUT_ONLY]
    out.append(("mass_spring_N3", lambda: mass_spring_qp(N=3)))
    out.append(("lqr_N1", lambda: lqr_instance_qp(random_lqr_batch(N=1, nx=4, nu=2, batch=1, seed=3), 0, 1)))
    return out


@pytest.mark.parametrize("clib", TIERS, indirect=True)
@pytest.mark.parametrize("make_qp", [pytest.param(m, id=n) for n, m in _structures()])
def test_segment_tables_follow_the_documented_rule(clib, make_qp):
    from acados_amd import OcpQpGpuBatch
    gb = OcpQpGpuBatch.from_qps([make_qp()] * 2, _clib=clib)
    L, d = gb._L, _dims(gb)
    kinds = [("input", L.ocp_qp_gpu_batch_bulk_len, L.ocp_qp_gpu_batch_bulk_offset, 0, IN_FIELDS, "", True),
             ("output", L.ocp_qp_gpu_batch_bulk_len, L.ocp_qp_gpu_batch_bulk_offset, 1, OUT_FIELDS, "", False),
             ("vector", L.ocp_qp_gpu_batch_bulk_len, L.ocp_qp_gpu_batch_bulk_offset, 2, VEC_FIELDS, "", True),
             ("seed", L.ocp_qp_gpu_batch_sens_bulk_len, L.ocp_qp_gpu_batch_sens_bulk_offset, 0, SEED_FIELDS, "seed_", False),
             ("direction", L.ocp_qp_gpu_batch_sens_bulk_len, L.ocp_qp_gpu_batch_sens_bulk_offset, 1, OUT_FIELDS, "sens_", False)]
    for kind, len_fn, off_fn, output, fields, prefix, value_segment in kinds:
        want, total = _expected(d, fields, prefix, value_segment)
        assert len_fn(gb._h, output) == total, kind
        names = [prefix + f for f in fields] + ["lbx#value", "no_such_field"]
        for k in range(d["N"] + 1):
            for name in names:
                # a field absent at a stage (length 0 there, or no field of this kind at all): -1 and length 0
                assert _offset(gb, off_fn, output, name, k) == want.get((name, k), (-1, 0)), (kind, name, k)
        for name in names:
            assert _offset(gb, off_fn, output, name, d["N"] + 1) == (-1, 0), (kind, name)
    # the value of an equality-flagged x sits right behind its bound
    for k in range(d["N"] + 1):
        if d["nbxe"][k]:
            for output in (0, 2):
                o, n = _offset(gb, L.ocp_qp_gpu_batch_bulk_offset, output, "lbx", k)
                assert n > 0 and _offset(gb, L.ocp_qp_gpu_batch_bulk_offset, output, "lbx#value", k) == (o + n, n), (output, k)
    # any other nonzero `output` is the output blob
    assert L.ocp_qp_gpu_batch_bulk_len(gb._h, 3) == L.ocp_qp_gpu_batch_bulk_len(gb._h, 1)
    for k in range(d["N"] + 1):
        for name in OUT_FIELDS + ("q", "lbx#value"):
            assert _offset(gb, L.ocp_qp_gpu_batch_bulk_offset, 3, name, k) == _offset(gb, L.ocp_qp_gpu_batch_bulk_offset, 1, name, k), (name, k)
    # the seed blob has no directions and the other way round
    assert _offset(gb, L.ocp_qp_gpu_batch_sens_bulk_offset, 0, "sens_x", 0) == (-1, 0)
    assert _offset(gb, L.ocp_qp_gpu_batch_sens_bulk_offset, 1, "seed_q", 0) == (-1, 0)
    assert _offset(gb, L.ocp_qp_gpu_batch_sens_bulk_offset, 1, "x", 0) == (-1, 0)


def _random_batch(clib, seed=1):
    """70 instances of pendulum_slack, every numeric entry its own: the structure's data scaled per instance and entry (signs and
    the symmetry of Q / R stay: the batch remains a convex QP that solves).  Returns the batch and its data as the batch holds it
    (input blob read back: the reference of the tests below, never written)"""
    from acados_amd import OcpQpGpuBatch
    qp = load_qp("casadi_qp_tests/pendulum_slack.json")
    gb = OcpQpGpuBatch.from_qps([qp] * B, _clib=clib)
    g = np.random.default_rng(seed)
    d = _dims(gb)
    blob = gb.get_bulk_in()
    segs, n = _expected(d, IN_FIELDS, value_segment=True)
    assert blob.shape == (B, n)
    for (f, k), (o, l) in segs.items():
        if f in ("b", "q", "r", "zl", "zu"):
            blob[:, o:o + l] *= g.uniform(0.8, 1.2, (B, l))
            blob[:, o:o + l] += 0.01 * g.standard_normal((B, l))
        elif f in ("Q", "R"):
            # full symmetric blocks: off-diagonal entries of at most 0.05 sqrt(M_ii M_jj), the block stays positive (semi)definite
            n_ = int(round(np.sqrt(l)))
            m = blob[:, o:o + l].reshape(B, n_, n_) * g.uniform(0.8, 1.2, (B, 1, 1))
            dg = np.sqrt(np.abs(np.einsum("bii->bi", m)))
            s_ = np.triu(g.uniform(-0.05, 0.05, (B, n_, n_)), 1)
            blob[:, o:o + l] = (m + (s_ + s_.transpose(0, 2, 1)) * dg[:, :, None] * dg[:, None, :]).reshape(B, l)
        elif f in ("Zl", "Zu"):
            blob[:, o:o + l] *= g.uniform(0.8, 1.2, (B, 1))
        elif f in ("A", "B", "S", "C", "D"):
            blob[:, o:o + l] *= g.uniform(0.95, 1.05, (B, l))
    gb.set_bulk(blob)
    ref = gb.get_bulk_in()
    ref.setflags(write=False)
    assert np.isfinite(ref).all() and len({ref[i].tobytes() for i in range(B)}) == B
    for (f, k), (o, l) in segs.items():
        if f in MATRICES:       # both triangles of Q and R included: what the per-field getter returns
            assert np.array_equal(ref[:, o:o + l], gb.get(f, k)), (f, k)
            assert f not in ("Q", "R") or l == 1 or np.count_nonzero(ref[:, o:o + l]) == ref[:, o:o + l].size, (f, k)
    return gb, d, segs, ref


def _eq_rows(gb, d, k):
    """positions inside lbx / ubx of the equality-flagged rows of stage k"""
    return gb.get_int("idxe", k) - d["nbu"][k] if d["nbxe"][k] else np.zeros(0, dtype=int)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_set_bulk_vec_leaves_the_matrices(clib):
    """(a) a vector blob with new vectors and masks: the matrices of the input blob stay byte-identical, the vector and mask
    entries read back are what was sent"""
    gb, d, segs, ref = _random_batch(clib)
    L = gb._L
    g = np.random.default_rng(2)
    vsegs, nv = _expected(d, VEC_FIELDS, value_segment=True)
    assert L.ocp_qp_gpu_batch_bulk_len(gb._h, 2) == nv
    vec = np.zeros((B, nv))
    for (f, k), (o, l) in vsegs.items():
        if f.endswith("_mask"):
            vec[:, o:o + l] = (g.uniform(size=(B, l)) < 0.8).astype(float)
            if f in ("lbx_mask", "ubx_mask"):
                vec[:, o + _eq_rows(gb, d, k)] = 1.0          # an equality-flagged row is always active
        elif f == "lbx#value":
            vec[:, o:o + l] = vec[:, o - l:o]                 # the same numbers as lbx
        else:
            vec[:, o:o + l] = g.standard_normal((B, l))
    assert L.ocp_qp_gpu_batch_set_bulk_vec(gb._h, _vp(vec), 0) == 0
    back = gb.get_bulk_in()
    for (f, k), (o, l) in segs.items():
        if f in MATRICES:
            assert back[:, o:o + l].tobytes() == ref[:, o:o + l].tobytes(), (f, k)
            assert np.array_equal(back[:, o:o + l], gb.get(f, k)), (f, k)
            continue
        vo, vl = vsegs[(f, k)]
        assert vl == l
        sent = vec[:, vo:vo + l]
        if f == "lbx#value":                                  # only the equality-flagged entries are the value of a variable
            eq = _eq_rows(gb, d, k)
            assert np.array_equal(back[:, o + eq], sent[:, eq]), (f, k)
        else:
            assert np.array_equal(back[:, o:o + l], sent), (f, k)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_set_bulk_out_get_bulk_round_trip(clib):
    """(b) an iterate written in the output blob layout comes back byte for byte"""
    gb, d, _, _ = _random_batch(clib)
    L = gb._L
    n = L.ocp_qp_gpu_batch_bulk_len(gb._h, 1)
    it = np.random.default_rng(3).standard_normal((B, n))
    assert L.ocp_qp_gpu_batch_set_bulk_out(gb._h, _vp(it), 0) == 0
    back = np.zeros((B, n))
    assert L.ocp_qp_gpu_batch_get_bulk(gb._h, _vp(back), 0) == 0
    assert back.tobytes() == it.tobytes()


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_bulk_seeds_equal_the_per_field_seeds(clib):
    """(c) _sens_set_bulk, _sens_solve, _sens_get_bulk: byte for byte the directions of the same seeds set field by field
    (_sens_set) and read field by field (_get "sens_*")"""
    gb, d, _, _ = _random_batch(clib)
    L = gb._L
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, 1e-8)
    assert gb.solve() == 0, gb.info("status")
    ssegs, ns_ = _expected(d, SEED_FIELDS, "seed_")
    osegs, no = _expected(d, OUT_FIELDS, "sens_")
    assert L.ocp_qp_gpu_batch_sens_bulk_len(gb._h, 0) == ns_ and L.ocp_qp_gpu_batch_sens_bulk_len(gb._h, 1) == no
    seeds = np.random.default_rng(4).standard_normal((B, ns_))
    for (f, k), (o, l) in ssegs.items():
        gb.sens_set(f, k, seeds[:, o:o + l])
    gb.sens_solve()
    single = np.zeros((B, no))
    for (f, k), (o, l) in osegs.items():
        single[:, o:o + l] = gb.get(f, k)
    assert np.isfinite(single).all() and np.abs(single).max() > 0
    assert L.ocp_qp_gpu_batch_sens_set_bulk(gb._h, _vp(seeds), 0) == 0
    gb.sens_solve()
    bulk = np.zeros((B, no))
    assert L.ocp_qp_gpu_batch_sens_get_bulk(gb._h, _vp(bulk), 0) == 0
    assert bulk.tobytes() == single.tobytes()


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_read_backs_into_device_visible_memory(clib):
    """(d) is_device = 1 with a pointer the device can write (ocp_qp_gpu_host_alloc: pinned and mapped on the GPU tier, plain memory
    under host simulation): _get_bulk and _get_bulk_in write what they copy to a host pointer"""
    gb, d, _, ref = _random_batch(clib)
    L = gb._L
    n1 = L.ocp_qp_gpu_batch_bulk_len(gb._h, 1)
    it = np.random.default_rng(5).standard_normal((B, n1))
    assert L.ocp_qp_gpu_batch_set_bulk_out(gb._h, _vp(it), 0) == 0
    for fn, n in ((L.ocp_qp_gpu_batch_get_bulk, n1), (L.ocp_qp_gpu_batch_get_bulk_in, ref.shape[1])):
        host = np.zeros((B, n))
        assert fn(gb._h, _vp(host), 0) == 0
        assert np.isfinite(host).all() and np.abs(host).max() > 0
        p = L.ocp_qp_gpu_host_alloc(host.nbytes)
        assert p
        try:
            mem = np.ctypeslib.as_array((C.c_double * host.size).from_address(p))
            mem[:] = np.nan
            assert fn(gb._h, C.c_void_p(p), 1) == 0
            assert mem.tobytes() == host.tobytes()
        finally:
            del mem
            L.ocp_qp_gpu_host_free(C.c_void_p(p))


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_time_pack_grows_once_per_blob(clib):
    """the four ways an input blob comes in add the time of their copies and launches to time_pack: a finite, non-negative amount
    each (host simulation has no meaningful clock: no ratio is asserted; reading the scalar resets it)"""
    gb, d, _, ref = _random_batch(clib)
    L = gb._L
    n, nv = ref.shape[1], L.ocp_qp_gpu_batch_bulk_len(gb._h, 2)
    blob = np.array(ref)
    vec = np.zeros((B, nv))
    for (f, k), (o, l) in _expected(d, VEC_FIELDS, value_segment=True)[0].items():
        io, il = _offset(gb, L.ocp_qp_gpu_batch_bulk_offset, 0, f, k)
        vec[:, o:o + l] = blob[:, io:io + il]
    # the gather's word table: one source array per instance, the blob itself
    block = np.array(ref)
    ptrs = np.array([block[i].ctypes.data for i in range(B)], dtype=np.uint64)
    idx = np.arange(n, dtype=np.int32)
    zero, neg = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    assert L.ocp_qp_gpu_batch_gather_tables(gb._h, 0, 1, n, _vp(zero), _vp(idx), _vp(idx), _vp(neg)) == 0

    def staged():
        for lo, hi in ((0, 33), (33, B)):
            assert L.ocp_qp_gpu_batch_set_bulk_chunk(gb._h, _vp(blob[lo:hi]), lo, hi - lo) == 0
        return L.ocp_qp_gpu_batch_set_bulk_staged(gb._h)

    assert L.ocp_qp_gpu_host_register(_vp(block), block.nbytes) == 0
    try:
        steps = {"set_bulk": lambda: L.ocp_qp_gpu_batch_set_bulk(gb._h, _vp(blob), 0),
                 "set_bulk_vec": lambda: L.ocp_qp_gpu_batch_set_bulk_vec(gb._h, _vp(vec), 0),
                 "staged": staged,
                 "gather_run": lambda: L.ocp_qp_gpu_batch_gather_run(gb._h, 0, _vp(ptrs))}
        grown = {}
        for name, step in steps.items():
            gb.scalar("time_pack")                       # (reads and resets)
            assert step() == 0, name
            grown[name] = gb.scalar("time_pack")
            assert np.isfinite(grown[name]) and grown[name] >= 0.0, (name, grown[name])
            assert gb.scalar("time_pack") == 0.0
            assert gb.get_bulk_in().tobytes() == ref.tobytes(), name
        # the gather counts its scatter once: its own measurement, not that plus a _set_bulk's on top (both finite, >= 0)
        assert np.isfinite(grown["gather_run"] + grown["set_bulk"]) and grown["gather_run"] + grown["set_bulk"] >= 0.0
        print("time_pack increments (s):", grown)
    finally:
        assert L.ocp_qp_gpu_host_unregister(_vp(block)) == 0


def _every_structure():
    from random_qp import random_structure_qp
    return _structures() + [(f"random_{s}", lambda s=s: random_structure_qp(s)) for s in (0, 1, 8, 11)]


@pytest.mark.parametrize("clib", TIERS, indirect=True)
@pytest.mark.parametrize("make_qp", [pytest.param(m, id=n) for n, m in _every_structure()])
def test_every_field_through_the_blob_and_the_getter(clib, make_qp):
    """The element rule of every field, through the blob entries and through the per-field getter, against the documented layout
    (_expected), on structures with changing dims, equality-flagged rows, general rows and slacks.  Entry e of instance i of the
    input blob is 1000 (i + 1) + e + 1 (a mask entry (e + i) mod 2), so an entry that lands in another place is seen.
    (a) after _set_bulk, get(f, k) is the blob's segment (f, k) for every input field and mask; Q and R come back as the symmetric
        matrix of the segment's lower triangle, lbx_mask / ubx_mask are compared without the equality-flagged rows (always active),
        the lbx#value segment has no getter;
    (b) _get_bulk_in returns the blob except in the upper triangles of Q / R, the mask entries of equality-flagged rows and the
        lbx#value entries of rows that are not equality-flagged;
    (c) after _set_bulk_out of 500 (i + 1) + e + 1, get(f, k) of u x sl su pi lam t is the segment."""
    from acados_amd import OcpQpGpuBatch
    gb = OcpQpGpuBatch.from_qps([make_qp()] * B, _clib=clib)
    d = _dims(gb)
    segs, n = _expected(d, IN_FIELDS, value_segment=True)
    inst = np.arange(B)[:, None]
    blob = 1000.0 * (inst + 1) + np.arange(n)[None, :] + 1.0
    free = np.zeros(n, dtype=bool)                       # entries _get_bulk_in need not return as they were sent
    for (f, k), (o, l) in segs.items():
        if f.endswith("_mask"):
            blob[:, o:o + l] = (np.arange(o, o + l)[None, :] + inst) % 2
            if f in ("lbx_mask", "ubx_mask"):
                free[o + _eq_rows(gb, d, k)] = True
        elif f in ("Q", "R"):
            m = int(round(np.sqrt(l)))
            free[o:o + l] = np.triu(np.ones((m, m), dtype=bool), 1).reshape(-1, order="F")
        elif f == "lbx#value":
            free[o:o + l] = True
            free[o + _eq_rows(gb, d, k)] = False
    sent = blob.copy()
    gb.set_bulk(blob)
    for (f, k), (o, l) in segs.items():
        if f == "lbx#value":
            continue
        want, got = sent[:, o:o + l], gb.get(f, k)
        if f in ("Q", "R"):
            m = int(round(np.sqrt(l)))
            low = np.tril(want.reshape(B, m, m).transpose(0, 2, 1))          # column-major segment -> [row, column]
            want = (low + np.tril(low, -1).transpose(0, 2, 1)).transpose(0, 2, 1).reshape(B, l)
        elif f in ("lbx_mask", "ubx_mask"):
            keep = np.setdiff1d(np.arange(l), _eq_rows(gb, d, k))
            want, got = want[:, keep], got[:, keep]
        assert np.array_equal(got, want), (f, k)
    back = gb.get_bulk_in()
    assert np.array_equal(back[:, ~free], sent[:, ~free]), np.argwhere(back[:, ~free] != sent[:, ~free])[:5]
    osegs, no = _expected(d, OUT_FIELDS)
    ob = 500.0 * (inst + 1) + np.arange(no)[None, :] + 1.0
    gb._blob_call(gb._L.ocp_qp_gpu_batch_set_bulk_out, ob, 1, "ocp_qp_gpu_batch_set_bulk_out")
    for (f, k), (o, l) in osegs.items():
        assert np.array_equal(gb.get(f, k), ob[:, o:o + l]), (f, k)

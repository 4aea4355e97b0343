"""What the stage-wise test files share (test_family_stage_edges.py, test_family_handovers.py, test_pcond_stagewise.py): one way to give
every stage of any batch data of its own, the table of the solver families with the recipe that pins each of them, the table of the
hand-overs between them, and the oracle's solve of an instance's read-back QP.

The generators of acados_amd.generators repeat ONE block [B A], one Hessian and one set of bounds over the horizon, so a sweep
that fetched stage k +- 1's block, mask word, bound vector or descriptor would not be noticed on their data.  stagewise_perturb
works through the input blob (get_bulk_in / bulk_offset / set_bulk), so one helper serves every structure.
A plain module like random_qp.py and hold_common.py."""
import numpy as np
import pytest

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
KKT_TOL = 2e-8       # the bar the suite uses for an independently recomputed residual of a solve at 1e-8

POS = ("Q", "R", "Zl", "Zu", "zl", "zu")          # x a positive scalar in [1, 1.5]: a positive definite block stays one
LIN = ("q", "r")                                  # + 0.05 N(0,1) per element
ANY = ("S", "A", "B", "b", "C", "D")              # x (1 + 0.05 N(0,1)) per element
LOW = ("lbu", "lbx", "lg")                        # - 0.3 U |v|: moved down
UPP = ("ubu", "ubx", "ug")                        # + 0.3 U |v|: moved up
PERTURBED = POS + LIN + ANY + LOW + UPP


def stagewise_perturb(gb, seed):
    """every field of every stage of the batch gb changed by a factor or an offset of its own, drawn per (stage, field) and shared
    by the instances (which differ through the generators); the x0 equality of stage 0 (lbx / ubx there) is left alone; bounds only
    move outwards, so a feasible QP stays feasible.  Asserted after the write, on the blob read back: every perturbed field that
    exists with the same length at stages k and k + 1 and is not identically zero there (S of chain_soft_qp is: no factor makes it
    stage-wise) differs between the two stages in EVERY instance, and instances 0 and 1 differ.  Returns the blob written."""
    g = np.random.default_rng(seed)
    blob = gb.get_bulk_in()
    N, B = gb.N, gb.n_batch
    for k in range(N + 1):
        for f in PERTURBED:
            o, n = gb.bulk_offset(0, f, k)
            if o < 0 or n <= 0 or (k == 0 and f in ("lbx", "ubx")):
                continue
            v = blob[:, o:o + n]
            if f in POS:
                v = v * (1.0 + 0.5 * g.uniform())
            elif f in LIN:
                v = v + 0.05 * g.standard_normal((1, n))
            elif f in ANY:
                v = v * (1.0 + 0.05 * g.standard_normal((1, n)))
            elif f in LOW:
                v = v - 0.3 * g.uniform() * np.abs(v)
            else:
                v = v + 0.3 * g.uniform() * np.abs(v)
            blob[:, o:o + n] = v
    gb.set_bulk(blob)
    back = gb.get_bulk_in()
    assert np.array_equal(back, blob)
    compared = 0
    for k in range(N):
        for f in PERTURBED:
            (o0, n0), (o1, n1) = gb.bulk_offset(0, f, k), gb.bulk_offset(0, f, k + 1)
            if o0 < 0 or o1 < 0 or n0 <= 0 or n0 != n1:
                continue
            a, b = back[:, o0:o0 + n0], back[:, o1:o1 + n1]
            if not a.any() and not b.any():
                continue
            assert np.all(np.any(a != b, axis=1)), (f, k, "stages k and k + 1 carry the same data in some instance")
            compared += 1
    assert compared >= 2 or N < 2, compared       # N = 1: Q (and q) of stages 0 and 1 at the least
    assert compared >= 1
    if B > 1:
        assert np.any(back[0] != back[1])
    return blob


# ---- the QPs of the table rows (host objects; the batch is built from them, then perturbed) -------------------------------------
def _lqr(nx, nu, xbox=False):
    """random_lqr_batch as host QPs; xbox: state bounds +-50 on every state after stage 0 (never active: they select the XBOX kernels
    and put a second bound vector into every stage), as test_small_block_pipeline_bit_identical_hostsim builds them"""
    def make(N, B, seed):
        from acados_amd.generators import lqr_instance_qp, random_lqr_batch
        data = random_lqr_batch(N=N, nx=nx, nu=nu, batch=B, seed=seed)
        qps = [lqr_instance_qp(data, i, N) for i in range(B)]
        if xbox:
            for qp in qps:
                for k in range(1, N + 1):
                    qp.set("idxb", k, np.arange((nu if k < N else 0) + nx))
                    qp.set("lbx", k, np.full(nx, -50.0))
                    qp.set("ubx", k, np.full(nx, 50.0))
                qp.make_consistent()
        return qps
    return make


def _chain(**kw):
    def make(N, B, seed):
        from acados_amd.generators import chain_soft_qp
        return [chain_soft_qp(i, N=N, seed=seed, **kw) for i in range(B)]
    return make


def structure_cases(qp):
    """which of the four structure cases a QP holds (as tests/test_data_grad.py::test_random_structures_cover_the_cases finds them)"""
    seen = set()
    for k in range(qp.N + 1):
        if int(qp.dims.ng[k]):
            seen.add("general")
        rev = np.asarray(qp.idxs_rev[k]).astype(int)
        if rev.size and np.any(rev >= 0) and len(set(rev[rev >= 0])) < int(np.sum(rev >= 0)):
            seen.add("shared")
        for f in ("lbu_mask", "ubu_mask", "lbx_mask", "ubx_mask", "lg_mask", "ug_mask"):
            m = np.asarray(getattr(qp, f)[k])
            if m.size and np.any(m == 0):
                seen.add("one-sided")
        if len(qp.idxe[k]):
            seen.add("x0")
    return seen


def structure_seed(N):
    """the first seed from 0 whose random_structure_qp of N stages holds a shared slack, a masked side, an equality-flagged x0 and
    general rows all together (N = 2: seed 9, nx = nu = 3; N = 9: seed 4, nx = 5, nu = 3, slacks at seven stages)"""
    from random_qp import random_structure_qp
    if N not in _STRUCT_SEED:
        _STRUCT_SEED[N] = next(s for s in range(1000) if structure_cases(random_structure_qp(s, N=N)) == {"general", "shared", "one-sided", "x0"})
    return _STRUCT_SEED[N]


_STRUCT_SEED = {}


def _struct(N, B, seed):
    """B copies of ONE random structure; make_batch makes the instances differ through the input blob (instance_noise)"""
    from random_qp import random_structure_qp
    return [random_structure_qp(structure_seed(N), N=N)] * B


def instance_noise(gb, seed):
    """q and r of instance i + 0.3 N(0,1), drawn per instance (a stream of its own per (seed, i): batches stay prefixes of one another);
    bounds and dynamics are untouched, so feasibility is that of the one structure.  Asserted on the blob read back: every instance
    differs from every other one.  Returns the blob written."""
    blob = gb.get_bulk_in()
    for i in range(gb.n_batch):
        g = np.random.default_rng([seed, i])
        for k in range(gb.N + 1):
            for f in LIN:
                o, n = gb.bulk_offset(0, f, k)
                if o >= 0 and n > 0:
                    blob[i, o:o + n] += 0.3 * g.standard_normal(n)
    gb.set_bulk(blob)
    back = gb.get_bulk_in()
    assert np.array_equal(back, blob)
    assert len({back[i].tobytes() for i in range(gb.n_batch)}) == gb.n_batch
    return blob


# instance i of a generator is the same QP whatever the batch size (counter-based streams), and the perturbation is drawn per
# (generator, N): the batches of one (row, N) are prefixes of one another, and rows that share a generator solve the same data
GENERATORS = {"lqr41": _lqr(4, 1), "lqr41x": _lqr(4, 1, xbox=True), "lqr83": _lqr(8, 3), "lqr124": _lqr(12, 4), "lqr815": _lqr(8, 15),
              "lqr246": _lqr(24, 6), "lqr144": _lqr(14, 4), "chain24": _chain(), "chain8": _chain(nx=8, nu=3, ng=4, nsx=2), "struct": _struct}
# generator seed per (generator, N), chosen WITH THE ORACLE ALONE (no kernel took part): the smallest seed from 1 at which the
# oracle's iteration counts of instances 0, 1, 2 of the perturbed batch take at least two values, so every batch of three or more
# holds instances that finish at different iterations
SEEDS = {g: {1: 1, 2: 1, 3: 1, 9: 1} for g in GENERATORS}
SEEDS["lqr144"].update({2: 2, 9: 2})
SEEDS["chain24"].update({2: 2})


def row_seed(row, N, handover=False):
    r = ROWS[row]
    return HANDOVER_SEEDS[(r["gen_key"], N, r["unit"])] if handover else SEEDS[r["gen_key"]][N]


def row_qps(row, N, B, handover=False):
    return GENERATORS[ROWS[row]["gen_key"]](N, B, row_seed(row, N, handover))


def perturb_seed(row, N, handover=False):
    return 7000 + 100 * row_seed(row, N, handover) + N


W16 = {"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "1"}
# env / opts / name / scalars as ROWS of tests/test_instance_isolation.py has them for the rows both tables hold.  gen_key: the row's
# generator; unit: instances that share a wave (64) or a workgroup of four 16-lane rows (4), 1: nothing but the launch; gen: general
# rows and slacks (sl su t are compared too, at 1e-7); slow: 3 to 16 s per case under host simulation.
# wpi-box<8,15> and its /rt twin report one name: the compile-time instantiation (GQP_CT of choose_family) is what the default takes at
# this shape, ACADOS_AMD_WPI_CT=0 is what keeps the run-time-shaped kernels
FAMILIES = {
    "1tpi-pipe": dict(env={"ACADOS_AMD_WPI": "0"}, gen_key="lqr41", name=("1tpi-pipe<NX=4,NU=1,XBOX=0",), unit=64),
    "1tpi-pipe/xbox": dict(env={"ACADOS_AMD_WPI": "0"}, gen_key="lqr41x", name=("1tpi-pipe<NX=4,NU=1,XBOX=1",), unit=64),
    "1tpi-gen": dict(env={"ACADOS_AMD_WPI": "0"}, gen_key="chain24", name=("1tpi<",), unit=64, gen=True),
    "w16-box/kx_solve": dict(env=W16, gen_key="lqr83", name=("w16-box<NX=8,NU=3>",), unit=4, scalars={"single_launch_solves": 1}),
    "w16-box/sweeps": dict(env=W16, opts={"solve_max": 0}, gen_key="lqr83", name=("w16-box<NX=8,NU=3>",), unit=4,
                           scalars={"single_launch_solves": 0}),
    "w16-box<12,4>": dict(env=W16, gen_key="lqr124", name=("w16-box<NX=12,NU=4>",), unit=4),
    "w16r-box/tiles": dict(env=W16, gen_key="lqr815", name=("w16r-box<NX=8,NU=15>",), unit=4, scalars={"w16_tiles": 1}),
    "w16r-box/rows": dict(env=dict(W16, ACADOS_AMD_W16T="0"), gen_key="lqr815", name=("w16r-box<NX=8,NU=15>",), unit=4,
                          scalars={"w16_tiles": 0}),
    "w16r-box<24,6>": dict(env=W16, gen_key="lqr246", name=("w16r-box<NX=24,NU=6>",), unit=4, scalars={"w16_tiles": 1}, slow=True),
    "w16r-gen8/tiles": dict(env=dict(W16, ACADOS_AMD_W16G="1"), gen_key="chain8", name=("w16r-gen<NX=8,NU=3,NG=4>",), unit=4, gen=True,
                            scalars={"w16_tiles": 1}),
    "w16r-gen8/rows": dict(env=dict(W16, ACADOS_AMD_W16G="1", ACADOS_AMD_W16T_GEN="0"), gen_key="chain8",
                           name=("w16r-gen<NX=8,NU=3,NG=4>",), unit=4, gen=True, scalars={"w16_tiles": 0}),
    "w16r-gen24/tiles": dict(env=dict(W16, ACADOS_AMD_W16G="1"), gen_key="chain24", name=("w16r-gen<NX=24,NU=3,NG=4>",), unit=4, gen=True,
                             scalars={"w16_tiles": 1}, slow=True),
    "wpi-box": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "0"}, gen_key="lqr83", name=("wpi-box(nx=8,nu=3,",), unit=1),
    "wpi-box<8,15>": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "0"}, gen_key="lqr815", name=("wpi-box(nx=8,nu=15,",), unit=1),
    "wpi-box<8,15>/rt": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "0", "ACADOS_AMD_WPI_CT": "0"}, gen_key="lqr815",
                             name=("wpi-box(nx=8,nu=15,",), unit=1),
    "wpi-mfma": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16R": "0", "ACADOS_AMD_WPI_MFMA": "1"}, gen_key="lqr144",
                     name=("wpi-box(nx=14,nu=4", "mfma"), unit=1),
    "wpi-gen": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16G": "0"}, gen_key="chain24", name=("wpi-gen(",), unit=1, gen=True),
    "ric0": dict(env=W16, opts={"ric_alg": 0}, gen_key="lqr83", name=("wpi-box(", ",ric0"), unit=1),
}
# ---- hand-overs (test_family_handovers.py) --------------------------------------------------------------------------------------
# one-instance-per-lane rows that FAMILIES does not hold: the C2 box kernels, and ONE random structure (tests/random_qp.py) with a
# shared slack, a masked side, an equality-flagged x0 and general rows, whose instances differ in q and r (instance_noise)
LANE = {"ACADOS_AMD_WPI": "0"}
HANDOVER_ROWS = {
    "1tpi-box<8,3>": dict(env=LANE, gen_key="lqr83", name=("1tpi-box<NX=8,NU=3,XBOX=0",), unit=64),
    "1tpi-gen/struct": dict(env=LANE, gen_key="struct", name=("1tpi<",), unit=64, gen=True),
}
ROWS = dict(FAMILIES, **HANDOVER_ROWS)
# lane row -> tail family: env steers sub_batch_create (family_switches) beside the row's own switches; tail: what
# ocp_qp_gpu_batch_tail_kernel_name reports (prefix, then substrings); slow: the tail family costs about a second per instance and
# stage sweep under host simulation
HANDOVERS = {
    "1tpi-box<8,3>/w16-box": dict(row="1tpi-box<8,3>", env={}, tail=("w16-box<NX=8,NU=3>",)),
    "1tpi-box<8,3>/wpi-box": dict(row="1tpi-box<8,3>", env={"ACADOS_AMD_W16": "0"}, tail=("wpi-box(nx=8,nu=3,",)),
    "1tpi-pipe/w16-box": dict(row="1tpi-pipe", env={}, tail=("w16-box<NX=4,NU=1>",)),
    "1tpi-pipe/wpi-box": dict(row="1tpi-pipe", env={"ACADOS_AMD_W16": "0"}, tail=("wpi-box(nx=4,nu=1,",)),
    "1tpi-pipe/xbox/w16-box": dict(row="1tpi-pipe/xbox", env={}, tail=("w16-box<NX=4,NU=1>",)),
    "1tpi-pipe/xbox/wpi-box": dict(row="1tpi-pipe/xbox", env={"ACADOS_AMD_W16": "0"}, tail=("wpi-box(nx=4,nu=1,",)),
    "1tpi-gen/w16r-gen/tiles": dict(row="1tpi-gen", env={}, tail=("w16r-gen<NX=24,NU=3,NG=4>",), slow=True),
    "1tpi-gen/w16r-gen/rows": dict(row="1tpi-gen", env={"ACADOS_AMD_W16T_GEN": "0"}, tail=("w16r-gen<NX=24,NU=3,NG=4>",),
                                   slow=True),
    "1tpi-gen/wpi-gen": dict(row="1tpi-gen", env={"ACADOS_AMD_W16G": "0"}, tail=("wpi-gen(nx=24,nu=3,ng=4,ns=8,",)),
    "1tpi-gen/struct/wpi-gen": dict(row="1tpi-gen/struct", env={}, tail=("wpi-gen(",)),
}
# generator seed per (generator, N, unit of the rows that use it), chosen WITH THE ORACLE ALONE (no kernel took part): the smallest
# seed from 1 at which the oracle's iteration counts c of the batch satisfy, at both batch sizes B of the unit (HANDOVER_BATCHES):
# c takes at least three values; some iteration j has 1 <= #{c > j} <= B / 2 (a compaction level is entered with compact_min 2);
# and for the one-instance-per-lane generators (unit 64, tail cases): max c is attained by exactly ONE instance (the late tail:
# exactly one survivor) and some j has 1 <= #{c > j} <= B / 4 (the default tail_div); and for the two generators of the combined case
# (lqr41x, chain24) at the larger B: some j has B / 4 < #{c > j} <= B / 2 (the level is entered before the tail rule holds).  Every test
# asserts its rule on the counts.
HANDOVER_BATCHES = {4: (5, 7), 64: (65, 130), 1: (3, 5)}
HANDOVER_SEEDS = {          # (the values the oracle's counts take at the larger batch size)
    ("lqr41", 2, 64): 1,      # 3 .. 8
    ("lqr41", 9, 64): 3,      # 4 .. 10
    ("lqr41x", 2, 64): 3,     # 3 .. 9
    ("lqr41x", 9, 64): 5,     # 4 .. 11
    ("lqr83", 2, 64): 2,      # 4 .. 10
    ("lqr83", 9, 64): 4,      # 5 .. 11
    ("chain24", 2, 64): 3,    # 6 .. 12, 14, 15
    ("chain24", 9, 64): 2,    # 7 .. 15
    ("struct", 2, 64): 1,     # 5 .. 11     (the seed of the instance noise; the structure: structure_seed)
    ("struct", 9, 64): 1,     # 10 .. 14
    ("lqr83", 2, 4): 1,       # 4 .. 8
    ("lqr83", 9, 4): 2,       # 6 .. 9
    ("lqr124", 2, 4): 1,      # 5, 6, 8
    ("lqr124", 9, 4): 1,      # 6 .. 10
    ("lqr815", 2, 4): 1,      # 5 .. 9
    ("lqr815", 9, 4): 1,      # 6, 7, 8
    ("lqr246", 2, 4): 1,      # 5, 6, 7
    ("lqr246", 9, 4): 1,      # 8, 9, 11
    ("chain8", 2, 4): 1,      # 5, 7, 8, 9, 11
    ("chain8", 9, 4): 1,      # 9, 10, 11
    ("chain24", 2, 4): 1,     # 8, 9, 10, 13
    ("chain24", 9, 4): 2,     # 9, 11, 12
    ("lqr83", 2, 1): 1,       # 4, 5, 6
    ("lqr83", 9, 1): 2,       # 6 .. 9
    ("lqr815", 2, 1): 11,     # 5 .. 8
    ("lqr815", 9, 1): 2,      # 6 .. 9
    ("lqr144", 2, 1): 2,      # 5, 6, 7
    ("lqr144", 9, 1): 2,      # 6, 8, 9
    ("chain24", 2, 1): 5,     # 9 .. 13
    ("chain24", 9, 1): 2,     # 9, 11, 12
}
BATCHES = {4: (1, 5, 7), 64: (1, 63, 65, 130), 1: (1, 3)}
RAGGED = {4: 5, 64: 65, 1: 3}
# 9: longer than every ring (kbs_pipeline: KBS_DEPTH = KBS_DEPTH_XBOX = 2 records; kx_factor_body: PD = W16Prefetch::FACTOR = 1) and than
# every stage-ahead fetch (one stage); what test_small_block_pipeline_bit_identical_hostsim uses
HORIZONS = (1, 2, 3, 9)
LONG = 9


def make_batch(clib, monkeypatch, row, N, B, iter_max=60, handover=False):
    """the row's batch of B instances over N stages, made stage-wise (the structure row: its instances made different), with the
    options of the family tests: all four tolerances 1e-8, no hand-over of the tail (the whole solve stays on the family under test),
    iter_max 60; handover: the generator seed of HANDOVER_SEEDS instead of SEEDS"""
    from acados_amd import OcpQpGpuBatch
    r = ROWS[row]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    gb = OcpQpGpuBatch.from_qps(row_qps(row, N, B, handover), _clib=clib)
    if r["gen_key"] == "struct":
        instance_noise(gb, perturb_seed(row, N, handover))
    else:
        stagewise_perturb(gb, perturb_seed(row, N, handover))
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, 1e-8)
    gb.opts_set("tail_max", 0)
    gb.opts_set("iter_max", iter_max)
    for k, v in r.get("opts", {}).items():
        gb.opts_set(k, v)
    return gb


def check_family(gb, row):
    """after a solve: the row ran on the family it names"""
    r = ROWS[row]
    assert gb.kernel_name.startswith(r["name"][0]) and all(s in gb.kernel_name for s in r["name"][1:]), (row, gb.kernel_name)
    for s, v in r.get("scalars", {}).items():
        assert int(gb.scalar(s)) == v, (row, s, gb.scalar(s))


_ORACLE = {}


def oracle_solve(gb, blob, i):
    """(qp, oracle) of the oracle's solve of instance i's own read-back QP; computed once per data (the key is the instance's input
    blob: rows that share a generator and batches that are prefixes of one another hold the same instance bit for bit)"""
    from oracle.oracle import OracleQp, default_opts
    key = (gb.dims.signature(), blob[i].tobytes())
    if key not in _ORACLE:
        qp = gb.to_qp(i)
        o = OracleQp(qp)
        o.solve(default_opts(tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8, iter_max=60))
        _ORACLE[key] = (qp, o)
    return _ORACLE[key]


def oracle_counts(gb, blob):
    """the oracle's iteration count of every instance of the batch (every one solved: status 0)"""
    out = np.zeros(gb.n_batch, dtype=int)
    for i in range(gb.n_batch):
        _, o = oracle_solve(gb, blob, i)
        assert o.status == 0, (i, o.status)
        out[i] = o.iter
    return out


def compared_lanes(B):
    """instances compared with the oracle: all of a batch of at most 8; of a larger one the lanes at the wave boundaries"""
    return list(range(B)) if B <= 8 else sorted({0, 1, 31, 62, 63, 64, B // 2, B - 2, B - 1} & set(range(B)))

"""What the stage-wise test files share (test_family_stage_edges.py, test_pcond_stagewise.py): one way to give every stage of any
batch data of its own, and the table of the solver families with the recipe that pins each of them.

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


# instance i of a generator is the same QP whatever the batch size (counter-based streams), and the perturbation is drawn per
# (generator, N): the batches of one (row, N) are prefixes of one another, and rows that share a generator solve the same data
GENERATORS = {"lqr41": _lqr(4, 1), "lqr41x": _lqr(4, 1, xbox=True), "lqr83": _lqr(8, 3), "lqr124": _lqr(12, 4), "lqr815": _lqr(8, 15),
              "lqr246": _lqr(24, 6), "lqr144": _lqr(14, 4), "chain24": _chain(), "chain8": _chain(nx=8, nu=3, ng=4, nsx=2)}
# generator seed per (generator, N), chosen WITH THE ORACLE ALONE (no kernel took part): the smallest seed from 1 at which the
# oracle's iteration counts of instances 0, 1, 2 of the perturbed batch take at least two values, so every batch of three or more
# holds instances that finish at different iterations
SEEDS = {g: {1: 1, 2: 1, 3: 1, 9: 1} for g in GENERATORS}
SEEDS["lqr144"].update({2: 2, 9: 2})
SEEDS["chain24"].update({2: 2})


def row_qps(row, N, B):
    g = FAMILIES[row]["gen_key"]
    return GENERATORS[g](N, B, SEEDS[g][N])


def perturb_seed(row, N):
    g = FAMILIES[row]["gen_key"]
    return 7000 + 100 * SEEDS[g][N] + N


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
BATCHES = {4: (1, 5, 7), 64: (1, 63, 65, 130), 1: (1, 3)}
RAGGED = {4: 5, 64: 65, 1: 3}
# 9: longer than every ring (kbs_pipeline: KBS_DEPTH = KBS_DEPTH_XBOX = 2 records; kx_factor_body: PD = W16Prefetch::FACTOR = 1) and than
# every stage-ahead fetch (one stage); what test_small_block_pipeline_bit_identical_hostsim uses
HORIZONS = (1, 2, 3, 9)
LONG = 9


def make_batch(clib, monkeypatch, row, N, B, iter_max=60):
    """the row's batch of B instances over N stages, made stage-wise, with the options of the family tests: all four tolerances
    1e-8, no hand-over of the tail (the whole solve stays on the family under test), iter_max 60"""
    from acados_amd import OcpQpGpuBatch
    r = FAMILIES[row]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    gb = OcpQpGpuBatch.from_qps(row_qps(row, N, B), _clib=clib)
    stagewise_perturb(gb, perturb_seed(row, N))
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, 1e-8)
    gb.opts_set("tail_max", 0)
    gb.opts_set("iter_max", iter_max)
    for k, v in r.get("opts", {}).items():
        gb.opts_set(k, v)
    return gb


def check_family(gb, row):
    """after a solve: the row ran on the family it names"""
    r = FAMILIES[row]
    assert gb.kernel_name.startswith(r["name"][0]) and all(s in gb.kernel_name for s in r["name"][1:]), (row, gb.kernel_name)
    for s, v in r.get("scalars", {}).items():
        assert int(gb.scalar(s)) == v, (row, s, gb.scalar(s))


def compared_lanes(B):
    """instances compared with the oracle: all of a batch of at most 8; of a larger one the lanes at the wave boundaries"""
    return list(range(B)) if B <= 8 else sorted({0, 1, 31, 62, 63, 64, B // 2, B - 2, B - 1} & set(range(B)))

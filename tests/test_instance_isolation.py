"""A failed instance must not disturb its neighbours.

The kernels put several independent QPs into one wave (64 on the one-instance-per-lane families, four 16-lane rows on the
sixteen-lanes families, four blocks per FP64 MFMA issue on the tile sweeps), and a wave keeps running while any of its
instances is alive.  Here batches are MIXED: instances whose data holds a NaN (ACADOS_NAN_DETECTED, 1) or whose bounds
cross (ACADOS_MAXITER 2 / ACADOS_MINSTEP 3) sit next to healthy ones, at every position of the sharing unit, and every
healthy instance has to come out BIT-IDENTICAL to the same batch without the poison ("the placement of an instance does not
enter its arithmetic") -- a NaN next to healthy data shows every mask-by-multiply, every reduction that drops or spreads a
NaN, every store that is not guarded.  Two healthy instances per row are also compared with the oracle, so that the two
device runs cannot be wrong in the same way.

Every test exists in both tiers: `hostsim` (kernel sources under g++, CPU) and `gpu` (the product library)."""
import numpy as np
import pytest

from conftest import compare_with_oracle
from oracle.oracle import OracleQp, default_opts

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
KKT_TOL = 2e-8       # the bar the suite uses for an independently recomputed residual of a solve at 1e-8
ITER_MAX = 30
INFOS = ("res_stat", "res_eq", "res_ineq", "res_comp", "mu")


@pytest.fixture
def clib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


# ---- the QPs of the table rows (host objects: what the oracle solves; built once per session) ------------------------------
_QPS = {}


def _lqr(nx, nu, N, B, seed):
    from acados_amd.generators import lqr_instance_qp, random_lqr_batch
    data = random_lqr_batch(N=N, nx=nx, nu=nu, batch=B, seed=seed)
    return [lqr_instance_qp(data, i, N) for i in range(B)]


def _chain(B, **kw):
    from acados_amd.generators import chain_soft_qp
    return [chain_soft_qp(i, N=4, **kw) for i in range(B)]


SOFT_SEED = 6    # a random structure without general rows that lands on w16-soft, with N >= 3 and input bounds after stage 0


def _soft(B):
    """one structure of test_sixteen_lanes_soft_box_rows_gpu, B copies with q / r perturbed per instance"""
    from random_qp import random_structure_qp
    g = np.random.default_rng(900 + SOFT_SEED)
    qps = []
    for _ in range(B):
        qp = random_structure_qp(SOFT_SEED, allow_general=False)
        for k in range(qp.N + 1):
            for f in ("q", "r"):
                v = np.asarray(getattr(qp, f)[k], dtype=float)
                if v.size:
                    qp.set(f, k, v * g.uniform(0.5, 1.5) + 0.1 * g.standard_normal(v.size))
        qp.make_consistent()
        qps.append(qp)
    return qps


def _qps(key):
    if key not in _QPS:
        _QPS[key] = {"lqr83/70": lambda: _lqr(8, 3, 4, 70, 31), "lqr41/70": lambda: _lqr(4, 1, 4, 70, 32),
                     "lqr83/14": lambda: _lqr(8, 3, 4, 14, 33), "lqr83/6": lambda: _lqr(8, 3, 4, 6, 34),
                     "lqr815/14": lambda: _lqr(8, 15, 4, 14, 35), "lqr144/6": lambda: _lqr(14, 4, 4, 6, 36),
                     "lqr83N10/9": lambda: _lqr(8, 3, 10, 9, 37),
                     "chain24/6": lambda: _chain(6), "chain24/10": lambda: _chain(10),
                     "chain8/10": lambda: _chain(10, nx=8, nu=3, ng=4, nsx=2), "soft/14": lambda: _soft(14)}[key]()
    return _QPS[key]


_ORACLE = {}


def _oracle(key, i, iter_max=ITER_MAX):
    """the oracle's solve of instance i of a clean batch, computed once"""
    if (key, i, iter_max) not in _ORACLE:
        o = OracleQp(_qps(key)[i])
        o.solve(default_opts(tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8, iter_max=iter_max))
        _ORACLE[(key, i, iter_max)] = o
    return _ORACLE[(key, i, iter_max)]


# ---- the family table ----------------------------------------------------------------------------------------------------------
# unit: instances that share a wave (64), a workgroup of four 16-lane rows (4); the wave-per-instance rows share nothing but the launch
W16 = {"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "1"}
ROWS = {
    "1tpi-box": dict(env={"ACADOS_AMD_WPI": "0"}, qps="lqr83/70", name=("1tpi-box<NX=8,NU=3",), unit=64),
    "1tpi-pipe": dict(env={"ACADOS_AMD_WPI": "0"}, qps="lqr41/70", name=("1tpi-pipe<NX=4,NU=1",), unit=64),
    "1tpi-gen": dict(env={"ACADOS_AMD_WPI": "0"}, qps="chain24/6", name=("1tpi<",), unit=64, gen=True),
    "w16-box/kx_solve": dict(env=W16, qps="lqr83/14", name=("w16-box<NX=8,NU=3>",), unit=4, scalars={"single_launch_solves": 1}),
    "w16-box/perm1": dict(env=dict(W16, ACADOS_AMD_W16_PERM="1"), opts={"solve_max": 0}, qps="lqr83/14", name=("w16-box<NX=8,NU=3>",),
                          unit=4, scalars={"single_launch_solves": 0}),
    "w16-box/perm0": dict(env=dict(W16, ACADOS_AMD_W16_PERM="0"), opts={"solve_max": 0}, qps="lqr83/14", name=("w16-box<NX=8,NU=3>",),
                          unit=4, scalars={"single_launch_solves": 0}),
    "w16-soft": dict(env=W16, qps="soft/14", name=("w16-soft<",), unit=4, soft=True),
    "w16r-box/tiles": dict(env=W16, qps="lqr815/14", name=("w16r-box<NX=8,NU=15>",), unit=4, scalars={"w16_tiles": 1}),
    "w16r-box/rows": dict(env=dict(W16, ACADOS_AMD_W16T="0"), qps="lqr815/14", name=("w16r-box<NX=8,NU=15>",), unit=4,
                          scalars={"w16_tiles": 0}),
    "w16r-gen8/tiles": dict(env=dict(W16, ACADOS_AMD_W16G="1"), qps="chain8/10", name=("w16r-gen<NX=8,NU=3,NG=4>",), unit=4, gen=True,
                            scalars={"w16_tiles": 1}),
    "w16r-gen8/rows": dict(env=dict(W16, ACADOS_AMD_W16G="1", ACADOS_AMD_W16T_GEN="0"), qps="chain8/10",
                           name=("w16r-gen<NX=8,NU=3,NG=4>",), unit=4, gen=True, scalars={"w16_tiles": 0}),
    "w16r-gen24/tiles": dict(env=dict(W16, ACADOS_AMD_W16G="1"), qps="chain24/10", name=("w16r-gen<NX=24,NU=3,NG=4>",), unit=4, gen=True,
                             scalars={"w16_tiles": 1}),
    "w16r-gen24/rows": dict(env=dict(W16, ACADOS_AMD_W16G="1", ACADOS_AMD_W16T_GEN="0"), qps="chain24/10",
                            name=("w16r-gen<NX=24,NU=3,NG=4>",), unit=4, gen=True, scalars={"w16_tiles": 0}),
    "wpi-box": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "0"}, qps="lqr83/6", name=("wpi-box(",), unit=1),
    "wpi-gen": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16G": "0"}, qps="chain24/6", name=("wpi-gen(",), unit=1, gen=True),
    # kw_factor_m, forced as test_mfma_blocked_cholesky_factor_kernel forces it, at the smallest shape of that test (nu + nx = 18)
    "wpi-mfma": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16R": "0", "ACADOS_AMD_WPI_MFMA": "1"}, qps="lqr144/6",
                     name=("wpi-box(nx=14,nu=4", "mfma"), unit=1),
    # ric_alg 0 on the w16-box row: the classical recursion lives on the wave-per-instance kernels
    "ric0": dict(env=W16, opts={"ric_alg": 0}, qps="lqr83/14", name=("wpi-box(", ",ric0"), unit=4),
    # partial condensing N = 10 -> two blocks of 5; B = 4 k + 1: km_pcond (3), kz_pcond (2), the run-time-shaped pair (0)
    "pcond3": dict(env={"ACADOS_AMD_WPI": "0"}, opts={"cond_N": 2}, qps="lqr83N10/9", name=("1tpi-box<NX=8,NU=3",), unit=4,
                   scalars={"pcond_kernel": 3}, pcond=True),
    "pcond2": dict(env={"ACADOS_AMD_WPI": "0", "ACADOS_AMD_PCOND_MFMA": "0"}, opts={"cond_N": 2}, qps="lqr83N10/9",
                   name=("1tpi-box<NX=8,NU=3",), unit=4, scalars={"pcond_kernel": 2}, pcond=True),
    "pcond0": dict(env={"ACADOS_AMD_WPI": "0", "ACADOS_AMD_PCOND_W16": "0", "ACADOS_AMD_PCOND_LANE_EXPAND": "0"}, opts={"cond_N": 2},
                   qps="lqr83N10/9", name=("1tpi-box<NX=8,NU=3",), unit=4, scalars={"pcond_kernel": 0}, pcond=True),
}

# poisoned instances by (unit, batch).  "ends": the first and the last instance of the batch are poisoned; sixteen-lanes rows: index
# mod 4 = 0, 1, 2, 3, one workgroup of four entirely dead, the one next to it entirely healthy; 64 per wave: lanes 0, 63, 64, the
# last instance, and one whole 16-lane group (16..31) / four consecutive lanes (40..43) dead; at least half of every batch healthy
LAYOUTS = {
    (4, 14): {"ends": [0, 2, 4, 5, 6, 7, 13], "inner": [1, 3, 8, 9, 10, 11, 12]},
    (4, 10): {"ends": [0, 1, 2, 3, 9], "inner": [4, 5, 6, 7, 8]},
    (4, 9): {"ends": [0, 2, 3, 8], "inner": [4, 5, 6, 7]},
    (64, 70): {"ends": [0, 63, 64, 69] + list(range(16, 32)), "inner": [1, 62, 65, 68, 40, 41, 42, 43]},
    (64, 6): {"ends": [0, 2, 5], "inner": [1, 3, 4]},
    (1, 6): {"ends": [0, 2, 5], "inner": [1, 3, 4]},
}


def _make(clib, monkeypatch, row, iter_max=ITER_MAX, tail_max=0):
    from acados_amd import OcpQpGpuBatch
    r = ROWS[row]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    gb = OcpQpGpuBatch.from_qps(_qps(r["qps"]), _clib=clib)
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, 1e-8)
    gb.opts_set("iter_max", iter_max)
    if tail_max is not None:
        gb.opts_set("tail_max", tail_max)       # no instance changes family mid-solve
    for k, v in r.get("opts", {}).items():
        gb.opts_set(k, v)
    return gb


def _check_family(gb, row):
    """after a solve: the row ran on the family it names"""
    r = ROWS[row]
    assert gb.kernel_name.startswith(r["name"][0]) and all(s in gb.kernel_name for s in r["name"][1:]), (row, gb.kernel_name)
    for s, v in r.get("scalars", {}).items():
        assert int(gb.scalar(s)) == v, (row, s, gb.scalar(s))


# ---- poison ----------------------------------------------------------------------------------------------------------------------
def _poison_plan(qp, gen, soft):
    """{kind: [(field, stage, element, value)]}: one NaN per kind, and the crossed input bounds.  Matrices are column-major in the
    blob: element n * n - 1 is the last diagonal entry.  Nothing touches q / Q of a state fixed by the x0 bound.  The sweeps order
    the variables of a stage [u; x]: on the two-rows shapes (nu + nx > 16) the last state -- Q's last diagonal entry -- lives in the
    second register row (index >= 16), R's last entry (variable nu - 1 <= 14) in the first."""
    d, N = qp.dims, qp.N
    nx, nu = [int(v) for v in d.nx], [int(v) for v in d.nu]
    ki = min(2, N - 1)                                            # an inner stage
    ku = max(k for k in range(N) if nu[k])                        # the last stage with inputs
    after0 = list(range(1, N)) + [0]                              # input bounds: after stage 0 where the structure has them there
    kb, rb = next((k, r) for k in after0 for r in reversed(range(int(d.nbu[k]))) if qp.lbu_mask[k][r] == 1.0)
    nan = np.nan

    def hard(k, r):    # an input bound with both sides present and no slack: crossing it leaves no feasible point
        rev = np.asarray(qp.idxs_rev[k]).astype(int)
        return qp.lbu_mask[k][r] == 1.0 and qp.ubu_mask[k][r] == 1.0 and (rev.size == 0 or rev[r] < 0)

    kc, rc = next((k, r) for k in after0 for r in range(int(d.nbu[k])) if hard(k, r))
    plan = {"A": [("A", ki, (nx[ki + 1] * nx[ki]) // 2, nan)],
            "B": [("B", 0, nx[1] * nu[0] - 1, nan)],
            "Q": [("Q", N, nx[N] * nx[N] - 1, nan)],
            "R": [("R", ku, nu[ku] * nu[ku] - 1, nan)],
            "b": [("b", 1 if N > 1 else 0, nx[2 if N > 1 else 1] - 1, nan)],
            "lbu": [("lbu", kb, rb, nan)],
            "infeasible": [("lbu", kc, rc, 5.0), ("ubu", kc, rc, -5.0)]}
    if gen:
        plan["C"] = [("C", 1, 1, nan)]
        plan["zl"] = [("zl", 2, int(d.ns[2]) - 1, nan)]
    if soft:
        ks = max(k for k in range(N + 1) if int(d.ns[k]))
        plan["zl"] = [("zl", ks, int(d.ns[ks]) - 1, nan)]
    return plan


def _assign(plan, idx, layout):
    """{instance: [kinds]}: the crossed bounds on one instance (inside the dead unit in "ends", outside in "inner"), the NaN kinds
    spread over the others -- one kind per instance where the batch has room, several where it has not (every kind is in the batch)"""
    nans = [k for k in plan if k != "infeasible"]
    rot = 0 if layout == "ends" else 3
    inf_at = idx[len(idx) // 2] if layout == "ends" else idx[0]
    rest = [i for i in idx if i != inf_at]
    out = {inf_at: ["infeasible"]}
    for j in range(max(len(nans), len(rest))):
        out.setdefault(rest[j % len(rest)], []).append(nans[(j + rot) % len(nans)])
    return out


def _poison(gb, plan, who):
    """through the input blob, so that one helper serves every structure"""
    blob = gb.get_bulk_in()
    for i, kinds in who.items():
        for kind in kinds:
            for f, k, e, v in plan[kind]:
                o, n = gb.bulk_offset(0, f, k)
                assert 0 <= e < n, (f, k, e, n)
                blob[i, o + e] = v
    gb.set_bulk(blob)
    back = gb.get_bulk_in()
    assert np.array_equal(np.isnan(back), np.isnan(blob)) and np.array_equal(np.nan_to_num(back), np.nan_to_num(blob))


# ---- what is compared --------------------------------------------------------------------------------------------------------------
def _snapshot(gb, ric=True):
    """everything a solve leaves behind, as host arrays"""
    d, N = gb.dims, gb.N
    out = {"status": gb.info("status").copy(), "iter": gb.info("iter").copy()}
    for f in INFOS:
        out[f] = gb.info(f).copy()
    for k in range(N + 1):
        fields = ["x", "u", "lam", "t"] + (["pi"] if k < N else []) + (["sl", "su"] if int(d.ns[k]) else []) + (["ric_L", "ric_l"] if ric else [])
        for f in fields:
            out[(f, k)] = gb.get(f, k)
    out["res_nrm"] = gb.res_compute()
    return out


def _assert_rows_identical(a, b, rows, what):
    for key in a:
        if key in ("status",):
            continue
        assert np.array_equal(a[key][rows], b[key][rows]), (what, key, [int(i) for i in rows if not np.array_equal(a[key][i], b[key][i])])


_TWIN = {}


def _twin(clib, monkeypatch, tier, row):
    """the clean twin of a row: same data, options and environment; solved once per tier"""
    if (tier, row) not in _TWIN:
        gb = _make(clib, monkeypatch, row)
        assert gb.solve() == 0, (row, gb.kernel_name, gb.info("status"))
        _check_family(gb, row)
        _TWIN[(tier, row)] = _snapshot(gb, ric=not ROWS[row].get("pcond"))
    return _TWIN[(tier, row)]


def _tier(request):
    return "gpu" if "gpu" in request.node.callspec.id.split("-") else "hostsim"


def _check_statuses(gb, snap, who):
    B = gb.n_batch
    st, it = snap["status"], snap["iter"]
    healthy = np.array([i for i in range(B) if i not in who])
    for i, kinds in who.items():
        if kinds == ["infeasible"]:
            assert st[i] in (2, 3) and it[i] <= ITER_MAX, (i, st[i], it[i])
        else:
            assert st[i] == 1, (i, kinds, st[i])          # ACADOS_NAN_DETECTED
            # ... and detected where the oracle detects it on the same data (read back from the batch): in the residual of the
            # initial iterate.  A reduction that drops the NaN of one lane finds it an iteration late, with status 1 all the same.
            o = OracleQp(gb.to_qp(i))
            assert o.solve(default_opts(tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8, iter_max=ITER_MAX)) == 1, (i, kinds)
            assert it[i] == o.iter == 0, (i, kinds, it[i], o.iter)
    assert np.all(st[healthy] == 0), (st, who)
    assert len(healthy) * 2 >= B
    return healthy


def _mixed(clib, monkeypatch, row, layout, tail_max=0):
    r = ROWS[row]
    qps = _qps(r["qps"])
    gb = _make(clib, monkeypatch, row, tail_max=tail_max)
    plan = _poison_plan(qps[0], r.get("gen", False), r.get("soft", False))
    who = _assign(plan, LAYOUTS[(r["unit"], len(qps))][layout], layout)
    assert set(k for v in who.values() for k in v) == set(plan)       # every kind is in the batch
    _poison(gb, plan, who)
    return gb, who


@pytest.mark.parametrize("clib", TIERS, indirect=True)
@pytest.mark.parametrize("layout", ["ends", "inner"])
@pytest.mark.parametrize("row", list(ROWS))
def test_failed_instances_leave_neighbours_bit_identical(clib, request, monkeypatch, row, layout):
    """every row of the family table, a batch with NaN in A, B, Q, R, b, lbu (C, zl where the structure has them) and one instance
    with crossed input bounds, next to its clean twin: solve() counts the poisoned instances, they report 1 / 2 or 3, every healthy
    instance reports 0 and equals the twin bit for bit (iterations, solution, multipliers, slacks, residual infos, the last factor),
    passes the independent residual kernel, and two of them agree with the oracle at 1e-8"""
    r = ROWS[row]
    twin = _twin(clib, monkeypatch, _tier(request), row)
    gb, who = _mixed(clib, monkeypatch, row, layout)
    assert gb.solve() == len(who), (row, gb.info("status"), who)
    _check_family(gb, row)
    snap = _snapshot(gb, ric=not r.get("pcond"))
    healthy = _check_statuses(gb, snap, who)
    _assert_rows_identical(twin, snap, healthy, row)
    nrm = snap["res_nrm"][healthy]
    assert np.all(np.isfinite(nrm)) and nrm.max() <= KKT_TOL, nrm
    qps = _qps(r["qps"])
    for i in (int(healthy[0]), int(healthy[-1])):
        o = _oracle(r["qps"], i)
        assert o.status == 0
        compare_with_oracle(lambda k, f: snap[(f, k)][i], o, qps[i], 1e-8)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_failed_instances_with_tail_hand_over(clib, monkeypatch):
    """1tpi-box with the hand-over of the tail on (default tail_max): the survivors of the mixed batch finish on another kernel
    family, so the healthy instances are compared with the oracle (1e-8) instead of bit-wise; statuses as above"""
    row = "1tpi-box"
    gb, who = _mixed(clib, monkeypatch, row, "ends", tail_max=None)
    assert gb.solve() == len(who)
    _check_family(gb, row)
    assert int(gb.scalar("tail_switches")) == 1
    snap = _snapshot(gb)
    healthy = _check_statuses(gb, snap, who)
    nrm = snap["res_nrm"][healthy]
    assert np.all(np.isfinite(nrm)) and nrm.max() <= KKT_TOL, nrm
    qps = _qps(ROWS[row]["qps"])
    for i in healthy:
        o = _oracle(ROWS[row]["qps"], int(i))
        assert o.status == 0
        compare_with_oracle(lambda k, f: snap[(f, k)][i], o, qps[i], 1e-8)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_tail_hand_over_from_the_general_rows_family(clib, monkeypatch):
    """1tpi-gen, clean data, six instances in one block of the root; tail_max 5, tail_div 1: as soon as one has converged the others
    go to the tail, at least two of them.  The general one-instance-per-lane finalize takes the multipliers of the fixed variables
    from the last factor sweep; for the instances that finished on the tail that sweep ran there, and the tail's own finalize -- one
    workgroup per instance with the tail's LDS, not the root's 64 instances per block -- computes them before the copy back.  Every
    instance passes the independent residual kernel and agrees with the oracle at 1e-8, multipliers included"""
    row = "1tpi-gen"
    gb = _make(clib, monkeypatch, row, tail_max=5)
    gb.opts_set("tail_div", 1)
    assert gb.solve() == 0
    _check_family(gb, row)
    assert int(gb.scalar("tail_switches")) == 1
    snap = _snapshot(gb)
    print("iterations", snap["iter"])
    assert np.all(snap["status"] == 0) and np.sum(snap["iter"] > snap["iter"].min()) >= 2      # two or more went to the tail
    nrm = snap["res_nrm"]
    assert np.all(np.isfinite(nrm)) and nrm.max() <= KKT_TOL, nrm
    qps = _qps(ROWS[row]["qps"])
    for i in range(len(qps)):
        o = _oracle(ROWS[row]["qps"], i)
        assert o.status == 0
        compare_with_oracle(lambda k, f: snap[(f, k)][i], o, qps[i], 1e-8)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
@pytest.mark.parametrize("row", list(ROWS))
def test_truncated_iterate_matches_oracle(clib, monkeypatch, row):
    """iter_max = 3 on clean data: every instance reports ACADOS_MAXITER (2) with iter == 3, and the iterate that comes back (x, u,
    pi, lam) is the oracle's iterate after the same three iterations, at the project's 1e-8.  The reference is the oracle alone.
    The partially condensed rows iterate on the CONDENSED QP -- another iteration than the full-space one (three iterations in: 3e-2
    apart) -- so there the oracle runs its three iterations on the condensed QP, the condensed iterate is compared at the same
    1e-8, and the expansion of that unfinished iterate is checked against the data: inputs and block-start states copied bit for
    bit, the states inside a block follow the dynamics (1e-12: rounding of four 11-term recursions on O(1) numbers).
    Measured worst deviation (printed per row), host simulation / MI355X:
      1tpi-box 4.4e-15 / 4.3e-15   1tpi-pipe 1.7e-14 / 2.0e-14   1tpi-gen 5.4e-14 / 3.5e-14   w16-box (all three) 3.7e-15 / 2.7e-15
      w16-soft 8.8e-16 / 9.1e-16   w16r-box tiles 2.9e-15 / 2.0e-15, rows 1.2e-15 / 1.3e-15   w16r-gen8 tiles 2.9e-13 / 3.8e-13, rows
      2.9e-13 / 2.9e-13   w16r-gen24 tiles 5.3e-14 / 3.2e-13, rows 2.1e-14 / 3.1e-13   wpi-box 1.9e-15 / 2.7e-15   wpi-gen 2.1e-14 /
      3.1e-14   wpi-mfma 3.5e-15 / 3.4e-15   ric0 2.9e-15 / 3.6e-15   pcond3 2.9e-15 / 3.2e-15   pcond2 5.1e-15 / 2.1e-15   pcond0
      3.6e-15 / 2.9e-15"""
    r = ROWS[row]
    qps = _qps(r["qps"])
    gb = _make(clib, monkeypatch, row, iter_max=3)
    assert gb.solve() == len(qps)
    _check_family(gb, row)
    assert np.all(gb.info("status") == 2) and np.all(gb.info("iter") == 3), (gb.info("status"), gb.info("iter"))
    worst = 0.0
    if r.get("pcond"):
        c = gb.condense()                       # the condensed data once more; the condensed iterate of the solve stays
        assert c is not None and c.N == 2
        csol = {(f, k): c.get(f, k) for k in range(c.N + 1) for f in ("x", "u", "lam") + (("pi",) if k < c.N else ())}
        for i in range(len(qps)):
            qc = c.to_qp(i)
            o = OracleQp(qc)
            assert o.solve(default_opts(tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8, iter_max=3)) == 2 and o.iter == 3
            worst = max(worst, compare_with_oracle(lambda k, f: csol[(f, k)][i], o, qc, np.inf, fields=("x", "u", "pi", "lam")))
        N, bs, nu = gb.N, gb.N // 2, int(qps[0].dims.nu[0])
        x, u = [gb.get("x", k) for k in range(N + 1)], [gb.get("u", k) for k in range(N)]
        for k in range(N + 1):
            j, s = min(k // bs, 2), k - min(k // bs, 2) * bs
            if s == 0:
                assert np.array_equal(x[k], csol[("x", j)]), k
            if k < N:
                assert np.array_equal(u[k], csol[("u", j)][:, s * nu:(s + 1) * nu]), k
            if s > 0:
                for i, qp in enumerate(qps):
                    want = np.asarray(qp.A[k - 1]) @ x[k - 1][i] + np.asarray(qp.B[k - 1]) @ u[k - 1][i] + np.asarray(qp.b[k - 1])
                    assert np.max(np.abs(x[k][i] - want) / np.maximum(1.0, np.abs(want))) <= 1e-12, (k, i)
    else:
        sol = {(f, k): gb.get(f, k) for k in range(gb.N + 1) for f in ("x", "u", "lam") + (("pi",) if k < gb.N else ())}
        for i, qp in enumerate(qps):
            o = _oracle(r["qps"], i, iter_max=3)
            assert o.status == 2 and o.iter == 3
            worst = max(worst, compare_with_oracle(lambda k, f: sol[(f, k)][i], o, qp, np.inf, fields=("x", "u", "pi", "lam")))
    print("truncated iterate, worst deviation from the oracle:", row, worst)
    assert worst <= 1e-8, (row, worst)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
@pytest.mark.parametrize("row", ["1tpi-box", "w16-box/kx_solve"])
def test_data_grad_downstream_of_failed_instances(clib, request, monkeypatch, row):
    """the reverse-mode gradient after a mixed solve (1tpi-box with the sliced adjoint): exact zero rows for the failed instances,
    finite rows for the healthy ones, bit-identical to the rows of the clean twin"""
    monkeypatch.setenv("ACADOS_AMD_SENS_SLICE", "2")
    clean = _make(clib, monkeypatch, row)
    assert clean.solve() == 0
    gb, who = _mixed(clib, monkeypatch, row, "ends")
    assert gb.solve() == len(who)
    _check_family(gb, row)
    cot = np.zeros((gb.n_batch, gb.bulk_len(1)))
    rng = np.random.default_rng(8)
    for k in range(gb.N + 1):
        for f in ("u", "x"):
            o, n = gb.bulk_offset(1, f, k)
            if n > 0:
                cot[:, o:o + n] = rng.standard_normal((gb.n_batch, n))
    g0, g1 = clean.data_grad(cot.copy()), gb.data_grad(cot.copy())
    bad = sorted(who)
    healthy = [i for i in range(gb.n_batch) if i not in who]
    assert np.all(g1[bad] == 0.0)
    assert np.all(np.isfinite(g1[healthy])) and np.all(np.any(g1[healthy] != 0.0, axis=1))
    assert np.array_equal(g0[healthy], g1[healthy])


@pytest.mark.parametrize("clib", TIERS, indirect=True)
@pytest.mark.parametrize("row", ["1tpi-box", "w16-box/kx_solve", "wpi-box", "pcond3"])
def test_nan_in_an_entry_the_solve_never_reads(clib, request, monkeypatch, row):
    """NaN in q of stage 0 at a state fixed by the equality-flagged x0 bound.  The un-condensed families never read that entry (the
    state is eliminated): status 0 and finite outputs, as the oracle returns -- while res_compute() returns NaN for that row,
    because the stationarity residual of stage 0 does read it.  With cond_N set the entry enters the condensed gradient: status 1.
    The healthy neighbours are bit-identical to the clean twin in both cases (status codes)."""
    r = ROWS[row]
    qps = _qps(r["qps"])
    twin = _twin(clib, monkeypatch, _tier(request), row)
    gb = _make(clib, monkeypatch, row)
    B = gb.n_batch
    bad = [1, B - 1]
    nx0 = int(qps[0].dims.nx[0])
    _poison(gb, {"q0": [("q", 0, nx0 - 1, np.nan)]}, {i: ["q0"] for i in bad})
    n_bad = gb.solve()
    _check_family(gb, row)
    snap = _snapshot(gb, ric=not r.get("pcond"))
    healthy = np.array([i for i in range(B) if i not in bad])
    assert np.all(snap["status"][healthy] == 0)
    _assert_rows_identical(twin, snap, healthy, row)
    assert np.all(np.isfinite(snap["res_nrm"][healthy])) and snap["res_nrm"][healthy].max() <= KKT_TOL
    if r.get("pcond"):
        assert n_bad == len(bad) and np.all(snap["status"][bad] == 1)
        return
    assert n_bad == 0 and np.all(snap["status"][bad] == 0)
    for key, v in snap.items():
        if key == "res_nrm":
            assert np.all(np.isnan(v[bad, 0]))                     # the residual kernel reads the entry
        else:
            assert np.all(np.isfinite(v[bad])), key
    # the oracle on the same poisoned QP: status 0, the same solution as without the NaN
    from acados_amd import OcpQpGpuBatch
    qp = OcpQpGpuBatch.from_qps([qps[1]], _clib=clib).to_qp(0)
    q0 = np.asarray(qp.q[0], dtype=float).copy()
    q0[nx0 - 1] = np.nan
    qp.set("q", 0, q0)
    o = OracleQp(qp)
    assert o.solve(default_opts(tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8, iter_max=ITER_MAX)) == 0
    assert all(np.all(np.isfinite(o.get(k, f))) for k in range(qp.N + 1) for f in ("x", "u", "lam", "t"))
    compare_with_oracle(lambda k, f: snap[(f, k)][1], o, qp, 1e-8)
    for k in range(qp.N + 1):
        for f in ("x", "u"):
            assert np.array_equal(snap[(f, k)][1], twin[(f, k)][1])   # the entry is not read at all


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_dense_list_with_a_partly_filled_last_workgroup(clib, monkeypatch):
    """w16-box at N = 2, batch 7 (the second workgroup carries three rows), launch per sweep.  Instances 1, 3 and 6 start close to the
    origin (x0 scaled by 1e-3: no input bound comes near) and converge first, so at least two have converged while another still
    iterates: the dense list of the live instances (ACADOS_AMD_W16_PERM, run_ipm) comes on and the grid of the sweeps shrinks.  Every
    output is bit for bit that of the solve without the list"""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch
    N, B = 2, 7
    data = random_lqr_batch(N=N, nx=8, nu=3, batch=B, seed=38)
    data["x0"][[1, 3, 6]] *= 1e-3
    for k, v in W16.items():
        monkeypatch.setenv(k, v)
    out = {}
    for perm in ("1", "0"):
        monkeypatch.setenv("ACADOS_AMD_W16_PERM", perm)
        gb = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, _clib=clib)
        fill_lqr_batch(gb, data, N)
        gb.opts_set("tol_stat", 1e-8)
        gb.opts_set("solve_max", 0)
        assert gb.solve() == 0
        assert gb.kernel_name.startswith("w16-box<NX=8,NU=3>") and int(gb.scalar("single_launch_solves")) == 0, gb.kernel_name
        out[perm] = {"iter": gb.info("iter").copy(), "status": gb.info("status").copy()}
        for k in range(N + 1):
            for f in ("x", "u", "pi", "lam", "t"):
                if not (f in ("u", "pi") and k == N):
                    out[perm][f, k] = np.array(gb.get(f, k), copy=True)
    it = np.sort(out["1"]["iter"])
    print("iterations", out["1"]["iter"])
    assert it[1] < it[-1]          # two have converged while one still iterates: 6 * nact <= 5 * 7, the list is on
    assert out["1"].keys() == out["0"].keys()
    for key in out["1"]:
        assert np.array_equal(out["1"][key], out["0"][key]), key

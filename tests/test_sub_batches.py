"""The sub-batches of a one-instance-per-lane batch: compaction level, tail, classical-Riccati child, sensitivity slices.

All four are made, loaded and stored by the same host code (gpu_batch.hip, sub_batch_create / _load / _store); the paths below are
the ones that code reshuffles and that no other test reaches: a tail that is re-used and has to grow, a tail made from a compaction
level, and every role on one object one after the other, with ric_alg and the stream priority changing in between.

Shape: nx = 8, nu = 3, N = 5, 130 instances (three tiles of 64, the last one partial) on the one-instance-per-lane box kernels: the
smallest batch in which a tail of up to 32 instances (a quarter of the level) and a half-batch compaction level both occur.  Data:
random box-constrained LQR instances (acados_amd/generators.py), two seeds picked under host simulation for their survivor counts
behind the factor sweep of iteration 5, 6, ...:
    SEED_A  130 122 85 42 13 3 0    tail_max 4: three instances go to the tail; compact_min 4: a level of 42, its tail takes 3
    SEED_B  130 122 75 31 12 2 0    tail_max 32: 31 instances go to the tail
Every test exists in both tiers: `hostsim` (kernel sources under g++, CPU) and `gpu` (the product library)."""
import numpy as np
import pytest

from conftest import compare_with_oracle
from oracle.oracle import OracleQp, default_opts

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
KKT_TOL = 2e-8       # the bar the suite uses for an independently recomputed residual of a solve at 1e-8
N, NX, NU, B = 5, 8, 3, 130
SEED_A, SEED_B = 1, 4
ITER_MAX = 30


@pytest.fixture
def clib(request, monkeypatch):
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")          # one instance per lane, whatever the batch size
    monkeypatch.setenv("ACADOS_AMD_SENS_SLICE", "50")  # 130 instances: three sensitivity slices, the last one short
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


_DATA = {}


def _data(seed):
    from acados_amd.generators import random_lqr_batch
    if seed not in _DATA:
        _DATA[seed] = random_lqr_batch(N=N, nx=NX, nu=NU, batch=B, seed=seed)
    return _DATA[seed]


def _make(clib, seed, **opts):
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims
    gb = OcpQpGpuBatch(lqr_dims(N, NX, NU), B, _clib=clib)
    fill_lqr_batch(gb, _data(seed), N)
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, 1e-8)
    gb.opts_set("iter_max", ITER_MAX)
    for k, v in opts.items():
        gb.opts_set(k, v)
    return gb


def _solve(gb):
    """a solve and everything it leaves behind: the output blob, iteration counts, statuses, the statistics tables"""
    bad = gb.solve()
    assert gb.kernel_name.startswith("1tpi-box<NX=8,NU=3" if gb.ric_alg else "wpi-box(nx=8,nu=3"), gb.kernel_name
    return {"bad": bad, "blob": gb.get_bulk(), "iter": gb.info("iter").copy(), "status": gb.info("status").copy(),
            "stat": np.stack([gb.stat(i, ITER_MAX + 2) for i in range(64)])}


def _assert_same_solve(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key]), (what, key)


def _sens(gb):
    """one seed set (q, r, b and the input bounds at every stage) and the directions sens_solve leaves"""
    rng = np.random.default_rng(77)
    for k in range(N + 1):
        gb.sens_set("seed_q", k, rng.standard_normal((B, NX)))
        if k < N:
            gb.sens_set("seed_r", k, rng.standard_normal((B, NU)))
            gb.sens_set("seed_b", k, rng.standard_normal((B, NX)))
            gb.sens_set("seed_lbu", k, rng.standard_normal((B, NU)))
            gb.sens_set("seed_ubu", k, rng.standard_normal((B, NU)))
    gb.sens_solve()
    out = {}
    for k in range(N + 1):
        for f in ("sens_x", "sens_lam", "sens_t") + (("sens_u", "sens_pi") if k < N else ()):
            out[(f, k)] = gb.get(f, k)
            assert np.all(np.isfinite(out[(f, k)])), (f, k)
    assert any(np.any(v != 0.0) for v in out.values())
    return out


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_reused_tail_grows(clib):
    """The first solve (tail_max 4) hands three instances to the tail, which is made for four.  New data through the bulk setter,
    tail_max 32, the same object again: 31 instances go, the tail has to be made anew.  Both solves switch once and end with every
    status 0, and the second one leaves, bit for bit, what a fresh batch with the same data and options leaves: output blob,
    iteration counts, statistics tables (the tail's rows are merged into the root's table: a tail that still had its four
    statistics slots would leave holes there).
    Mutation (host simulation only -- on a device it writes behind an allocation as soon as a tail is handed more than its padded
    capacity): with the re-creation branch of compact_into removed this test fails on the statistics tables."""
    fresh = _make(clib, SEED_B, tail_max=32)
    want = _solve(fresh)
    assert want["bad"] == 0 and int(fresh.scalar("tail_switches")) == 1
    gb = _make(clib, SEED_A, tail_max=4)
    first = _solve(gb)
    assert first["bad"] == 0 and np.all(first["status"] == 0) and int(gb.scalar("tail_switches")) == 1
    gb.set_bulk(fresh.get_bulk_in())
    gb.opts_set("tail_max", 32)
    second = _solve(gb)
    assert second["bad"] == 0 and np.all(second["status"] == 0) and int(gb.scalar("tail_switches")) == 1
    _assert_same_solve(want, second, "re-used tail")


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_tail_below_a_compaction_level(clib):
    """compact_min 4 with the default tail: the root compacts its survivors into a level and that level, not the root, hands its
    last ones to a tail.  Every instance ends with status 0, passes the independent residual kernel and agrees with the oracle at
    1e-8.  The statistics table has no iteration column: row r IS iteration r, and k_stat_merge puts the rows of a sub-level at
    the offset of the iteration it was entered at.  So for every instance with a table (the first 64): rows 0 .. iter are all
    there (mu > 0), the rows from 1 on carry the step lengths of the iteration before, the last row passes the exit test, and
    nothing stands behind it -- a merge at a wrong offset leaves a hole or a row too many."""
    from acados_amd.generators import lqr_instance_qp
    gb = _make(clib, SEED_A, compact_min=4)
    got = _solve(gb)
    assert int(gb.scalar("compactions")) >= 1 and int(gb.scalar("tail_switches")) == 1
    assert got["bad"] == 0 and np.all(got["status"] == 0)
    nrm = gb.res_compute()
    assert np.all(np.isfinite(nrm)) and nrm.max() <= KKT_TOL, nrm.max()
    sol = {(f, k): gb.get(f, k) for k in range(N + 1) for f in ("x", "u", "lam") + (("pi",) if k < N else ())}
    for i in range(B):
        qp = lqr_instance_qp(_data(SEED_A), i, N)
        o = OracleQp(qp)
        assert o.solve(default_opts(tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8, iter_max=ITER_MAX)) == 0
        compare_with_oracle(lambda k, f: sol[(f, k)][i], o, qp, 1e-8, fields=("x", "u", "pi", "lam"))
    it = got["iter"]
    assert it[:64].max() > it[:64].min()          # instances of the table finish on the root, on the level and on the tail
    for i in range(64):
        st, n = got["stat"][i], int(it[i])
        assert np.all(st[:n + 1, 6] > 0.0), (i, n, st[:, 6])
        assert np.all(st[1:n + 1, 0] > 0.0) and np.all(st[1:n + 1, 4] > 0.0), (i, n, st[:, 0], st[:, 4])
        assert np.all(st[n, 7:11] <= 1e-8), (i, n, st[n, 7:11])
        assert np.all(st[n + 1:] == 0.0), (i, n)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_every_role_on_one_object(clib):
    """One object: a solve with ric_alg 1 (tail), sens_solve in three slices, ric_alg 0 with a solve (classical-Riccati child) and
    sens_solve (slices in the classical layout), back to ric_alg 1 and a solve.  Each step leaves, bit for bit, what a fresh
    object leaves that does only that step.  Then stream_priority -1 and one more ric_alg 0 solve: the result does not move.  So
    a change of ric_alg drops the sub-batches of the old kernel set and the next use builds the right ones, and a new stream
    priority reaches all of them."""
    want = {}
    for ric in (1, 0):
        fresh = _make(clib, SEED_A, ric_alg=ric)
        want[("solve", ric)] = _solve(fresh)
        assert want[("solve", ric)]["bad"] == 0
        assert int(fresh.scalar("tail_switches")) == ric      # ric_alg 0: the whole solve runs one wave per instance
        want[("sens", ric)] = _sens(fresh)
    gb = _make(clib, SEED_A)
    for ric in (1, 0):
        gb.opts_set("ric_alg", ric)
        _assert_same_solve(want[("solve", ric)], _solve(gb), ("solve", ric))
        got = _sens(gb)
        for key, v in want[("sens", ric)].items():
            assert np.array_equal(v, got[key]), ("sens", ric, key)
    gb.opts_set("ric_alg", 1)
    _assert_same_solve(want[("solve", 1)], _solve(gb), "back to ric_alg 1")
    gb.opts_set("ric_alg", 0)
    _assert_same_solve(want[("solve", 0)], _solve(gb), "ric_alg 0 again")
    gb.opts_set("stream_priority", -1)
    _assert_same_solve(want[("solve", 0)], _solve(gb), "ric_alg 0 after stream_priority -1")


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_compaction_level_of_a_two_activity_word_batch(clib):
    """nx = 30, nu = 3: stage 0 has 2 (30 + 3) = 66 inequality sides, more than one activity word holds, so the batch runs one wave
    per instance with two words per stage (kernel wpi-box(nx=30,nu=3,lds=19560B)).  Eight instances, N = 3; x0 of instances 1, 3
    and 6 is scaled by 1e-3, so they finish early and, with compact_min 2, the survivors go on in a compaction level.  That level
    takes the family of its parent whole (gpu_batch.hip, sub_batch_create), the two activity words included: the solve returns 0
    failures with at least one compaction, and iterate, iteration counts and statuses are, bit for bit, those of the same batch
    solved without compaction.
    Mutation: where the level's family is chosen anew from its dims instead (the parent commit of choose_family), no kernel set
    serves it -- "cannot create the compaction sub-batch", solve() returns -1 and three instances are left at status -2."""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch
    n, nx, nu, batch = 3, 30, 3, 8
    data = random_lqr_batch(N=n, nx=nx, nu=nu, batch=batch, seed=5)
    data["x0"][[1, 3, 6]] *= 1e-3
    runs = []
    for compact_min in (1 << 30, 2):
        gb = OcpQpGpuBatch(lqr_dims(n, nx, nu), batch, _clib=clib)
        fill_lqr_batch(gb, data, n)
        gb.opts_set("tol_stat", 1e-8)
        gb.opts_set("compact_min", compact_min)
        gb.opts_set("tail_max", 0)
        bad = gb.solve()
        assert gb.kernel_name == "wpi-box(nx=30,nu=3,lds=19560B)", gb.kernel_name
        assert bad == 0, (compact_min, bad, gb.info("status"))
        runs.append({"blob": gb.get_bulk(), "iter": gb.info("iter").copy(), "status": gb.info("status").copy(),
                     "compactions": int(gb.scalar("compactions"))})
    plain, compacted = runs
    assert plain["compactions"] == 0 and compacted["compactions"] >= 1
    assert len(set(plain["iter"].tolist())) >= 2, plain["iter"]      # instances really finish at different iterations
    for key in ("blob", "iter", "status"):
        assert np.array_equal(plain[key], compacted[key]), key

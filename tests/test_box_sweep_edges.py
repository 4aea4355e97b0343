"""Both tiers: the one-instance-per-lane box sweeps (ipm_kernels_box.hpp) at the places where a peeled stage 0 or a fetch
that runs a stage ahead goes wrong first -- horizons of one, two and three stages, batches of one, one short of a wave,
one beyond a wave and several waves with a ragged last one, the redo pair of the conditional corrector, and finished
lanes riding along beside lanes that still iterate.

Every stage carries data of its own (the generator repeats one block over the horizon, and a sweep that read a
neighbouring stage's block would not be noticed on that).  Each instance is compared with the oracle at 1e-8
(tests/conftest.py compare_with_oracle: x, u, pi, lam, all four tolerances 1e-8) and must take exactly the oracle's number
of iterations; the whole solve stays on the family under test (ACADOS_AMD_WPI=0, no hand-over of the tail)."""
import numpy as np
import pytest

from conftest import compare_with_oracle, has_gpu
from oracle.oracle import OracleQp, default_opts

NX, NU = 8, 3


def _stagewise_batch(clib, N, B, seed, x0_scale=None, cost_scale=None):
    """C2-shaped batch (acados_amd.generators.random_lqr_batch) whose stages differ: dynamics, cost and input bounds of
    every stage perturbed by factors of their own; x0_scale / cost_scale: per-instance factors on x0 and on (q, r)"""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch
    data = random_lqr_batch(N=N, nx=NX, nu=NU, batch=B, seed=seed)
    if x0_scale is not None:
        data["x0"] = data["x0"] * np.asarray(x0_scale)[:, None]
    gb = OcpQpGpuBatch(lqr_dims(N, NX, NU), B, _clib=clib)
    fill_lqr_batch(gb, data, N)
    g = np.random.default_rng(seed + 5000)
    cs = np.ones((B, 1)) if cost_scale is None else np.asarray(cost_scale, dtype=float)[:, None]
    for k in range(N + 1):
        fields = [("Q", "pos"), ("q", "lin")] + ([("R", "pos"), ("S", "any"), ("r", "lin"), ("A", "any"), ("B", "any"), ("b", "any"),
                                                 ("lbu", "bnd"), ("ubu", "bnd")] if k < N else [])
        w = 1.0 + 0.3 * g.uniform()          # one width for both input bounds of the stage: lbu < 0 < ubu stays
        for f, kind in fields:
            v = gb.get(f, k)
            if kind == "pos":                # a positive factor keeps the block positive definite
                v = v * (1.0 + 0.5 * g.uniform())
            elif kind == "bnd":
                v = v * w
            elif kind == "lin":
                v = (v + 0.05 * g.standard_normal((1, v.shape[1]))) * cs
            else:
                v = v * (1.0 + 0.05 * g.standard_normal((1, v.shape[1])))
            gb.set(f, k, v)
    return gb


def _solve_and_check(gb, which, tol=1e-8, **opts):
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, 1e-8)
    gb.opts_set("tail_max", 0)               # the whole solve on the family under test
    for f, v in opts.items():
        gb.opts_set(f, v)
    bad = gb.solve()
    assert gb.kernel_name.startswith("1tpi-box"), gb.kernel_name
    assert bad == 0, (gb.info("status"), gb.info("iter"))
    it = gb.info("iter")
    worst = 0.0
    for i in which:
        qp = gb.to_qp(i)
        o = OracleQp(qp)
        assert o.solve(default_opts(tol_stat=1e-8, **{k: v for k, v in opts.items() if k == "iter_max"})) == 0, i
        print(f"instance {i}: iterations {int(it[i])} (oracle {o.iter})", end="")
        e = compare_with_oracle(lambda k, f: gb.get(f, k)[i], o, qp, tol, fields=("x", "u", "pi", "lam"))
        print(f", worst deviation {e:.2e}")
        assert int(it[i]) == o.iter, (i, int(it[i]), o.iter)
        worst = max(worst, e)
    return it, worst


CASES = [(N, B) for N in (1, 2, 3, 50) for B in (1, 63, 65, 200)]


def _which(B, full):
    """instances compared with the oracle: all of a small batch; of a larger one the lanes at the wave boundaries"""
    return list(range(B)) if full or B <= 8 else sorted({0, 1, 31, 62, 63, 64, B // 2, B - 2, B - 1} & set(range(B)))


def _horizon_and_batch_edges(clib, N, B):
    gb = _stagewise_batch(clib, N, B, seed=100 * N + B)
    _solve_and_check(gb, _which(B, full=False))


def _redo_pair(clib):
    """The conditional corrector (cond_pred_corr, tests/conftest.py limit_cycle_case is the model): an instance whose
    corrector step would more than double the duality measure is flagged and the redo pair -- kb_backrhs and
    kb_forward<CORR> with redo = 1, only the flagged lanes take part -- computes a centering-only step for it.  Costs scaled far
    apart within the batch make some instances take that path: switching the conditional corrector off changes their
    iterates (asserted: the pair really ran), and with it on every instance agrees with the oracle."""
    B, N = 24, 6
    g = np.random.default_rng(77)
    cost = g.uniform(-2.0, 3.0, B) * 10.0 ** g.uniform(0.0, 2.0, B)
    runs = []
    for cpc in (1, 0):
        gb = _stagewise_batch(clib, N, B, seed=31, cost_scale=cost)
        for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
            gb.opts_set(f, 1e-8)
        gb.opts_set("tail_max", 0)
        gb.opts_set("cond_pred_corr", cpc)
        gb.solve()
        runs.append(gb)
    on, off = runs
    took = [i for i in range(B) if int(on.info("iter")[i]) != int(off.info("iter")[i])
            or not np.array_equal(on.get("u", 0)[i], off.get("u", 0)[i])]
    print("instances whose solve changes with the conditional corrector:", took)
    assert took, "no instance took the redo pair"
    _solve_and_check(_stagewise_batch(clib, N, B, seed=31, cost_scale=cost), list(range(B)))


def _finished_lanes_ride_along(clib):
    """easy instances (x0 near the origin: no bound becomes active, a handful of iterations) and hard ones (x0 far out) side by
    side in every wave: the easy lanes finish early and ride along through every sweep of the hard ones"""
    B, N = 70, 12
    scale = np.where(np.arange(B) % 3 == 0, 0.02, 1.6)
    gb = _stagewise_batch(clib, N, B, seed=9, x0_scale=scale)
    it, _ = _solve_and_check(gb, _which(B, full=True))
    easy, hard = it[np.arange(B) % 3 == 0], it[np.arange(B) % 3 != 0]
    print("iterations easy", sorted(set(easy.tolist())), "hard", sorted(set(hard.tolist())))
    assert easy.max() < hard.max() and len(set(it[:64].tolist())) >= 3, it


# ---------------------------------------------------------------- host simulation

@pytest.fixture
def one_per_lane(monkeypatch):
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")


@pytest.mark.parametrize("N,B", CASES)
def test_horizon_and_batch_edges_hostsim(hostsim_lib, one_per_lane, N, B):
    _horizon_and_batch_edges(hostsim_lib, N, B)


def test_redo_pair_hostsim(hostsim_lib, one_per_lane):
    _redo_pair(hostsim_lib)


def test_finished_lanes_ride_along_hostsim(hostsim_lib, one_per_lane):
    _finished_lanes_ride_along(hostsim_lib)


# ---------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("N,B", CASES)
def test_horizon_and_batch_edges_gpu(gpu_lib, one_per_lane, N, B):
    _horizon_and_batch_edges(None, N, B)


@pytest.mark.gpu
def test_redo_pair_gpu(gpu_lib, one_per_lane):
    _redo_pair(None)


@pytest.mark.gpu
def test_finished_lanes_ride_along_gpu(gpu_lib, one_per_lane):
    _finished_lanes_ride_along(None)

"""What tests/test_full_dense.py shares: the rows of the dense full-condensing path (kd_solve, dense_kernels.hpp), their batches with
data of their own at every stage, the references of an instance's read-back QP (each computed once per data) and the comparison
with them.  None of the references is the code under test: dense_ref.solve_exact (a dense active-set solve with its own certificate),
the oracle (a stage-wise Riccati IPM on the original QP), dense_ref.kkt_residual_norms.
A plain module like stagewise_common.py."""
import numpy as np

from stagewise_common import GENERATORS, SEEDS, compared_lanes, instance_noise, stagewise_perturb, structure_cases

# the settings of the certified tests (conftest.certified_random_structures_case)
TIGHT = dict(tol_stat=1e-9, tol_eq=1e-11, tol_ineq=1e-11, tol_comp=1e-12)
ITER_MAX = 100
ITER_CAP = 40          # the dense path holds the dynamics exactly and follows other iterates than the oracle: counts are not compared
PRIMAL_BAR = 1e-9      # the project's bar against a certified solution, relative to max(1, |ref|)
# multipliers: how far an interior point at TIGHT sits from the vertex's multipliers, measured reference against reference (the
# oracle at TIGHT against the oracle at tol_comp 1e-13 on the QPs of case (a): test_multiplier_bar_source); the bar is 64 times that
MULT_MEASURED = 4.2e-9
MULT_BAR = 64 * MULT_MEASURED

HORIZONS = (1, 2, 3, 9)
LQR_ROWS = ("lqr41", "lqr41x", "lqr83", "lqr815")
# hard random structures (tests/random_qp.py, allow_slack=False), seeds from a search on the generator alone (asserted in
# test_hard_structure_seeds): "hard-x0" the first seed holding exactly {general, one-sided, x0}; "hard-free" the first seed with a free
# x0, general and one-sided rows and, from N = 3 on, a state dimension that switches mid-horizon
HARD_SEEDS = {"hard-x0": {1: 3, 2: 1, 3: 1, 9: 0}, "hard-free": {1: 2, 2: 0, 3: 0, 9: 9}}
ROWS = LQR_ROWS + tuple(HARD_SEEDS)


def hard_qp(seed, N):
    from random_qp import random_structure_qp
    return random_structure_qp(seed, N=N, allow_slack=False)


def hard_seed_search(row, N):
    """the first seed from 0 that holds what the row asks for"""
    for s in range(1000):
        qp = hard_qp(s, N)
        cases = structure_cases(qp)
        if row == "hard-x0" and cases == {"general", "one-sided", "x0"}:
            return s
        if row == "hard-free" and cases == {"general", "one-sided"} and (N < 3 or len(set(int(v) for v in qp.dims.nx)) > 1):
            return s
    raise AssertionError((row, N))


def row_qps(row, N, B):
    if row in HARD_SEEDS:
        return [hard_qp(HARD_SEEDS[row][N], N)] * B
    return GENERATORS[row](N, B, SEEDS[row].get(N, 1))


def tight(gb, iter_max=ITER_MAX):
    for f, v in TIGHT.items():
        gb.opts_set(f, v)
    gb.opts_set("iter_max", iter_max)


def layout_env(monkeypatch, tiled):
    """tiled: the wave-tiled HBM layout of the one-instance-per-lane families; else the instance-major one"""
    monkeypatch.setenv("ACADOS_AMD_WPI", "0" if tiled else "1")


def check_layout(gb, tiled):
    assert gb.kernel_name.startswith("1tpi") == bool(tiled), gb.kernel_name


def dense_batch(clib, monkeypatch, row, N, B, tiled=False, qps=None, dense=True):
    """the row's batch of B instances over N stages with data of its own at every stage (a hard structure: its instances made
    different), TIGHT, iter_max 100, on the dense path.  Batches of one (row, N) are prefixes of one another.  Returns (gb, input blob)"""
    from acados_amd import OcpQpGpuBatch
    layout_env(monkeypatch, tiled)
    gb = OcpQpGpuBatch.from_qps(row_qps(row, N, B) if qps is None else qps, _clib=clib)
    if qps is None:
        if row in HARD_SEEDS:
            instance_noise(gb, 8000 + N)
        else:
            stagewise_perturb(gb, 7000 + 100 * SEEDS[row].get(N, 1) + N)
    tight(gb)
    gb.opts_set("full_dense", 1 if dense else 0)
    return gb, gb.get_bulk_in()


# ---- references, once per data ----------------------------------------------------------------------------------------------------
_REF = {}


def references(gb, blob, i, qp=None):
    """(qp, certified primal solution {field: [per stage]}, oracle at TIGHT) of instance i's read-back QP"""
    from dense_ref import solve_exact, split
    from oracle.oracle import OracleQp, default_opts
    key = (gb.dims.signature(), tuple(tuple(int(e) for e in gb.get_int("idxe", k)) if int(gb._nbxe[k]) else () for k in range(gb.N + 1)),
           blob[i].tobytes())
    if key not in _REF:
        qp = gb.to_qp(i) if qp is None else qp
        w, off, info = solve_exact(qp)
        assert info["cert"] <= 1e-10 and info["stationarity"] <= 1e-9, info
        o = OracleQp(qp)
        assert o.solve(default_opts(iter_max=ITER_MAX, **TIGHT)) == 0, (o.status, o.iter)
        _REF[key] = (qp, split(qp, w, off), o)
    return _REF[key]


def rel(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if ref.size else 0.0


def multiplier_views(qp, k, lam):
    """lam of stage k as it is compared: the sides of rows that are not equality-flagged as they are, the flagged rows by the
    difference upper - lower (the one number stationarity determines), and stage 0 folded as the reference's getters fold it
    (conftest.fold_stage0)"""
    from conftest import fold_stage0
    d = qp.dims
    nbg = int(d.nb[k] + d.ng[k])
    eq = np.zeros(nbg, dtype=bool)
    eq[[int(e) for e in qp.idxe[k]]] = True
    lo, up = lam[:nbg], lam[nbg:2 * nbg]
    out = [lo[~eq], up[~eq], (up - lo)[eq]]
    if k == 0:
        out.append(fold_stage0(lam, nbg))
    return np.concatenate(out)


def slacks_view(qp, k, t):
    """t of stage k on the rows that are not equality-flagged (a flagged row takes no part: it has no slack)"""
    nbg = int(qp.dims.nb[k] + qp.dims.ng[k])
    eq = np.zeros(nbg, dtype=bool)
    eq[[int(e) for e in qp.idxe[k]]] = True
    return np.concatenate([t[:nbg][~eq], t[nbg:2 * nbg][~eq]])


def compare_instance(gb, sol, i, qp, exact, o, worst):
    """instance i of a dense solve against its references; sol: {(field, stage): [B, n]}; worst: {reference: deviation}, updated"""
    from dense_ref import kkt_residual_norms
    N = qp.N
    for k in range(N + 1):
        for f in ("u", "x"):
            e = rel(sol[(f, k)][i][:exact[f][k].size], exact[f][k])
            assert e <= PRIMAL_BAR, ("solve_exact", i, k, f, e)
            worst["solve_exact"] = max(worst.get("solve_exact", 0.0), e)
        e = rel(slacks_view(qp, k, sol[("t", k)][i]), slacks_view(qp, k, o.get(k, "t")))
        assert e <= PRIMAL_BAR, ("oracle", i, k, "t", e)
        worst["oracle t"] = max(worst.get("oracle t", 0.0), e)
        e = rel(multiplier_views(qp, k, sol[("lam", k)][i]), multiplier_views(qp, k, o.get(k, "lam")))
        assert e <= MULT_BAR, ("oracle", i, k, "lam", e, sol[("lam", k)][i], o.get(k, "lam"))
        worst["oracle lam"] = max(worst.get("oracle lam", 0.0), e)
        if k < N:
            e = rel(sol[("pi", k)][i], o.get(k, "pi"))
            assert e <= MULT_BAR, ("oracle", i, k, "pi", e)
            worst["oracle pi"] = max(worst.get("oracle pi", 0.0), e)
    nrm = kkt_residual_norms(qp, lambda k, f: sol[(f, k)][i] if not (f == "pi" and k == N) else np.zeros(0))
    for j, f in enumerate(TIGHT):
        assert nrm[j] <= TIGHT[f] * (1.0 + 1e-3) + 1e-12, ("kkt_residual_norms", i, f, nrm)
        worst["kkt " + f] = max(worst.get("kkt " + f, 0.0), float(nrm[j]))


def solution(gb):
    N = gb.N
    fields = ("u", "x", "sl", "su", "pi", "lam", "t")
    return {(f, k): gb.get(f, k) for k in range(N + 1) for f in fields if not (f == "pi" and k == N)}


def check_dense_solve(gb, blob, lanes=None, qps=None, iter_cap=ITER_CAP):
    """after solve() on the dense path: status 0 and at most iter_cap iterations on EVERY instance, the four norms of the independent
    residual kernel each below its own tolerance, and the instances `lanes` (default: compared_lanes) against their references.
    Returns {reference: worst deviation}"""
    st, it = gb.info("status"), gb.info("iter")
    assert np.all(st == 0), st
    assert np.all(it <= iter_cap) and np.all(it >= 1), it
    nrm = gb.res_compute()
    for j, f in enumerate(TIGHT):
        assert np.all(nrm[:, j] <= TIGHT[f] * (1.0 + 1e-3) + 1e-12), ("res_compute", f, nrm[:, j].max())
    sol = solution(gb)
    worst = {"res_compute " + f: float(nrm[:, j].max()) for j, f in enumerate(TIGHT)}
    for i in (compared_lanes(gb.n_batch) if lanes is None else lanes):
        qp, exact, o = references(gb, blob, i, None if qps is None else qps[i])
        compare_instance(gb, sol, i, qp, exact, o, worst)
    return worst


def results(gb):
    """everything a solve leaves per instance: output blob, iter, status, the four residual norms, mu"""
    return (gb.get_bulk(),) + tuple(gb.info(f).copy() for f in ("iter", "status", "res_stat", "res_eq", "res_ineq", "res_comp", "mu"))


def assert_same_results(a, b, rows=None, what=""):
    for j, (x, y) in enumerate(zip(a, b)):
        if rows is not None:
            x, y = x[rows], y[rows]
        assert np.array_equal(x, y), (what, j)

"""The dense full-condensing path (option full_dense: kd_solve of dense_kernels.hpp through dense_solve of gpu_batch.hip) on every
edge: data of its own at every stage, short horizons, both HBM layouts with ragged tiles, loops that wrap over the dense columns
and the rows, slices of the batch, NaN isolation and truncation, fixed inputs, the initialisations, the refusals, and what follows
a dense solve (sensitivities, data gradients, Riccati getters, a stage-wise solve of the same batch).

References, none of them the code under test (tests/dense_common.py): dense_ref.solve_exact on the instance's read-back QP with its
certificate asserted (primal u x at 1e-9 relative to max(1, |ref|)); the oracle at the same tolerances (pi, lam, t); the four norms of
res_compute() and of dense_ref.kkt_residual_norms, each against its own tolerance x (1 + 1e-3) + 1e-12; dense_ref.sens_dense; dense_grad
of test_data_grad.py.  Tolerances of the comparison cases: tol_stat 1e-9, tol_eq 1e-11, tol_ineq 1e-11, tol_comp 1e-12, iter_max 100.
Iteration counts are not compared with the oracle's (the dense path holds the dynamics exactly and follows other iterates): at most 40.

The multiplier bar is measured reference against reference (test_multiplier_bar_source): the worst relative deviation of the oracle's
pi / lam at these tolerances from the oracle's own at tol_comp 1e-13 on the compared QPs of case (a) is 4.1e-9 (MULT_MEASURED = 4.2e-9),
which is how far an interior point at this tolerance sits from the vertex's multipliers; the bar is 64 times that, 2.7e-7.

Measured worst deviations, host simulation / MI355X: solve_exact 2.4e-10 / 3.4e-10; oracle t 2.7e-10 / 3.3e-10, lam 6.7e-10 / 1.5e-9,
pi 5.6e-10 / 1.4e-9; stationarity by res_compute() 9.3e-10 / 9.6e-10 (profiles/NOTES.md holds the rest and the mutation check).

Every test exists in both tiers: `hostsim` (kernel sources under g++, CPU) and `gpu` (the product library); cases that cost more than
a few seconds under the host simulation run on the device only."""
import numpy as np
import pytest

import dense_common as dc
from dense_common import (HARD_SEEDS, HORIZONS, ITER_MAX, MULT_BAR, MULT_MEASURED, ROWS, TIGHT, assert_same_results, check_dense_solve,
                          check_layout, dense_batch, results)
from stagewise_common import TIERS, compared_lanes

HOST, GPU = TIERS


@pytest.fixture
def clib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


def _params(cases):
    """cases: (host, id, values...) -> pytest params, the clib first; host: the case also runs under the host simulation"""
    out = []
    for host, cid, *vals in cases:
        for t in ([HOST] if host else []) + [GPU]:
            out.append(pytest.param(t.values[0], *vals, id=f"{cid}-{t.id}", marks=t.marks))
    return out


def _check_columns(gb, row):
    """(N + 1) NU + NX dense columns, NU and NX the dims the kernel family pads every stage to: the stage dims themselves on the
    LQR rows, at least the largest stage on a structure with dims of its own per stage"""
    d = gb.dims
    least, cols = (gb.N + 1) * int(max(d.nu)) + int(max(d.nx)), int(gb.scalar("dense_columns"))
    assert cols == least if row in dc.LQR_ROWS else cols >= least, (cols, least)


def _fmt(worst):
    return {k: f"{v:.1e}" for k, v in worst.items()}


# ---- where the seeds and the multiplier bar come from (no kernel takes part) ----------------------------------------------------------
def test_hard_structure_seeds():
    """the seeds of the two hard structures come from a search on the generator alone"""
    for row, seeds in HARD_SEEDS.items():
        for N, seed in seeds.items():
            assert dc.hard_seed_search(row, N) == seed, (row, N)
    assert [int(v) for v in dc.hard_qp(HARD_SEEDS["hard-free"][3], 3).dims.nx] == [6, 6, 1, 1]
    assert dict(HARD_SEEDS["hard-x0"]) == {1: 3, 2: 1, 3: 1, 9: 0} and dict(HARD_SEEDS["hard-free"]) == {1: 2, 2: 0, 3: 0, 9: 9}


BAR_LANES = sorted(set(range(5)) | set(compared_lanes(65)) | set(compared_lanes(130)))


def test_multiplier_bar_source(hostsim_lib, monkeypatch):
    """where MULT_MEASURED comes from, reference against reference (the library only carries the data): over every instance that
    cases (a) and (c) compare, the oracle's pi and lam at the tolerances of the comparison cases against the oracle's own at tol_comp
    1e-13.  Measured 4.10e-9 (hard-free, N = 9, instance 62, stage 5; 2.6e-10 over instances 0 to 2); MULT_MEASURED = 4.2e-9 is that
    figure rounded up, the bar of the multipliers 64 times it, 2.7e-7"""
    from oracle.oracle import OracleQp, default_opts
    worst, where = 0.0, None
    for row in ROWS:
        for N in HORIZONS:
            gb, _ = dense_batch(hostsim_lib, monkeypatch, row, N, 130)
            for i in BAR_LANES:
                qp = gb.to_qp(i)
                a, b = OracleQp(qp), OracleQp(qp)
                assert a.solve(default_opts(iter_max=ITER_MAX, **TIGHT)) == 0
                assert b.solve(default_opts(iter_max=ITER_MAX, **dict(TIGHT, tol_comp=1e-13))) == 0
                for k in range(N + 1):
                    dev = dc.rel(dc.multiplier_views(qp, k, a.get(k, "lam")), dc.multiplier_views(qp, k, b.get(k, "lam")))
                    if k < N:
                        dev = max(dev, dc.rel(a.get(k, "pi"), b.get(k, "pi")))
                    if dev > worst:
                        worst, where = dev, (row, N, i, k)
    print(f"oracle at tol_comp 1e-12 against the oracle at 1e-13: {worst:.2e} at {where}")
    assert worst <= MULT_MEASURED and MULT_BAR == 64 * MULT_MEASURED and MULT_BAR <= 1e-6, worst


# ---- (a) stage-wise data on every structure the path accepts ---------------------------------------------------------------------------
def _grid_a():
    for row in ROWS:
        for N in HORIZONS:
            for B, tiled in ((1, False), (3, False), (65, True), (130, True)):
                # (host simulation, wave-tiled leg: lqr41 at N = 2, and the fixed-x0 structure on the general one-instance-per-lane
                # family, whose finalize kernel does not recover the multipliers of x0: they are kd_solve's own there)
                host = (B == 3 or N == 2) if not tiled else (B == 65 and (row, N) in (("lqr41", 2), ("hard-x0", 1)))
                yield host, f"{row}-N{N}-B{B}", row, N, B, tiled


@pytest.mark.parametrize("clib,row,N,B,tiled", _params(_grid_a()), indirect=["clib"])
def test_dense_on_stagewise_data(clib, monkeypatch, row, N, B, tiled):
    """(a) the LQR generators made stage-wise (lqr41x: state bounds behind stage 0 become rows of the state map) and two hard random
    structures (fixed x0; free x0 with a state dimension that switches mid-horizon), N = 1, 2, 3, 9; instance-major batches of 1 and 3,
    wave-tiled ragged batches of 65 and 130.  Measured worst deviations, host simulation / MI355X: see profiles/NOTES.md"""
    gb, blob = dense_batch(clib, monkeypatch, row, N, B, tiled)
    assert gb.solve() == 0, (gb.info("status"), gb.info("iter"))
    check_layout(gb, tiled)
    _check_columns(gb, row)
    assert int(gb.scalar("dense_slice")) == B
    worst = check_dense_solve(gb, blob)
    print(f"(a) {row} N={N} B={B} {gb.kernel_name}: iterations {sorted(set(gb.info('iter').tolist()))}", _fmt(worst))


# ---- (b) loops that wrap over the dense columns and over the rows ----------------------------------------------------------------------
@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_dense_loops_wrap(clib, monkeypatch):
    """(b) nx = 8, nu = 15 with state bounds, N = 16: 17 * 15 + 8 = 263 dense columns and 376 inequality rows, both past the 256 threads
    of the workgroup, so the Cholesky, the triangular solves, the reduced gradient, the fixed flags and every row loop stride twice.
    (13 s under the host simulation)"""
    from stagewise_common import _lqr, stagewise_perturb
    from acados_amd import OcpQpGpuBatch
    N, B = 16, 3
    dc.layout_env(monkeypatch, False)
    gb = OcpQpGpuBatch.from_qps(_lqr(8, 15, xbox=True)(N, B, 1), _clib=clib)
    stagewise_perturb(gb, 7116)
    dc.tight(gb)
    gb.opts_set("full_dense", 1)
    blob = gb.get_bulk_in()
    d = gb.dims
    rows = int(np.sum(d.nbx) + np.sum(d.nbu) + np.sum(d.ng))
    assert rows == 16 * 23 + 8 and rows > 256
    assert gb.solve() == 0, (gb.info("status"), gb.info("iter"))
    assert int(gb.scalar("dense_columns")) == 263
    worst = check_dense_solve(gb, blob)
    print(f"(b) 263 columns, {rows} rows: iterations {gb.info('iter').tolist()}", _fmt(worst))


# ---- (c) slices ------------------------------------------------------------------------------------------------------------------------
def _grid_c():
    for row in ROWS:
        for N in HORIZONS:
            yield (N == 3 and row in ("lqr41x", "lqr83", "hard-x0", "hard-free")), f"{row}-N{N}-B5", row, N, 5, False, (1, 2, 5)
            yield False, f"{row}-N{N}-B130", row, N, 130, True, (64, 1)


@pytest.mark.parametrize("clib,row,N,B,tiled,slices", _params(_grid_c()), indirect=["clib"])
def test_dense_slices(clib, monkeypatch, row, N, B, tiled, slices):
    """(c) option full_dense_slice: the batch worked off in launches of `slice` instances, every launch on the same workspace blocks.
    Output blob, iter, status, residual norms and mu are bit-identical to the unsliced solve; the batch reports ceil(B / slice) + 1
    launches (the finalize kernel is the last) and the slice in force; a change of the option takes effect at the next solve, and the
    workspace follows"""
    ref, _ = dense_batch(clib, monkeypatch, row, N, B, tiled)
    assert ref.solve() == 0
    check_layout(ref, tiled)
    assert int(ref.scalar("dense_slice")) == B and int(ref.scalar("launches")) == 2
    per_instance = ref.scalar("dense_workspace_bytes") / B
    want = results(ref)
    first, _ = dense_batch(clib, monkeypatch, row, N, B, tiled)     # the option set before the first dense solve of a batch ...
    first.opts_set("full_dense_slice", slices[0])
    for gb, todo in ((first, slices[:1]), (ref, slices + (0,))):     # ... and changed between the solves of one
        for s in todo:
            gb.opts_set("full_dense_slice", s)
            assert gb.solve() == 0, (s, gb.info("status"))
            eff = min(s, B) if s else B
            assert int(gb.scalar("dense_slice")) == eff, (s, gb.scalar("dense_slice"))
            assert int(gb.scalar("launches")) == -(-B // eff) + 1, (s, gb.scalar("launches"))
            assert gb.scalar("dense_workspace_bytes") == per_instance * eff
            assert_same_results(results(gb), want, what=(row, N, B, s))


# ---- (d) isolation and truncation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clib,row,tiled", _params([(True, "lqr83", "lqr83", False), (True, "hard-free", "hard-free", False),
                                                    (False, "lqr83-tiled", "lqr83", True)]), indirect=["clib"])
def test_dense_isolation_and_truncation(clib, monkeypatch, row, tiled):
    """(d) B = 5 in slices of 2: a NaN in q of a middle stage of instances 0 and 2 (instance 4 then runs on workspace block 0 behind
    a poisoned instance) ends those two with status 1 and leaves every other instance bit-identical to the clean run; iter_max 3
    ends every instance with status 2, iter 3 and a finite iterate"""
    N, B = 3, 5
    gb, blob = dense_batch(clib, monkeypatch, row, N, B, tiled)
    gb.opts_set("full_dense_slice", 2)
    assert gb.solve() == 0
    check_layout(gb, tiled)
    assert int(gb.scalar("launches")) == 4
    clean = results(gb)
    assert np.all(clean[1] > 3), clean[1]
    bad = blob.copy()
    o, n = gb.bulk_offset(0, "q", N // 2 + 1)
    assert n > 0
    bad[[0, 2], o + n // 2] = np.nan
    gb.set_bulk(bad)
    assert gb.solve() == 2
    assert gb.info("status").tolist() == [1, 0, 1, 0, 0], gb.info("status")
    assert_same_results(results(gb), clean, rows=[1, 3, 4], what="next to a NaN")
    gb.set_bulk(blob)
    gb.opts_set("iter_max", 3)
    assert gb.solve() == B
    assert np.all(gb.info("status") == 2) and np.all(gb.info("iter") == 3), (gb.info("status"), gb.info("iter"))
    assert np.all(np.isfinite(gb.get_bulk())) and np.all(np.isfinite(gb.info("mu")))
    gb.opts_set("iter_max", ITER_MAX)
    assert gb.solve() == 0
    assert_same_results(results(gb), clean, what="behind the truncated solve")


# ---- (e) fixed inputs ------------------------------------------------------------------------------------------------------------------
# row, x0 fixed, wave-tiled, flagged input rows (stage, row of idxb): lqr83 bounds every input, row = input; the fixed-x0 hard structure
# at N = 3 bounds input 1 at stage 0 (row 0) and both inputs at stage 2.  The first two run on a box family, whose kb_finalize recovers
# the multipliers of the flagged rows again behind kd_solve; on the general one-instance-per-lane family (third variant) nothing does,
# so there the values compared with the oracle are kd_solve's own, the branch for inputs behind stage 0 included
FIXED_INPUTS = {"x0-fixed": ("lqr83", True, False, ((0, 1), (2, 2))), "x0-free": ("lqr83", False, False, ((0, 1), (2, 2))),
                "general-tiled": ("hard-x0", True, True, ((0, 0), (2, 1)))}


@pytest.mark.parametrize("clib,variant", _params([(True, v, v) for v in FIXED_INPUTS]), indirect=["clib"])
def test_dense_fixed_inputs(clib, monkeypatch, variant):
    """(e) "fixed variables (idxe) anywhere among the inputs": one input of stage 0 and one of stage 2 equality-flagged (lbu == ubu
    there), with x0 fixed or free.  Primal against solve_exact, the fixed entries equal to their value exactly, and the multipliers of
    the flagged rows against the oracle at the measured bar.  (The host class AcadosOcpQp accepts idxe on state bounds only, as the
    reference's does: the QPs are made consistent without its dims check.)"""
    row, x0, tiled, flagged = FIXED_INPUTS[variant]
    N, B = 3, 3
    plain, _ = dense_batch(clib, monkeypatch, row, N, B, tiled)
    qps, vals = [plain.to_qp(i) for i in range(B)], {}
    nu, nx = int(plain.dims.nu[0]), int(plain.dims.nx[0])
    for i, qp in enumerate(qps):
        for k, r in flagged:
            assert r < int(qp.dims.nbu[k])
            lo, up = qp.lbu[k].copy(), qp.ubu[k].copy()
            vals[(i, k, int(qp.idxb[k][r]))] = lo[r] = up[r] = lo[r] + 0.7 * (up[r] - lo[r])
            qp.set("lbu", k, lo); qp.set("ubu", k, up)
            for f in ("lbu_mask", "ubu_mask"):
                m = qp._f[f][k].copy()
                m[r] = 1.0
                qp.set(f, k, m)
        if not x0:
            for f in ("lbx", "ubx", "lbx_mask", "ubx_mask"):
                qp.set(f, 0, np.zeros(0))
            qp.set("idxb", 0, np.arange(nu))
            qp.set("idxs_rev", 0, -np.ones(nu, dtype=int))
        nbu0 = int(qp.dims.nbu[0])
        idxe = {k: [r for kk, r in flagged if kk == k] for k in (0, 2)}
        idxe[0] += [nbu0 + e for e in range(nx)] if x0 else []
        for k in (0, 2):
            qp.set("idxe", k, idxe[k])
        qp.make_consistent(assert_dims=False)
    gb, blob = dense_batch(clib, monkeypatch, row, N, B, tiled, qps=qps)
    assert gb.get_int("idxe", 0).tolist() == idxe[0] and gb.get_int("idxe", 2).tolist() == idxe[2]
    assert gb.solve() == 0, (gb.info("status"), gb.info("iter"))
    check_layout(gb, tiled)
    assert gb.kernel_name.startswith("1tpi<" if tiled else "w16-box"), gb.kernel_name
    for (i, k, j), v in vals.items():
        assert gb.get("u", k)[i, j] == v, (i, k, j)
    worst = check_dense_solve(gb, blob, qps=qps)
    print(f"(e) {variant} {gb.kernel_name}: iterations {gb.info('iter').tolist()}", _fmt(worst))


# ---- (f) initialisation and loop options -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clib,row", _params([(True, "lqr83", "lqr83"), (True, "hard-x0", "hard-x0")]), indirect=["clib"])
def test_dense_initialisations(clib, monkeypatch, row):
    """(f) the three t0_init schemes start from different points and all reach the certified solution at 1e-9.  The predictor-only
    loop (pred_corr 0) of kd_solve cannot be reached: the batch has no such option, which is what is asserted here"""
    N, B = 3, 3
    gb, blob = dense_batch(clib, monkeypatch, row, N, B)
    gb.opts_set("mu0", 4.0)      # at the default mu0 = 1 schemes 0 (lam = t = sqrt(mu0)) and 1 (lam = mu0, t = 1) are one start
    ends = {}
    for t0 in (0, 1, 2):
        gb.opts_set("t0_init", t0)
        assert gb.solve() == 0, (t0, gb.info("status"))
        worst = check_dense_solve(gb, blob)
        ends[t0] = gb.get_bulk()
        print(f"(f) {row} t0_init {t0}: iterations {gb.info('iter').tolist()}", _fmt(worst))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert np.all(np.any(ends[a] != ends[b], axis=1)), (a, b)
    with pytest.raises(ValueError):
        gb.opts_set("pred_corr", 0)


REDO_SEED = 41


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_dense_conditional_redo(clib, monkeypatch):
    """(f) the conditional redo phase (cond_pred_corr, HPIPM's duality-measure test behind the corrector).  On the batches of (a) it
    never triggers: cond_pred_corr 0 and 1 give the same bits there.  It does on gradients that are large against the bounds: the hard
    structure of seed 41 (N = 4, fixed x0, four general rows), eight instances with q and r times U(-20, 30) + 3 N(0, 1), where some
    instances take the redo.  With the redo (default) every instance reaches the certified solution within the iteration cap; without it
    at least one instance follows other iterates (measured: instances 0, 1, 2, of which 1 runs into iter_max -- the limit cycle the redo
    ends), and every instance that still converges reaches the same certified solution"""
    from acados_amd import OcpQpGpuBatch
    from random_qp import random_structure_qp
    B = 8
    dc.layout_env(monkeypatch, False)
    qp = random_structure_qp(REDO_SEED, allow_slack=False)
    assert qp.N == 4 and len(qp.idxe[0]) == int(qp.dims.nx[0]) and int(np.sum(qp.dims.ng)) == 4
    gb = OcpQpGpuBatch.from_qps([qp] * B, _clib=clib)
    g = np.random.default_rng(REDO_SEED + 9000)
    for k in range(qp.N + 1):
        for f in ("q", "r"):
            a0 = gb.get(f, k)
            if a0.shape[1]:
                gb.set(f, k, a0 * g.uniform(-20.0, 30.0, (B, 1)) + 3 * g.standard_normal(a0.shape))
    dc.tight(gb)
    gb.opts_set("full_dense", 1)
    blob = gb.get_bulk_in()
    assert gb.solve() == 0, (gb.info("status"), gb.info("iter"))
    worst = check_dense_solve(gb, blob)
    with_redo = results(gb)
    print(f"(f) redo on: iterations {gb.info('iter').tolist()}", _fmt(worst))
    gb.opts_set("cond_pred_corr", 0)
    gb.solve()
    st, out = gb.info("status"), gb.get_bulk()
    differ = [i for i in range(B) if not np.array_equal(out[i], with_redo[0][i])]
    print(f"(f) redo off: iterations {gb.info('iter').tolist()}, status {st.tolist()}, other iterates in {differ}")
    assert differ, "cond_pred_corr 0 changed nothing: the option is not honoured, or the redo never triggers on these data"
    assert np.all((st == 0) | (st == 2)), st
    sol, w2 = dc.solution(gb), {}
    for i in np.flatnonzero(st == 0):
        dc.compare_instance(gb, sol, int(i), *dc.references(gb, blob, int(i)), w2)


# ---- (g) refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clib,what", _params([(True, "slacks", "slacks"), (True, "fixed-state", "fixed-state")]), indirect=["clib"])
def test_dense_refusals(clib, monkeypatch, what):
    """(g) slacks, and a state equality-flagged behind stage 0, are refused: solve() returns B, every status is 4, every iter 0, and
    the iterate is untouched; back on full_dense 0 the slack batch solves on the stage-wise family"""
    from acados_amd import OcpQpGpuBatch
    from stagewise_common import GENERATORS
    N, B = 2, 3
    dc.layout_env(monkeypatch, False)
    if what == "slacks":
        qps = GENERATORS["chain24"](N, B, 1)
    else:
        qps = GENERATORS["lqr41x"](N, B, 1)
        for qp in qps:
            lo, up = qp.lbx[1].copy(), qp.ubx[1].copy()
            lo[0] = up[0] = 0.1
            qp.set("lbx", 1, lo); qp.set("ubx", 1, up)
            qp.set("idxe", 1, [1])          # row 1 of idxb at stage 1: the first state
            qp.make_consistent()
    gb = OcpQpGpuBatch.from_qps(qps, _clib=clib)
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, 1e-8)
    gb.opts_set("iter_max", ITER_MAX)
    gb.opts_set("full_dense", 1)
    g = np.random.default_rng(5)
    for k in range(N + 1):
        # (x of a stage with equality-flagged states is left alone: their value lives in the iterate)
        for f in ("u", "pi", "lam", "t", "sl", "su") + (() if len(qps[0].idxe[k]) else ("x",)):
            n = gb._len(f, k) if not (f == "pi" and k == N) else 0
            if n:
                gb.set(f, k, g.uniform(0.5, 1.5, (B, n)))
    before = gb.get_bulk()
    assert np.count_nonzero(before) > 0.8 * before.size
    assert gb.solve() == B
    assert np.all(gb.info("status") == 4) and np.all(gb.info("iter") == 0), (gb.info("status"), gb.info("iter"))
    assert np.array_equal(gb.get_bulk(), before)
    if what == "slacks":        # (a state flagged behind stage 0 is outside what the stage-wise families solve as well: DESIGN 7)
        gb.opts_set("full_dense", 0)
        assert gb.solve() == 0, gb.info("status")
        assert np.all(gb.info("status") == 0) and np.all(gb.info("iter") > 0)
        assert gb.res_compute().max() <= 2e-8
        assert gb.kernel_name.startswith(("w16r-gen<", "wpi-gen("))


# ---- (h) what follows a dense solve ----------------------------------------------------------------------------------------------------
# tol / bars: the box rows at the tolerances and bars of test_kkt_sens.py::test_sensitivities_box_vs_dense; the hard structure holds
# active general rows, whose stage matrix H + sum Gamma a a' has condition ~ Gamma = lam / t: a one-shot sensitivity solve out of its
# Cholesky factor carries Gamma * eps, with the stage-wise iterate as with the dense one (measured at 1e-9: 5e-5 and 2e-4 against the
# dense solve at the batch's own iterate), so it takes the tolerance and bars of test_sensitivities_soft_and_general_rows_vs_dense.
# With tol_own at 2e-4 the leg at the batch's own iterate no longer proves on this row that the factor belongs to the dense iterate:
# there the Riccati getter (P of stage N, 1e-9) and the data gradient, taken behind a dense solve of its own, do.
# grad_tol / grad: tolerance of that dense solve and the bar of test_data_grad.py on the gradient: 1e-9 on the box rows; 1e-4, its bar
# for structures with active general rows (DENSE_BAR), on the hard structure, solved at 1e-7 where that bar holds with room (measured
# 5.4e-6; the error follows eps / min t, 2e-4 at 1e-8 from the dense and 1e-4 from the stage-wise iterate: DESIGN 7)
BOX_BARS = dict(tol=1e-6)
GEN_BARS = dict(tol=2e-4, tol_own=2e-4, tol_mult_own=1e-4, tol_mult=5e-4, tol_solve=1e-8)
FOLLOW = {"w16": dict(env={"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "1"}, row="lqr83", N=4, name="w16-box", tol=1e-9, bars=BOX_BARS,
                 grad_tol=1e-9, grad=1e-9),
          "1tpi": dict(env={"ACADOS_AMD_WPI": "0"}, row="lqr83", N=4, name="1tpi-box", tol=1e-9, bars=BOX_BARS, grad_tol=1e-9, grad=1e-9),
          "hard-x0": dict(env={"ACADOS_AMD_WPI": "1"}, row="hard-x0", N=3, name="", tol=1e-8, bars=GEN_BARS, grad_tol=1e-7, grad=1e-4)}


@pytest.mark.parametrize("clib,case", _params([(True, c, c) for c in FOLLOW]), indirect=["clib"])
def test_after_a_dense_solve(clib, monkeypatch, case):
    """(h) dense_solve leaves the factor of the stage-wise sweeps stale and borrows rd rm dlam dt pcorr: the Riccati getter, the
    sensitivities (seeds in q, b and x0; on the box rows the leg at the batch's own iterate at 1e-8 is the sharp one) and the data
    gradient refactor at the DENSE iterate, and a stage-wise solve of the same batch afterwards is bit-identical to one of a batch that never ran the dense path"""
    from test_data_grad import _rel, dense_grad, random_cot
    from test_kkt_sens import _check_sens
    c = FOLLOW[case]
    for k, v in dict(c["env"], ACADOS_AMD_SENS_SLICE="2").items():
        monkeypatch.setenv(k, v)
    N, B = c["N"], 3

    def batch(dense):
        from acados_amd import OcpQpGpuBatch
        gb = OcpQpGpuBatch.from_qps(dc.row_qps(c["row"], N, B), _clib=clib)
        if c["row"] in HARD_SEEDS:
            dc.instance_noise(gb, 8000 + N)
        else:
            dc.stagewise_perturb(gb, 7000 + 100 + N)
        for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
            gb.opts_set(f, c["tol"])
        gb.opts_set("iter_max", ITER_MAX)
        gb.opts_set("full_dense", dense)
        return gb

    gb = batch(1)
    assert gb.solve() == 0, (gb.info("status"), gb.info("iter"))
    assert gb.kernel_name.startswith(c["name"]), gb.kernel_name
    assert gb.res_compute().max() <= c["tol"] * (1.0 + 1e-3) + 1e-12
    qps = [gb.to_qp(i) for i in range(B)]
    d = gb.dims
    # Riccati getter: P_N = Q_N + J' diag(lam / t) J over the rows of stage N (no inputs there), from the batch's own lam and t
    lam, t, P = gb.get("lam", N), gb.get("t", N), gb.riccati(N)["P"]
    for i, qp in enumerate(qps):
        nbg = int(d.nb[N] + d.ng[N])
        J = np.zeros((nbg, int(d.nx[N])))
        J[np.arange(int(d.nb[N])), np.asarray(qp.idxb[N], dtype=int)] = 1.0
        J[int(d.nb[N]):] = qp.C[N]
        on = t[i] > 0.0
        gam = (np.where(on, lam[i], 0.0) / np.where(on, t[i], 1.0))
        want = qp.Q[N] + J.T @ ((gam[:nbg] + gam[nbg:2 * nbg])[:, None] * J)
        assert np.max(np.abs(P[i] - want)) <= 1e-9 * np.max(np.abs(want)), (case, i, np.max(np.abs(P[i] - want)), np.max(np.abs(want)))
    # sensitivities
    rng = np.random.default_rng(3)
    ex = [rng.standard_normal((B, int(d.nx[k]))) for k in range(N + 1)]
    seeds = {"q": ([("seed_q", k, ex[k]) for k in range(N + 1)], {("q", k): ex[k] for k in range(N + 1)}),
             "b": ([("seed_b", k, ex[k + 1]) for k in range(N)], {("b", k): ex[k + 1] for k in range(N)}),
             "x0": ([("seed_lbx", 0, ex[0]), ("seed_ubx", 0, ex[0])], {("lbx", 0): ex[0], ("ubx", 0): ex[0]})}
    for name, (sdev, sdense) in seeds.items():
        worst = _check_sens(gb, qps, sdev, sdense, fields=("x", "u", "pi", "lam", "t"), **c["bars"])
        assert worst <= c["bars"]["tol"], (name, worst)
        print(f"(h) {case} sensitivities, seed {name}: worst deviation from the dense solve at the oracle's solution {worst:.1e}")
    # data gradient, behind a dense solve of its own: the factor is stale again, the refresh is data_grad's to make
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, c["grad_tol"])
    assert gb.solve() == 0
    cot = random_cot(gb, np.random.default_rng(2))
    g = gb.data_grad(cot)
    for i in range(B):
        err = _rel(g[i], dense_grad(gb, qps[i], i, cot[i]))
        assert err <= c["grad"], (case, i, err)
        print(f"(h) {case} data gradient, instance {i}: {err:.1e} from the dense adjoint")
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, c["tol"])
    # clean hand-back
    gb.opts_set("full_dense", 0)
    assert gb.solve() == 0
    fresh = batch(0)
    assert fresh.solve() == 0
    assert gb.kernel_name == fresh.kernel_name
    assert_same_results(results(gb), results(fresh), what="stage-wise solve behind a dense one")
    for k in range(N + 1):
        for f in ("ric_L", "ric_l"):
            assert np.array_equal(gb.get(f, k), fresh.get(f, k)), (f, k)

"""ric_alg 0: the classical Riccati recursion (P carried unfactored; only the reduced Hessian has to be positive definite).

Indefinite test problems with a known answer: a positive-definite QP with, for every k < N,
    stage k   + 1/2 d_k |A_k x + B_k u + b_k|^2     (R += d B'B, S += d B'A, Q += d A'A, r += d B'b, q += d A'b)
    stage k+1 - 1/2 d_k |x|^2                        (Q_{k+1} -= d I).
On the dynamics the objective is unchanged up to a constant: the primal solution and the inequality multipliers are the
original QP's (the oracle solves that one), P_k becomes P_k - d_{k-1} I, R~ + B'PB and the gains stay.  The stage blocks of
the transformed QP have negative eigenvalues, which the square-root form cannot represent.  Every test runs on the
host-simulation tier and on the device."""
import copy

import numpy as np
import pytest

from conftest import GOLDEN_PAIRS, load_qp
from dense_ref import kkt_residual_norms, sens_dense
from oracle.oracle import OracleQp, default_opts
from random_qp import random_structure_qp

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
KKT_TOL = 1e-8 * (1.0 + 1e-3) + 1e-13
TOLS = ("tol_stat", "tol_eq", "tol_ineq", "tol_comp")


@pytest.fixture
def clib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


def _stage_H(qp, k):
    R, S, Q = (np.atleast_2d(np.asarray(getattr(qp, f)[k], dtype=float)) for f in ("R", "S", "Q"))
    nu, nx = int(qp.dims.nu[k]), int(qp.dims.nx[k])
    H = np.zeros((nu + nx, nu + nx))
    H[:nu, :nu] = R.reshape(nu, nu) if nu else 0.0
    if nu:
        H[:nu, nu:] = S.reshape(nu, nx)
        H[nu:, :nu] = S.reshape(nu, nx).T
    H[nu:, nu:] = Q.reshape(nx, nx)
    return H


def indefinite(qp, factor=3.0):
    """(transformed QP, d): d_k = factor * the largest eigenvalue of any stage block of qp"""
    N = qp.N
    d = factor * max(np.linalg.eigvalsh(_stage_H(qp, k)).max() for k in range(N + 1))
    t = copy.deepcopy(qp)
    for k in range(N):
        A, B, b = (np.atleast_2d(np.asarray(getattr(qp, f)[k], dtype=float)) for f in ("A", "B", "b"))
        nx1, nx, nu = int(qp.dims.nx[k + 1]), int(qp.dims.nx[k]), int(qp.dims.nu[k])
        A, B, b = A.reshape(nx1, nx), B.reshape(nx1, nu), b.reshape(nx1)
        H = _stage_H(t, k)
        r = np.asarray(t.r[k], dtype=float).reshape(nu)
        q = np.asarray(t.q[k], dtype=float).reshape(nx)
        t.set("R", k, H[:nu, :nu] + d * B.T @ B)
        t.set("S", k, H[:nu, nu:] + d * B.T @ A)
        t.set("Q", k, H[nu:, nu:] + d * A.T @ A)
        t.set("r", k, r + d * B.T @ b)
        t.set("q", k, q + d * A.T @ b)
        Hn = _stage_H(t, k + 1)
        t.set("Q", k + 1, Hn[int(qp.dims.nu[k + 1]):, int(qp.dims.nu[k + 1]):] - d * np.eye(nx1))
    # the square-root form cannot represent these blocks: the terminal one is indefinite by construction
    assert np.linalg.eigvalsh(_stage_H(t, N)).min() < 0.0
    assert sum(np.linalg.eigvalsh(_stage_H(t, k)).min() < 0.0 for k in range(N + 1)) >= 1
    return t, d


def _batch(clib, qps, ric_alg, tol=1e-8):
    from acados_amd import OcpQpGpuBatch
    gb = OcpQpGpuBatch.from_qps(qps, _clib=clib)
    for f in TOLS:
        gb.opts_set(f, tol)
    gb.opts_set("ric_alg", ric_alg)
    return gb


def _oracle(qp, tol=1e-8):
    o = OracleQp(qp)
    assert o.solve(default_opts(**{f: tol for f in TOLS})) == 0
    return o


def _getter(gb, i):
    return lambda k, f: gb.get(f, k)[i] if not (f == "pi" and k == gb.N) else np.zeros(0)


def _max_diff(gb, i, o, N, fields=("u", "x", "sl", "su", "lam", "t", "pi")):
    worst = 0.0
    for k in range(N + 1):
        for f in fields:
            if f == "pi" and k == N:
                continue
            want = o.get(k, f)
            if want.size:
                worst = max(worst, float(np.max(np.abs(gb.get(f, k)[i] - want))))
    return worst


def _pd_cases():
    from acados_amd.generators import mass_spring_qp
    cases = [("golden:" + p, load_qp(p)) for p, _ in GOLDEN_PAIRS]
    cases.append(("mass_spring", mass_spring_qp(N=6)))
    for seed in range(10):
        cases.append((f"random{seed}", random_structure_qp(seed, N=4, allow_slack=seed % 3 == 0)))
    return cases


# ---------------------------------------------------------------------------------------------------- 1. options

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_ric_alg_options(clib, monkeypatch):
    """ric_alg 0 is accepted by the Python options and by the batch, 2 is refused; the batch names its classical kernel set,
    also for shapes that would otherwise run the one-instance-per-lane or sixteen-lanes families"""
    from acados_amd import AcadosOcpQpOptions
    from acados_amd.generators import mass_spring_qp
    o = AcadosOcpQpOptions()
    o.ric_alg = 0
    o.make_consistent(6)
    o.ric_alg = 2
    with pytest.raises(ValueError):
        o.make_consistent(6)
    qp = mass_spring_qp(N=4)
    for env in ({"ACADOS_AMD_WPI": "0"}, {"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "1"}, {"ACADOS_AMD_WPI": "1"}):
        for key in ("ACADOS_AMD_WPI", "ACADOS_AMD_W16"):
            monkeypatch.delenv(key, raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        gb = _batch(clib, [qp, qp], 1)
        name1 = gb.kernel_name
        assert "ric0" not in name1 and gb.ric_alg == 1
        gb.opts_set("ric_alg", 0)
        assert gb.ric_alg == 0 and gb.kernel_name.startswith("wpi-box(") and "ric0" in gb.kernel_name, (env, gb.kernel_name)
        gb.opts_set("ric_alg", 0)   # the same value again
        with pytest.raises(ValueError):
            gb.opts_set("ric_alg", 2)
        assert gb.ric_alg == 0
        gb.opts_set("ric_alg", 1)
        assert gb.kernel_name == name1 and gb.ric_alg == 1
        gb.close()


# ------------------------------------------------------------------------------------ 2. positive-definite parity

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_ric0_positive_definite_parity(clib):
    """on positive-definite QPs the classical recursion reaches the oracle's solution at the parity bar"""
    diffs = []
    for name, qp in _pd_cases():
        o = _oracle(qp)
        gb = _batch(clib, [qp, qp], 0)
        assert "ric0" in gb.kernel_name
        assert gb.solve() == 0, name
        assert np.all(gb.info("status") == 0), name
        d = _max_diff(gb, 1, o, qp.N)
        assert d <= 1e-8, (name, d)
        diffs.append(d)
        nrm = gb.res_compute()
        assert np.all(nrm <= KKT_TOL), (name, nrm)
        gb.close()
    assert np.median(diffs) <= 1e-9, diffs


# ------------------------------------------------------------------------------------------ 3. indefinite QPs

def _indefinite_cases(gpu):
    from acados_amd.generators import mass_spring_qp
    cases = [("mass_spring", mass_spring_qp(N=6 if not gpu else 10))]
    for seed in (1, 2, 4, 5, 7):   # box
        cases.append((f"box{seed}", random_structure_qp(seed, N=4, allow_general=False, allow_slack=False)))
    for seed in (3, 6, 8):         # general rows and slacks
        cases.append((f"gen{seed}", random_structure_qp(seed, N=4)))
    return cases


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_ric0_indefinite(clib, request):
    """indefinite stage blocks: status 0, the original QP's primal solution and inequality multipliers, and KKT residuals of
    the transformed QP at tolerance -- by the device's residual kernel and by the independent NumPy restatement, whose
    stationarity rows pin the dynamics multipliers pi (unique: the dynamics rows have full rank)"""
    gpu = "gpu" in request.node.callspec.id
    for name, qp in _indefinite_cases(gpu):
        t, _ = indefinite(qp)
        o = _oracle(qp, tol=1e-10)
        gb = _batch(clib, [t, t], 0, tol=1e-10)
        assert gb.solve() == 0, name
        assert np.all(gb.info("status") == 0), name
        scale = max(1.0, max(np.max(np.abs(o.get(k, f))) for k in range(qp.N + 1) for f in ("u", "x") if o.get(k, f).size))
        d = _max_diff(gb, 1, o, qp.N, fields=("u", "x", "sl", "su", "lam"))
        assert d <= 1e-7 * scale, (name, d)
        nrm = gb.res_compute()
        assert np.all(nrm <= 1e-10 * (1.0 + 1e-3) + 1e-12), (name, nrm)
        ref = kkt_residual_norms(t, _getter(gb, 1))
        assert np.all(ref <= 1e-9), (name, ref)
        gb.close()


# ------------------------------------------------------------------------------------------------ 4. getters

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_ric0_getters(clib, monkeypatch):
    """riccati() of the classical layout: on a positive-definite QP the oracle's factor (same relations as the square-root
    getters); on the indefinite transform of a QP whose only inequality rows are the x0 equality, P_k = P_k(original) - d I
    with K and k unchanged, by riccati() and by the solver_get slot"""
    from acados_amd.generators import mass_spring_qp
    monkeypatch.setenv("ACADOS_AMD_WPI", "1")
    qp = mass_spring_qp(N=6)
    o = _oracle(qp)
    o.refactor()
    gb = _batch(clib, [qp, qp], 0)
    assert gb.solve() == 0
    for k in range(qp.N + 1):
        nu = int(qp.dims.nu[k])
        nv = nu + int(qp.dims.nx[k])
        Lo = o.get(k, "ric_L").reshape(nv, nv, order="F")
        ric = gb.riccati(k)
        Lx = Lo[nu:, nu:]
        assert np.allclose(ric["P"][1], Lx @ Lx.T, rtol=1e-6, atol=1e-9), k
        assert np.allclose(ric["p"][1], Lx @ o.get(k, "ric_l")[nu:], rtol=1e-5, atol=1e-9), k
        if nu:
            M = Lo @ Lo.T
            assert np.allclose(ric["K"][1], -np.linalg.solve(M[:nu, :nu], M[:nu, nu:]), rtol=1e-5, atol=1e-7), k
            assert np.allclose(ric["Lr"][1], Lo[:nu, :nu], rtol=1e-6, atol=1e-9), k
    gb.close()
    base = _free_qp(5)
    t, d = indefinite(base)
    g1 = _batch(clib, [base, base], 1)
    g0 = _batch(clib, [t, t], 0)
    assert g1.solve() == 0 and g0.solve() == 0
    for k in range(base.N + 1):
        r1, r0 = g1.riccati(k), g0.riccati(k)
        want = r1["P"][1] - (d * np.eye(r1["P"].shape[1]) if k > 0 else 0.0)
        if k > 0:
            assert np.linalg.eigvalsh(r0["P"][1]).min() < 0.0, k   # P itself indefinite: no Cholesky factor of it exists
        assert np.allclose(r0["P"][1], want, rtol=1e-6, atol=1e-6 * np.max(np.abs(want))), k
        if k < base.N:
            assert np.allclose(r0["K"][1], r1["K"][1], rtol=1e-6, atol=1e-8), k
            assert np.allclose(r0["k"][1], r1["k"][1], rtol=1e-6, atol=1e-8), k
    g0.close(); g1.close()
    _solver_get_check(clib, base, t, d)


def _free_qp(seed, N=5, nx=4, nu=2):
    """strictly convex QP whose only inequality rows are x0 (equality-flagged): every multiplier is inactive"""
    from acados_amd import AcadosOcpQp
    g = np.random.default_rng(seed)
    qp = AcadosOcpQp(N)
    for k in range(N + 1):
        n = nx + (nu if k < N else 0)
        M = g.standard_normal((n, n))
        H = M @ M.T / n + 0.5 * np.eye(n)
        m = nu if k < N else 0
        qp.set("R", k, H[:m, :m]); qp.set("S", k, H[:m, m:]); qp.set("Q", k, H[m:, m:])
        qp.set("r", k, g.standard_normal(m)); qp.set("q", k, g.standard_normal(nx))
        if k < N:
            qp.set("A", k, 0.5 * g.standard_normal((nx, nx)) / np.sqrt(nx)); qp.set("B", k, g.standard_normal((nx, nu)))
            qp.set("b", k, 0.1 * g.standard_normal(nx))
    x0 = g.uniform(-1, 1, nx)
    qp.set("idxb", 0, nu + np.arange(nx)); qp.set("lbx", 0, x0); qp.set("ubx", 0, x0); qp.set("idxe", 0, np.arange(nx))
    qp.make_consistent()
    return qp


def _solver_get_check(clib, base, t, d):
    """the solver_get slot (ocp_qp_gpu_ipm_solver_get) on the classical layout against the square-root one"""
    import ctypes as C
    from acados_amd import AcadosOcpQpOptions, AcadosOcpQpSolver
    clib.ocp_qp_solver_get_ric.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    nu, nx = int(base.dims.nu[0]), int(base.dims.nx[0])
    out = {}
    for ric, qp in ((1, base), (0, t)):
        opts = AcadosOcpQpOptions()
        opts.tol_stat = opts.tol_eq = opts.tol_ineq = opts.tol_comp = 1e-10
        opts.ric_alg = ric
        s = AcadosOcpQpSolver(qp, opts, _clib=clib)
        assert s.solve() == 0
        for k in (0, 2):
            for name, s1, s2 in (("K", nu, nx), ("k", nu, 1), ("P", nx, nx), ("p", nx, 1), ("Lr", nu, nu)):
                a = np.zeros(s1 * s2)
                clib.ocp_qp_solver_get_ric(s.c_solver, s.c_in, s.c_out, name.encode(), k, a.ctypes.data_as(C.c_void_p), s1, s2)
                out[(ric, k, name)] = a.reshape(s2, s1).T
    for k in (0, 2):
        want = out[(1, k, "P")] - (d * np.eye(nx) if k else 0.0)
        assert np.allclose(out[(0, k, "P")], want, rtol=1e-6, atol=1e-6 * np.max(np.abs(want))), k
        for name in ("K", "k", "Lr"):
            assert np.allclose(out[(0, k, name)], out[(1, k, name)], rtol=1e-6, atol=1e-8), (k, name)


# ------------------------------------------------------------------------------------------------ 7. round trips

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_ric_alg_round_trip(clib):
    """1 -> 0 -> 1 on one batch: each solve gives its variant's result and name"""
    from acados_amd.generators import mass_spring_qp
    qp = mass_spring_qp(N=6)
    gb = _batch(clib, [qp, qp], 1)
    assert gb.solve() == 0
    x1 = [gb.get("x", k).copy() for k in range(qp.N + 1)]
    n1 = gb.kernel_name
    gb.opts_set("ric_alg", 0)
    assert "ric0" in gb.kernel_name
    assert gb.solve() == 0
    for k in range(qp.N + 1):
        assert np.max(np.abs(gb.get("x", k) - x1[k])) <= 1e-8
    gb.opts_set("ric_alg", 1)
    assert gb.kernel_name == n1
    assert gb.solve() == 0
    for k in range(qp.N + 1):
        assert np.array_equal(gb.get("x", k), x1[k])
    gb.close()


def test_ric0_compaction_is_bit_identical_hostsim(hostsim_lib):
    """the classical sweeps on compacted sub-batches: every output bit equals the run without compaction"""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch
    N, B = 8, 96
    data = random_lqr_batch(N=N, batch=B, seed=9)
    runs = []
    for cmin in (1 << 30, 4):
        gb = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, _clib=hostsim_lib)
        fill_lqr_batch(gb, data, N)
        gb.opts_set("tol_stat", 1e-8)
        gb.opts_set("ric_alg", 0)
        gb.opts_set("compact_min", cmin)
        gb.opts_set("tail_max", 0)
        assert "ric0" in gb.kernel_name
        assert gb.solve() == 0
        runs.append(gb)
    assert int(runs[0].scalar("compactions")) == 0 and int(runs[1].scalar("compactions")) >= 1
    for f in ("status", "iter", "res_stat", "res_comp", "mu"):
        assert np.array_equal(runs[0].info(f), runs[1].info(f)), f
    for k in range(N + 1):
        for f in ("x", "u", "lam", "t") + (("pi",) if k < N else ()):
            assert np.array_equal(runs[0].get(f, k), runs[1].get(f, k)), (f, k)


# ----------------------------------------------------------------------------- hand-over of one-instance-per-lane batches

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_ric0_hand_over_solve(clib, monkeypatch):
    """a batch on the one-instance-per-lane family (ACADOS_AMD_WPI=0) solves with ric_alg 0 on a wave-per-instance
    sub-batch: solution and statuses of the indefinite QP, the iteration statistics and the classical factor read through
    the parent; and a factor asked for right after switching ric_alg (no solve in between) is the classical one too"""
    from acados_amd.generators import mass_spring_qp
    qp = mass_spring_qp(N=6)
    t, d = indefinite(qp)
    o = _oracle(qp, tol=1e-10)
    monkeypatch.setenv("ACADOS_AMD_WPI", "1")
    ref = _batch(clib, [t, t, t], 0, tol=1e-10)
    assert ref.solve() == 0
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")
    gb = _batch(clib, [t, t, t], 1, tol=1e-10)
    assert gb.kernel_name.startswith("1tpi")
    gb.opts_set("ric_alg", 0)
    assert gb.kernel_name.startswith("wpi-box(") and "ric0" in gb.kernel_name
    assert gb.solve() == 0
    assert np.all(gb.info("status") == 0)
    assert np.array_equal(gb.info("iter"), ref.info("iter"))
    scale = max(1.0, max(np.max(np.abs(o.get(k, f))) for k in range(qp.N + 1) for f in ("u", "x") if o.get(k, f).size))
    assert _max_diff(gb, 2, o, qp.N, fields=("u", "x", "lam")) <= 1e-7 * scale
    st = gb.stat(0)
    assert np.any(st != 0.0) and np.array_equal(st, ref.stat(0))
    for k in range(qp.N + 1):
        assert np.array_equal(gb.get("ric_L", k), ref.get("ric_L", k)), k
        r, rr = gb.riccati(k), ref.riccati(k)
        for f in ("P", "p", "K", "k"):
            assert np.array_equal(r[f], rr[f]), (k, f)
    gb.close()
    # solve with the square-root form, switch, read the factor before the next solve
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")
    gb = _batch(clib, [qp, qp], 1)
    assert gb.solve() == 0
    P1 = [gb.riccati(k)["P"].copy() for k in range(qp.N + 1)]
    gb.opts_set("ric_alg", 0)
    for k in range(1, qp.N + 1):
        P0 = gb.riccati(k)["P"]
        assert np.allclose(P0, P1[k], rtol=1e-8, atol=1e-10 * np.max(np.abs(P1[k]))), k
    gb.close()


# ----------------------------------------------------------------------------------------------- 5. sensitivities

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_ric0_sensitivities(clib):
    """sens_solve on an indefinite QP (the sweeps of the classical factor at the solution) against the dense linearised-KKT
    solve of the same QP at the device's solution (every field, to rounding) and, for seeds the transform leaves alone (q, r,
    x0), the primal sensitivities of the ORIGINAL QP at the oracle's solution"""
    from acados_amd.generators import mass_spring_qp
    qp = mass_spring_qp(N=5)
    t, _ = indefinite(qp)
    o = _oracle(qp, tol=1e-10)
    B = 2
    gb = _batch(clib, [t] * B, 0, tol=1e-10)
    assert gb.solve() == 0
    nx, nu = int(qp.dims.nx[0]), int(qp.dims.nu[0])
    rng = np.random.default_rng(4)
    ex, eu = rng.standard_normal((B, nx)), rng.standard_normal((B, nu))
    cases = {
        "q": ([("seed_q", k, ex) for k in range(qp.N + 1)], {("q", k): ex for k in range(qp.N + 1)}),
        "r": ([("seed_r", 1, eu)], {("r", 1): eu}),
        "x0": ([("seed_lbx", 0, ex), ("seed_ubx", 0, ex)], {("lbx", 0): ex, ("ubx", 0): ex}),
        "b": ([("seed_b", k, ex) for k in range(qp.N)], {("b", k): ex for k in range(qp.N)}),
    }
    for name, (sdev, sdense) in cases.items():
        for (f, k, v) in sdev:
            gb.sens_set(f, k, v)
        gb.sens_solve()
        for i in range(B):
            sd = {key: val[i] for key, val in sdense.items()}
            refs = [("own", sens_dense(t, _getter(gb, i), sd))]
            if name != "b":
                refs.append(("original", sens_dense(qp, o.get, sd)))
            for which, ref in refs:
                scale = max(1.0, max(np.max(np.abs(ref(k, f))) for k in range(qp.N + 1) for f in ("x", "u") if ref(k, f).size))
                fields = ("x", "u", "pi", "lam", "t") if which == "own" else ("x", "u")
                for k in range(qp.N + 1):
                    for f in fields:
                        if f == "pi" and k == qp.N:
                            continue
                        want, got = ref(k, f), gb.get("sens_" + f, k)[i]
                        if f in ("lam", "t"):
                            sel = np.array([(k, e) in ref.active for e in range(want.size)], dtype=bool)
                            got, want = got[sel], want[sel]
                        if want.size == 0:
                            continue
                        err = np.max(np.abs(got - want)) / max(scale, np.max(np.abs(want)))
                        lim = (2e-6 if f in ("lam", "t") else 1e-8) if which == "own" else 1e-6
                        assert err <= lim, (name, which, i, k, f, err)
    gb.close()


# --------------------------------------------------------------------------------------------- 6. partial condensing

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_ric0_partial_condensing(clib):
    """cond_N < N with ric_alg 0 on an indefinite QP: the condensed batch runs the classical sweeps and the expanded solution
    is the original QP's"""
    from acados_amd.generators import mass_spring_qp
    qp = mass_spring_qp(N=6)
    t, _ = indefinite(qp)
    o = _oracle(qp, tol=1e-10)
    gb = _batch(clib, [t, t], 0, tol=1e-10)
    gb.opts_set("cond_N", 3)
    assert gb.solve() == 0
    assert int(gb.scalar("cond_N_active")) == 3
    assert "ric0" in gb.condensed_kernel_name()
    assert np.all(gb.info("status") == 0)
    scale = max(1.0, max(np.max(np.abs(o.get(k, f))) for k in range(qp.N + 1) for f in ("u", "x") if o.get(k, f).size))
    d = _max_diff(gb, 1, o, qp.N, fields=("u", "x", "lam"))
    assert d <= 1e-6 * scale, d
    gb.close()


# ---------------------------------------------------------------------------------------------------------- 8. ISA

def test_ric0_kernels_no_scratch():
    """every classical instantiation in the product library: no scratch, no more spilled VGPRs than its square-root twin"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "acados_amd", "csrc", "libacados_amd_qp.so")
    if not os.path.exists(lib):
        pytest.skip("product library not built")
    sys.path.insert(0, os.path.join(root, "tools"))
    import isa_lint
    if not isa_lint.READELF:
        pytest.skip("llvm-readelf not found")
    import tempfile
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for q, co in enumerate(isa_lint.code_objects(lib)):
            path = os.path.join(tmp, f"co{q}.o")
            with open(path, "wb") as f:
                f.write(co)
            meta.update(isa_lint.metadata(path))
    names = isa_lint.demangle(list(meta))
    ric0 = [s for s in meta if ", 0, 0, true>(" in names[s] and
            any(names[s].startswith("void gqp::" + f + "<") for f in ("kw_factor", "kw_backrhs", "kw_fwd"))]
    assert len(ric0) == 22, [names[s] for s in ric0]
    twin = {names[s]: s for s in meta}
    for s in ric0:
        assert int(meta[s].get("private_segment_fixed_size", 0)) == 0, names[s]
        # no spilled VGPRs -- except where the square-root twin already has them (kw_factor<8, true>: n = 57..64 with general
        # rows sits at the 512-VGPR ceiling); the classical one may not spill more
        sq = twin[names[s].replace(", true>(", ", false>(")]
        assert int(meta[s].get("vgpr_spill_count", 0)) <= int(meta[sq].get("vgpr_spill_count", 0)), names[s]

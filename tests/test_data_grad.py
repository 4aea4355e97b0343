"""Reverse-mode gradients of the QP solution w.r.t. the QP data (ocp_qp_gpu_batch_adj_seed_bulk / _data_grad_bulk,
grad_kernels.hpp, acados_amd/torch_qp.py; DESIGN.md "Data gradients").

References that do not come from the contraction kernel:
  * a dense adjoint at the solver's own iterate: ONE dense solve of the linearised KKT system (tests/dense_ref.py
    sens_dense) seeded with the cotangent, the formulas of DESIGN.md restated in NumPy, and the value of an
    equality-flagged bound (x0) by FORWARD directions (one dense solve per fixed variable);
  * central differences of the loss, every entry re-solved (GPU tier)."""
import ctypes as C

import numpy as np
import pytest

from dense_ref import sens_dense
from random_qp import random_structure_qp

VEC_OUT = ("u", "x", "sl", "su")


def _tight(gb, tol, iter_max=None):
    for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
        gb.opts_set(f, tol)
    if iter_max:
        gb.opts_set("iter_max", iter_max)


def random_cot(gb, rng):
    """a cotangent on u x sl su of every stage, zero on pi lam t"""
    cot = np.zeros((gb.n_batch, gb.bulk_len(1)))
    for k in range(gb.N + 1):
        for f in VEC_OUT:
            o, n = gb.bulk_offset(1, f, k)
            if n > 0:
                cot[:, o:o + n] = rng.standard_normal((gb.n_batch, n))
    return cot


def _seg(gb, output, f, k):
    o, n = gb.bulk_offset(output, f, k)
    return (o, n) if n > 0 else (None, 0)


def dense_grad(gb, qp, i, cot_row, x0=True):
    """dL/d(input blob) of instance i from the dense adjoint at the device's own iterate (DESIGN.md formulas in NumPy);
    x0=False leaves the value entries of equality-flagged bounds at 0 (they need one dense solve per fixed variable)"""
    N, d = qp.N, qp.dims
    get = lambda k, f: gb.get(f, k)[i] if not (f == "pi" and k == N) else np.zeros(0)
    cot = {}
    for k in range(N + 1):
        for f in VEC_OUT:
            o, n = _seg(gb, 1, f, k)
            cot[(k, f)] = cot_row[o:o + n] if n else np.zeros(0)
    seeds = {}
    for k in range(N + 1):
        for f, sf in (("u", "r"), ("x", "q"), ("sl", "zl"), ("su", "zu")):
            if cot[(k, f)].size:
                seeds[(sf, k)] = cot[(k, f)]
    adj = sens_dense(qp, get, seeds)
    g = np.zeros(gb.bulk_len(0))

    def put(f, k, v):
        o, n = _seg(gb, 0, f, k)
        if n:
            v = np.asarray(v, dtype=float)
            g[o:o + n] = v.flatten(order="F") if v.ndim == 2 else v

    for k in range(N + 1):
        nu, nx, ns = int(d.nu[k]), int(d.nx[k]), int(d.ns[k])
        nb, ng = int(d.nb[k]), int(d.ng[k])
        nbu, nbg = int(d.nbu[k]), nb + ng
        u, x, sl, su = get(k, "u"), get(k, "x"), get(k, "sl"), get(k, "su")
        uh, xh, slh, suh = adj(k, "u"), adj(k, "x"), adj(k, "sl"), adj(k, "su")
        w, wh = np.concatenate([u, x]), np.concatenate([uh, xh])
        act = np.array([(k, e) in adj.active for e in range(2 * nbg + 2 * ns)], dtype=bool)
        lam = np.where(act, get(k, "lam"), 0.0)
        lamh = np.where(act, adj(k, "lam"), 0.0)
        if k < N:
            pi, pih = get(k, "pi"), adj(k, "pi")
            put("A", k, np.outer(pih, x) + np.outer(pi, xh))
            put("B", k, np.outer(pih, u) + np.outer(pi, uh))
            put("b", k, pih)
        put("Q", k, 0.5 * (np.outer(xh, x) + np.outer(x, xh)))
        put("R", k, 0.5 * (np.outer(uh, u) + np.outer(u, uh)))
        put("S", k, np.outer(uh, x) + np.outer(u, xh))
        put("q", k, xh)
        put("r", k, uh)
        lo, up = lamh[:nbg], lamh[nbg:2 * nbg]
        put("lbu", k, lo[:nbu]); put("lbx", k, lo[nbu:nb]); put("lg", k, lo[nb:])
        put("ubu", k, -up[:nbu]); put("ubx", k, -up[nbu:nb]); put("ug", k, -up[nb:])
        if ng:
            dl, dlh = lam[nbg + nb:2 * nbg] - lam[nb:nbg], up[nb:] - lo[nb:]
            put("D", k, np.outer(dlh, u) + np.outer(dl, uh))
            put("C", k, np.outer(dlh, x) + np.outer(dl, xh))
        if ns:
            put("Zl", k, slh * sl); put("Zu", k, suh * su)
            put("zl", k, slh); put("zu", k, suh)
            put("lls", k, lamh[2 * nbg:2 * nbg + ns]); put("lus", k, lamh[2 * nbg + ns:])
        idxe = [int(e) for e in qp.idxe[k]]
        if idxe and x0:
            # the equality-flagged bound (x0): its value by forward directions, its bound entry takes no part
            o, n = _seg(gb, 0, "lbx#value", k)
            ov = np.zeros(n)
            for row in idxe:
                e = np.zeros(int(d.nbx[k]))
                e[row - nbu] = 1.0
                fwd = sens_dense(qp, get, {("lbx", k): e})
                ov[row - nbu] = sum(float(cot[(kk, f)] @ fwd(kk, f)) for kk in range(N + 1) for f in VEC_OUT if cot[(kk, f)].size)
            g[o:o + n] = ov
            for f in ("lbx", "ubx"):
                o, n = _seg(gb, 0, f, k)
                for row in idxe:
                    g[o + row - nbu] = 0.0
    return g


def contraction_numpy(gb, i, cot_row):
    """the kernel's formulas restated in NumPy on the SOLVER'S OWN adjoint direction (sens_* after data_grad): checks the
    contraction alone (layouts, field map, signs), to rounding"""
    N = gb.N
    dims = gb.dims
    sol = {(k, f): gb.get(f, k)[i] for k in range(N + 1) for f in ("u", "x", "sl", "su", "lam")}
    adj = {(k, f): gb.get("sens_" + f, k)[i] for k in range(N + 1) for f in ("u", "x", "sl", "su", "lam")}
    for k in range(N):
        sol[(k, "pi")], adj[(k, "pi")] = gb.get("pi", k)[i], gb.get("sens_pi", k)[i]
    g = np.zeros(gb.bulk_len(0))
    blob = gb.get_bulk_in()[i]

    def put(f, k, v):
        o, n = _seg(gb, 0, f, k)
        if n:
            v = np.asarray(v, dtype=float)
            g[o:o + n] = v.flatten(order="F") if v.ndim == 2 else v

    for k in range(N + 1):
        nb = len(gb.get_int("idxb", k)) if int(dims.nb[k]) else 0
        ng, ns, nbu = int(dims.ng[k]), int(dims.ns[k]), int(dims.nbu[k])
        nbg = nb + ng
        idxe = list(gb.get_int("idxe", k)) if int(dims.nbx[k]) else []
        masks = []
        for f, n in (("lbu_mask", nbu), ("lbx_mask", nb - nbu), ("lg_mask", ng), ("ubu_mask", nbu), ("ubx_mask", nb - nbu), ("ug_mask", ng),
                     ("lls_mask", ns), ("lus_mask", ns)):
            o, m = _seg(gb, 0, f, k)
            masks.append(blob[o:o + m] if m else np.zeros(0))
        act = np.concatenate(masks) != 0
        for r in idxe:
            act[r] = act[nbg + r] = False
        lam, lamh = np.where(act, sol[(k, "lam")], 0.0), np.where(act, adj[(k, "lam")], 0.0)
        u, x, uh, xh = sol[(k, "u")], sol[(k, "x")], adj[(k, "u")], adj[(k, "x")]
        if k < N:
            put("A", k, np.outer(adj[(k, "pi")], x) + np.outer(sol[(k, "pi")], xh))
            put("B", k, np.outer(adj[(k, "pi")], u) + np.outer(sol[(k, "pi")], uh))
            put("b", k, adj[(k, "pi")])
        put("Q", k, 0.5 * (np.outer(xh, x) + np.outer(x, xh)))
        put("R", k, 0.5 * (np.outer(uh, u) + np.outer(u, uh)))
        put("S", k, np.outer(uh, x) + np.outer(u, xh))
        put("q", k, xh); put("r", k, uh)
        lo, up = lamh[:nbg], lamh[nbg:2 * nbg]
        put("lbu", k, lo[:nbu]); put("lbx", k, lo[nbu:nb]); put("lg", k, lo[nb:])
        put("ubu", k, -up[:nbu]); put("ubx", k, -up[nbu:nb]); put("ug", k, -up[nb:])
        if ng:
            dl, dlh = lam[nbg + nb:2 * nbg] - lam[nb:nbg], up[nb:] - lo[nb:]
            put("D", k, np.outer(dlh, u) + np.outer(dl, uh)); put("C", k, np.outer(dlh, x) + np.outer(dl, xh))
        if ns:
            sl, su, slh, suh = sol[(k, "sl")], sol[(k, "su")], adj[(k, "sl")], adj[(k, "su")]
            put("Zl", k, slh * sl); put("Zu", k, suh * su); put("zl", k, slh); put("zu", k, suh)
            put("lls", k, lamh[2 * nbg:2 * nbg + ns]); put("lus", k, lamh[2 * nbg + ns:])
        for r in idxe:
            for f in ("lbx", "ubx"):
                o, _ = _seg(gb, 0, f, k)
                g[o + r - nbu] = 0.0
    return g


def _mask_value_segments(gb, g):
    """the x0 value entries (checked separately against forward directions)"""
    g = g.copy()
    for k in range(gb.N + 1):
        o, n = _seg(gb, 0, "lbx#value", k)
        if n:
            g[..., o:o + n] = 0.0
    return g


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ------------------------------------------------------------------------------------------------------------------
# CPU tier: the kernel sources under the host simulation
# ------------------------------------------------------------------------------------------------------------------

STRUCT_SEEDS = [3, 5, 8, 11, 17, 23]
# seeds 17 and 23 hold ACTIVE soft general rows: the stage matrix H + sum Gamma a a' has condition ~ Gamma = lam / t, and a
# direction out of its Cholesky factor carries Gamma * eps of rounding against the dense solve (the bar of
# test_kkt_sens.py::test_sensitivities_soft_and_general_rows_vs_dense); the contraction itself is checked to rounding on all
DENSE_BAR = {17: 1e-4, 23: 1e-4}


def _struct_batch(L, seed, B=2, tol=1e-10):
    from acados_amd import OcpQpGpuBatch
    qps = [random_structure_qp(seed)] * B
    gb = OcpQpGpuBatch.from_qps(qps, _clib=L)
    _tight(gb, tol, 100)
    return gb, qps


def test_random_structures_cover_the_cases():
    """the structures below hold general rows, shared slacks, one-sided masks and an equality-flagged x0"""
    seen = set()
    for s in STRUCT_SEEDS:
        qp = random_structure_qp(s)
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
    assert seen == {"general", "shared", "one-sided", "x0"}, seen


@pytest.mark.parametrize("seed", STRUCT_SEEDS)
def test_data_grad_vs_dense_adjoint_hostsim(hostsim_lib, seed):
    """gradient blob vs the dense adjoint at the solver's own iterate (1e-9 relative to max(1, |g|)), and the contraction
    alone vs its NumPy restatement on the solver's own direction (rounding)"""
    gb, qps = _struct_batch(hostsim_lib, seed, tol=1e-10 if seed not in DENSE_BAR else 1e-8)
    assert gb.solve() == 0
    cot = random_cot(gb, np.random.default_rng(seed))
    g = gb.data_grad(cot)
    assert g.shape == (2, gb.bulk_len(0)) and np.all(np.isfinite(g))
    for i in range(2):
        own = contraction_numpy(gb, i, cot[i])
        assert _rel(_mask_value_segments(gb, g[i]), _mask_value_segments(gb, own)) <= 1e-12
        ref = dense_grad(gb, qps[i], i, cot[i])
        err = _rel(g[i], ref)
        assert err <= DENSE_BAR.get(seed, 1e-9), (seed, i, err)


def test_data_grad_one_instance_per_lane_hostsim(hostsim_lib, monkeypatch):
    """the sliced path: a one-instance-per-lane batch runs its adjoint sweeps in slices of a wave-per-instance sub-batch"""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, lqr_instance_qp, random_lqr_batch
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")
    monkeypatch.setenv("ACADOS_AMD_SENS_SLICE", "2")
    N, B = 4, 5
    data = random_lqr_batch(N=N, batch=B, seed=21)
    gb = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, _clib=hostsim_lib)
    fill_lqr_batch(gb, data, N)
    _tight(gb, 1e-10)
    assert gb.solve() == 0
    assert gb.kernel_name.startswith("1tpi")
    cot = random_cot(gb, np.random.default_rng(2))
    g = gb.data_grad(cot)
    for i in (0, 3, 4):
        err = _rel(g[i], dense_grad(gb, lqr_instance_qp(data, i, N), i, cot[i]))
        assert err <= 1e-9, (i, err)


def test_data_grad_refuses_multiplier_cotangents_and_zeroes_failed_rows(hostsim_lib):
    """a nonzero cotangent on pi / lam / t is refused (not ignored); an instance whose solve failed gets a zero row"""
    gb, _ = _struct_batch(hostsim_lib, 5, B=3)
    assert gb.solve() == 0
    cot = random_cot(gb, np.random.default_rng(0))
    bad = cot.copy()
    o, n = _seg(gb, 1, "lam", 0)
    bad[1, o] = 1.0
    with pytest.raises(RuntimeError):
        gb.data_grad(bad)
    g = gb.data_grad(cot)          # the refused seed left nothing behind
    assert np.all(np.isfinite(g)) and np.any(g[1] != 0)
    gb.opts_set("iter_max", 1)     # nothing converges in one iteration
    assert gb.solve() == 3
    g = gb.data_grad(cot)
    assert np.all(g == 0.0)


# ------------------------------------------------------------------------------------------------------------------
# GPU tier: the product library
# ------------------------------------------------------------------------------------------------------------------

def _gpu_case(name):
    from acados_amd import OcpQpGpuBatch
    from acados_amd import generators as G
    if name in ("c2_1tpi", "w16_box", "ric0", "pcond"):
        N, B = {"c2_1tpi": (10, 16384), "w16_box": (10, 1024), "ric0": (10, 512), "pcond": (20, 1024)}[name]
        data = G.random_lqr_batch(N=N, batch=B, seed=7)
        gb = OcpQpGpuBatch(G.lqr_dims(N, 8, 3), B, device=0)
        G.fill_lqr_batch(gb, data, N)
        inst = lambda i: G.lqr_instance_qp(data, i, N)
    else:
        N, B = 4, 1024
        data = G.chain_soft_batch(N=N, batch=B, seed=1)
        gb = OcpQpGpuBatch(G.chain_soft_dims(N), B, device=0)
        G.fill_chain_soft_batch(gb, data, N)
        gb.opts_set("tol_comp_soft_scale", 1.0)
        inst = lambda i: G.chain_soft_instance_qp(data, i, N)
    if name == "ric0":
        gb.opts_set("ric_alg", 0)
    if name == "pcond":
        gb.opts_set("cond_N", 5)
    return gb, inst


GPU_CASES = {"c2_1tpi": ("0", "0", "1tpi"), "w16_box": ("1", "1", "w16-box"), "chain_soft": ("1", "0", "wpi-gen"),
             "ric0": ("1", "0", None), "pcond": ("0", "0", None)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GPU_CASES))
def test_data_grad_vs_dense_adjoint_gpu(gpu_lib, monkeypatch, case):
    """every kernel family the adjoint runs in (one instance per lane through the sliced path, sixteen lanes, wave per
    instance with general soft rows, classical Riccati, after partial condensing): gradient blob vs the dense adjoint at the
    device's own solution on sampled instances"""
    wpi, w16, fam = GPU_CASES[case]
    monkeypatch.setenv("ACADOS_AMD_WPI", wpi)
    monkeypatch.setenv("ACADOS_AMD_W16", w16)
    gb, inst = _gpu_case(case)
    soft = case == "chain_soft"
    _tight(gb, 1e-8 if soft else 1e-10, 100)
    assert gb.solve() == 0
    if fam:
        assert gb.kernel_name.startswith(fam), gb.kernel_name
    if case == "ric0":
        assert ",ric0" in gb.kernel_name
    cot = random_cot(gb, np.random.default_rng(1))
    g = gb.data_grad(cot)
    sample = np.random.default_rng(2).choice(gb.n_batch, 4, replace=False)
    for i in sample:
        ref = dense_grad(gb, inst(int(i)), int(i), cot[i], x0=False)
        err = _rel(_mask_value_segments(gb, g[i]), ref)
        assert err <= (1e-4 if soft else 1e-7), (case, int(i), err)
    # the contraction alone, on the solver's own direction
    own = contraction_numpy(gb, int(sample[0]), cot[sample[0]])
    assert _rel(_mask_value_segments(gb, g[sample[0]]), _mask_value_segments(gb, own)) <= 1e-12


@pytest.mark.gpu
def test_data_grad_central_differences_gpu(gpu_lib, monkeypatch):
    """central differences of L = cot . solution on 64 random blob entries (symmetric pairs for Q / R), every entry
    re-solved at 1e-11; only instances whose active set does not move are compared"""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch
    N, B = 10, 8
    data = random_lqr_batch(N=N, batch=B, seed=5)
    gb = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, device=0)
    fill_lqr_batch(gb, data, N)
    _tight(gb, 1e-11, 100)
    assert gb.solve() == 0
    blob, sol = gb.get_bulk_in(), gb.get_bulk()
    cot = random_cot(gb, np.random.default_rng(4))
    g = gb.data_grad(cot)
    lam_idx = np.concatenate([np.arange(*(lambda o, n: (o, o + n))(*gb.bulk_offset(1, "lam", k))) for k in range(N + 1)])
    act0 = sol[:, lam_idx] > 1e-6
    segs = []
    for k in range(N + 1):
        for f in ("A", "B", "b", "Q", "S", "R", "q", "r", "lbu", "ubu", "lbx#value"):
            o, n = gb.bulk_offset(0, f, k)
            if n > 0:
                segs.append((f, o, n))
    rng = np.random.default_rng(6)
    h, checked = 1e-5, 0

    def run(bl):
        b2 = gb
        b2.set_bulk(np.ascontiguousarray(bl))
        assert b2.solve() == 0
        s2 = b2.get_bulk()
        return np.sum(s2 * cot, axis=1), s2[:, lam_idx] > 1e-6

    for _ in range(64):
        f, o, n = segs[int(rng.integers(len(segs)))]
        e = int(rng.integers(n))
        idx = [o + e]
        if f in ("Q", "R"):
            d = int(round(np.sqrt(n)))
            idx = sorted({o + (e // d) * d + e % d, o + (e % d) * d + e // d})
        if f == "lbx#value":
            o2, _ = gb.bulk_offset(0, "lbx", 0)
            idx = [o + e, o2 + e]     # the bound and its value: the same number in the caller's data
        bp, bm = blob.copy(), blob.copy()
        bp[:, idx] += h
        bm[:, idx] -= h
        lp, ap = run(bp)
        lm, am = run(bm)
        fd = (lp - lm) / (2 * h)
        an = g[:, idx].sum(axis=1)
        same = np.all(ap == act0, axis=1) & np.all(am == act0, axis=1)
        for i in np.nonzero(same)[0]:
            assert abs(fd[i] - an[i]) <= 1e-5 * max(1.0, abs(fd[i])), (f, e, int(i), fd[i], an[i])
            checked += 1
    assert checked >= 64 * 4


@pytest.mark.gpu
def test_torch_autograd_gpu():
    """torch.autograd over the solve: gradcheck of a thin wrapper (q of two stages and one entry of A as inputs), a
    ten-step gradient descent on q towards a target trajectory, and a zero (not NaN) gradient for a failed instance"""
    import torch
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch
    from acados_amd.torch_qp import blob_views, qp_solve
    N, B = 6, 32
    data = random_lqr_batch(N=N, nx=4, nu=2, batch=B, seed=3)
    gb = OcpQpGpuBatch(lqr_dims(N, 4, 2), B, device=0)
    fill_lqr_batch(gb, data, N)
    _tight(gb, 1e-11, 100)
    assert gb.solve() == 0
    base = torch.from_numpy(gb.get_bulk_in()).cuda()
    o1, n1 = gb.bulk_offset(0, "q", 1)
    o3, n3 = gb.bulk_offset(0, "q", 3)
    oa, _ = gb.bulk_offset(0, "A", 2)
    ox = [gb.bulk_offset(1, "x", k) for k in range(N + 1)]

    def wrapper(q1, q3, a):
        blob = base.clone()
        blob[:, o1:o1 + n1] = q1
        blob[:, o3:o3 + n3] = q3
        blob[:, oa] = a
        sol = qp_solve(gb, blob)
        return torch.cat([sol[:, o:o + n] for o, n in ox], dim=1)

    q1 = base[:, o1:o1 + n1].clone().requires_grad_(True)
    q3 = base[:, o3:o3 + n3].clone().requires_grad_(True)
    a = base[:, oa].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(wrapper, (q1, q3, a), eps=1e-6, atol=1e-6, rtol=1e-4)
    # gradient descent on the whole q towards a target trajectory
    blob = base.clone()
    v = blob_views(gb, blob)
    assert v[("A", 0)].shape == (B, 4, 4) and torch.equal(v[("q", 1)], blob[:, o1:o1 + n1])
    target = torch.zeros((B, sum(n for _, n in ox)), dtype=torch.float64, device="cuda")
    qidx = torch.cat([torch.arange(*(lambda o, n: (o, o + n))(*gb.bulk_offset(0, "q", k))) for k in range(N + 1)]).cuda()
    qv = blob[:, qidx].clone().requires_grad_(True)
    losses = []
    for _ in range(10):
        bl = blob.clone()
        bl[:, qidx] = qv
        sol = qp_solve(gb, bl)
        x = torch.cat([sol[:, o:o + n] for o, n in ox], dim=1)
        loss = ((x - target) ** 2).sum()
        qv.grad = None
        loss.backward()
        losses.append(float(loss))
        with torch.no_grad():
            qv -= 0.05 * qv.grad
    assert all(b < a_ for a_, b in zip(losses, losses[1:])), losses
    # a failed instance: zero row, not NaN
    gb.opts_set("iter_max", 1)
    bl = blob.clone().requires_grad_(True)
    sol = qp_solve(gb, bl)
    x = torch.cat([sol[:, o:o + n] for o, n in ox], dim=1)
    x.sum().backward()
    st = gb.info("status")
    assert np.any(st != 0) and torch.all(torch.isfinite(bl.grad))
    assert torch.all(bl.grad[torch.from_numpy(st != 0).cuda()] == 0)

"""Reverse mode on the WHOLE output blob: cotangents on pi, lam and t (ocp_qp_gpu_batch_adj_seed_all_bulk, grad_kernels.hpp
k_adj_seed_all, OcpQpGpuBatch.data_vjp, backward of acados_amd/torch_qp.py; DESIGN.md 4.8 "Cotangents on the multipliers").

The definition is the reference: data_vjp(g) is the input-blob row v with <v, t> = <g, data_jvp(t)> for every tangent t, and
data_jvp is pinned against a dense linearised KKT solve by tests/test_data_jvp.py.  So the tests are dot-product identities against
data_jvp, bit comparisons against data_grad where the cotangent is zero on pi lam t, and bit comparisons of the result with and
without cotangents that must be ignored.

The identity holds to the noise of d lam = -(lam / t) dt on active sides (eps lam / t, tenfold per digit of the solve tolerance:
tests/test_data_jvp.py), not to rounding.  existing_path_defect measures that noise on the sensitivity sweeps alone (no kernel of
this file's subject runs in it): the bars of the GPU tier are ten times its value per case, rounded up to a power of ten and never
looser than 1e-4 (profiles/NOTES.md, "Data VJP", holds the measured values)."""
import ctypes as C

import numpy as np
import pytest

from test_data_grad import DENSE_BAR, STRUCT_SEEDS, VEC_OUT, _seg, _struct_batch, _tight, random_cot
from test_data_jvp import TIERS, _lane_batch, _sens_seg, _solved_struct, _stage_info, clib, random_tangent, sens_bulk  # noqa: F401

LOWER, UPPER = ("lbu", "lbx", "lg"), ("ubu", "ubx", "ug")


def full_cot(gb, rng):
    """a standard normal cotangent on EVERY entry of the output blob"""
    return rng.standard_normal((gb.n_batch, gb.bulk_len(1)))


def only(gb, cot, fields):
    """cot with every field but `fields` set to zero"""
    out = np.zeros_like(cot)
    for k in range(gb.N + 1):
        for f in fields:
            o, n = _seg(gb, 1, f, k)
            if n:
                out[:, o:o + n] = cot[:, o:o + n]
    return out


def takes_part(gb):
    """[n_batch, bulk_len(1)] bool: False for lam / t of the sides outside the activity mask and of equality-flagged rows, and for
    the equality-flagged variables themselves"""
    blob_in = gb.get_bulk_in()
    on = np.ones((gb.n_batch, gb.bulk_len(1)), dtype=bool)
    for k in range(gb.N + 1):
        nu = int(gb.dims.nu[k])
        for i in range(gb.n_batch):
            nbu, nb, ng, ns, idxe, act = _stage_info(gb, k, blob_in[i])
            for f in ("lam", "t"):
                o, n = _seg(gb, 1, f, k)
                if n:
                    on[i, o:o + n] = act
            for r in idxe:
                v = int(gb.get_int("idxb", k)[r])
                o, _ = _seg(gb, 1, "u" if v < nu else "x", k)
                on[i, o + (v if v < nu else v - nu)] = False
    return on


def output_to_seed(gb):
    """the map under which the sensitivity solve is symmetric: (output entry, seed entry, sign) -- u x sl su pi to the seed of r q zl
    zu b with +, lam of a lower side (lbu lbx lg lls lus) to + its natural-sign bound seed, lam of an upper side to - its seed"""
    rows = []
    for k in range(gb.N + 1):
        for fo, fs in (("u", "r"), ("x", "q"), ("sl", "zl"), ("su", "zu"), ("pi", "b")):
            (o, n), (os_, m) = _seg(gb, 1, fo, k), _sens_seg(gb, fs, k)
            assert n == m, (fo, k)
            rows += [(o + e, os_ + e, 1.0) for e in range(n)]
        ol, nl = _seg(gb, 1, "lam", k)
        pos = 0
        for fs in LOWER + UPPER + ("lls", "lus"):
            os_, m = _sens_seg(gb, fs, k)
            rows += [(ol + pos + e, os_ + e, -1.0 if fs in UPPER else 1.0) for e in range(m)]
            pos += m
        assert pos == nl, (k, pos, nl)
    out, seed, sign = (np.array(c) for c in zip(*rows))
    return out.astype(int), seed.astype(int), sign.astype(float)


def existing_path_defect(gb, rng):
    """what the sensitivity sweeps alone leave of the symmetry the new entry relies on (no data_vjp, no data_jvp): seed with the
    mapped cotangent g, read the directions back through the same map, and compare <g, sens(s)> with <mapped sens(mapped g), s> for a
    random seed set s, per instance; cotangent and seeds of what takes no part are zero.  Worst |a - b| / (sum |g D| + sum |grad s|)"""
    out, seed, sign = output_to_seed(gb)
    on = takes_part(gb)[:, out]
    slen = gb._L.ocp_qp_gpu_batch_sens_bulk_len(gb._h, 0)
    g, s = np.zeros((gb.n_batch, gb.bulk_len(1))), np.zeros((gb.n_batch, slen))
    g[:, out] = np.where(on, rng.standard_normal(on.shape), 0.0)
    s[:, seed] = np.where(on, rng.standard_normal(on.shape), 0.0)
    mapped = np.zeros_like(s)
    mapped[:, seed] = sign * g[:, out]
    D = sens_bulk(gb, s)
    grad = np.zeros_like(s)
    grad[:, seed] = sign * np.where(on, sens_bulk(gb, mapped)[:, out], 0.0)
    a, b = np.sum(g * D, axis=1), np.sum(grad * s, axis=1)
    den = np.sum(np.abs(g * D), axis=1) + np.sum(np.abs(grad * s), axis=1)
    assert np.all(den > 0)
    return float(np.max(np.abs(a - b) / den))


def check_identity(gb, t, g, bar, what=""):
    """<g, data_jvp(t)> against <data_vjp(g), t> per instance, the ratio of test_data_jvp.check_dot_product; returns data_vjp(g)"""
    jv = gb.data_jvp(t)
    v = gb.data_vjp(g)
    a, b = np.sum(g * jv, axis=1), np.sum(v * t, axis=1)
    den = np.sum(np.abs(g * jv), axis=1) + np.sum(np.abs(v * t), axis=1)
    assert np.all(den > 0) and np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    ratio = np.abs(a - b) / den
    print(f"data_vjp dot product{what}: worst |a - b| / (sum |g jvp| + sum |vjp t|) = {ratio.max():.2e} (bar {bar:.0e})")
    assert np.all(np.abs(a - b) <= bar * den), (int(np.argmax(ratio)), float(ratio.max()))
    return v


def check_full_cotangent(gb, rng, bar, what=""):
    """test 1: a full cotangent meets the identity, and the multipliers' part of it is not ignored"""
    g = full_cot(gb, rng)
    v = check_identity(gb, random_tangent(gb, rng), g, bar, what)
    primal = gb.data_grad(only(gb, g, VEC_OUT))
    assert all(not np.array_equal(v[i], primal[i]) for i in range(gb.n_batch))


# ------------------------------------------------------------------------------------------------------------------
# CPU tier: the kernel sources under the host simulation
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", STRUCT_SEEDS)
def test_vjp_full_cotangent_hostsim(hostsim_lib, seed):
    """test 1 at a solve tolerance of 1e-6: the sweeps alone measure <= 8.2e-8 there (existing_path_defect, restricted cotangents
    included); the bar of 1e-6 leaves a factor of 12 for the matrix terms of the contraction"""
    gb, _ = _struct_batch(hostsim_lib, seed, tol=1e-6)
    assert gb.solve() == 0
    check_full_cotangent(gb, np.random.default_rng(400 + seed), 1e-6)


def test_vjp_full_cotangent_one_instance_per_lane_hostsim(hostsim_lib, monkeypatch):
    """test 1 through the sliced path of a one-instance-per-lane batch"""
    gb, _ = _lane_batch(hostsim_lib, monkeypatch)
    _tight(gb, 1e-6, 100)
    assert gb.solve() == 0
    assert gb.kernel_name.startswith("1tpi")
    check_full_cotangent(gb, np.random.default_rng(5), 1e-6)


@pytest.mark.parametrize("seed", STRUCT_SEEDS)
def test_vjp_t_only_and_primal_only_hostsim(hostsim_lib, seed):
    """test 2: where the noise of d lam does not enter -- a cotangent on t alone (the fold), one on u x sl su alone -- the identity
    holds with the bars of test_jvp_dot_product_hostsim at its tolerances"""
    gb, _ = _solved_struct(hostsim_lib, seed)
    rng = np.random.default_rng(500 + seed)
    g, t = full_cot(gb, rng), random_tangent(gb, rng)
    bar = DENSE_BAR.get(seed, 1e-9)
    vt = check_identity(gb, t, only(gb, g, ("t",)), bar, " (t alone)")
    assert np.any(vt != 0)
    check_identity(gb, t, only(gb, g, VEC_OUT), bar, " (u x sl su alone)")


# ------------------------------------------------------------------------------------------------------------------
# both tiers: bits against data_grad, cotangents that are ignored, a failed instance, the state left behind
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_vjp_bits_of_data_grad(clib):
    """test 3: a cotangent that is zero on pi lam t gives the bits of data_grad"""
    for seed in (5, 17):
        gb, _ = _solved_struct(clib, seed)
        cot = random_cot(gb, np.random.default_rng(600 + seed))
        want = gb.data_grad(cot)
        assert np.array_equal(gb.data_vjp(cot), want) and np.any(want != 0)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_vjp_ignores_sides_that_take_no_part(clib):
    """test 4: cotangents on lam and t of masked sides and of equality-flagged rows change no bit of the result (seed 5 holds an
    equality-flagged x0; one-sided masks: test_data_grad.test_random_structures_cover_the_cases)"""
    seen_eq = seen_mask = False
    for seed in STRUCT_SEEDS:
        gb, qps = _solved_struct(clib, seed)
        rng = np.random.default_rng(700 + seed)
        g = full_cot(gb, rng)
        off = ~takes_part(gb)
        for f in VEC_OUT + ("pi",):     # (an equality-flagged variable's own cotangent does count: only lam and t are dropped)
            for k in range(gb.N + 1):
                o, n = _seg(gb, 1, f, k)
                if n:
                    off[:, o:o + n] = False
        if not off.any():
            continue
        seen_eq |= any(len(qps[0].idxe[k]) for k in range(gb.N + 1))
        seen_mask |= any(np.any(np.asarray(getattr(qps[0], f)[k]) == 0) for k in range(gb.N + 1)
                         for f in ("lbu_mask", "ubu_mask", "lbx_mask", "ubx_mask", "lg_mask", "ug_mask"))
        base = np.where(off, 0.0, g)
        want = gb.data_vjp(base)
        assert np.array_equal(gb.data_vjp(g), want) and np.any(want != 0), seed
    assert seen_eq and seen_mask


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_vjp_failed_instance_and_state_left_behind(clib):
    """test 5: a NaN in q of the middle instance gives a zero row and leaves the others those of a clean batch; the adjoint seed is
    used up by its _data_grad_bulk; data_grad, data_jvp and a re-solve afterwards are those of a batch that never ran data_vjp;
    data_grad still refuses a multiplier cotangent"""
    clean, _ = _struct_batch(clib, 5, B=3)
    bad, _ = _struct_batch(clib, 5, B=3)
    fresh, _ = _struct_batch(clib, 5, B=3)
    q = bad.get("q", 1)
    q[1, 0] = np.nan
    bad.set("q", 1, q)
    assert clean.solve() == 0 and fresh.solve() == 0
    assert bad.solve() == 1
    st = bad.info("status")
    assert st[1] != 0 and st[0] == 0 and st[2] == 0
    rng = np.random.default_rng(8)
    g, t, cot = full_cot(clean, rng), random_tangent(clean, rng), random_cot(clean, rng)
    want, got = clean.data_vjp(g), bad.data_vjp(g)
    assert np.all(got[1] == 0.0)
    assert np.array_equal(got[[0, 2]], want[[0, 2]]) and np.any(want[1] != 0)
    assert np.array_equal(clean.data_vjp(g), want)      # the same bits twice
    L = clean._L
    grad = np.zeros((clean.n_batch, clean.bulk_len(0)))
    assert L.ocp_qp_gpu_batch_data_grad_bulk(clean._h, grad.ctypes.data_as(C.c_void_p), 0) == -1   # the seed was used up
    assert L.ocp_qp_gpu_batch_adj_seed_all_bulk(clean._h, g.ctypes.data_as(C.c_void_p), 0) == 0
    assert L.ocp_qp_gpu_batch_data_grad_bulk(clean._h, grad.ctypes.data_as(C.c_void_p), 0) == 0
    assert np.array_equal(grad, want)
    assert L.ocp_qp_gpu_batch_data_grad_bulk(clean._h, grad.ctypes.data_as(C.c_void_p), 0) == -1
    assert np.array_equal(clean.data_grad(cot), fresh.data_grad(cot))
    assert np.array_equal(clean.data_jvp(t), fresh.data_jvp(t))
    refused = cot.copy()
    refused[1, _seg(clean, 1, "lam", 0)[0]] = 1.0
    with pytest.raises(RuntimeError):
        clean.data_grad(refused)
    assert np.array_equal(clean.data_grad(cot), fresh.data_grad(cot))
    assert clean.solve() == 0 and fresh.solve() == 0
    assert np.array_equal(clean.info("iter"), fresh.info("iter"))
    assert np.array_equal(clean.get_bulk(), fresh.get_bulk())


# ------------------------------------------------------------------------------------------------------------------
# GPU tier: the product library
# ------------------------------------------------------------------------------------------------------------------

# case: (ACADOS_AMD_WPI, ACADOS_AMD_W16, kernel family, option, what the sweeps alone measured, the bar: ten times that, rounded up to
# a power of ten, capped at 1e-4 -- the project's bar for active general rows).  LQR nx 8 nu 3, N 4, 130 instances: two full tiles plus
# two, sensitivity slices of 64 (ragged); chain_soft_batch N 4, 66 instances.  All solved at 1e-6.
VJP_GPU_CASES = {
    "1tpi": ("0", "0", "1tpi", None, 5.56e-8, 1e-6),
    "w16_box": ("1", "1", "w16-box", None, 7.26e-8, 1e-6),
    "ric0": ("1", "0", None, ("ric_alg", 0), 3.66e-8, 1e-6),
    "pcond": ("0", "0", None, ("cond_N", 2), 4.01e-8, 1e-6),
    "wpi_gen": ("1", "0", "wpi-gen", None, 7.01e-8, 1e-6),
}


def _vjp_gpu_case(monkeypatch, case):
    from acados_amd import OcpQpGpuBatch
    from acados_amd import generators as G
    wpi, w16, fam, opt, _, bar = VJP_GPU_CASES[case]
    monkeypatch.setenv("ACADOS_AMD_WPI", wpi)
    monkeypatch.setenv("ACADOS_AMD_W16", w16)
    monkeypatch.setenv("ACADOS_AMD_SENS_SLICE", "64")
    N = 4
    if case == "wpi_gen":
        B = 66
        gb = OcpQpGpuBatch(G.chain_soft_dims(N), B, device=0)
        G.fill_chain_soft_batch(gb, G.chain_soft_batch(N=N, batch=B, seed=1), N)
        gb.opts_set("tol_comp_soft_scale", 1.0)
    else:
        B = 130
        gb = OcpQpGpuBatch(G.lqr_dims(N, 8, 3), B, device=0)
        G.fill_lqr_batch(gb, G.random_lqr_batch(N=N, batch=B, seed=7), N)
    if opt:
        gb.opts_set(*opt)
    _tight(gb, 1e-6, 100)
    assert gb.solve() == 0
    if fam:
        assert gb.kernel_name.startswith(fam), gb.kernel_name
    if case == "ric0":
        assert ",ric0" in gb.kernel_name, gb.kernel_name
    if case == "pcond":
        assert gb.condensed_kernel_name(), gb.kernel_name
    return gb, bar


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(VJP_GPU_CASES))
def test_vjp_full_cotangent_gpu(gpu_lib, monkeypatch, case):
    """test 6: the identity of test 1 on every kernel family the adjoint runs in, with the bar of the case"""
    gb, bar = _vjp_gpu_case(monkeypatch, case)
    print(f"{case}: kernel {gb.kernel_name}, sweeps alone {existing_path_defect(gb, np.random.default_rng(9)):.2e}")
    check_full_cotangent(gb, np.random.default_rng(10), bar, f" ({case})")


@pytest.mark.gpu
def test_vjp_torch_backward_gpu(gpu_lib):
    """test 7: backward of a loss that reads pi, lam and t entries gives the bits of data_vjp of the same cotangent"""
    import torch
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch
    from acados_amd.torch_qp import qp_solve
    N, B = 6, 32
    gb = OcpQpGpuBatch(lqr_dims(N, 4, 2), B, device=0)
    fill_lqr_batch(gb, random_lqr_batch(N=N, nx=4, nu=2, batch=B, seed=3), N)
    _tight(gb, 1e-8, 100)
    assert gb.solve() == 0
    blob = torch.from_numpy(gb.get_bulk_in()).cuda().requires_grad_(True)
    w = torch.from_numpy(only(gb, full_cot(gb, np.random.default_rng(11)), ("x", "pi", "lam", "t"))).cuda()
    for f in ("pi", "lam", "t"):
        o, n = gb.bulk_offset(1, f, 1)
        assert n > 0 and bool((w[:, o:o + n] != 0).all())
    sol = qp_solve(gb, blob)
    (w * sol).sum().backward()
    want = gb.data_vjp(w)
    assert want.is_cuda and bool(torch.isfinite(want).all()) and bool((want != 0).any())
    assert torch.equal(blob.grad, want)
    assert np.array_equal(want.cpu().numpy(), gb.data_vjp(w.cpu().numpy()))      # host arrays and CUDA tensors alike

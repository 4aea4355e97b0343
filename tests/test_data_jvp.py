"""Forward-mode derivative of the QP solution along a tangent of all QP data (ocp_qp_gpu_batch_data_jvp_bulk, grad_kernels.hpp
k_data_tangent, acados_amd/torch_qp.py; DESIGN.md "Data gradients", Forward mode).

References that are not the tangent kernel:
  * the bulk sensitivity path (_sens_set_bulk -> _sens_solve -> _sens_get_bulk) for tangents in the vector data: bit for bit;
  * ONE dense solve of the linearised KKT system (tests/dense_ref.py sens_dense) seeded with the seed table of DESIGN.md restated
    in NumPy, at the oracle's solution and at the batch's own iterate, through test_kkt_sens._check_sens with that file's bars;
  * reverse mode: <g, data_jvp(t)> = <data_grad(g), t> (data_grad is pinned against a dense adjoint and central differences by
    tests/test_data_grad.py).
Tangents are standard normal on EVERY entry of the input blob: masks and index entries (ignored), both triangles of Q and R drawn
independently, the bound entries and the value entry of an equality-flagged row.

Measured (worst ratio |a - b| / (sum |g jvp| + sum |grad t|) of the dot-product test, worst deviation of case 2 from the dense solve
at the oracle's solution): profiles/NOTES.md, "Data JVP"."""
import ctypes as C

import numpy as np
import pytest

from test_data_grad import DENSE_BAR, GPU_CASES, STRUCT_SEEDS, _gpu_case, _seg, _struct_batch, _tight, random_cot
from test_kkt_sens import _check_sens

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
SEED_FIELDS = ("r", "q", "zl", "zu", "b", "lbu", "lbx", "lg", "ubu", "ubx", "ug", "lls", "lus")
OUT_FIELDS = ("u", "x", "sl", "su", "pi", "lam", "t")
# the bars of tests/test_kkt_sens.py for seed sets that move bounds (ours move every bound): test_sensitivities_box_vs_dense
# (tol 1e-6, multipliers 1e-2 where an active bound moves) and test_sensitivities_soft_and_general_rows_vs_dense (2e-4; multipliers
# 1e-3 where the bound of a general row moves) -- selected as tests/test_full_dense.py case (h) selects them.
# The bars belong to the tolerance those tests solve at (DENSE_TOL: 1e-9 / 1e-8, the oracle's too): d lam = -(lam / t) d t of an
# active side carries eps * Gamma, Gamma = lam / t, which grows tenfold with every digit of tol_comp (measured under host simulation
# on the C2 class, d lam against the dense solve at the oracle's solution: up to 1e-3 at 1e-9, 1.1e-2 at 1e-10).  The dense
# comparison therefore re-solves at that tolerance; the other cases keep the tolerances of tests/test_data_grad.py.
BOX_BARS = dict(tol=1e-6, tol_mult_own=1e-2, tol_mult=1e-2)
GEN_BARS = dict(tol=2e-4, tol_own=2e-4, tol_mult_own=1e-3, tol_mult=1e-3, tol_solve=1e-8)
DENSE_TOL = {False: 1e-9, True: 1e-8}   # by class: general rows / slacks active or not


@pytest.fixture
def clib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


def _is_gpu(request):
    return "gpu" in request.node.callspec.id.split("-")


def random_tangent(gb, rng):
    return rng.standard_normal((gb.n_batch, gb.bulk_len(0)))


def _sens_seg(gb, f, k):
    n = C.c_int(0)
    o = gb._L.ocp_qp_gpu_batch_sens_bulk_offset(gb._h, 0, ("seed_" + f).encode(), int(k), C.byref(n))
    return (int(o), int(n.value)) if n.value > 0 else (None, 0)


def sens_bulk(gb, seeds):
    """the existing bulk sensitivity path: every seed in one blob, the sweeps, every direction in one blob"""
    L = gb._L
    seeds = np.ascontiguousarray(seeds)
    assert seeds.shape == (gb.n_batch, L.ocp_qp_gpu_batch_sens_bulk_len(gb._h, 0))
    assert L.ocp_qp_gpu_batch_sens_set_bulk(gb._h, seeds.ctypes.data_as(C.c_void_p), 0) == 0
    gb.sens_solve()
    out = np.zeros((gb.n_batch, gb.bulk_len(1)))
    assert L.ocp_qp_gpu_batch_sens_get_bulk(gb._h, out.ctypes.data_as(C.c_void_p), 0) == 0
    return out


def _stage_info(gb, k, blob_in_row):
    """(nbu, nb, ng, ns, equality-flagged rows, sides that take part) of stage k of one instance"""
    d = gb.dims
    nb = len(gb.get_int("idxb", k)) if int(d.nb[k]) else 0
    ng, ns, nbu = int(d.ng[k]), int(d.ns[k]), int(d.nbu[k])
    idxe = [int(r) for r in gb.get_int("idxe", k)] if int(d.nbx[k]) else []
    masks = []
    for f in ("lbu_mask", "lbx_mask", "lg_mask", "ubu_mask", "ubx_mask", "ug_mask", "lls_mask", "lus_mask"):
        o, m = _seg(gb, 0, f, k)
        masks.append(blob_in_row[o:o + m] if m else np.zeros(0))
    act = np.concatenate(masks) != 0
    for r in idxe:
        act[r] = act[nb + ng + r] = False
    return nbu, nb, ng, ns, idxe, act


def seed_table(gb, i, t, sol, blob_in, gated=True):
    """the seed table of DESIGN.md 4.8 "Forward mode" in NumPy for instance i: {(seed field, stage): vector} from the tangent row t,
    the solution row sol (output blob) and the masks of the input blob row.  gated: the seeds of sides that take no part are 0 (what the
    kernel writes); the dense reference leaves such sides out by itself"""
    N, d = gb.N, gb.dims
    seeds = {}

    def tin(f, k, shape=None):
        o, n = _seg(gb, 0, f, k)
        v = t[o:o + n].copy() if n else np.zeros(0)
        return v.reshape(shape, order="F") if shape is not None else v

    def out(f, k):
        o, n = _seg(gb, 1, f, k)
        return sol[o:o + n] if n else np.zeros(0)

    for k in range(N + 1):
        nu, nx = int(d.nu[k]), int(d.nx[k])
        nbu, nb, ng, ns, idxe, act = _stage_info(gb, k, blob_in)
        nbg = nb + ng
        u, x, sl, su = out("u", k), out("x", k), out("sl", k), out("su", k)
        lam = np.where(act, out("lam", k), 0.0)
        Qd, Rd, Sd = tin("Q", k, (nx, nx)), tin("R", k, (nu, nu)), tin("S", k, (nu, nx))
        sr = tin("r", k) + 0.5 * (Rd + Rd.T) @ u + Sd @ x
        sq = tin("q", k) + 0.5 * (Qd + Qd.T) @ x + Sd.T @ u
        if k < N:
            nx1 = int(d.nx[k + 1])
            Ad, Bd, pi = tin("A", k, (nx1, nx)), tin("B", k, (nx1, nu)), out("pi", k)
            sr, sq = sr + Bd.T @ pi, sq + Ad.T @ pi
            seeds[("b", k)] = tin("b", k) + Ad @ x + Bd @ u
        lo = {"lbu": tin("lbu", k), "lbx": tin("lbx", k).copy(), "lg": tin("lg", k)}
        up = {"ubu": tin("ubu", k), "ubx": tin("ubx", k).copy(), "ug": tin("ug", k)}
        if ng:
            Cd, Dd = tin("C", k, (ng, nx)), tin("D", k, (ng, nu))
            dl = lam[nbg + nb:2 * nbg] - lam[nb:nbg]
            sr, sq = sr + Dd.T @ dl, sq + Cd.T @ dl
            lo["lg"] = lo["lg"] - (Cd @ x + Dd @ u)
            up["ug"] = up["ug"] - (Cd @ x + Dd @ u)
        for r in idxe:   # an equality-flagged row: seed_lbx is the tangent of the variable's value, the bounds take no part
            lo["lbx"][r - nbu] = tin("lbx#value", k)[r - nbu]
            up["ubx"][r - nbu] = 0.0
        slack = {}
        if ns:
            seeds[("zl", k)] = tin("zl", k) + tin("Zl", k) * sl
            seeds[("zu", k)] = tin("zu", k) + tin("Zu", k) * su
            slack = {"lls": tin("lls", k), "lus": tin("lus", k)}
        if gated:
            on = act.copy()
            for r in idxe:
                on[r] = True   # (the lower side of the row carries the value seed)
            for (f, v), a in zip(list(lo.items()) + list(up.items()) + list(slack.items()),
                                 (on[:nbu], on[nbu:nb], on[nb:nbg], on[nbg:nbg + nbu], on[nbg + nbu:nbg + nb], on[nbg + nb:2 * nbg],
                                  on[2 * nbg:2 * nbg + ns], on[2 * nbg + ns:])):
                v[...] = np.where(a, v, 0.0) if v.size else v
        seeds[("r", k)], seeds[("q", k)] = sr, sq
        for f, v in list(lo.items()) + list(up.items()) + list(slack.items()):
            seeds[(f, k)] = v
    return seeds


def seed_blob(gb, seeds_per_instance):
    """{(field, stage): vector} of every instance -> the seed blob of _sens_set_bulk"""
    blob = np.zeros((gb.n_batch, gb._L.ocp_qp_gpu_batch_sens_bulk_len(gb._h, 0)))
    for i, seeds in enumerate(seeds_per_instance):
        for (f, k), v in seeds.items():
            o, n = _sens_seg(gb, f, k)
            assert n == v.size, (f, k, n, v.size)
            if n:
                blob[i, o:o + n] = v
    return blob


def vector_only(gb, t):
    """t with every matrix entry (A B Q S R C D Zl Zu) set to zero"""
    v = t.copy()
    for k in range(gb.N + 1):
        for f in ("A", "B", "Q", "S", "R", "C", "D", "Zl", "Zu"):
            o, n = _seg(gb, 0, f, k)
            if n:
                v[:, o:o + n] = 0.0
    return v


class _JvpAsSens:
    """what _check_sens drives: sens_solve runs the JVP, sens_<field> is read out of the blob it returned (rows: the instances compared)"""

    def __init__(self, gb, t, rows):
        self.gb, self.t, self.rows, self.N, self.out = gb, t, list(rows), gb.N, None

    def sens_set(self, f, k, v):
        raise AssertionError("the JVP takes no single seeds")

    def sens_solve(self):
        self.out = self.gb.data_jvp(self.t)

    def get(self, f, k):
        if f.startswith("sens_"):
            o, n = self.gb.bulk_offset(1, f[5:], k)
            return self.out[self.rows, o:o + n] if n > 0 else np.zeros((len(self.rows), 0))
        return self.gb.get(f, k)[self.rows]


def check_vector_bits(gb, rng):
    """case 1: a tangent in r q zl zu b, the bounds and the value entries gives the bits of the existing bulk sensitivity path"""
    t = vector_only(gb, random_tangent(gb, rng))
    # on a vector tangent the seeds ARE the tangent, field by field (an equality-flagged row apart: seed_lbx = its value entry)
    seeds = np.zeros((gb.n_batch, gb._L.ocp_qp_gpu_batch_sens_bulk_len(gb._h, 0)))
    for k in range(gb.N + 1):
        for f in SEED_FIELDS:
            (o, n), (os_, ns_) = _seg(gb, 0, f, k), _sens_seg(gb, f, k)
            assert n == ns_, (f, k)
            if n:
                seeds[:, os_:os_ + n] = t[:, o:o + n]
        nbu = int(gb.dims.nbu[k])
        for r in ([int(r) for r in gb.get_int("idxe", k)] if int(gb.dims.nbx[k]) else []):
            seeds[:, _sens_seg(gb, "lbx", k)[0] + r - nbu] = t[:, _seg(gb, 0, "lbx#value", k)[0] + r - nbu]
            seeds[:, _sens_seg(gb, "ubx", k)[0] + r - nbu] = 0.0
    # ... and the NumPy seed table says the same
    sol, blob_in = gb.get_bulk(), gb.get_bulk_in()
    assert np.array_equal(seed_blob(gb, [seed_table(gb, 0, t[0], sol[0], blob_in[0], gated=False)])[0], seeds[0])
    want = sens_bulk(gb, seeds)
    got = gb.data_jvp(t)
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
    assert np.any(got != 0)


def check_vs_dense(gb, qps, rows, rng, gen, soft_scale=None):
    """case 2: every output field against the dense linearised solve seeded with the NumPy seed table (gen: the class of structures
    with active general rows, its bars and its tolerance)"""
    bars = GEN_BARS if gen else BOX_BARS
    _tight(gb, DENSE_TOL[gen], 100)
    assert gb.solve() == 0
    t = random_tangent(gb, rng)
    sol, blob_in = gb.get_bulk(), gb.get_bulk_in()
    per = [seed_table(gb, i, t[i], sol[i], blob_in[i], gated=False) for i in rows]
    dense = {key: np.stack([p[key] for p in per]) for key in per[0]}
    drv = _JvpAsSens(gb, t, rows)
    worst = _check_sens(drv, qps, [], dense, fields=("x", "u", "pi", "sl", "su", "lam", "t"), soft_scale=soft_scale, **bars)
    for q, i in enumerate(rows):   # sides that take no part (masked, equality-flagged): lam and t of the result are 0
        for k in range(gb.N + 1):
            act = _stage_info(gb, k, blob_in[i])[5]
            for f in ("lam", "t"):
                assert np.all(drv.get("sens_" + f, k)[q][~act] == 0.0), (i, k, f)
    print(f"data_jvp vs dense solve at the oracle's solution: worst {worst:.2e} (bar {bars['tol']:.0e})")
    assert worst <= bars["tol"], worst
    return worst


def check_dot_product(gb, rng, bar):
    """case 3: <g, jvp(t)> over u x sl su against <data_grad(g), t>, per instance"""
    t, cot = random_tangent(gb, rng), random_cot(gb, rng)
    jv = gb.data_jvp(t)
    g = gb.data_grad(cot)
    a, b = np.sum(cot * jv, axis=1), np.sum(g * t, axis=1)
    den = np.sum(np.abs(cot * jv), axis=1) + np.sum(np.abs(g * t), axis=1)
    ratio = np.abs(a - b) / den
    print(f"data_jvp dot product: worst |a - b| / (sum |g jvp| + sum |grad t|) = {ratio.max():.2e} (bar {bar:.0e})")
    assert np.all(den > 0) and np.all(np.isfinite(ratio))
    assert np.all(np.abs(a - b) <= bar * den), (int(np.argmax(ratio)), float(ratio.max()))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------
# CPU tier: the kernel sources under the host simulation
# ------------------------------------------------------------------------------------------------------------------

# structures with ACTIVE general rows at the solution (hard or soft; test_structure_classes pins the list): their stage matrix
# H + sum Gamma a a' has condition ~ Gamma = lam / t, and pi / lam out of a one-shot sensitivity solve carry Gamma * eps -- the class
# of test_sensitivities_soft_and_general_rows_vs_dense, whose bars belong to an iterate at 1e-8 (Gamma ~ 1e10; 1e14 at 1e-10), so
# the dense comparison solves these at 1e-8 as that test does.  Seed 11 holds box rows only: the box bars at 1e-10.
GEN_SEEDS = (3, 5, 8, 17, 23)


def _solved_struct(L, seed, B=2, tol=None):
    gb, qps = _struct_batch(L, seed, B=B, tol=tol or (1e-10 if seed not in DENSE_BAR else 1e-8))
    assert gb.solve() == 0
    return gb, qps


def _active_general_rows(gb):
    d, found = gb.dims, False
    for k in range(gb.N + 1):
        nb, ng = int(d.nb[k]), int(d.ng[k])
        lam, t = gb.get("lam", k), gb.get("t", k)
        for o in (nb, 2 * nb + ng):
            found |= bool(np.any(lam[:, o:o + ng] > t[:, o:o + ng]))
    return found


def test_structure_classes(hostsim_lib):
    """the class each structure's bars are chosen by is a property of its solution: an active general row or none"""
    for seed in STRUCT_SEEDS:
        gb, _ = _solved_struct(hostsim_lib, seed)
        assert _active_general_rows(gb) == (seed in GEN_SEEDS), seed


def _lane_batch(L, monkeypatch):
    """the batch of test_data_grad_one_instance_per_lane_hostsim: the sliced sub-batch path"""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, lqr_instance_qp, random_lqr_batch
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")
    monkeypatch.setenv("ACADOS_AMD_SENS_SLICE", "2")
    N, B = 4, 5
    data = random_lqr_batch(N=N, batch=B, seed=21)
    gb = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, _clib=L)
    fill_lqr_batch(gb, data, N)
    _tight(gb, 1e-10)
    assert gb.solve() == 0
    assert gb.kernel_name.startswith("1tpi")
    return gb, [lqr_instance_qp(data, i, N) for i in range(B)]


@pytest.mark.parametrize("seed", STRUCT_SEEDS)
def test_jvp_vector_tangent_bits_hostsim(hostsim_lib, seed):
    gb, _ = _solved_struct(hostsim_lib, seed)
    check_vector_bits(gb, np.random.default_rng(100 + seed))


@pytest.mark.parametrize("seed", STRUCT_SEEDS)
def test_jvp_vs_dense_hostsim(hostsim_lib, seed):
    gb, qps = _struct_batch(hostsim_lib, seed)
    check_vs_dense(gb, qps, range(2), np.random.default_rng(200 + seed), seed in GEN_SEEDS)


@pytest.mark.parametrize("seed", STRUCT_SEEDS)
def test_jvp_dot_product_hostsim(hostsim_lib, seed):
    gb, _ = _solved_struct(hostsim_lib, seed)
    check_dot_product(gb, np.random.default_rng(300 + seed), DENSE_BAR.get(seed, 1e-9))


def test_jvp_one_instance_per_lane_hostsim(hostsim_lib, monkeypatch):
    """cases 1 to 3 through the sliced path of a one-instance-per-lane batch"""
    gb, qps = _lane_batch(hostsim_lib, monkeypatch)
    check_vector_bits(gb, np.random.default_rng(1))
    check_dot_product(gb, np.random.default_rng(3), 1e-9)
    check_vs_dense(gb, qps, range(gb.n_batch), np.random.default_rng(2), False)


# ------------------------------------------------------------------------------------------------------------------
# GPU tier: the product library
# ------------------------------------------------------------------------------------------------------------------

def _solved_gpu_case(monkeypatch, case):
    wpi, w16, fam = GPU_CASES[case]
    monkeypatch.setenv("ACADOS_AMD_WPI", wpi)
    monkeypatch.setenv("ACADOS_AMD_W16", w16)
    gb, inst = _gpu_case(case)
    soft = case == "chain_soft"
    _tight(gb, 1e-8 if soft else 1e-10, 100)
    assert gb.solve() == 0
    if fam:
        assert gb.kernel_name.startswith(fam), gb.kernel_name
    return gb, inst, soft


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GPU_CASES))
def test_jvp_gpu(gpu_lib, monkeypatch, case):
    """cases 1 to 3 on every kernel family the sweeps run in, the dense comparison on the instances
    test_data_grad_vs_dense_adjoint_gpu samples"""
    gb, inst, soft = _solved_gpu_case(monkeypatch, case)
    check_vector_bits(gb, np.random.default_rng(1))
    check_dot_product(gb, np.random.default_rng(4), 1e-4 if soft else 1e-7)
    sample = [int(i) for i in np.random.default_rng(2).choice(gb.n_batch, 4, replace=False)]
    check_vs_dense(gb, [inst(i) for i in sample], sample, np.random.default_rng(3), soft, soft_scale=1.0 if soft else None)


@pytest.mark.gpu
def test_jvp_torch_forward_ad_gpu(gpu_lib):
    """case 7: forward_ad through qp_solve and the plain qp_jvp give the bits of data_jvp"""
    import torch
    import torch.autograd.forward_ad as fwAD
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch
    from acados_amd.torch_qp import qp_jvp, qp_solve
    N, B = 6, 32
    gb = OcpQpGpuBatch(lqr_dims(N, 4, 2), B, device=0)
    fill_lqr_batch(gb, random_lqr_batch(N=N, nx=4, nu=2, batch=B, seed=3), N)
    _tight(gb, 1e-10, 100)
    assert gb.solve() == 0
    blob = torch.from_numpy(gb.get_bulk_in()).cuda()
    t = torch.from_numpy(random_tangent(gb, np.random.default_rng(5))).cuda()
    want = gb.data_jvp(t)
    assert want.is_cuda and bool(torch.isfinite(want).all()) and bool((want != 0).any())
    assert np.array_equal(want.cpu().numpy(), gb.data_jvp(t.cpu().numpy()))      # host arrays and CUDA tensors alike
    with fwAD.dual_level():
        sol = qp_solve(gb, fwAD.make_dual(blob, t))
        primal, tangent = fwAD.unpack_dual(sol)
        assert tangent is not None and torch.equal(tangent, want)
        assert torch.equal(primal, gb.get_bulk(torch.empty_like(primal)))
    assert torch.equal(qp_jvp(gb, blob, t), want)


# ------------------------------------------------------------------------------------------------------------------
# both tiers: the symmetric part, a failed instance, the state left behind (small structured batches)
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_jvp_symmetric_part(clib):
    """case 4: 1.0 in the single entry Q_ij (i != j) of one stage against 0.5 in (i, j) and (j, i)"""
    gb, _ = _solved_struct(clib, 5)
    o, n = gb.bulk_offset(0, "Q", 1)
    nx = int(gb.dims.nx[1])
    assert n == nx * nx and nx >= 2
    i, j = 1, 0
    one, half = np.zeros((gb.n_batch, gb.bulk_len(0))), np.zeros((gb.n_batch, gb.bulk_len(0)))
    one[:, o + i + j * nx] = 1.0
    half[:, o + i + j * nx] = half[:, o + j + i * nx] = 0.5
    a, b = gb.data_jvp(one), gb.data_jvp(half)
    assert np.any(a != 0)
    assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(a)), (np.max(np.abs(a - b)), np.max(np.abs(a)))


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_jvp_failed_instance(clib):
    """case 5: a NaN in q of the middle instance: its row is zero, the others are those of a clean batch"""
    clean, _ = _struct_batch(clib, 5, B=3)
    bad, _ = _struct_batch(clib, 5, B=3)
    q = bad.get("q", 1)
    q[1, 0] = np.nan
    bad.set("q", 1, q)
    assert clean.solve() == 0
    assert bad.solve() == 1
    st = bad.info("status")
    assert st[1] != 0 and st[0] == 0 and st[2] == 0
    t = random_tangent(clean, np.random.default_rng(6))
    want, got = clean.data_jvp(t), bad.data_jvp(t)
    assert np.all(got[1] == 0.0)
    assert np.array_equal(got[[0, 2]], want[[0, 2]]) and np.any(want[1] != 0)


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_jvp_state_left_behind(clib):
    """case 6: the same bits twice; no adjoint seed survives a JVP; reverse mode and a solve afterwards are those of a batch that
    never ran one"""
    gb, _ = _solved_struct(clib, 8)
    fresh, _ = _solved_struct(clib, 8)
    rng = np.random.default_rng(7)
    t, cot = random_tangent(gb, rng), random_cot(gb, rng)
    first = gb.data_jvp(t)
    assert np.array_equal(gb.data_jvp(t), first)
    L = gb._L
    grad = np.zeros((gb.n_batch, gb.bulk_len(0)))
    assert L.ocp_qp_gpu_batch_adj_seed_bulk(gb._h, cot.ctypes.data_as(C.c_void_p), 0) == 0
    gb.data_jvp(t)
    assert L.ocp_qp_gpu_batch_data_grad_bulk(gb._h, grad.ctypes.data_as(C.c_void_p), 0) == -1   # the JVP took the seed set
    assert np.array_equal(gb.data_grad(cot), fresh.data_grad(cot))
    assert np.array_equal(gb.data_jvp(t), first)
    assert gb.solve() == 0 and fresh.solve() == 0
    assert np.array_equal(gb.info("iter"), fresh.info("iter"))
    assert np.array_equal(gb.get_bulk(), fresh.get_bulk())

"""The condensing and expansion kernels against a plain evaluation of the condensing formulas; both tiers.

Elsewhere the condensed data is checked only through an oracle solve of the read-back QP, at 2e-6 / 1e-4 (tests/conftest.py
compare_condensed_with_oracle), on data that repeats one block over the horizon.  The condensing kernels fetch the next stage while
they contract the current one (prefetch(k0), then `if (ii + 1 < bs) prefetch(k + 1)`): here every stage carries data of its own
(tests/stagewise_common.py stagewise_perturb), and every entry of the condensed QP is compared with tests/dense_ref.py
condense_block_ref -- the formulas in 80-bit extended precision, no solver.

Cases, B = 5 (a group of four instances plus one), family forced with ACADOS_AMD_WPI=0:
  nx 8 nu 3:  (N, cond_N) = (10, 2) blocks 5, 5;  (9, 2) blocks 5, 4: a ragged last block, the child has nu = [15, 12, 0];
              (5, 1) one block and the terminal stage;  (6, 2) blocks 3, 3: no compiled set covers the block size
  nx 4 nu 1:  (8, 2) blocks 4, 4;  (7, 2) blocks 4, 3                                                   -- GQP_PCONDZ(4, 1, 4)
each on km_pcond (the default, pcond_kernel 3), kz_pcond (ACADOS_AMD_PCOND_MFMA=0: 2) and the run-time-shaped pair kw_pcond /
kw_pexpand (ACADOS_AMD_PCOND_W16=0, ACADOS_AMD_PCOND_LANE_EXPAND=0: 0); (6, 2) reports 0 whatever the switches say.

Compared, for every instance and child stage: R S Q, r q, A B b entrywise, the deviation relative to max(1, max |ref|) of the field;
the passed-through input bounds lbu ubu bit-equal to the parent's.  Expansion: the oracle's solution of the read-back condensed QP is
written into the child, expand() maps it back, and x u pi of every parent stage are compared with expand_block_ref (forward
simulation, adjoint recursion) under the same rule; lam and t of the input bounds are bit-equal to the child's; with lane expansion
on and off (pexpand_kernel 1 / 0).

TOLERANCE.  Reference against reference: over exactly these cases, the largest deviation (same rule) of the same formulas evaluated
in plain float64 NumPy from the extended-precision evaluation is 4.6e-16 for the condensed blocks and 4.3e-16 for the expansion
(test_tolerance_source_hostsim measures it again on every run); MEASURED_F64 = 4.7e-16 is that figure rounded up.  The tolerance is
64 times that, TOL = 3.0e-14: room for another summation order and for fused multiply-adds.  It stays below 1e-12.
The kernels deviate from the reference by 3.0e-16 to 8.6e-16 under host simulation and by 2.0e-16 to 5.6e-16 on the MI355X (printed
per case)."""
import numpy as np
import pytest

from dense_ref import condense_block_ref, expand_block_ref
from oracle.oracle import OracleQp, default_opts
from stagewise_common import GENERATORS, TIERS, stagewise_perturb

MEASURED_F64 = 4.7e-16
TOL = 64 * MEASURED_F64
B = 5
CASES = [("lqr83", 10, 2), ("lqr83", 9, 2), ("lqr83", 5, 1), ("lqr83", 6, 2), ("lqr41", 8, 2), ("lqr41", 7, 2)]
KERNELS = {"km_pcond": ({}, 3, 1),
           "kz_pcond": ({"ACADOS_AMD_PCOND_MFMA": "0"}, 2, 1),
           "kw_pcond": ({"ACADOS_AMD_PCOND_W16": "0", "ACADOS_AMD_PCOND_LANE_EXPAND": "0"}, 0, 0),
           "km_pcond/kw_pexpand": ({"ACADOS_AMD_PCOND_LANE_EXPAND": "0"}, 3, 0)}
COMPILED_BS = {"lqr83": 5, "lqr41": 4}        # block sizes of GQP_PCONDZ / GQP_PCOND


@pytest.fixture
def clib(request, monkeypatch):
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


def blocks(N, cond_N):
    """first stage of every block, as d_part_cond_qp_compute_block_size: N / cond_N each, the remainder to the first blocks; then the
    terminal stage"""
    start = [0]
    for j in range(cond_N):
        start.append(start[-1] + N // cond_N + (1 if j < N % cond_N else 0))
    assert start[-1] == N
    return start


def dev(got, ref):
    ref = np.asarray(ref)
    got = np.asarray(got, dtype=ref.dtype)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref))))) if ref.size else 0.0


def parent_batch(clib, gen, N, cond_N):
    from acados_amd import OcpQpGpuBatch
    gb = OcpQpGpuBatch.from_qps(GENERATORS[gen](N, B, 50 + N), _clib=clib)
    stagewise_perturb(gb, 8000 + N)
    gb.opts_set("cond_N", cond_N)
    return gb


_PARENT_QPS = {}


def parent_qps(gb, gen, N):
    """the instances' own read-back QPs, once per case (the data does not depend on the tier or the condensing kernel; asserted by the
    blob)"""
    blob = gb.get_bulk_in()
    if (gen, N) not in _PARENT_QPS:
        _PARENT_QPS[gen, N] = (blob, [gb.to_qp(i) for i in range(B)])
    assert np.array_equal(_PARENT_QPS[gen, N][0], blob)
    return _PARENT_QPS[gen, N][1]


def condensed_deviation(qp, qc, start, dtype=np.longdouble):
    """largest deviation of the condensed QP qc from the reference condensing of qp over the blocks `start`; the bounds bit for bit"""
    N, N2 = qp.N, len(start) - 1
    assert qc.N == N2
    worst = 0.0
    for j in range(N2 + 1):
        k0, k1 = (start[j], start[j + 1]) if j < N2 else (N, N + 1)
        ref = condense_block_ref(qp, k0, k1, dtype=dtype)
        assert int(qc.dims.nu[j]) == sum(int(qp.dims.nu[k]) for k in range(k0, k1)) and int(qc.dims.nx[j]) == int(qp.dims.nx[k0])
        for f in ("R", "S", "Q", "r", "q") + (("A", "B", "b") if j < N2 else ()):
            e = dev(getattr(qc, f)[j], ref[f])
            assert e <= TOL, (f, j, e)
            worst = max(worst, e)
        for f in ("lbu", "ubu"):
            want = np.concatenate([np.asarray(getattr(qp, f)[k], dtype=float) for k in range(k0, k1)])
            assert np.array_equal(np.asarray(getattr(qc, f)[j]), want), (f, j)
    return worst


@pytest.mark.parametrize("clib", TIERS, indirect=True)
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("gen,N,cond_N", CASES)
def test_condensing_matches_the_formulas(clib, monkeypatch, gen, N, cond_N, kernel):
    env, pcond, pexpand = KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gb = parent_batch(clib, gen, N, cond_N)
    start = blocks(N, cond_N)
    compiled = max(np.diff(start)) == COMPILED_BS[gen]
    c = gb.condense()
    assert c is not None and c.N == cond_N
    assert gb.kernel_name.startswith("1tpi-"), gb.kernel_name
    assert int(gb.scalar("pcond_kernel")) == (pcond if compiled else 0), (kernel, gb.scalar("pcond_kernel"))
    assert int(gb.scalar("pexpand_kernel")) == (pexpand if compiled else 0), (kernel, gb.scalar("pexpand_kernel"))
    qps = parent_qps(gb, gen, N)
    nu = int(qps[0].dims.nu[0])
    assert list(c.dims.nu) == [int(bs) * nu for bs in np.diff(start)] + [0]

    # ---- condensing
    qcs = [c.to_qp(i) for i in range(B)]
    worst_c = max(condensed_deviation(qps[i], qcs[i], start) for i in range(B))

    # ---- expansion of the oracle's solution of the condensed QP
    fields = ("x", "u", "lam", "t", "pi")
    sol = {(f, j): np.zeros((B, c._len(f, j))) for j in range(c.N + 1) for f in fields if not (f == "pi" and j == c.N)}
    for i in range(B):
        o = OracleQp(qcs[i])
        assert o.solve(default_opts(tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8, iter_max=60)) == 0, i
        for (f, j), a in sol.items():
            a[i] = o.get(j, f)
    for (f, j), a in sol.items():
        if a.size:
            c.set(f, j, a)
    child = {key: c.get(*key) for key in sol}
    for key, a in sol.items():
        assert np.array_equal(child[key], a), key
    gb.expand()
    worst_e = 0.0
    for j in range(c.N + 1):
        k0, k1 = (start[j], start[j + 1]) if j < c.N else (N, N + 1)
        got = {(f, k): gb.get(f, k) for k in range(k0, k1) for f in ("x", "u", "lam", "t") + (("pi",) if k < N else ())}
        nbc = int(c.dims.nbu[j] + c.dims.nbx[j])
        for i in range(B):
            ref = expand_block_ref(qps[i], k0, k1, child["u", j][i], child["x", j][i], child["pi", j][i] if j < c.N else None)
            for key, want in ref.items():
                e = dev(got[key][i], want)
                assert e <= TOL, (key, i, e)
                worst_e = max(worst_e, e)
            for k in range(k0, min(k1, N)):
                nb = int(qps[i].dims.nb[k])
                lo = (k - k0) * nu
                for f in ("lam", "t"):
                    assert np.array_equal(got[f, k][i][:nu], child[f, j][i][lo:lo + nu]), (f, k, i)
                    assert np.array_equal(got[f, k][i][nb:nb + nu], child[f, j][i][nbc + lo:nbc + lo + nu]), (f, k, i)
    print(f"{gen} N={N} cond_N={cond_N} {kernel}: worst deviation condensing {worst_c:.2e}, expansion {worst_e:.2e} (bound {TOL:.2e})")


def test_tolerance_source_hostsim(hostsim_lib, monkeypatch):
    """where MEASURED_F64 comes from, reference against reference (no kernel takes part: the library only carries the data): over
    the cases above, the formulas of dense_ref.py in plain float64 against the same formulas in extended precision -- the condensed
    blocks, and the expansion of the oracle's full-space solution (its inputs, block-start states and block-end multipliers)"""
    assert np.finfo(np.longdouble).eps < 1e-18          # 80-bit extended precision is what the reference runs in
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")
    worst_c = worst_e = 0.0
    for gen, N, cond_N in CASES:
        gb = parent_batch(hostsim_lib, gen, N, cond_N)
        start = blocks(N, cond_N)
        for qp in parent_qps(gb, gen, N):
            o = OracleQp(qp)
            assert o.solve(default_opts(tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8, iter_max=60)) == 0
            for j in range(cond_N + 1):
                k0, k1 = (start[j], start[j + 1]) if j < cond_N else (N, N + 1)
                ld, f64 = condense_block_ref(qp, k0, k1), condense_block_ref(qp, k0, k1, dtype=np.float64)
                worst_c = max([worst_c] + [dev(f64[f], ld[f]) for f in ld])
                ubar = np.concatenate([o.get(k, "u") for k in range(k0, k1)])
                args = (qp, k0, k1, ubar, o.get(k0, "x"), o.get(k1 - 1, "pi") if j < cond_N else None)
                ld, f64 = expand_block_ref(*args), expand_block_ref(*args, dtype=np.float64)
                worst_e = max([worst_e] + [dev(f64[key], ld[key]) for key in ld])
    print(f"float64 against extended precision: condensing {worst_c:.2e}, expansion {worst_e:.2e}")
    assert max(worst_c, worst_e) <= MEASURED_F64 and TOL == 64 * MEASURED_F64 and TOL <= 1e-12

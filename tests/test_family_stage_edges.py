"""Every solver family on stage-wise data, at short horizons and ragged batches; both tiers.

Every family fetches ahead of the stage it computes -- a register ring of stage records (kx_*, kbs_*), LDS-DMA of the packed block one
stage ahead (ky_*), prefetch_v(k +- 1) (ky_*, kt_factor), register prefetch (kw_factor_m) -- and the generators repeat one block over
the horizon, so on their data a fetch of a neighbouring stage's block, mask word, bound vector or descriptor changes nothing.  Here
every stage carries data of its own (tests/stagewise_common.py stagewise_perturb), the horizon is shorter than, equal to and longer
than every ring (N = 1, 2, 3, 9) and the batch sits at the family's sharing unit: one instance, one short of it, one beyond, several
units with a ragged last one.

Per case (all four tolerances 1e-8, no hand-over of the tail, iter_max 60): solve() == 0; the solve stayed on the family of the row
(kernel name and scalars); the independent residual kernel stays below 2e-8; every instance of a batch of at most 8 -- of a larger one
the lanes at the wave boundaries -- agrees with the oracle's solve of that instance's own read-back QP (x u pi lam at 1e-8 on the box
rows as tests/test_box_sweep_edges.py has it; x u pi lam sl su t at 1e-7 on the rows with general rows and slacks, the tolerance of
test_random_structures_gpu for such structures) and takes EXACTLY the oracle's number of iterations -- a sweep on a wrong block
usually still converges, in another number of iterations; the iteration counts of a batch of three or more take at least two values
(the seeds of stagewise_common.SEEDS were chosen with the oracle for that).

Grid.  gpu tier: every (N, B) of the row.  hostsim tier: every N at the row's ragged B (5, 65, 3), the remaining B at N = 2; the two
rows that cost seconds per case under simulation (w16r-box<24,6>, w16r-gen24) run N <= 3 there and the long horizon on the device.

Measured worst deviation from the oracle (printed per case), host simulation / MI355X: box rows 9.2e-15 / 4.5e-14, rows with general
rows and slacks 1.8e-10 / 2.5e-10."""
import numpy as np
import pytest

from conftest import compare_with_oracle
from stagewise_common import BATCHES, FAMILIES, HORIZONS, KKT_TOL, LONG, RAGGED, TIERS, check_family, compared_lanes, make_batch
from stagewise_common import oracle_solve as _oracle


@pytest.fixture
def clib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


def _grid():
    out = []
    for row, r in FAMILIES.items():
        for N in HORIZONS:
            for B in BATCHES[r["unit"]]:
                host = (B == RAGGED[r["unit"]] or N == 2) and not (r.get("slow") and N == LONG)
                tiers = [t for t in TIERS if t.id == "gpu" or host]
                for t in tiers:
                    out.append(pytest.param(t.values[0], row, N, B, id=f"{row}-N{N}-B{B}-{t.id}", marks=t.marks))
    return out


def _fields(row):
    return ("x", "u", "pi", "lam") + (("sl", "su", "t") if FAMILIES[row].get("gen") else ())


def _solve_case(clib, monkeypatch, row, N, B):
    gb = make_batch(clib, monkeypatch, row, N, B)
    blob = gb.get_bulk_in()
    bad = gb.solve()
    check_family(gb, row)
    assert bad == 0, (row, gb.info("status"), gb.info("iter"))
    return gb, blob


@pytest.mark.parametrize("clib,row,N,B", _grid(), indirect=["clib"])
def test_family_on_stagewise_data(clib, monkeypatch, row, N, B):
    gb, blob = _solve_case(clib, monkeypatch, row, N, B)
    nrm = gb.res_compute()
    assert np.all(np.isfinite(nrm)) and nrm.max() <= KKT_TOL, nrm.max()
    it = gb.info("iter")
    fields = _fields(row)
    sol = {(f, k): gb.get(f, k) for k in range(N + 1) for f in fields if not (f == "pi" and k == N)}
    tol = 1e-7 if FAMILIES[row].get("gen") else 1e-8
    worst = 0.0
    for i in compared_lanes(B):
        qp, o = _oracle(gb, blob, i)
        assert o.status == 0, (row, i, o.status)
        worst = max(worst, compare_with_oracle(lambda k, f: sol[(f, k)][i], o, qp, tol, fields=fields))
        assert int(it[i]) == o.iter, (row, i, int(it[i]), o.iter)
    print(f"{row} N={N} B={B}: iterations {sorted(set(it.tolist()))}, worst deviation from the oracle {worst:.2e}")
    if B >= 3:
        assert len(set(it.tolist())) >= 2, it


@pytest.mark.parametrize("clib", TIERS, indirect=True)
def test_two_rows_per_lane_families_agree_on_stagewise_data(clib, monkeypatch):
    """the pair rule of test_two_rows_per_lane_family_gpu on data where a stage mix-up shows: the tile sweep, the register-row sweep
    and the compile-time wave-per-instance kernels of the nx = 8, nu = 15 shape solve the same perturbed batch (N = 3, B = 7):
    equal iteration counts, x u pi lam equal to rtol = atol = 1e-9"""
    N, B = 3, 7
    sols = {}
    for row in ("w16r-box/tiles", "w16r-box/rows", "wpi-box<8,15>"):
        gb, blob = _solve_case(clib, monkeypatch, row, N, B)
        sols[row] = (blob, gb.info("iter").copy(),
                     {(f, k): gb.get(f, k).copy() for k in range(N + 1) for f in ("x", "u", "pi", "lam") if not (f in ("u", "pi") and k == N)})
        for k in FAMILIES[row]["env"]:
            monkeypatch.delenv(k)
    ref = sols["w16r-box/tiles"]
    for row in ("w16r-box/rows", "wpi-box<8,15>"):
        blob, it, sol = sols[row]
        assert np.array_equal(blob, ref[0])                      # the same data
        assert np.array_equal(it, ref[1]), (row, it, ref[1])
        for key, v in sol.items():
            np.testing.assert_allclose(v, ref[2][key], rtol=1e-9, atol=1e-9, err_msg=f"{row} {key}")

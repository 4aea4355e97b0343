"""The dispatch table of DESIGN.md 4 -- which kernel family serves which shape, batch size and structure -- row by row.

Every row creates a batch, sets its structure and lets `scalar("tol_comp_effective")` finalize it: no data, no solve.  What a row
leaves -- the kernel name, the `w16_tiles` scalar, or a refusal -- is compared with tests/dispatch_table.json, which
tools/record_dispatch_table.py wrote on the commit named in that file, before choose_family() existed (gpu_batch.hip).  The rows
stand on both sides of every rule of the table: the batch thresholds of each family, the 77 % rule of the two-rows shapes, shapes no
one-instance-per-lane set covers, state bounds behind stage 0, general rows and shared slacks, both values of every ACADOS_AMD_*
switch that steers the choice, the limits on inequality sides and on nu + nx, and ric_alg going 0 and back around the moment the
structure is finalized.  N = 1 throughout: a row takes at most 0.15 s under host simulation.

Both tiers run the same host code, so they share the expected values."""
import json
import os

import numpy as np
import pytest

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dispatch_table.json")

# every switch that steers the family choice: a row runs with exactly the ones it names
SWITCHES = ("ACADOS_AMD_WPI", "ACADOS_AMD_WPI_V1", "ACADOS_AMD_WPI_BATCH_MAX", "ACADOS_AMD_W16", "ACADOS_AMD_W16R", "ACADOS_AMD_W16G",
            "ACADOS_AMD_W16T", "ACADOS_AMD_W16T_GEN", "ACADOS_AMD_WPI_MFMA", "ACADOS_AMD_WPI_MFMA_PF", "ACADOS_AMD_WPI_CT",
            "ACADOS_AMD_W16_LDS_ALIGN", "ACADOS_AMD_GENERAL_KERNELS", "ACADOS_AMD_KB_SMALL")


def _dims(kind, nx, nu):
    """(dims, structure) of a row's shape, N = 1; structure: list of (field, stage, values) for set_int"""
    from acados_amd.generators import chain_soft_dims, lqr_dims
    from acados_amd.ocp_qp import AcadosOcpQpDims
    if kind == "lqr":            # bounds on the controls and on every state of stage 0, none of them equality-flagged
        return lqr_dims(1, nx, nu), []
    if kind == "lqr_x0":         # ... x0 equality-flagged: no inequality row on a state
        return lqr_dims(1, nx, nu), [("idxe", 0, nu + np.arange(nx))]
    if kind == "xbox":           # ... and bounds on every state behind stage 0
        d = lqr_dims(1, nx, nu)
        d.nbx[1] = nx
        d.nb[:] = d.nbu + d.nbx
        return d, []
    if kind == "free":           # bounds on the controls only
        d = lqr_dims(1, nx, nu)
        d.nbx[0] = 0
        d.nb[:] = d.nbu + d.nbx
        return d, []
    if kind == "shared_slack":   # the golden structure pend_idxs_rev_min_qp0: two general rows per stage sharing one slack
        d = lqr_dims(1, nx, nu)
        d.ng[:] = 2
        d.ns[:] = 1
        return d, [("idxs_rev", k, [-1] * int(d.nb[k]) + [0, 0]) for k in (0, 1)]
    if kind in ("soft", "soft_shared"):   # three state bounds at stage 1, two slacks: one per row / the first shared by two rows
        d = lqr_dims(1, nx, nu)
        d.nbx[1] = 3
        d.ns[1] = 2
        d.nb[:] = d.nbu + d.nbx
        return d, [("idxe", 0, nu + np.arange(nx)), ("idxs_rev", 1, [0, 1, -1] if kind == "soft" else [0, 0, 1])]
    if kind == "c4":             # the C4 class: four soft state bounds, four soft general rows
        d = chain_soft_dims(1, nx, nu)
        ixs = 6 * np.arange(4) + 1
        return d, [("idxe", 0, nu + np.arange(nx)), ("idxb", 1, ixs), ("idxs_rev", 1, np.arange(8))]
    raise ValueError(kind)


def _row(rid, kind, nx, nu, batch, env=None, ric=None):
    return {"id": rid, "kind": kind, "nx": nx, "nu": nu, "batch": batch, "env": env or {}, "ric": ric}


def _both(name, kind, nx, nu, batch, extra=None):
    """the switch at 0 and at 1"""
    return [_row(f"{name}={v}", kind, nx, nu, batch, dict(extra or {}, **{"ACADOS_AMD_" + name: str(v)})) for v in (0, 1)]


ROWS = [
    # box shapes with state bounds
    _row("c2_20480", "lqr", 8, 3, 20480),
    _row("c2_20481", "lqr", 8, 3, 20481),
    _row("c2_8192_w16_off", "lqr", 8, 3, 8192, {"ACADOS_AMD_W16": "0"}),
    _row("c2_8193_w16_off", "lqr", 8, 3, 8193, {"ACADOS_AMD_W16": "0"}),
    _row("small_4096", "lqr", 4, 1, 4096),
    _row("small_4097", "lqr", 4, 1, 4097),
    _row("small_64_lane_plain", "lqr", 4, 1, 64, {"ACADOS_AMD_WPI": "0", "ACADOS_AMD_KB_SMALL": "0"}),
    _row("two_rows_8_10", "lqr", 8, 10, 64),
    _row("two_rows_8_9_77pct", "lqr", 8, 9, 64),
    _row("two_rows_20_4", "lqr", 20, 4, 64),
    _row("two_rows_20_3_77pct", "lqr", 20, 3, 64),
    _row("no_lane_set_8_4", "lqr", 8, 4, 70000),
    _row("no_lane_set_9_4", "lqr", 9, 4, 70000),
    # (4, 1): state bounds behind stage 0 move the threshold
    _row("small_xbox_12288", "xbox", 4, 1, 12288),
    _row("small_xbox_12289", "xbox", 4, 1, 12289),
    _row("small_12288", "lqr", 4, 1, 12288),
    _row("small_x0_4097", "lqr_x0", 4, 1, 4097),
    _row("c2_x0_20481", "lqr_x0", 8, 3, 20481),
    _row("c2_free_20481", "free", 8, 3, 20481),
    # general rows, slacks
    _row("shared_slack_2048", "shared_slack", 4, 1, 2048),
    _row("shared_slack_2049", "shared_slack", 4, 1, 2049),
    _row("soft_box", "soft", 8, 3, 64),
    _row("soft_box_shared", "soft_shared", 8, 3, 64),
    _row("soft_box_shared_100000", "soft_shared", 8, 3, 100000),
    _row("c4_gen", "c4", 24, 3, 64),
    _row("c4_gen_100000", "c4", 24, 3, 100000),
    # limits
    _row("sides_66", "lqr", 30, 3, 8),
    _row("sides_128", "lqr", 60, 4, 8),
    _row("sides_130", "lqr", 61, 4, 8),
    _row("n_64", "free", 54, 10, 8),
    _row("n_70", "free", 60, 10, 8),
    # ric_alg around the finalized structure, on a wave-per-instance, a sixteen-lanes and a one-instance-per-lane batch
    _row("ric_wpi", "lqr", 20, 3, 64, ric=[0, "finalize", 1, 0, 1]),
    _row("ric_wpi_after", "lqr", 20, 3, 64, ric=["finalize", 0, 1]),
    _row("ric_w16_soft_shared", "soft_shared", 8, 3, 64, ric=[0, "finalize", 1, 0, 1]),
    _row("ric_w16", "lqr", 8, 3, 64, ric=[0, 1, "finalize", 0, 1]),
    _row("ric_lane", "lqr", 8, 3, 20481, ric=[0, "finalize", 1, 0, 1]),
]
# every switch at 0 and at 1, on the smallest shape on which it changes the name or the w16_tiles scalar (ACADOS_AMD_WPI_CT swaps
# kernels of one name: its rows show that both values leave the name alone)
ROWS += _both("WPI", "lqr", 8, 3, 20481) + _both("WPI", "lqr", 8, 3, 64) + _both("WPI_V1", "lqr", 8, 3, 64)
ROWS += _both("WPI_BATCH_MAX", "lqr", 8, 3, 1) + _both("W16", "lqr", 8, 3, 64) + _both("W16R", "lqr", 8, 10, 64)
ROWS += _both("W16G", "c4", 24, 3, 64) + _both("W16T", "lqr", 8, 10, 64) + _both("W16T_GEN", "c4", 24, 3, 64)
ROWS += _both("WPI_MFMA", "lqr", 20, 3, 64) + _both("WPI_MFMA", "c4", 24, 3, 64, {"ACADOS_AMD_W16G": "0"})
ROWS += _both("WPI_CT", "lqr", 8, 15, 64, {"ACADOS_AMD_W16R": "0"})
ROWS += _both("GENERAL_KERNELS", "lqr", 8, 3, 20481) + _both("KB_SMALL", "lqr", 4, 1, 4097)


def row_key(r):
    return f"{r['id']}:{r['kind']}({r['nx']},{r['nu']})x{r['batch']}"


assert len({row_key(r) for r in ROWS}) == len(ROWS)


def evaluate(clib, r, setenv, delenv):
    """what row r leaves: {"refused": true} or {"name", "w16_tiles"} (+ "ric": the name behind every step of r["ric"])"""
    from acados_amd import OcpQpGpuBatch
    for s in SWITCHES:
        delenv(s)
    for k, v in r["env"].items():
        setenv(k, v)
    dims, structure = _dims(r["kind"], r["nx"], r["nu"])
    try:
        gb = OcpQpGpuBatch(dims, r["batch"], _clib=clib)
    except RuntimeError:
        return {"refused": True}
    for f, k, v in structure:
        gb.set_int(f, k, v)
    out = {}
    if r["ric"]:
        out["ric"] = []
        for step in r["ric"]:
            if step == "finalize":
                gb.scalar("tol_comp_effective")
            else:
                gb.opts_set("ric_alg", step)
            out["ric"].append(gb.kernel_name)
    gb.scalar("tol_comp_effective")
    out["name"] = gb.kernel_name
    out["w16_tiles"] = int(gb.scalar("w16_tiles"))
    gb.close()
    return out


@pytest.fixture
def clib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


def _expected(cache={}):
    if not cache:
        with open(TABLE) as f:
            cache.update(json.load(f))
    return cache


@pytest.mark.parametrize("clib", TIERS, indirect=True)
@pytest.mark.parametrize("row", ROWS, ids=row_key)
def test_dispatch_row(clib, row, monkeypatch):
    want = _expected()["rows"][row_key(row) + "".join(f" {k}={v}" for k, v in sorted(row["env"].items()))]
    got = evaluate(clib, row, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert got == want, (row, got, want)


def test_table_covers_both_sides_of_the_rules():
    """the recorded table itself: the rows the issue read off the parent commit, and that every pair of rows that stands on the
    two sides of a rule really differs"""
    EXPECTED = _expected()
    rows = {k.split(":")[0] + "".join(" " + e for e in k.split(" ")[1:]): v for k, v in EXPECTED["rows"].items()}
    name = lambda k: rows[k].get("name")
    assert name("c2_20480") == "w16-box<NX=8,NU=3>" and name("c2_20481") == "1tpi-box<NX=8,NU=3,XBOX=1>"
    assert name("c2_8192_w16_off ACADOS_AMD_W16=0") == "wpi-box(nx=8,nu=3,lds=3192B)"
    assert name("c2_8193_w16_off ACADOS_AMD_W16=0").startswith("1tpi-box")
    assert name("small_4096") == "w16-box<NX=4,NU=1>" and name("small_4097") == "1tpi-pipe<NX=4,NU=1,XBOX=1>"
    assert name("small_64_lane_plain ACADOS_AMD_KB_SMALL=0 ACADOS_AMD_WPI=0") == "1tpi-box<NX=4,NU=1,XBOX=1>"
    assert name("two_rows_8_10") == "w16r-box<NX=8,NU=15>" and name("two_rows_8_9_77pct") == "wpi-box(nx=8,nu=9,lds=5304B)"
    assert name("two_rows_20_4") == "w16r-box<NX=24,NU=6>" and name("two_rows_20_3_77pct") == "wpi-box(nx=20,nu=3,lds=10200B)"
    assert name("no_lane_set_8_4") == name("no_lane_set_9_4") == "w16-box<NX=12,NU=4>"
    assert name("small_xbox_12288").startswith("w16-box") and name("small_xbox_12289").startswith("1tpi-pipe")
    assert name("small_12288").startswith("1tpi-pipe")
    assert name("shared_slack_2048").startswith("wpi-gen(") and name("shared_slack_2049").startswith("1tpi<NX=4,NU=1,NG=2,NS=3>")
    assert name("soft_box") == "w16-soft<NX=8,NU=3>" and name("soft_box_shared").startswith("wpi-gen(nx=8,nu=3")
    assert name("c4_gen").startswith("w16r-gen<NX=24,NU=3,NG=4>")
    assert name("sides_66") == "wpi-box(nx=30,nu=3,lds=19560B)" and rows["sides_130"] == {"refused": True} and rows["n_70"] == {"refused": True}
    assert "refused" not in rows["sides_128"] and "refused" not in rows["n_64"]
    ric = rows["ric_wpi"]["ric"]
    assert ",ric0" in ric[0] and ",ric0" in ric[1] and ric[2] == rows["two_rows_20_3_77pct"]["name"] and ",ric0" in ric[3] and ric[4] == ric[2]
    for sw in ("WPI", "WPI_V1", "WPI_BATCH_MAX", "W16", "W16R", "W16G", "W16T", "W16T_GEN", "WPI_MFMA", "KB_SMALL"):
        pair = [v for k, v in EXPECTED["rows"].items() if k.startswith(sw + "=") and f"ACADOS_AMD_{sw}=" in k]
        assert len(pair) >= 2 and any(a != b for a in pair for b in pair), sw

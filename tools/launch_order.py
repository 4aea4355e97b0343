"""The ordered launch list of a few small solves, to compare two builds of the library launch for launch (profiles/NOTES.md,
"IPM loop: one sweep launcher"): kernel name, grid, workgroup size and LDS bytes of every dispatch, in dispatch order.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_order.py solve [family]
    python tools/launch_order.py list [--runs] OUT > launches.txt (finds the *kernel_trace.csv below OUT)

`solve family` runs the solves of the second group only; `list --runs` writes a run of equal consecutive lines as one line, "N x ...".

The solves: the 130-instance one-instance-per-lane box batch of tests/test_hold_factor.py (held dynamics; defaults: the tail hands
over; compact_min 4; compact_min 4 with tail_max 0: a compaction level), the 7-instance sixteen-lanes batch of
tests/test_instance_isolation.py::test_dense_list_with_a_partly_filled_last_workgroup (the dense list comes on, launch per sweep) and
a 2-instance wave-per-instance batch; then the paths on which a batch changes its family (profiles/NOTES.md, "Kernel family of a batch: one
record"): a 5-instance soft-box batch whose slack structure (one slack shared by two rows) sends it from the sixteen-lanes family to
wave per instance, a 2-instance wave-per-instance batch solved three times with ric_alg 1, 0, 1, and LAST the 8-instance batch with
two activity words per stage of tests/test_sub_batches.py::test_compaction_level_of_a_two_activity_word_batch (a build without that
compaction level ends its listing there).  No counters, no other tracing in the same run."""
import csv
import glob
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def solve(family_only=False):
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch

    def run(tag, env, N, B, data, opts, dims=None, structure=None, more_data=None, ric_algs=(None,)):
        for k in ("ACADOS_AMD_WPI", "ACADOS_AMD_W16", "ACADOS_AMD_W16_PERM", "ACADOS_AMD_WPI_BATCH_MAX"):
            os.environ.pop(k, None)
        os.environ.update(env)
        gb = OcpQpGpuBatch(dims or lqr_dims(N, 8, 3), B, device=0)
        if structure:
            structure(gb)
        fill_lqr_batch(gb, data, N)
        if more_data:
            more_data(gb)
        gb.opts_set("tol_stat", 1e-8)
        for f, v in opts.items():
            gb.opts_set(f, v)
        for ric in ric_algs:
            if ric is not None:
                gb.opts_set("ric_alg", ric)
            bad = gb.solve()
            report(tag if ric is None else f"{tag}/ric_alg{ric}", gb, bad)

    def report(tag, gb, bad):
        print(f"{tag}: kernel {gb.kernel_name}, not converged {bad}, iter max {gb.info('iter').max()}, launches {int(gb.scalar('launches'))}, "
              f"tail switches {int(gb.scalar('tail_switches'))}, compactions {int(gb.scalar('compactions'))}, "
              f"fact held {int(gb.scalar('fact_held_launches'))}, rhs held {int(gb.scalar('rhs_held_launches'))}", flush=True)

    box = random_lqr_batch(N=3, nx=8, nu=3, batch=130, seed=43)
    for tag, opts in () if family_only else (("box130/defaults", {}), ("box130/compact_min4", {"compact_min": 4}), ("box130/compact_min4,tail_max0", {"compact_min": 4, "tail_max": 0})):
        run(tag, {"ACADOS_AMD_WPI": "0"}, 3, 130, box, opts)
    if not family_only:
        w16 = random_lqr_batch(N=2, nx=8, nu=3, batch=7, seed=38)
        w16["x0"][[1, 3, 6]] *= 1e-3
        run("w16/7", {"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "1"}, 2, 7, w16, {"solve_max": 0})
        run("wpi/2", {"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "0"}, 3, 2, random_lqr_batch(N=3, nx=8, nu=3, batch=2, seed=39), {})

    # soft bounds on three states behind stage 0, two slacks, the first shared by two rows: created on w16-soft, finalized on wpi-gen
    soft_dims = lqr_dims(2, 8, 3)
    soft_dims.nbx[1:] = 3
    soft_dims.ns[1:] = 2
    soft_dims.nb[:] = soft_dims.nbu + soft_dims.nbx

    def soft_shared(gb):
        gb.set_int("idxs_rev", 1, [-1, -1, -1, 0, 0, 1])
        gb.set_int("idxs_rev", 2, [0, 0, 1])

    def soft_data(gb):
        ones = lambda m, v: np.full((5, m), v)
        for k in (1, 2):
            gb.set("lbx", k, ones(3, -0.3)); gb.set("ubx", k, ones(3, 0.3))
            gb.set("Zl", k, ones(2, 1e2)); gb.set("Zu", k, ones(2, 1e2))
            gb.set("zl", k, ones(2, 1e1)); gb.set("zu", k, ones(2, 1e1))
            gb.set("lls", k, ones(2, 0.0)); gb.set("lus", k, ones(2, 0.0))

    run("soft-shared/5", {}, 2, 5, random_lqr_batch(N=2, nx=8, nu=3, batch=5, seed=40), {}, dims=soft_dims, structure=soft_shared, more_data=soft_data)
    run("wpi/2", {"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "0"}, 3, 2, random_lqr_batch(N=3, nx=8, nu=3, batch=2, seed=39), {}, ric_algs=(1, 0, 1))
    two = random_lqr_batch(N=3, nx=30, nu=3, batch=8, seed=5)
    two["x0"][[1, 3, 6]] *= 1e-3
    run("two-words/8", {}, 3, 8, two, {"compact_min": 2, "tail_max": 0}, dims=lqr_dims(3, 30, 3))


def listing(out_dir, runs=False):
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    col = {c.lower(): c for c in rows[0]}
    get = lambda r, name: r[col[name.lower()]] if name.lower() in col else "?"
    rows.sort(key=lambda r: int(get(r, "Dispatch_Id" if "dispatch_id" in col else "Start_Timestamp")))
    lines = []
    for r in rows:
        grid = "x".join(get(r, "Grid_Size_" + a) for a in "XYZ")
        wg = "x".join(get(r, "Workgroup_Size_" + a) for a in "XYZ")
        lines.append(f"{get(r, 'Kernel_Name')}\tgrid {grid}\tworkgroup {wg}\tlds {get(r, 'LDS_Block_Size')}")
    for line, group in itertools.groupby(lines) if runs else ((ln, [ln]) for ln in lines):
        n = len(list(group))
        print(line if n == 1 else f"{n} x {line}")


if __name__ == "__main__":
    if sys.argv[1:] in (["solve"], ["solve", "family"]):
        solve(family_only=len(sys.argv) == 3)
    elif sys.argv[1:2] == ["list"] and len(sys.argv) == 3 + (sys.argv[2:3] == ["--runs"]):
        listing(sys.argv[-1], runs=len(sys.argv) == 4)
    else:
        sys.exit(__doc__)

"""The ordered launch list of four small solves, to compare two builds of the library launch for launch (profiles/NOTES.md,
"IPM loop: one sweep launcher"): kernel name, grid, workgroup size and LDS bytes of every dispatch, in dispatch order.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_order.py solve
    python tools/launch_order.py list OUT > launches.txt          (finds the *kernel_trace.csv below OUT)

The solves: the 130-instance one-instance-per-lane box batch of tests/test_hold_factor.py (held dynamics; defaults: the tail hands
over; compact_min 4; compact_min 4 with tail_max 0: a compaction level), the 7-instance sixteen-lanes batch of
tests/test_instance_isolation.py::test_dense_list_with_a_partly_filled_last_workgroup (the dense list comes on, launch per sweep) and
a 2-instance wave-per-instance batch.  No counters, no other tracing in the same run."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def solve():
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch

    def run(tag, env, N, B, data, opts):
        for k in ("ACADOS_AMD_WPI", "ACADOS_AMD_W16", "ACADOS_AMD_W16_PERM"):
            os.environ.pop(k, None)
        os.environ.update(env)
        gb = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, device=0)
        fill_lqr_batch(gb, data, N)
        gb.opts_set("tol_stat", 1e-8)
        for f, v in opts.items():
            gb.opts_set(f, v)
        bad = gb.solve()
        print(f"{tag}: kernel {gb.kernel_name}, not converged {bad}, iter max {gb.info('iter').max()}, launches {int(gb.scalar('launches'))}, "
              f"tail switches {int(gb.scalar('tail_switches'))}, compactions {int(gb.scalar('compactions'))}, "
              f"fact held {int(gb.scalar('fact_held_launches'))}, rhs held {int(gb.scalar('rhs_held_launches'))}", flush=True)

    box = random_lqr_batch(N=3, nx=8, nu=3, batch=130, seed=43)
    for tag, opts in (("box130/defaults", {}), ("box130/compact_min4", {"compact_min": 4}), ("box130/compact_min4,tail_max0", {"compact_min": 4, "tail_max": 0})):
        run(tag, {"ACADOS_AMD_WPI": "0"}, 3, 130, box, opts)
    w16 = random_lqr_batch(N=2, nx=8, nu=3, batch=7, seed=38)
    w16["x0"][[1, 3, 6]] *= 1e-3
    run("w16/7", {"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "1"}, 2, 7, w16, {"solve_max": 0})
    run("wpi/2", {"ACADOS_AMD_WPI": "1", "ACADOS_AMD_W16": "0"}, 3, 2, random_lqr_batch(N=3, nx=8, nu=3, batch=2, seed=39), {})


def listing(out_dir):
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    col = {c.lower(): c for c in rows[0]}
    get = lambda r, name: r[col[name.lower()]] if name.lower() in col else "?"
    rows.sort(key=lambda r: int(get(r, "Dispatch_Id" if "dispatch_id" in col else "Start_Timestamp")))
    for r in rows:
        grid = "x".join(get(r, "Grid_Size_" + a) for a in "XYZ")
        wg = "x".join(get(r, "Workgroup_Size_" + a) for a in "XYZ")
        print(f"{get(r, 'Kernel_Name')}\tgrid {grid}\tworkgroup {wg}\tlds {get(r, 'LDS_Block_Size')}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["solve"]:
        solve()
    elif sys.argv[1:2] == ["list"] and len(sys.argv) == 3:
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)

"""Solve rate and factor-sweep time of the classical Riccati recursion (ric_alg 0) against the square-root one (ric_alg 1),
both on the wave-per-instance family (ACADOS_AMD_WPI=1), for the C4 shape (nx 24, nu 3, general rows and slacks, 16,384
instances) and the C2 shape (nx 8, nu 3, 8,192 instances).  One line per (shape, ric_alg):
  python tools/ric_alg_rate.py [out.json]    (sets ACADOS_AMD_WPI=1 ACADOS_AMD_W16=0 ACADOS_AMD_WPI_MFMA=0 unless given)
Per-class kernel times come from the batch's own event timing (option "profile"); run it under
rocprofv3 --kernel-trace --stats for the per-kernel view."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ACADOS_AMD_WPI", "1")
os.environ.setdefault("ACADOS_AMD_W16", "0")        # the square-root side on the same family: not the sixteen-lanes kernels
os.environ.setdefault("ACADOS_AMD_WPI_MFMA", "0")   # ... nor the MFMA factor sweep
from acados_amd import OcpQpGpuBatch  # noqa: E402
from acados_amd.generators import (chain_soft_batch, chain_soft_dims, fill_chain_soft_batch, fill_lqr_batch,  # noqa: E402
                                   lqr_dims, random_lqr_batch)

REPS = int(os.environ.get("RIC_RATE_REPS", "5"))


def shapes():
    yield "C4", 16384, lambda: (chain_soft_dims(), 40, chain_soft_batch(batch=16384), fill_chain_soft_batch)
    yield "C2", 8192, lambda: (lqr_dims(50, 8, 3), 50, random_lqr_batch(N=50, batch=8192, seed=3), fill_lqr_batch)


def main():
    rows = []
    for name, B, make in shapes():
        dims, N, data, fill = make()
        ref = None
        for ric in (1, 0):
            g = OcpQpGpuBatch(dims, B)
            fill(g, data, N)
            g.opts_set("ric_alg", ric)
            g.solve()   # warm-up: module load, LDS attributes
            ts = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                bad = g.solve()
                ts.append(time.perf_counter() - t0)
            g.scalar("prof_reset")
            g.opts_set("profile", 1)
            g.solve()
            g.opts_set("profile", 0)
            ms = {c: g.scalar("prof_ms_" + c) / max(g.scalar("prof_cnt_" + c), 1) for c in ("back_fact", "fwd_aff", "back_rhs", "fwd_corr")}
            x = np.concatenate([g.get("x", k) for k in range(N + 1)], axis=1)
            dx = None if ref is None else float(np.max(np.abs(x - ref)))
            ref = x if ref is None else ref
            row = {"shape": name, "batch": B, "ric_alg": ric, "kernel": g.kernel_name, "solve_ms_min": min(ts) * 1e3,
                   "solve_ms_median": float(np.median(ts)) * 1e3, "solves_per_s": B / min(ts), "failures": int(bad),
                   "iters_mean": float(np.mean(g.info("iter"))), "sweep_ms": ms, "max_x_diff_vs_ric1": dx}
            print(json.dumps(row), flush=True)
            rows.append(row)
            g.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

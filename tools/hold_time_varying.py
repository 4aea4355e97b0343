"""Development aid: what the held dynamics of the box sweeps (ipm_kernels_box.hpp) cost a QP whose dynamics are NOT the same at
every stage.  The C2 batch (65,536 instances, N = 50, nx = 8, nu = 3) with one entry of A of every instance moved by one ulp at
one stage: no tile is stage-invariant (tiles_invariant == 0), every sweep fetches [B A]' at every stage, and the solve must take
what it takes with the option hold_dynamics = 0 and on a library without the feature (a development build of the parent commit
in tools/ab/).  ONE configuration per process -- where a batch lies in memory moves a C2 solve by several ms (the first batch a
process creates is the slowest), so the configurations are compared as the only batch of processes run in turn:
  python tools/hold_time_varying.py hold1 | hold0 | libacados_amd_qp_<tag>.so"""
import ctypes, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acados_amd import OcpQpGpuBatch, _lib
from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch

N, B, STAGE, SOLVES = 50, 65536, 25, 7
what = sys.argv[1] if len(sys.argv) > 1 else "hold1"
hold = {"hold1": 1, "hold0": 0}.get(what)
clib = None if hold is not None else _lib.bind(ctypes.CDLL(os.path.join(ROOT, "tools", "ab", what)))
data = random_lqr_batch(N=N, nx=8, nu=3, batch=B, seed=3)
A1 = data["A"].copy()
A1[:, 1, 2] = np.nextafter(A1[:, 1, 2], np.inf)
g = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, _clib=clib)
fill_lqr_batch(g, data, N)
g.set("A", STAGE, A1)
for f in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp"):
    g.opts_set(f, 1e-8)
if hold is not None:
    g.opts_set("hold_dynamics", hold)
bad = g.solve()   # warm-up
if hold:
    assert int(g.scalar("tiles_invariant")) == 0, g.scalar("tiles_invariant")
ts = []
for _ in range(SOLVES):
    t0 = time.perf_counter(); g.solve(); ts.append(time.perf_counter() - t0)
ms = np.array(ts) * 1e3
g.scalar("prof_reset"); g.opts_set("profile", 1); g.solve()
pl = {c: g.scalar("prof_ms_" + c) / max(g.scalar("prof_cnt_" + c), 1) for c in ("back_fact", "fwd_aff", "back_rhs", "fwd_corr")}
it = g.info("iter")
print(f"{what:30s} failures {bad}  iterations {it.sum()} (max {it.max()})  median {np.median(ms):7.2f} ms  min {ms.min():7.2f}  max {ms.max():7.2f}  "
      f"all {' '.join(f'{t:.2f}' for t in ms)}  per launch: fact {pl['back_fact']:.3f} faff {pl['fwd_aff']:.3f} "
      f"rhs {pl['back_rhs']:.3f} fcor {pl['fwd_corr']:.3f} ms", flush=True)

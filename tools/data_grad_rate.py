"""Cost of the reverse-mode data gradient (ocp_qp_gpu_batch_adj_seed_bulk + _data_grad_bulk) against solve(), C2 shape
(N 50, nx 8, nu 3) at 65,536 instances, device-resident tensors throughout.  HIP events on the batch's stream:
  solve        ocp_qp_gpu_batch_solve
  seed         _adj_seed_bulk (cotangent scatter; the factorisation at the solution where the sweeps run in place)
  sweeps       _sens_set_bulk + _sens_solve with an all-zero seed: the adjoint sweeps alone (sliced on this family)
  grad_total   _data_grad_bulk: sweeps + contraction
  seed_all     _adj_seed_all_bulk with a cotangent on every entry of the output blob (u x sl su pi lam t), grad_total_all the
               _data_grad_bulk behind it
  contraction  grad_total - sweeps; GB/s = gradient bytes written / contraction time
    python tools/data_grad_rate.py [batch] [out.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acados_amd import OcpQpGpuBatch  # noqa: E402
from acados_amd.generators import fill_lqr_batch, lqr_dims, random_lqr_batch  # noqa: E402

REPS = 3


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    N = 50
    gb = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, device=0)
    fill_lqr_batch(gb, random_lqr_batch(N=N, batch=B, seed=3), N)
    st = torch.cuda.ExternalStream(gb.stream)
    L = gb._L
    lin, lout, lseed = gb.bulk_len(0), gb.bulk_len(1), L.ocp_qp_gpu_batch_sens_bulk_len(gb._h, 0)
    cot = torch.zeros((B, lout), dtype=torch.float64, device="cuda")
    for k in range(N + 1):
        o, n = gb.bulk_offset(1, "x", k)
        cot[:, o:o + n] = 1.0
    cot_all = torch.randn((B, lout), dtype=torch.float64, device="cuda")
    grad = torch.empty((B, lin), dtype=torch.float64, device="cuda")
    zseed = torch.zeros((B, lseed), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        rc = fn()
        e1.record(st)
        e1.synchronize()
        assert rc == 0 or rc is None, rc
        return e0.elapsed_time(e1)

    res = {k: [] for k in ("solve", "seed", "sweeps", "grad_total", "seed_all", "grad_total_all")}
    p = lambda t: C.c_void_p(t.data_ptr())
    gb.solve()   # warm-up: module load, sub-batches
    for _ in range(REPS):
        res["solve"].append(timed(lambda: gb.solve()))
        res["sweeps"].append(timed(lambda: L.ocp_qp_gpu_batch_sens_set_bulk(gb._h, p(zseed), 1) or L.ocp_qp_gpu_batch_sens_solve(gb._h)))
        res["seed"].append(timed(lambda: L.ocp_qp_gpu_batch_adj_seed_bulk(gb._h, p(cot), 1)))
        res["grad_total"].append(timed(lambda: L.ocp_qp_gpu_batch_data_grad_bulk(gb._h, p(grad), 1)))
        res["seed_all"].append(timed(lambda: L.ocp_qp_gpu_batch_adj_seed_all_bulk(gb._h, p(cot_all), 1)))
        res["grad_total_all"].append(timed(lambda: L.ocp_qp_gpu_batch_data_grad_bulk(gb._h, p(grad), 1)))
    ms = {k: float(np.median(v)) for k, v in res.items()}
    contraction = max(ms["grad_total"] - ms["sweeps"], 1e-6)
    row = {"shape": "C2", "N": N, "batch": B, "kernel": gb.kernel_name, "ms": ms, "contraction_ms": contraction,
           "grad_bytes": 8 * B * lin, "contraction_GBps": 8 * B * lin / contraction * 1e-6,
           "grad_over_solve": (ms["seed"] + ms["grad_total"]) / ms["solve"], "contraction_over_solve": contraction / ms["solve"],
           "finite": bool(torch.isfinite(grad).all())}
    print(json.dumps(row), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()

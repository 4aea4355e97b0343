"""Cost of the forward-mode data derivative (ocp_qp_gpu_batch_data_jvp_bulk) against solve() and against the reverse-mode gradient
in the same run, C2 shape (N 50, nx 8, nu 3) at 65,536 instances, device-resident tensors throughout.  HIP events on the batch's
stream, median of REPS after a warm-up of every timed call:
  solve        ocp_qp_gpu_batch_solve
  sweeps       _sens_set_bulk + _sens_solve with an all-zero seed blob: seed scatter + the sweeps (sliced on this family)
  readback     _sens_get_bulk into a device tensor
  jvp_total    _data_jvp_bulk: tangent kernel + seed scatter + sweeps + read-back
  tangent      jvp_total - sweeps - readback; GB/s = (tangent bytes read + seed bytes written) / tangent time
  grad_seed, grad_total   _adj_seed_bulk, _data_grad_bulk (tools/data_grad_rate.py's figures, here for the same box and run)
    python tools/data_jvp_rate.py [batch] [out.json]"""
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

REPS = 5


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    N = 50
    gb = OcpQpGpuBatch(lqr_dims(N, 8, 3), B, device=0)
    fill_lqr_batch(gb, random_lqr_batch(N=N, batch=B, seed=3), N)
    st = torch.cuda.ExternalStream(gb.stream)
    L = gb._L
    lin, lout, lseed = gb.bulk_len(0), gb.bulk_len(1), L.ocp_qp_gpu_batch_sens_bulk_len(gb._h, 0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    tangent = torch.randn((B, lin), dtype=torch.float64, device="cuda", generator=gen)
    cot = torch.zeros((B, lout), dtype=torch.float64, device="cuda")
    for k in range(N + 1):
        o, n = gb.bulk_offset(1, "x", k)
        cot[:, o:o + n] = 1.0
    out = torch.empty((B, lout), dtype=torch.float64, device="cuda")
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

    p = lambda t: C.c_void_p(t.data_ptr())
    calls = {
        "solve": lambda: gb.solve(),
        "sweeps": lambda: L.ocp_qp_gpu_batch_sens_set_bulk(gb._h, p(zseed), 1) or L.ocp_qp_gpu_batch_sens_solve(gb._h),
        "readback": lambda: L.ocp_qp_gpu_batch_sens_get_bulk(gb._h, p(out), 1),
        "jvp_total": lambda: L.ocp_qp_gpu_batch_data_jvp_bulk(gb._h, p(tangent), p(out), 1),
        "grad_seed": lambda: L.ocp_qp_gpu_batch_adj_seed_bulk(gb._h, p(cot), 1),
        "grad_total": lambda: L.ocp_qp_gpu_batch_data_grad_bulk(gb._h, p(grad), 1),
    }
    res = {k: [] for k in calls}
    for rep in range(REPS + 1):   # rep 0: warm-up of every call (module load, sub-batches, tables)
        for k, fn in calls.items():
            ms = timed(fn)
            if rep:
                res[k].append(ms)
    ms = {k: float(np.median(v)) for k, v in res.items()}
    spread = {k: [float(min(v)), float(max(v))] for k, v in res.items()}
    tan = max(ms["jvp_total"] - ms["sweeps"] - ms["readback"], 1e-6)
    contraction = max(ms["grad_total"] - ms["sweeps"], 1e-6)
    row = {"shape": "C2", "N": N, "batch": B, "kernel": gb.kernel_name, "reps": REPS, "ms": ms, "min_max_ms": spread,
           "tangent_ms": tan, "tangent_bytes": 8 * B * (lin + lseed), "tangent_GBps": 8 * B * (lin + lseed) / tan * 1e-6,
           "jvp_over_solve": ms["jvp_total"] / ms["solve"], "tangent_over_solve": tan / ms["solve"],
           "grad_contraction_ms": contraction, "grad_over_solve": (ms["grad_seed"] + ms["grad_total"]) / ms["solve"],
           "finite": bool(torch.isfinite(out).all())}
    print(json.dumps(row), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()

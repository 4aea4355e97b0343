"""torch.autograd over the batched QP solve ("Data gradients").

    sol = qp_solve(gb, blob)        # blob: [n_batch, gb.bulk_len(0)] float64 CUDA tensor, the input blob layout
    loss(sol).backward()            # blob.grad: dL/d(blob), same shape as blob

Forward: _set_bulk (device pointer) -> solve -> _get_bulk (device pointer), nothing through the host.  Backward: one adjoint solve
and the contraction kernel (OcpQpGpuBatch.data_vjp: ocp_qp_gpu_batch_adj_seed_all_bulk + _data_grad_bulk), gradient w.r.t. the QP
data only; the cotangent may touch every entry of the solution, u x sl su pi lam t (one on t is folded into lam of its side; those on
lam and t of sides that take no part are ignored).  Q and R receive the symmetric gradient in both triangles.  Instances whose solve
failed get a zero gradient row.  Forward mode: under torch.autograd.forward_ad a tangent of `blob` comes out as the tangent of `sol` (u x sl su pi lam
t; ocp_qp_gpu_batch_data_jvp_bulk: the tangent folded into one seed set and one sensitivity solve); qp_jvp is the same without a
dual level.  torch is imported when this module is, not by `import acados_amd`.
"""
import torch

INPUT, OUTPUT = 0, 1


class _QpSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blob, gb):
        blob = blob.detach().contiguous()
        gb.set_bulk(blob)
        gb.solve()
        sol = torch.empty((gb.n_batch, gb.bulk_len(OUTPUT)), dtype=torch.float64, device=blob.device)
        gb.get_bulk(sol)
        gb._torch_token = token = object()
        ctx.gb, ctx.token = gb, token
        ctx.save_for_backward(blob)
        ctx.save_for_forward(blob)
        return sol

    @staticmethod
    def _restore(ctx):
        gb = ctx.gb
        if getattr(gb, "_torch_token", None) is not ctx.token:
            # the batch has solved other data since this forward: restore the solution the derivative belongs to
            (blob,) = ctx.saved_tensors
            gb.set_bulk(blob)
            gb.solve()
            gb._torch_token = ctx.token
        return gb

    @staticmethod
    def backward(ctx, grad_sol):
        gb = _QpSolve._restore(ctx)
        return gb.data_vjp(grad_sol.detach().to(torch.float64).contiguous()), None

    @staticmethod
    def jvp(ctx, blob_t, _):
        gb = _QpSolve._restore(ctx)
        return gb.data_jvp(blob_t.detach().to(torch.float64).contiguous())


def qp_solve(gb, blob):
    """solution blob [n_batch, bulk_len(1)] of the QPs in `blob` (input blob layout), differentiable w.r.t. `blob`"""
    if not (blob.is_cuda and blob.dtype == torch.float64):
        raise TypeError("qp_solve: blob must be a float64 CUDA tensor")
    return _QpSolve.apply(blob, gb)


def qp_jvp(gb, blob, tangent):
    """d(solution) [n_batch, bulk_len(1)] of the QPs in `blob` along `tangent` (both in the input blob layout): solves `blob`,
    then ocp_qp_gpu_batch_data_jvp_bulk; what forward_ad gives through qp_solve, without a dual level"""
    for t in (blob, tangent):
        if not (t.is_cuda and t.dtype == torch.float64):
            raise TypeError("qp_jvp: blob and tangent must be float64 CUDA tensors")
    gb.set_bulk(blob.detach().contiguous())
    gb.solve()
    gb._torch_token = object()
    return gb.data_jvp(tangent.detach().contiguous())


def blob_views(gb, blob, output=INPUT):
    """{(field, stage): view of `blob`} -- vectors [n_batch, n], matrices [n_batch, rows, cols] (column-major storage, so the
    view is the transpose of a row-major reshape); views share storage with `blob`"""
    from .gpu_batch import DATA_FIELDS
    d = gb.dims
    fields = DATA_FIELDS + ("lbx#value",) if output == INPUT else ("u", "x", "sl", "su", "pi", "lam", "t")
    shape = {"A": lambda k: (int(d.nx[k + 1]), int(d.nx[k])), "B": lambda k: (int(d.nx[k + 1]), int(d.nu[k])),
             "Q": lambda k: (int(d.nx[k]), int(d.nx[k])), "R": lambda k: (int(d.nu[k]), int(d.nu[k])),
             "S": lambda k: (int(d.nu[k]), int(d.nx[k])), "C": lambda k: (int(d.ng[k]), int(d.nx[k])),
             "D": lambda k: (int(d.ng[k]), int(d.nu[k]))}
    out = {}
    for k in range(gb.N + 1):
        for f in fields:
            o, n = gb.bulk_offset(output, f, k)
            if n <= 0:
                continue
            v = blob[:, o:o + n]
            if f in shape:
                r, c = shape[f](k)
                v = v.reshape(blob.shape[0], c, r).transpose(1, 2)
            out[(f, k)] = v
    return out

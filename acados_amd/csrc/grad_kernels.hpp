/*
 * grad_kernels.hpp -- reverse-mode gradient of the QP solution w.r.t. every entry of the QP data ("Data gradients").
 *
 * Given the solution (w, pi, lam) and the adjoint direction (w^, pi^, lam^) -- the sensitivity sweeps run with the output
 * cotangent as seed in (r, q, zl, zu) -- every entry of the INPUT blob (ocp_qp_gpu_batch_bulk_len / _offset, output = 0) is one of
 *   op 1  c * D[a]                                                 vectors: r q zl zu, b (pi^), bounds (+-lam^ of their side)
 *   op 2  c * ((D[a] - D[a2]) S[b] + (S[a] - S[a2]) D[b])          matrices: Q R S Zl Zu (a, b both in w), A B (a in pi),
 *                                                                  C D (a: upper side, a2: lower side of the general row)
 *   op 3  sum over terms t in [a, a2): c_t * T[tab_t](elem_t) * D[d_t]   an equality-flagged bound's value (x0): the stationarity
 *                                                                  row of the fixed variable applied to the adjoint direction
 *   op 0  0                                                        masks; rows that do not take part
 * where S[] / D[] are the instance's solution / adjoint direction in the OUTPUT blob layout (u x sl su pi lam t), held in LDS, with
 * lam of the sides that do not take part set to 0.  The tables (host-built, gpu_batch.hip grad_build) are the same for every
 * instance.
 *
 * Mapping: one workgroup of 256 lanes per instance.  Phase 1 gathers S and D of the instance into LDS from the batch's own arrays
 * (either layout, through the bulk-unpack element map).  Phase 2 walks the blob with the lanes along its elements: the dominant
 * traffic, the gradient blob itself (as many bytes as the input blob), is written as consecutive 8-byte words by consecutive lanes;
 * the op table (24 B per element, the same for every instance) is served by L2.  Workgroups are renumbered so that consecutive
 * instances run on the same XCD: the wave-tiled arrays of phase 1 put 16 instances into one 128-byte line, which then stays in one L2.
 *
 * Forward mode (k_data_tangent, below): the same tables transposed -- a tangent of the input blob folded into one seed set.
 *
 * The seed of the adjoint sweeps: k_adj_seed for a cotangent on u x sl su (it refuses one on pi lam t), k_adj_seed_all for a
 * cotangent on every entry of the output blob; k_data_grad follows either.
 */
#ifndef GRAD_KERNELS_HPP_
#define GRAD_KERNELS_HPP_

#include "ipm_kernels.hpp"

#ifndef GQP_DYN_SHARED
#define GQP_DYN_SHARED(name) extern __shared__ double name[]
#endif

namespace gqp
{

struct GradOp
{
    int op, a, a2, b;
    double c;
};

struct GradTerm
{
    int tab, elem, d, pad_;
    double c;
};

#define GQP_GRAD_THREADS 256
#define GQP_GRAD_XCD 8 /* workgroups are dealt round-robin to the XCDs of the device */

/* tables T: 0..4 solution (ux sv pi lam t), 5..9 direction (dux dsv dpi dlam dt), 10 RSQ, 11 BAt, 12 DCt, 13 cotangent (ux layout).
 * o_arr / o_elem: the bulk-unpack map of the output blob with its array indices renumbered to 0..4; o_gate: activity bit
 * stage_word * 64 + bit of a lam / t entry (-1: no gate, -2: never takes part -- an equality-flagged row). */
static __global__ void __launch_bounds__(GQP_GRAD_THREADS) k_data_grad(double *grad, int nb, int len, const GradOp *ops, const GradTerm *terms,
                                                                      int olen, const int *o_arr, const int *o_elem, const int *o_gate,
                                                                      GArrTable T, GArrU64 amask, const int *status, int per)
{
    GQP_DYN_SHARED(lds);
    double *S = lds, *D = lds + olen;
    const int bx = blockIdx.x, tid = threadIdx.x;
    const int i = (bx % GQP_GRAD_XCD) * per + bx / GQP_GRAD_XCD;
    if (i >= nb) return;
    double *out = grad + (size_t) i * (size_t) len;
    if (status[i] != 0)
    {
        for (int e = tid; e < len; e += GQP_GRAD_THREADS) out[e] = 0.0;
        return;
    }
    for (int e = tid; e < olen; e += GQP_GRAD_THREADS)
    {
        const int a = o_arr[e], g = o_gate[e];
        double s = 0.0, d = 0.0;
        bool on = a >= 0 && g != -2;
        if (on && g >= 0) on = (GATL(amask, g >> 6) >> (g & 63)) & 1;
        if (on)
        {
            s = GATL(T.a[a], o_elem[e]);
            d = GATL(T.a[a + 5], o_elem[e]);
        }
        S[e] = s;
        D[e] = d;
    }
    __syncthreads();
    for (int e = tid; e < len; e += GQP_GRAD_THREADS)
    {
        const GradOp o = ops[e];
        double v = 0.0;
        if (o.op == 1)
            v = o.c * D[o.a];
        else if (o.op == 2)
        {
            const double da = o.a2 >= 0 ? D[o.a] - D[o.a2] : D[o.a], sa = o.a2 >= 0 ? S[o.a] - S[o.a2] : S[o.a];
            v = o.c * (da * S[o.b] + sa * D[o.b]);
        }
        else if (o.op == 3)
            for (int q = o.a; q < o.a2; q++)
            {
                const GradTerm t = terms[q];
                const double m = t.tab >= 0 ? GATL(T.a[t.tab], t.elem) : 1.0;
                v += t.c * m * (t.d >= 0 ? D[t.d] : 1.0);
            }
        out[e] = v;
    }
}

/* FORWARD MODE, the transpose of k_data_grad: a tangent of the INPUT blob, contracted with the solution, folded into one seed set
 * (BLOB_SEED layout, natural-sign bounds: what _sens_set_bulk takes).  Entry e of the seed blob is
 *   sum over terms q in [row[e], row[e + 1]): c_q * tangent[te_q] * (si_q >= 0 ? S[si_q] : 1)
 * in the order of the table (host-built, gpu_batch.hip tangent_build: the ops of grad_build transposed; the same for every
 * instance), or 0 where its gate says that the side takes no part (s_gate: as o_gate).  One workgroup per instance, numbered as in
 * k_data_grad; phase 1 is its phase 1 without the direction; phase 2 runs the lanes along the seed entries, every lane sums its
 * own list: no atomics, the same bits on every run.  An instance whose solve failed gets an all-zero seed row. */
struct TanTerm
{
    int te, si;
    double c;
};

static __global__ void __launch_bounds__(GQP_GRAD_THREADS) k_data_tangent(double *seed, int nb, int slen, const double *tangent, int len, const int *row,
                                                                         const TanTerm *terms, const int *s_gate, int olen, const int *o_arr,
                                                                         const int *o_elem, const int *o_gate, GArrTable T, GArrU64 amask,
                                                                         const int *status, int per)
{
    GQP_DYN_SHARED(lds);
    double *S = lds;
    const int bx = blockIdx.x, tid = threadIdx.x;
    const int i = (bx % GQP_GRAD_XCD) * per + bx / GQP_GRAD_XCD;
    if (i >= nb) return;
    double *out = seed + (size_t) i * (size_t) slen;
    if (status[i] != 0)
    {
        for (int e = tid; e < slen; e += GQP_GRAD_THREADS) out[e] = 0.0;
        return;
    }
    for (int e = tid; e < olen; e += GQP_GRAD_THREADS)
    {
        const int a = o_arr[e], g = o_gate[e];
        double s = 0.0;
        bool on = a >= 0 && g != -2;
        if (on && g >= 0) on = (GATL(amask, g >> 6) >> (g & 63)) & 1;
        if (on) s = GATL(T.a[a], o_elem[e]);
        S[e] = s;
    }
    __syncthreads();
    const double *tan = tangent + (size_t) i * (size_t) len;
    for (int e = tid; e < slen; e += GQP_GRAD_THREADS)
    {
        const int g = s_gate[e];
        bool on = g != -2;
        if (on && g >= 0) on = (GATL(amask, g >> 6) >> (g & 63)) & 1;
        double v = 0.0;
        if (on)
            for (int q = row[e]; q < row[e + 1]; q++)
            {
                const TanTerm t = terms[q];
                v += t.c * tan[t.te] * (t.si >= 0 ? S[t.si] : 1.0);
            }
        out[e] = v;
    }
}

/* the cotangent of the primal outputs (OUTPUT blob layout) as seed of the adjoint sweeps: entry e goes to element c_elem[e] of
 * rg (c_kind 1; u x), rgs (2; sl su), or only to the cotangent copy (3; a fixed variable: its row takes no seed); pi lam t (c_kind 0)
 * must be zero -- a nonzero one raises *bad.  Every u / x entry is also kept in `cot` (the fixed variables' own term of op 3).
 * Grid (elements / 256, instances). */
static __global__ void __launch_bounds__(256) k_adj_seed(const double *blob, int nb, int len, const int *c_kind, const int *c_elem, GArr rg,
                                                         GArr rgs, GArr cot, int *bad)
{
    const int i = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb || e >= len) return;
    const double v = blob[(size_t) i * len + e];
    const int kd = c_kind[e];
    if (kd == 0)
    {
        if (v != 0.0) *bad = 1;
        return;
    }
    if (kd == 2) { GATL(rgs, c_elem[e]) = v; return; }
    GATL(cot, c_elem[e]) = v;
    if (kd == 1) GATL(rg, c_elem[e]) = v;
}

/* the cotangent of the WHOLE output blob as seed of the adjoint sweeps (the transpose of the read-back of k_data_tangent's solve):
 * entry e goes, times c, to element dst of the seed array `slot` of T (the table of _sens_set_bulk: rg rgs rb rd; -1: to none) and,
 * as it is, to element cot of the cotangent copy (u x; -1: no copy).  The table (host-built, gpu_batch.hip seed_all_build) is the
 * same for every instance:
 *   u x        rg, and the copy; a fixed variable: the copy only (its row takes no seed)
 *   sl su      rgs
 *   pi         rb of the dynamics it is the multiplier of
 *   lam        rd of its side, where the side takes part (gate: activity bit stage_word * 64 + bit; an equality-flagged row has
 *              slot -1), with the cotangent of t folded in: lam dt + t dlam = 0 along every direction of the sweeps, so
 *              <g_lam, dlam> + <g_t, dt> = <g_lam - (t / lam) g_t, dlam>.  g_t is entry `part` of the same row, lam and t are
 *              element le of the batch's arrays; where lam is not > 0 the t term is dropped
 *   t          nothing: its lam lane consumes it
 * One writer per destination, plain stores; an instance whose solve failed writes nothing (its seeds stay 0).
 * Grid (elements / 256, instances): consecutive lanes read consecutive words of the instance's row. */
struct SeedOp
{
    int slot, dst, cot, gate, le, part;
    double c;
};

static __global__ void __launch_bounds__(256) k_adj_seed_all(const double *blob, int nb, int len, const SeedOp *ops, GArrTable T, GArr cot, GArr lam,
                                                             GArr t, GArrU64 amask, const int *status)
{
    const int i = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb || e >= len || status[i] != 0) return;
    const SeedOp o = ops[e];
    if (o.slot < 0 && o.cot < 0) return;
    const double *row = blob + (size_t) i * len;
    double v = row[e];
    if (o.cot >= 0) GATL(cot, o.cot) = v;
    if (o.slot < 0) return;
    if (o.gate >= 0)
    {
        if (!((GATL(amask, o.gate >> 6) >> (o.gate & 63)) & 1)) return;
        const double l = GATL(lam, o.le);
        if (l > 0.0) v -= GATL(t, o.le) / l * row[o.part];
    }
    GATL(T.a[o.slot], o.dst) = o.c * v;
}

} // namespace gqp

#endif

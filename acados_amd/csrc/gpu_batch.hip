/*
 * gpu_batch.hip -- host side of the device-resident OCP-QP batch: HBM allocation, layout
 * conversion (pack / unpack kernels), kernel dispatch by shape, and the IPM launch loop.
 * C-ABI declared in include/acados_amd/ocp_qp_gpu_batch.h.
 */
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <climits>
#include <vector>

#include "acados_amd/ocp_qp_gpu_batch.h"
#include "gpu_ipm_internal.h"
#include "ipm_kernels.hpp"
#include "ipm_kernels_box.hpp"
#include "ipm_kernels_box_small.hpp"
#include "ipm_kernels_wpi.hpp"
#include "ipm_kernels_w16.hpp"
#include "ipm_kernels_w16r.hpp"
#include "ipm_kernels_w16t.hpp"
#include "ipm_kernels_wpi_mfma.hpp"
#include "res_kernels.hpp"
#include "pcond_kernels_w16.hpp"
#include "pcond_kernels_mfma.hpp"
#include "dense_kernels.hpp"
#include "grad_kernels.hpp"
#include "kernel_sets.h"

/* a failing HIP call is not something a solve can recover from (lost device, out of HBM): message + exit(1), acados'
 * convention for errors that are not a solver status (`printf(...); exit(1);` throughout acados/ocp_qp/); what a solve
 * itself can report -- NaN, MAXITER, MINSTEP, infeasible -- comes back per instance as acados return codes */
/* ... with one exception (round-3 review): a HIP error is not the caller's mistake, and n host threads of an MPC fleet may
 * share this process (rendezvous mode).  HIPCHK reports and THROWS; every extern "C" entry that does device work catches at
 * the boundary (function-try-block) and returns -1 (NULL for the creators): the adapters turn that into ACADOS_QP_FAILURE
 * for the instances of the call, the process lives on.  No exception ever crosses the C-ABI. */
struct gqp_hip_failure { int code; };
#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess)                                                                  \
        {                                                                                      \
            fprintf(stderr, "\nerror: acados_amd: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            throw gqp_hip_failure{(int) e_};                                                   \
        }                                                                                      \
    } while (0)

namespace
{

/* compiled shape classes; a batch is served by the cheapest one that covers it */
const KernelSet g_ksets[] = {
    GQP_KSET(4, 1, 0, 0),
    GQP_KSET(4, 1, 2, 3),
    GQP_KSET(4, 4, 0, 0), /* child shape of (4,1) condensed in blocks of <= 4 */
    GQP_KSET(8, 3, 0, 0),
    GQP_KSET(12, 3, 0, 0),
};

/* sixteen-lanes-per-instance sweeps (ipm_kernels_w16.hpp): compiled (NX, NU) with nu + nx <= 16 */
struct W16Set
{
    int NX, NU, NG; /* NG > 0: two-rows-per-lane GEN kernels (general rows + one slack per row) in the SOFT slots */
    kern_redo_t fact, rhs, faff, fcor;
    kern_redo_t sfact, srhs, sfaff, sfcor; /* SOFT variants: soft box rows, one slack per row */
    size_t shmem;
    kern_redo_t solve, ssolve; /* the whole solve in one launch (small batches); null: launch per sweep only */
    kern_redo_t tfact;         /* two-rows shapes, box rows: the factor sweep on 4 x 4 MFMA tiles (ipm_kernels_w16t.hpp), the default */
    size_t tshmem;
};
#define GQP_W16(NX, NU)                                                                                       \
    {NX, NU, 0, gqp::kx_factor<NX, NU>, gqp::kx_backrhs<NX, NU>, gqp::kx_fwd<NX, NU, false>, gqp::kx_fwd<NX, NU, true>, \
     gqp::kx_factor<NX, NU, true>, gqp::kx_backrhs<NX, NU, true>, gqp::kx_fwd<NX, NU, false, true>,            \
     gqp::kx_fwd<NX, NU, true, true>, 4 * gqp::W16Lds<NX, NU>::SZ * sizeof(double), gqp::kx_solve<NX, NU>, gqp::kx_solve<NX, NU, true>, \
     nullptr, 0}
/* ... and with 17 <= nu + nx <= 32 (ipm_kernels_w16r.hpp: two rows per lane; box rows without slacks) */
#define GQP_W16R(NX, NU)                                                                                      \
    {NX, NU, 0, gqp::ky_factor<NX, NU>, gqp::ky_backrhs<NX, NU>, gqp::ky_fwd<NX, NU, false>, gqp::ky_fwd<NX, NU, true>, \
     nullptr, nullptr, nullptr, nullptr, 4 * gqp::W16RLds<NX, NU>::SZ * sizeof(double), nullptr, nullptr,                \
     gqp::kt_factor<NX, NU>, 4 * gqp::W16TLds<NX, NU>::SZ * sizeof(double)}
/* ... with general rows and slacks (one slack per row): the C4 class; the same kernels at nu + nx <= 16 (R = 1 row per lane:
 * <12,4,4>, <8,3,4>) put general rows + slacks of the small shapes on the sixteen-lanes family too */
#define GQP_W16G(NX, NU, NG)                                                                                  \
    {NX, NU, NG, nullptr, nullptr, nullptr, nullptr, gqp::ky_factor<NX, NU, NG>, gqp::ky_backrhs<NX, NU, NG>,     \
     gqp::ky_fwd<NX, NU, false, NG>, gqp::ky_fwd<NX, NU, true, NG>, 4 * gqp::W16RLds<NX, NU, NG>::SZ * sizeof(double), nullptr, nullptr, \
     gqp::kt_factor<NX, NU, NG>, 4 * gqp::W16TLds<NX, NU, NG>::SZ * sizeof(double)}
/* ... the same on register rows only (ky_factor): the tile sweep of this instantiation does not fit the register file
 * (kt_factor<24,3,8>: 6 spilled VGPRs; spill traffic is HBM traffic there -- the ISA lint of `make` refuses it) */
#define GQP_W16G_ROWS(NX, NU, NG)                                                                             \
    {NX, NU, NG, nullptr, nullptr, nullptr, nullptr, gqp::ky_factor<NX, NU, NG>, gqp::ky_backrhs<NX, NU, NG>,     \
     gqp::ky_fwd<NX, NU, false, NG>, gqp::ky_fwd<NX, NU, true, NG>, 4 * gqp::W16RLds<NX, NU, NG>::SZ * sizeof(double), nullptr, nullptr, \
     nullptr, 0}
const W16Set g_w16_sets[] = {GQP_W16(4, 1), GQP_W16(8, 3), GQP_W16(12, 3), GQP_W16(4, 4), GQP_W16(12, 4),
                             GQP_W16R(8, 15), GQP_W16R(24, 6), GQP_W16G(24, 3, 4), GQP_W16G_ROWS(24, 3, 8), GQP_W16G(12, 4, 4), GQP_W16G(8, 3, 4)};

/* condensing of the box-only class on register rows, sixteen lanes per block (pcond_kernels_w16.hpp): compiled
 * (NX, NU, block size) with nx + bs * nu <= 32 */
struct PcondzSet
{
    int NX, NU, BS;
    kern_pcond_t cond;
    size_t shmem;
    kern_pcond_t cond_m; /* the same contraction on the FP64 matrix pipe, v_mfma_f64_4x4x4_4b_f64 (pcond_kernels_mfma.hpp): the default */
};
#define GQP_PCONDZ(NX, NU, BS) {NX, NU, BS, gqp::kz_pcond<NX, NU, BS>, 4 * gqp::PcondzLds<NX, NU, BS>::SZ * sizeof(double), gqp::km_pcond<NX, NU, BS>}
const PcondzSet g_pcondz_sets[] = {GQP_PCONDZ(8, 3, 5), GQP_PCONDZ(4, 1, 4)};

/* The kernel family of a batch: the answer to DESIGN.md 4's table -- which kernels serve this shape and batch size, on which
 * mapping of instances to lanes, in which array layout, with how much dynamic LDS per launch kind -- as ONE record.  choose_family()
 * fills it from the dims and the batch size, family_structure() finishes it once idxb / idxs_rev / idxe are known
 * (finalize_structure), ric_configure() swaps it for ric_alg 0 and back, a compaction level copies its parent's whole; every reader
 * (pick_kernels, launch_level, wpi_lds_attributes, the scalars) goes through it.  Both functions stand in front of
 * batch_create_shape. */
enum FamilyMap { MAP_LANE, MAP_W16, MAP_WPI }; /* one instance per lane / sixteen lanes per instance / one wave per instance */
struct FamilyLds /* dynamic LDS bytes per launch kind (one instance per lane: none) */
{
    size_t fact = 0;  /* factor sweep (the tile sweep of the small two-rows shapes runs two waves per SIMD: its own, smaller tile) */
    size_t rhs = 0;   /* rhs sweep; the whole-solve kernel of the sixteen-lanes family */
    size_t fwd = 0;   /* forward sweeps (wave per instance: one factor buffer instead of two) */
    size_t whole = 0; /* init and finalize: wave-per-instance kernels in every family but one instance per lane */
};
struct Family
{
    FamilyMap map = MAP_LANE;
    int aos = 0;       /* instance-major arrays: every family but one instance per lane */
    int AW = 1;        /* activity words per stage (64 inequality sides each); 2 only on wave per instance */
    const KernelSet *compiled = nullptr; /* one instance per lane: the compiled shape class that serves the batch */
    KernelSet own_ks;  /* every other mapping: the kernel set put together for the padded dims */
    FamilyLds lds;
    KernelSet wpi_ks;  /* soft sixteen-lanes family: the wave-per-instance set of the same padded dims and its LDS bytes, what the */
    FamilyLds wpi_lds; /* batch falls back to if the slack structure is not one-slack-per-row (family_structure) */
    bool soft = false; /* sixteen lanes: soft box rows (one slack per row) */
    int ng = 0;        /* ... of the GEN two-rows-per-lane set: general rows per stage it carries (slacks on them too) */
    int tiles = 0;     /* ... two-rows family: factor sweep on 4 x 4 MFMA tiles (kt_factor) */
    kern_redo_t solve = nullptr; /* ... whole-solve kernel (batches of at most solve_max instances) */
    bool mfma = false; /* wave per instance: the factor sweep is the blocked-Cholesky / MFMA kernel (17 <= n <= 32) */
    bool use_box = false;  /* box-only fast path */
    int xbox = 0;          /* an inequality row on a state */
    bool kb_plain = true;  /* one-instance-per-lane box batch: the phase-ordered kernels (false: the pipelined small-block ones) */
    std::string name;      /* family_name() of the record and the ric_alg it serves */

    bool lane() const { return map == MAP_LANE; }
    bool w16() const { return map == MAP_W16; }
    const KernelSet *ks() const { return map == MAP_LANE ? compiled : &own_ks; }
};

/* The ACADOS_AMD_* switches that steer the family (cross-checks, tests, tools), as family_switches() reads them */
struct Switch
{
    bool set = false;
    int v = 0;
    bool off() const { return set && v == 0; }
    bool on() const { return set && v != 0; }
};
struct FamilySwitches
{
    Switch wpi, wpi_v1, wpi_batch_max, w16, w16r, w16g, w16t, w16t_gen, wpi_mfma, wpi_mfma_pf, wpi_ct, w16_lds_align; /* choose_family */
    Switch general_kernels, kb_small; /* family_structure */
    Switch ext_update, w16_perm;      /* every solve (run_ipm) */
};

/* what choose_family is told of the dims, and what a caller may pin */
struct DimsSummary
{
    int mx = 0, mu = 0, mg = 0, ms = 0; /* largest nx, nu, ng, ns of a stage */
    int nct_max = 0;                    /* most inequality sides of a stage, 2 (nb + ng) + 2 ns */
    bool xbox_dims = false;             /* state bounds after stage 0 */
};
struct ForcedChoice
{
    int NX = 0, NU = 0;             /* padded dims to match exactly (the condensed batch) */
    const Family *parent = nullptr; /* a sub-batch: the family of the batch it takes instances from ... */
    bool wpi = false;               /* ... false: a compaction level, which runs that very family; true: the tail, classical-Riccati
                                       and sensitivity roles, wave per instance at exactly the parent's padded dims */
};
struct FamilyChoice
{
    bool ok = false;
    Family f;
    std::string refusal; /* !ok: the message */
};

} // namespace

/* Sub-batches that take instances of a batch over (sub_batch_create / _load / _store below), created on first use:
 * the still-iterating instances in a dense batch of the same family (next level of run_ipm, capacity <= B/2), and three
 * wave-per-instance batches at the padded dims: the tail for the last survivors of a one-instance-per-lane level, the one every
 * ric_alg 0 solve of such a batch is handed to, the one its sensitivities run in slice by slice.  (The condensed batch `child` of
 * partial condensing is a different QP, not a subset of the instances: not one of them) */
enum SubRole { SUB_COMPACT, SUB_TAIL, SUB_RIC0, SUB_SENS, SUB_ROLES };
struct SubBatch
{
    ocp_qp_gpu_batch *c = nullptr;
    int *d_list = nullptr; /* instance index (in the parent) of every slot of `c`; lives as long as the parent */
    int list_cap = 0;
    int cap = 0;           /* instances `c` was made for */
};

/* Blobs: all QP data / a whole iterate / every seed of every instance as ONE instance-major array, moved by one copy and one
 * launch per direction ("Blobs"; the bulk section below).  One map per kind, built on first use (blob_map); what a
 * kind consists of is its row of k_blobs.  Every kind's map carries every pointer: d_sgn / d_elem2 are filled for BLOB_SEED only
 * and d_moff / d_mstage / d_mbit are empty tables where a kind has no mask entry (nm == 0) -- a member per kind would take a
 * variant or a second struct beside the array of maps, more than the two null pointers cost */
enum BlobKind { BLOB_IN, BLOB_OUT, BLOB_VEC, BLOB_SEED, BLOB_KINDS };
struct BulkMap
{
    bool built = false;
    int len = 0, nm = 0;
    std::vector<std::string> fields; /* per segment */
    std::vector<int> seg_row, seg_stage, seg_off, seg_len; /* (seg_row: the field's row of k_fields) */
    bool writes_dyn = false, writes_hess = false; /* a scatter of the kind writes [B A]' / RSQ: no stored held verdict stays */
    std::vector<int> arr, elem;      /* per entry: array of T (-1: none) and element in it; d_arr / d_elem are these (grad_build reads them) */
    int *d_arr = nullptr, *d_elem = nullptr, *d_moff = nullptr, *d_mstage = nullptr, *d_mbit = nullptr;
    int *d_sgn = nullptr, *d_elem2 = nullptr; /* seed blob only: sign of the entry in the residual arrays, slot in sfix */
    int *d_arr_g = nullptr, *d_elem_g = nullptr; /* READ direction: d_arr / d_elem themselves, except for the input blob
                                                    (_get_bulk_in): the strict upper triangles of Q and R (not written: only the
                                                    lower triangle of the caller's block is valid) are read from the mirrored element */
    gqp::GArrTable T;
};

/* Held dynamics of the one-instance-per-lane box sweeps (ipm_kernels_box.hpp), the host's side, owned by the root batch.  One
 * root loop (run_ipm; the polish pass is a root loop of its own) goes DETECTING -> AWAITING -> COUNTED: begin() zeroes
 * GqpDev::tile_inv; the first affine forward sweep runs with bits(true) and counts the lanes with stage-invariant [B A]' into it;
 * after_detect() copies the counters back and records an event behind the copy; before_factor(), at the top of the next iteration,
 * waits for that event -- not for the stream -- and counts the full tiles; from then on all_held() says whether a launch may take
 * the held entries; end() zeroes tile_inv again, so every other launch of these kernels (sub-levels, sensitivities, a later solve)
 * finds the counters at zero.
 *   Verdicts outlive the solve.  What the detector finds is a property of the resident matrices: every writer of GqpDev::BAt /
 *   RSQ of a root batch bumps ver_dyn / ver_hess (data_written), a solve's count is stored with the version it was taken at, and a
 *   root loop that finds the stored version current starts COUNTED -- counters copied from d_kept, no detect bit, no read-back, no
 *   event wait, iteration 1 on the held entries.  The polish pass always detects for itself.  A count is stored only where every
 *   instance was still running when the detecting sweep was launched (a wave without a running lane leaves that sweep before it
 *   counts: such a count says less than the data) or where it is full anyway.
 *   Held Hessian: where every tile is held and the held factor entry exists, hessian_verdict() runs gqp::k_hess_invariant once per
 *   ver_hess and the held factor launches read one copy of RSQ (GqpOpts::hold bit 2) while the verdict is current and positive.
 * Methods: in front of run_ipm. */
#ifndef GQP_COMPACT_HELD /* (development builds: the other default, for A/B runs of bench.py) */
#define GQP_COMPACT_HELD 0
#endif
struct HeldDynamics
{
    /* the last solve: scalars "tiles_invariant" (of the solve's own loop, or the stored count it started from), "fact_held_launches"
     * / "rhs_held_launches" (launches of IpmKernels::fact_held / rhs_held, the polish pass's included), "hess_held_launches" (those
     * of fact_held with hold bit 2), "hess_detector_runs", "detecting_sweeps" (1 where the solve's own loop ran the detecting sweep,
     * 0 where it started from a stored count), "level_held_launches" (those of the held launches above that a dense held level
     * made, see adopt()), "slim_dyn_copies" / "slim_hess_copies" (hand-overs whose gather of BAt / RSQ read two stage slots per
     * instance, sub_batch_load); reset by ocp_qp_gpu_batch_solve */
    int tiles_invariant = 0, fact_launches = 0, rhs_launches = 0, hess_launches = 0, hess_detects = 0, detects = 0;
    int level_launches = 0, slim_dyn = 0, slim_hess = 0;
    hipEvent_t ev = nullptr; /* recorded behind the read-back of the counters */
    /* the data and what is known about it (0 is no version: nothing is known at the start) */
    unsigned ver_dyn = 1, ver_hess = 1;  /* versions of the arrays behind [B A]' and of RSQ */
    unsigned kept_at = 0;                /* ver_dyn the stored count was taken at */
    int kept_tiles = 0;                  /* ... the count, its counters in d_kept */
    int *d_kept = nullptr;               /* [Bp / 64], beside GqpDev::tile_inv */
    unsigned hess_at = 0;                /* ver_hess the Hessian verdict was taken at */
    bool hess_inv = false;               /* ... the verdict: RSQ of every instance is the same at the stages 0 .. N-1 */
    int *d_hess_cnt = nullptr;           /* [Bp / 64] agreeing lanes per tile, written by k_hess_invariant */
    unsigned pending_ver = 0;            /* ver_dyn at the detecting sweep of this loop; 0: its count is not to be stored */
    bool complete = false;               /* ... every instance was running when that sweep was launched: every wave counted */
    /* the root loop that runs */
    ocp_qp_gpu_batch *b = nullptr; /* null: a sub-level's record, which does nothing (but see adopt()) */
    bool enabled = false;          /* option hold_dynamics on a one-instance-per-lane box batch */
    bool polish = false;           /* the loop of the polish pass: its count stays its own */
    bool level = false;            /* the record of a dense held level while its loop runs (adopt()) */
    enum { DETECTING, AWAITING, COUNTED } state = COUNTED;
    int tiles = 0;                 /* full tiles this loop counted */

    void begin(ocp_qp_gpu_batch *root, hipStream_t s, bool polish_loop);
    /* GqpOpts::hold of a launch of this loop: bit 0 tiles with a full counter hold; bit 1 (the affine sweep while DETECTING) count */
    int bits(bool affine_sweep = false) const { return !enabled ? 0 : (affine_sweep && state == DETECTING) ? 3 : 1; }
    void after_detect(hipStream_t s, bool all_running);
    void before_factor(bool fact_entry);
    void stream_drained();
    void count();
    bool all_held() const;
    /* is the Hessian of every instance stage-invariant?  Asked where a held factor launch is about to go out; runs the detector
     * (one launch, one read-back, one wait for the stream) where ver_hess has moved since the stored verdict */
    bool hessian_verdict(hipStream_t s);
    void end(hipStream_t s);
    /* the record of a dense level that an all-held root loop made of its survivors (option compact_held): every tile of its `cnt`
     * slots holds, by the root's count; the Hessian verdict is the root's.  It starts COUNTED, so it never detects, never waits and
     * never stores a count; its launches are counted into the root's scalars (run_ipm); end() switches it off again */
    void adopt(ocp_qp_gpu_batch *level, int cnt, bool root_hess_inv);
    /* the verdicts a hand-over may use WITHOUT asking for one: [B A]' of every instance is stage-invariant / so is RSQ */
    bool dyn_known() const { return all_held(); }
    bool hess_known() const { return hess_at == ver_hess && hess_inv; }
    /* a writer of a root batch's matrices: the arrays behind [B A]' (dyn) and / or RSQ (hess) are not what they were */
    void data_written(bool dyn, bool hess) { if (dyn) ver_dyn++; if (hess) ver_hess++; if (!ver_dyn) ver_dyn = 1; if (!ver_hess) ver_hess = 1; }
};

struct ocp_qp_gpu_batch
{
    int B = 0, Bp = 0, N = 0, device = 0;
    std::vector<int> nx, nu, nbx, nbu, nb, ng, ns, nbxe;
    std::vector<std::vector<int>> idxb, idxs_rev, idxe; /* as given (original row order) */
    std::vector<std::vector<int>> perm;                   /* original box row -> sorted row */
    bool finalized = false;
    Family fam;            /* the kernel family that serves the batch (choose_family, family_structure, ric_configure) */
    int w16_slots = 0;     /* row slots a sweep launch covers: B, or the live instances once GqpDev::perm lists them */
    int *d_side_map = nullptr; /* k_step_update: side -> stage * 128 + activity bit (-1: equality-flagged row), built on first use */
    int solve_max = 256;   /* largest batch that is solved in one launch (option "solve_max", 0 = off) */
    int n_single_launch = 0;
    std::vector<GqpStage> st;
    GqpStage *d_st = nullptr;
    GqpDev D = {};
    GqpOpts O;
    bool has_slack = false;            /* some stage has slack variables (set with the dims) */
    /* full condensing of any size (option "full_dense": dense_kernels.hpp, dense_solve below) */
    int full_dense = 0;
    gqp::KdRow *d_kd_rows = nullptr;
    gqp::KdDims kd = {};
    int kd_unsupported = 0;
    double *d_kd_ws = nullptr;
    int kd_slice = 0;
    int full_dense_slice = 0;          /* option "full_dense_slice": instances per kd_solve launch (0: as many as 8 GiB of workspace hold) */
    /* terminal polishing step (option "polish", opt-in: polish_pass below) */
    int polish = 0;
    double polish_ratio = 1e-3;
    double polish_min = 0.0; /* ... and min(lam, t) above this (absolute): a pair whose smaller member is already below the accuracy wanted cannot move the point by more */
    int n_polished = 0, n_polish_reverted = 0;
    int *d_pol_status = nullptr, *d_pol_iter = nullptr, *d_pol_flag = nullptr, *d_pol_cnt = nullptr;
    double *d_pol_sc = nullptr;
    GArr pol_ux = {nullptr, 0, 0}, pol_sv = {nullptr, 0, 0}, pol_pi = {nullptr, 0, 0}, pol_lam = {nullptr, 0, 0}, pol_t = {nullptr, 0, 0};
    double tol_comp_soft_scale = 1.0; /* effective_opts: opt-in tighter exit on complementarity of a soft-constrained class (1 = the tolerance as given, the reference's semantics) */
    int nct_tot = 0, ns2_tot = 0, ng_tot = 0;
    std::vector<void *> allocs;
    size_t bytes = 0;
    double *d_stage = nullptr; /* staging for host->device field blocks */
    double *d_chunks = nullptr; /* the input blob handed over in pieces (_set_bulk_chunk): its own buffer -- d_stage is reused by */
    size_t chunks_cap = 0;      /* every other transfer (a hot start's _set_bulk_out comes between the chunks and the scatter) */
    /* zero-copy gather (ocp_qp_gpu_batch_gather_tables / _gather_run): word tables of the full input blob [BLOB_IN] and of its vector part [BLOB_VEC] */
    struct GatherTab { int P = 0, n_words = 0, full = 0; int *d_slot = nullptr, *d_off = nullptr, *d_pos = nullptr; unsigned char *d_neg = nullptr; } gtab[BLOB_KINDS];
    const double **d_gptrs = nullptr;
    size_t gptrs_cap = 0;
    long chunks_got = 0;        /* instances handed over since the last _set_bulk_staged (it refuses to scatter a partial blob) */
    hipEvent_t chunks_ev = nullptr; /* recorded in front of the first chunk of a round: time_pack covers copies + scatter as _set_bulk's does */
    size_t stage_cap = 0;
    int *d_map = nullptr;
    int map_cap = 0;
    int *h_nact = nullptr; /* pinned */
    int *d_perm = nullptr, *d_perm_cnt = nullptr; /* sixteen-lanes sweeps: dense list of the still-iterating instances */
    int *h_ints = nullptr; /* pinned, 2 * Bp ints: per-instance status / iteration read-backs of a solve (no heap traffic per call) */
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double time_tot = 0.0, time_pack = 0.0;
    int last_iters = 0, launches = 0;
    int print_level = 0;
    double t0_min = 1e-16, lam0_min = 1e-16; /* lower clips of t / lam at a hot start (HPIPM args of the same name) */
    int profile = 0;                 /* per-kernel-class HIP event timing on the launch stream */
    int stream_priority = 0;         /* HIP stream priority of this batch and of the sub-batches it creates (0: default) */
    std::vector<hipEvent_t> prof_ev; /* pool, pairs (start, stop) */
    std::vector<int> prof_cls;       /* kernel class of each recorded pair */
    double prof_ms[6] = {0, 0, 0, 0, 0, 0};
    int prof_cnt[6] = {0, 0, 0, 0, 0, 0};
    int stat_inst = 0, stat_rows = 0;
    /* partial condensing (pcond_kernels.hpp) */
    int cond_N = 0;                 /* requested N2; 0 or N = full space */
    int cond_keep_iterate = 0;      /* hot start of a condensed solve from the child's own last iterate (not from the root's) */
    std::vector<int> user_blocks;   /* cond_block_size (N2 entries) or empty: N/N2 each, remainder to the first blocks */
    int pcond_state = 0;            /* 0 unchecked, 1 active, -1 not applicable (message printed once) */
    ocp_qp_gpu_batch *child = nullptr;
    const PcondSet *pc = nullptr;   /* compiled one-instance-per-lane condensing kernels, or ... */
    int pc_rt = 0;                  /* ... the run-time-shaped wave-per-instance ones (kw_pcond / kw_pexpand) */
    int pc_lane_expand = 0;         /* the expansion runs on the compiled one-instance-per-lane kernel although condensing does not */
    const PcondzSet *pcz = nullptr; /* condensing on register rows, sixteen lanes per block (box-only class, compiled shapes) */
    int pcz_mfma = 1;               /* ... on the FP64 matrix pipe (km_pcond); ACADOS_AMD_PCOND_MFMA=0: on register rows with DPP broadcasts (kz_pcond) */
    size_t pc_shmem = 0;
    std::vector<int> blk_start;
    gqp::PcondMap pmap;
    double time_xcond = 0.0;
    bool lhs_ready = false;         /* condense_lhs done: the next solve only condenses the vector part */
    SubBatch sub[SUB_ROLES];
    int compact_min = 1 << 30;           /* levels smaller than this are not compacted; off by default: it only
                                            pays once every sweep kernel is bandwidth-bound */
    int tail_max = 12288;                /* switch to the tail sub-batch when at most this many instances (and 1 / tail_div of the ROOT batch, at every level) remain; 0 = off */
    int tail_div = 4;
    int n_tail_switches = 0;
    /* held dynamics of the one-instance-per-lane box sweeps (ipm_kernels_box.hpp; run_ipm) */
    int hold_dynamics = 1;               /* option: 1 = tiles whose [B A]' is found stage-invariant keep it in registers, 0 = never */
    int hold_hessian = 1;                /* option: 1 = held factor launches read one copy of a stage-invariant RSQ, 0 = every stage its own */
    int compact_held = GQP_COMPACT_HELD; /* option: 1 = a level of at least compact_held_min instances whose tiles all hold continues in a dense level that
                                            stays on the held entries once half of it has converged (run_ipm), 0 = never */
    int compact_held_min = 32768;
    HeldDynamics held;                   /* the protocol of the root loop, what the last solve counted and what is known of the data */
    /* solution sensitivities / factor at the solution */
    bool factor_stale = false;           /* the last solve finished instances on a sub-level: Lf of the root is not theirs */
    bool sens_open = false;              /* seeds are being collected (rg, rb, rd hold seeds, not residuals) */
    GArr sfix = {nullptr, 0, 0};         /* derivative of the equality-flagged variables (e.g. x0), [N+2][n] */
    int *d_saved_status = nullptr;
    /* Riccati recursion (option "ric_alg"): 1 square-root (every family), 0 classical (wave-per-instance sweeps only, RIC0 of
     * ipm_kernels_wpi.hpp).  A wave-per-instance-layout batch swaps its family in place (ric1_fam keeps what it replaced); a
     * one-instance-per-lane batch hands every solve to sub[SUB_RIC0], a wave-per-instance batch at its padded dims */
    int ric_alg = 1;
    Family ric1_fam;         /* ... the family ric_alg 1 runs on, kept while ric_alg 0 is on (ric_configure) */
    bool ric1_saved = false;
    int n_compactions = 0;
    /* KKT residuals of the current (data, iterate) on demand (res_kernels.hpp) */
    gqp::ResOut R = {{nullptr, 0, 0}, {nullptr, 0, 0}, {nullptr, 0, 0}, {nullptr, 0, 0}, {nullptr, 0, 0}, nullptr, 0};
    /* bulk pack / unpack (one H2D + one launch per direction) */
    BulkMap blob[BLOB_KINDS];
    /* reverse-mode data gradients (grad_kernels.hpp): op table over the input blob, gather / gate table of the output blob,
     * cotangent scatter table, the cotangent itself in the ux layout (the fixed variables' own term) */
    struct GradMap
    {
        bool built = false;
        int len = 0, olen = 0;
        size_t lds = 0;
        gqp::GradOp *d_ops = nullptr;
        gqp::GradTerm *d_terms = nullptr;
        int *d_oarr = nullptr, *d_oelem = nullptr, *d_ogate = nullptr, *d_ckind = nullptr, *d_celem = nullptr, *d_bad = nullptr;
        GArr cot = {nullptr, 0, 0};
        bool seeded = false; /* an adjoint seed is in the residual arrays: data_grad may run */
        /* forward mode (k_data_tangent, tangent_build): the ops transposed into one term list per entry of the seed blob, the
         * gates of its bound entries, the seed blob of the batch */
        std::vector<gqp::GradOp> h_ops; /* host copy of d_ops: what tangent_build transposes */
        bool tan_built = false;
        int slen = 0;
        int *d_trow = nullptr, *d_sgate = nullptr;
        gqp::TanTerm *d_tterms = nullptr;
        double *d_seed = nullptr;
        /* the adjoint seed of a cotangent on the whole output blob (k_adj_seed_all, seed_all_build): one entry per output entry */
        std::vector<int> h_ckind, h_ogate; /* host copies of d_ckind / d_ogate: what seed_all_build reads */
        bool all_built = false;
        gqp::SeedOp *d_sops = nullptr;
    } grad;
};

namespace
{

template <class T>
T *dalloc(ocp_qp_gpu_batch *b, size_t cnt)
{
    void *p = nullptr;
    size_t bytes = sizeof(T) * (cnt ? cnt : 1);
    HIPCHK(hipMalloc(&p, bytes));
    HIPCHK(hipMemset(p, 0, bytes));
    b->allocs.push_back(p);
    b->bytes += bytes;
    return (T *) p;
}

/* gives back ONE array of dalloc (bytes as it was asked for) that is about to be replaced by another size */
void dfree(ocp_qp_gpu_batch *b, void *p, size_t bytes)
{
    HIPCHK(hipStreamSynchronize(b->stream));
    b->allocs.erase(std::find(b->allocs.begin(), b->allocs.end(), p));
    b->bytes -= bytes ? bytes : sizeof(double);
    HIPCHK(hipFree(p));
}

/* wave-tiled per-instance array with E elements per instance (gpu_ipm_internal.h, GArrT) */
template <class T>
GArrT<T> garr(ocp_qp_gpu_batch *b, size_t E)
{
    GArrT<T> a;
    a.aos = b->fam.aos;
    a.E = (int) (E ? E : 1);
    a.p = dalloc<T>(b, (size_t) a.E * (size_t) b->Bp);
    return a;
}

void opts_default(GqpOpts &o)
{
    /* acados defaults on top of mode BALANCE: ocp_qp_hpipm.c:101-113 */
    o.mu0 = 1e0;
    o.tol_stat = 1e-6; o.tol_eq = 1e-8; o.tol_ineq = 1e-8; o.tol_comp = 1e-8;
    o.alpha_min = 1e-8; o.tau_min = 0.0; o.lam_min = 1e-16; o.t_min = 1e-16; o.reg_prim = 1e-15;
    o.iter_max = 50; o.pred_corr = 1; o.cond_pred_corr = 1; o.warm_start = 0; o.ext_update = 0; o.hold = 0;
    o.t0_init = 2; /* acados_ocp_options.py:1128-1143: the default is the residual-based start */
}

/* options as the kernels see them.
 * (1) OPT-IN (option "tol_comp_soft_scale", default 1 = off: the solver stops at the tol_comp it is given, as HPIPM does,
 *     ocp_qp_hpipm.c:104-107).  With a value < 1, soft-constrained classes (any stage with slacks) use
 *     tol_comp * tol_comp_soft_scale in the exit test.  Why one may want it: a soft row with a small
 *     multiplier lam* sits at t = mu / lam* on the central path, and with slack penalties of 1e2 the primal solution is
 *     flat: at mu ~ 1e-8 the C4 iterate is a median 3e-7 / worst 1e-4 (relative) away from the exact solution although
 *     all four KKT residuals are <= 1e-8 (profiles/r04_c4_distance_to_solution.txt) -- two solvers stopping inside that
 *     ball cannot agree to 1e-6.  Three more orders of mu cost 1.4 iterations of 12.7 and bring it to 3e-10 / 3e-6 * sqrt.
 * (2) Barrier floor: the complementarity target never drops below 1e-3 of that tolerance (see oracle/ocp_qp_oracle.c
 *     tau_eff: below it only the rounding error of the Newton step grows). */
GqpOpts effective_opts(const GqpOpts &o, const ocp_qp_gpu_batch *b)
{
    GqpOpts e = o;
    if (b->has_slack && b->tol_comp_soft_scale > 0.0 && b->tol_comp_soft_scale < 1.0) e.tol_comp = o.tol_comp * b->tol_comp_soft_scale;
    const double f = 1e-3 * e.tol_comp;
    if (e.tau_min < f) e.tau_min = f;
    return e;
}

int padded_var(const ocp_qp_gpu_batch *b, int k, int iv)
{
    /* index in [u(nu_k); x(nx_k)] -> index in padded [u(NU); x(NX)] */
    return iv < b->nu[k] ? iv : b->fam.ks()->NU + (iv - b->nu[k]);
}

/* the classical Riccati kernel set of the wave-per-instance family at padded dims (wx, wu) */
KernelSet wpi_ric0_set(int wx, int wu, int mg, int ms)
{
    const bool gen = mg > 0 || ms > 0;
    static const kern_redo_t fact_box[8] = {gqp::kw_factor<1, false, 0, 0, true>, gqp::kw_factor<2, false, 0, 0, true>,
                                            gqp::kw_factor<3, false, 0, 0, true>, gqp::kw_factor<4, false, 0, 0, true>,
                                            gqp::kw_factor<5, false, 0, 0, true>, gqp::kw_factor<6, false, 0, 0, true>,
                                            gqp::kw_factor<7, false, 0, 0, true>, gqp::kw_factor<8, false, 0, 0, true>};
    static const kern_redo_t fact_gen[8] = {gqp::kw_factor<1, true, 0, 0, true>, gqp::kw_factor<2, true, 0, 0, true>,
                                            gqp::kw_factor<3, true, 0, 0, true>, gqp::kw_factor<4, true, 0, 0, true>,
                                            gqp::kw_factor<5, true, 0, 0, true>, gqp::kw_factor<6, true, 0, 0, true>,
                                            gqp::kw_factor<7, true, 0, 0, true>, gqp::kw_factor<8, true, 0, 0, true>};
    const int t8 = (wx + wu + 7) / 8 - 1;
    const kern_redo_t fact = gen ? fact_gen[t8] : fact_box[t8];
    const kern_redo_t rhs = gen ? gqp::kw_backrhs<true, 0, 0, true> : gqp::kw_backrhs<false, 0, 0, true>;
    const kern_redo_t faff = gen ? gqp::kw_fwd<false, true, 0, 0, true> : gqp::kw_fwd<false, false, 0, 0, true>;
    const kern_redo_t fcor = gen ? gqp::kw_fwd<true, true, 0, 0, true> : gqp::kw_fwd<true, false, 0, 0, true>;
    const kern_opts_t init = gen ? gqp::kw_init<true> : gqp::kw_init<false>;
    const kern_plain_t fin = gen ? gqp::kw_finalize<true> : gqp::kw_finalize<false>;
    return KernelSet{wx, wu, mg, ms, init, fact, rhs, faff, fcor, fin, {{fact, fact}, {rhs, rhs}, {faff, faff}, {fcor, fcor}}, fin};
}

/* ---- the kernel family of a batch: DESIGN.md 4's table in code ---- */

FamilySwitches family_switches()
{
    FamilySwitches sw;
    const struct { const char *name; Switch FamilySwitches::*m; } all[] = {
        {"ACADOS_AMD_WPI", &FamilySwitches::wpi}, {"ACADOS_AMD_WPI_V1", &FamilySwitches::wpi_v1},
        {"ACADOS_AMD_WPI_BATCH_MAX", &FamilySwitches::wpi_batch_max}, {"ACADOS_AMD_W16", &FamilySwitches::w16},
        {"ACADOS_AMD_W16R", &FamilySwitches::w16r}, {"ACADOS_AMD_W16G", &FamilySwitches::w16g},
        {"ACADOS_AMD_W16T", &FamilySwitches::w16t}, {"ACADOS_AMD_W16T_GEN", &FamilySwitches::w16t_gen},
        {"ACADOS_AMD_WPI_MFMA", &FamilySwitches::wpi_mfma}, {"ACADOS_AMD_WPI_MFMA_PF", &FamilySwitches::wpi_mfma_pf},
        {"ACADOS_AMD_WPI_CT", &FamilySwitches::wpi_ct}, {"ACADOS_AMD_W16_LDS_ALIGN", &FamilySwitches::w16_lds_align},
        {"ACADOS_AMD_GENERAL_KERNELS", &FamilySwitches::general_kernels}, {"ACADOS_AMD_KB_SMALL", &FamilySwitches::kb_small},
        {"ACADOS_AMD_EXT_UPDATE", &FamilySwitches::ext_update}, {"ACADOS_AMD_W16_PERM", &FamilySwitches::w16_perm}};
    for (const auto &e : all)
        if (const char *v = getenv(e.name)) { (sw.*e.m).set = true; (sw.*e.m).v = atoi(v); }
    return sw;
}

/* the family of the classical Riccati recursion at the padded dims of f: the RIC0 kernels of the wave-per-instance family.  What a
 * wave-per-instance-layout batch runs on while ric_alg is 0, and what a one-instance-per-lane batch hands its solves to */
Family ric0_family(const Family &f)
{
    const int wx = f.ks()->NX, wu = f.ks()->NU, mg = f.ks()->NG, ms = f.ks()->NS;
    const size_t con = gqp::wpi_con_doubles(wx + wu, mg, ms);
    Family r = f;
    r.map = MAP_WPI;
    r.own_ks = wpi_ric0_set(wx, wu, mg, ms);
    r.solve = nullptr;
    r.mfma = false;
    r.lds.rhs = r.lds.whole = (gqp::wpi3_lds_doubles(wx, wu) + con) * sizeof(double);
    r.lds.fwd = (gqp::wpi3_lds_doubles(wx, wu, 1) + con) * sizeof(double);
    r.lds.fact = (gqp::wpi2_ric0_lds_doubles(wx, wu) + con) * sizeof(double);
    return r;
}

/* the kernel name of a family as ocp_qp_gpu_batch_kernel_name reports it; ric_alg 0: of what the solves then run on */
std::string family_name(const Family &f, int ric_alg)
{
    if (ric_alg == 0 && f.lane()) return family_name(ric0_family(f), 0);
    const KernelSet &k = *f.ks();
    char nm[160];
    if (f.w16() && f.ng) snprintf(nm, sizeof(nm), "w16r-gen<NX=%d,NU=%d,NG=%d>", k.NX, k.NU, f.ng);
    else if (f.w16()) snprintf(nm, sizeof(nm), f.soft ? "w16-soft<NX=%d,NU=%d>" : k.NX + k.NU > 16 ? "w16r-box<NX=%d,NU=%d>" : "w16-box<NX=%d,NU=%d>", k.NX, k.NU);
    else if (!f.lane())
    {
        const char *tag = f.mfma ? ",mfma" : ric_alg == 0 ? ",ric0" : "";
        if (k.NG || k.NS) snprintf(nm, sizeof(nm), "wpi-gen(nx=%d,nu=%d,ng=%d,ns=%d,lds=%zuB%s)", k.NX, k.NU, k.NG, k.NS, f.lds.fact, tag);
        else snprintf(nm, sizeof(nm), "wpi-box(nx=%d,nu=%d,lds=%zuB%s)", k.NX, k.NU, f.mfma ? f.lds.fact : f.lds.rhs, tag);
    }
    else if (f.use_box) snprintf(nm, sizeof(nm), "1tpi-%s<NX=%d,NU=%d,XBOX=%d>", f.kb_plain ? "box" : "pipe", k.NX, k.NU, f.xbox);
    else snprintf(nm, sizeof(nm), "1tpi<NX=%d,NU=%d,NG=%d,NS=%d>", k.NX, k.NU, k.NG, k.NS);
    return nm;
}

/* batch thresholds of the table (measured crossovers; the rules that use them are in choose_family) */
#define GQP_WPI_MIN_N 13       /* nu+nx from which the wave-per-instance kernels serve every batch */
#define GQP_WPI_BATCH_MAX 8192 /* batch size up to which they also serve the smaller stage blocks */
#define GQP_W16_BATCH_MAX 20480 /* ... where a 16-lanes-per-instance instantiation exists (crossover of the C2 shape: ~20k) */
#define GQP_WPI_GEN_SMALL_MAX 2048   /* ... for nu + nx <= 6 with general rows / shared slacks (compiled general set) */
#define GQP_W16_SMALL_MAX 4096       /* ... against the pipelined small-block kernels (nu + nx <= 6) */
#define GQP_W16_SMALL_XBOX_MAX 12288 /* ... the same with box rows on the states */

/* Which family serves a batch of n_batch instances with these dims: the table of DESIGN.md 4.  No HIP call, no allocation, nothing
 * of a batch is touched; a refusal comes back with its message.  The switches are the cross-checks of the tests and tools. */
FamilyChoice choose_family(const DimsSummary &d, int n_batch, const ForcedChoice &forced, const FamilySwitches &sw)
{
    FamilyChoice out;
    Family &f = out.f;
    const int mx = d.mx, mu = d.mu, mg = d.mg, ms = d.ms;
    /* inequality sides per stage: 64 per activity word; the one-instance-per-lane kernels read one word, the
     * wave-per-instance ones up to two */
    if (d.nct_max > 128)
    {
        char msg[160];
        snprintf(msg, sizeof(msg), "acados_amd: a stage has %d inequality sides (2(nb+ng)+2ns > 128): unsupported\n", d.nct_max);
        out.refusal = msg;
        return out;
    }
    if (forced.parent && !forced.wpi) /* a compaction level runs the very family of its parent */
    {
        f = *forced.parent;
        out.ok = true;
        return out;
    }
    /* padded dims to match exactly: the ones given, or the parent's for its wave-per-instance sub-batches */
    const int force_NX = forced.wpi ? forced.parent->ks()->NX : forced.NX, force_NU = forced.wpi ? forced.parent->ks()->NU : forced.NU;
    /* compiled shape classes: a batch is served by the cheapest one that covers it */
    const KernelSet *lane = nullptr;
    double best = 1e300;
    auto consider = [&](const KernelSet &ks) {
        if (ks.NX < mx || ks.NU < mu || ks.NG < mg || ks.NS < ms) return;
        if (force_NX && (ks.NX != force_NX || ks.NU != force_NU || ks.NG || ks.NS)) return;
        const double n = ks.NX + ks.NU;
        const double cost = n * n * n + 10.0 * (ks.NG + ks.NS) * n * n;
        if (cost < best) { best = cost; lane = &ks; }
    };
    for (const KernelSet &ks : g_ksets) consider(ks);
    /* the rolled-loop / scratch-resident instantiations only serve as a cross-check of the wave-per-instance
     * family (ACADOS_AMD_WPI=0); by default a shape no register-resident instantiation covers goes there */
    if (sw.wpi.off())
        for (int q = 0; q < g_n_ksets_large; q++) consider(g_ksets_large[q]);
    if (forced.parent) lane = forced.parent->ks();
    /* wave-per-instance family (ipm_kernels_wpi.hpp): box-constrained QPs whose stage block is too large for
     * the one-instance-per-lane register mapping.  Dimensions are runtime values there: no padding to a
     * compiled shape.  ACADOS_AMD_WPI=0/1 overrides the size rule (tests). */
    const bool need_wpi = d.nct_max > 64;
    if (need_wpi) lane = nullptr; /* no one-instance-per-lane kernel may serve it */
    int wx = force_NX ? force_NX : mx, wu = force_NU ? force_NU : mu;
    const bool gen = mg > 0 || ms > 0;
    const bool ref = sw.wpi_v1.on() && !gen;
    /* sixteen lanes per instance: the smallest compiled shape that covers the dims (per-stage dims live inside
     * the padded shape); a sub-level created for a hand-over must match its parent's padded dims exactly */
    const bool soft_dims = mg == 0 && ms > 0; /* slacks on box rows only: the SOFT variants, if the structure allows */
    const W16Set *w16 = nullptr;
    if (!need_wpi && !ref && !sw.w16.off())
        for (const W16Set &ws : g_w16_sets)
        {
            bool fits = force_NX ? (ws.NX == wx && ws.NU == wu) : (ws.NX >= wx && ws.NU >= wu);
            if (!gen) fits = fits && ws.fact && ws.NG == 0;
            else if (soft_dims) fits = fits && ws.sfact && ws.NG == 0;                       /* slacks on box rows only */
            /* general rows (a small block with a compiled one-instance-per-lane general set -- the golden shared-slack
             * structure, nx = 4, nu = 1 -- keeps the dispatch it was measured with: gen_small below) */
            else fits = fits && ws.sfact && ws.NG >= mg && !sw.w16g.off() && !(lane && lane->NX + lane->NU <= 6);
            if (ws.NX + ws.NU > 16 && sw.w16r.off()) fits = false;
            /* two rows per lane: dims run PADDED inside the compiled shape, so its ~2.3x over the wave-per-instance
             * kernels (which take dims at run time) is gone once the padded block has more than twice the work:
             * the shape must cover at least 77 % of the compiled nu + nx */
            if (ws.NX + ws.NU > 16 && !force_NX && 13 * (wx + wu) < 10 * (ws.NX + ws.NU)) fits = false;
            if (fits && (!w16 || ws.NX + ws.NU < w16->NX + w16->NU)) w16 = &ws;
        }
    const bool has_w16 = w16 != nullptr;
    /* size rule: large stage blocks always; small ones while the batch is too small to fill the chip with 64
     * instances per wave (measured crossover on the C2 shape between 4,096 and 16,384 instances,
     * tools/family_crossover.py).  ACADOS_AMD_WPI_BATCH_MAX overrides the batch threshold. */
    /* state bounds after stage 0 (the mass-spring class, DimsSummary::xbox_dims): the one-instance-per-lane kernels of that class
     * run out of registers, the sixteen-lanes kernels win at every batch size measured (tools/xbox_rate.py) */
    /* nu + nx <= 6: the pipelined one-instance-per-lane kernels (ipm_kernels_box_small.hpp) take over much earlier
     * -- measured crossover on nx = 4, nu = 1 between 2,048 and 4,096 instances (N = 100; 4,096 ... 7,281 at N = 20),
     * with bounds on every state between 7,281 and 16,384; at 65,536 they are 2.7-2.9x (1.4x) ahead
     * (tools/small_shape_crossover.py) */
    const bool kb_small = !gen && lane && lane->NX + lane->NU <= 6;
    /* general rows / shared slacks on a small block with a compiled one-instance-per-lane set (the reference's golden
     * structure pend_idxs_rev_min_qp0: nx = 4, nu = 1, two general rows sharing one slack): 1,024 instances 3.45 ms
     * there against 2.65 ms on the wave-per-instance kernels, 8,192: 4.4 against 9.2 ms, 65,536: 8.4 against 74 ms */
    const bool gen_small = gen && lane && lane->NX + lane->NU <= 6;
    const int batch_max = sw.wpi_batch_max.set ? sw.wpi_batch_max.v
                        : !has_w16 ? (gen_small ? GQP_WPI_GEN_SMALL_MAX : GQP_WPI_BATCH_MAX)
                        : kb_small ? (d.xbox_dims ? GQP_W16_SMALL_XBOX_MAX : GQP_W16_SMALL_MAX)
                        /* general rows / slacks on the sixteen-lanes GEN kernels: the one-instance-per-lane alternative is the
                         * general set of a (much) larger padded shape with its blocks in scratch -- never */
                        : (d.xbox_dims || (gen && !soft_dims && !gen_small) ? INT_MAX : GQP_W16_BATCH_MAX);
    /* (a shape no compiled one-instance-per-lane set covers runs here whatever the override says) */
    const bool want = forced.wpi || need_wpi || !lane || (sw.wpi.set ? sw.wpi.v != 0 : (wx + wu >= GQP_WPI_MIN_N || n_batch <= batch_max));
    if (want && wx + wu <= 64 && wx >= 1 && mg <= 32 && ms <= 32)
    {
        if (w16) { wx = w16->NX; wu = w16->NU; }
        /* factor sweep: register-tile kernel for the tile count of this shape; rhs-only and forward sweeps on
         * the packed factor; GEN variants carry general constraints and slacks.  ACADOS_AMD_WPI_V1=1 selects
         * the plain LDS-resident reference kernels of the family (box-constrained QPs only), kept for
         * cross-checking. */
        static const kern_redo_t fact_box[8] = {gqp::kw_factor<1, false>, gqp::kw_factor<2, false>, gqp::kw_factor<3, false>,
                                                gqp::kw_factor<4, false>, gqp::kw_factor<5, false>, gqp::kw_factor<6, false>,
                                                gqp::kw_factor<7, false>, gqp::kw_factor<8, false>};
        static const kern_redo_t fact_gen[8] = {gqp::kw_factor<1, true>, gqp::kw_factor<2, true>, gqp::kw_factor<3, true>,
                                                gqp::kw_factor<4, true>, gqp::kw_factor<5, true>, gqp::kw_factor<6, true>,
                                                gqp::kw_factor<7, true>, gqp::kw_factor<8, true>};
        const int t8 = (wx + wu + 7) / 8 - 1;
        /* 17 <= n <= 32: blocked Cholesky + the O(n^3) parts on the FP64 matrix pipe (ipm_kernels_wpi_mfma.hpp).
         * Measured (tools/factor_variants.py, 4,096 instances): C4 class 3.97 vs 4.10 ms per factor launch, box class
         * nx=24 nu=6 2.40 vs 2.07 ms, condensed C3 shape 0.35 vs 0.33 ms -- the FP64 matrix pipe is slower than the
         * vector pipe on this chip (tools/mfma_f64_probe), so it serves the class it helps (general rows + slacks) by
         * default; ACADOS_AMD_WPI_MFMA=1 / 0 forces it on / off for every shape in range */
        const bool mfma = !ref && !w16 && wx + wu > 16 && wx + wu <= 32 && (sw.wpi_mfma.set ? sw.wpi_mfma.v != 0 : gen);
        kern_redo_t fact_ct = nullptr, rhs_ct = nullptr, faff_ct = nullptr, fcor_ct = nullptr;
        /* compile-time dims where they pay: the condensed C3 shape (nx=8 nu=15, box): factor sweep 0.328 -> 0.287 ms
         * per 4,096 launch.  Measured and NOT kept: nx=24 nu=3 general (4.09 -> 5.13 ms) and nx=24 nu=6 box (2.07 ->
         * 2.15 ms) -- full unrolling costs those shapes more in registers than the folded arithmetic saves
         * (tools/factor_variants.py).  ACADOS_AMD_WPI_CT=0 keeps the run-time-shaped instantiations */
        if (!ref && !w16 && !sw.wpi_ct.off())
        {
#define GQP_CT(GENV, X, U, T)                                                                                     \
    if (gen == GENV && wx == X && wu == U)                                                                        \
    {                                                                                                             \
        fact_ct = gqp::kw_factor<T, GENV, X, U>; rhs_ct = gqp::kw_backrhs<GENV, X, U>;                               \
        faff_ct = gqp::kw_fwd<false, GENV, X, U>; fcor_ct = gqp::kw_fwd<true, GENV, X, U>;                             \
    }
            GQP_CT(false, 8, 15, 3)
#undef GQP_CT
        }
        static const kern_redo_t fact_mf[2][3] = {{gqp::kw_factor_m<false, 0>, gqp::kw_factor_m<false, 1>, gqp::kw_factor_m<false, 2>},
                                                  {gqp::kw_factor_m<true, 0>, gqp::kw_factor_m<true, 1>, gqp::kw_factor_m<true, 2>}};
        const int pf = sw.wpi_mfma_pf.set ? std::max(0, std::min(2, sw.wpi_mfma_pf.v)) : 0; /* register prefetch did not pay (VGPR pressure) */
        const kern_redo_t fact = ref ? gqp::kw_backward<true> : mfma ? fact_mf[gen ? 1 : 0][pf] : fact_ct ? fact_ct : gen ? fact_gen[t8] : fact_box[t8];
        kern_redo_t rhs = ref ? gqp::kw_backward<false> : gen ? gqp::kw_backrhs<true> : gqp::kw_backrhs<false>;
        kern_redo_t faff = ref ? gqp::kw_forward<false> : gen ? gqp::kw_fwd<false, true> : gqp::kw_fwd<false, false>;
        kern_redo_t fcor = ref ? gqp::kw_forward<true> : gen ? gqp::kw_fwd<true, true> : gqp::kw_fwd<true, false>;
        if (rhs_ct) { rhs = rhs_ct; faff = faff_ct; fcor = fcor_ct; }

        const kern_opts_t init = gen ? gqp::kw_init<true> : gqp::kw_init<false>;
        const kern_plain_t fin = gen ? gqp::kw_finalize<true> : gqp::kw_finalize<false>;
        f.own_ks = KernelSet{wx, wu, mg, ms, init, fact, rhs, faff, fcor, fin,
                             {{fact, fact}, {rhs, rhs}, {faff, faff}, {fcor, fcor}}, fin};
        f.map = MAP_WPI;
        f.mfma = mfma;
        f.aos = 1;
        f.AW = need_wpi ? 2 : 1;
        const size_t con = gqp::wpi_con_doubles(wx + wu, mg, ms);
        f.lds.rhs = f.lds.whole = (ref ? gqp::wpi_lds_doubles(wx, wu) : gqp::wpi3_lds_doubles(wx, wu) + con) * sizeof(double);
        f.lds.fwd = (ref ? gqp::wpi_lds_doubles(wx, wu) : gqp::wpi3_lds_doubles(wx, wu, 1) + con) * sizeof(double);
        f.lds.fact = (ref ? gqp::wpi_lds_doubles(wx, wu) : (mfma ? gqp::wpim_lds_doubles(wx, wu) : gqp::wpi2_lds_doubles(wx, wu)) + con) * sizeof(double);
        /* small box-constrained stage blocks: four instances per wave, register rows + DPP row broadcasts */
        if (w16)
        {
            const W16Set &ws = *w16;
            f.wpi_ks = f.own_ks; /* what the batch falls back to if the slack structure is not one-slack-per-box-row */
            f.wpi_lds = f.lds;
            /* ACADOS_AMD_W16T=0: the factor sweep of the two-rows family on register rows (ky_factor); _W16T_GEN=0: of the GEN
             * instantiations alone */
            const bool tiles = ws.tfact && !sw.w16t.off() && !(gen && sw.w16t_gen.off());
            const kern_redo_t kf = tiles ? ws.tfact : (gen ? ws.sfact : ws.fact), kr = gen ? ws.srhs : ws.rhs;
            const kern_redo_t ka = gen ? ws.sfaff : ws.faff, kc = gen ? ws.sfcor : ws.fcor;
            f.own_ks.back_fact = kf; f.own_ks.back_rhs = kr; f.own_ks.fwd_aff = ka; f.own_ks.fwd_corr = kc;
            for (int q = 0; q < 2; q++)
            {
                f.own_ks.box.fact[q] = kf; f.own_ks.box.rhs[q] = kr;
                f.own_ks.box.fwd_aff[q] = ka; f.own_ks.box.fwd_corr[q] = kc;
            }
            f.map = MAP_W16;
            f.soft = gen;
            f.ng = ws.NG;
            f.tiles = tiles;
            f.solve = gen ? ws.ssolve : ws.solve;
            f.lds.rhs = f.lds.fwd = ws.shmem; /* (init and finalize stay the wave-per-instance kernels: lds.whole) */
            f.lds.fact = tiles ? ws.tshmem : ws.shmem;
            if (sw.w16_lds_align.set && sw.w16_lds_align.v > 1) /* development: allocation rounded up / padded */
            {
                const size_t a = (size_t) sw.w16_lds_align.v;
                f.lds.rhs = f.lds.fwd = (f.lds.rhs + a - 1) / a * a;
                f.lds.fact = (f.lds.fact + a - 1) / a * a;
            }
        }
    }
    if (f.lane())
    {
        if (!lane)
        {
            char msg[160];
            snprintf(msg, sizeof(msg), "acados_amd: no kernel instantiation covers nx<=%d nu<=%d ng<=%d ns<=%d\n", mx, mu, mg, ms);
            out.refusal = msg;
            return out;
        }
        f.compiled = lane;
    }
    f.name = family_name(f, 1);
    out.ok = true;
    return out;
}

/* The second step, once the structure is known (finalize_structure): st as built there from idxb / idxs_rev / idxe, the slack
 * references and the equality flags themselves.  The SOFT sixteen-lanes family falls back to wave per instance where a slack is
 * shared; box-only fast path, box rows on states, the pipelined small-block kernels. */
void family_structure(Family &f, const std::vector<GqpStage> &st, const std::vector<std::vector<int>> &idxs_rev,
                      const std::vector<std::vector<int>> &idxe, const FamilySwitches &sw)
{
    const int NX = f.ks()->NX, NU = f.ks()->NU;
    if (f.w16() && f.soft)
    {
        /* the SOFT sixteen-lanes kernels eliminate a slack inside the lane that owns its row: every slack must belong
         * to exactly one box row that is not an equality-flagged one; anything else runs on the general
         * wave-per-instance kernels of the same padded dims */
        bool ok = true;
        for (size_t k = 0; k < st.size() && ok; k++)
        {
            const GqpStage &S = st[k];
            std::vector<int> refs(S.ns, 0);
            for (int r = 0; r < S.nb + (f.ng ? S.ng : 0); r++)
                if (S.srev[r] >= 0) refs[S.srev[r]]++;
            for (int q = 0; q < S.ns; q++) ok = ok && refs[q] == 1;
            if (!f.ng) ok = ok && S.ng == 0;
            else ok = ok && __builtin_popcountll(S.bmask & ~S.emask) + S.ng <= 16; /* GEN: one inequality row per lane */
            for (size_t e = 0; e < idxe[k].size(); e++) ok = ok && idxs_rev[k][idxe[k][e]] < 0;
        }
        if (!ok)
        {
            f.map = MAP_WPI;
            f.own_ks = f.wpi_ks;
            f.lds = f.wpi_lds;
            f.solve = nullptr;
            f.soft = false;
            f.tiles = 0;
        }
    }
    int o_g = 0, o_s = 0;
    f.xbox = 0;
    for (const GqpStage &S : st)
    {
        o_g += S.ng; o_s += S.ns;
        if (((S.bmask & ~S.emask) >> NU) != 0) f.xbox = 1;
    }
    /* ACADOS_AMD_GENERAL_KERNELS (any value): the general sweeps for a box-only batch (cross-check) */
    f.use_box = !f.lane() || (o_g == 0 && o_s == 0 && !sw.general_kernels.set);
    /* nu + nx <= 6: the pipelined kernels of ipm_kernels_box_small.hpp ("1tpi-pipe"); ACADOS_AMD_KB_SMALL=0 keeps the
     * phase-ordered ones of ipm_kernels_box.hpp (cross-check) */
    if (f.use_box && f.lane()) f.kb_plain = sw.kb_small.off() || NX + NU > 6;
    f.name = family_name(f, 1);
}

/* dynamic LDS above the default limit: raise it for the four sweep kernels of the batch's own set */
static void wpi_lds_attributes(ocp_qp_gpu_batch *b)
{
    const Family &f = b->fam;
    /* (a sixteen-lanes family: the largest of ITS sizes and of the wave-per-instance init / finalize -- the parent of this function
     * took the two wave-per-instance sweep sizes there; neither reaches 64 KB at nu + nx <= 32, so no call differs) */
    const size_t most = std::max(std::max(f.lds.fact, f.lds.rhs), std::max(f.lds.fwd, f.lds.whole));
    if (most <= 64 * 1024) return;
    const void *fns[] = {(const void *) f.own_ks.back_fact, (const void *) f.own_ks.back_rhs,
                         (const void *) f.own_ks.fwd_aff, (const void *) f.own_ks.fwd_corr};
    for (const void *fn : fns)
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) most));
}

/* the family and name of a batch for its ric_alg (see ocp_qp_gpu_batch::ric_alg) */
static void ric_configure(ocp_qp_gpu_batch *b)
{
    if (b->ric_alg == 1)
    {
        if (!b->ric1_saved) return;
        b->fam = b->ric1_fam;
        b->ric1_saved = false;
    }
    else
    {
        if (!b->ric1_saved) { b->ric1_fam = b->fam; b->ric1_saved = true; }
        if (!b->fam.lane()) b->fam = ric0_family(b->fam);
        b->fam.name = family_name(b->fam, 0);
    }
    if (!b->fam.lane() && b->finalized) wpi_lds_attributes(b);
}

void finalize_structure(ocp_qp_gpu_batch *b)
{
    if (b->finalized) return;
    /* ric_alg 0 set before the structure: the checks below decide for the set ric_alg 1 runs (the sixteen-lanes soft fallback,
     * the LDS limits); the classical family goes back on afterwards */
    const bool ric0 = b->ric_alg == 0 && b->ric1_saved;
    if (ric0) { b->ric_alg = 1; ric_configure(b); }
    const int N = b->N, NX = b->fam.ks()->NX, NU = b->fam.ks()->NU;
    const int n = NX + NU, NP = n * (n + 1) / 2;
    b->st.assign(N + 1, GqpStage());
    b->perm.assign(N + 1, std::vector<int>());
    int o_ct = 0, o_s = 0, o_g = 0;
    for (int k = 0; k <= N; k++)
    {
        GqpStage &S = b->st[k];
        memset(&S, 0, sizeof(S));
        S.nb = b->nb[k]; S.ng = b->ng[k]; S.ns = b->ns[k];
        if (S.ns > 0) b->has_slack = true;
        S.o_ct = o_ct; S.o_s = o_s; S.o_g = o_g; S.has_dyn = k < N;
        const int nbg = S.nb + S.ng, nct = 2 * nbg + 2 * S.ns;
        if (nct > 64 * b->fam.AW || nbg > GQP_MAX_ROWS)
        {
            fprintf(stderr, "acados_amd: stage %d has %d inequality sides (> %d): unsupported\n", k, nct, 64 * b->fam.AW);
            exit(1); /* not reachable through ocp_qp_gpu_batch_create, which refuses such dims */
        }
        /* sort box rows by variable */
        std::vector<int> order(S.nb);
        for (int r = 0; r < S.nb; r++) order[r] = r;
        std::sort(order.begin(), order.end(), [&](int a, int c) { return b->idxb[k][a] < b->idxb[k][c]; });
        b->perm[k].assign(S.nb, 0);
        for (int sp = 0; sp < S.nb; sp++)
        {
            const int ob = order[sp];
            b->perm[k][ob] = sp;
            const int iv = b->idxb[k][ob];
            if (iv < 0 || iv >= b->nu[k] + b->nx[k]) { fprintf(stderr, "acados_amd: idxb out of range at stage %d\n", k); exit(1); }
            const int pv = padded_var(b, k, iv);
            if ((S.bmask >> pv) & 1) { fprintf(stderr, "acados_amd: duplicate idxb entry at stage %d: unsupported\n", k); exit(1); }
            S.bmask |= (uint64_t) 1 << pv;
        }
        for (int r = 0; r < GQP_MAX_ROWS; r++) S.srev[r] = -1;
        for (int r = 0; r < nbg; r++)
        {
            const int sj = b->idxs_rev[k][r];
            if (sj >= S.ns) { fprintf(stderr, "acados_amd: idxs_rev out of range at stage %d\n", k); exit(1); }
            const int row = r < S.nb ? b->perm[k][r] : r;
            S.srev[row] = (int8_t) sj;
        }
        for (size_t e = 0; e < b->idxe[k].size(); e++)
        {
            const int ob = b->idxe[k][e];
            if (ob < 0 || ob >= S.nb) { fprintf(stderr, "acados_amd: idxe out of range at stage %d\n", k); exit(1); }
            S.emask |= (uint64_t) 1 << padded_var(b, k, b->idxb[k][ob]);
        }
        o_ct += nct; o_s += 2 * S.ns; o_g += S.ng;
    }
    b->nct_tot = o_ct; b->ns2_tot = o_s; b->ng_tot = o_g;
    family_structure(b->fam, b->st, b->idxs_rev, b->idxe, family_switches());
    if (!b->fam.lane()) wpi_lds_attributes(b); /* more than the default dynamic LDS limit: raised for the four sweep kernels */
    b->d_st = dalloc<GqpStage>(b, N + 1);
    HIPCHK(hipMemcpy(b->d_st, b->st.data(), sizeof(GqpStage) * (N + 1), hipMemcpyHostToDevice));

    GqpDev &D = b->D;
    const size_t Bp = b->Bp;
    D.B = b->B; D.Bp = b->Bp; D.N = N; D.NX = NX; D.NU = NU; D.NG = b->fam.ks()->NG; D.NS = b->fam.ks()->NS;
    D.st = (GqpStagePtr) (uintptr_t) b->d_st;
    const size_t RP = 16; /* spare row elements (clamped dummy row index) */
    D.BAt = garr<double>(b, (size_t) ((N + 1) * n * NX));
    D.bvec = garr<double>(b, (size_t) ((N + 1) * NX));
    D.RSQ = garr<double>(b, (size_t) ((N + 1) * NP));
    D.rq = garr<double>(b, (size_t) ((N + 1) * n));
    D.dvec = garr<double>(b, (size_t) ((o_ct + RP)));
    D.AW = b->fam.AW;
    D.amask = garr<uint64_t>(b, (size_t) ((N + 1) * b->fam.AW));
    /* (+ n spare elements: the sixteen-lanes GEN kernels prefetch the stage's rows of [D C] branch-free, a stage WITHOUT general rows
     * reads element 0 of its (empty) block -- for such stages at the end of the horizon that is the element behind the last row:
     * found by the structure fuzz of round 6, seed 9193, a fault only where the array ended on a page boundary) */
    D.DCt = garr<double>(b, (size_t) (o_g * n + n));
    /* (at least one (Z, z) pair: the branch-free row functions of the sixteen-lanes GEN kernels read the pair of slack 0 through
     * clamped addresses also in a batch without slacks -- with one element per instance the z of the LAST instance lay behind the
     * allocation: found by the structure fuzz of round 5, a fault only where the array ended on a page boundary) */
    D.Zz = garr<double>(b, (size_t) (o_s > 0 ? o_s * 2 : 2));
    D.ux = garr<double>(b, (size_t) ((N + 2) * n));
    D.sv = garr<double>(b, (size_t) (o_s));
    D.pi = garr<double>(b, (size_t) ((N + 2) * NX));
    D.lam = garr<double>(b, (size_t) ((o_ct + RP)));
    D.t = garr<double>(b, (size_t) ((o_ct + RP)));
    D.rg = garr<double>(b, (size_t) ((N + 1) * n));
    D.rgs = garr<double>(b, (size_t) (o_s));
    D.rb = garr<double>(b, (size_t) ((N + 1) * NX));
    D.rd = garr<double>(b, (size_t) ((o_ct + RP)));
    D.rm = garr<double>(b, (size_t) ((o_ct + RP)));
    D.dux = garr<double>(b, (size_t) ((N + 2) * n));
    D.dsv = garr<double>(b, (size_t) (o_s));
    D.dpi = garr<double>(b, (size_t) ((N + 2) * NX));
    D.dlam = garr<double>(b, (size_t) ((o_ct + RP)));
    D.dt = garr<double>(b, (size_t) ((o_ct + RP)));
    D.pcorr = garr<double>(b, (size_t) ((o_ct + RP)));
    D.sD = garr<double>(b, (size_t) (o_s));
    D.sR = garr<double>(b, (size_t) (o_s));
    D.Lf = garr<double>(b, (size_t) ((N + 1) * NP));
    D.lf = garr<double>(b, (size_t) ((N + 1) * n));
    D.res = dalloc<double>(b, 4 * Bp);
    D.mu = dalloc<double>(b, Bp); D.smu = dalloc<double>(b, Bp);
    D.alpha = dalloc<double>(b, Bp); D.obj = dalloc<double>(b, Bp);
    D.apend = dalloc<double>(b, Bp);
    D.iter = dalloc<int>(b, Bp); D.status = dalloc<int>(b, Bp);
    D.n_active = dalloc<int>(b, 1);
    D.tile_inv = dalloc<int>(b, (size_t) Bp / 64);
    b->held.d_kept = dalloc<int>(b, (size_t) Bp / 64);
    b->held.d_hess_cnt = dalloc<int>(b, (size_t) Bp / 64);
    b->stat_inst = b->B < 64 ? b->B : 64;
    b->stat_rows = 0;
    D.stat = nullptr; D.stat_inst = 0; D.stat_rows = 0;
    D.perm = nullptr; D.n_perm = 0;

    /* neutral padding: unit Hessian diagonal on padded variables */
    const int grid = (b->B + 63) / 64;
    for (int k = 0; k <= N; k++)
    {
        for (int j = 0; j < n; j++)
        {
            const bool real = j < NU ? j < b->nu[k] : (j - NU) < b->nx[k];
            if (!real)
                hipLaunchKernelGGL(gqp::k_fill_strided, dim3(grid), dim3(64), 0, b->stream, D.RSQ, 1.0, b->B,
                                   k * NP + PK(j, j));
        }
        /* activity: every existing row side, minus equality-flagged rows */
        const GqpStage &S = b->st[k];
        const int nbg = S.nb + S.ng, nct = 2 * nbg + 2 * S.ns;
        uint64_t m[2] = {0, 0};
        for (int e = 0; e < nct; e++) m[e >> 6] |= (uint64_t) 1 << (e & 63);
        for (size_t e = 0; e < b->idxe[k].size(); e++)
        {
            const int sp = b->perm[k][b->idxe[k][e]];
            m[sp >> 6] &= ~((uint64_t) 1 << (sp & 63));
            m[(nbg + sp) >> 6] &= ~((uint64_t) 1 << ((nbg + sp) & 63));
        }
        for (int w = 0; w < b->fam.AW; w++)
            hipLaunchKernelGGL(gqp::k_fill_u64, dim3(grid), dim3(64), 0, b->stream, D.amask, m[w], b->Bp, k * b->fam.AW + w);
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    b->finalized = true;
    if (ric0) { b->ric_alg = 0; ric_configure(b); }
}

void ensure_stat(ocp_qp_gpu_batch *b)
{
    const int rows = b->O.iter_max + 2;
    if (b->stat_rows >= rows) return;
    /* (re)allocate the statistics table for the first stat_inst instances */
    b->D.stat = dalloc<double>(b, (size_t) rows * GQP_STAT_COLS * b->stat_inst);
    b->stat_rows = rows;
    b->D.stat_rows = rows;
    b->D.stat_inst = b->stat_inst;
}

/* ---- the fields of the C ABI: one table (k_fields) behind _set, _get, _sens_set, the blob maps and the data gradient ---- */

/* Every per-instance array a device table (gqp::GArrTable) can hold.  A table is a list of these names in the order its kernels
 * count the slots in; slot_of turns a name into the slot of a table, arr_of into the array of a batch */
enum Arr
{
    ARR_NONE = -1,
    ARR_BAt, ARR_bvec, ARR_RSQ, ARR_rq, ARR_dvec, ARR_DCt, ARR_Zz, ARR_ux, ARR_sv, ARR_pi, ARR_lam, ARR_t, /* data and iterate */
    ARR_dux, ARR_dsv, ARR_dpi, ARR_dlam, ARR_dt, /* directions of a seed pass, in the order of ux .. t (direction_of) */
    ARR_rg, ARR_rgs, ARR_rb, ARR_rd,             /* residuals: where the seeds go */
    ARR_Lf, ARR_lf,                              /* factor of the last factorisation */
    ARR_DEV_END,                                 /* ... so far members of GqpDev; the batch's own: */
    ARR_sfix = ARR_DEV_END, ARR_cot, ARR_res_g, ARR_res_gs, ARR_res_b, ARR_res_d, ARR_res_m
};
typedef GArr GqpDev::*GqpArrMember;

GArr arr_of(const ocp_qp_gpu_batch *b, Arr a)
{
    static const GqpArrMember dev[ARR_DEV_END] = {&GqpDev::BAt, &GqpDev::bvec, &GqpDev::RSQ, &GqpDev::rq, &GqpDev::dvec, &GqpDev::DCt, &GqpDev::Zz,
                                                  &GqpDev::ux, &GqpDev::sv, &GqpDev::pi, &GqpDev::lam, &GqpDev::t, &GqpDev::dux, &GqpDev::dsv,
                                                  &GqpDev::dpi, &GqpDev::dlam, &GqpDev::dt, &GqpDev::rg, &GqpDev::rgs, &GqpDev::rb, &GqpDev::rd,
                                                  &GqpDev::Lf, &GqpDev::lf};
    if (a >= 0 && a < ARR_DEV_END) return b->D.*dev[a];
    switch (a)
    {
    case ARR_sfix: return b->sfix;
    case ARR_cot: return b->grad.cot;
    case ARR_res_g: return b->R.g;
    case ARR_res_gs: return b->R.gs;
    case ARR_res_b: return b->R.b;
    case ARR_res_d: return b->R.d;
    case ARR_res_m: return b->R.m;
    default: return GArr{nullptr, 0, 0};
    }
}

/* the direction array behind sens_<field>: an iterate array has one */
Arr direction_of(Arr a) { return a >= ARR_ux && a <= ARR_t ? Arr(ARR_dux + (a - ARR_ux)) : ARR_NONE; }

/* the three device tables.  State: the blob scatter / gather kernels (every kind but the seeds).  Seeds: k_bulk_scatter_seed (slot 4
 * is where it writes the derivative of a fixed variable).  Gradient: k_data_grad (a solution array and its direction are 5 apart) */
const Arr k_state_arrays[] = {ARR_BAt, ARR_bvec, ARR_RSQ, ARR_rq, ARR_dvec, ARR_DCt, ARR_Zz, ARR_ux, ARR_sv, ARR_pi, ARR_lam, ARR_t};
const Arr k_seed_arrays[] = {ARR_rg, ARR_rgs, ARR_rb, ARR_rd, ARR_sfix};
const Arr k_grad_arrays[] = {ARR_ux, ARR_sv, ARR_pi, ARR_lam, ARR_t, ARR_dux, ARR_dsv, ARR_dpi, ARR_dlam, ARR_dt, ARR_RSQ, ARR_BAt, ARR_DCt, ARR_cot};

template <size_t n>
int slot_of(const Arr (&table)[n], Arr a)
{
    for (size_t q = 0; q < n; q++) if (table[q] == a) return (int) q;
    return -1;
}

template <size_t n>
void table_fill(const ocp_qp_gpu_batch *b, gqp::GArrTable &T, const Arr (&table)[n])
{
    for (size_t q = 0; q < 16; q++) T.a[q] = q < n ? arr_of(b, table[q]) : GArr{nullptr, 0, 0};
}

/* One row per field name.  `arr` and `rule` say where element e of the field lives (rule: the element of arr per entry, in units
 * of Bp doubles, -1 for none; a mask's bit in the activity words of its stage); cls / up / p are the rule's parameters: the
 * variables (u, x) or the rows (u box, x box, general, slack) the field ranges over, the upper side, a position.  `seed` / `sign`:
 * the residual array seed_<name> goes to and the sign it is stored with there (lower bounds negated; the slack lower bounds
 * lls, lus are both lower bounds).  `grad`: what the data gradient of an entry is (grad_build), ga / gb the output-blob fields of
 * its factors, gc its coefficient */
enum Cls { C_NONE, C_U, C_X, C_BU, C_BX, C_G, C_S };
enum
{
    F_DYN = 1,   /* lives at the stages 0 .. N-1 only */
    F_SYM = 2,   /* the packed lower triangle holds the matrix: a READ mirrors it */
    F_MASK = 4,  /* activity bits, not doubles */
    F_VALUE = 8, /* an equality-flagged row's entry is also the value of its variable (second map, into ux / sfix) */
    F_RES = 16   /* residual of the last _res_compute: read only */
};
enum GradKind { G_NONE, G_VEC, G_PROD, G_DIAG, G_GEN, G_CT };
struct FieldCtx;
struct FieldRow
{
    const char *name;
    Arr arr;
    void (*rule)(const FieldCtx &, const FieldRow &, std::vector<int> &);
    Cls cls = C_NONE;
    int up = 0, p = 0;
    unsigned flags = 0;
    Arr seed = ARR_NONE;
    int sign = 1;
    GradKind grad = G_NONE;
    const char *ga = nullptr, *gb = nullptr;
    double gc = 1.0;
};

/* what the rules see of one stage */
struct FieldCtx
{
    const ocp_qp_gpu_batch *b;
    const int k;
    const GqpStage &S;
    const int NX, NU, n, NP, nx, nu, nx1, nbu, nbx, ng, ns, nbg;
    FieldCtx(const ocp_qp_gpu_batch *b_, int k_)
        : b(b_), k(k_), S(b_->st[k_]), NX(b_->fam.ks()->NX), NU(b_->fam.ks()->NU), n(NX + NU), NP(n * (n + 1) / 2), nx(b_->nx[k_]), nu(b_->nu[k_]),
          nx1(k_ < b_->N ? b_->nx[k_ + 1] : 0), nbu(b_->nbu[k_]), nbx(b_->nbx[k_]), ng(S.ng), ns(S.ns), nbg(S.nb + S.ng) {}
    /* the variables of a class: how many, and where they start in the padded [u(NU); x(NX)] */
    int nvar(Cls c) const { return c == C_X ? nx : nu; }
    int voff(Cls c) const { return c == C_X ? NU : 0; }
    int pv(int iv) const { return padded_var(b, k, iv); }
    /* inequality sides, counted as lam / t list them: lower then upper side of the box rows (the caller's order) and the general
     * rows, then the lower bounds of sl and of su.  ct_row: the row of entry e of a bound field among box + general rows; ct_pos:
     * its side; ct_dev: where a side lives in dvec / lam / t / the activity bits (box rows sorted there) */
    int ct_count(Cls c) const { return c == C_BU ? nbu : c == C_BX ? nbx : c == C_G ? ng : ns; }
    int ct_row(const FieldRow &r, int e) const { return (r.cls == C_BU ? 0 : r.cls == C_BX ? nbu : S.nb) + e; }
    int ct_pos(const FieldRow &r, int e) const { return r.cls == C_S ? 2 * nbg + r.up * ns + e : r.up * nbg + ct_row(r, e); }
    int ct_dev(int pos) const
    {
        if (pos >= 2 * nbg) return pos;
        const int row = pos % nbg;
        return pos - row + (row < S.nb ? b->perm[k][row] : row);
    }
    bool eq(int row) const { return row < S.nb && std::find(b->idxe[k].begin(), b->idxe[k].end(), row) != b->idxe[k].end(); }
    bool ct_eq(const FieldRow &r, int e) const { return r.cls != C_S && eq(ct_row(r, e)); }
};

void rule_dyn_mat(const FieldCtx &c, const FieldRow &r, std::vector<int> &m) /* A, B: columns of [B A]' */
{
    for (int j = 0; j < c.nvar(r.cls); j++) for (int i = 0; i < c.nx1; i++) m.push_back((c.k * c.n + c.voff(r.cls) + j) * c.NX + i);
}
void rule_dyn_vec(const FieldCtx &c, const FieldRow &r, std::vector<int> &m) /* b; acados pi[k] = multiplier of the dynamics producing x_{k+1}: slot k+1 */
{
    for (int i = 0; i < c.nx1; i++) m.push_back((c.k + r.p) * c.NX + i);
}
void rule_hess(const FieldCtx &c, const FieldRow &r, std::vector<int> &m) /* Q, R */
{
    const int d = c.nvar(r.cls), o = c.voff(r.cls);
    for (int j = 0; j < d; j++) for (int i = 0; i < d; i++) m.push_back(i >= j ? c.k * c.NP + PK(o + i, o + j) : -1);
}
void rule_cross(const FieldCtx &c, const FieldRow &, std::vector<int> &m) /* S is nu x nx: u'Sx */
{
    for (int jx = 0; jx < c.nx; jx++) for (int iu = 0; iu < c.nu; iu++) m.push_back(c.k * c.NP + PK(c.NU + jx, iu));
}
void rule_var(const FieldCtx &c, const FieldRow &r, std::vector<int> &m) /* q r x u */
{
    for (int i = 0; i < c.nvar(r.cls); i++) m.push_back(c.k * c.n + c.voff(r.cls) + i);
}
void rule_gen_mat(const FieldCtx &c, const FieldRow &r, std::vector<int> &m) /* C, D: rows of [D C] */
{
    for (int j = 0; j < c.nvar(r.cls); j++) for (int g = 0; g < c.ng; g++) m.push_back((c.S.o_g + g) * c.n + c.voff(r.cls) + j);
}
void rule_penalty(const FieldCtx &c, const FieldRow &r, std::vector<int> &m) /* (Z, z) pairs */
{
    for (int j = 0; j < c.ns; j++) m.push_back((c.S.o_s + r.up * c.ns + j) * 2 + r.p);
}
void rule_slack(const FieldCtx &c, const FieldRow &r, std::vector<int> &m) /* sl su, and the seeds of zl zu in rgs */
{
    for (int j = 0; j < c.ns; j++) m.push_back(c.S.o_s + r.up * c.ns + j);
}
void rule_slack_both(const FieldCtx &c, const FieldRow &, std::vector<int> &m) /* [sl; su] */
{
    for (int j = 0; j < 2 * c.ns; j++) m.push_back(c.S.o_s + j);
}
void rule_ct(const FieldCtx &c, const FieldRow &r, std::vector<int> &m) /* a bound field, or its mask (equality-flagged rows: no bit) */
{
    for (int e = 0; e < c.ct_count(r.cls); e++)
    {
        const int d = c.ct_dev(c.ct_pos(r, e));
        m.push_back(r.flags & F_MASK ? (c.ct_eq(r, e) ? -1 : d) : c.S.o_ct + d);
    }
}
void rule_ct_all(const FieldCtx &c, const FieldRow &, std::vector<int> &m) /* lam, t */
{
    for (int pos = 0; pos < 2 * c.nbg + 2 * c.ns; pos++) m.push_back(c.S.o_ct + c.ct_dev(pos));
}
/* Cholesky factor of the stage matrix of the last factorisation, variables [u;x] of this stage (padding removed), nv x nv
 * column-major, lower triangle (upper = 0).
 * ric_alg 0 (classical layout, get_int "ric_alg"), stages k >= 1: columns 0..nu-1 as above ([Lu; Lxu], the factor of
 * R~ + B'PB and its coupling rows), the trailing x-block is the lower triangle of P_k itself; ric_l = [lu; p_k].
 * Stage 0 is the full factor in both layouts. */
void rule_fact_mat(const FieldCtx &c, const FieldRow &, std::vector<int> &m)
{
    const int nv = c.nu + c.nx;
    for (int j = 0; j < nv; j++) for (int i = 0; i < nv; i++) m.push_back(i >= j ? c.k * c.NP + PK(c.pv(i), c.pv(j)) : -1);
}
void rule_fact_vec(const FieldCtx &c, const FieldRow &, std::vector<int> &m) /* [u; x] of the stage */
{
    for (int i = 0; i < c.nu + c.nx; i++) m.push_back(c.k * c.n + c.pv(i));
}

/* a bound field and its mask */
#define GQP_CT_ROWS(name, cls, up, sign, flags) \
    {name, ARR_dvec, rule_ct, cls, up, 0, flags, ARR_rd, sign, G_CT}, {name "_mask", ARR_NONE, rule_ct, cls, up, 0, F_MASK}
const FieldRow k_fields[] = {
    /* name, array, rule, class, upper, p, flags, seed array, seed sign, gradient kind, its factors, its coefficient */
    {"A", ARR_BAt, rule_dyn_mat, C_X, 0, 0, F_DYN, ARR_NONE, 1, G_PROD, "pi", "x"},
    {"B", ARR_BAt, rule_dyn_mat, C_U, 0, 0, F_DYN, ARR_NONE, 1, G_PROD, "pi", "u"},
    {"b", ARR_bvec, rule_dyn_vec, C_NONE, 0, 0, F_DYN, ARR_rb, 1, G_VEC, "pi"},
    {"Q", ARR_RSQ, rule_hess, C_X, 0, 0, F_SYM, ARR_NONE, 1, G_PROD, "x", "x", 0.5},
    {"R", ARR_RSQ, rule_hess, C_U, 0, 0, F_SYM, ARR_NONE, 1, G_PROD, "u", "u", 0.5},
    {"S", ARR_RSQ, rule_cross, C_NONE, 0, 0, 0, ARR_NONE, 1, G_PROD, "u", "x"},
    {"q", ARR_rq, rule_var, C_X, 0, 0, 0, ARR_rg, 1, G_VEC, "x"},
    {"r", ARR_rq, rule_var, C_U, 0, 0, 0, ARR_rg, 1, G_VEC, "u"},
    GQP_CT_ROWS("lbu", C_BU, 0, -1, 0),
    GQP_CT_ROWS("ubu", C_BU, 1, 1, 0),
    GQP_CT_ROWS("lbx", C_BX, 0, -1, F_VALUE),
    GQP_CT_ROWS("ubx", C_BX, 1, 1, 0),
    GQP_CT_ROWS("lg", C_G, 0, -1, 0),
    GQP_CT_ROWS("ug", C_G, 1, 1, 0),
    GQP_CT_ROWS("lls", C_S, 0, -1, 0),
    GQP_CT_ROWS("lus", C_S, 1, -1, 0), /* su >= lus is a LOWER bound of the slack, like lls */
    {"C", ARR_DCt, rule_gen_mat, C_X, 0, 0, 0, ARR_NONE, 1, G_GEN, nullptr, "x"},
    {"D", ARR_DCt, rule_gen_mat, C_U, 0, 0, 0, ARR_NONE, 1, G_GEN, nullptr, "u"},
    {"Zl", ARR_Zz, rule_penalty, C_NONE, 0, 0, 0, ARR_NONE, 1, G_DIAG, "sl", nullptr, 0.5},
    {"Zu", ARR_Zz, rule_penalty, C_NONE, 1, 0, 0, ARR_NONE, 1, G_DIAG, "su", nullptr, 0.5},
    /* (the seed of zl / zu is the gradient of the slack penalty: the slack part of the stationarity residual, indexed like sl / su) */
    {"zl", ARR_Zz, rule_penalty, C_NONE, 0, 1, 0, ARR_rgs, 1, G_VEC, "sl"},
    {"zu", ARR_Zz, rule_penalty, C_NONE, 1, 1, 0, ARR_rgs, 1, G_VEC, "su"},
    {"u", ARR_ux, rule_var, C_U},
    {"x", ARR_ux, rule_var, C_X},
    {"sl", ARR_sv, rule_slack, C_NONE, 0},
    {"su", ARR_sv, rule_slack, C_NONE, 1},
    {"pi", ARR_pi, rule_dyn_vec, C_NONE, 0, 1, F_DYN},
    {"lam", ARR_lam, rule_ct_all},
    {"t", ARR_t, rule_ct_all},
    {"ric_L", ARR_Lf, rule_fact_mat},
    {"ric_l", ARR_lf, rule_fact_vec},
    /* residual vectors of the last ocp_qp_gpu_batch_res_compute -- the element rule of the quantity each belongs to: res_g [u; x],
     * res_gs [sl; su], res_b like pi (but in slot k), res_d and res_m like lam */
    {"res_g", ARR_res_g, rule_fact_vec, C_NONE, 0, 0, F_RES},
    {"res_gs", ARR_res_gs, rule_slack_both, C_NONE, 0, 0, F_RES},
    {"res_b", ARR_res_b, rule_dyn_vec, C_NONE, 0, 0, F_DYN | F_RES},
    {"res_d", ARR_res_d, rule_ct_all, C_NONE, 0, 0, F_RES},
    {"res_m", ARR_res_m, rule_ct_all, C_NONE, 0, 0, F_RES},
};

/* the one place a field name is compared */
const FieldRow *field_row(const char *name)
{
    for (const FieldRow &r : k_fields) if (!strcmp(name, r.name)) return &r;
    return nullptr;
}

/* a batch's answer for (field, stage): the data itself, the seed seed_<name> or the direction sens_<name> */
enum FieldUse { USE_DATA, USE_SEED, USE_SENS };
struct FieldRef
{
    const FieldRow *row = nullptr;
    int k = 0, len = -1;
    Arr arr = ARR_NONE, arr2 = ARR_NONE;
    std::vector<int> map, map2; /* element of arr (arr2) per entry, -1: none; bit positions for a mask */
    bool mask() const { return row->flags & F_MASK; }
};

/* Returns the field length; -1: no such field, not at this stage, or not in this use */
int field_resolve(const ocp_qp_gpu_batch *b, const FieldRow *r, int k, FieldUse use, FieldRef &s)
{
    s = FieldRef();
    s.row = r; s.k = k;
    if (!r || k < 0 || k > b->N || ((r->flags & F_DYN) && k == b->N)) return -1;
    s.arr = use == USE_SEED ? r->seed : use == USE_SENS ? direction_of(r->arr) : r->arr;
    if (s.arr == ARR_NONE && !(use == USE_DATA && s.mask())) return -1;
    const FieldCtx c(b, k);
    (s.arr == ARR_rgs ? rule_slack : r->rule)(c, *r, s.map);
    if (r->flags & F_VALUE)
    {
        /* equality-flagged x bounds: the bound value is the value of the variable, its seed the derivative of the variable */
        s.arr2 = use == USE_SEED ? ARR_sfix : ARR_ux;
        s.map2.assign(c.nbx, -1);
        for (int ob : b->idxe[k])
            if (ob >= c.nbu && ob < c.nbu + c.nbx) s.map2[ob - c.nbu] = k * c.n + c.pv(b->idxb[k][ob]);
    }
    return s.len = (int) s.map.size();
}

/* a map whose lower triangle (column-major, dim x dim) is filled: the upper one refers to the mirrored element */
void mirror_lower(std::vector<int> &map, int dim)
{
    for (int c = 0; c < dim; c++) for (int r = 0; r < c; r++) map[c * dim + r] = map[r * dim + c];
}

int *upload_map(ocp_qp_gpu_batch *b, const std::vector<int> &map)
{
    if ((int) map.size() > b->map_cap)
    {
        b->map_cap = (int) map.size() * 2 + 64;
        b->d_map = dalloc<int>(b, b->map_cap);
    }
    /* the previous launch using d_map must be done before it is overwritten */
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipMemcpy(b->d_map, map.data(), sizeof(int) * map.size(), hipMemcpyHostToDevice));
    return b->d_map;
}

const double *stage_in(ocp_qp_gpu_batch *b, const double *data, size_t cnt, int is_device)
{
    if (is_device) return data;
    if (cnt > b->stage_cap)
    {
        b->stage_cap = cnt * 2;
        b->d_stage = dalloc<double>(b, b->stage_cap);
    }
    HIPCHK(hipMemcpyAsync(b->d_stage, data, sizeof(double) * cnt, hipMemcpyHostToDevice, b->stream));
    return b->d_stage;
}

/* the other direction: where the launches write `cnt` doubles for the caller -- its own pointer where that is a device pointer,
 * else the staging area; behind the launches stage_out_done copies to the caller, if there is a copy, and waits for the stream */
double *stage_out(ocp_qp_gpu_batch *b, double *data, size_t cnt, int is_device)
{
    if (is_device) return data;
    if (cnt > b->stage_cap)
    {
        b->stage_cap = cnt * 2;
        b->d_stage = dalloc<double>(b, b->stage_cap);
    }
    return b->d_stage;
}

void stage_out_done(ocp_qp_gpu_batch *b, double *data, size_t cnt, int is_device)
{
    if (!is_device) HIPCHK(hipMemcpyAsync(data, b->d_stage, sizeof(double) * cnt, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
}

/* a table built on the host as a device array that lives as long as the batch (blocking copy; an empty table is one zeroed element) */
template <class T>
T *upload(ocp_qp_gpu_batch *b, const T *h, size_t cnt)
{
    T *d = dalloc<T>(b, cnt);
    if (cnt) HIPCHK(hipMemcpy(d, h, sizeof(T) * cnt, hipMemcpyHostToDevice));
    return d;
}

template <class T>
T *upload(ocp_qp_gpu_batch *b, const std::vector<T> &h) { return upload(b, h.data(), h.size()); }

/* what the launches of `run` and the copies in front of them take on the stream since the event `started` was recorded (the
 * first chunk of a staged round), waited for, added to time_pack */
template <class F>
void pack_timed_since(ocp_qp_gpu_batch *b, hipEvent_t started, F run)
{
    run();
    HIPCHK(hipEventRecord(b->ev1, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, started, b->ev1));
    b->time_pack += ms * 1e-3;
}

/* ... from here.  ev0 / ev1 are free outside a solve */
template <class F>
void pack_timed(ocp_qp_gpu_batch *b, F run)
{
    HIPCHK(hipEventRecord(b->ev0, b->stream));
    pack_timed_since(b, b->ev0, run);
}

} // namespace

/* one array of a level <-> the same array of its sub-level (dir 0: gather the listed instances, 1: scatter back);
 * levels of different layouts exchange through the LDS-transposing kernel */
template <class T>
static void copy_level(const GArrT<T> &big, const GArrT<T> &small, const int *d_list, int cnt, int dir, hipStream_t s)
{
    if (!(big.E > 0 && big.p && small.p) || cnt <= 0) return;
    const dim3 grid((cnt + 63) / 64, (big.E + 63) / 64), block(64);
    if (big.aos != small.aos) GQP_LAUNCH_COOP(gqp::k_compact_tile<T>, grid, block, 0, s, big, small, d_list, cnt, dir);
    else hipLaunchKernelGGL(gqp::k_compact_copy<T>, grid, block, 0, s, big, small, d_list, cnt, dir);
}

extern "C" {

/* forced: what a condensed batch or a sub-batch pins of the family choice (ForcedChoice).  Plain arguments: the library keeps no
 * state outside the objects its caller owns (SURVEY 8b "Threading"). */
static ocp_qp_gpu_batch *batch_create_shape(int N, const int *nx, const int *nu, const int *nbx, const int *nbu,
                                            const int *ng, const int *ns, int n_batch, int device, const ForcedChoice &forced);

ocp_qp_gpu_batch *ocp_qp_gpu_batch_create(int N, const int *nx, const int *nu, const int *nbx, const int *nbu,
                                          const int *ng, const int *ns, int n_batch, int device)
try
{
    return batch_create_shape(N, nx, nu, nbx, nbu, ng, ns, n_batch, device, ForcedChoice());
}
catch (const gqp_hip_failure &) { return nullptr; }

/* the object, its family (choose_family), the stream and pinned buffers every batch has */
static ocp_qp_gpu_batch *batch_create_shape(int N, const int *nx, const int *nu, const int *nbx, const int *nbu,
                                            const int *ng, const int *ns, int n_batch, int device, const ForcedChoice &forced)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    {
        fprintf(stderr, "acados_amd: no HIP device available -- the GPU OCP-QP path cannot run\n");
        return nullptr;
    }
    if (device >= 0) HIPCHK(hipSetDevice(device));
    ocp_qp_gpu_batch *b = new ocp_qp_gpu_batch();
    HIPCHK(hipGetDevice(&b->device));
    b->B = n_batch;
    b->Bp = (n_batch + 63) / 64 * 64;
    b->w16_slots = n_batch;
    b->N = N;
    DimsSummary d;
    for (int k = 0; k <= N; k++)
    {
        b->nx.push_back(nx[k]); b->nu.push_back(nu[k]); b->nbx.push_back(nbx[k]); b->nbu.push_back(nbu[k]);
        b->nb.push_back(nbx[k] + nbu[k]); b->ng.push_back(ng[k]); b->ns.push_back(ns[k]); b->nbxe.push_back(0);
        d.mx = std::max(d.mx, nx[k]); d.mu = std::max(d.mu, nu[k]); d.mg = std::max(d.mg, ng[k]); d.ms = std::max(d.ms, ns[k]);
        d.nct_max = std::max(d.nct_max, 2 * (nbx[k] + nbu[k] + ng[k]) + 2 * ns[k]);
        d.xbox_dims = d.xbox_dims || (k >= 1 && nbx[k] > 0);
        std::vector<int> ib;
        for (int i = 0; i < nbu[k]; i++) ib.push_back(i);
        for (int i = 0; i < nbx[k]; i++) ib.push_back(nu[k] + i);
        b->idxb.push_back(ib);
        b->idxs_rev.push_back(std::vector<int>(nbx[k] + nbu[k] + ng[k], -1));
        b->idxe.push_back(std::vector<int>());
    }
    FamilyChoice choice = choose_family(d, n_batch, forced, family_switches());
    if (!choice.ok)
    {
        fputs(choice.refusal.c_str(), stderr);
        delete b;
        return nullptr;
    }
    b->fam = choice.f;
    opts_default(b->O);
    HIPCHK(hipStreamCreate(&b->stream));
    HIPCHK(hipEventCreate(&b->ev0));
    HIPCHK(hipEventCreate(&b->ev1));
    HIPCHK(hipHostMalloc((void **) &b->h_nact, sizeof(int)));
    HIPCHK(hipHostMalloc((void **) &b->h_ints, sizeof(int) * 2 * (size_t) b->Bp));
    return b;
}

void ocp_qp_gpu_batch_destroy(ocp_qp_gpu_batch *b)
try
{
    if (!b) return;
    (void) hipSetDevice(b->device);
    (void) hipStreamSynchronize(b->stream);
    for (void *p : b->allocs) (void) hipFree(p);
    (void) hipHostFree(b->h_nact);
    (void) hipHostFree(b->h_ints);
    (void) hipEventDestroy(b->ev0);
    (void) hipEventDestroy(b->ev1);
    if (b->chunks_ev) (void) hipEventDestroy(b->chunks_ev);
    if (b->held.ev) (void) hipEventDestroy(b->held.ev);
    for (hipEvent_t e : b->prof_ev) (void) hipEventDestroy(e);
    (void) hipStreamDestroy(b->stream);
    if (b->child) ocp_qp_gpu_batch_destroy(b->child);
    for (SubBatch &sb : b->sub) ocp_qp_gpu_batch_destroy(sb.c);
    delete b;
}
catch (const gqp_hip_failure &) {}

int ocp_qp_gpu_batch_set_int(ocp_qp_gpu_batch *b, const char *f, int k, const int *v, int cnt)
try
{
    if (b->finalized)
    {
        fprintf(stderr, "acados_amd: structure field %s must be set before numeric data\n", f);
        return -1;
    }
    if (k < 0 || k > b->N) return -1;
    if (!strcmp(f, "idxb")) { b->idxb[k].assign(v, v + b->nb[k]); return 0; }
    if (!strcmp(f, "idxbu")) { for (int i = 0; i < b->nbu[k]; i++) b->idxb[k][i] = v[i]; return 0; }
    if (!strcmp(f, "idxbx")) { for (int i = 0; i < b->nbx[k]; i++) b->idxb[k][b->nbu[k] + i] = b->nu[k] + v[i]; return 0; }
    if (!strcmp(f, "idxs_rev")) { b->idxs_rev[k].assign(v, v + b->nb[k] + b->ng[k]); return 0; }
    if (!strcmp(f, "idxe")) { b->idxe[k].assign(v, v + cnt); b->nbxe[k] = cnt; return 0; }
    fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_set_int: unknown field %s\n", f);
    return -1;
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_set(ocp_qp_gpu_batch *b, const char *f, int stage, const double *data, int is_device)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, b->stream));
    const int k0 = stage < 0 ? 0 : stage, k1 = stage < 0 ? b->N : stage;
    const int grid = (b->B + 63) / 64;
    int rc = 0;
    const double *src = nullptr;
    int src_len = -1;
    const FieldRow *row = field_row(f);
    if (row && (row->flags & F_RES)) row = nullptr; /* (read only) */
    for (int k = k0; k <= k1; k++)
    {
        FieldRef s;
        const int len = field_resolve(b, row, k, USE_DATA, s);
        if (len < 0)
        {
            if (stage < 0) continue; /* field absent at this stage (e.g. A at N) */
            rc = -1;
            break;
        }
        if (len == 0) continue;
        if (src_len != len) { src = stage_in(b, data, (size_t) b->B * len, is_device); src_len = len; }
        int *dm = upload_map(b, s.map);
        if (s.mask())
        {
            hipLaunchKernelGGL(gqp::k_setmask, dim3(grid), dim3(64), 0, b->stream, src, b->B, len, dm, b->D.amask, k, b->fam.AW);
            continue;
        }
        b->held.data_written(s.arr == ARR_BAt, s.arr == ARR_RSQ); /* a writer of [B A]' / RSQ: stored verdicts are of older data */
        hipLaunchKernelGGL(gqp::k_scatter, dim3(grid), dim3(64), 0, b->stream, src, b->B, len, dm, arr_of(b, s.arr));
        if (s.arr2 != ARR_NONE)
        {
            dm = upload_map(b, s.map2);
            hipLaunchKernelGGL(gqp::k_scatter, dim3(grid), dim3(64), 0, b->stream, src, b->B, len, dm, arr_of(b, s.arr2));
        }
    }
    HIPCHK(hipEventRecord(e1, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    b->time_pack += ms * 1e-3;
    HIPCHK(hipEventDestroy(e0)); HIPCHK(hipEventDestroy(e1));
    if (rc) fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_set: unknown field %s (stage %d)\n", f, stage);
    return rc;
}
catch (const gqp_hip_failure &) { return -1; }

/* a new ric_alg: the sub-batches built for the old kernel set go, the factor in HBM is the old one's */
static void ric_switch(ocp_qp_gpu_batch *b, int v)
{
    b->ric_alg = v;
    for (SubBatch &sb : b->sub) { ocp_qp_gpu_batch_destroy(sb.c); sb.c = nullptr; } /* (the lists stay) */
    b->factor_stale = true;
    b->sens_open = false;
    if (b->child) ric_switch(b->child, v); /* the condensed batch of partial condensing */
    ric_configure(b);
}

/* (re)create the batch's stream with a priority; the batch must be idle */
static void set_stream_priority(ocp_qp_gpu_batch *b, int prio)
{
    int lo = 0, hi = 0; /* hip: "least" (numerically largest) and "greatest" (numerically smallest) priority */
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    const int p = prio < hi ? hi : (prio > lo ? lo : prio);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipStreamDestroy(b->stream));
    HIPCHK(hipStreamCreateWithPriority(&b->stream, hipStreamDefault, p));
    b->stream_priority = prio;
    /* sub-batches that exist already follow (the classical-Riccati one, the sensitivity slices and the condensed batch launch on
     * streams of their own); the ones created later take the priority at creation (round-3 advice) */
    for (SubBatch &sb : b->sub) if (sb.c) set_stream_priority(sb.c, prio);
    if (b->child) set_stream_priority(b->child, prio);
}

int ocp_qp_gpu_batch_opts_set(ocp_qp_gpu_batch *b, const char *f, const void *v)
try
{
    GqpOpts &o = b->O;
    const double *d = (const double *) v;
    const int *i = (const int *) v;
    if (!strcmp(f, "iter_max")) o.iter_max = *i;
    else if (!strcmp(f, "tol_stat")) o.tol_stat = *d;
    else if (!strcmp(f, "tol_eq")) o.tol_eq = *d;
    else if (!strcmp(f, "tol_ineq")) o.tol_ineq = *d;
    else if (!strcmp(f, "tol_comp")) o.tol_comp = *d;
    else if (!strcmp(f, "warm_start")) o.warm_start = *i;
    else if (!strcmp(f, "mu0")) { if (*d > 0.0) o.mu0 = *d; }
    else if (!strcmp(f, "alpha_min")) o.alpha_min = *d;
    else if (!strcmp(f, "tau_min")) o.tau_min = *d;
    else if (!strcmp(f, "tol_comp_soft_scale")) b->tol_comp_soft_scale = *d;
    else if (!strcmp(f, "full_dense")) b->full_dense = *i != 0;
    else if (!strcmp(f, "full_dense_slice")) b->full_dense_slice = *i < 0 ? 0 : *i;
    else if (!strcmp(f, "polish")) b->polish = *i < 0 ? 0 : (*i > 8 ? 8 : *i);
    else if (!strcmp(f, "polish_ratio")) b->polish_ratio = *d;
    else if (!strcmp(f, "polish_min")) b->polish_min = *d;
    else if (!strcmp(f, "reg_prim")) o.reg_prim = *d;
    else if (!strcmp(f, "cond_pred_corr")) o.cond_pred_corr = *i;
    else if (!strcmp(f, "print_level")) b->print_level = *i;
    else if (!strcmp(f, "profile")) b->profile = *i;
    else if (!strcmp(f, "cond_keep_iterate")) b->cond_keep_iterate = *i;
    else if (!strcmp(f, "marker"))
    {
        /* one empty launch named k_marker<id> on the batch's stream (id 0..15): section mark for rocprofv3 summaries */
        typedef void (*marker_t)(int *);
        static const marker_t mk[16] = {gqp::k_marker<0>, gqp::k_marker<1>, gqp::k_marker<2>, gqp::k_marker<3>, gqp::k_marker<4>,
                                        gqp::k_marker<5>, gqp::k_marker<6>, gqp::k_marker<7>, gqp::k_marker<8>, gqp::k_marker<9>,
                                        gqp::k_marker<10>, gqp::k_marker<11>, gqp::k_marker<12>, gqp::k_marker<13>,
                                        gqp::k_marker<14>, gqp::k_marker<15>};
        HIPCHK(hipSetDevice(b->device));
        hipLaunchKernelGGL(mk[*i & 15], dim3(1), dim3(64), 0, b->stream, (int *) nullptr);
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    else if (!strcmp(f, "stream_priority"))
    {
        /* several batches solved concurrently from host threads (the C5 classes): the long ones on a high-priority
         * stream (negative value, clamped to the device's range) are dispatched first, the short ones fill the gaps */
        set_stream_priority(b, *i); /* (every sub-batch and the condensed batch follow inside) */
    }
    else if (!strcmp(f, "compact_min")) b->compact_min = *i;
    else if (!strcmp(f, "tail_max")) b->tail_max = *i;
    else if (!strcmp(f, "hold_dynamics")) b->hold_dynamics = *i != 0;
    else if (!strcmp(f, "hold_hessian")) b->hold_hessian = *i != 0;
    else if (!strcmp(f, "compact_held")) b->compact_held = *i != 0;
    else if (!strcmp(f, "compact_held_min")) b->compact_held_min = *i;
    else if (!strcmp(f, "tail_div")) b->tail_div = *i < 1 ? 1 : *i;
    else if (!strcmp(f, "solve_max")) b->solve_max = *i;
    else if (!strcmp(f, "cond_N"))
    {
        if (*i != b->cond_N)
        {
            b->cond_N = *i;
            b->user_blocks.clear();
            b->pcond_state = 0;
            if (b->child) { ocp_qp_gpu_batch_destroy(b->child); b->child = nullptr; }
        }
    }
    else if (!strcmp(f, "cond_block_size"))
    {
        /* user block sizes, N2 + 1 entries as ocp_qp_partial_condensing.c:305-313; set cond_N first.  They must sum to
         * N (:346-356).  A non-zero LAST entry (the reference's own test: qp_solver_cond_block_size = [6, 5, 4, 2, 2, 1],
         * examples/acados_python/tests/pcond_getters_test.py:200) asks HPIPM to fold the last stages' inputs into the terminal
         * stage; here those stages form one more block in front of an input-free terminal stage (the condensed QP has
         * N2 + 1 stages with inputs instead of N2 -- the solution of the original QP is the same, the layout of the condensed
         * one differs: INTEGRATION.md 3). */
        const int N2 = b->cond_N;
        if (N2 <= 0 || N2 >= b->N) { fprintf(stderr, "acados_amd: cond_block_size needs cond_N in 1..N-1 first\n"); return -1; }
        int sum = 0;
        for (int j = 0; j <= N2; j++) sum += i[j];
        bool ok = sum == b->N && i[N2] >= 0;
        for (int j = 0; j < N2; j++) ok = ok && i[j] >= 1;
        if (!ok)
        {
            fprintf(stderr, "acados_amd: partial condensing: block sizes must be >= 1 (the last one >= 0) and sum to N = %d (got %d)\n", b->N, sum);
            return -1;
        }
        const std::vector<int> blocks(i, i + N2 + (i[N2] > 0 ? 1 : 0));
        if (blocks != b->user_blocks) /* the same sizes again (an adapter sends its options before every solve): nothing to redo */
        {
            b->user_blocks = blocks;
            b->pcond_state = 0;
            if (b->child) { ocp_qp_gpu_batch_destroy(b->child); b->child = nullptr; }
        }
    }
    else if (!strcmp(f, "t0_min")) b->t0_min = *d;
    else if (!strcmp(f, "lam0_min")) b->lam0_min = *d;
    else if (!strcmp(f, "update_fact_exit")) { /* the factor sweep factorises before it decides: the factor at the exit
                                                  point is always there (and re-done lazily after a hand-over) */ }
    else if (!strcmp(f, "t0_init"))
    {
        /* acados_ocp_options.py:1128-1143: 0 lam = t = sqrt(mu0); 1 lam = mu0, t = 1; 2 from the constraint residuals */
        if (*i < 0 || *i > 2) { fprintf(stderr, "acados_amd: t0_init must be 0, 1 or 2, got %d\n", *i); return -1; }
        o.t0_init = *i;
    }
    else if (!strcmp(f, "ric_alg"))
    {
        /* acados_ocp_options.py:1084-1101: 1 square-root Riccati (the full-space stage Hessian must be positive definite), 0
         * classical (only the reduced Hessian must be).  The same value again (the adapters resend their options before every
         * solve) costs nothing; a change takes effect at the next solve */
        if (*i != 0 && *i != 1) { fprintf(stderr, "acados_amd: ric_alg must be 0 or 1, got %d\n", *i); return -1; }
        if (*i != b->ric_alg) ric_switch(b, *i);
    }
    else if (!strcmp(f, "hpipm_mode"))
    {
        /* modes only reset defaults in the reference (ocp_qp_hpipm.c:142-165) */
        const char *mode = (const char *) v;
        if (strcmp(mode, "BALANCE") && strcmp(mode, "SPEED") && strcmp(mode, "SPEED_ABS") && strcmp(mode, "ROBUST"))
        {
            fprintf(stderr, "acados_amd: got non-supported mode %s\n", mode);
            return -1;
        }
        const double t1 = o.tol_stat, t2 = o.tol_eq, t3 = o.tol_ineq, t4 = o.tol_comp;
        const int im = o.iter_max, ws = o.warm_start;
        opts_default(o);
        o.tol_stat = t1; o.tol_eq = t2; o.tol_ineq = t3; o.tol_comp = t4; o.iter_max = im; o.warm_start = ws;
    }
    else
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_opts_set: unknown option %s\n", f);
        return -1;
    }
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }


/* ---- partial condensing (ocp_qp_partial_condensing.c:523-556, :664-689) ---- */
static void pcond_setup(ocp_qp_gpu_batch *b)
{
    /* blocks with inputs: cond_N of them, one more when the user's last block size is not 0 (see "cond_block_size") */
    const int N = b->N, N2 = (int) b->user_blocks.size() == b->cond_N + 1 ? b->cond_N + 1 : b->cond_N;
    b->pcond_state = -1;
    auto decline = [&](const char *why) {
        if (b->full_dense) return; /* the caller knows: this batch only probes whether ONE block fits a condensed stage (FULL_CONDENSING) */
        fprintf(stderr, "acados_amd: cond_N=%d requested but %s; solving the full-space QP (N2 = N, the default of "
                        "ocp_qp_partial_condensing.c:243-265) -- the solution is identical\n", N2, why);
    };
    if (b->cond_N <= 0 || b->cond_N >= N) return;
    /* block sizes as d_part_cond_qp_compute_block_size: N/N2 each, remainder to the first blocks */
    b->blk_start.assign(N2 + 1, 0);
    int bsmax = 0;
    for (int j = 0; j < N2; j++)
    {
        const int bs = (int) b->user_blocks.size() == N2 ? b->user_blocks[j] : N / N2 + (j < N % N2 ? 1 : 0);
        b->blk_start[j + 1] = b->blk_start[j] + bs;
        bsmax = std::max(bsmax, bs);
    }
    std::vector<char> is_start(N + 1, 0);
    for (int j = 0; j <= N2; j++) is_start[b->blk_start[j]] = 1;
    /* box-only class: input bounds anywhere, state bounds at block starts only -- every child row is a box row;
     * anything else (state bounds inside a block, general rows, slacks) makes general rows in the condensed stages,
     * which only the wave-per-instance condensing kernels write */
    bool box_class = true;
    for (int k = 0; k <= N; k++)
        if (b->ng[k] || b->ns[k] || (b->nbx[k] && !is_start[k])) box_class = false;
    b->pc = nullptr;
    b->pc_rt = 0;
    for (int q = 0; q < g_n_pcond_sets; q++)
        if (g_pcond_sets[q].NX == b->fam.ks()->NX && g_pcond_sets[q].NU == b->fam.ks()->NU && g_pcond_sets[q].BSMAX >= bsmax &&
            (!b->pc || g_pcond_sets[q].BSMAX < b->pc->BSMAX))
            b->pc = &g_pcond_sets[q];
    /* the wave-per-instance condensing kernels take every shape with nx + bs*nu <= 64 at run time; the compiled
     * one-instance-per-lane ones remain as the cross-check (ACADOS_AMD_PCOND_1TPI=1) */
    {
        const char *e1 = getenv("ACADOS_AMD_PCOND_1TPI");
        const bool want_1tpi = e1 && atoi(e1) != 0 && box_class;
        if (!(want_1tpi && b->pc) && b->fam.ks()->NX + bsmax * b->fam.ks()->NU <= 64) b->pc_rt = 1;
    }
    /* Expansion of a WAVE-TILED parent: element e of eight neighbouring instances shares a 64-byte line, so a kernel that
     * walks one instance per wave moves eight lines for every one it uses -- kw_pexpand is bound by that traffic (13.3 ms
     * per 65,536 instances of the C2 shape).  The compiled one-instance-per-lane kernel reads the same data coalesced:
     * 1.6 ms.  (Condensing stays with kw_pcond: the per-lane block matrices of k_pcond do not fit the register file.) */
    {
        const char *e2 = getenv("ACADOS_AMD_PCOND_LANE_EXPAND");
        b->pc_lane_expand = b->pc && b->pc->BSMAX == bsmax && box_class && !b->fam.aos && !(e2 && atoi(e2) == 0);
    }
    b->pcz = nullptr;
    {
        const char *e3 = getenv("ACADOS_AMD_PCOND_W16");
        if (box_class && !(e3 && atoi(e3) == 0))
            for (const PcondzSet &z : g_pcondz_sets)
                if (z.NX == b->fam.ks()->NX && z.NU == b->fam.ks()->NU && z.BS == bsmax) b->pcz = &z;
        const char *e4 = getenv("ACADOS_AMD_PCOND_MFMA");
        b->pcz_mfma = !(e4 && atoi(e4) == 0);
    }
    if (!box_class && !b->pc_rt) { decline("the condensed stage (nx + block size * nu > 64) is beyond the condensing kernels"); return; }
    if (!b->pc && !b->pc_rt) { decline("no condensing kernel covers this shape / block size"); return; }
    const int NU = b->fam.ks()->NU, BS = b->pc_rt ? bsmax : b->pc->BSMAX;
    b->pc_shmem = gqp::pcondw_lds_doubles(b->fam.ks()->NX, NU, BS * NU) * sizeof(double);

    /* child dims + structure.  Child rows in their original order: [input boxes of the block's stages][state boxes of
     * the block's first stage][general rows: per stage of the block, its state boxes (inner stages) then its general
     * rows]; child slacks: the block's stages one after the other */
    std::vector<int> cnx(N2 + 1), cnu(N2 + 1), cnbx(N2 + 1), cnbu(N2 + 1), cng(N2 + 1, 0), cns(N2 + 1, 0);
    std::vector<std::vector<int>> cidxb(N2 + 1), row_kp(N2 + 1), row_op(N2 + 1), crev(N2 + 1);
    std::vector<int> cidxe, h_gk(N + 2, 0), h_grp, h_gvar, h_soff(N2 + 2, 0), h_skp, h_ssp, slack_base(N + 1, 0);
    for (int j = 0; j <= N2; j++)
    {
        const int k0 = b->blk_start[j], k1 = j < N2 ? b->blk_start[j + 1] : N + 1;
        const int kend = j < N2 ? k1 : k0 + 1; /* stages of this block */
        cnx[j] = b->nx[k0];
        cnu[j] = j < N2 ? (k1 - k0) * NU : 0;
        for (int k = k0; k < (j < N2 ? k1 : k0); k++)
            for (int r = 0; r < b->nbu[k]; r++)
            {
                cidxb[j].push_back((k - k0) * NU + b->idxb[k][r]);
                row_kp[j].push_back(k); row_op[j].push_back(r);
            }
        cnbu[j] = (int) cidxb[j].size();
        for (int r = 0; r < b->nbx[k0]; r++)
        {
            cidxb[j].push_back(cnu[j] + (b->idxb[k0][b->nbu[k0] + r] - b->nu[k0]));
            row_kp[j].push_back(k0); row_op[j].push_back(b->nbu[k0] + r);
        }
        cnbx[j] = b->nbx[k0];
        if (j == 0)
            for (size_t e = 0; e < b->idxe[0].size(); e++) cidxe.push_back(cnbu[0] + (b->idxe[0][e] - b->nbu[0]));
        if (j > 0 && !b->idxe[k0].empty()) { decline("equality-flagged bounds after stage 0"); return; }
        if (j == N2 && b->nbu[N]) { decline("input bounds at the terminal stage"); return; }
        for (int k = k0; k < kend; k++)
        {
            if (k > k0 && !b->idxe[k].empty()) { decline("equality-flagged bounds after stage 0"); return; }
            h_gk[k] = (int) h_grp.size();
            if (k > k0)
                for (int r = b->nbu[k]; r < b->nb[k]; r++)
                {
                    h_grp.push_back(b->perm[k][r]); h_gvar.push_back(b->idxb[k][r] - b->nu[k]);
                    row_kp[j].push_back(k); row_op[j].push_back(r);
                }
            for (int g = 0; g < b->ng[k]; g++)
            {
                h_grp.push_back(b->nb[k] + g); h_gvar.push_back(0);
                row_kp[j].push_back(k); row_op[j].push_back(b->nb[k] + g);
            }
            slack_base[k] = cns[j];
            for (int q = 0; q < b->ns[k]; q++) { h_skp.push_back(k); h_ssp.push_back(q); }
            cns[j] += b->ns[k];
        }
        cng[j] = (int) row_kp[j].size() - (int) cidxb[j].size();
        h_soff[j + 1] = h_soff[j] + cns[j];
        const int nrow = (int) row_kp[j].size();
        if (nrow > GQP_MAX_ROWS || 2 * nrow + 2 * cns[j] > 128)
        {
            decline("a condensed stage would carry more than 64 inequality rows / 128 sides");
            return;
        }
        crev[j].assign(nrow, -1);
        for (int oc = 0; oc < nrow; oc++)
        {
            const int k = row_kp[j][oc], sj = b->idxs_rev[k].empty() ? -1 : b->idxs_rev[k][row_op[j][oc]];
            if (sj >= 0) crev[j][oc] = slack_base[k] + sj;
        }
    }
    h_gk[N + 1] = (int) h_grp.size();
    ocp_qp_gpu_batch *c = batch_create_shape(N2, cnx.data(), cnu.data(), cnbx.data(), cnbu.data(), cng.data(), cns.data(),
                                             b->B, b->device, ForcedChoice{b->fam.ks()->NX, BS * NU});
    if (c && b->stream_priority) set_stream_priority(c, b->stream_priority);
    if (!c) { decline("the condensed shape has no kernel instantiation"); return; }
    if (b->ric_alg != c->ric_alg) ric_switch(c, b->ric_alg); /* condensing never factorises: the child's sweeps carry the choice */
    for (int j = 0; j <= N2; j++)
    {
        if (!cidxb[j].empty()) ocp_qp_gpu_batch_set_int(c, "idxb", j, cidxb[j].data(), (int) cidxb[j].size());
        if (cns[j]) ocp_qp_gpu_batch_set_int(c, "idxs_rev", j, crev[j].data(), (int) crev[j].size());
    }
    ocp_qp_gpu_batch_set_int(c, "idxe", 0, cidxe.data(), (int) cidxe.size());
    finalize_structure(c);
    /* row maps in the sorted (device) row order of both batches: box rows sorted by variable, general rows as listed */
    std::vector<int> h_off(N2 + 2, 0), h_kp, h_rp;
    for (int j = 0; j <= N2; j++)
    {
        const int nb = (int) cidxb[j].size(), nrow = (int) row_kp[j].size();
        std::vector<int> kp(nrow), rp(nrow);
        for (int oc = 0; oc < nrow; oc++)
        {
            const int rc = oc < nb ? c->perm[j][oc] : oc;
            const int k = row_kp[j][oc], op = row_op[j][oc];
            kp[rc] = k;
            rp[rc] = op < b->nb[k] ? b->perm[k][op] : op;
        }
        h_kp.insert(h_kp.end(), kp.begin(), kp.end());
        h_rp.insert(h_rp.end(), rp.begin(), rp.end());
        h_off[j + 1] = h_off[j] + nrow;
    }
    auto up = [&](const std::vector<int> &v) {
        int *d = dalloc<int>(b, std::max<size_t>(1, v.size()));
        if (!v.empty()) HIPCHK(hipMemcpy(d, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice));
        return d;
    };
    int *d_start = up(b->blk_start), *d_kp = up(h_kp), *d_rp = up(h_rp), *d_off = up(h_off);
    b->pmap.gk_off = up(h_gk); b->pmap.g_rp = up(h_grp); b->pmap.g_var = up(h_gvar);
    b->pmap.slk_off = up(h_soff); b->pmap.slk_kp = up(h_skp); b->pmap.slk_sp = up(h_ssp);
    b->pmap.blk_start = d_start; b->pmap.row_kp = d_kp; b->pmap.row_rp = d_rp; b->pmap.row_off = d_off; b->pmap.N2 = N2;
    b->child = c;
    b->pcond_state = 1;
}

static void pcond_launch(ocp_qp_gpu_batch *b, bool expand)
{
    ocp_qp_gpu_batch *c = b->child;
    if (!expand) c->held.data_written(true, true); /* the condensing kernels write the child's matrices: it is the root of its own solve */
    if (!expand && b->pcz && b->pc_rt && b->fam.AW <= 1 && c->fam.AW <= 1)
    {
        const dim3 grid((b->B + 3) / 4, b->pmap.N2 + 1);
        if (b->pcz_mfma)
            GQP_LAUNCH_COOP(b->pcz->cond_m, dim3((b->B + KM_PCOND_THREADS / 16 - 1) / (KM_PCOND_THREADS / 16), b->pmap.N2 + 1), dim3(KM_PCOND_THREADS), 0,
                            b->stream, b->D, c->D, b->pmap);
        else GQP_LAUNCH_COOP(b->pcz->cond, grid, dim3(64), b->pcz->shmem, b->stream, b->D, c->D, b->pmap);
        return;
    }
    if ((b->pc_rt || b->fam.AW > 1 || c->fam.AW > 1) && !(expand && b->pc_lane_expand && b->fam.AW <= 1 && c->fam.AW <= 1))
    {
        /* (the expansion keeps four 64-entry vectors in LDS, not the condensing's block matrices: with the small allocation a CU holds
         *  all the waves its SIMDs take) */
        if (expand) GQP_LAUNCH_COOP(gqp::kw_pexpand, dim3(b->Bp, b->pmap.N2 + 1), dim3(64), 4 * 64 * sizeof(double), b->stream, b->D, c->D, b->pmap);
        else GQP_LAUNCH_COOP(gqp::kw_pcond, dim3(b->Bp), dim3(64), b->pc_shmem, b->stream, b->D, c->D, b->pmap);
    }
    else
    {
        const kern_pcond_t kern = expand ? b->pc->expand : b->pc->cond;
        hipLaunchKernelGGL(kern, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, b->D, c->D, b->pmap);
    }
}

static int pcond_solve(ocp_qp_gpu_batch *b, int mode = 3)
{
    ocp_qp_gpu_batch *c = b->child;
    b->pmap.mode = mode;
    const dim3 grid((b->B + 63) / 64), block(64);
    hipEvent_t e0, e1, e2, e3;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventCreate(&e2)); HIPCHK(hipEventCreate(&e3));
    c->O = b->O;
    c->tol_comp_soft_scale = b->tol_comp_soft_scale;
    c->polish = b->polish; c->polish_ratio = b->polish_ratio; c->polish_min = b->polish_min;
    c->print_level = b->print_level;
    HIPCHK(hipEventRecord(e0, b->stream));
    pcond_launch(b, false);
    if (b->O.warm_start >= 2 && !b->cond_keep_iterate)
        /* hot start: the root's iterate restated in the condensed variables (condense_qp_out,
         * ocp_qp_xcond_solver.c:554-565) is the child's starting point -- unless the caller keeps the child's own last
         * iterate (the reference's default: initialize_next_xcond_qp_from_qp_out clear) */
        hipLaunchKernelGGL(gqp::k_pcond_sol, grid, block, 0, b->stream, b->D, c->D, b->pmap);
    HIPCHK(hipEventRecord(e1, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    c->t0_min = b->t0_min; c->lam0_min = b->lam0_min;
    c->profile = b->profile; /* per-class event times of the condensed solve are reported on the root */
    const int bad = ocp_qp_gpu_batch_solve(c);
    for (int q = 0; q < 6; q++)
    {
        b->prof_ms[q] += c->prof_ms[q]; b->prof_cnt[q] += c->prof_cnt[q];
        c->prof_ms[q] = 0.0; c->prof_cnt[q] = 0;
    }
    HIPCHK(hipEventRecord(e2, b->stream));
    pcond_launch(b, true);
    HIPCHK(hipEventRecord(e3, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipGetLastError());
    float m0 = 0.f, m1 = 0.f;
    HIPCHK(hipEventElapsedTime(&m0, e0, e1));
    HIPCHK(hipEventElapsedTime(&m1, e2, e3));
    b->time_xcond = (m0 + m1) * 1e-3;
    b->time_tot = c->time_tot + b->time_xcond;
    b->last_iters = c->last_iters;
    b->launches = c->launches + 2;
    HIPCHK(hipEventDestroy(e0)); HIPCHK(hipEventDestroy(e1)); HIPCHK(hipEventDestroy(e2)); HIPCHK(hipEventDestroy(e3));
    return bad;
}

/* ---- the IPM launch loop of one level (root batch or compaction sub-batch) ---- */
extern "C++" { /* (templates among them: the surrounding block has C linkage) */
/* a sweep kernel of one level with the dynamic LDS bytes it takes in that level's family (the one-instance-per-lane family: none) */
struct Sweep
{
    kern_redo_t fn;
    size_t shm;
};
struct IpmKernels
{
    Sweep fact, rhs, faff, fcorr;
    Sweep fact_held, rhs_held; /* fact / rhs with [B A]' held across the stages, for a launch whose tiles are all held (static LDS of
                                * their own); fn null: there is none */
    kern_plain_t final_;
};

/* One launch of a kernel of level b.  Grid and launch form come from the family, here and nowhere else: the four sweeps of a
 * sixteen-lanes batch pack 4 row slots into a 64-lane workgroup (w16_slots is read NOW: run_ipm shrinks it when the permutation comes
 * on); the wave-per-instance families take one single-wave workgroup per instance, stage matrices in dynamic LDS; one instance per
 * lane is a plain launch of 64 instances per single-wave block without dynamic LDS. */
template <class Kern, class... Args>
static void launch_level(const ocp_qp_gpu_batch *b, Kern fn, size_t shm, bool sweep, hipStream_t s, const Args &...args)
{
    if (sweep && b->fam.w16()) GQP_LAUNCH_COOP(fn, dim3((b->w16_slots + 3) / 4), dim3(64), shm, s, args...);
    else if (!b->fam.lane()) GQP_LAUNCH_COOP(fn, dim3(b->B), dim3(64), shm, s, args...);
    else hipLaunchKernelGGL(fn, dim3((b->B + 63) / 64), dim3(64), 0, s, args...);
}
static void launch_sweep(const ocp_qp_gpu_batch *b, const Sweep &k, hipStream_t s, const GqpDev &D, const GqpOpts &O, int redo)
{
    launch_level(b, k.fn, k.shm, true, s, D, O, redo);
}
/* init and finalize: one block per instance / per 64 instances in every family, the LDS bytes of the rhs sweep */
template <class Kern, class... Args>
static void launch_whole(const ocp_qp_gpu_batch *b, Kern fn, hipStream_t s, const Args &...args)
{
    launch_level(b, fn, b->fam.lds.whole, false, s, args...);
}

static IpmKernels pick_kernels(const ocp_qp_gpu_batch *b)
{
    const KernelSet *ks = b->fam.ks();
    const int xb = b->fam.xbox;
    const bool lane_box = b->fam.use_box && b->fam.lane();
    /* the family's box sweeps: the serving ones, or the ipm_kernels_box.hpp kernels where the batch asks for them */
    const BoxSweeps &bx = (lane_box && b->fam.kb_plain && ks->kb.fact[xb]) ? ks->kb : ks->box;
    const FamilyLds &lds = b->fam.lds;
    IpmKernels k;
    k.fact = {b->fam.use_box ? bx.fact[xb] : ks->back_fact, lds.fact};
    k.rhs = {b->fam.use_box ? bx.rhs[xb] : ks->back_rhs, lds.rhs};
    k.faff = {b->fam.use_box ? bx.fwd_aff[xb] : ks->fwd_aff, lds.fwd};
    k.fcorr = {b->fam.use_box ? bx.fwd_corr[xb] : ks->fwd_corr, lds.fwd};
    /* held entries: one instance per lane, box rows on the controls only */
    const bool held = lane_box && !xb;
    k.fact_held = {held ? bx.fact_held : nullptr, 0};
    k.rhs_held = {held ? bx.rhs_held : nullptr, 0};
    k.final_ = b->fam.use_box ? ks->box_finalize : ks->finalize;
    return k;
}

/* per-kernel-class HIP event timing, accumulated on the ROOT batch */
struct Prof
{
    ocp_qp_gpu_batch *root;
    size_t used = 0;
    /* launch() bracketed by an event pair of class cls -- where `on`: the root level only (full-batch launches) */
    template <class F>
    void timed(int cls, hipStream_t s, bool on, F &&launch)
    {
        on = on && root->profile;
        if (on)
        {
            if (used + 2 > root->prof_ev.size())
            {
                hipEvent_t e0, e1;
                HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
                root->prof_ev.push_back(e0); root->prof_ev.push_back(e1);
            }
            root->prof_cls.push_back(cls);
            HIPCHK(hipEventRecord(root->prof_ev[used], s));
        }
        launch();
        if (on)
        {
            HIPCHK(hipEventRecord(root->prof_ev[used + 1], s));
            used += 2;
        }
    }
};
} /* extern "C++" */

static ocp_qp_gpu_batch *compact_into(ocp_qp_gpu_batch *b, ocp_qp_gpu_batch *root, hipStream_t s, SubRole role, const HeldDynamics *known);
static void compact_back(ocp_qp_gpu_batch *b, hipStream_t s, SubRole role, int it0);
static void run_ipm(ocp_qp_gpu_batch *b, ocp_qp_gpu_batch *root, Prof &prof, hipStream_t s, int it, bool polish = false);

/*
 * One level of the IPM loop.  After the factor kernel of every iteration the host reads the
 * number of still-iterating instances.  Converged instances are scattered over the waves, so a
 * wave keeps paying full HBM traffic as long as ONE of its 64 lanes is active; when at most half
 * of the level is still iterating, the survivors (QP data + iterate, ~98 KB each for C2) are
 * copied into a dense sub-batch, the loop continues there (recursively), and the results are
 * scattered back.  Per-instance arithmetic is unchanged, so results are bit-identical.
 *
 * Held dynamics (ipm_kernels_box.hpp; the protocol is HeldDynamics below): the ROOT level runs every sweep of its loop with
 * GqpOpts::hold bit 0 and lets its first affine forward sweep count the lanes with stage-invariant [B A]' (bit 1).  From the
 * iteration after that one on, if EVERY tile of the batch is held, the factor launch and both rhs-only launches go to the entries
 * that hold the block too (IpmKernels::fact_held, gqp::kh_factor; IpmKernels::rhs_held, gqp::kh_backrhs).  They read no flag: a
 * mixed batch, the iteration that detects and every launch outside this loop (sub-levels, tail, sensitivities, ric_alg 0) keep
 * K.fact and K.rhs, which fetch at every stage.  Sub-levels never set either bit and nothing of it is copied by compact_into --
 * with one exception, the dense held level (option compact_held): a loop whose tiles ALL hold may compact its survivors into a level
 * that runs the held entries too; that level's record is switched on by HeldDynamics::adopt and off again by end().
 * What the loop knows of the matrices also shortens its hand-overs (sub_batch_load, "held data").
 */
/* side -> (stage, activity bit) of k_step_update, once per batch */
static const int *side_map(ocp_qp_gpu_batch *b)
{
    if (b->d_side_map) return b->d_side_map;
    std::vector<int> h((size_t) std::max(b->nct_tot, 1), -1);
    for (int k = 0; k <= b->N; k++)
    {
        const GqpStage &S = b->st[k];
        const int nbg = S.nb + S.ng;
        int sp = 0;
        for (int pv = 0; pv < 64; pv++)
            if ((S.bmask >> pv) & 1)
            {
                if (!((S.emask >> pv) & 1)) { h[S.o_ct + sp] = k * 128 + sp; h[S.o_ct + nbg + sp] = k * 128 + nbg + sp; }
                sp++;
            }
        for (int g = 0; g < S.ng; g++) { h[S.o_ct + S.nb + g] = k * 128 + S.nb + g; h[S.o_ct + nbg + S.nb + g] = k * 128 + nbg + S.nb + g; }
        for (int q = 0; q < 2 * S.ns; q++) h[S.o_ct + 2 * nbg + q] = k * 128 + 2 * nbg + q;
    }
    b->d_side_map = dalloc<int>(b, h.size());
    HIPCHK(hipMemcpy(b->d_side_map, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice));
    return b->d_side_map;
}

/* 1: the host waits for the detector's counters right behind the detecting sweep, so that the rhs pair of that iteration is held
 * too -- one held launch pair more per solve for one drained queue (the cross-check: make variant TAG=holdsync
 * DEFS=-DGQP_HOLD_SYNC=1, tools/variant_rate.py c2 libacados_amd_qp_holdsync.so; kept at 0 until both are measured, profiles/NOTES.md) */
#ifndef GQP_HOLD_SYNC
#define GQP_HOLD_SYNC 0
#endif

void HeldDynamics::begin(ocp_qp_gpu_batch *root, hipStream_t s, bool polish_loop)
{
    b = root;
    polish = polish_loop;
    enabled = b->hold_dynamics && b->fam.use_box && b->fam.lane();
    pending_ver = 0;
    const size_t bytes = sizeof(int) * (size_t) (b->Bp / 64);
    if (enabled && !polish && kept_at == ver_dyn)
    {
        /* the matrices are the ones the stored count was taken on: the loop starts where the detecting iteration would leave it */
        state = COUNTED;
        tiles = tiles_invariant = kept_tiles;
        HIPCHK(hipMemcpyAsync(b->D.tile_inv, d_kept, bytes, hipMemcpyDeviceToDevice, s));
        return;
    }
    state = enabled ? DETECTING : COUNTED;
    tiles = 0;
    HIPCHK(hipMemsetAsync(b->D.tile_inv, 0, bytes, s));
}

void HeldDynamics::after_detect(hipStream_t s, bool all_running)
{
    if (state != DETECTING) return;
    HIPCHK(hipMemcpyAsync(b->h_ints, b->D.tile_inv, sizeof(int) * (size_t) (b->Bp / 64), hipMemcpyDeviceToHost, s));
    if (!polish)
    {
        /* the counters as they stand, for the solves to come (count() decides whether they are kept) */
        HIPCHK(hipMemcpyAsync(d_kept, b->D.tile_inv, sizeof(int) * (size_t) (b->Bp / 64), hipMemcpyDeviceToDevice, s));
        pending_ver = ver_dyn;
        complete = all_running;
        detects++;
    }
    if (!ev) HIPCHK(hipEventCreate(&ev)); /* once per batch */
    HIPCHK(hipEventRecord(ev, s));
    state = AWAITING;
#if GQP_HOLD_SYNC
    HIPCHK(hipStreamSynchronize(s));
    count();
#endif
}

void HeldDynamics::before_factor(bool fact_entry)
{
    if (state != AWAITING) return;
    /* a shape without a held factor entry has nothing to choose here: its count is taken behind the wait for the stream that
     * follows the factor launch anyway (stream_drained), in time for the rhs pair */
    if (!fact_entry) return;
    /* the counters were copied back behind the detecting sweep of the iteration before: wait for THAT copy, not for the stream
     * -- the rhs and corrector launches of that iteration are still queued behind it, the device does not idle -- so that this
     * factor launch can already be the held one */
#if defined(__HIPCC__) /* (the host simulation copies synchronously: nothing to wait for) */
    HIPCHK(hipEventSynchronize(ev));
#endif
    count();
}

void HeldDynamics::count()
{
    tiles = 0;
    for (int q = 0; q < (b->B + 63) / 64; q++) tiles += b->h_ints[q] == std::min(64, b->B - 64 * q);
    if (!polish) tiles_invariant = tiles;
    state = COUNTED;
    /* kept for the solves to come: a full count always; a partial one only where no wave can have left the sweep uncounted */
    if (pending_ver && (complete || tiles == (b->B + 63) / 64))
    {
        kept_at = pending_ver;
        kept_tiles = tiles;
    }
    pending_ver = 0;
}

void HeldDynamics::stream_drained()
{
    if (state == AWAITING) count();
}

bool HeldDynamics::all_held() const { return enabled && state == COUNTED && tiles == (b->B + 63) / 64; }

bool HeldDynamics::hessian_verdict(hipStream_t s)
{
    if (hess_at == ver_hess) return hess_inv;
    const int nt = (b->B + 63) / 64;
    int *h = b->h_ints; /* (the counters of the dynamics have been summed: count() is behind us) */
    HIPCHK(hipMemsetAsync(d_hess_cnt, 0, sizeof(int) * (size_t) (b->Bp / 64), s));
    hipLaunchKernelGGL(gqp::k_hess_invariant, dim3(nt), dim3(64), 0, s, b->D, d_hess_cnt);
    HIPCHK(hipMemcpyAsync(h, d_hess_cnt, sizeof(int) * (size_t) nt, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int full = 0;
    for (int q = 0; q < nt; q++) full += h[q] == std::min(64, b->B - 64 * q);
    hess_inv = full == nt;
    hess_at = ver_hess;
    hess_detects++;
    return hess_inv;
}

void HeldDynamics::end(hipStream_t s)
{
    if (b) HIPCHK(hipMemsetAsync(b->D.tile_inv, 0, sizeof(int) * (size_t) (b->Bp / 64), s));
    if (level) enabled = level = false;
}

void HeldDynamics::adopt(ocp_qp_gpu_batch *lv, int cnt, bool root_hess_inv)
{
    b = lv;
    enabled = level = true;
    polish = false;
    pending_ver = 0;
    state = COUNTED;
    tiles = (cnt + 63) / 64;
    hess_at = ver_hess; /* (sub_batch_load has bumped the versions: the verdict is of what it copied) */
    hess_inv = root_hess_inv;
}

static void run_ipm(ocp_qp_gpu_batch *b, ocp_qp_gpu_batch *root, Prof &prof, hipStream_t s, int it, bool polish)
{
    const IpmKernels K = pick_kernels(b);
    const bool top = b == root; /* per-class timing and held dynamics belong to the root level */
    GqpDev D = b->D;
    GqpOpts O = effective_opts(root->O, root);
    /* sixteen-lanes families, launch per sweep: the step is applied by a launch of its own (k_step_update) instead of a pass at
     * the end of the corrector sweep, which walks the stages one after the other inside a latency-bound kernel.  Measured
     * (tools/ext_update_ab.py, profiles/r05_ext_update_ab.txt; identical iterates): general rows + slacks (two memory round trips
     * per stage in the pass) C4 124.0 -> 120.4 ms; box classes of 7,281 instances +0.2 ... +1.1 %; the condensed C3 batch
     * (65,536 instances, bandwidth-bound: the pass overlaps with other workgroups' sweeps, a launch of its own does not) 48.4 ->
     * 49.4 ms; short horizons (N = 20) lose what one more launch per iteration costs (r05_ext_update_ab2.txt: -2.6 % at nx = 12) -- so:
     * GEN always, box classes up to 16,384 instances from N = 50 on.  ACADOS_AMD_EXT_UPDATE=0 / 1 forces the pass / the launch */
    const FamilySwitches sw = family_switches(); /* (read at every solve: tools/ext_update_ab.py changes them between two) */
    const bool ext_update = b->fam.w16() && (sw.ext_update.set ? sw.ext_update.v != 0 : (b->fam.ng > 0 || (b->B <= 16384 && b->N >= 50)));
    HeldDynamics none; /* a sub-level takes no part -- but for the dense level of an all-held root (compact_into: adopt()) */
    HeldDynamics &H = top ? root->held : b->held.level ? b->held : none;
    HeldDynamics &Hroot = root->held; /* the scalars of the solve */
    if (top) H.begin(root, s, polish);
    O.hold = H.bits();
    GqpOpts Oc = O; /* options of the corrector-sweep launches */
    Oc.ext_update = ext_update ? 1 : 0;
    const int *smap = ext_update ? side_map(b) : nullptr;
    b->w16_slots = b->B;
    /* sixteen lanes per instance: once a sixth of the slots has converged the sweeps run over a dense list of the live
     * instances (row slot -> instance, GqpDev::perm) -- no data moves, the grid shrinks, every wave carries four live rows */
    const bool use_perm = b->fam.w16() && !sw.w16_perm.off();
    if (top && b->fam.w16() && b->fam.solve && b->B <= root->solve_max && !D.perm)
    {
        /* small batch: every 16-lane row runs this loop by itself inside one launch (kx_solve) */
        prof.timed(1, s, true, [&] { launch_sweep(b, Sweep{b->fam.solve, b->fam.lds.rhs}, s, D, O, 0); });
        root->launches++;
        root->n_single_launch++;
        HIPCHK(hipMemcpyAsync(b->h_nact, D.n_active, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (*b->h_nact <= 0)
        {
            H.end(s);
            return;
        }
        /* (never taken: a row leaves the kernel only with its instance out of the RUNNING state) */
    }
    for (;; it++)
    {
        H.before_factor(K.fact_held.fn != nullptr);
        /* the held entries (factor here, the rhs pair below) read no flag: one tile that must fetch keeps K.fact / K.rhs for the
         * whole launch, and so does every launch in front of the count (the iteration that detects) */
        const bool all_held = H.all_held();
        const bool fact_held = all_held && K.fact_held.fn, rhs_held = all_held && K.rhs_held.fn;
        /* ... and where the packed Hessian is stage-invariant too, the held factor launch reads one copy of it (hold bit 2) */
        const bool hess_held = fact_held && root->hold_hessian && H.hessian_verdict(s);
        GqpOpts Of = O;
        if (hess_held) Of.hold |= 4;
        prof.timed(1, s, top, [&] { launch_sweep(b, fact_held ? K.fact_held : K.fact, s, D, Of, 0); });
        if (fact_held) Hroot.fact_launches++;
        if (hess_held) Hroot.hess_launches++;
        if (fact_held && !top) Hroot.level_launches++;
        root->launches++;
        HIPCHK(hipMemcpyAsync(b->h_nact, D.n_active, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        H.stream_drained();
        const int nact = *b->h_nact;
        if (root->print_level > 1) printf("acados_amd: ipm iter %d level size %d active %d\n", it, b->B, nact);
        if (nact <= 0 || it > O.iter_max) break;
        if (use_perm && nact >= 1 && 6 * nact <= 5 * b->w16_slots)
        {
            if (!b->d_perm) { b->d_perm = dalloc<int>(b, b->Bp); b->d_perm_cnt = dalloc<int>(b, 1); }
            HIPCHK(hipMemsetAsync(b->d_perm_cnt, 0, sizeof(int), s));
            hipLaunchKernelGGL(gqp::k_active_perm, dim3((b->B + 255) / 256), dim3(256), 0, s, D, b->d_perm, b->d_perm_cnt);
            D.perm = b->d_perm;
            D.n_perm = nact;
            b->w16_slots = nact;
        }
        /* what this loop knows of the matrices goes with a hand-over (sub_batch_load: the slim gather) */
        const HeldDynamics *known = &H != &none ? &H : nullptr;
        /* (the tail rule measures the survivors against the ROOT's batch at every level: when the tail takes over, and with it every
         * output bit, does not depend on whether a level was made in between) */
        if (b->fam.lane() && root->tail_max > 0 && nact <= root->tail_max && (long) root->tail_div * nact <= root->B)
        {
            /* the last survivors of a one-instance-per-lane level: a wave that still has ONE active lane pays
             * the full per-wave latency of every sweep, so the tail continues one wave per instance */
            ocp_qp_gpu_batch *tail = compact_into(b, root, s, SUB_TAIL, known);
            root->n_tail_switches++;
            run_ipm(tail, root, prof, s, it);
            /* the family's own finalize first: the general one-instance-per-lane kernels refresh the multipliers
             * of the fixed variables in every factor sweep and their finalize relies on that, the wave-per-instance
             * kernels compute them once at the end */
            launch_whole(tail, pick_kernels(tail).final_, s, tail->D);
            root->launches++;
            compact_back(b, s, SUB_TAIL, it);
            break;
        }
        /* a dense level of the survivors: by size (compact_min, off by default), or -- compact_held -- where every tile of this
         * loop holds: the level then stays on the held entries (HeldDynamics::adopt) and its hand-over reads two stage slots */
        const bool held_level = root->compact_held && all_held && b->B >= root->compact_held_min;
        if ((b->B >= root->compact_min || held_level) && 2 * nact <= b->B)
        {
            ocp_qp_gpu_batch *level = compact_into(b, root, s, SUB_COMPACT, known);
            if (held_level)
            {
                level->held.adopt(level, level->B, root->hold_hessian && H.hess_known());
                hipLaunchKernelGGL(gqp::k_level_held, dim3(level->Bp / 64), dim3(64), 0, s, level->D, level->B);
            }
            root->n_compactions++;
            run_ipm(level, root, prof, s, it);
            compact_back(b, s, SUB_COMPACT, it);
            break;
        }
        GqpOpts Oa = O;
        Oa.hold = H.bits(true);
        prof.timed(2, s, top, [&] { launch_sweep(b, K.faff, s, D, Oa, 0); });
        H.after_detect(s, nact == b->B);
        const Sweep &k_rhs = rhs_held ? K.rhs_held : K.rhs;
        prof.timed(3, s, top, [&] { launch_sweep(b, k_rhs, s, D, O, 0); });
        prof.timed(4, s, top, [&] { launch_sweep(b, K.fcorr, s, D, Oc, 0); });
        root->launches += 3;
        if (O.cond_pred_corr)
        {
            launch_sweep(b, k_rhs, s, D, O, 1);
            launch_sweep(b, K.fcorr, s, D, Oc, 1);
            root->launches += 2;
        }
        if (rhs_held) Hroot.rhs_launches += O.cond_pred_corr ? 2 : 1;
        if (rhs_held && !top) Hroot.level_launches += O.cond_pred_corr ? 2 : 1;
        if (ext_update)
        {
            /* (behind the redo pair: an instance whose corrector collapsed gets its step length there) */
            const int blocks = D.ux.aos ? b->B : (b->B + GQP_UPD_THREADS - 1) / GQP_UPD_THREADS;
            hipLaunchKernelGGL(gqp::k_step_update, dim3(blocks), dim3(GQP_UPD_THREADS), 0, s, D, O, smap, b->nct_tot, b->ns2_tot);
            root->launches++;
        }
    }
    b->w16_slots = b->B; /* launches outside this loop (sensitivity passes) cover every instance again */
    H.end(s);
}

/*
 * Terminal polishing step (option "polish" = 1, opt-in; status and iteration counts of the solve are unchanged).  Behind the loop,
 * converged instances that still hold a BALANCED complementarity pair -- min(lam, t) > polish_ratio * max(lam, t) on a row that takes
 * part: the weakly active rows an IPM leaves at t = mu / lam*, the whole of the distance between its exit point and the solution
 *  -- run ONE more iteration of the same four sweeps (k_polish_select: iteration counter 0 against iter_max 1, exit
 * tolerances that cannot be met, statistics table off).  Near the solution a Mehrotra iteration is the affine step but for
 * sigma = (mu_aff / mu)^3 ~ 1e-9: mu falls by three orders and more.  The polished point must pass the exit test the solve was
 * run with; an instance whose does not gets its iterate back (k_polish_restore / k_polish_revert: counted in "polish_reverted").
 * Cost: one iteration + one factor sweep over the instances selected -- in the one-instance-per-lane family over every 64-instance
 * tile that holds one.  Measured: profiles/NOTES.md round 6.
 */
static void polish_pass(ocp_qp_gpu_batch *b, Prof &prof, hipStream_t s)
{
    b->n_polished = b->n_polish_reverted = 0;
    GqpDev &D = b->D;
    if (!b->d_pol_status)
    {
        b->d_pol_status = dalloc<int>(b, b->Bp); b->d_pol_iter = dalloc<int>(b, b->Bp); b->d_pol_flag = dalloc<int>(b, b->Bp);
        b->d_pol_cnt = dalloc<int>(b, 2);
        b->d_pol_sc = dalloc<double>(b, (size_t) 6 * b->Bp);
        b->pol_ux = garr<double>(b, D.ux.E); b->pol_sv = garr<double>(b, D.sv.E); b->pol_pi = garr<double>(b, D.pi.E);
        b->pol_lam = garr<double>(b, D.lam.E); b->pol_t = garr<double>(b, D.t.E);
    }
    const dim3 g64((b->B + 63) / 64), blk(64);
    HIPCHK(hipMemsetAsync(b->d_pol_cnt, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(gqp::k_polish_select, g64, blk, 0, s, D, side_map(b), b->nct_tot, b->polish_ratio, b->polish_min, b->d_pol_status, b->d_pol_iter, b->d_pol_sc,
                       b->d_pol_cnt);
    HIPCHK(hipMemcpyAsync(b->h_nact, b->d_pol_cnt, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int nsel = *b->h_nact;
    b->launches++;
    if (nsel <= 0)
    {
        hipLaunchKernelGGL(gqp::k_status_restore, g64, blk, 0, s, D, b->d_pol_status); /* (nothing changed; keeps the two paths alike) */
        return;
    }
    const struct { GArr src, dst; } cp[] = {{D.ux, b->pol_ux}, {D.sv, b->pol_sv}, {D.pi, b->pol_pi}, {D.lam, b->pol_lam}, {D.t, b->pol_t}};
    for (const auto &c : cp) HIPCHK(hipMemcpyAsync(c.dst.p, c.src.p, sizeof(double) * (size_t) c.src.E * b->Bp, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(D.n_active, b->h_nact, sizeof(int), hipMemcpyHostToDevice, s));
    const GqpOpts keep = b->O;
    const int keep_stat = D.stat_inst;
    b->O.tol_stat = b->O.tol_eq = b->O.tol_ineq = b->O.tol_comp = -1.0; /* the loop's exit test cannot pass: it ends at iter_max */
    b->O.iter_max = b->polish; /* option value = iterations of the pass (1 unless asked otherwise) */
    const GqpOpts Oeff = effective_opts(keep, b);
    b->O.tau_min = Oeff.tau_min; /* the barrier floor of the solve (derived from ITS tol_comp) */
    D.stat_inst = 0;             /* the statistics table keeps the solve's rows */
    run_ipm(b, b, prof, s, 0, true); /* (a root loop of its own: it detects held dynamics again and adds to the held launch counts) */
    b->O = keep;
    D.stat_inst = keep_stat;
    hipLaunchKernelGGL(gqp::k_polish_restore, g64, blk, 0, s, D, Oeff, b->d_pol_status, b->d_pol_iter, b->d_pol_sc, b->d_pol_flag, b->d_pol_cnt + 1);
    HIPCHK(hipMemcpyAsync(b->h_nact, b->d_pol_cnt + 1, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    b->launches++;
    b->n_polished = nsel;
    b->n_polish_reverted = *b->h_nact;
    if (b->n_polish_reverted > 0)
    {
        const int blocks = D.ux.aos ? b->B : (b->B + GQP_UPD_THREADS - 1) / GQP_UPD_THREADS;
        hipLaunchKernelGGL(gqp::k_polish_revert, dim3(blocks), dim3(GQP_UPD_THREADS), 0, s, D, b->d_pol_flag, b->pol_ux, b->pol_sv, b->pol_pi, b->pol_lam,
                           b->pol_t);
        b->launches++;
    }
}

/* Sub-batches (SubRole): creation, option hand-down, load and store exist once, here.  What differs per role stays with the callers:
 * how the list is built, n_active and the statistics rows of the levels, the order inside a sensitivity slice, the scalars a
 * ric_alg 0 solve reports */
/* arrays that define a QP instance and its iterate (everything else is recomputed) */
static const std::vector<GqpArrMember> g_state_arrays = {&GqpDev::BAt, &GqpDev::bvec, &GqpDev::RSQ, &GqpDev::rq, &GqpDev::dvec, &GqpDev::DCt,
                                                         &GqpDev::Zz, &GqpDev::ux, &GqpDev::sv, &GqpDev::pi, &GqpDev::lam, &GqpDev::t};
/* what comes back: the iterate of a solve, the directions of a seed pass, the factor at the solution */
static const std::vector<GqpArrMember> g_result_arrays = {&GqpDev::ux, &GqpDev::sv, &GqpDev::pi, &GqpDev::lam, &GqpDev::t};
static const std::vector<GqpArrMember> g_direction_arrays = {&GqpDev::dux, &GqpDev::dsv, &GqpDev::dpi, &GqpDev::dlam, &GqpDev::dt};
static const std::vector<GqpArrMember> g_factor_arrays = {&GqpDev::Lf, &GqpDev::lf};
enum SubStore { SUB_RESULT, SUB_DIRECTION, SUB_FACTOR };

/* room for n entries in the device list of a role */
static void sub_list_reserve(ocp_qp_gpu_batch *b, SubBatch &sb, int n)
{
    if (sb.d_list && n <= sb.list_cap) return;
    sb.list_cap = n;
    sb.d_list = dalloc<int>(b, n);
}

/* the sub-batch of `role` for `cap` instances of b: the very family of b (compaction) or the wave-per-instance family at the very
 * same padded dims (every other role).  Not being able to make one is a device failure like any other: the entry returns -1 */
static ocp_qp_gpu_batch *sub_batch_create(ocp_qp_gpu_batch *b, SubRole role, int cap)
{
    static const char *const names[SUB_ROLES] = {"compaction", "tail", "classical-Riccati", "sensitivity"};
    /* the family comes from the role: a compaction level runs its parent's, every other role the wave-per-instance family at the
     * parent's padded dims (choose_family) */
    ForcedChoice forced;
    forced.parent = &b->fam;
    forced.wpi = role != SUB_COMPACT;
    ocp_qp_gpu_batch *c = batch_create_shape(b->N, b->nx.data(), b->nu.data(), b->nbx.data(), b->nbu.data(), b->ng.data(), b->ns.data(), cap,
                                             b->device, forced);
    if (!c)
    {
        fprintf(stderr, "acados_amd: cannot create the %s sub-batch\n", names[role]);
        throw gqp_hip_failure{-1};
    }
    if (b->stream_priority) set_stream_priority(c, b->stream_priority);
    c->idxb = b->idxb; c->idxs_rev = b->idxs_rev; c->idxe = b->idxe; c->nbxe = b->nbxe;
    switch (role)
    {
    case SUB_COMPACT:
    case SUB_TAIL: /* a level sizes the sub-batches below it by the thresholds it was made under */
        c->compact_min = b->compact_min; c->tail_max = b->tail_max; c->tail_div = b->tail_div;
        break;
    case SUB_RIC0:
        c->ric_alg = 0;
        ric_configure(c);
        break;
    case SUB_SENS:
        c->tail_max = 0;
        c->ric_alg = b->ric_alg; /* the factor at the solution in the layout of the batch's Riccati recursion */
        ric_configure(c);
        break;
    default: break;
    }
    finalize_structure(c);
    if (role == SUB_SENS) c->sfix = garr<double>(c, (size_t) (c->N + 2) * (c->D.NX + c->D.NU));
    b->sub[role].c = c;
    b->sub[role].cap = cap;
    return c;
}

/* Run options of the solving batch for a sub-batch: per role what is handed down, no more */
static void sub_batch_opts(const ocp_qp_gpu_batch *from, ocp_qp_gpu_batch *c, SubRole role)
{
    /* every role: the IPM options and the exit scale of the soft classes (effective_opts).  For the two levels `from` is the ROOT of
     * the solve, not the level above.  The sensitivity sub-batch only factorises and sweeps: it needs nothing else */
    c->O = from->O;
    c->tol_comp_soft_scale = from->tol_comp_soft_scale;
    if (role != SUB_RIC0) return;
    /* the classical-Riccati sub-batch runs a whole solve of its own: polish pass, printing, profiling, the compaction and
     * single-launch thresholds, the hot-start clips (a wave-per-instance batch has no tail and holds no dynamics: not those) */
    c->polish = from->polish; c->polish_ratio = from->polish_ratio; c->polish_min = from->polish_min;
    c->print_level = from->print_level; c->profile = from->profile; c->compact_min = from->compact_min; c->solve_max = from->solve_max;
    c->t0_min = from->t0_min; c->lam0_min = from->lam0_min;
}

static void sub_copy(ocp_qp_gpu_batch *b, const SubBatch &sb, const std::vector<GqpArrMember> &arrays, int cnt, int dir, hipStream_t s)
{
    for (GqpArrMember m : arrays) copy_level(b->D.*m, sb.c->D.*m, sb.d_list, cnt, dir, s);
}

/* QP data, iterate, activity masks and loop scalars of the `cnt` listed instances of b into the first slots of the sub-batch.
 * Returns with the copies done: the caller may reuse its host list, the sub-batch may launch on a stream of its own */
/* Held data (`known`: the record of the IPM loop that hands over -- the root's, or a dense held level's; `root` takes the tally):
 * where that record says every tile holds its dynamics, the N stage slots of BAt are N copies of one block, and under a current
 * positive Hessian verdict so are those of RSQ at the stages 0 .. N-1 -- 50 of the 51 slots of the two arrays that make up three
 * quarters of an instance's state on C2.  Such an array goes through gqp::k_compact_held, which reads the slots N-1 and N and
 * writes them all: the same bits as the full copy.  No verdict is asked for the copy's sake; every other caller copies in full */
static void sub_batch_load(ocp_qp_gpu_batch *b, const SubBatch &sb, int cnt, hipStream_t s, const HeldDynamics *known = nullptr,
                           ocp_qp_gpu_batch *root = nullptr)
{
    ocp_qp_gpu_batch *c = sb.c;
    c->B = cnt; /* the sub-batch works on `cnt` slots of its capacity */
    c->D.B = cnt;
    c->held.data_written(true, true); /* (a dense held level takes its verdicts from the loop above it, after this: adopt()) */
    const auto slim_ok = [&](const GArr &big, const GArr &small) {
        return cnt > 0 && b->N >= 1 && big.p && small.p && big.E == small.E && big.E > 0 && big.E % (b->N + 1) == 0;
    };
    const bool slim_dyn = known && root && known->dyn_known() && slim_ok(b->D.BAt, c->D.BAt);
    const bool slim_hess = known && root && root->hold_hessian && known->hess_known() && slim_ok(b->D.RSQ, c->D.RSQ);
    for (GqpArrMember m : g_state_arrays)
    {
        const GArr &big = b->D.*m, &small = c->D.*m;
        if ((m == &GqpDev::BAt && slim_dyn) || (m == &GqpDev::RSQ && slim_hess))
        {
            /* (up to eight parts share the destination stages of a tile: 51 stage slots are written from one read) */
            const int chunks = (big.E / (b->N + 1) + 63) / 64, parts = std::min(b->N + 1, 8);
            GQP_LAUNCH_COOP(gqp::k_compact_held, dim3((cnt + 63) / 64, chunks * parts), dim3(64), 0, s, big, small, sb.d_list, cnt, b->N);
        }
        else copy_level(big, small, sb.d_list, cnt, 0, s);
    }
    if (slim_dyn) root->held.slim_dyn++;
    if (slim_hess) root->held.slim_hess++;
    copy_level(b->D.amask, c->D.amask, sb.d_list, cnt, 0, s);
    hipLaunchKernelGGL(gqp::k_compact_scalars, dim3((cnt + 63) / 64), dim3(64), 0, s, b->D, c->D, sb.d_list, cnt, 0);
    HIPCHK(hipStreamSynchronize(s));
}

/* ... and back: the iterate with the per-instance scalars of a solve, the directions of a seed pass, or the factor (not synchronised) */
static void sub_batch_store(ocp_qp_gpu_batch *b, const SubBatch &sb, int cnt, SubStore what, hipStream_t s)
{
    sub_copy(b, sb, what == SUB_RESULT ? g_result_arrays : what == SUB_DIRECTION ? g_direction_arrays : g_factor_arrays, cnt, 1, s);
    if (what == SUB_RESULT)
        hipLaunchKernelGGL(gqp::k_compact_scalars, dim3((cnt + 63) / 64), dim3(64), 0, s, b->D, sb.c->D, sb.d_list, cnt, 1);
}

static ocp_qp_gpu_batch *compact_into(ocp_qp_gpu_batch *b, ocp_qp_gpu_batch *root, hipStream_t s, SubRole role, const HeldDynamics *known)
{
    const bool tail = role == SUB_TAIL;
    SubBatch &sb = b->sub[role];
    /* sorted list of the still-iterating instances (sorted => the gather reads stay coalesced) */
    int *st = b->h_ints, *list = b->h_ints + b->Bp; /* pinned, owned by the level */
    HIPCHK(hipMemcpy(st, b->D.status, sizeof(int) * b->B, hipMemcpyDeviceToHost));
    int cnt = 0;
    for (int i = 0; i < b->B; i++) if (st[i] == GQP_RUNNING) list[cnt++] = i;
    /* capacities follow the level's CAPACITY (Bp), not its current count: a level is re-used by later solves with
     * more survivors (its B changes between solves) */
    sub_list_reserve(b, sb, std::max(cnt, (b->Bp + 1) / 2));
    if (sb.c && cnt > (tail ? sb.cap : sb.c->Bp))
    {
        /* more survivors than the sub-batch was sized for (tail_max raised, or a later solve of a re-used level) */
        ocp_qp_gpu_batch_destroy(sb.c);
        sb.c = nullptr;
    }
    if (!sb.c) sub_batch_create(b, role, tail ? std::max(cnt, std::min(b->tail_max, sb.list_cap)) : std::max(cnt, (b->Bp + 1) / 2));
    ocp_qp_gpu_batch *c = sb.c;
    HIPCHK(hipMemcpyAsync(sb.d_list, list, sizeof(int) * cnt, hipMemcpyHostToDevice, s));
    sub_batch_load(b, sb, cnt, s, known, root); /* (synchronises: `list` (host) must outlive the copy) */
    *c->h_nact = cnt;
    HIPCHK(hipMemcpyAsync(c->D.n_active, c->h_nact, sizeof(int), hipMemcpyHostToDevice, s));
    /* the level keeps its own statistics rows for its first slots; merged into the parent's table afterwards */
    sub_batch_opts(root, c, role);
    ensure_stat(c);
    HIPCHK(hipMemsetAsync(c->D.stat, 0, sizeof(double) * (size_t) c->stat_rows * GQP_STAT_COLS * c->stat_inst, s));
    return c;
}

static void compact_back(ocp_qp_gpu_batch *b, hipStream_t s, SubRole role, int it0)
{
    const SubBatch &sb = b->sub[role];
    ocp_qp_gpu_batch *c = sb.c;
    const int cnt = c->B;
    if (b->D.stat && c->D.stat)
        hipLaunchKernelGGL(gqp::k_stat_merge, dim3(1, std::max(1, std::min(b->stat_rows, c->stat_rows) - it0)), dim3(64), 0, s, b->D,
                           c->D, sb.d_list, cnt < 64 ? cnt : 64, it0);
    sub_batch_store(b, sb, cnt, SUB_RESULT, s);
}

/* behind a solve: iteration counts and statuses into h_ints; sets last_iters, returns the number of instances that failed */
static int solve_epilogue(ocp_qp_gpu_batch *b)
{
    int *itv = b->h_ints, *st = b->h_ints + b->Bp;
    HIPCHK(hipMemcpy(itv, b->D.iter, sizeof(int) * b->B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(st, b->D.status, sizeof(int) * b->B, hipMemcpyDeviceToHost));
    int mx = 0, bad = 0;
    for (int q = 0; q < b->B; q++) { mx = std::max(mx, itv[q]); bad += st[q] != 0; }
    b->last_iters = mx;
    return bad;
}

/*
 * FULL CONDENSING of any size (option "full_dense" = 1; FULL_CONDENSING_GPU_IPM past what one condensed stage of the stage-wise
 * families may carry): one workgroup per instance condenses every state but x0, runs the IPM on the dense problem and expands
 * (dense_kernels.hpp), multipliers of the equality-flagged rows included.  The batch is worked off in slices whose workspace stays
 * below 8 GiB (option "full_dense_slice": of that many instances); the family's own finalize kernel then sets the masked sides, as
 * after a stage-wise solve.
 */
static int dense_solve(ocp_qp_gpu_batch *b)
{
    hipStream_t s = b->stream;
    const GqpDev &D = b->D;
    if (!b->d_kd_rows)
    {
        std::vector<gqp::KdRow> rows;
        b->kd_unsupported = b->has_slack ? 1 : 0;
        for (int k = 0; k <= b->N; k++)
        {
            const GqpStage &S = b->st[k];
            const int nbg = S.nb + S.ng;
            if (S.ns > 0) b->kd_unsupported = 1;
            int sp = 0;
            for (int pv = 0; pv < 64; pv++)
                if ((S.bmask >> pv) & 1)
                {
                    const int fixed = (int) ((S.emask >> pv) & 1);
                    if (fixed && pv >= D.NU && k > 0) b->kd_unsupported = 1; /* a fixed state behind stage 0 is not a dense variable */
                    rows.push_back({k, pv, -1, S.o_ct + sp, S.o_ct + nbg + sp, sp, nbg + sp, fixed});
                    sp++;
                }
            for (int g = 0; g < S.ng; g++) rows.push_back({k, -1, S.o_g + g, S.o_ct + S.nb + g, S.o_ct + nbg + S.nb + g, S.nb + g, nbg + S.nb + g, 0});
        }
        if (b->kd_unsupported)
            fprintf(stderr, "acados_amd: full_dense: slacks and equality-flagged states behind stage 0 are not supported by the dense path (every "
                            "instance returns status 4); use the stage-wise solver (cond_N >= 1 blocks within the limits, or none)\n");
        gqp::KdDims &S = b->kd;
        const int K = b->N + 1, NX = D.NX, NU = D.NU, n = NX + NU;
        S.K = K; S.n = n; S.nvu = K * NU; S.nv = S.nvu + NX; S.R = (int) rows.size();
        size_t o = 0;
        auto take = [&](size_t cnt) { const size_t at = o; o += (cnt + 7) & ~(size_t) 7; return at; };
        S.oG = take((size_t) K * NX * S.nv); S.oc = take((size_t) K * NX); S.oH = take((size_t) K * n * n); S.og = take((size_t) K * n);
        S.orw = take((size_t) K * n); S.oM = take((size_t) S.nv * S.nv); S.orhs = take(S.nv); S.odv = take(S.nv); S.ov = take(S.nv);
        S.ow = take((size_t) K * n); S.odw = take((size_t) K * n); S.oP = take((size_t) NX * S.nv);
        S.W = o;
        b->d_kd_rows = dalloc<gqp::KdRow>(b, rows.size());
        if (!rows.empty()) HIPCHK(hipMemcpy(b->d_kd_rows, rows.data(), sizeof(gqp::KdRow) * rows.size(), hipMemcpyHostToDevice));
    }
    /* instances per launch: option "full_dense_slice", else what 8 GiB of workspace hold; the workspace follows a change */
    const size_t budget = (size_t) 8 << 30;
    const size_t fit = b->full_dense_slice > 0 ? (size_t) b->full_dense_slice : budget / (b->kd.W * sizeof(double));
    const int slice = (int) std::max<size_t>(1, std::min<size_t>((size_t) b->B, fit));
    if (slice != b->kd_slice)
    {
        if (b->d_kd_ws) dfree(b, b->d_kd_ws, sizeof(double) * (size_t) b->kd_slice * b->kd.W);
        b->kd_slice = slice;
        b->d_kd_ws = dalloc<double>(b, (size_t) b->kd_slice * b->kd.W);
    }
    const GqpOpts O = effective_opts(b->O, b);
    HIPCHK(hipEventRecord(b->ev0, s));
    for (int first = 0; first < b->B; first += b->kd_slice)
    {
        const int cnt = std::min(b->kd_slice, b->B - first);
        GQP_LAUNCH_COOP(gqp::kd_solve, dim3(cnt), dim3(GQP_KD_THREADS), 0, s, D, O, b->kd, (const gqp::KdRow *) b->d_kd_rows, b->d_kd_ws, first,
                        b->kd_unsupported);
    }
    b->launches = (b->B + b->kd_slice - 1) / b->kd_slice;
    if (!b->kd_unsupported)
    {
        launch_whole(b, pick_kernels(b).final_, s, D);
        b->launches++;
    }
    HIPCHK(hipEventRecord(b->ev1, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    b->time_tot = ms * 1e-3;
    b->time_xcond = 0.0;
    b->factor_stale = true;   /* Lf of the stage-wise sweeps does not belong to this solution: the sensitivity slots refactor */
    b->sens_open = false;
    return solve_epilogue(b);
}

static void refactor_at_solution(ocp_qp_gpu_batch *b);

/*
 * ric_alg 0 on a one-instance-per-lane batch: the classical sweeps exist in the wave-per-instance family only.  The whole
 * batch (QP data, iterate, loop scalars) is copied into sub[SUB_RIC0] -- that family at the same padded dims, the conversion of
 * the tail switch --, solved there, and the iterate, the factor at the solution and the per-instance results come back.
 */
static ocp_qp_gpu_batch *ric0_copy_in(ocp_qp_gpu_batch *b)
{
    SubBatch &sb = b->sub[SUB_RIC0];
    if (!sb.c)
    {
        sub_batch_create(b, SUB_RIC0, b->B);
        std::vector<int> list(b->B); /* 0 .. B-1: the whole batch goes */
        for (int i = 0; i < b->B; i++) list[i] = i;
        sub_list_reserve(b, sb, b->Bp);
        HIPCHK(hipMemcpy(sb.d_list, list.data(), sizeof(int) * b->B, hipMemcpyHostToDevice));
    }
    sub_batch_opts(b, sb.c, SUB_RIC0);
    sub_batch_load(b, sb, b->B, b->stream); /* (synchronises: the sub-batch works on its own stream) */
    return sb.c;
}

/* the factor of the classical-Riccati sub-batch (classical layout) into the parent's Lf / lf */
static void ric0_factor_back(ocp_qp_gpu_batch *b)
{
    sub_batch_store(b, b->sub[SUB_RIC0], b->B, SUB_FACTOR, b->stream);
    HIPCHK(hipStreamSynchronize(b->stream));
    b->factor_stale = false;
}

/* the classical factor at the current iterate of a one-instance-per-lane batch (ric_alg 0): its own kernels only have the
 * square-root layout, which the getters would read as the classical one */
static void ric0_refactor(ocp_qp_gpu_batch *b)
{
    refactor_at_solution(ric0_copy_in(b));
    ric0_factor_back(b);
}

static int ric0_solve(ocp_qp_gpu_batch *b)
{
    ocp_qp_gpu_batch *c = ric0_copy_in(b);
    const int bad = ocp_qp_gpu_batch_solve(c);
    if (bad < 0) return bad;
    if (c->factor_stale) refactor_at_solution(c);
    sub_batch_store(b, b->sub[SUB_RIC0], b->B, SUB_RESULT, b->stream);
    ric0_factor_back(b);
    b->time_tot = c->time_tot; b->time_xcond = 0.0;
    b->last_iters = c->last_iters; b->launches = c->launches;
    b->n_compactions = c->n_compactions; b->n_tail_switches = 0; b->n_single_launch = c->n_single_launch;
    b->n_polished = c->n_polished; b->n_polish_reverted = c->n_polish_reverted;
    b->sens_open = false;
    return bad;
}

int ocp_qp_gpu_batch_solve(ocp_qp_gpu_batch *b)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    if (b->full_dense) return dense_solve(b);
    if (b->cond_N > 0 && b->cond_N < b->N)
    {
        if (b->pcond_state == 0) pcond_setup(b);
        if (b->pcond_state == 1) return pcond_solve(b, b->lhs_ready ? 2 : 3);
    }
    if (b->ric_alg == 0 && b->fam.lane()) return ric0_solve(b);
    b->time_xcond = 0.0;
    ensure_stat(b);
    const KernelSet *ks = b->fam.ks();
    GqpDev D = b->D;
    GqpOpts O = effective_opts(b->O, b);
    const dim3 grid((b->B + 63) / 64), block(64);
    hipStream_t s = b->stream;
    b->launches = 0;
    b->n_compactions = 0;
    b->n_tail_switches = 0;
    b->n_single_launch = 0;
    b->held.tiles_invariant = b->held.rhs_launches = b->held.fact_launches = b->held.hess_launches = b->held.hess_detects = b->held.detects = 0;
    b->held.level_launches = b->held.slim_dyn = b->held.slim_hess = 0;
    /* kernel classes: 0 init, 1 back_fact, 2 fwd_aff, 3 back_rhs, 4 fwd_corr, 5 finalize */
    b->prof_cls.clear();
    Prof prof;
    prof.root = b;

    HIPCHK(hipEventRecord(b->ev0, s));
    *b->h_nact = b->B;
    HIPCHK(hipMemcpyAsync(D.n_active, b->h_nact, sizeof(int), hipMemcpyHostToDevice, s));
    if (D.stat) HIPCHK(hipMemsetAsync(D.stat, 0, sizeof(double) * (size_t) b->stat_rows * GQP_STAT_COLS * b->stat_inst, s));
    if (O.warm_start < 2)
    {
        prof.timed(0, s, true, [&] { launch_whole(b, ks->init, s, D, O); });
        b->launches++;
    }
    else
    {
        /* hot start: keep (ux, pi, lam, t) as they are in HBM; loop state reset as a cold start leaves it */
        const double clip = O.warm_start == 2 ? 0.1 : 0.0;
        hipLaunchKernelGGL(gqp::k_hot_start, grid, block, 0, s, D, std::max(clip, b->t0_min), std::max(clip, b->lam0_min));
        b->launches++;
    }
    HIPCHK(hipMemsetAsync(D.apend, 0, sizeof(double) * (size_t) b->Bp, s)); /* no step pending (a solve always ends behind a factor sweep; belt and braces) */
    run_ipm(b, b, prof, s, 0);
    b->n_polished = b->n_polish_reverted = 0;
    if (b->polish) polish_pass(b, prof, s);
    b->factor_stale = b->n_tail_switches + b->n_compactions > 0;
    b->sens_open = false;
    launch_whole(b, pick_kernels(b).final_, s, D);
    b->launches++;
    HIPCHK(hipEventRecord(b->ev1, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    b->time_tot = ms * 1e-3;
    for (size_t q = 0; q < b->prof_cls.size(); q++)
    {
        float pm = 0.f;
        HIPCHK(hipEventElapsedTime(&pm, b->prof_ev[2 * q], b->prof_ev[2 * q + 1]));
        b->prof_ms[b->prof_cls[q]] += pm;
        b->prof_cnt[b->prof_cls[q]]++;
    }
    return solve_epilogue(b);
}
catch (const gqp_hip_failure &) { return -1; }

/* One factor sweep at the final iterate with every instance awake: Lf / lf of the whole batch belong to the
 * solution afterwards (after a tail switch the root's factors of the handed-over instances are older).  Statuses
 * are restored. */
static void refactor_at_solution(ocp_qp_gpu_batch *b)
{
    if (b->ric_alg == 0 && b->fam.lane()) { ric0_refactor(b); return; }
    hipStream_t s = b->stream;
    const dim3 g64((b->B + 63) / 64), blk(64);
    if (!b->d_saved_status) b->d_saved_status = dalloc<int>(b, b->Bp);
    GqpOpts O = effective_opts(b->O, b);
    hipLaunchKernelGGL(gqp::k_sens_prep, g64, blk, 0, s, b->D, O.tau_min, b->d_saved_status);
    launch_sweep(b, pick_kernels(b).fact, s, b->D, O, 0);
    hipLaunchKernelGGL(gqp::k_status_restore, g64, blk, 0, s, b->D, b->d_saved_status);
    HIPCHK(hipStreamSynchronize(s));
    b->factor_stale = false;
}

static int sens_begin(ocp_qp_gpu_batch *b)
{
    if (b->sens_open) return 0;
    /* after a partially condensed solve the expanded solution sits in this (full-space) batch: the factorisation at
     * the solution and the seed sweeps run here, the condensed sub-batch is not involved */
    /* a one-instance-per-lane batch hands slices of itself to a wave-per-instance sub-batch in sens_solve */
    if (!b->fam.lane()) refactor_at_solution(b);
    const GqpDev &D = b->D;
    const int n = D.NX + D.NU;
    if (!b->sfix.p) b->sfix = garr<double>(b, (size_t) (b->N + 2) * n);
    const GArr z[] = {D.rg, D.rgs, D.rb, D.rd, b->sfix};
    for (const GArr &a : z) HIPCHK(hipMemsetAsync(a.p, 0, sizeof(double) * (size_t) a.E * b->Bp, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->sens_open = true;
    return 0;
}

int ocp_qp_gpu_batch_sens_set(ocp_qp_gpu_batch *b, const char *f, int k, const double *data)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    if (strncmp(f, "seed_", 5) || k < 0 || k > b->N)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_sens_set: unknown seed %s (stage %d)\n", f, k);
        return -1;
    }
    if (sens_begin(b)) return -1;
    FieldRef s;
    const int len = field_resolve(b, field_row(f + 5), k, USE_SEED, s);
    if (len < 0)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_sens_set: %s is not a seed of this stage (seeds: seed_q seed_r seed_zl seed_zu seed_b "
                        "seed_lbu seed_ubu seed_lbx seed_ubx seed_lg seed_ug seed_lls seed_lus)\n", f);
        return -1;
    }
    if (len == 0) return 0;
    std::vector<double> h((size_t) b->B * len);
    for (size_t e = 0; e < h.size(); e++) h[e] = s.row->sign * data[e];
    const double *src = stage_in(b, h.data(), h.size(), 0);
    int *dm = upload_map(b, s.map);
    hipLaunchKernelGGL(gqp::k_scatter, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, src, b->B, len, dm, arr_of(b, s.arr));
    HIPCHK(hipStreamSynchronize(b->stream));
    /* equality-flagged bounds: the seed of the bound is the derivative of the variable itself */
    if (std::any_of(s.map2.begin(), s.map2.end(), [](int m) { return m >= 0; }))
    {
        src = stage_in(b, data, (size_t) b->B * len, 0);
        dm = upload_map(b, s.map2);
        hipLaunchKernelGGL(gqp::k_scatter, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, src, b->B, len, dm, arr_of(b, s.arr2));
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* the seed pass on a wave-per-instance / sixteen-lanes batch whose factor belongs to the solution */
static void sens_pass(ocp_qp_gpu_batch *b, hipStream_t s)
{
    const dim3 g64((b->B + 63) / 64), blk(64);
    GqpOpts O = effective_opts(b->O, b);
    const IpmKernels K = pick_kernels(b);
    hipLaunchKernelGGL(gqp::k_sens_fixed, g64, blk, 0, s, b->D, b->sfix, 0);
    hipLaunchKernelGGL(gqp::k_sens_prep, g64, blk, 0, s, b->D, O.tau_min, b->d_saved_status);
    launch_sweep(b, K.rhs, s, b->D, O, 2);
    launch_sweep(b, K.fcorr, s, b->D, O, 2);
    hipLaunchKernelGGL(gqp::k_sens_fixed, g64, blk, 0, s, b->D, b->sfix, 1);
    hipLaunchKernelGGL(gqp::k_status_restore, g64, blk, 0, s, b->D, b->d_saved_status);
}

/*
 * One-instance-per-lane batches: the direction-only sweeps exist in the wave-per-instance families only, so the
 * batch is walked in slices of at most GQP_SENS_SLICE instances; a slice (QP data, solution, seeds) is copied into a
 * sub-batch of the wave-per-instance family at the same padded dims (the tail switch's conversion), factorised there
 * at the solution, swept, and the directions are copied back.  ~3 extra passes over the data per call.
 */
#define GQP_SENS_SLICE 16384
static void sens_solve_sliced(ocp_qp_gpu_batch *b)
{
    hipStream_t s = b->stream;
    SubBatch &sb = b->sub[SUB_SENS];
    if (!sb.c)
    {
        const char *env = getenv("ACADOS_AMD_SENS_SLICE"); /* the slice size is fixed at first use */
        sub_batch_create(b, SUB_SENS, std::min(b->B, env && atoi(env) > 0 ? atoi(env) : GQP_SENS_SLICE));
        sub_list_reserve(b, sb, sb.cap);
    }
    ocp_qp_gpu_batch *c = sb.c;
    const int cap = sb.cap;
    sub_batch_opts(b, c, SUB_SENS);
    std::vector<int> list(cap);
    for (int i0 = 0; i0 < b->B; i0 += cap)
    {
        const int cnt = std::min(cap, b->B - i0);
        for (int j = 0; j < cnt; j++) list[j] = i0 + j;
        HIPCHK(hipMemcpyAsync(sb.d_list, list.data(), sizeof(int) * cnt, hipMemcpyHostToDevice, s));
        sub_batch_load(b, sb, cnt, s); /* (synchronises: the sub-batch works on its own stream) */
        refactor_at_solution(c);       /* writes the residual arrays: the seeds go in afterwards */
        for (GqpArrMember m : {&GqpDev::rg, &GqpDev::rgs, &GqpDev::rb, &GqpDev::rd}) copy_level(b->D.*m, c->D.*m, sb.d_list, cnt, 0, s);
        copy_level(b->sfix, c->sfix, sb.d_list, cnt, 0, s);
        HIPCHK(hipStreamSynchronize(s));
        sens_pass(c, c->stream);
        HIPCHK(hipStreamSynchronize(c->stream));
        sub_batch_store(b, sb, cnt, SUB_DIRECTION, s);
        HIPCHK(hipStreamSynchronize(s));
    }
}

int ocp_qp_gpu_batch_sens_solve(ocp_qp_gpu_batch *b)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    if (sens_begin(b)) return -1; /* no seed set: all-zero seeds, zero sensitivities */
    if (b->fam.lane())
    {
        sens_solve_sliced(b);
        HIPCHK(hipGetLastError());
        b->sens_open = false;
        return 0;
    }
    sens_pass(b, b->stream);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipGetLastError());
    b->sens_open = false;
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_get(ocp_qp_gpu_batch *b, const char *f, int k, double *data, int is_device)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    if (b->factor_stale && !strncmp(f, "ric_", 4)) refactor_at_solution(b);
    if (!strncmp(f, "res_", 4) && !b->R.nrm) { fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_get: %s before ocp_qp_gpu_batch_res_compute\n", f); return -1; }
    /* sensitivities: the direction arrays of the last ocp_qp_gpu_batch_sens_solve */
    const bool is_sens = !strncmp(f, "sens_", 5);
    FieldRef s;
    const int len = field_resolve(b, field_row(is_sens ? f + 5 : f), k, is_sens ? USE_SENS : USE_DATA, s);
    if (len < 0)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_get: field %s not available at stage %d\n", f, k);
        return -1;
    }
    if (len == 0) return 0;
    if (s.row->flags & F_SYM) mirror_lower(s.map, FieldCtx(b, k).nvar(s.row->cls)); /* the reader gets the whole matrix */
    const size_t cnt = (size_t) b->B * len;
    double *dst = stage_out(b, data, cnt, is_device);
    int *dm = upload_map(b, s.map);
    if (s.mask()) /* activity of the sides as 1.0 / 0.0 (equality-flagged rows: 1.0) */
        hipLaunchKernelGGL(gqp::k_getmask, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, dst, b->B, len, dm, b->D.amask, k, b->fam.AW);
    else
        hipLaunchKernelGGL(gqp::k_gather, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, dst, b->B, len, dm, arr_of(b, s.arr));
    stage_out_done(b, data, cnt, is_device);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* KKT residuals of the QP data and the iterate (ux, pi, lam, t) that are in HBM right now -- whoever put them there
 * (the solver, a warm-start set, an expansion): ocp_qp_res_compute + ocp_qp_res_compute_nrm_inf of
 * acados/ocp_qp/ocp_qp_common.c:559-667 for the whole batch in one launch.  Independent of the IPM sweeps. */
int ocp_qp_gpu_batch_res_compute(ocp_qp_gpu_batch *b)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    const GqpDev &D = b->D;
    if (!b->R.nrm)
    {
        const int n = D.NX + D.NU;
        b->R.g = garr<double>(b, (size_t) (b->N + 1) * n);
        b->R.gs = garr<double>(b, (size_t) b->ns2_tot);
        b->R.b = garr<double>(b, (size_t) (b->N + 1) * D.NX);
        b->R.d = garr<double>(b, (size_t) b->nct_tot + 16);
        b->R.m = garr<double>(b, (size_t) b->nct_tot + 16);
        b->R.nrm = dalloc<double>(b, 4 * (size_t) b->Bp);
        b->R.Bp = b->Bp;
    }
    hipLaunchKernelGGL(gqp::k_res_compute, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, b->D, b->R);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipGetLastError());
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* res[i * 4 + q]: inf-norms of res_g, res_b, res_d, res_m of instance i (ocp_qp_res_compute_nrm_inf) */
int ocp_qp_gpu_batch_res_nrm_inf(ocp_qp_gpu_batch *b, double *res)
try
{
    if (!b->R.nrm && ocp_qp_gpu_batch_res_compute(b) != 0) return -1;
    std::vector<double> h(4 * (size_t) b->Bp);
    HIPCHK(hipMemcpy(h.data(), b->R.nrm, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < b->B; i++)
        for (int q = 0; q < 4; q++) res[(size_t) i * 4 + q] = h[(size_t) q * b->Bp + i];
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_get_info(ocp_qp_gpu_batch *b, const char *f, void *data)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    const GqpDev &D = b->D;
    const size_t B = b->B;
    if (!strcmp(f, "status")) { HIPCHK(hipMemcpy(data, D.status, sizeof(int) * B, hipMemcpyDeviceToHost)); return 0; }
    if (!strcmp(f, "iter")) { HIPCHK(hipMemcpy(data, D.iter, sizeof(int) * B, hipMemcpyDeviceToHost)); return 0; }
    const char *names[4] = {"res_stat", "res_eq", "res_ineq", "res_comp"};
    for (int q = 0; q < 4; q++)
        if (!strcmp(f, names[q]))
        {
            HIPCHK(hipMemcpy(data, D.res + (size_t) q * b->Bp, sizeof(double) * B, hipMemcpyDeviceToHost));
            return 0;
        }
    if (!strcmp(f, "mu")) { HIPCHK(hipMemcpy(data, D.mu, sizeof(double) * B, hipMemcpyDeviceToHost)); return 0; }
    if (!strcmp(f, "obj")) { HIPCHK(hipMemcpy(data, D.obj, sizeof(double) * B, hipMemcpyDeviceToHost)); return 0; }
    fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_get_info: unknown field %s\n", f);
    return -1;
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_get_stat(ocp_qp_gpu_batch *b, int inst, double *stat, int max_rows)
try
{
    HIPCHK(hipSetDevice(b->device));
    if (b->pcond_state == 1 && b->child) return ocp_qp_gpu_batch_get_stat(b->child, inst, stat, max_rows);
    if (b->ric_alg == 0 && b->fam.lane() && b->sub[SUB_RIC0].c) return ocp_qp_gpu_batch_get_stat(b->sub[SUB_RIC0].c, inst, stat, max_rows);
    if (!b->D.stat || inst < 0 || inst >= b->stat_inst) return -1;
    const int rows = std::min(max_rows, b->stat_rows);
    std::vector<double> h((size_t) b->stat_rows * GQP_STAT_COLS * b->stat_inst);
    HIPCHK(hipMemcpy(h.data(), b->D.stat, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < GQP_STAT_COLS; c++)
            stat[r * GQP_STAT_COLS + c] = h[((size_t) r * GQP_STAT_COLS + c) * b->stat_inst + inst];
    return rows;
}
catch (const gqp_hip_failure &) { return -1; }

double ocp_qp_gpu_batch_get_scalar(ocp_qp_gpu_batch *b, const char *f)
try
{
    if (!strcmp(f, "time_tot")) return b->time_tot;
    if (!strcmp(f, "time_pack")) { double t = b->time_pack; b->time_pack = 0.0; return t; }
    if (!strcmp(f, "iter_max_batch")) return (double) b->last_iters;
    if (!strcmp(f, "launches")) return (double) b->launches;
    if (!strcmp(f, "time_xcond")) return b->time_xcond;
    if (!strcmp(f, "compactions")) return (double) b->n_compactions;
    if (!strcmp(f, "w16_tiles")) return (double) b->fam.tiles;
    if (!strcmp(f, "tail_switches")) return (double) b->n_tail_switches;
    if (!strcmp(f, "tiles_invariant")) return (double) b->held.tiles_invariant;
    if (!strcmp(f, "rhs_held_launches")) return (double) b->held.rhs_launches;
    if (!strcmp(f, "fact_held_launches")) return (double) b->held.fact_launches;
    if (!strcmp(f, "hess_held_launches")) return (double) b->held.hess_launches;
    if (!strcmp(f, "hess_detector_runs")) return (double) b->held.hess_detects;
    if (!strcmp(f, "detecting_sweeps")) return (double) b->held.detects;
    if (!strcmp(f, "level_held_launches")) return (double) b->held.level_launches;
    if (!strcmp(f, "slim_dyn_copies")) return (double) b->held.slim_dyn;
    if (!strcmp(f, "slim_hess_copies")) return (double) b->held.slim_hess;
    if (!strcmp(f, "single_launch_solves")) return (double) b->n_single_launch;
    if (!strcmp(f, "cond_N_active")) return b->pcond_state == 1 ? (double) b->child->N : (double) b->N;
    if (!strcmp(f, "tol_comp_soft_scale")) return b->tol_comp_soft_scale;
    if (!strcmp(f, "polish")) return b->polish;
    if (!strcmp(f, "full_dense")) return b->full_dense;
    if (!strcmp(f, "dense_columns")) return b->kd.nv;
    if (!strcmp(f, "dense_slice")) return b->kd_slice;
    if (!strcmp(f, "dense_workspace_bytes")) return (double) b->kd.W * 8.0 * b->kd_slice;
    if (!strcmp(f, "polished")) return b->child && b->pcond_state == 1 && b->cond_N > 0 && b->cond_N < b->N ? b->child->n_polished : b->n_polished;
    if (!strcmp(f, "polish_reverted")) return b->child && b->pcond_state == 1 && b->cond_N > 0 && b->cond_N < b->N ? b->child->n_polish_reverted : b->n_polish_reverted;
    if (!strcmp(f, "tol_comp_effective")) { finalize_structure(b); return effective_opts(b->O, b).tol_comp; }
    /* which condensing / expansion kernels serve the batch: 2 sixteen lanes per block, 1 one instance per lane, 0 one wave
     * per instance (meaningful once partial condensing is active) */
    if (!strcmp(f, "pcond_kernel")) return b->pcond_state != 1 ? -1.0 : (b->pcz && b->pc_rt && b->fam.AW <= 1 && b->child->fam.AW <= 1) ? (b->pcz_mfma ? 3.0 : 2.0) : b->pc_rt ? 0.0 : 1.0;
    if (!strcmp(f, "pexpand_kernel")) return b->pcond_state != 1 ? -1.0 : (!b->pc_rt || b->pc_lane_expand) ? 1.0 : 0.0;
    {
        /* accumulated per-kernel-class event times (ms) and launch counts since the last reset */
        const char *cls[6] = {"init", "back_fact", "fwd_aff", "back_rhs", "fwd_corr", "finalize"};
        for (int q = 0; q < 6; q++)
        {
            char nm[64];
            snprintf(nm, sizeof(nm), "prof_ms_%s", cls[q]);
            if (!strcmp(f, nm)) return b->prof_ms[q];
            snprintf(nm, sizeof(nm), "prof_cnt_%s", cls[q]);
            if (!strcmp(f, nm)) return (double) b->prof_cnt[q];
        }
        if (!strcmp(f, "prof_reset"))
        {
            for (int q = 0; q < 6; q++) { b->prof_ms[q] = 0.0; b->prof_cnt[q] = 0; }
            return 0.0;
        }
    }
    fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_get_scalar: unknown field %s\n", f);
    return -1.0;
}
catch (const gqp_hip_failure &) { return NAN; } /* "tol_comp_effective" finalises the structure on the device */

int ocp_qp_gpu_batch_condense_lhs(ocp_qp_gpu_batch *b)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    b->lhs_ready = false;
    if (!(b->cond_N > 0 && b->cond_N < b->N)) return 0;
    if (b->pcond_state == 0) pcond_setup(b);
    if (b->pcond_state != 1) return 0;
    b->pmap.mode = 1;
    pcond_launch(b, false);
    HIPCHK(hipStreamSynchronize(b->stream));
    b->lhs_ready = true;
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* condensing-only boundary (interfaces/acados_c/condensing_interface.h:73-75): the condensed QP as an object of its
 * own, and the expansion of a solution of it */
ocp_qp_gpu_batch *ocp_qp_gpu_batch_condense(ocp_qp_gpu_batch *b)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    if (!(b->cond_N > 0 && b->cond_N < b->N)) return nullptr;
    if (b->pcond_state == 0) pcond_setup(b);
    if (b->pcond_state != 1) return nullptr;
    b->pmap.mode = 3;
    pcond_launch(b, false);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipGetLastError());
    b->lhs_ready = false;
    return b->child;
}
catch (const gqp_hip_failure &) { return nullptr; }

/* vector part alone (gbar, bbar, bounds) on top of a resident matrix part: the `condense_rhs` slot of
 * ocp_qp_xcond_config (ocp_qp_partial_condensing.c:602-630); returns the condensed batch like _condense */
ocp_qp_gpu_batch *ocp_qp_gpu_batch_condense_rhs(ocp_qp_gpu_batch *b)
try
{
    HIPCHK(hipSetDevice(b->device));
    finalize_structure(b);
    if (b->pcond_state != 1 || !b->child) return ocp_qp_gpu_batch_condense(b); /* no lhs yet: everything */
    b->pmap.mode = 2;
    pcond_launch(b, false);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipGetLastError());
    return b->child;
}
catch (const gqp_hip_failure &) { return nullptr; }

/* the current iterate of `b` restated in the condensed variables, written into the condensed batch: the
 * `condense_qp_out` slot (ocp_qp_partial_condensing.c:559-571) */
int ocp_qp_gpu_batch_condense_sol(ocp_qp_gpu_batch *b)
try
{
    HIPCHK(hipSetDevice(b->device));
    if (b->pcond_state != 1 || !b->child) return -1;
    hipLaunchKernelGGL(gqp::k_pcond_sol, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, b->D, b->child->D, b->pmap);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipGetLastError());
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* the condensed batch currently owned by `b` (after _condense / _condense_lhs), or NULL */
ocp_qp_gpu_batch *ocp_qp_gpu_batch_condensed(ocp_qp_gpu_batch *b) { return b->pcond_state == 1 ? b->child : nullptr; }

int ocp_qp_gpu_batch_expand(ocp_qp_gpu_batch *b)
try
{
    HIPCHK(hipSetDevice(b->device));
    if (b->pcond_state != 1 || !b->child) return -1;
    HIPCHK(hipStreamSynchronize(b->child->stream));
    pcond_launch(b, true);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipGetLastError());
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_get_dims(ocp_qp_gpu_batch *b, const char *f, int *out)
{
    const std::vector<int> *v = nullptr;
    if (!strcmp(f, "N")) { out[0] = b->N; return 0; }
    if (!strcmp(f, "n_batch")) { out[0] = b->B; return 0; }
    if (!strcmp(f, "nx")) v = &b->nx; else if (!strcmp(f, "nu")) v = &b->nu; else if (!strcmp(f, "nbx")) v = &b->nbx;
    else if (!strcmp(f, "nbu")) v = &b->nbu; else if (!strcmp(f, "nb")) v = &b->nb; else if (!strcmp(f, "ng")) v = &b->ng;
    else if (!strcmp(f, "ns")) v = &b->ns; else if (!strcmp(f, "nbxe")) v = &b->nbxe;
    if (!v) { fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_get_dims: unknown field %s\n", f); return -1; }
    for (int k = 0; k <= b->N; k++) out[k] = (*v)[k];
    return 0;
}

int ocp_qp_gpu_batch_get_int(ocp_qp_gpu_batch *b, const char *f, int k, int *out)
{
    if (k < 0 || k > b->N) return -1;
    const std::vector<int> *v = nullptr;
    if (!strcmp(f, "ric_alg")) { out[0] = b->ric_alg; return 1; } /* 0: Lf / lf hold the classical layout (ric_L, ric_l) */
    if (!strcmp(f, "idxb")) v = &b->idxb[k]; else if (!strcmp(f, "idxs_rev")) v = &b->idxs_rev[k]; else if (!strcmp(f, "idxe")) v = &b->idxe[k];
    if (!v) { fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_get_int: unknown field %s\n", f); return -1; }
    for (size_t e = 0; e < v->size(); e++) out[e] = (*v)[e];
    return (int) v->size();
}

int ocp_qp_gpu_batch_condense_rhs_and_solve(ocp_qp_gpu_batch *b)
try
{
    const int bad = ocp_qp_gpu_batch_solve(b); /* uses mode 2 when the lhs is in place */
    b->lhs_ready = false;
    return bad;
}
catch (const gqp_hip_failure &) { return -1; }


/* ---- bulk pack / unpack ---- */
static const char *const k_bulk_in_fields[] = {"A", "B", "b", "Q", "S", "R", "q", "r", "lbu", "ubu", "lbx", "ubx", "lg", "ug",
                                               "C", "D", "Zl", "Zu", "zl", "zu", "lls", "lus", "lbu_mask", "ubu_mask",
                                               "lbx_mask", "ubx_mask", "lg_mask", "ug_mask", "lls_mask", "lus_mask"};
static const char *const k_bulk_out_fields[] = {"u", "x", "sl", "su", "pi", "lam", "t"};
/* the VECTOR part of the input blob (which = 2): what changes between the two halves of an RTI step -- gradient, dynamics offset,
 * bounds, masks (ocp_nlp_common.c:3119-3138 writes exactly these between condense_lhs and condense_rhs_and_solve); 12.6 KB per
 * C2-shaped QP against 85 KB for the whole blob */
static const char *const k_bulk_vec_fields[] = {"b", "q", "r", "lbu", "ubu", "lbx", "ubx", "lg", "ug", "zl", "zu", "lls", "lus", "lbu_mask", "ubu_mask",
                                                "lbx_mask", "ubx_mask", "lg_mask", "ug_mask", "lls_mask", "lus_mask"};
/* every seed of every instance (the batched eval_forw_sens / eval_adj_sens of the acados-side adapter; callers
 * interfaces/acados_template/acados_template/c_templates_tera/acados_solver.in.c:3292-3337) */
static const char *const k_seed_fields[] = {"r", "q", "zl", "zu", "b", "lbu", "lbx", "lg", "ubu", "ubx", "ug", "lls", "lus"};

/* The kinds of blob.  A new kind is a row here (+ its BlobKind): the field list in blob order (names of k_fields), the prefix its
 * segment names carry in the offset queries with the use of the fields that goes with it, and whether it is READ through a table
 * pair of its own (d_arr_g / d_elem_g; else through the pair it is written by).  What one blob entry refers to is the field's row
 * of k_fields (field_resolve), applied to the fields of the walk (blob_fields): a mask field is a bit segment of the activity words
 * (k_bulk_masks / k_bulk_masks_get), a kind that lists A / B or Q / R / S leaves no stored held verdict standing when it is
 * scattered (BulkMap::writes_dyn / writes_hess) */
struct BlobDesc
{
    const char *const *fields;
    int nf;
    const char *prefix;
    FieldUse use;
    bool read_map;
};
#define GQP_BLOB(fields, prefix, use, read_map) {fields, (int) (sizeof(fields) / sizeof(fields[0])), prefix, use, read_map}
static const BlobDesc k_blobs[BLOB_KINDS] = {
    /* BLOB_IN   */ GQP_BLOB(k_bulk_in_fields, "", USE_DATA, true),
    /* BLOB_OUT  */ GQP_BLOB(k_bulk_out_fields, "", USE_DATA, false),
    /* BLOB_VEC  */ GQP_BLOB(k_bulk_vec_fields, "", USE_DATA, false),
    /* BLOB_SEED */ GQP_BLOB(k_seed_fields, "seed_", USE_SEED, false),
};

/* the public integers: `output` of _bulk_len / _bulk_offset is 0 for the input blob, 2 for its vector part and anything else for
 * the output blob; `which` of the gather entries (has_out = false) is 2 for the vector part and anything else for the input blob */
static BlobKind blob_kind(int v, bool has_out = true)
{
    if (v == 2) return BLOB_VEC;
    return v && has_out ? BLOB_OUT : BLOB_IN;
}

/* a segment of the field s, its entries referring to element m[e] of `slot` (m[e] < 0: to nothing) */
static void blob_segment_add(BulkMap &M, const std::string &name, const FieldRef &s, int slot, const std::vector<int> &m)
{
    M.fields.push_back(name); M.seg_row.push_back((int) (s.row - k_fields)); M.seg_stage.push_back(s.k);
    M.seg_off.push_back((int) M.arr.size()); M.seg_len.push_back(s.len);
    for (int el : m) { M.arr.push_back(el >= 0 ? slot : -1); M.elem.push_back(el >= 0 ? el : 0); }
}

/* the layout of every kind: stage-major, the kind's field order, fields of length 0 at a stage skipped */
static void blob_fields(ocp_qp_gpu_batch *b, const BlobDesc &K, const std::function<void(const FieldRef &)> &visit)
{
    std::vector<const FieldRow *> rows;
    for (int fi = 0; fi < K.nf; fi++)
    {
        rows.push_back(field_row(K.fields[fi]));
        if (rows.back()) continue;
        fprintf(stderr, "\nerror: acados_amd: blob field %s is not a field of k_fields\n", K.fields[fi]);
        throw gqp_hip_failure{-1};
    }
    FieldRef s;
    for (int k = 0; k <= b->N; k++)
        for (const FieldRow *r : rows)
            if (field_resolve(b, r, k, K.use, s) > 0) visit(s);
}

/* the map of a kind, built on its first use */
static BulkMap &blob_map(ocp_qp_gpu_batch *b, BlobKind kind) /* throws gqp_hip_failure: callers are inside a guarded entry */
{
    HIPCHK(hipSetDevice(b->device));
    BulkMap &M = b->blob[kind];
    if (M.built) return M;
    finalize_structure(b);
    const BlobDesc &K = k_blobs[kind];
    if (kind == BLOB_SEED)
    {
        /* entry -> residual array (slot of k_seed_arrays: the table of _sens_set_bulk), element, sign there, slot in sfix */
        std::vector<int> sgn, elem2;
        blob_fields(b, K, [&](const FieldRef &s) {
            blob_segment_add(M, K.prefix + std::string(s.row->name), s, slot_of(k_seed_arrays, s.arr), s.map);
            for (int e = 0; e < s.len; e++)
            {
                sgn.push_back(s.row->sign);
                elem2.push_back(s.arr2 != ARR_NONE && s.map2[e] >= 0 ? s.map2[e] : -1);
            }
        });
        M.d_sgn = upload(b, sgn); M.d_elem2 = upload(b, elem2);
    }
    else
    {
        /* entry -> array (slot of k_state_arrays) and element in it; a mask entry -> (position, stage, bit) */
        table_fill(b, M.T, k_state_arrays);
        std::vector<int> moff, mstage, mbit, arr_g, elem_g;
        blob_fields(b, K, [&](const FieldRef &s) {
            const int o = (int) M.arr.size(), slot = slot_of(k_state_arrays, s.arr);
            blob_segment_add(M, K.prefix + std::string(s.row->name), s, slot, s.mask() ? std::vector<int>(s.len, -1) : s.map);
            if (s.mask())
                for (int e = 0; e < s.len; e++) { moff.push_back(o + e); mstage.push_back(s.k); mbit.push_back(s.map[e]); }
            M.writes_dyn |= s.arr == ARR_BAt; M.writes_hess |= s.arr == ARR_RSQ;
            if (s.arr2 != ARR_NONE)
                /* equality-flagged x bounds also define the value of the variable: a second, hidden
                 * segment that re-reads the same blob entries is not possible, so those entries are
                 * written through a duplicate segment placed right after (the caller's blob carries
                 * lbx twice: once as bound, once as value -- see ocp_qp_gpu_batch_bulk_offset) */
                blob_segment_add(M, std::string(s.row->name) + "#value", s, slot_of(k_state_arrays, s.arr2), s.map2);
            if (!K.read_map) return;
            /* the read map: what was just added, with the strict upper triangle of Q / R read from the mirrored element */
            arr_g.insert(arr_g.end(), M.arr.begin() + o, M.arr.end()); elem_g.insert(elem_g.end(), M.elem.begin() + o, M.elem.end());
            if (!(s.row->flags & F_SYM)) return;
            std::vector<int> g = s.map;
            mirror_lower(g, FieldCtx(b, s.k).nvar(s.row->cls));
            for (int e = 0; e < s.len; e++) { arr_g[o + e] = g[e] >= 0 ? slot : -1; elem_g[o + e] = g[e] >= 0 ? g[e] : 0; }
        });
        M.nm = (int) moff.size();
        if (K.read_map) { M.d_arr_g = upload(b, arr_g); M.d_elem_g = upload(b, elem_g); }
        M.d_moff = upload(b, moff); M.d_mstage = upload(b, mstage); M.d_mbit = upload(b, mbit);
    }
    M.len = (int) M.arr.size();
    M.d_arr = upload(b, M.arr); M.d_elem = upload(b, M.elem);
    if (!M.d_arr_g) { M.d_arr_g = M.d_arr; M.d_elem_g = M.d_elem; }
    M.built = true;
    return M;
}

/* position and length of one field at one stage; -1 / 0: not in the blob */
static int blob_segment(const BulkMap &M, const char *field, int stage, int *len)
{
    for (size_t q = 0; q < M.fields.size(); q++)
        if (M.seg_stage[q] == stage && M.fields[q] == field)
        {
            if (len) *len = M.seg_len[q];
            return M.seg_off[q];
        }
    if (len) *len = 0;
    return -1;
}

/* the C-ABI entries of the layout queries: the first of them after create builds the per-stage structure and the segment
 * tables on the device (dalloc / hipMemcpy / hipFuncSetAttribute) -- where an out-of-memory error of a large batch shows up
 * first.  No exception crosses the C ABI: -1 (no valid length / offset is negative) */
int ocp_qp_gpu_batch_bulk_len(ocp_qp_gpu_batch *b, int output)
try { return blob_map(b, blob_kind(output)).len; }
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_bulk_offset(ocp_qp_gpu_batch *b, int output, const char *field, int stage, int *len)
try { return blob_segment(blob_map(b, blob_kind(output)), field, stage, len); }
catch (const gqp_hip_failure &) { if (len) *len = 0; return -1; }

#define GQP_MASK_SPC 4 /* stages per thread of k_bulk_masks */

/* the arrays of a bulk map -> blob (instance-major): as bulk_scatter_launch below */
static void bulk_gather_launch(ocp_qp_gpu_batch *b, double *dst, int len, const int *d_arr, const int *d_elem, const gqp::GArrTable &T)
{
    if (b->fam.aos && !getenv("ACADOS_AMD_SCATTER_PLAIN"))
        hipLaunchKernelGGL(gqp::k_bulk_gather_aos, dim3((len + 255) / 256, b->B), dim3(256), 0, b->stream, dst, b->B, len, d_arr, d_elem, T);
    else if (!getenv("ACADOS_AMD_SCATTER_PLAIN"))
        GQP_LAUNCH_COOP(gqp::k_bulk_gather_tile, dim3((b->B + 63) / 64, (len + 63) / 64), dim3(64), 0, b->stream, dst, b->B, len, d_arr, d_elem, T);
    else
        hipLaunchKernelGGL(gqp::k_bulk_gather, dim3((b->B + 63) / 64, (len + 255) / 256), dim3(64), 0, b->stream, dst, b->B, len, d_arr, d_elem, T);
}

/* blob (instance-major) -> the arrays of a bulk map: lanes along the elements where the destinations are instance-major too, through
 * an LDS tile where they are wave-tiled (ACADOS_AMD_SCATTER_PLAIN=1: one lane per instance, the cross-check) */
static void bulk_scatter_launch(ocp_qp_gpu_batch *b, const double *src, int len, BulkMap &M)
{
    if (b->fam.aos && !getenv("ACADOS_AMD_SCATTER_PLAIN"))
        hipLaunchKernelGGL(gqp::k_bulk_scatter_aos, dim3((len + 255) / 256, b->B), dim3(256), 0, b->stream, src, b->B, len, M.d_arr, M.d_elem, M.T);
    else if (!getenv("ACADOS_AMD_SCATTER_PLAIN"))
        GQP_LAUNCH_COOP(gqp::k_bulk_scatter_tile, dim3((b->B + 63) / 64, (len + 63) / 64), dim3(64), 0, b->stream, src, b->B, len, M.d_arr, M.d_elem, M.T);
    else
        hipLaunchKernelGGL(gqp::k_bulk_scatter, dim3((b->B + 63) / 64, (len + 255) / 256), dim3(64), 0, b->stream, src, b->B, len, M.d_arr, M.d_elem, M.T);
}

/* a device-side blob of the kind of map M, BLOB_IN / BLOB_VEC (BLOB_OUT: no masks), into the batch: the scatter launch and, where
 * the kind has mask entries, the launch that turns them into the activity words.  No wait, no timing: those are the caller's */
static void blob_scatter(ocp_qp_gpu_batch *b, BulkMap &M, const double *src)
{
    b->held.data_written(M.writes_dyn, M.writes_hess);
    bulk_scatter_launch(b, src, M.len, M);
    if (M.nm)
        hipLaunchKernelGGL(gqp::k_bulk_masks, dim3((b->B + 63) / 64, (b->N + 1 + GQP_MASK_SPC - 1) / GQP_MASK_SPC), dim3(64), 0, b->stream, src, b->B, M.len, M.d_moff,
                           M.d_mstage, M.d_mbit, M.nm, b->D.amask, b->fam.AW, GQP_MASK_SPC);
}

/* the caller's blob of a kind: copy (where it is a host pointer) + scatter, timed and waited for */
static void blob_set(ocp_qp_gpu_batch *b, BlobKind kind, const double *blob, int is_device)
{
    BulkMap &M = blob_map(b, kind);
    pack_timed(b, [&] { blob_scatter(b, M, stage_in(b, blob, (size_t) b->B * M.len, is_device)); });
}

int ocp_qp_gpu_batch_set_bulk(ocp_qp_gpu_batch *b, const double *blob, int is_device)
try
{
    blob_set(b, BLOB_IN, blob, is_device);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* the vector fields alone (blob layout: ocp_qp_gpu_batch_bulk_len / _bulk_offset with which = 2): the matrices stay what the last
 * _set_bulk brought -- the host side of an RTI feedback step (condense_lhs done, new gradient / offsets / bounds) */
int ocp_qp_gpu_batch_set_bulk_vec(ocp_qp_gpu_batch *b, const double *blob, int is_device)
try
{
    blob_set(b, BLOB_VEC, blob, is_device);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* ---- zero-copy gather: the device reads the instances' QP data from the caller's own (registered) host memory ----
 * Through the boundary the host pass that copies n capsules' member arrays into a pinned blob is bound by the host memory system
 * (1.8 GB/s per thread on 16 threads) while a kernel reads registered host memory at the PCIe rate (56 GB/s,
 * profiles/r06_zero_copy_probe.txt).  _host_register pins a block and maps it for the device (hipHostRegister; device pointer = host
 * pointer); _gather_tables takes the class-wide word tables once; _gather_run takes the per-instance source pointers of this call,
 * gathers into the device-side blob and scatters it as _set_bulk / _set_bulk_vec do -- byte-identical to the blob path. */
int ocp_qp_gpu_host_register(void *p, size_t bytes)
{
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) { (void) hipGetLastError(); return -1; }
    void *dp = nullptr; /* the gather takes HOST addresses: only where the device sees the block at the same one */
    if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess || dp != p)
    {
        (void) hipGetLastError();
        (void) hipHostUnregister(p);
        return -1;
    }
    return 0;
}

int ocp_qp_gpu_host_unregister(void *p)
{
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void) hipGetLastError(); return -1; }
    return 0;
}

int ocp_qp_gpu_batch_gather_tables(ocp_qp_gpu_batch *b, int which, int P, int n_words, const int *w_slot, const int *w_off, const int *w_pos,
                                   const unsigned char *w_neg)
try
{
    const BlobKind kind = blob_kind(which, false);
    const int len = blob_map(b, kind).len;
    for (int w = 0; w < n_words; w++)
        if (w_slot[w] < 0 || w_slot[w] >= P || w_pos[w] < 0 || w_pos[w] >= len || w_off[w] < 0) return -1;
    auto &G = b->gtab[kind];
    G.P = P; G.n_words = n_words;
    {
        /* do the words write EVERY position of the blob?  If not, the gather clears its buffer first: the positions no word writes
         * are zero for the scatter (the buffer is shared with the other blob and the chunk protocol) */
        std::vector<char> seen((size_t) len, 0);
        int covered = 0;
        for (int w = 0; w < n_words; w++) if (!seen[w_pos[w]]) { seen[w_pos[w]] = 1; covered++; }
        G.full = covered == len;
    }
    G.d_slot = upload(b, w_slot, n_words); G.d_off = upload(b, w_off, n_words); G.d_pos = upload(b, w_pos, n_words); G.d_neg = upload(b, w_neg, n_words);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* the buffer of the device-side input blob (chunk protocol and zero-copy gather; one for both blobs: the full one is the longer).
 * B * len is fixed for a batch: exactly that.  True where it was allocated here: nothing of a round is in it */
static bool chunks_reserve(ocp_qp_gpu_batch *b)
{
    const size_t cnt = (size_t) b->B * blob_map(b, BLOB_IN).len;
    if (cnt <= b->chunks_cap) return false;
    HIPCHK(hipStreamSynchronize(b->stream)); /* (only ever on the first use by a batch: nothing of it is in flight yet) */
    b->chunks_cap = cnt;
    b->d_chunks = dalloc<double>(b, b->chunks_cap);
    return true;
}

int ocp_qp_gpu_batch_gather_run(ocp_qp_gpu_batch *b, int which, const void *const *ptrs)
try
{
    HIPCHK(hipSetDevice(b->device));
    const BlobKind kind = blob_kind(which, false);
    auto &G = b->gtab[kind];
    if (G.n_words <= 0 || G.P <= 0) return -1;
    BulkMap &M = blob_map(b, kind);
    const int len = M.len;
    chunks_reserve(b);
    const size_t np = (size_t) b->B * G.P;
    if (np > b->gptrs_cap) { b->gptrs_cap = np; b->d_gptrs = dalloc<const double *>(b, np); }
    pack_timed(b, [&] { /* pointer copy + gather + scatter */
        HIPCHK(hipMemcpyAsync(b->d_gptrs, ptrs, sizeof(void *) * np, hipMemcpyHostToDevice, b->stream));
        if (!G.full) HIPCHK(hipMemsetAsync(b->d_chunks, 0, sizeof(double) * (size_t) b->B * (size_t) len, b->stream));
        hipLaunchKernelGGL(gqp::k_gather_host, dim3((G.n_words + 255) / 256, b->B), dim3(256), 0, b->stream, (const double *const *) b->d_gptrs, G.P, b->B,
                           G.n_words, (const int *) G.d_slot, (const int *) G.d_off, (const int *) G.d_pos, (const unsigned char *) G.d_neg, b->d_chunks, len);
        b->chunks_got = 0; /* (the chunk protocol shares the buffer: a round in flight is void) */
        blob_scatter(b, M, b->d_chunks);
    });
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* _set_bulk in pieces: a caller that fills its blob instance range by instance range (host threads unpacking n acados structs)
 * hands every finished range over at once -- the host->device copy of range j runs while range j + 1 is still being filled --
 * and scatters when the last one is in.  `blob_chunk` points at instance `first` of the caller's (pinned) blob; nothing is waited
 * for here.  _set_bulk_staged: the scatter launch (+ masks) over what the chunks brought, then the usual wait. */
int ocp_qp_gpu_batch_set_bulk_chunk(ocp_qp_gpu_batch *b, const double *blob_chunk, int first, int count)
try
{
    const int len = blob_map(b, BLOB_IN).len;
    if (first < 0 || count < 0 || first + count > b->B) return -1;
    if (chunks_reserve(b)) b->chunks_got = 0;
    if (b->chunks_got == 0)
    {
        if (!b->chunks_ev) HIPCHK(hipEventCreate(&b->chunks_ev));
        HIPCHK(hipEventRecord(b->chunks_ev, b->stream));
    }
    b->chunks_got += count;
    if (count)
        HIPCHK(hipMemcpyAsync(b->d_chunks + (size_t) first * len, blob_chunk, sizeof(double) * (size_t) count * len, hipMemcpyHostToDevice, b->stream));
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_set_bulk_staged(ocp_qp_gpu_batch *b)
try
{
    BulkMap &M = blob_map(b, BLOB_IN);
    if ((size_t) b->B * M.len > b->chunks_cap) return -1; /* no chunk was ever handed over */
    /* every instance must have arrived in THIS round: a missing range would scatter the previous call's data for those instances
     * (ranges are the caller's to keep disjoint: the count is what can be checked here) */
    const long got = b->chunks_got;
    b->chunks_got = 0;
    if (got != (long) b->B)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_set_bulk_staged: %ld of %d instances were handed over since the last scatter\n", got, b->B);
        return -1;
    }
    pack_timed_since(b, b->chunks_ev, [&] { blob_scatter(b, M, b->d_chunks); }); /* first chunk ... scatter */
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* the QP data of the batch in the INPUT blob layout (inverse of _set_bulk): how the acados-side condensing module reads the
 * condensed QP of a child batch back into acados' containers (integration/ocp_qp_gpu_pcond.c) -- one launch (+ one for the
 * masks) and one device->host copy instead of one copy per field and stage */
int ocp_qp_gpu_batch_get_bulk_in(ocp_qp_gpu_batch *b, double *blob, int is_device)
try
{
    BulkMap &M = blob_map(b, BLOB_IN);
    const size_t cnt = (size_t) b->B * M.len;
    double *dst = stage_out(b, blob, cnt, is_device);
    bulk_gather_launch(b, dst, M.len, M.d_arr_g, M.d_elem_g, M.T);
    if (M.nm)
        hipLaunchKernelGGL(gqp::k_bulk_masks_get, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, dst, b->B, M.len, M.d_moff,
                           M.d_mstage, M.d_mbit, M.nm, b->D.amask, b->fam.AW);
    stage_out_done(b, blob, cnt, is_device);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* an iterate in the OUTPUT blob layout (u x sl su pi lam t) written into the batch: the starting point of a hot
 * start, one host->device copy and one launch (inverse of _get_bulk) */
int ocp_qp_gpu_batch_set_bulk_out(ocp_qp_gpu_batch *b, const double *blob, int is_device)
try
{
    BulkMap &M = blob_map(b, BLOB_OUT);
    blob_scatter(b, M, stage_in(b, blob, (size_t) b->B * M.len, is_device));
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* the OUTPUT blob read from the solution arrays, or (directions) through the same element maps from the direction arrays of the
 * last _sens_solve */
static void blob_get_out(ocp_qp_gpu_batch *b, double *blob, int is_device, bool directions)
{
    BulkMap &M = blob_map(b, BLOB_OUT);
    gqp::GArrTable T = M.T;
    if (directions)
        for (Arr a : {ARR_ux, ARR_sv, ARR_pi, ARR_lam, ARR_t}) T.a[slot_of(k_state_arrays, a)] = arr_of(b, direction_of(a));
    const size_t cnt = (size_t) b->B * M.len;
    bulk_gather_launch(b, stage_out(b, blob, cnt, is_device), M.len, M.d_arr_g, M.d_elem_g, T);
    stage_out_done(b, blob, cnt, is_device);
}

int ocp_qp_gpu_batch_get_bulk(ocp_qp_gpu_batch *b, double *blob, int is_device)
try
{
    blob_get_out(b, blob, is_device, false);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* ---- bulk seeds / sensitivities: every seed of every instance in one host->device copy and one launch, every
 * direction back in one launch and one copy (BLOB_SEED in, BLOB_OUT back) ---- */
int ocp_qp_gpu_batch_sens_bulk_len(ocp_qp_gpu_batch *b, int output)
try { return blob_map(b, output ? BLOB_OUT : BLOB_SEED).len; }
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_sens_bulk_offset(ocp_qp_gpu_batch *b, int output, const char *field, int stage, int *len)
try
{
    if (!output) return blob_segment(blob_map(b, BLOB_SEED), field, stage, len);
    if (strncmp(field, "sens_", 5)) { if (len) *len = 0; return -1; }
    return blob_segment(blob_map(b, BLOB_OUT), field + 5, stage, len);
}
catch (const gqp_hip_failure &) { if (len) *len = 0; return -1; }

int ocp_qp_gpu_batch_sens_set_bulk(ocp_qp_gpu_batch *b, const double *blob, int is_device)
try
{
    BulkMap &M = blob_map(b, BLOB_SEED);
    const int len = M.len;
    if (sens_begin(b)) return -1; /* zeroes the seed arrays, factorises at the solution where the sweeps run in place */
    if (len == 0) return 0;
    table_fill(b, M.T, k_seed_arrays);
    const double *src = stage_in(b, blob, (size_t) b->B * len, is_device);
    const dim3 grid((b->B + 63) / 64, (len + 255) / 256), block(64);
    hipLaunchKernelGGL(gqp::k_bulk_scatter_seed, grid, block, 0, b->stream, src, b->B, len, M.d_arr, M.d_elem, M.d_sgn, M.d_elem2, M.T);
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_sens_get_bulk(ocp_qp_gpu_batch *b, double *blob, int is_device)
try
{
    blob_get_out(b, blob, is_device, true);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* ---- reverse-mode data gradients (grad_kernels.hpp, DESIGN.md "Data gradients") ---- */
static void grad_build(ocp_qp_gpu_batch *b)
{
    auto &G = b->grad;
    if (G.built) return;
    const BulkMap &Mi = blob_map(b, BLOB_IN), &Mo = blob_map(b, BLOB_OUT);
    const int len = Mi.len, olen = Mo.len;
    const int N = b->N, NX = b->fam.ks()->NX, NU = b->fam.ks()->NU, n = NX + NU, NP = n * (n + 1) / 2;
    auto ob = [&](const char *f, int k, int *len = nullptr) {
        int l = 0;
        const int o = f ? blob_segment(Mo, f, k, &l) : -1;
        if (len) *len = l;
        return l > 0 ? o : -1;
    };
    /* output blob: gather map renumbered to the kernel's table, activity gates, cotangent destinations */
    std::vector<int> oarr(olen, -1), oelem = Mo.elem, ogate(olen, -1), ckind(olen, 0), celem(olen, 0);
    for (int e = 0; e < olen; e++) oarr[e] = Mo.arr[e] >= 0 ? slot_of(k_grad_arrays, k_state_arrays[Mo.arr[e]]) : -1;
    for (size_t q = 0; q < Mo.fields.size(); q++)
    {
        const int k = Mo.seg_stage[q], o = Mo.seg_off[q], l = Mo.seg_len[q];
        const FieldCtx c(b, k);
        for (int e = 0; e < l; e++)
            switch (k_fields[Mo.seg_row[q]].arr)
            {
            case ARR_ux: /* to rg, but for a fixed variable */
                ckind[o + e] = ((c.S.emask >> (oelem[o + e] - k * n)) & 1) ? 3 : 1;
                celem[o + e] = oelem[o + e];
                break;
            case ARR_sv: /* to rgs */
                ckind[o + e] = 2;
                celem[o + e] = oelem[o + e];
                break;
            case ARR_lam:
            case ARR_t:
            {
                const int bit = oelem[o + e] - c.S.o_ct;
                ogate[o + e] = (k * b->fam.AW + bit / 64) * 64 + bit % 64;
                if (e < 2 * c.nbg && c.eq(e % c.nbg)) ogate[o + e] = -2; /* (the sides in the original row order) */
                break;
            }
            default: break;
            }
    }
    const int t_hess = slot_of(k_grad_arrays, ARR_RSQ), t_dyn = slot_of(k_grad_arrays, ARR_BAt), t_gen = slot_of(k_grad_arrays, ARR_DCt),
              t_cot = slot_of(k_grad_arrays, ARR_cot);
    /* input blob: one op per entry */
    std::vector<gqp::GradOp> ops(len, gqp::GradOp{0, 0, -1, 0, 0.0});
    std::vector<gqp::GradTerm> terms;
    for (size_t q = 0; q < Mi.fields.size(); q++)
    {
        const FieldRow &r = k_fields[Mi.seg_row[q]];
        const int k = Mi.seg_stage[q], o = Mi.seg_off[q], l = Mi.seg_len[q];
        const FieldCtx c(b, k);
        const GqpStage &S = c.S;
        const int nx = c.nx, nu = c.nu, nx1 = c.nx1, ng = c.ng, nb = S.nb, nbg = c.nbg;
        const int ou = ob("u", k), ox = ob("x", k), opi = k < N ? ob("pi", k) : -1, olam = ob("lam", k);
        int la = 0; /* the row's own factors: S[] / D[] of the fields ga (la long) and gb */
        const int oa = ob(r.ga, k, &la), og = ob(r.gb, k);
        auto vec = [&](int e, int a, double co) { ops[o + e] = gqp::GradOp{1, a, -1, 0, co}; };
        auto prod = [&](int e, int a, int a2, int bb, double co) { ops[o + e] = gqp::GradOp{2, a, a2, bb, co}; };
        if (Mi.fields[q] == "lbx#value")
        {
            for (int e = 0; e < l; e++)
            {
                const int row = c.nbu + e;
                if (!c.eq(row)) continue;
                /* the value of a fixed variable: its stationarity row applied to the adjoint direction, plus its own cotangent */
                const int vi = b->idxb[k][row], j = c.pv(vi);
                const int t0 = (int) terms.size();
                terms.push_back(gqp::GradTerm{t_cot, k * n + j, -1, 0, 1.0});
                for (int i = 0; i < nu + nx; i++)
                {
                    const int pr = c.pv(i);
                    terms.push_back(gqp::GradTerm{t_hess, k * NP + (pr >= j ? PK(pr, j) : PK(j, pr)), i < nu ? ou + i : ox + i - nu, 0, 1.0});
                }
                for (int i = 0; i < nx1; i++) terms.push_back(gqp::GradTerm{t_dyn, (k * n + j) * NX + i, opi + i, 0, 1.0});
                if (vi >= nu && k > 0) terms.push_back(gqp::GradTerm{-1, 0, ob("pi", k - 1) + vi - nu, 0, -1.0});
                for (int g = 0; g < ng; g++)
                {
                    terms.push_back(gqp::GradTerm{t_gen, (S.o_g + g) * n + j, olam + nbg + nb + g, 0, 1.0});
                    terms.push_back(gqp::GradTerm{t_gen, (S.o_g + g) * n + j, olam + nb + g, 0, -1.0});
                }
                ops[o + e] = gqp::GradOp{3, t0, (int) terms.size(), 0, 0.0};
            }
            continue;
        }
        for (int e = 0; e < l; e++)
            switch (r.grad)
            {
            case G_VEC: vec(e, oa + e, 1.0); break;                                   /* b q r zl zu: the direction of their variable */
            case G_PROD: prod(e, oa + e % la, -1, og + e / la, r.gc); break;          /* A B Q R S: entry (row of ga, column of gb) */
            case G_DIAG: prod(e, oa + e, -1, oa + e, r.gc); break;                    /* Zl Zu */
            case G_GEN: prod(e, olam + nbg + nb + e % ng, olam + nb + e % ng, og + e / ng, 1.0); break; /* C D: upper minus lower side */
            case G_CT: if (!c.ct_eq(r, e)) vec(e, olam + c.ct_pos(r, e), -r.sign); break; /* a bound: -+ lam^ of its side, the seed's sign reversed */
            default: break;                                                          /* masks: op 0 */
            }
    }
    G.len = len;
    G.olen = olen;
    G.lds = sizeof(double) * 2 * (size_t) olen;
    G.d_ops = upload(b, ops);
    G.h_ops = ops;
    G.d_terms = upload(b, terms);
    G.d_oarr = upload(b, oarr); G.d_oelem = upload(b, oelem); G.d_ogate = upload(b, ogate);
    G.d_ckind = upload(b, ckind); G.d_celem = upload(b, celem);
    G.h_ckind = ckind; G.h_ogate = ogate;
    G.d_bad = dalloc<int>(b, 1);
    G.cot = garr<double>(b, (size_t) (N + 2) * n);
    if (G.lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *) gqp::k_data_grad, hipFuncAttributeMaxDynamicSharedMemorySize, (int) G.lds));
    G.built = true;
}

int ocp_qp_gpu_batch_adj_seed_bulk(ocp_qp_gpu_batch *b, const double *cot, int is_device)
try
{
    HIPCHK(hipSetDevice(b->device));
    grad_build(b);
    auto &G = b->grad;
    if (G.lds > 160 * 1024)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_adj_seed_bulk: the solution of one instance (%d doubles) does not fit the LDS of a workgroup\n", G.olen);
        return -1;
    }
    G.seeded = false;
    if (sens_begin(b)) return -1; /* zeroes the seed arrays, factorises at the solution where the sweeps run in place */
    const double *src = stage_in(b, cot, (size_t) b->B * G.olen, is_device);
    HIPCHK(hipMemsetAsync(G.d_bad, 0, sizeof(int), b->stream));
    HIPCHK(hipMemsetAsync(G.cot.p, 0, sizeof(double) * (size_t) G.cot.E * b->Bp, b->stream));
    if (G.olen)
        hipLaunchKernelGGL(gqp::k_adj_seed, dim3((G.olen + 255) / 256, b->B), dim3(256), 0, b->stream, src, b->B, G.olen, G.d_ckind, G.d_celem,
                           b->D.rg, b->D.rgs, G.cot, G.d_bad);
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, G.d_bad, sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (bad)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_adj_seed_bulk: cotangents on pi / lam / t are not supported (only u x sl su)\n");
        sens_begin(b); /* leave an all-zero seed set, not a partial one */
        HIPCHK(hipMemsetAsync(b->D.rg.p, 0, sizeof(double) * (size_t) b->D.rg.E * b->Bp, b->stream));
        HIPCHK(hipMemsetAsync(b->D.rgs.p, 0, sizeof(double) * (size_t) b->D.rgs.E * b->Bp, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        return -1;
    }
    G.seeded = true;
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_data_grad_bulk(ocp_qp_gpu_batch *b, double *grad, int is_device)
try
{
    HIPCHK(hipSetDevice(b->device));
    grad_build(b);
    auto &G = b->grad;
    if (!G.seeded || !b->sens_open)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_data_grad_bulk: no adjoint seed (call ocp_qp_gpu_batch_adj_seed_bulk after the solve)\n");
        return -1;
    }
    G.seeded = false;
    if (ocp_qp_gpu_batch_sens_solve(b)) return -1; /* the adjoint direction, in dux dsv dpi dlam dt */
    const size_t cnt = (size_t) b->B * G.len;
    double *dst = stage_out(b, grad, cnt, is_device);
    const GqpDev &D = b->D;
    gqp::GArrTable T;
    table_fill(b, T, k_grad_arrays);
    const int per = (b->B + GQP_GRAD_XCD - 1) / GQP_GRAD_XCD;
    if (G.len)
        GQP_LAUNCH_COOP(gqp::k_data_grad, dim3(per * GQP_GRAD_XCD), dim3(GQP_GRAD_THREADS), G.lds, b->stream, dst, b->B, G.len, G.d_ops, G.d_terms,
                        G.olen, G.d_oarr, G.d_oelem, G.d_ogate, T, D.amask, D.status, per);
    HIPCHK(hipGetLastError());
    stage_out_done(b, grad, cnt, is_device);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* output-blob entry d -> the seed entry (BLOB_SEED) that the direction D[d] of the sweeps is the derivative to, and its sign: the
 * seed of r q zl zu b for u x sl su pi, of a bound (natural sign) for lam of its side, + for a lower and - for an upper side (the
 * sign its gradient carries); se = -1 for t, for both sides of an equality-flagged row and for an entry without a seed.  The sweeps
 * are symmetric under this map, so it is read in both directions: forward mode feeds the seed from the tangent of what D[d]
 * multiplies (tangent_build), reverse mode seeds entry se with the cotangent of entry d (seed_all_build) */
struct DSeed { int se; double c; };
static std::vector<DSeed> seed_of_output(ocp_qp_gpu_batch *b)
{
    const BulkMap &Mo = blob_map(b, BLOB_OUT), &Ms = blob_map(b, BLOB_SEED);
    std::vector<DSeed> dmap(Mo.len, DSeed{-1, 0.0});
    for (size_t q = 0; q < Ms.fields.size(); q++)
    {
        const FieldRow &r = k_fields[Ms.seg_row[q]];
        const int k = Ms.seg_stage[q], o = Ms.seg_off[q], l = Ms.seg_len[q];
        const FieldCtx c(b, k);
        int la = 0, ll = 0;
        const int oa = r.ga ? blob_segment(Mo, r.ga, k, &la) : -1, olam = blob_segment(Mo, "lam", k, &ll);
        if ((r.grad == G_VEC && (oa < 0 || la != l)) || (r.grad == G_CT && olam < 0))
        {
            fprintf(stderr, "\nerror: acados_amd: seed field %s of stage %d has no counterpart in the output blob\n", r.name, k);
            throw gqp_hip_failure{-1};
        }
        for (int e = 0; e < l; e++)
            if (r.grad == G_VEC)
                dmap[oa + e] = DSeed{o + e, 1.0};
            else if (r.grad == G_CT && !c.ct_eq(r, e))
            {
                const int pos = c.ct_pos(r, e);
                if (pos >= ll)
                {
                    fprintf(stderr, "\nerror: acados_amd: seed field %s of stage %d lies outside lam of the output blob\n", r.name, k);
                    throw gqp_hip_failure{-1};
                }
                dmap[olam + pos] = DSeed{o + e, -(double) r.sign};
            }
    }
    return dmap;
}

/* the table of k_adj_seed_all: where the cotangent of every output entry goes (seed_of_output for the seed entry, the seed blob's
 * own map for its residual array, element and stored sign) */
static void seed_all_build(ocp_qp_gpu_batch *b)
{
    grad_build(b);
    auto &G = b->grad;
    if (G.all_built) return;
    const BulkMap &Mo = blob_map(b, BLOB_OUT), &Ms = blob_map(b, BLOB_SEED);
    const std::vector<DSeed> dmap = seed_of_output(b);
    std::vector<int> ssgn(Ms.len, 1); /* the sign a seed entry is stored with (what blob_map uploaded as d_sgn) */
    for (size_t q = 0; q < Ms.fields.size(); q++)
        for (int e = 0; e < Ms.seg_len[q]; e++) ssgn[Ms.seg_off[q] + e] = k_fields[Ms.seg_row[q]].sign;
    std::vector<gqp::SeedOp> ops(G.olen, gqp::SeedOp{-1, 0, -1, -1, 0, 0, 0.0});
    for (size_t q = 0; q < Mo.fields.size(); q++)
    {
        const Arr arr = k_fields[Mo.seg_row[q]].arr;
        const int k = Mo.seg_stage[q], o = Mo.seg_off[q], l = Mo.seg_len[q];
        int lt = 0;
        const int ot = arr == ARR_lam ? blob_segment(Mo, "t", k, &lt) : -1; /* the partner of a lam entry: t of the same side */
        if (arr == ARR_t) continue;                                        /* (consumed by its lam entry) */
        for (int e = 0; e < l; e++)
        {
            const int d = o + e;
            gqp::SeedOp &p = ops[d];
            if (arr == ARR_ux) p.cot = G.h_ckind[d] ? Mo.elem[d] : -1; /* kinds 1 and 3: the fixed variables' own term of op 3 */
            const int se = dmap[d].se;
            if (G.h_ckind[d] == 3 || G.h_ogate[d] == -2 || se < 0 || Ms.arr[se] < 0) continue;
            p.slot = Ms.arr[se];
            p.dst = Ms.elem[se];
            p.c = dmap[d].c * ssgn[se];
            if (arr != ARR_lam) continue;
            p.gate = G.h_ogate[d];
            p.le = Mo.elem[d];
            p.part = ot + e;
            if (ot < 0 || lt != l || p.gate < 0)
            {
                fprintf(stderr, "\nerror: acados_amd: lam of stage %d has no t / no activity bit in the output blob\n", k);
                throw gqp_hip_failure{-1};
            }
        }
    }
    /* (what the kernel indexes with) */
    const GArr dst[] = {b->D.rg, b->D.rgs, b->D.rb, b->D.rd};
    for (int d = 0; d < G.olen; d++)
    {
        const gqp::SeedOp &p = ops[d];
        const bool lamrow = p.slot >= 0 && p.gate >= 0;
        if (p.slot >= 4 || (p.slot >= 0 && (p.dst < 0 || p.dst >= dst[p.slot].E)) || p.cot >= G.cot.E ||
            (lamrow && (p.le < 0 || p.le >= b->D.lam.E || p.le >= b->D.t.E || p.part < 0 || p.part >= G.olen || (p.gate >> 6) >= b->D.amask.E)))
        {
            fprintf(stderr, "\nerror: acados_amd: adjoint seed table out of range at output entry %d\n", d);
            throw gqp_hip_failure{-1};
        }
    }
    G.d_sops = upload(b, ops);
    G.all_built = true;
}

/* _adj_seed_bulk for a cotangent on every entry of the output blob: the same sequence, k_adj_seed_all in place of k_adj_seed; refuses
 * nothing.  _data_grad_bulk follows it as it is: its contraction holds for any right-hand side of the symmetric system */
int ocp_qp_gpu_batch_adj_seed_all_bulk(ocp_qp_gpu_batch *b, const double *cot, int is_device)
try
{
    HIPCHK(hipSetDevice(b->device));
    seed_all_build(b);
    auto &G = b->grad;
    if (G.lds > 160 * 1024)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_adj_seed_all_bulk: the solution of one instance (%d doubles) does not fit the LDS of a workgroup\n", G.olen);
        return -1;
    }
    G.seeded = false;
    if (sens_begin(b)) return -1; /* zeroes the seed arrays, factorises at the solution where the sweeps run in place */
    const double *src = stage_in(b, cot, (size_t) b->B * G.olen, is_device);
    HIPCHK(hipMemsetAsync(G.cot.p, 0, sizeof(double) * (size_t) G.cot.E * b->Bp, b->stream));
    gqp::GArrTable T;
    table_fill(b, T, k_seed_arrays);
    if (G.olen)
        hipLaunchKernelGGL(gqp::k_adj_seed_all, dim3((G.olen + 255) / 256, b->B), dim3(256), 0, b->stream, src, b->B, G.olen, G.d_sops, T, G.cot,
                           b->D.lam, b->D.t, b->D.amask, b->D.status);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    G.seeded = true;
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* ---- forward-mode data derivative (grad_kernels.hpp k_data_tangent, DESIGN.md "Data gradients", Forward mode) ----
 * the ops of grad_build transposed: where the gradient of an input entry e reads the adjoint direction D[d], the tangent of e
 * feeds the seed that D[d] is the derivative to -- the seed of r q zl zu b for u x sl su pi, of a bound for lam of its side
 * (with the sign its gradient carries).  One term list per entry of the seed blob, the entry's own tangent first, then the matrix
 * entries in blob order. */
static void tangent_build(ocp_qp_gpu_batch *b)
{
    grad_build(b);
    auto &G = b->grad;
    if (G.tan_built) return;
    const BulkMap &Mi = blob_map(b, BLOB_IN), &Ms = blob_map(b, BLOB_SEED);
    const int slen = Ms.len;
    const std::vector<DSeed> dmap = seed_of_output(b);
    std::vector<std::vector<gqp::TanTerm>> lists(slen);
    std::vector<int> sgate(slen, -1);
    for (size_t q = 0; q < Ms.fields.size(); q++)
    {
        const FieldRow &r = k_fields[Ms.seg_row[q]];
        const int k = Ms.seg_stage[q], o = Ms.seg_off[q], l = Ms.seg_len[q];
        const FieldCtx c(b, k);
        int li = 0, lv = 0;
        const int oi = blob_segment(Mi, r.name, k, &li); /* the same field of the input blob */
        const int ov = (r.flags & F_VALUE) ? blob_segment(Mi, (std::string(r.name) + "#value").c_str(), k, &lv) : -1;
        if (oi < 0 || li != l || (ov >= 0 && lv != l))
        {
            fprintf(stderr, "\nerror: acados_amd: seed field %s of stage %d has no counterpart in the input blob\n", r.name, k);
            throw gqp_hip_failure{-1};
        }
        for (int e = 0; e < l; e++)
            if (r.grad == G_VEC)
                lists[o + e].push_back(gqp::TanTerm{oi + e, -1, 1.0});
            else if (r.grad == G_CT && c.ct_eq(r, e))
            {
                /* an equality-flagged row: the seed of lbx is the derivative of the variable's value, the bounds take no part */
                if (ov >= 0) lists[o + e].push_back(gqp::TanTerm{ov + e, -1, 1.0});
                else sgate[o + e] = -2;
            }
            else if (r.grad == G_CT)
            {
                const int d = c.ct_dev(c.ct_pos(r, e));
                sgate[o + e] = (k * b->fam.AW + d / 64) * 64 + d % 64;
                lists[o + e].push_back(gqp::TanTerm{oi + e, -1, 1.0});
            }
    }
    for (int e = 0; e < G.len; e++)
    {
        const gqp::GradOp &p = G.h_ops[e];
        if (p.op != 2) continue;
        /* c (D[a] - D[a2]) S[b] + c (S[a] - S[a2]) D[b], transposed */
        auto add = [&](int d, double co, int si) {
            if (d < 0 || dmap[d].se < 0) return;
            lists[dmap[d].se].push_back(gqp::TanTerm{e, si, co * dmap[d].c});
        };
        add(p.a, p.c, p.b);
        add(p.a2, -p.c, p.b);
        add(p.b, p.c, p.a);
        if (p.a2 >= 0) add(p.b, -p.c, p.a2);
    }
    std::vector<int> row(slen + 1, 0);
    std::vector<gqp::TanTerm> terms;
    for (int e = 0; e < slen; e++)
    {
        for (const gqp::TanTerm &t : lists[e])
        {
            if (t.te < 0 || t.te >= G.len || t.si >= G.olen) /* (what the kernel indexes with) */
            {
                fprintf(stderr, "\nerror: acados_amd: tangent table out of range at seed entry %d\n", e);
                throw gqp_hip_failure{-1};
            }
            terms.push_back(t);
        }
        row[e + 1] = (int) terms.size();
    }
    G.slen = slen;
    G.d_trow = upload(b, row); G.d_tterms = upload(b, terms); G.d_sgate = upload(b, sgate);
    G.d_seed = dalloc<double>(b, (size_t) b->B * (size_t) std::max(slen, 1));
    if (G.lds / 2 > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *) gqp::k_data_tangent, hipFuncAttributeMaxDynamicSharedMemorySize, (int) (G.lds / 2)));
    G.tan_built = true;
}

/* d(solution) along a tangent of the whole QP data: tangent in the INPUT blob layout, the result in the OUTPUT blob layout
 * (u x sl su pi lam t), with the KKT matrix at the final iterate -- the tangent folded into one seed set on the device, then the
 * bulk sensitivity path as it is (_sens_set_bulk on the device blob, _sens_solve, the read-back of _sens_get_bulk) */
int ocp_qp_gpu_batch_data_jvp_bulk(ocp_qp_gpu_batch *b, const double *tangent, double *out, int is_device)
try
{
    HIPCHK(hipSetDevice(b->device));
    tangent_build(b);
    auto &G = b->grad;
    if (G.lds > 160 * 1024)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_data_jvp_bulk: the solution of one instance (%d doubles) does not fit the LDS of a workgroup\n", G.olen);
        return -1;
    }
    G.seeded = false;      /* the residual arrays hold this call's seeds from here on: no adjoint seed survives it */
    b->sens_open = false;  /* ... and a seed set of its own: _sens_set_bulk zeroes what an open one held */
    const double *src = stage_in(b, tangent, (size_t) b->B * G.len, is_device);
    gqp::GArrTable T;
    table_fill(b, T, k_grad_arrays);
    const int per = (b->B + GQP_GRAD_XCD - 1) / GQP_GRAD_XCD;
    if (G.slen)
        GQP_LAUNCH_COOP(gqp::k_data_tangent, dim3(per * GQP_GRAD_XCD), dim3(GQP_GRAD_THREADS), G.lds / 2, b->stream, G.d_seed, b->B, G.slen, src, G.len,
                        G.d_trow, G.d_tterms, G.d_sgate, G.olen, G.d_oarr, G.d_oelem, G.d_ogate, T, b->D.amask, b->D.status, per);
    HIPCHK(hipGetLastError());
    if (ocp_qp_gpu_batch_sens_set_bulk(b, G.d_seed, 1)) return -1;
    if (ocp_qp_gpu_batch_sens_solve(b)) return -1;
    const size_t cnt = (size_t) b->B * G.olen;
    double *dst = stage_out(b, out, cnt, is_device);
    blob_get_out(b, dst, 1, true);
    /* instances whose solve failed: their factor is no factor of a KKT matrix, whatever the sweeps made of a zero seed is zeroed */
    std::vector<int> st(b->B);
    HIPCHK(hipMemcpy(st.data(), b->D.status, sizeof(int) * b->B, hipMemcpyDeviceToHost));
    for (int i = 0; i < b->B;)
    {
        int j = i;
        while (j < b->B && st[j] != 0) j++;
        if (j > i && G.olen) HIPCHK(hipMemsetAsync(dst + (size_t) i * G.olen, 0, sizeof(double) * (size_t) (j - i) * G.olen, b->stream));
        i = j + 1;
    }
    stage_out_done(b, out, cnt, is_device);
    return 0;
}
catch (const gqp_hip_failure &) { return -1; }

/* pinned host memory for callers that stage their own blobs (the acados-side adapter is plain C and has no HIP) */
void *ocp_qp_gpu_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 8) != hipSuccess)
    {
        fprintf(stderr, "acados_amd: cannot allocate %zu bytes of pinned host memory\n", bytes);
        return nullptr;
    }
    return p;
}

void ocp_qp_gpu_host_free(void *p)
{
    if (p) (void) hipHostFree(p);
}

/* ---- multi-GPU: the ONLY collective of the path -- one gather over xGMI of the solutions and their
 * per-instance status / iteration counts plus the per-rank solve time, from device buffers on the batch's stream.
 * The communicator is a table of five transport entries (ocp_qp_gpu_comm_ops): RCCL's, bound at run time (dlopen: the copy
 * PyTorch has already loaded if there is one, so that the process holds a single RCCL instance; else the ROCm one), or a
 * table the host program supplies (ocp_qp_gpu_comm_create_from_ops: an MPI program, or the CPU test tier, which drives the
 * packing / offset / ordering logic below with torch.distributed's gloo as the transport).  One process per GPU; the RCCL
 * unique id travels between the processes by whatever means the host program has (torch.distributed broadcast in
 * bench.py, MPI_Bcast in a C harness). ---- */
struct ocp_qp_gpu_comm
{
    ocp_qp_gpu_comm_ops ops = {};
    int n = 0, rank = 0, device = 0;
    /* RCCL backing (null for an injected table) */
    void *lib = nullptr;
    void *comm = nullptr; /* ncclComm_t */
    struct uid { char internal[128]; };
    int (*get_uid)(uid *) = nullptr;
    int (*init_rank)(void **, int, uid, int) = nullptr;
    int (*nccl_all_gather)(const void *, void *, size_t, int, void *, void *) = nullptr;
    int (*nccl_send)(const void *, size_t, int, int, void *, void *) = nullptr;
    int (*nccl_recv)(void *, size_t, int, int, void *, void *) = nullptr;
    int (*nccl_group_start)() = nullptr;
    int (*nccl_group_end)() = nullptr;
    int (*destroy)(void *) = nullptr;
    const char *(*err)(int) = nullptr;
};

#if defined(__HIPCC__)
#include <dlfcn.h>
static bool rccl_bind(ocp_qp_gpu_comm *c)
{
    const char *names[] = {"librccl.so", "librccl.so.1"};
    for (const char *n : names)
        if ((c->lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break; /* already in the process (PyTorch's copy) */
    if (!c->lib)
    {
        const char *load[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : load)
            if ((c->lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    }
    if (!c->lib) { fprintf(stderr, "acados_amd: RCCL (librccl.so) cannot be loaded: %s\n", dlerror()); return false; }
    c->get_uid = (int (*)(ocp_qp_gpu_comm::uid *)) dlsym(c->lib, "ncclGetUniqueId");
    c->init_rank = (int (*)(void **, int, ocp_qp_gpu_comm::uid, int)) dlsym(c->lib, "ncclCommInitRank");
    c->nccl_all_gather = (int (*)(const void *, void *, size_t, int, void *, void *)) dlsym(c->lib, "ncclAllGather");
    c->nccl_send = (int (*)(const void *, size_t, int, int, void *, void *)) dlsym(c->lib, "ncclSend");
    c->nccl_recv = (int (*)(void *, size_t, int, int, void *, void *)) dlsym(c->lib, "ncclRecv");
    c->nccl_group_start = (int (*)()) dlsym(c->lib, "ncclGroupStart");
    c->nccl_group_end = (int (*)()) dlsym(c->lib, "ncclGroupEnd");
    c->destroy = (int (*)(void *)) dlsym(c->lib, "ncclCommDestroy");
    c->err = (const char *(*)(int)) dlsym(c->lib, "ncclGetErrorString");
    /* every entry the two gathers use is required HERE, on every rank alike: a rank that found out inside a collective
     * that it lacks ncclSend would leave while the others wait in the group (round-3 review) */
    if (!c->get_uid || !c->init_rank || !c->nccl_all_gather || !c->destroy || !c->nccl_send || !c->nccl_recv || !c->nccl_group_start
        || !c->nccl_group_end)
    {
        fprintf(stderr, "acados_amd: librccl.so lacks a collective / point-to-point entry point (ncclAllGather, ncclSend, ncclRecv, ncclGroupStart/End)\n");
        return false;
    }
    return true;
}

/* the RCCL rows of the transport table; ctx = the communicator.  ncclDataType_t: ncclInt32 = 2, ncclFloat64 = 8 (rccl.h) --
 * the table's dtype codes are those numbers */
static int rccl_report(ocp_qp_gpu_comm *c, int r, const char *what)
{
    if (r != 0) fprintf(stderr, "acados_amd: RCCL error %d (%s) in %s\n", r, c->err ? c->err(r) : "?", what);
    return r;
}
static int rccl_op_all_gather(void *ctx, const void *sendbuf, void *recvbuf, size_t count, int dtype, void *stream)
{
    ocp_qp_gpu_comm *c = (ocp_qp_gpu_comm *) ctx;
    return rccl_report(c, c->nccl_all_gather(sendbuf, recvbuf, count, dtype, c->comm, stream), "ncclAllGather");
}
static int rccl_op_send(void *ctx, const void *buf, size_t count, int dtype, int peer, void *stream)
{
    ocp_qp_gpu_comm *c = (ocp_qp_gpu_comm *) ctx;
    return rccl_report(c, c->nccl_send(buf, count, dtype, peer, c->comm, stream), "ncclSend");
}
static int rccl_op_recv(void *ctx, void *buf, size_t count, int dtype, int peer, void *stream)
{
    ocp_qp_gpu_comm *c = (ocp_qp_gpu_comm *) ctx;
    return rccl_report(c, c->nccl_recv(buf, count, dtype, peer, c->comm, stream), "ncclRecv");
}
static int rccl_op_group_start(void *ctx) { ocp_qp_gpu_comm *c = (ocp_qp_gpu_comm *) ctx; return rccl_report(c, c->nccl_group_start(), "ncclGroupStart"); }
static int rccl_op_group_end(void *ctx) { ocp_qp_gpu_comm *c = (ocp_qp_gpu_comm *) ctx; return rccl_report(c, c->nccl_group_end(), "ncclGroupEnd"); }

int ocp_qp_gpu_comm_unique_id(void *id128)
{
    ocp_qp_gpu_comm c;
    if (!rccl_bind(&c)) return -1;
    return rccl_report(&c, c.get_uid((ocp_qp_gpu_comm::uid *) id128), "ncclGetUniqueId") == 0 ? 0 : -1;
}

ocp_qp_gpu_comm *ocp_qp_gpu_comm_create(const void *id128, int n_ranks, int rank, int device)
try
{
    ocp_qp_gpu_comm *c = new ocp_qp_gpu_comm();
    if (!rccl_bind(c)) { delete c; return nullptr; }
    if (device >= 0) HIPCHK(hipSetDevice(device));
    HIPCHK(hipGetDevice(&c->device));
    c->n = n_ranks; c->rank = rank;
    ocp_qp_gpu_comm::uid id;
    memcpy(&id, id128, sizeof(id));
    const int r = c->init_rank(&c->comm, n_ranks, id, rank);
    if (r != 0)
    {
        fprintf(stderr, "acados_amd: ncclCommInitRank failed: %d (%s)\n", r, c->err ? c->err(r) : "?");
        delete c;
        return nullptr;
    }
    c->ops.ctx = c;
    c->ops.all_gather = rccl_op_all_gather;
    c->ops.send = rccl_op_send;
    c->ops.recv = rccl_op_recv;
    c->ops.group_start = rccl_op_group_start;
    c->ops.group_end = rccl_op_group_end;
    return c;
}
catch (const gqp_hip_failure &) { return nullptr; }
#else  /* host-simulation build of the CPU test tier: no RCCL; communicators come from ocp_qp_gpu_comm_create_from_ops */
int ocp_qp_gpu_comm_unique_id(void *) { return -1; }
ocp_qp_gpu_comm *ocp_qp_gpu_comm_create(const void *, int, int, int) { return nullptr; }
#endif

ocp_qp_gpu_comm *ocp_qp_gpu_comm_create_from_ops(const ocp_qp_gpu_comm_ops *ops, int n_ranks, int rank)
{
    if (!ops || !ops->all_gather || !ops->send || !ops->recv || !ops->group_start || !ops->group_end || n_ranks < 1 || rank < 0 || rank >= n_ranks)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_comm_create_from_ops: incomplete transport table or rank %d outside 0..%d\n", rank, n_ranks - 1);
        return nullptr;
    }
    ocp_qp_gpu_comm *c = new ocp_qp_gpu_comm();
    c->ops = *ops;
    c->n = n_ranks; c->rank = rank;
    return c;
}

void ocp_qp_gpu_comm_destroy(ocp_qp_gpu_comm *c)
{
    if (!c) return;
    if (c->comm && c->destroy) (void) c->destroy(c->comm);
    delete c;
}

/* The gather of the path.  root < 0: every rank receives everything; root >= 0: that rank only (the buffers of the other
 * ranks may be NULL).  counts: instances per rank (n_ranks entries) or NULL = b->B on every rank.  The receive buffers are
 * laid out in RANK ORDER, rank r's instances starting at instance offset sum(counts[0..r-1]):
 *     sol_all [sum counts][bulk_len(out)] doubles, info_all [sum counts][2] ints (status, iter), time_all [n_ranks] doubles.
 * Equal counts + all ranks receive: three ncclAllGather (ring over xGMI).  Otherwise -- gather to a root, or UNEVEN shards,
 * which ncclAllGather cannot express -- point-to-point sends / receives with their exact counts inside ONE group: to a
 * root every other rank moves 1x its payload instead of receiving n_ranks x (SURVEY 5 costs the 8-GPU C2 payload at 5.5 ms
 * this way against ~40 ms for the ring all-gather).  A transport error never leaves a group open: the group is always
 * ended before the error is returned (round-3 review). */
static int gather_impl(ocp_qp_gpu_batch *b, ocp_qp_gpu_comm *c, int root, const int *counts, double *sol_all, int *info_all, double *time_all)
{
    if (!c) return -1;
    HIPCHK(hipSetDevice(b->device));
    if (root >= c->n) { fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_gather: root %d outside 0..%d\n", root, c->n - 1); return -1; }
    if (counts && counts[c->rank] != b->B)
    {
        fprintf(stderr, "acados_amd: ocp_qp_gpu_batch_gather: counts[%d] = %d but this rank's batch holds %d instances\n", c->rank, counts[c->rank], b->B);
        return -1;
    }
    BulkMap &M = blob_map(b, BLOB_OUT);
    const int len = M.len;
    const size_t cnt = (size_t) b->B * len;
    /* send buffers: the solution blob of this rank (gather launch into the staging area), status / iter interleaved */
    double *blob = stage_out(b, nullptr, cnt + (size_t) b->B + 8, 0); /* doubles: blob + room for 2*B ints + the time */
    int *info = (int *) (blob + cnt);
    double *tm = blob + cnt + b->B + 1;
    bulk_gather_launch(b, blob, len, M.d_arr_g, M.d_elem_g, M.T);
    hipLaunchKernelGGL(gqp::k_pack_info, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, b->D, info);
    HIPCHK(hipMemcpyAsync(tm, &b->time_tot, sizeof(double), hipMemcpyHostToDevice, b->stream));
    bool even = true;
    if (counts) for (int r = 0; r < c->n; r++) even = even && counts[r] == b->B;
    const ocp_qp_gpu_comm_ops &T = c->ops;
    void *st = (void *) b->stream;
    int rc = 0;
    if (root < 0 && even)
    {
        if ((rc = T.all_gather(T.ctx, blob, sol_all, cnt, GQP_COMM_F64, st)) == 0
            && (rc = T.all_gather(T.ctx, info, info_all, 2 * (size_t) b->B, GQP_COMM_I32, st)) == 0)
            rc = T.all_gather(T.ctx, tm, time_all, 1, GQP_COMM_F64, st);
    }
    else
    {
        rc = T.group_start(T.ctx);
        if (rc != 0) return -1; /* no group was opened */
        for (int dst = 0; dst < c->n && rc == 0; dst++)
        {
            if (root >= 0 && dst != root) continue;
            if ((rc = T.send(T.ctx, blob, cnt, GQP_COMM_F64, dst, st)) == 0 && (rc = T.send(T.ctx, info, 2 * (size_t) b->B, GQP_COMM_I32, dst, st)) == 0)
                rc = T.send(T.ctx, tm, 1, GQP_COMM_F64, dst, st);
        }
        if (root < 0 || c->rank == root)
        {
            size_t off = 0; /* instances of the ranks before r */
            for (int r = 0; r < c->n && rc == 0; r++)
            {
                const size_t nr = counts ? (size_t) counts[r] : (size_t) b->B;
                if ((rc = T.recv(T.ctx, sol_all + off * len, nr * len, GQP_COMM_F64, r, st)) == 0
                    && (rc = T.recv(T.ctx, info_all + off * 2, nr * 2, GQP_COMM_I32, r, st)) == 0)
                    rc = T.recv(T.ctx, time_all + r, 1, GQP_COMM_F64, r, st);
                off += nr;
            }
        }
        const int re = T.group_end(T.ctx); /* always: an open group would swallow every later call of this process */
        if (rc == 0) rc = re;
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return rc == 0 ? 0 : -1;
}

int ocp_qp_gpu_batch_gather(ocp_qp_gpu_batch *b, ocp_qp_gpu_comm *c, double *sol_all, int *info_all, double *time_all)
try
{
    return gather_impl(b, c, -1, nullptr, sol_all, info_all, time_all);
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_gather_root(ocp_qp_gpu_batch *b, ocp_qp_gpu_comm *c, int root, double *sol_all, int *info_all, double *time_all)
try
{
    return gather_impl(b, c, root < 0 ? 0 : root, nullptr, sol_all, info_all, time_all);
}
catch (const gqp_hip_failure &) { return -1; }

int ocp_qp_gpu_batch_gather_v(ocp_qp_gpu_batch *b, ocp_qp_gpu_comm *c, int root, const int *counts, double *sol_all, int *info_all, double *time_all)
try
{
    return gather_impl(b, c, root, counts, sol_all, info_all, time_all);
}
catch (const gqp_hip_failure &) { return -1; }

size_t ocp_qp_gpu_batch_bytes(const ocp_qp_gpu_batch *b) { return b->bytes; }
void *ocp_qp_gpu_batch_stream(ocp_qp_gpu_batch *b) { return (void *) b->stream; }
const char *ocp_qp_gpu_batch_kernel_name(const ocp_qp_gpu_batch *b) { return b->fam.name.c_str(); }
const char *ocp_qp_gpu_batch_tail_kernel_name(const ocp_qp_gpu_batch *b)
{
    /* the tail hangs below the level that handed over (run_ipm): the batch itself, or the compaction level below it */
    for (; b; b = b->sub[SUB_COMPACT].c)
        if (b->sub[SUB_TAIL].c) return b->sub[SUB_TAIL].c->fam.name.c_str();
    return "";
}

} /* extern "C" */

#if defined(GQP_WPI_TIMING)
/* development aid (make timing): per-phase cycle counters of the wave-per-instance factor kernel */
extern "C" void gqp_wpi_cycles_read(unsigned long long *out, int reset)
{
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(gqp::gqp_wpi_cycles), sizeof(unsigned long long) * 16));
    if (reset)
    {
        unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gqp::gqp_wpi_cycles), z, sizeof(z)));
    }
}
#endif

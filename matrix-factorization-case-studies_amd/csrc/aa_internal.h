// aa_internal.h -- shared declarations of libaa_hip.so (gfx950 only).
//
// Data layout in HBM (all device buffers are zero-initialised, padded, and owned
// by the context):
//   X        [n_pad][ldx]   T (float|double)  row-major data (or kernel) matrix;
//                            n_pad = roundup(n,128), ldx = p_pad = roundup(p,128);
//                            padding rows/columns are ZERO so GEMM kernels need no
//                            bounds checks and padding never contributes to a sum.
//   "tall"   [n_pad][KP]    double            per-sample x per-component arrays:
//                            Ct (dictionary, TRANSPOSED: component on the fast axis),
//                            Z, D (search direction), G (C XX' or C K, transposed),
//                            g (gradient), H (XX'Z or KZ), XW ...   KP = 32 or 64.
//   "wide"   [KP][p_pad]    double (+ a T copy used as MFMA operand)
//                            P = C X, Q = D X, ZtX = Z'X, Wt.
//   small    [KP][KP]       double            Gram products.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aa_hip.h"
#include "dict_plan.h"
#include "gram_plan.h"
#include "group_plan.h"
#include "pass_plan.h"

namespace aa {

void set_error(const char *fmt, ...);

#define AA_CHECK_HIP(expr)                                                              \
    do {                                                                                \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess) {                                                        \
            aa::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,                 \
                          hipGetErrorString(e__));                                      \
            return AA_ERR_HIP;                                                          \
        }                                                                               \
    } while (0)

#define AA_CHECK(expr)                                                                  \
    do {                                                                                \
        int rc__ = (expr);                                                              \
        if (rc__ != AA_OK) return rc__;                                                 \
    } while (0)

#define AA_REQUIRE(cond, code, ...)                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            aa::set_error(__VA_ARGS__);                                                 \
            return code;                                                                \
        }                                                                               \
    } while (0)

inline long round_up(long v, long m) { return (v + m - 1) / m * m; }

// The polynomial kernel kappa(x, y) = (gamma x.y + coef0)^degree as a function of the dot product s = x.y.
// The only place the device evaluates it: the K V products, the distance column and the trace all call
// this, so they agree to the rounding of s.  The power is degree - 1 multiplications in a fixed order
// (no pow()): b = gamma s + coef0 (one fma), v = b, then v = v * b.
struct PolyKernel {
    double gamma, coef0;
    int degree;
};
__device__ __forceinline__ double poly_kappa(double s, const PolyKernel pk)
{
    const double b = fma(pk.gamma, s, pk.coef0);
    double v = b;
    for (int i = 1; i < pk.degree; ++i) v *= b;
    return v;
}

// A feature-space kernel that is never formed: its kind and parameters, host side.  A context holds two
// (Ctx::kernel, Ctx::cross).  Code that only asks whether a matrix is stored tests `kind` for non-zero; what
// depends on the formula switches on it.  The device takes gamma (RBF) or poly() (POLY) by value.
enum { IMPLICIT_RBF = 1, IMPLICIT_POLY = 2 };   // KernelSpec::kind
struct KernelSpec {
    int kind = 0;              // 0: none; RBF: exp(-gamma ||x - y||^2); POLY: poly_kappa(x.y, poly())
    double gamma = 0.0, coef0 = 0.0;
    int degree = 1;
    PolyKernel poly() const { return PolyKernel{gamma, coef0, degree}; }
    const char *name() const { return kind == IMPLICIT_POLY ? "polynomial" : "RBF"; }
    const char *stem() const { return kind == IMPLICIT_POLY ? "poly" : "rbf"; }   // aa_set_<stem>_reference, ...
    // what the kind's product kernels ask of the feature buffer: k_rbf_kv reads the features in pairs, the tile
    // body of k_poly_kv_mfma in chunks of 32 that must stay inside the zero-padded row
    long feat_ld(long p) const { return round_up(p, kind == IMPLICIT_POLY ? 32 : 2); }
    bool cross_reads_norms() const { return kind == IMPLICIT_RBF; }   // |y_r|^2 and |x_c|^2 beside the dot product
};
// gamma > 0 (both kinds), coef0 >= 0 (K positive semi-definite) and degree >= 1 (POLY), all finite (a NaN fails
// every comparison)
inline int kernel_spec_check(const KernelSpec &s)
{
    if (s.kind == IMPLICIT_RBF) AA_REQUIRE(s.gamma > 0.0 && s.gamma < 1e300, AA_ERR_ARG, "gamma must be positive");
    if (s.kind == IMPLICIT_POLY)
        AA_REQUIRE(s.gamma > 0.0 && s.gamma < 1e300 && s.coef0 >= 0.0 && s.coef0 < 1e300 && s.degree >= 1, AA_ERR_ARG,
                   "the polynomial kernel needs gamma > 0, coef0 >= 0 and degree >= 1 (finite); got %g, %g, %d", s.gamma,
                   s.coef0, s.degree);
    return AA_OK;
}

// zero rows allocated past n_pad in X and in every tall array, so software-pipelined
// kernels may prefetch past the end of their row range without a guard
#define AA_SLACK_ROWS 64

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool borrowed = false;     // aliases another context's buffer (aa_share_data): never freed here
    int alloc(size_t b)
    {
        if (b <= bytes && p && !borrowed) return AA_OK;
        release();
        if (b == 0) b = 16;
        AA_CHECK_HIP(hipMalloc(&p, b));
        bytes = b;
        // zero fill on the null stream, waited for: the contexts' streams are non-blocking (nothing
        // they run is ordered against the null stream), and allocations are rare
        AA_CHECK_HIP(hipMemsetAsync(p, 0, b, nullptr));
        AA_CHECK_HIP(hipStreamSynchronize(nullptr));
        return AA_OK;
    }
    void release()
    {
        if (p && !borrowed) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        borrowed = false;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};
// a DevBuf that lives for one call: released on scope exit, so its function returns through AA_CHECK /
// AA_CHECK_HIP wherever it fails.  (The members of Ctx are plain DevBufs: aa_ctx_destroy owns them.)
struct ScopedDevBuf : DevBuf {
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { release(); }
};

// ------------------------------------------------------------------ scalars
// Device-resident scalar state of the dictionary SPG solver and the projection
// passes.  Written by single-thread "scalar stage" kernels so the host does not
// have to synchronise inside an SPG iteration.
enum ScalarSlot {
    SC_TRACE = 0,   // tr(XX') or tr(K)
    SC_S1,          // tr(C * HD)            H = XX'Z or KZ
    SC_A0,          // tr(M * C K C')
    SC_F_OLD,
    SC_F_NEW,
    SC_ALPHA,       // BB step
    SC_ALPHA_SET,   // 0 => derive alpha from the first projected-gradient step
    SC_LAMBDA,
    SC_DELTA,       // <d, g>
    SC_DD,          // <d, d>
    SC_S1D,         // tr(D * HD)
    SC_A1,
    SC_A2,
    SC_DGN,         // <d, g_new>
    SC_RES2,        // ||res||^2
    SC_RESINF,
    SC_NFEVAL,
    SC_FLAGS,
    SC_PROJ_A,      // multiplier of g inside the current projection: w = x - a*g
    SC_AINV,        // max |P(x-g)-x|
    SC_FNORM,       // divisor of f (k in both forms)
    SC_FMEM0,       // f_mem[0..15]
    SC_COUNT = SC_FMEM0 + 16
};

struct ProjState {          // per projection, device memory
    double t[AA_MAX_K];
    double cnt[AA_MAX_K];
    int done;
    int passes;
    double mx[AA_MAX_K];          // column maxima of the current projection
    int shrunk[AA_MAX_K];         // the support has started to shrink (oscillation guard)
    double warm[4][AA_MAX_K];     // final thresholds of the previous projection of each kind
    // multi-rank list projection: a rank whose candidate list did not fit, or a union too long
    // for the solver, leaves a column unconverged.  The host checks that right away only while
    // the lists of that kind of projection are not known to be short; otherwise the check is
    // deferred to the next point where the host reads device state anyway (sticky flag).
    int overflow_sticky;          // set when any column of any projection was left unconverged
    int list_max[4];              // longest gathered list (over the columns) of the last projection per kind
    int fin_arrived;              // blocks of the running first / finish pass that have written their partials
                                  // (FinTail: the last one finalizes and puts it back to 0)
};

#define AA_SC_STRIDE 64      // doubles per slot of the per-slot scalar blocks (>= SC_COUNT)

struct IterState {          // device-side loop status of a fit (aa_iterate, aa_gpnh_iterate) or of a restart slot
    int stop, converged, error_stage, stop_iter, last_iter, spg_flags;
    int not_definite;       // GPNH: the normal equations of a dictionary update were not positive definite
    int pad1;
};

// The outer iteration's judge: the monotonicity check, then the stopping criterion
// (archetypal_analysis.py:167-197), evaluated on the device by one thread.  The rule is constant for a
// loop; the rest names the iteration judged.  Kernels take either part by value.
struct JudgeRule {
    double tol, mono_tol;
    int criterion, require, upd_dict, upd_w;
    int track_spg;          // an SPG run is behind the dictionary update: fold its flags into the status record
};
struct LoopJudge {
    JudgeRule rule;
    int on, it;             // on: a rule is set (a zeroed record judges nothing)
    double cost0;
    IterState *st;
};
// the only reader of the rule's fields of aa_iter_params (beside the argument checks)
inline LoopJudge loop_judge(const aa_iter_params *ip, int it, double cost0, IterState *st, int track_spg)
{
    LoopJudge jd;
    memset(&jd, 0, sizeof(jd));
    jd.rule.tol = ip->tolerance;
    jd.rule.mono_tol = ip->mono_tolerance;
    jd.rule.criterion = ip->criterion;
    jd.rule.require = ip->require_monotonic;
    jd.rule.upd_dict = ip->update_dictionary;
    jd.rule.upd_w = ip->update_weights;
    jd.rule.track_spg = track_spg;
    jd.on = 1;
    jd.it = it;
    jd.cost0 = cost0;
    jd.st = st;
    return jd;
}

// ------------------------------------------------------------------ context
struct Comm;   // RCCL wrapper (comm.hip)
struct P2P;    // one-shot peer-to-peer all-reduce over IPC-mapped buffers (comm.hip)

struct Ctx {
    int device = 0;
    int dtype = AA_F64;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;             // side stream: the QP's straggler kernel
    hipStream_t stream3 = nullptr;             // the live consumers of parked QP samples (qp_live): a queue of
                                               // their own, stream2 may still hold the residual projection
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    // restarts side by side, both families (aa_slots_*, aa_gpnh_slots_*): per-slot cost records, counters,
    // status, initial costs
    DevBuf slotCosts, slotCounters, slotStates, slotCost0;
    int slots_R = 0, slots_k = 0, slots_stride = 0, slots_max_outer = 0;
    // AA restarts side by side (aa_slots_*): the launchers of the coupled steps pick their per-slot
    // forms while this is set; per-slot SPG scalars [R][AA_SC_STRIDE]
    bool slots_aa = false, slots_started = false;
    unsigned slots_cold = 0;                   // slots loaded since the last iteration: their next dictionary
                                               // update is the cold one of a fit (projection of the caller's
                                               // factors, products recomputed); slots_cold_cols: their columns
    unsigned slots_cold_cols = 0xffffffffu;
    DevBuf slotSaveP, slotSaveGr;              // C X and (C X X')' of the running slots across a reload
    DevBuf slotSnapP;                          // C X of every slot at its stopping iteration
    aa_iter_params slots_ip;
    aa_spg_params slots_sp, slots_scale_sp;
    aa_gpnh_params slots_gp;
    aa_qp_params slots_qp;
    DevBuf qpLive;                             // ready[cap] | done[cap] flags of the live hand-over (QpLive)
    long qp_live_cap = 0;
    int qp_live_epoch = 0;
    char pass_names[2][48] = {{0}, {0}};       // last reduce-over-rows / row-local kernel launched (aa_pass_kernels)
    char qp_names[192] = {0};                  // what the last launch_qp launched, ';'-separated (aa_qp_kernels)
    char spg_path[512] = {0};                  // set-up and kernels of the latest dictionary update, ';'-separated (aa_spg_path)
    bool spg_path_full = false;                // an entry did not fit: the later ones are dropped too
    bool qp_tail_pending = false;              // stragglers run on stream2, results in tmpTall by slot
    // the residual projection of the dictionary SPG (spg.py:250-276: convergence flags only) runs on
    // the side stream beside the weights QP, on its own scratch set (launch_proj_side / join_side)
    hipEvent_t evFork2 = nullptr, evJoin2 = nullptr;
    bool qp_perm_ready = false;                // the previous QP launch of this context left the order of the next one in qpPerm (k_qp_wave_ord)
    long qp_perm_n = 0;
    bool side_pending = false;
    DevBuf tmpTall2, redPartial2, redOut2, proj2, projList2, projSegCnt2;
    int projPassHint2[4] = {0, 0, 0, 0};
    bool projWarm2[4] = {false, false, false, false};
    // measurement (aa_gemm_timing): HIP event pairs around every launch of the two pass kernels
    bool time_gemm = false;
    std::vector<hipEvent_t> gemmEvents[2];     // [0] reduce-over-rows, [1] row-local: start, stop, ...
    const int *qp_tail_rows = nullptr;         // device: overflow slot -> row
    const unsigned int *qp_tail_count = nullptr;   // device: number of overflow slots
    Comm *comm = nullptr;
    P2P *p2p = nullptr;
    int rank = 0, world = 1;
    bool force_comm = false;                   // AA_FORCE_RCCL=1: use RCCL even with one rank
    // multi-rank: small reductions that ride in the tail of the next all-reduce instead of having one of
    // their own (pack_comm).  ride_dst: where the rider's values go (the tail of a wide buffer, or the
    // second region of redGather); ride_count: doubles there; ride: the k_post step owed after the all-reduce
    struct RidePost {
        bool on = false;
        int kind = 0, mode = 0, NV = 0, slot = 0, gated = 0, stage_after = -1;
        unsigned max_mask = 0u;
        aa_spg_params sp;
        double *red = nullptr;
        ProjState *ps = nullptr;
        double *gather = nullptr;              // where its [world][NV][KP] values sit
        long count = 0;
    };
    RidePost ride, ride_grad;
    double *ride_dst = nullptr;                // explicit tail content of a wide buffer (Z'Z behind Z'X): its start
    long ride_count = 0;                       // ... and length
    double *ride_gather_next = nullptr;        // the next closing reduction of a projection goes here and waits (ride)
    // Who can read the tail of a one-iteration dictionary SPG (dict_plan.h: dict_tail_needed): the status record's
    // spg_flags as the host last fetched them (run_device_loop, once per batch; 0 at the start of a loop) -- once
    // they carry AA_SPG_FLAG_MAX_ITER no later residual projection changes what the fit reports.
    int loop_spg_flags = 0;
    bool ride_grad_next = false;               // the next launch_grad's dot rides with the projection that follows it

    // data
    int form = AA_FORM_DATA;
    long n = 0, n_pad = 0, p = 0, p_pad = 0, n_global = 0, row_offset = 0;
    DevBuf X;
    bool have_data = false;
    double trace = 0.0;
    bool have_trace = false;

    // problem
    int k = 0, KP = 0;
    bool have_state = false, grams_valid = false, gpnh_valid = false;
    std::vector<double> alpha;                 // host copy
    std::vector<double> ZtZ, CKCt, CKZ;        // host copies (k x k, dense k), fetched on demand
    bool dict_inputs_overridden = false;

    // tall arrays
    DevBuf Ct, Zt, Dt, Gr, Gn, gk, gn, H, tmpTall;
    // wide arrays
    DevBuf P, Q, ZtX, Pw, Qw;                  // Pw/Qw: T-typed MFMA operand copies
    DevBuf wideScratch;                        // KP x max(p_pad, n_pad) double
    // reduction scratch
    DevBuf partial;                            // GEMM split-row partials
    DevBuf groupFlags;                         // flagged reduce-over-rows: a byte per aligned group of 4 rows of the tall operand
    DevBuf slabMode;                           // ... a byte per slab (1: gathered, 0: dense), then the two slab counters
    DevBuf rlPartial;                          // row-local GEMM split over column chunks (short, wide data)
    DevBuf redPartial;                         // tall/wide reduction partials
    DevBuf gramOut;                            // up to 4 KPxKP results
    DevBuf gramState;                          // [3][KP*KP] on the device: Z'Z | C K C' | C K Z
    DevBuf costDev;                            // costs recorded by aa_outer_iterations
    DevBuf costSlot;                           // device counter: next free slot of costDev
    bool host_grams_valid = false;             // the host copies below match gramState
    DevBuf redOut;                             // finalized [NV][KP] reduction results
    DevBuf redGather;                          // multi-rank: [world][NV][KP] per-rank results
    DevBuf listGather;                         // multi-rank: [world][KP][cap + 1] candidate lists
    DevBuf scalars;                            // SC_COUNT doubles
    DevBuf proj;                               // ProjState
    DevBuf projList, projSegCnt;               // candidate lists of the column projection
    DevBuf Mdev, alphaDev;                     // KP*KP, KP
    DevBuf iterState, snapC, snapZ, snapAlpha; // aa_iterate: status record, factors at the stopping iteration
    DevBuf qpIters;                            // n ints: pass counts of the latest weights update
    DevBuf qpPerm;                             // n ints: sample order of the lane kernel
    DevBuf feat, featNorm;                     // implicit kernels: features [n_pad][feat_ld] (float64) and their squared norms
    long feat_p = 0, feat_ld = 0;
    KernelSpec kernel;                         // K_ij = kappa(x_i, x_j) of the features (aa_set_*_features); kind 0: none
    // KernelAA.transform on an implicit kernel (aa_set_rbf_reference, aa_set_poly_reference): the reference rows
    // X_S [cross_s_pad][p_pad], their squared norms (RBF), V = D' on them [cross_s_pad][KP], the squared norms of the
    // resident rows (also the linear kernel's diagonal), and the kernel-form cost's operands
    DevBuf crossX, crossNorm, crossV, rowNorm, xformCost;
    long cross_s = 0, cross_s_pad = 0;
    int cross_k = 0;
    KernelSpec cross;                          // the reference set's kernel, valid while cross_s > 0
    DevBuf scoreScratch;                       // aa_gpnh_residual_scores: [slab][p_pad] | [split][n_pad] partials, the sums, the total
    DevBuf fsScratch;                          // FurthestSum on the device: running sums, one distance column, state, alive flags
    // the layout of fsScratch as the latest selection on the current rows left it (aa_get_furthest_sum_state);
    // fs_k == 0: no selection since the last install
    int fs_k = 0;
    size_t fs_off_col = 0, fs_off_st = 0, fs_off_alive = 0;
    bool qp_iters_valid = false;               // qpIters belongs to the current rows / state
    bool linear_kernel = false;                // data form, KernelAA conventions: K = X X' implicit (aa_set_linear_kernel)
    DevBuf qpStats;                            // 2 long long
    void *hostPinned = nullptr;                // small pinned staging
    size_t hostPinnedBytes = 0;

    long nslab = 0, rows_per_slab = 0;         // reduce-over-rows decomposition
    int tallBlocks = 0;                        // blocks of the tall reductions
    int projPassHint[4] = {0, 0, 0, 0};        // Michelot passes the last projection of each kind needed
    bool projWarm[4] = {false, false, false, false};   // ProjState::warm[kind] is valid
    long projCounts[4] = {0, 0, 0, 0};         // launch_proj calls by strategy: small32, small64, list, iterative (aa_proj_counts)
    bool projListShort[4] = {false, false, false, false};   // multi-rank: gathered lists of this kind were <= a quarter of the solver's capacity at the last poll
    bool x_feasible = false;                   // dictionary known to be on the simplex
    bool products_valid = false;               // P (= CX) and Gr (= C XX' or C K) match Ct
    bool ckz_valid = false;                    // gramState's C K Z matches Ct and H
};

// What the latest dictionary update ran (aa_spg_path): a host-side string that dictionary_update, launch_grad and
// launch_linesearch_fused write beside their launches and nothing that launches reads.  From the first entry that
// does not fit on, entries are dropped whole (a long SPG run repeats its entries anyway).
void spg_name(Ctx *c, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#define SPG_NAME(...) spg_name(c, __VA_ARGS__)

// a stored matrix in data form: X holds the n x p rows themselves -- not a kernel matrix, and not nothing
// behind an implicit kernel.  (An implicit kernel always comes with form == AA_FORM_KERNEL: install_begin.)
inline bool has_stored_data(const Ctx *c) { return c->have_data && !c->kernel.kind && c->form == AA_FORM_DATA; }

// ------------------------------------------------------------------ kernels_gemm.hip
// out[KP][p_pad] (double) = sum_r A[r][i] * X[r][c];  A tall double, X T.
// Also refreshes the T-typed operand copy outT (may alias out when T == double).
// flag_buf (nullable; &c->groupFlags): the caller expects A_tall to be zero in most of its rows.  With
// option reduce_sparse the call then flags the operand's non-zero groups of 4 rows (launch_group_flags),
// gathers those in the slabs with at most reduce_sparse_max of them and runs the dense kernel on the
// other slabs only: the same bits as the plain call for finite X (kernels_gemm.hip).  While aa_gemm_timing is on
// the call is the plain one, so that the event pairs keep timing full passes.
int launch_reduce_rows(Ctx *c, const double *A_tall, double *out_wide, void *outT,
                       bool main_only = false, DevBuf *flag_buf = nullptr);
#define AA_SLAB_MODE_BYTES 256                 // Ctx::slabMode: a mode byte per slab (nslab <= 256), then two counters
static_assert(REDUCE_ROWS_MAX_SLABS <= AA_SLAB_MODE_BYTES, "a mode byte per slab");
// second stage of the split-row reduction (after a main_only launch): sums the slab partials
// plus `extra_slabs` further slabs appended by launch_reduce_rows_fixup
int launch_reduce_rows_finish(Ctx *c, double *out_wide, void *outT, int extra_slabs);
// appends sum_s (znew[s] - Z[rows[s]]) x_{rows[s]}' as QP_FIX_SLABS slabs of partials
int launch_reduce_rows_fixup(Ctx *c, const unsigned int *count_dev, const int *rows_dev,
                             const double *zslot, const double *Ztall);
// out[n_pad][KP] (double) = sum_c X[r][c] * B[i][c];  B wide, T-typed.
int launch_row_local(Ctx *c, const void *B_wideT, double *out_tall);
int launch_stream_probe(Ctx *c, int variant);   // measurement: one streaming read of X

// ------------------------------------------------------------------ kernels_tall.hip
int tall_setup(Ctx *c);
int launch_proj(Ctx *c, const double *x, const double *g, double a_const, int a_slot, int mode,
                const aa_spg_params *sp = nullptr, int stage_after = -1);
enum { PROJ_FEAS = 0, PROJ_ALPHA = 1, PROJ_DIR = 2, PROJ_RES = 3 };
// gout = (M Graw - H a) scale.  d_for_dot: <d, gout> goes to scalar slot dot_slot; xupd (needs d_for_dot):
// x += lambda d in the same pass; stage_after >= 0 (with sp): the scalar stage that consumes <d, g> (ST_BB) runs
// inside the finalize kernel; setup_sp: the dictionary update's set-up rides along as block 0 (DictSetup), with
// setup_fnorm its SC_FNORM
struct GradArgs {
    const double *Graw;
    double *gout;
    const double *d_for_dot = nullptr;
    int dot_slot = 0;
    double *xupd = nullptr;
    const aa_spg_params *sp = nullptr;
    int stage_after = -1;
    const aa_spg_params *setup_sp = nullptr;
    double setup_fnorm = 0.0;
};
int launch_grad(Ctx *c, const double *H, double scale, const GradArgs &a);
int launch_tall_axpy_lambda(Ctx *c, double *x, const double *d);             // x += lambda * d
// the same on the groups of 4 rows that launch_group_flags marked in d (Ctx::group_flags_fresh): the same bits
int launch_tall_axpy_lambda_flagged(Ctx *c, double *x, const double *d, const unsigned char *flags);
// flags[g] = 1 if any entry of rows 4g..4g+3 of the tall array compares != 0.0 (NaN does, -0.0 does not),
// g < n_pad / 4; also zeroes the two slab counters of the gather kernel that follows
int launch_group_flags(Ctx *c, const double *A_tall, unsigned char *flags, unsigned int *counters);
int launch_tall_dot_scaled(Ctx *c, const double *x, const double *H, const double *alpha_dev,
                           int slot);   // sum x*H*alpha (alpha_dev nullable => 1)
int launch_gram_tall(Ctx *c, const double *A, const double *B, double *out_dev, bool local_only = false);
int launch_ride_post(Ctx *c, Ctx::RidePost *rp, const double *gather);   // the k_post step a rider is owed
#define AA_WIDE_TAIL(KP) ((size_t)(KP) * (KP) + (size_t)64 * 4 * (KP))   // doubles behind a wide buffer for riders // A'B  (KPxKP)
int launch_gram_wide(Ctx *c, const double *A, const double *B, double *out_dev); // A B' (KPxKP)
int launch_scale_gram(Ctx *c, double *dst, const double *src);      // dst = D src D
// cost from gramState; with a counter: out_dev[(*counter)++]; with a judge: the outer iteration's judge
// rides in the kernel, behind the iteration's last cost
int launch_aa_cost(Ctx *c, double *out_dev, int *slot_counter_dev = nullptr, const LoopJudge *judge = nullptr);
int launch_set_scalars(Ctx *c, double trace, double fnorm);          // SC_TRACE, SC_FNORM
int launch_wide_axpy_lambda(Ctx *c, double *P, const double *Q, void *PT);   // P += lambda*Q; PT = T(P)
int launch_wide_to_T(Ctx *c, const double *src, void *dstT);
int launch_transpose_wide_to_tall(Ctx *c, const double *wide, double *tall); // [KP][p_pad] -> [n_pad][KP] (kernel form)
int launch_transpose_tall_to_wide(Ctx *c, const double *tall, double *wide, void *wideT);
int launch_scalar_stage(Ctx *c, int stage, const aa_spg_params *sp, int it);
int launch_linesearch_fused(Ctx *c, const aa_spg_params *sp, double *cost_out, int *cost_slot);
int launch_dict_setup(Ctx *c, const aa_spg_params *sp, double fnorm, unsigned slotmask = 0xffffffffu);
// the judge of iteration jd.it (judged: the cost kernel before it has run it already), then the conditional
// snapshot of the factors when the loop stopped at that iteration: Z and the dictionary -- C' with the scale
// factors (AA), or -- wide_dict -- W' (GPNH)
int launch_iter_judge(Ctx *c, const LoopJudge &jd, const double *costs, bool judged, bool wide_dict);
int launch_cost_carry(Ctx *c, double *costs, int *slot, double cost0);
// jd: iteration, initial cost and status record of the single fit (the slots take theirs from the slot
// records), and the rule whose monotonicity check follows the update
int launch_scale_factors(Ctx *c, const aa_spg_params *sp, double delta_box, const LoopJudge &jd,
                         const double *costs, const int *slot);
int launch_col_has_nan(Ctx *c, const void *raw_dev, int host_dtype, long ld, long n_total, long p_full,
                       const double *w_dev /*nullable*/, unsigned char *flags_dev);
int launch_gather_weight(Ctx *c, const void *raw_dev, int host_dtype, long ld, long row0, long n,
                         const int *idx_dev, long p_valid, const double *w_dev);
int launch_data_to_double(Ctx *c, double *out_dev);
// column moments of the resident matrix in two sweeps (float64 arithmetic, fixed summation order) and the
// affine row-block copy behind aa_set_data_rows_affine
#define AA_MOMENT_MAX_SLABS 2048
long moment_slab_rows(long n, long p_pad, long *nslab_out);          // rows per slab; *nslab_out <= min(n, AA_MOMENT_MAX_SLABS)
int launch_col_moments(Ctx *c, double *partial_dev /* nslab x p_pad */, double *mean_dev /* p_pad */,
                       double *var_dev /* p_pad, nullable */);
int launch_affine_rows(Ctx *c, const void *owner_X, long row0, const double *shift_dev /*nullable*/,
                       const double *scale_dev /*nullable*/);
// weighted column sums (at most AA_MAX_COEF_ROWS coefficient rows, on the f64 matrix cores) and the per-row model
// copy behind aa_data_weighted_column_sums / aa_data_grouped_sqdev / aa_set_data_rows_model
#define AA_MAX_COEF_ROWS 16
int launch_col_weighted_sums(Ctx *c, int G, const double *At_dev /* n x 16 */, const int *grp_dev /* n, nullable */,
                             const double *centre_dev /* Gc x p_pad, nullable: plain sums */,
                             double *partial_dev /* nslab x G x p_pad */, double *out_dev /* G x p_pad */);
int launch_model_rows(Ctx *c, const void *owner_X, long row0, const int *grp_dev, const double *shift_dev,
                      const double *icpt_dev, const double *slope_dev, const double *t_dev, const double *scale_dev,
                      void *dst = nullptr /* null: c->X; else a buffer of its layout (aa_time_kernel) */);
// slot-major sums and copy for up to AA_MAX_SLOTS row labels (kernels_slots.hip) behind aa_data_slot_sums /
// aa_set_data_rows_slots: a GroupPlan (group_plan.h) on the device -- rows: the row list by slot; chunks: (slot,
// begin, len) per chunk; chunk_first: G + 1
struct SlotPlanDev {
    const int *rows, *chunks, *chunk_first;
    long nchunk;
    int G;
};
int launch_slot_sums(Ctx *c, const SlotPlanDev &pd, const double *centre_dev /* G x p_pad, nullable: plain sums */,
                     double *partial_dev /* nchunk x p_pad */, double *out_dev /* G x p_pad */);
int launch_slot_rows(Ctx *c, const void *owner_X, long row0, const SlotPlanDev &pd, const double *shift_dev,
                     const double *scale_dev, void *dst = nullptr /* null: c->X; else a buffer of its layout */);
// row gather behind aa_set_data_take (idx_dev null: the rows in order) and the float64 feature buffer of an
// implicit kernel from a resident matrix; owner_dtype / owner_ld: element type and leading dimension of owner_X
int launch_gather_rows(Ctx *c, const void *owner_X, int owner_dtype, long owner_ld, const long *idx_dev,
                       void *dst = nullptr /* null: c->X; else a buffer of its layout (aa_time_kernel) */);
int launch_features_from_data(Ctx *c, const void *owner_X, int owner_dtype, long owner_ld, long n, long p, double *F,
                              long ldf);
int launch_gpnh_solve(Ctx *c, double lambda, int *ok_dev);
// R restarts side by side (kernels_tall.hip: RestartSlots); rule: what the slots' judges apply (what = 2; a
// zeroed one otherwise)
int launch_gpnh_solve_slots(Ctx *c, double lambda);
int launch_gpnh_cost_slots(Ctx *c, double lambda, unsigned mask, int what, const JudgeRule &rule, bool form_gram);
int launch_gpnh_snap_slots(Ctx *c);
int launch_aa_cost_slots(Ctx *c, int what, const JudgeRule &rule);
int launch_aa_snap_slots(Ctx *c);
int launch_qp_slots_aa(Ctx *c, const aa_qp_params *p);      // kernels_qp.hip: quad + wave kernels, grid.y = slot
int launch_qp_slots(Ctx *c, int R, int k, const double *gram_dev, const aa_qp_params *p);   // kernels_qp.hip
bool gpnh_cost_can_gram(const Ctx *c);
int launch_gpnh_cost(Ctx *c, double lambda, double *out_dev, int *slot_counter, bool from_wide = false,
                     bool gram_w = false, const LoopJudge *judge = nullptr);
enum { ST_INIT_F = 0, ST_ALPHA = 1, ST_LINESEARCH = 2, ST_BB = 3, ST_CONV = 4 };
int launch_row_sqnorm_sum(Ctx *c, double *trace_out_host);
int launch_distance_column(Ctx *c, long j_local, int owner_has_row, const double *xj_host, double *d_host);
int kernel_kv(Ctx *c, const double *V_tall, double *out_tall);   // out = K V for c->kernel (tall in, tall out)
int kernel_cross(Ctx *c);          // Gr (XW) = kappa(Y, X_S) V for c->cross and the reference set of aa_set_*_reference
int launch_poly_trace(Ctx *c, double *trace_out_host);   // sum_i poly_kappa(|x_i|^2) from featNorm, fixed order
int launch_row_norms(Ctx *c, const double *F, long ld, long p, long rows, double *nrm);   // nrm[r] = |F_r|^2
// sum_t (d_t - 2 z_t.XW_t + z_t' A z_t) over the resident rows (A: KP x KP device, d: device or null = 1;
// part: (n + 255) / 256 + 1 doubles of scratch)
int launch_kernel_transform_cost(Ctx *c, const double *A_dev, const double *d_dev, double *part, double *out_host);
// the same terms per sample (aa_kernel_sample_residuals): r_dev / dout_dev n doubles each, part 2 nb + 2 doubles
// (nb = (n + 255) / 256) whose last two receive sum r and sum d; kind: AA_DIAG_*, d_dev (GIVEN) / nrm_dev (POLY
// with c->cross.poly(), LINEAR: squared row norms) n doubles.  Launches only
int launch_kernel_sample_residuals(Ctx *c, const double *A_dev, int kind, const double *d_dev, const double *nrm_dev,
                                   double *r_dev, double *dout_dev, double *part);
int launch_furthest_sum(Ctx *c, int k, int start, const int *exclude_host, int n_ex, int extra_steps,
                        int *selected_host, int *tie_host);
// copies out of fsScratch (any pointer may be null); launches nothing
int fetch_furthest_sum_state(Ctx *c, double *sums, unsigned char *alive, double *column, int *cur, int *tie,
                             int *selected);
int launch_row_broadcast(Ctx *c, long j_local, bool own);
int launch_proj_side(Ctx *c, const double *x, const double *g, double a_const, int a_slot, int mode,
                     const aa_spg_params *sp, int stage_after);   // launch_proj on the side stream / scratch set
int join_side(Ctx *c);             // the main stream waits for a pending side-stream projection
// Copies and fills ORDERED ON THE CONTEXT'S STREAM.  The streams of a context are created
// hipStreamNonBlocking (round 4): the legacy null stream orders nothing for them any more, and a
// null-stream hipMemcpy in one context is no longer a barrier across every context of the process
// (worker threads of fit_restarts, stream capture).  ctx_memcpy: the side stream joined, the copy
// enqueued on the main stream, the host waits for it (the semantics the synchronous hipMemcpy had
// for this context).  ctx_memset: enqueued only -- whatever reads the buffer is enqueued behind it.
inline hipError_t ctx_memcpy(Ctx *c, void *dst, const void *src, size_t nbytes, hipMemcpyKind kind)
{
    if (join_side(c) != AA_OK) return hipErrorUnknown;
    hipError_t e = hipMemcpyAsync(dst, src, nbytes, kind, c->stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
}
inline hipError_t ctx_memcpy2d(Ctx *c, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                               size_t height, hipMemcpyKind kind)
{
    if (join_side(c) != AA_OK) return hipErrorUnknown;
    hipError_t e = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, c->stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
}
inline hipError_t ctx_memset(Ctx *c, void *dst, int value, size_t nbytes)
{
    return hipMemsetAsync(dst, value, nbytes, c->stream);
}
bool side_available(const Ctx *c);  // dict_side_available (dict_plan.h) of this context
int side_begin(Ctx *c);            // launch_* calls go to the side stream (own scratch set) until side_end
int side_begin_behind(Ctx *c);
int side_end(Ctx *c);
int proj_poll_multirank(Ctx *c);   // multi-rank: read the deferred overflow flag / list lengths (host sync point)   // multi-rank: row j -> wideScratch on every rank
int launch_residual_cost(Ctx *c, const double *Ztall, const double *Wwide, const double *alpha_dev,
                         double *out_host /* null: launches only (aa_time_kernel) */);
// column / row / total sums of squares of X - Z W' (Z = Zt, W = P) in one pass on the f64 matrix cores;
// host outputs nullable; fetch == false: launches only (aa_time_kernel)
int launch_residual_scores(Ctx *c, double *col_host, double *row_host, double *sse_host, bool fetch = true);

// ------------------------------------------------------------------ kernels_pca.hip
// G_dev ([pl.g_ld][pl.g_ld] doubles, whole 64 x 64 tiles) = Xc Xc' or Xc' Xc of c's stored matrix as gram_plan cut
// it; shift_dev: p_pad doubles, zero padded (all zero: no centring); partial_dev: pl.partial_bytes (one split: unused)
int launch_gram(Ctx *c, const GramPlan &pl, const double *shift_dev, double *partial_dev, double *G_dev);
// the projection behind aa_set_data_projected: rows [row0, row0 + n) of owner_X, centred by shift_dev (owner_ld
// doubles, zero padded), onto the q rows of V_dev ([project_v_rows(q)][owner_ld] doubles, zero padded) into
// dst ([.][dst_ld] of dst_dtype), rows < n and columns < q only
int project_v_rows(int q);
int launch_project_rows(Ctx *c, const void *owner_X, int owner_dtype, long owner_ld, long p, long row0, long n, int q,
                        const double *V_dev, const double *shift_dev, void *dst, long dst_ld, int dst_dtype);

// ------------------------------------------------------------------ kernels_qp.hip
// A_host (k x k) and bscale_host (k or null) come from the host, or -- A_host == nullptr --
// the Hessian is D G D with G = gram_dev (KP x KP, device) and D = bscale = alphaDev, set
// up by a kernel (no host synchronisation).  What it launches -- mapping, caps, sample order,
// continuation -- is decided by qp_plan (qp_plan.h) from the qp_* knobs and these arguments.
int launch_qp(Ctx *c, const double *A_host, const double *Btall, long stride_j, long stride_t,
              const double *bscale_host /*k or null*/, double *Ztall, int ldz, long n, int k,
              const aa_qp_params *p, int *iters_dev, aa_qp_stats *stats,
              const double *gram_dev = nullptr, bool defer_tail = false);
// defer_tail: the wave-per-sample kernel of the stragglers runs on the side stream and leaves
// its results in tmpTall, indexed by overflow slot (c->qp_tail_pending); the caller overlaps
// the reduce-over-rows pass of Z'X with it, then calls launch_qp_tail_fixup: it waits for
// the stragglers, adds sum_s (z_new - z_old)_s x_s' as QP_FIX_SLABS extra slabs of the
// split-row partials (device-side count, no host synchronisation) and commits z_new to Z.
// It is honoured only while the qp_overlap_tail knob is set: qp_plan asks the knob as well,
// and the one caller that passes defer_tail passes it by that knob.
#define QP_FIX_SLABS 32
int launch_qp_tail_fixup(Ctx *c, double *Ztall);
int launch_simplex_rows_generic(hipStream_t s, const double *in, double *out, long rows, long cols);

// process-wide knobs (aa_set_option; the table is in solver.hip)
extern int g_use_graph;                                                      // solver.hip
extern int g_proj_mode, g_proj_small, g_proj_list_cap, g_proj_check_always;  // kernels_tall.hip
extern int g_fuse_finalize, g_fin_in_last, g_gram_side, g_setup_in_grad;     // kernels_tall.hip
extern int g_pack_comm, g_pq_mfma;                                           // kernels_tall.hip
extern int g_proj_res_side, g_grad_side, g_spg_tail;                         // kernels_tall.hip
inline DictKnobs dict_knobs()                    // the knobs dict_plan (dict_plan.h) decides by, as they are now
{
    return DictKnobs{g_fuse_finalize, g_setup_in_grad, g_grad_side, g_spg_tail, g_pack_comm, g_proj_mode,
                     g_proj_res_side};
}
extern int g_row_local_variant, g_row_local_split, g_row_local_acc64, g_f64_mfma;   // kernels_gemm.hip
extern int g_reduce_sparse, g_reduce_sparse_max;                                    // kernels_gemm.hip
inline PassKnobs pass_knobs()                    // the knobs the pass plans (pass_plan.h) decide by, as they are now
{
    return PassKnobs{g_row_local_variant, g_row_local_acc64, g_row_local_split, g_f64_mfma, g_reduce_sparse,
                     g_reduce_sparse_max};
}
// launch_reduce_rows with a flag buffer takes its flagged sequence, i.e. leaves the group flags of its operand in
// that buffer: the plan's own predicate, for the callers that reuse the flags
inline bool reduce_rows_flags_operand(const Ctx *c)
{
    return reduce_rows_takes_flags(pass_knobs(), c->dtype == AA_F32, c->time_gemm);
}
extern int g_qp_pass_cap, g_qp_mode, g_qp_quad_cap, g_qp_sort;               // kernels_qp.hip
extern int g_qp_fused_order, g_qp_wave_lazy, g_qp_quad_lazy;                 // kernels_qp.hip
extern int g_qp_overlap_tail, g_qp_live;                                     // kernels_qp.hip

// ------------------------------------------------------------------ comm.hip
int comm_unique_id(void *id128);
int comm_init(Ctx *c, const void *id128, int rank, int world);
void comm_destroy(Ctx *c);
int comm_allreduce(Ctx *c, double *dev, long count, int op);   // in place, on c->stream
int p2p_export(Ctx *c, int world, void *handle64);   // this rank's receive buffer as an IPC handle
int p2p_init(Ctx *c, const void *handles, int rank, int world);   // handles: world x 64 bytes, in rank order
int p2p_check(Ctx *c);             // a kernel of the peer-to-peer all-reduce gave up waiting?

}  // namespace aa

// solver.hip -- host drivers of the device-resident solver and the extern "C" surface
// declared in include/aa_hip.h.
//
// Dictionary update = the reference's spg() (spg.py:46-283) specialised to the
// dictionary objective (archetypal_analysis.py:261-341), restated so that one SPG
// iteration costs TWO passes over X instead of the reference's seven:
//   * C X is linear in C:       (C + lam D) X = CX + lam DX            (one pass: DX)
//   * f is quadratic in C:      f(C + lam D) follows from tr(C H D), tr(D H D) and the
//                               k x k Grams of CX, DX -> every line-search trial is
//                               scalar arithmetic (stage kernels, kernels_tall.hip)
//   * the gradient at the accepted point needs (CX + lam DX) X'         (one pass)
//     and doubles as the C XX' the weights update consumes (archetypal_analysis.py:619)
//   * the gradient at the top of the next iteration (spg.py:176) is the one just
//     computed (spg.py:233).
// The reference's quirks are kept: f divides by k while the data-form gradient divides
// by n (archetypal_analysis.py:265 vs :297), f_mem starts as zeros (spg.py:153),
// sigma_one is an absolute bound (spg.py:28).
#include "aa_internal.h"

#include <climits>
#include <functional>
#include <mutex>

namespace aa {

int g_outer_nosync = 0;
int g_use_graph = 0;     // 1: aa_outer_iterations replays a captured pair of iterations (measured neutral)

static thread_local std::string g_err;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

static inline size_t esize(const Ctx *c) { return c->dtype == AA_F32 ? 4 : 8; }

// T-typed MFMA operand copy of a wide double array (aliases the array itself in f64)
static inline void *operandT(Ctx *c, DevBuf &dbl, DevBuf &shadow)
{
    return c->dtype == AA_F32 ? shadow.p : dbl.p;
}

static int ensure_problem(Ctx *c, int k)
{
    AA_REQUIRE(c->have_data, AA_ERR_STATE, "set_data must precede the factors");
    AA_REQUIRE(k >= 1 && k <= AA_MAX_K, AA_ERR_ARG,
               "n_components = %d unsupported by the HIP backend (1..%d)", k, AA_MAX_K);
    const int KP = k <= 32 ? 32 : 64;
    if (c->k == k && c->KP == KP && c->Ct.p) return AA_OK;
    c->k = k;
    c->KP = KP;
    const size_t tall = (size_t)(c->n_pad + AA_SLACK_ROWS) * KP * sizeof(double);
    const size_t wide = ((size_t)KP * c->p_pad + AA_WIDE_TAIL(KP)) * sizeof(double);   // (tail: riders of the all-reduce)
    DevBuf *talls[] = {&c->Ct, &c->Zt, &c->Dt, &c->Gr, &c->Gn, &c->gk, &c->gn, &c->H, &c->tmpTall};
    for (DevBuf *b : talls) {
        b->release();
        AA_CHECK(b->alloc(tall));
    }
    DevBuf *wides[] = {&c->P, &c->Q, &c->ZtX, &c->wideScratch};
    for (DevBuf *b : wides) {
        b->release();
        AA_CHECK(b->alloc(wide));
    }
    c->Pw.release();
    c->Qw.release();
    if (c->dtype == AA_F32) {
        AA_CHECK(c->Pw.alloc((size_t)KP * c->p_pad * sizeof(float)));
        AA_CHECK(c->Qw.alloc((size_t)KP * c->p_pad * sizeof(float)));
    }
    // split-row decomposition of the reduce-over-rows GEMM
    const PassSlabs slabs = pass_slabs(c->dtype == AA_F32, c->n_pad, c->p_pad);
    c->nslab = slabs.nslab;
    c->rows_per_slab = slabs.rows_per_slab;
    c->partial.release();
    AA_CHECK(c->partial.alloc((size_t)(c->nslab + QP_FIX_SLABS) * KP * c->p_pad * esize(c)));
    AA_CHECK(c->groupFlags.alloc((size_t)c->n_pad / 4 + AA_SLACK_ROWS));
    AA_CHECK(c->slabMode.alloc(AA_SLAB_MODE_BYTES + 2 * sizeof(unsigned int)));
    AA_CHECK(tall_setup(c));
    c->alpha.assign(k, 1.0);
    c->ZtZ.assign((size_t)k * k, 0.0);
    c->CKCt.assign((size_t)k * k, 0.0);
    c->CKZ.assign((size_t)k * k, 0.0);
    c->grams_valid = false;
    c->host_grams_valid = false;
    c->gpnh_valid = false;
    c->have_state = false;
    c->dict_inputs_overridden = false;
    return AA_OK;
}

static int upload_alpha(Ctx *c)
{
    std::vector<double> a(c->KP, 0.0);
    for (int i = 0; i < c->k; ++i) a[i] = c->alpha[i];
    AA_CHECK_HIP(ctx_memcpy(c, c->alphaDev.p, a.data(), a.size() * sizeof(double), hipMemcpyHostToDevice));
    return AA_OK;
}

// host k x k (dense) <- device KP x KP
static int fetch_gram(Ctx *c, const double *dev, std::vector<double> &out)
{
    std::vector<double> tmp((size_t)c->KP * c->KP);
    AA_CHECK_HIP(hipMemcpyAsync(tmp.data(), dev, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    out.resize((size_t)c->k * c->k);
    for (int i = 0; i < c->k; ++i)
        for (int j = 0; j < c->k; ++j) out[(size_t)i * c->k + j] = tmp[(size_t)i * c->KP + j];
    return AA_OK;
}

static int upload_tall(Ctx *c, DevBuf &dst, const double *src, long ld_row, long ld_col, long rows, int cols)
{
    // dst[r][i] = src[r*ld_row + i*ld_col], zero padded to [n_pad][KP]
    std::vector<double> tmp((size_t)c->n_pad * c->KP, 0.0);
    for (long r = 0; r < rows; ++r)
        for (int i = 0; i < cols; ++i) tmp[(size_t)r * c->KP + i] = src[r * ld_row + i * ld_col];
    AA_CHECK_HIP(ctx_memcpy(c, dst.p, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    return AA_OK;
}

static int download_tall(Ctx *c, const DevBuf &src, double *dst, long ld_row, long ld_col, long rows, int cols)
{
    std::vector<double> tmp((size_t)c->n_pad * c->KP);
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy(c, tmp.data(), src.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (long r = 0; r < rows; ++r)
        for (int i = 0; i < cols; ++i) dst[r * ld_row + i * ld_col] = tmp[(size_t)r * c->KP + i];
    return AA_OK;
}

// device-resident Gram state [Z'Z | C K C' | C K Z]; the host copies follow on demand
static inline double *dev_ZtZ(Ctx *c) { return c->gramState.as<double>(); }
static inline double *dev_CKCt(Ctx *c) { return c->gramState.as<double>() + (size_t)c->KP * c->KP; }
static inline double *dev_CKZ(Ctx *c) { return c->gramState.as<double>() + (size_t)2 * c->KP * c->KP; }

// C K Z = C' H (k x k) is only needed by the host (scale-factor update, aa_get_grams) and
// by the Gram form of the cost: after a dictionary update it is recomputed on demand
static int ensure_ckz(Ctx *c)
{
    if (c->ckz_valid) return AA_OK;
    AA_CHECK(launch_gram_tall(c, c->Ct.as<double>(), c->H.as<double>(), dev_CKZ(c)));
    c->ckz_valid = true;
    c->host_grams_valid = false;
    return AA_OK;
}

static int sync_host_grams(Ctx *c)
{
    AA_CHECK(ensure_ckz(c));
    if (c->host_grams_valid) return AA_OK;
    const size_t GS = (size_t)c->KP * c->KP;
    std::vector<double> tmp(3 * GS);
    AA_CHECK_HIP(hipMemcpyAsync(tmp.data(), c->gramState.p, tmp.size() * sizeof(double),
                                hipMemcpyDeviceToHost, c->stream));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    std::vector<double> *dst[3] = {&c->ZtZ, &c->CKCt, &c->CKZ};
    for (int m = 0; m < 3; ++m) {
        dst[m]->resize((size_t)c->k * c->k);
        for (int i = 0; i < c->k; ++i)
            for (int j = 0; j < c->k; ++j) (*dst[m])[(size_t)i * c->k + j] = tmp[m * GS + (size_t)i * c->KP + j];
    }
    c->host_grams_valid = true;
    return AA_OK;
}

// cost of the current state (archetypal_analysis.py:553-556), evaluated on the device
static int device_cost(Ctx *c, double *cost)
{
    AA_CHECK(c->costDev.alloc(64 * sizeof(double)));
    AA_CHECK(ensure_ckz(c));
    AA_CHECK(launch_aa_cost(c, c->costDev.as<double>()));
    AA_CHECK_HIP(hipMemcpyAsync(cost, c->costDev.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    return AA_OK;
}

static int ensure_trace(Ctx *c)
{
    if (c->have_trace) return AA_OK;
    if (c->kernel.kind == IMPLICIT_RBF) {    // every diagonal entry is exp(0) = 1
        c->trace = (double)c->n_global;
        c->have_trace = true;
        return AA_OK;
    }
    if (c->kernel.kind == IMPLICIT_POLY) {   // sum_i (gamma |x_i|^2 + coef0)^degree
        AA_CHECK(launch_poly_trace(c, &c->trace));
        c->have_trace = true;
        return AA_OK;
    }
    AA_CHECK(launch_row_sqnorm_sum(c, &c->trace));
    c->have_trace = true;
    return AA_OK;
}

// ----------------------------------------------------------------- Gram refresh
static int refresh_after_dictionary(Ctx *c, bool recompute_products, bool ckct_done = false)
{
    double *gpp = dev_CKCt(c);
    if (c->form == AA_FORM_DATA) {
        if (recompute_products) {
            AA_CHECK(launch_reduce_rows(c, c->Ct.as<double>(), c->P.as<double>(), operandT(c, c->P, c->Pw)));
            AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gr.as<double>()));
        }
        // the fused line search leaves (P + lam Q)(P + lam Q)' in the Gram state and the host
        // fetches C K Z on demand (ensure_ckz)
        if (ckct_done) {
            c->products_valid = true;
            c->ckz_valid = false;
            c->host_grams_valid = false;
            return AA_OK;
        }
        AA_CHECK(launch_gram_wide(c, c->P.as<double>(), c->P.as<double>(), gpp));
    } else {
        if (recompute_products && c->kernel.kind) {
            AA_CHECK(kernel_kv(c, c->Ct.as<double>(), c->Gr.as<double>()));      // (C K)' = K C'
        } else if (recompute_products) {
            AA_CHECK(launch_reduce_rows(c, c->Ct.as<double>(), c->wideScratch.as<double>(), nullptr));
            AA_CHECK(launch_transpose_wide_to_tall(c, c->wideScratch.as<double>(), c->Gr.as<double>()));
        }
        AA_CHECK(launch_gram_tall(c, c->Gr.as<double>(), c->Ct.as<double>(), gpp));
    }
    c->products_valid = true;
    AA_CHECK(launch_gram_tall(c, c->Ct.as<double>(), c->H.as<double>(), dev_CKZ(c)));
    c->ckz_valid = true;
    c->host_grams_valid = false;
    return AA_OK;
}

static int refresh_after_weights(Ctx *c)
{
    if (c->form == AA_FORM_DATA) {
        // Z'X.  When the QP's stragglers are still running on the side stream, the pass
        // over X starts with the Z of the lane kernel and the rows that change afterwards
        // enter as a rank-m correction (launch_qp_tail_fixup), so the latency-bound tail of
        // the weights update hides behind an HBM-bound pass.
        const bool tail = c->qp_tail_pending;
        // Z'Z needs the weights only: on the side stream, beside the HBM-bound pass, instead of 16 us of
        // two small launches between the two passes (joined below, with the dictionary's side work)
        const bool multi = c->world > 1 || c->force_comm;
        const bool pack = multi && g_pack_comm;         // Z'Z rides in the tail of the Z'X all-reduce
        const bool gram_on_side = g_gram_side && !tail && !c->slots_aa && side_available(c);
        if (gram_on_side) {
            AA_CHECK(side_begin_behind(c));
            const int rc = launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), dev_ZtZ(c));
            AA_CHECK(side_end(c));
            AA_CHECK(rc);
        }
        AA_CHECK(launch_reduce_rows(c, c->Zt.as<double>(), c->ZtX.as<double>(), operandT(c, c->ZtX, c->Qw), true));
        if (tail) AA_CHECK(launch_qp_tail_fixup(c, c->Zt.as<double>()));
        if (pack) {
            double *tailp = c->ZtX.as<double>() + (size_t)c->KP * c->p_pad;
            AA_CHECK(launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), tailp, true));
            c->ride_dst = tailp;
            c->ride_count = (long)c->KP * c->KP;
        }
        AA_CHECK(launch_reduce_rows_finish(c, c->ZtX.as<double>(), operandT(c, c->ZtX, c->Qw),
                                           tail ? QP_FIX_SLABS : 0));
        if (pack)
            AA_CHECK_HIP(hipMemcpyAsync(dev_ZtZ(c), c->ZtX.as<double>() + (size_t)c->KP * c->p_pad,
                                        (size_t)c->KP * c->KP * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        else if (!gram_on_side) AA_CHECK(launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), dev_ZtZ(c)));
        AA_CHECK(join_side(c));                  // the side stream's gradient kernel reads the old H and updates C
        AA_CHECK(launch_row_local(c, operandT(c, c->ZtX, c->Qw), c->H.as<double>()));
    } else {
        if (c->qp_tail_pending) AA_CHECK(launch_qp_tail_fixup(c, c->Zt.as<double>()));   // not used
        AA_CHECK(launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), dev_ZtZ(c)));
        if (c->kernel.kind) {
            AA_CHECK(kernel_kv(c, c->Zt.as<double>(), c->H.as<double>()));       // K Z
        } else {
            AA_CHECK(launch_transpose_tall_to_wide(c, c->Zt.as<double>(), c->ZtX.as<double>(),
                                                   operandT(c, c->ZtX, c->Qw)));
            AA_CHECK(launch_row_local(c, operandT(c, c->ZtX, c->Qw), c->H.as<double>()));
        }
    }
    AA_CHECK(launch_gram_tall(c, c->Ct.as<double>(), c->H.as<double>(), dev_CKZ(c)));
    c->ckz_valid = true;
    c->host_grams_valid = false;
    c->dict_inputs_overridden = false;
    return AA_OK;
}

static int prepare(Ctx *c, double *cost)
{
    AA_REQUIRE(c->have_state, AA_ERR_STATE, "set_state must precede prepare");
    AA_CHECK(ensure_trace(c));
    AA_CHECK(upload_alpha(c));
    AA_CHECK(refresh_after_weights(c));          // ZtZ, H = XX'Z (or KZ), CKZ (overwritten below)
    AA_CHECK(refresh_after_dictionary(c, true)); // CX, C XX', C XX' C', C XX' Z
    c->grams_valid = true;
    if (cost) AA_CHECK(device_cost(c, cost));
    return AA_OK;
}

// ----------------------------------------------------------------- restart slots: mixed cold / warm groups
// A slot that has just been loaded (slots_cold) goes through the COLD dictionary update of a fit --
// factors projected, C X, (C X)(C X)' and C X X' recomputed -- while the other slots of the group
// are in the middle of theirs and must keep the products they carry (C X is updated as P + lambda Q:
// recomputing it gives other bits).  The recomputing kernels run on the stacked arrays; these
// helpers put the warm slots' parts back afterwards.
static unsigned slots_all_mask(const Ctx *c) { return c->slots_R >= 32 ? 0xffffffffu : ((1u << c->slots_R) - 1u); }
static bool slots_mixed(const Ctx *c) { return c->slots_aa && c->slots_cold != 0 && c->slots_cold != slots_all_mask(c); }

static int slots_save_P(Ctx *c)
{
    const size_t wide = (size_t)c->KP * c->p_pad * sizeof(double);
    AA_CHECK(c->slotSaveP.alloc(wide));
    AA_CHECK_HIP(hipMemcpyAsync(c->slotSaveP.p, c->P.p, wide, hipMemcpyDeviceToDevice, c->stream));
    return AA_OK;
}
static int slots_restore_P_warm(Ctx *c)
{
    const int k = c->slots_k;
    for (int r = 0; r < c->slots_R; ++r) {
        if ((c->slots_cold >> r) & 1u) continue;
        const size_t off = (size_t)r * k * c->p_pad;
        AA_CHECK_HIP(hipMemcpyAsync(c->P.as<double>() + off, c->slotSaveP.as<double>() + off,
                                    (size_t)k * c->p_pad * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    if (c->dtype == AA_F32) AA_CHECK(launch_wide_to_T(c, c->P.as<double>(), operandT(c, c->P, c->Pw)));
    return AA_OK;
}

// ----------------------------------------------------------------- dictionary SPG
// What launches is decided by dict_plan (dict_plan.h) from the knobs and the facts of the call; the functions
// below run the plan and ask nothing else.
//
// What the caller knows about an update.  cost_out / cost_slot (device, nullable): where the cost after the
// update is recorded.  *cost_recorded tells the caller whether that happened inside the update (fused line
// search, one SPG iteration) or is still to be done with launch_aa_cost.  weights_follow, loop_update,
// loop_judged: see DictPlanIn.
struct DictCall {
    bool refresh = true;
    double *cost_out = nullptr;
    int *cost_slot = nullptr;
    bool *cost_recorded = nullptr;
    bool weights_follow = false, loop_update = false, loop_judged = false;
};

static DictPlanIn dict_plan_in(const Ctx *c, const aa_spg_params *sp, const aa_spg_stats *st, const DictCall &call)
{
    DictPlanIn in{};
    in.form = c->form == AA_FORM_DATA ? (c->linear_kernel ? DictForm::data_as_kernel : DictForm::data)
              : c->kernel.kind ? DictForm::implicit_kernel : DictForm::kernel_matrix;
    in.slots_aa = c->slots_aa;
    in.slots_mixed = slots_mixed(c);
    in.multi = c->world > 1 || c->force_comm;
    in.x_feasible = c->x_feasible;
    in.products_valid = c->products_valid;
    in.grams_valid = c->grams_valid;
    in.ckz_valid = c->ckz_valid;
    in.dict_inputs_overridden = c->dict_inputs_overridden;
    in.stats = st != nullptr;
    in.cost_dst = call.cost_out != nullptr;
    in.max_iterations = sp->max_iterations;
    in.max_feval = sp->max_feval;
    in.alpha0_negative = sp->alpha0 < 0.0;
    in.weights_follow = call.weights_follow;
    in.loop_update = call.loop_update;
    in.loop_judged = call.loop_judged;
    in.max_iter_seen = (c->loop_spg_flags & AA_SPG_FLAG_MAX_ITER) != 0;
    in.side_resources = c->stream2 && c->proj2.p && c->evFork2;
    in.flags_operand = reduce_rows_flags_operand(c);
    return in;
}

// The start (DictPlan::start): M, the scalars, f(x) and the products the first gradient reads.
static int dict_start(Ctx *c, const DictPlan &pl, const aa_spg_params *sp)
{
    const double fnorm = (double)c->k;
    if (pl.start == DictStart::fast_in_grad) return AA_OK;          // block 0 of the gradient launch does it
    if (pl.start == DictStart::fast_setup) return launch_dict_setup(c, sp, fnorm);      // spg.py:153-157
    const bool warm = pl.start == DictStart::warm;
    double *x = c->Ct.as<double>();
    double *gram = c->gramOut.as<double>();
    // M = D Z'Z D  (archetypal_analysis.py:310,330), formed on the device
    AA_CHECK(launch_scale_gram(c, c->Mdev.as<double>(), dev_ZtZ(c)));
    AA_CHECK(launch_set_scalars(c, c->trace, fnorm));              // archetypal_analysis.py:265,277
    if (pl.project_start) AA_CHECK(launch_proj(c, x, nullptr, 0.0, -1, PROJ_FEAS));
    if (warm) {
        AA_CHECK_HIP(hipMemcpyAsync(gram, dev_CKCt(c), (size_t)c->KP * c->KP * sizeof(double),
                                    hipMemcpyDeviceToDevice, c->stream));
    } else if (pl.data) {
        if (pl.save_restore_P) AA_CHECK(slots_save_P(c));
        AA_CHECK(launch_reduce_rows(c, x, c->P.as<double>(), operandT(c, c->P, c->Pw)));
        if (pl.save_restore_P) AA_CHECK(slots_restore_P_warm(c));
        AA_CHECK(launch_gram_wide(c, c->P.as<double>(), c->P.as<double>(), gram));
    } else {
        if (pl.implicit) {
            AA_CHECK(kernel_kv(c, x, c->Gr.as<double>()));
        } else {
            AA_CHECK(launch_reduce_rows(c, x, c->wideScratch.as<double>(), nullptr));
            AA_CHECK(launch_transpose_wide_to_tall(c, c->wideScratch.as<double>(), c->Gr.as<double>()));
        }
        AA_CHECK(launch_gram_tall(c, c->Gr.as<double>(), x, gram));
    }
    AA_CHECK(launch_tall_dot_scaled(c, x, c->H.as<double>(), c->alphaDev.as<double>(), SC_S1));
    AA_CHECK(launch_scalar_stage(c, ST_INIT_F, sp, 0));                         // spg.py:156
    // the slots that are in the middle of their fits start this update the way they always do
    if (pl.warm_slots_setup) AA_CHECK(launch_dict_setup(c, sp, fnorm, slots_all_mask(c) & ~c->slots_cold));
    if (pl.data && !warm) AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gr.as<double>()));
    return AA_OK;
}

// One SPG iteration up to the accepted step length: the direction d = P(x - alpha g) - x, its products and the
// line search.
static int dict_direction_linesearch(Ctx *c, const DictPlan &pl, const aa_spg_params *sp, const DictCall &call)
{
    const int KP = c->KP;
    const size_t GS = (size_t)KP * KP;
    double *x = c->Ct.as<double>();
    double *gram = c->gramOut.as<double>();
    // multi-rank: the closing reduction of this projection (<d,g>, <d,d>, ...: read by the line search
    // only) rides with the all-reduce of Q = D'X
    if (pl.ride_dir) c->ride_gather_next = c->Q.as<double>() + (size_t)KP * c->p_pad;
    AA_CHECK(launch_proj(c, x, c->gk.as<double>(), 0.0, SC_ALPHA, PROJ_DIR));   // spg.py:191-194,206
    if (pl.data) {
        // d = P(x - alpha g) - x is zero outside supp(x) and supp(P(.)): a few hundred rows
        AA_CHECK(launch_reduce_rows(c, c->Dt.as<double>(), c->Q.as<double>(), nullptr, false, &c->groupFlags));
        if (pl.line_search == DictLineSearch::fused) {
            // (P Q'), (Q Q'), the line search, the Gram of the accepted point and -- with one
            // SPG iteration per update -- the cost after the update: one launch
            AA_CHECK(launch_linesearch_fused(c, sp, pl.record_cost ? call.cost_out : nullptr,
                                             pl.record_cost ? call.cost_slot : nullptr));
            if (pl.record_cost && call.cost_recorded) *call.cost_recorded = true;
        } else {
            AA_CHECK(launch_gram_wide(c, c->P.as<double>(), c->Q.as<double>(), gram + GS));
            AA_CHECK(launch_gram_wide(c, c->Q.as<double>(), c->Q.as<double>(), gram + 2 * GS));
            AA_CHECK(launch_scalar_stage(c, ST_LINESEARCH, sp, 1));
            SPG_NAME("k_gram_wide<%d>x2;k_scalar_stage", KP);
        }
        return AA_OK;
    }
    if (pl.implicit) {
        AA_CHECK(kernel_kv(c, c->Dt.as<double>(), c->Gn.as<double>()));          // (D K)' = K D'
    } else {
        AA_CHECK(launch_reduce_rows(c, c->Dt.as<double>(), c->wideScratch.as<double>(), nullptr, false,
                                    &c->groupFlags));
        AA_CHECK(launch_transpose_wide_to_tall(c, c->wideScratch.as<double>(), c->Gn.as<double>()));
    }
    AA_CHECK(launch_gram_tall(c, c->Gn.as<double>(), x, gram + GS));
    AA_CHECK(launch_gram_tall(c, c->Gn.as<double>(), c->Dt.as<double>(), gram + 2 * GS));
    AA_CHECK(launch_gram_tall(c, c->Gr.as<double>(), c->Dt.as<double>(), gram + 3 * GS));
    AA_CHECK(launch_scalar_stage(c, ST_LINESEARCH, sp, 0));
    SPG_NAME("k_gram_tall<%d>x3;k_scalar_stage", KP);
    return AA_OK;
}

// The step x += lambda d and the tail of the iteration (DictPlan::tail): g_new with <d, g_new>, the BB stage
// (spg.py:232-244) and the residual projection (spg.py:250-276).  Leaves the new products and gradient in Gr, gk.
static int dict_tail(Ctx *c, const DictPlan &pl, const aa_spg_params *sp, double gscale)
{
    const int KP = c->KP;
    double *x = c->Ct.as<double>();
    GradArgs g{pl.data ? c->Gn.as<double>() : c->Gr.as<double>(), c->gn.as<double>()};
    g.d_for_dot = c->Dt.as<double>();
    g.dot_slot = SC_DGN;
    g.sp = sp;
    g.stage_after = ST_BB;
    if (pl.data) {
        AA_CHECK(launch_wide_axpy_lambda(c, c->P.as<double>(), c->Q.as<double>(), operandT(c, c->P, c->Pw)));
        if (pl.tail_skipped()) {
            // Nobody reads the tail (dict_tail_needed): the step x += lambda d is all that is left of it, on the
            // main stream -- C K Z of the refresh after the weights update is its first reader -- and on the
            // row groups the D'X pass flagged in d where it did (the same bits: k_tall_axpy_flagged).  No
            // fork, nothing for refresh_after_weights to join, and the QP has the CUs to itself.  g_new, the
            // BB scalars, ||res|| and the flags of the tail keep what an earlier update left there.
            if (pl.tail == DictTail::skip_flagged)
                AA_CHECK(launch_tall_axpy_lambda_flagged(c, x, c->Dt.as<double>(), c->groupFlags.as<unsigned char>()));
            else
                AA_CHECK(launch_tall_axpy_lambda(c, x, c->Dt.as<double>()));
            AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gn.as<double>()));
            // (not an SPG_NAME: the step tables of tests/test_spg_step_host.py hold the names of a whole step)
            spg_name(c, "tail:skip");
            std::swap(c->Gr, c->Gn);
            std::swap(c->gk, c->gn);
            return AA_OK;
        }
        AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gn.as<double>()));
        // With one SPG iteration per update nobody on the main stream waits for g_new, the step
        // x += lambda d, the BB stage or the residual projection before the update of the
        // weights has run (the QP reads C XX' and the Gram of the accepted point only): the whole
        // tail of the SPG iteration goes to the side stream and runs beside the QP (round 4:
        // 36 + 14 us of gradient kernel and finalize step off the critical path).  Joined in
        // refresh_after_weights before H = X (X'Z)' is overwritten (the gradient reads the old
        // H) and before C K Z is formed from the updated C.
        if (pl.tail == DictTail::side_whole) AA_CHECK(side_begin(c));
        // multi-rank: <d, g_new> rides with the first reduction of the residual projection below
        if (pl.ride_grad) c->ride_grad_next = true;
        // x = x_old + lam d happens inside the gradient kernel (it reads d for <d, g_new>),
        // the BB stage in the last block of that kernel
        g.xupd = x;
    } else {
        AA_CHECK(launch_tall_axpy_lambda(c, x, c->Dt.as<double>()));            // x = x_old + lam d
        AA_CHECK(launch_tall_axpy_lambda(c, c->Gr.as<double>(), c->Gn.as<double>()));
    }
    AA_CHECK(launch_grad(c, c->H.as<double>(), gscale, g));
    // multi-rank, a weights update next: the closing sums of the residual projection (convergence flags
    // only: read by the judge behind the weights update) wait for the Z'X all-reduce and ride behind Z'Z
    if (pl.ride_res) c->ride_gather_next = c->ZtX.as<double>() + (size_t)KP * c->p_pad + (size_t)KP * KP;
    // with one SPG iteration per update nobody waits for the flags: side stream
    if (pl.tail == DictTail::side_whole) {
        const int rc = launch_proj(c, x, c->gn.as<double>(), 1.0, -1, PROJ_RES, sp, ST_CONV);
        AA_CHECK(side_end(c));
        AA_CHECK(rc);
    } else if (pl.tail == DictTail::side_proj)
        AA_CHECK(launch_proj_side(c, x, c->gn.as<double>(), 1.0, -1, PROJ_RES, sp, ST_CONV));
    else
        AA_CHECK(launch_proj(c, x, c->gn.as<double>(), 1.0, -1, PROJ_RES, sp, ST_CONV));
    if (pl.data) std::swap(c->Gr, c->Gn);
    std::swap(c->gk, c->gn);
    return AA_OK;
}

static int dictionary_update(Ctx *c, const aa_spg_params *sp, aa_spg_stats *st, const DictCall &call)
{
    AA_REQUIRE(c->have_state && (c->grams_valid || c->dict_inputs_overridden), AA_ERR_STATE,
               "dictionary_update needs prepare() or set_dictionary_inputs() first");
    AA_REQUIRE(sp->max_iterations >= 1, AA_ERR_ARG, "spg max_iterations must be >= 1");
    AA_REQUIRE(sp->memory <= 16, AA_ERR_ARG,
               "spg memory = %d exceeds the HIP backend limit of 16", sp->memory);
    const DictPlan pl = dict_plan(dict_knobs(), dict_plan_in(c, sp, st, call));
    if (call.cost_recorded) *call.cost_recorded = false;
    AA_CHECK(join_side(c));

    double *x = c->Ct.as<double>();
    const double gscale = 1.0 / (pl.scale_by_n ? (double)c->n_global : (double)c->k);
    c->spg_path[0] = 0;
    c->spg_path_full = false;
    if (pl.start == DictStart::fast_in_grad) SPG_NAME("fast:in_grad");
    else if (pl.start == DictStart::fast_setup) SPG_NAME("fast:k_dict_setup");
    else if (pl.start == DictStart::warm) SPG_NAME("warm");
    else SPG_NAME("cold");
    AA_CHECK(dict_start(c, pl, sp));
    c->products_valid = false;
    GradArgs g0{c->Gr.as<double>(), c->gk.as<double>()};
    if (pl.start == DictStart::fast_in_grad) {
        g0.setup_sp = sp;
        g0.setup_fnorm = (double)c->k;
    }
    AA_CHECK(launch_grad(c, c->H.as<double>(), gscale, g0));

    std::vector<double> sc(SC_COUNT, 0.0);
    int n_iter = -1, flags = 0;
    for (int it = 0; it < sp->max_iterations; ++it) {
        n_iter = it;
        if (it == 0 && pl.alpha_first)                                          // spg.py:178-189
            AA_CHECK(launch_proj(c, x, c->gk.as<double>(), 1.0, -1, PROJ_ALPHA, sp, ST_ALPHA));
        AA_CHECK(dict_direction_linesearch(c, pl, sp, call));
        AA_CHECK(dict_tail(c, pl, sp, gscale));
        if (pl.tail_skipped()) break;
        if (pl.read_back(it)) {
            AA_CHECK_HIP(hipMemcpyAsync(sc.data(), c->scalars.p, SC_COUNT * sizeof(double),
                                        hipMemcpyDeviceToHost, c->stream));
            AA_CHECK_HIP(hipStreamSynchronize(c->stream));
            AA_CHECK(proj_poll_multirank(c));
            flags = (int)sc[SC_FLAGS];
            if (flags & (AA_SPG_FLAG_CONVERGED | AA_SPG_FLAG_MAX_FEVAL)) break;
        }
    }
    if (n_iter == sp->max_iterations - 1 && !(flags & AA_SPG_FLAG_CONVERGED))
        flags |= AA_SPG_FLAG_MAX_ITER;                                          // spg.py:278-281
    if (st) {
        st->f = sc[SC_F_OLD];
        st->n_iter = n_iter;
        st->n_feval = (int)sc[SC_NFEVAL];
        st->flags = flags;
        st->res_norm = sqrt(sc[SC_RES2]);
    }
    c->x_feasible = true;
    if (call.refresh) AA_CHECK(refresh_after_dictionary(c, false, pl.ckct_done));
    return AA_OK;
}

static int weights_update(Ctx *c, const aa_qp_params *qp, aa_qp_stats *stats)
{
    AA_REQUIRE(c->have_state && c->grams_valid, AA_ERR_STATE, "weights_update needs prepare() first");
    // Hessian D C K C' D (archetypal_analysis.py:387) and b-scale D are set up on the device
    const bool defer = g_qp_overlap_tail && c->form == AA_FORM_DATA;
    AA_CHECK(c->qpIters.alloc((size_t)c->n * sizeof(int)));
    if (c->slots_aa) {                           // restarts side by side: one QP per sample and slot
        AA_CHECK(launch_qp_slots_aa(c, qp));
        c->qp_iters_valid = false;
        AA_CHECK(refresh_after_weights(c));
        AA_CHECK(join_side(c));
        return AA_OK;
    }
    AA_CHECK(launch_qp(c, nullptr, c->Gr.as<double>(), 1, c->KP, nullptr, c->Zt.as<double>(), c->KP, c->n,
                       c->k, qp, c->qpIters.as<int>(), stats, dev_CKCt(c), defer));
    c->qp_iters_valid = true;
    AA_CHECK(refresh_after_weights(c));
    AA_CHECK(join_side(c));                      // the judge behind this update reads the SPG flags
    return AA_OK;
}

}  // namespace aa

// ===========================================================================
// extern "C"
// ===========================================================================
using namespace aa;

struct aa_ctx {
    Ctx c;
};

extern "C" {

const char *aa_last_error(void) { return g_err.c_str(); }
int aa_version(void) { return 100; }

// One row per knob.  flag: any value is accepted and stored as value != 0; otherwise the value must lie
// in lo..hi.  The option comment of include/aa_hip.h lists exactly these names (tests/test_cpu_host.py).
struct AaOption {
    const char *name;
    int *target;
    int lo, hi;
    bool flag;
};
static const AaOption kOptions[] = {
    {"row_local_variant", &g_row_local_variant, -1, 9, false},
    {"row_local_acc64", &g_row_local_acc64, 0, 2, false},
    {"row_local_split", &g_row_local_split, 0, 1, true},
    {"f64_mfma", &g_f64_mfma, 0, 3, false},
    {"reduce_sparse", &g_reduce_sparse, 0, 1, true},
    {"reduce_sparse_max", &g_reduce_sparse_max, -1, INT_MAX, false},
    {"proj_mode", &g_proj_mode, 0, 1, false},
    {"proj_small", &g_proj_small, INT_MIN, INT_MAX, false},
    {"proj_list_cap", &g_proj_list_cap, 1, 2048, false},
    {"proj_check", &g_proj_check_always, 0, 1, true},
    {"proj_res_side", &g_proj_res_side, 0, 1, true},   // takes effect at the next aa_set_state of a new problem size
    {"fuse_finalize", &g_fuse_finalize, 0, 1, true},
    {"use_graph", &g_use_graph, 0, 1, true},
    {"outer_nosync", &g_outer_nosync, 0, 1, true},
    {"pq_mfma", &g_pq_mfma, 0, 1, true},
    {"qp_mode", &g_qp_mode, 0, 4, false},
    {"qp_pass_cap", &g_qp_pass_cap, 1, INT_MAX, false},
    {"qp_quad_cap", &g_qp_quad_cap, 0, INT_MAX, false},
    {"qp_sort", &g_qp_sort, 0, 1, true},
    {"qp_live", &g_qp_live, 0, 1, true},
    {"qp_overlap_tail", &g_qp_overlap_tail, 0, 1, true},
    {"qp_fused_order", &g_qp_fused_order, 0, 1, true},
    {"qp_wave_lazy", &g_qp_wave_lazy, 0, 1, true},
    {"qp_quad_lazy", &g_qp_quad_lazy, 0, 1, true},
    {"fin_in_last", &g_fin_in_last, 0, 1, true},
    {"setup_in_grad", &g_setup_in_grad, 0, 1, true},
    {"gram_side", &g_gram_side, 0, 1, true},
    {"grad_side", &g_grad_side, 0, 1, true},
    {"spg_tail", &g_spg_tail, 0, 1, true},
    {"pack_comm", &g_pack_comm, 0, 1, true},
};

int aa_set_option(const char *name, int value)
{
    AA_REQUIRE(name != nullptr, AA_ERR_ARG, "null option name");
    for (const AaOption &o : kOptions) {
        if (strcmp(name, o.name)) continue;
        AA_REQUIRE(o.flag || (value >= o.lo && value <= o.hi), AA_ERR_ARG, "%s must be in %d..%d", o.name, o.lo, o.hi);
        *o.target = o.flag ? (value != 0) : value;
        return AA_OK;
    }
    set_error("unknown option '%s'", name);
    return AA_ERR_ARG;
}

int aa_device_count(int *count)
{
    int n = 0;
    AA_CHECK_HIP(hipGetDeviceCount(&n));
    *count = n;
    return AA_OK;
}

int aa_ctx_create(aa_ctx **out, int device, int dtype)
{
    AA_REQUIRE(out != nullptr, AA_ERR_ARG, "null ctx pointer");
    AA_REQUIRE(dtype == AA_F32 || dtype == AA_F64, AA_ERR_ARG, "bad dtype %d", dtype);
    int n = 0;
    AA_CHECK_HIP(hipGetDeviceCount(&n));
    AA_REQUIRE(n > 0, AA_ERR_HIP, "no HIP device visible");
    AA_REQUIRE(device >= 0 && device < n, AA_ERR_ARG, "device %d out of range (0..%d)", device, n - 1);
    AA_CHECK_HIP(hipSetDevice(device));
    aa_ctx *h = new aa_ctx();
    h->c.device = device;
    h->c.dtype = dtype;
    // non-blocking streams: no implicit synchronisation with the legacy null stream, i.e. with the
    // other contexts of the process (every copy and fill of this library goes through a stream:
    // ctx_memcpy / ctx_memset)
    hipError_t e = hipStreamCreateWithFlags(&h->c.stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        int lo = 0, hi = 0;                       // numerically lower = higher priority
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        e = hipStreamCreateWithPriority(&h->c.stream2, hipStreamNonBlocking, hi);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->c.stream3, hipStreamNonBlocking, hi);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->c.evFork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->c.evJoin, hipEventDisableTiming);
    if (e != hipSuccess) {
        set_error("hipStreamCreate: %s", hipGetErrorString(e));
        delete h;
        return AA_ERR_HIP;
    }
    *out = h;
    return AA_OK;
}

int aa_ctx_destroy(aa_ctx *h)
{
    if (!h) return AA_OK;
    Ctx *c = &h->c;
    (void)hipSetDevice(c->device);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->stream3) (void)hipStreamSynchronize(c->stream3);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    comm_destroy(c);
    DevBuf *all[] = {&c->X, &c->Ct, &c->Zt, &c->Dt, &c->Gr, &c->Gn, &c->gk, &c->gn, &c->H, &c->tmpTall,
                     &c->P, &c->Q, &c->ZtX, &c->Pw, &c->Qw, &c->wideScratch, &c->partial, &c->groupFlags, &c->slabMode, &c->rlPartial, &c->redPartial,
                     &c->gramOut, &c->gramState, &c->costDev, &c->costSlot, &c->redOut, &c->redGather, &c->listGather, &c->scalars, &c->proj, &c->projList, &c->projSegCnt, &c->Mdev, &c->alphaDev, &c->iterState, &c->snapC, &c->snapZ, &c->snapAlpha, &c->qpIters, &c->qpPerm, &c->fsScratch, &c->feat, &c->featNorm,
                     &c->crossX, &c->crossNorm, &c->crossV, &c->rowNorm, &c->xformCost, &c->scoreScratch,
                     &c->qpStats, &c->qpLive, &c->slotCosts, &c->slotCounters, &c->slotStates, &c->slotCost0, &c->slotSnapP, &c->slotSaveP, &c->slotSaveGr, &c->tmpTall2, &c->redPartial2, &c->redOut2, &c->proj2, &c->projList2, &c->projSegCnt2};
    for (DevBuf *b : all) b->release();
    if (c->evFork2) (void)hipEventDestroy(c->evFork2);
    if (c->evJoin2) (void)hipEventDestroy(c->evJoin2);
    for (int w = 0; w < 2; ++w)
        for (hipEvent_t e : c->gemmEvents[w]) (void)hipEventDestroy(e);
    if (c->evFork) (void)hipEventDestroy(c->evFork);
    if (c->evJoin) (void)hipEventDestroy(c->evJoin);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream3) (void)hipStreamDestroy(c->stream3);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete h;
    return AA_OK;
}

int aa_set_linear_kernel(aa_ctx *h, int on)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    AA_REQUIRE(!on || h->c.form == AA_FORM_DATA, AA_ERR_STATE, "aa_set_linear_kernel needs a data matrix");
    h->c.linear_kernel = on != 0;
    return AA_OK;
}

// ------------------------------------------------------------------ installing data
// Every entry point that gives a context its matrix is: its argument checks, install_begin, its fill of the
// new buffer, install_commit.  Between the two the context holds no data, so a fill that fails leaves it
// that way and never half-installed; a call refused by its argument checks has not touched the context.
struct Install {
    int form = AA_FORM_DATA;
    long n = 0, p = 0, p_pad = 0;              // n_pad is roundup(n, 128) everywhere
    long n_global = 0, row_offset = 0;
    long feat_p = 0, feat_ld = 0;              // feat_ld > 0: feat [n_pad + slack][feat_ld] and featNorm instead of X
    const DevBuf *borrow = nullptr;            // aa_share_data: X aliases this buffer instead of being allocated
};

// the common shape: n rows of p columns of the context's own, data form, single rank
static Install install_rows(long n, long p, long p_pad)
{
    Install in;
    in.n = in.n_global = n;
    in.p = p;
    in.p_pad = p_pad;
    return in;
}

// what a new matrix resets -- everything that belongs to the rows, the kernel or the factors of the old one
// (buffers other than X / feat / featNorm stay allocated) -- and the zero-filled buffer it goes into
static int install_begin(Ctx *c, const Install &in)
{
    c->have_data = false;
    c->form = in.form;
    c->linear_kernel = false;
    c->kernel = KernelSpec{};                  // an implicit kernel's installer names it once its fill has succeeded
    c->cross_s = 0;                            // a reference set belongs to the rows it was set for
    c->n = in.n;
    c->p = in.p;
    c->n_pad = round_up(in.n, 128);
    c->p_pad = in.p_pad;
    c->n_global = in.n_global;
    c->row_offset = in.row_offset;
    c->have_trace = false;
    c->k = 0;                                  // forces (re)allocation of the factor buffers
    c->KP = 0;
    c->have_state = false;
    c->grams_valid = false;
    c->qp_iters_valid = false;                 // pass counts and sample order of the previous rows
    c->qp_perm_ready = false;
    c->qp_perm_n = 0;
    c->fs_k = 0;                               // a selection belongs to the rows it ran on
    c->X.release();                            // (an implicit kernel: nothing stands in for K)
    if (in.borrow) {
        c->X.p = in.borrow->p;                 // read-only everywhere in the solver
        c->X.bytes = in.borrow->bytes;
        c->X.borrowed = true;
        return AA_OK;
    }
    if (!in.feat_ld)
        return c->X.alloc((size_t)(c->n_pad + AA_SLACK_ROWS) * c->p_pad * esize(c));
    c->feat_p = in.feat_p;
    c->feat_ld = in.feat_ld;
    AA_CHECK(c->feat.alloc((size_t)(c->n_pad + AA_SLACK_ROWS) * c->feat_ld * sizeof(double)));
    AA_CHECK_HIP(ctx_memset(c, c->feat.p, 0, c->feat.bytes));
    return c->featNorm.alloc((size_t)(c->n_pad + AA_SLACK_ROWS) * sizeof(double));
}

// after the fill and whatever it waits for have succeeded
static void install_commit(Ctx *c) { c->have_data = true; }

// What the entry points that read another context's matrix ask of the pair: two contexts, the owner holding a
// stored matrix in data form (kernel_form_too: or a stored kernel matrix), both single rank, element types that
// go together, one device.  `who` names the entry point; `code` is what its family returns for the rank and
// element-type refusals (AA_ERR_ARG: rows / take / share, AA_ERR_STATE: features).
enum OwnerDtype { DTYPE_SAME = 0, DTYPE_MAY_WIDEN = 1, DTYPE_INTO_F64 = 2 /* ctx float64, owner of either type */ };
static int check_owner(const aa_ctx *h, const aa_ctx *owner, const char *who, int code, OwnerDtype rule,
                       bool kernel_form_too = false)
{
    AA_REQUIRE(h && owner && h != owner, AA_ERR_ARG, "%s: two different contexts needed", who);
    const Ctx *c = &h->c, *o = &owner->c;
    AA_REQUIRE(kernel_form_too ? o->have_data && !o->kernel.kind : has_stored_data(o), AA_ERR_STATE,
               "%s: the owner holds no stored %s", who, kernel_form_too ? "matrix" : "data matrix (data form)");
    AA_REQUIRE(c->world == 1 && !c->force_comm && o->world == 1 && !o->force_comm, code, "%s is single-rank", who);
    static const char *const needed[] = {"same data type needed",
                                         "equal data types, or a float32 owner widened into a float64 context",
                                         "a float64 context needed"};
    const bool widens = rule == DTYPE_MAY_WIDEN && o->dtype == AA_F32 && c->dtype == AA_F64;
    AA_REQUIRE(rule == DTYPE_INTO_F64 ? c->dtype == AA_F64 : (o->dtype == c->dtype || widens), code, "%s: %s", who,
               needed[rule]);
    AA_REQUIRE(o->device == c->device, AA_ERR_ARG, "%s: same device needed", who);
    return AA_OK;
}

// The features of the implicit kernel `spec`: the kernel form of the algorithm (/k conventions, tr K) on a
// virtual n x n matrix.  From the host (X, n, p, ld), or -- `who` names the entry point -- the rows of `owner`'s
// resident data matrix, converted on the device.  The context is float64 and single rank for both; check_owner
// says so first for an owner, with its own words.
static int set_kernel_features(aa_ctx *h, const KernelSpec &spec, const double *X, long n, long p, long ld,
                               const aa_ctx *owner = nullptr, const char *who = nullptr)
{
    if (who) {
        AA_CHECK(check_owner(h, owner, who, AA_ERR_STATE, DTYPE_INTO_F64));
        n = owner->c.n;
        p = owner->c.p;
        AA_REQUIRE(p < (1L << 30), AA_ERR_ARG, "bad shape n=%ld p=%ld", n, p);
    } else {
        AA_REQUIRE(h && X, AA_ERR_ARG, "null argument");
        AA_REQUIRE(n >= 1 && p >= 1 && ld >= p && p < (1L << 30), AA_ERR_ARG, "bad shape n=%ld p=%ld ld=%ld", n, p, ld);
    }
    AA_CHECK(kernel_spec_check(spec));
    Ctx *c = &h->c;
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_STATE, "the implicit %s kernel is single-rank", spec.name());
    AA_REQUIRE(c->dtype == AA_F64, AA_ERR_STATE, "the implicit %s kernel needs a float64 context", spec.name());
    AA_CHECK_HIP(hipSetDevice(c->device));
    Install in = install_rows(n, n, round_up(n, 128));
    in.form = AA_FORM_KERNEL;
    in.feat_p = p;
    in.feat_ld = spec.feat_ld(p);
    AA_CHECK(install_begin(c, in));
    if (who)
        AA_CHECK(launch_features_from_data(c, owner->c.X.p, owner->c.dtype, owner->c.p_pad, n, p, c->feat.as<double>(),
                                           c->feat_ld));
    else
        AA_CHECK_HIP(ctx_memcpy2d(c, c->feat.p, (size_t)c->feat_ld * sizeof(double), X, (size_t)ld * sizeof(double),
                                  (size_t)p * sizeof(double), (size_t)n, hipMemcpyHostToDevice));
    AA_CHECK(launch_row_norms(c, c->feat.as<double>(), c->feat_ld, c->feat_p, c->n_pad, c->featNorm.as<double>()));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));   // the owner has been read: it may go
    c->kernel = spec;
    install_commit(c);
    return AA_OK;
}

int aa_set_rbf_features(aa_ctx *h, const double *X, long n, long p, long ld, double gamma)
{
    return set_kernel_features(h, KernelSpec{IMPLICIT_RBF, gamma}, X, n, p, ld);
}

int aa_set_poly_features(aa_ctx *h, const double *X, long n, long p, long ld, double gamma, double coef0, int degree)
{
    return set_kernel_features(h, KernelSpec{IMPLICIT_POLY, gamma, coef0, degree}, X, n, p, ld);
}

int aa_set_rbf_features_resident(aa_ctx *h, const aa_ctx *owner, double gamma)
{
    return set_kernel_features(h, KernelSpec{IMPLICIT_RBF, gamma}, nullptr, 0, 0, 0, owner, "aa_set_rbf_features_resident");
}

int aa_set_poly_features_resident(aa_ctx *h, const aa_ctx *owner, double gamma, double coef0, int degree)
{
    return set_kernel_features(h, KernelSpec{IMPLICIT_POLY, gamma, coef0, degree}, nullptr, 0, 0, 0, owner,
                               "aa_set_poly_features_resident");
}

int aa_comm_get_unique_id(void *id128) { return comm_unique_id(id128); }

int aa_ctx_comm_init(aa_ctx *h, const void *id128, int rank, int world)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    return comm_init(&h->c, id128, rank, world);
}

int aa_ctx_p2p_export(aa_ctx *h, int world, void *handle64)
{
    AA_REQUIRE(h && handle64, AA_ERR_ARG, "null argument");
    return p2p_export(&h->c, world, handle64);
}

int aa_ctx_p2p_init(aa_ctx *h, const void *handles, int rank, int world)
{
    AA_REQUIRE(h && handles, AA_ERR_ARG, "null argument");
    return p2p_init(&h->c, handles, rank, world);
}

int aa_ctx_allreduce_host(aa_ctx *h, double *buf, int count, int op)
{
    AA_REQUIRE(h && buf && count >= 0, AA_ERR_ARG, "bad arguments");
    Ctx *c = &h->c;
    if ((c->world <= 1 && !c->force_comm) || count == 0) return AA_OK;
    AA_CHECK_HIP(hipSetDevice(c->device));
    ScopedDevBuf tmp;
    AA_CHECK(tmp.alloc((size_t)count * sizeof(double)));
    AA_CHECK_HIP(hipMemcpyAsync(tmp.p, buf, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    AA_CHECK(comm_allreduce(c, tmp.as<double>(), count, op));
    AA_CHECK_HIP(hipMemcpyAsync(buf, tmp.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    return AA_OK;
}

int aa_set_data(aa_ctx *h, const void *X, int host_dtype, long n, long p, long ld, int form,
                long n_global, long row_offset)
{
    AA_REQUIRE(h && X, AA_ERR_ARG, "null argument");
    AA_REQUIRE(n >= 1 && p >= 1 && ld >= p, AA_ERR_ARG, "bad shape n=%ld p=%ld ld=%ld", n, p, ld);
    AA_REQUIRE(host_dtype == AA_F32 || host_dtype == AA_F64, AA_ERR_ARG, "bad host dtype");
    AA_REQUIRE(form == AA_FORM_DATA || form == AA_FORM_KERNEL, AA_ERR_ARG, "bad form");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    if (form == AA_FORM_KERNEL)
        AA_REQUIRE((c->world == 1 && !c->force_comm) && n == p && n_global == n && row_offset == 0, AA_ERR_ARG,
                   "kernel form needs a square matrix on a single rank");
    AA_REQUIRE(n_global >= n && row_offset >= 0 && row_offset + n <= n_global, AA_ERR_ARG, "bad shard");
    Install in = install_rows(n, p, round_up(p, 128));   // (kernel form: p == n, so p_pad == n_pad)
    in.form = form;
    in.n_global = n_global;
    in.row_offset = row_offset;
    AA_CHECK(install_begin(c, in));
    const size_t es = esize(c);
    const size_t hes = host_dtype == AA_F32 ? 4 : 8;
    if (host_dtype == c->dtype) {
        AA_CHECK_HIP(ctx_memcpy2d(c, c->X.p, (size_t)c->p_pad * es, X, (size_t)ld * hes, (size_t)p * es,
                                 (size_t)n, hipMemcpyHostToDevice));
    } else {
        const long chunk = 2048;
        std::vector<unsigned char> tmp((size_t)chunk * p * es);
        for (long r0 = 0; r0 < n; r0 += chunk) {
            const long rows = (n - r0 < chunk) ? n - r0 : chunk;
            if (c->dtype == AA_F32) {
                const double *src = reinterpret_cast<const double *>(X);
                float *dst = reinterpret_cast<float *>(tmp.data());
                for (long r = 0; r < rows; ++r)
                    for (long q = 0; q < p; ++q) dst[r * p + q] = (float)src[(r0 + r) * ld + q];
            } else {
                const float *src = reinterpret_cast<const float *>(X);
                double *dst = reinterpret_cast<double *>(tmp.data());
                for (long r = 0; r < rows; ++r)
                    for (long q = 0; q < p; ++q) dst[r * p + q] = (double)src[(r0 + r) * ld + q];
            }
            AA_CHECK_HIP(ctx_memcpy2d(c, reinterpret_cast<unsigned char *>(c->X.p) + (size_t)r0 * c->p_pad * es,
                                     (size_t)c->p_pad * es, tmp.data(), (size_t)p * es, (size_t)p * es,
                                     (size_t)rows, hipMemcpyHostToDevice));
        }
    }
    install_commit(c);
    return AA_OK;
}

int aa_share_data(aa_ctx *h, const aa_ctx *owner)
{
    AA_CHECK(check_owner(h, owner, "aa_share_data", AA_ERR_ARG, DTYPE_SAME, /* kernel_form_too */ true));
    Ctx *c = &h->c;
    const Ctx *o = &owner->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    Install in = install_rows(o->n, o->p, o->p_pad);
    in.form = o->form;
    in.n_global = o->n_global;
    in.row_offset = o->row_offset;
    in.borrow = &o->X;
    AA_CHECK(install_begin(c, in));
    c->have_trace = o->have_trace;             // the owner's trace pass serves every context that shares its matrix
    c->trace = o->trace;
    install_commit(c);
    return AA_OK;
}

int aa_set_data_rows(aa_ctx *h, const aa_ctx *owner, long row0, long n)
{
    AA_CHECK(check_owner(h, owner, "aa_set_data_rows", AA_ERR_ARG, DTYPE_SAME));
    Ctx *c = &h->c;
    const Ctx *o = &owner->c;
    AA_REQUIRE(row0 >= 0 && n >= 1 && n <= o->n && row0 <= o->n - n, AA_ERR_ARG, "bad row block [%ld, %ld) of %ld", row0,
               row0 + n, o->n);
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(install_begin(c, install_rows(n, o->p, o->p_pad)));
    // rows are contiguous with the same leading dimension, their padding columns already zero
    const size_t es = esize(c);
    AA_CHECK_HIP(ctx_memcpy(c, c->X.p, reinterpret_cast<const unsigned char *>(o->X.p) + (size_t)row0 * o->p_pad * es,
                            (size_t)n * c->p_pad * es, hipMemcpyDeviceToDevice));
    install_commit(c);
    return AA_OK;
}

int aa_set_data_rows_affine(aa_ctx *h, const aa_ctx *owner, long row0, long n, const double *shift, const double *scale)
{
    AA_CHECK(check_owner(h, owner, "aa_set_data_rows_affine", AA_ERR_ARG, DTYPE_SAME));
    Ctx *c = &h->c;
    const Ctx *o = &owner->c;
    AA_REQUIRE(row0 >= 0 && n >= 1 && n <= o->n && row0 <= o->n - n, AA_ERR_ARG, "bad row block [%ld, %ld) of %ld", row0,
               row0 + n, o->n);
    // refused before anything of ctx is released: a zero or non-finite divisor, a non-finite shift
    for (long j = 0; j < o->p; ++j) {
        AA_REQUIRE(!scale || (scale[j] != 0.0 && scale[j] - scale[j] == 0.0), AA_ERR_ARG,
                   "aa_set_data_rows_affine: scale[%ld] = %g is zero or not finite", j, scale[j]);
        AA_REQUIRE(!shift || shift[j] - shift[j] == 0.0, AA_ERR_ARG,
                   "aa_set_data_rows_affine: shift[%ld] = %g is not finite", j, shift[j]);
    }
    AA_CHECK_HIP(hipSetDevice(c->device));
    ScopedDevBuf coef;                                                        // shift | scale, p_pad doubles each
    AA_CHECK(coef.alloc((size_t)2 * o->p_pad * sizeof(double)));
    double *dshift = shift ? coef.as<double>() : nullptr, *dscale = scale ? coef.as<double>() + o->p_pad : nullptr;
    if (shift) AA_CHECK_HIP(ctx_memcpy(c, dshift, shift, (size_t)o->p * sizeof(double), hipMemcpyHostToDevice));
    if (scale) AA_CHECK_HIP(ctx_memcpy(c, dscale, scale, (size_t)o->p * sizeof(double), hipMemcpyHostToDevice));
    AA_CHECK(install_begin(c, install_rows(n, o->p, o->p_pad)));
    AA_CHECK(launch_affine_rows(c, o->X.p, row0, dshift, dscale));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    install_commit(c);
    return AA_OK;
}

int aa_set_data_take(aa_ctx *h, const aa_ctx *owner, const long *idx, long n)
{
    AA_CHECK(check_owner(h, owner, "aa_set_data_take", AA_ERR_ARG, DTYPE_MAY_WIDEN));
    Ctx *c = &h->c;
    const Ctx *o = &owner->c;
    AA_REQUIRE(n >= 1 && (idx || n <= o->n), AA_ERR_ARG, "bad row count %ld (the owner holds %ld rows)", n, o->n);
    // refused before anything of ctx is released and before any launch: the gather kernel reads whatever row it is given
    for (long r = 0; idx && r < n; ++r)
        AA_REQUIRE(idx[r] >= 0 && idx[r] < o->n, AA_ERR_ARG, "aa_set_data_take: idx[%ld] = %ld is outside [0, %ld)", r,
                   idx[r], o->n);
    AA_CHECK_HIP(hipSetDevice(c->device));
    ScopedDevBuf didx;
    if (idx) {
        AA_CHECK(didx.alloc((size_t)n * sizeof(long)));
        AA_CHECK_HIP(ctx_memcpy(c, didx.p, idx, (size_t)n * sizeof(long), hipMemcpyHostToDevice));
    }
    // p_pad is the context's own: a widened copy need not share the owner's
    AA_CHECK(install_begin(c, install_rows(n, o->p, round_up(o->p, 128))));
    AA_CHECK(launch_gather_rows(c, o->X.p, o->dtype, o->p_pad, idx ? didx.as<long>() : (const long *)nullptr));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    install_commit(c);
    return AA_OK;
}

// the compute units gram_plan fills
static int device_cus(const Ctx *c, int *cus)
{
    AA_CHECK_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, c->device));
    return AA_OK;
}

// a p_pad-long float64 table on the device from p host values (null: zeros), the padding zero
static int upload_padded_row(Ctx *c, ScopedDevBuf &dst, const double *src, long p, long p_pad)
{
    AA_CHECK(dst.alloc((size_t)p_pad * sizeof(double)));                      // zero filled
    if (src) AA_CHECK_HIP(ctx_memcpy(c, dst.p, src, (size_t)p * sizeof(double), hipMemcpyHostToDevice));
    return AA_OK;
}

int aa_data_gram(aa_ctx *h, int side, const double *shift, double *out, long ldo)
{
    AA_REQUIRE(h && out, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(has_stored_data(c), AA_ERR_STATE, "aa_data_gram: no stored data matrix (data form)");
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_ARG, "aa_data_gram is single-rank");
    AA_REQUIRE(side == AA_GRAM_ROWS || side == AA_GRAM_COLS, AA_ERR_ARG, "aa_data_gram: side %d (AA_GRAM_ROWS or AA_GRAM_COLS)",
               side);
    const long d = side == AA_GRAM_ROWS ? c->n : c->p;
    AA_REQUIRE(d <= GRAM_MAX_D, AA_ERR_ARG, "aa_data_gram: a %ld x %ld Gram matrix (at most %ld x %ld are formed)", d, d,
               GRAM_MAX_D, GRAM_MAX_D);
    AA_REQUIRE(ldo >= d, AA_ERR_ARG, "aa_data_gram: leading dimension %ld of a %ld x %ld result", ldo, d, d);
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(join_side(c));
    int cus = 0;
    AA_CHECK(device_cus(c, &cus));
    const GramPlan pl = gram_plan(side, c->n, c->p, (int)esize(c), cus);
    ScopedDevBuf dshift, partial, G;
    AA_CHECK(upload_padded_row(c, dshift, shift, c->p, c->p_pad));
    AA_CHECK(partial.alloc((size_t)pl.partial_bytes));
    AA_CHECK(G.alloc((size_t)pl.g_ld * pl.g_ld * sizeof(double)));
    AA_CHECK(launch_gram(c, pl, dshift.as<double>(), partial.as<double>(), G.as<double>()));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy2d(c, out, (size_t)ldo * sizeof(double), G.p, (size_t)pl.g_ld * sizeof(double),
                              (size_t)d * sizeof(double), (size_t)d, hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_set_data_projected(aa_ctx *h, const aa_ctx *owner, long row0, long n, int q, const double *V, long ldv,
                          const double *shift)
{
    AA_CHECK(check_owner(h, owner, "aa_set_data_projected", AA_ERR_ARG, DTYPE_MAY_WIDEN));
    Ctx *c = &h->c;
    const Ctx *o = &owner->c;
    AA_REQUIRE(row0 >= 0 && n >= 1 && n <= o->n && row0 <= o->n - n, AA_ERR_ARG, "bad row block [%ld, %ld) of %ld", row0,
               row0 + n, o->n);
    AA_REQUIRE(q >= 1 && q <= AA_MAX_PROJECTED, AA_ERR_ARG, "aa_set_data_projected: %d components (1 to %d are supported)",
               q, AA_MAX_PROJECTED);
    AA_REQUIRE(V && ldv >= o->p, AA_ERR_ARG, "aa_set_data_projected: a %d x %ld matrix V with ldv >= %ld needed", q, o->p,
               o->p);
    // refused before anything of ctx is released: a non-finite direction or shift
    for (int i = 0; i < q; ++i)
        for (long j = 0; j < o->p; ++j)
            AA_REQUIRE(V[(size_t)i * ldv + j] - V[(size_t)i * ldv + j] == 0.0, AA_ERR_ARG,
                       "aa_set_data_projected: V[%d][%ld] = %g is not finite", i, j, V[(size_t)i * ldv + j]);
    for (long j = 0; shift && j < o->p; ++j)
        AA_REQUIRE(shift[j] - shift[j] == 0.0, AA_ERR_ARG, "aa_set_data_projected: shift[%ld] = %g is not finite", j,
                   shift[j]);
    AA_CHECK_HIP(hipSetDevice(c->device));
    ScopedDevBuf dshift, dV;                                                  // V widened to [rows of its tiles][p_pad]
    AA_CHECK(upload_padded_row(c, dshift, shift, o->p, o->p_pad));
    AA_CHECK(dV.alloc((size_t)project_v_rows(q) * o->p_pad * sizeof(double)));   // zero filled: both paddings
    AA_CHECK_HIP(ctx_memcpy2d(c, dV.p, (size_t)o->p_pad * sizeof(double), V, (size_t)ldv * sizeof(double),
                              (size_t)o->p * sizeof(double), (size_t)q, hipMemcpyHostToDevice));
    AA_CHECK(install_begin(c, install_rows(n, q, round_up(q, 128))));
    AA_CHECK(launch_project_rows(c, o->X.p, o->dtype, o->p_pad, o->p, row0, n, q, dV.as<double>(), dshift.as<double>(),
                                 c->X.p, c->p_pad, c->dtype));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));   // the owner and the two tables have been read: they may go
    install_commit(c);
    return AA_OK;
}

int aa_data_column_moments(aa_ctx *h, double *mean, double *var)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(has_stored_data(c), AA_ERR_STATE, "aa_data_column_moments: no stored data matrix (data form)");
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_ARG, "aa_data_column_moments is single-rank");
    if (!mean && !var) return AA_OK;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(join_side(c));
    long nslab = 0;
    (void)moment_slab_rows(c->n, c->p_pad, &nslab);
    ScopedDevBuf partial, mom;                                                // mom: mean | var, p_pad doubles each
    AA_CHECK(partial.alloc((size_t)nslab * c->p_pad * sizeof(double)));
    AA_CHECK(mom.alloc((size_t)2 * c->p_pad * sizeof(double)));
    double *dvar = var ? mom.as<double>() + c->p_pad : nullptr;
    AA_CHECK(launch_col_moments(c, partial.as<double>(), mom.as<double>(), dvar));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    if (mean) AA_CHECK_HIP(ctx_memcpy(c, mean, mom.p, (size_t)c->p * sizeof(double), hipMemcpyDeviceToHost));
    if (var) AA_CHECK_HIP(ctx_memcpy(c, var, dvar, (size_t)c->p * sizeof(double), hipMemcpyDeviceToHost));
    return AA_OK;
}

// out (G x p, host) = the weighted column sums of c's matrix; group / centre null: plain sums
static int weighted_column_sums(aa_ctx *h, const char *who, int G, const double *A, const int *group,
                                const double *centre, int Gc, double *out)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(has_stored_data(c), AA_ERR_STATE, "%s: no stored data matrix (data form)", who);
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_ARG, "%s is single-rank", who);
    AA_REQUIRE(A && out, AA_ERR_ARG, "null argument");
    AA_REQUIRE(G >= 1 && G <= AA_MAX_COEF_ROWS, AA_ERR_ARG, "%s: %d coefficient rows (1 to %d are supported)", who, G,
               AA_MAX_COEF_ROWS);
    if (centre) {
        AA_REQUIRE(group && Gc >= 1 && Gc <= AA_MAX_COEF_ROWS, AA_ERR_ARG,
                   "%s: a centre table needs row labels and 1 to %d rows; got %d", who, AA_MAX_COEF_ROWS, Gc);
        for (long r = 0; r < c->n; ++r)
            AA_REQUIRE(group[r] >= -1 && group[r] < Gc, AA_ERR_ARG, "%s: group[%ld] = %d is outside [-1, %d)", who, r,
                       group[r], Gc);
    }
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(join_side(c));
    long nslab = 0;
    (void)moment_slab_rows(c->n, c->p_pad, &nslab);
    std::vector<double> At((size_t)c->n * AA_MAX_COEF_ROWS, 0.0);            // transposed, rows g >= G zero
    for (int g = 0; g < G; ++g)
        for (long t = 0; t < c->n; ++t) At[(size_t)t * AA_MAX_COEF_ROWS + g] = A[(size_t)g * c->n + t];
    ScopedDevBuf dAt, dgrp, dcen, partial, sums;
    AA_CHECK(dAt.alloc(At.size() * sizeof(double)));
    AA_CHECK(partial.alloc((size_t)nslab * G * c->p_pad * sizeof(double)));
    AA_CHECK(sums.alloc((size_t)G * c->p_pad * sizeof(double)));
    AA_CHECK_HIP(ctx_memcpy(c, dAt.p, At.data(), At.size() * sizeof(double), hipMemcpyHostToDevice));
    if (centre) {
        AA_CHECK(dgrp.alloc((size_t)c->n * sizeof(int)));
        AA_CHECK(dcen.alloc((size_t)Gc * c->p_pad * sizeof(double)));     // zero filled: the padding columns stay zero
        AA_CHECK_HIP(ctx_memcpy(c, dgrp.p, group, (size_t)c->n * sizeof(int), hipMemcpyHostToDevice));
        AA_CHECK_HIP(ctx_memcpy2d(c, dcen.p, (size_t)c->p_pad * sizeof(double), centre, (size_t)c->p * sizeof(double),
                                  (size_t)c->p * sizeof(double), (size_t)Gc, hipMemcpyHostToDevice));
    }
    AA_CHECK(launch_col_weighted_sums(c, G, dAt.as<double>(), centre ? dgrp.as<int>() : (const int *)nullptr,
                                      centre ? dcen.as<double>() : (const double *)nullptr, partial.as<double>(),
                                      sums.as<double>()));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy2d(c, out, (size_t)c->p * sizeof(double), sums.p, (size_t)c->p_pad * sizeof(double),
                              (size_t)c->p * sizeof(double), (size_t)G, hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_data_weighted_column_sums(aa_ctx *h, int G, const double *A, double *out)
{
    return weighted_column_sums(h, "aa_data_weighted_column_sums", G, A, nullptr, nullptr, 0, out);
}

int aa_data_grouped_sqdev(aa_ctx *h, int G, const double *A, const int *group, const double *centre, int Gc, double *out)
{
    AA_REQUIRE(group && centre, AA_ERR_ARG, "null argument");
    return weighted_column_sums(h, "aa_data_grouped_sqdev", G, A, group, centre, Gc, out);
}

int aa_set_data_rows_model(aa_ctx *h, const aa_ctx *owner, long row0, long n, int G, const int *group,
                           const double *shift, const double *icpt, const double *slope, const double *t,
                           const double *scale)
{
    AA_CHECK(check_owner(h, owner, "aa_set_data_rows_model", AA_ERR_ARG, DTYPE_SAME));
    Ctx *c = &h->c;
    const Ctx *o = &owner->c;
    AA_REQUIRE(row0 >= 0 && n >= 1 && n <= o->n && row0 <= o->n - n, AA_ERR_ARG, "bad row block [%ld, %ld) of %ld", row0,
               row0 + n, o->n);
    const bool tables = shift || scale, trend = icpt || slope || t;
    AA_REQUIRE(!trend || (icpt && slope && t), AA_ERR_ARG,
               "aa_set_data_rows_model: intercept, slope and row times come together or not at all");
    // refused before anything of ctx is released: too many groups, a label without a table row, a zero or
    // non-finite divisor, a non-finite shift, slope, intercept or row time
    AA_REQUIRE(G >= 1 && G <= AA_MAX_COEF_ROWS, AA_ERR_ARG, "aa_set_data_rows_model: %d groups (1 to %d are supported)",
               G, AA_MAX_COEF_ROWS);
    AA_REQUIRE(!tables || group || G == 1, AA_ERR_ARG, "aa_set_data_rows_model: tables of %d groups need row labels", G);
    for (long r = 0; tables && group && r < n; ++r)
        AA_REQUIRE(group[r] >= 0 && group[r] < G, AA_ERR_ARG, "aa_set_data_rows_model: group[%ld] = %d is outside [0, %d)",
                   r, group[r], G);
    for (long j = 0; tables && j < (long)G * o->p; ++j) {
        AA_REQUIRE(!scale || (scale[j] != 0.0 && scale[j] - scale[j] == 0.0), AA_ERR_ARG,
                   "aa_set_data_rows_model: scale[%ld][%ld] = %g is zero or not finite", j / o->p, j % o->p, scale[j]);
        AA_REQUIRE(!shift || shift[j] - shift[j] == 0.0, AA_ERR_ARG,
                   "aa_set_data_rows_model: shift[%ld][%ld] = %g is not finite", j / o->p, j % o->p, shift[j]);
    }
    for (long j = 0; trend && j < o->p; ++j)
        AA_REQUIRE(icpt[j] - icpt[j] == 0.0 && slope[j] - slope[j] == 0.0, AA_ERR_ARG,
                   "aa_set_data_rows_model: intercept %g / slope %g of column %ld is not finite", icpt[j], slope[j], j);
    for (long r = 0; trend && r < n; ++r)
        AA_REQUIRE(t[r] - t[r] == 0.0, AA_ERR_ARG, "aa_set_data_rows_model: t[%ld] = %g is not finite", r, t[r]);
    AA_CHECK_HIP(hipSetDevice(c->device));
    const size_t row = (size_t)o->p_pad * sizeof(double), used = (size_t)o->p * sizeof(double);
    ScopedDevBuf dgrp, dtab, dtrend, dt;                  // dtab: shift | scale, G x p_pad each; dtrend: icpt | slope
    const int *g_dev = nullptr;
    const double *shift_dev = nullptr, *scale_dev = nullptr, *icpt_dev = nullptr, *slope_dev = nullptr, *t_dev = nullptr;
    if (tables && group) {
        AA_CHECK(dgrp.alloc((size_t)n * sizeof(int)));
        AA_CHECK_HIP(ctx_memcpy(c, dgrp.p, group, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        g_dev = dgrp.as<int>();
    }
    if (tables) {
        AA_CHECK(dtab.alloc((size_t)2 * G * row));
        if (shift) {
            shift_dev = dtab.as<double>();
            AA_CHECK_HIP(ctx_memcpy2d(c, dtab.p, row, shift, used, used, (size_t)G, hipMemcpyHostToDevice));
        }
        if (scale) {
            scale_dev = dtab.as<double>() + (size_t)G * o->p_pad;
            AA_CHECK_HIP(ctx_memcpy2d(c, dtab.as<double>() + (size_t)G * o->p_pad, row, scale, used, used, (size_t)G,
                                      hipMemcpyHostToDevice));
        }
    }
    if (trend) {
        AA_CHECK(dtrend.alloc(2 * row));
        AA_CHECK(dt.alloc((size_t)n * sizeof(double)));
        icpt_dev = dtrend.as<double>();
        slope_dev = dtrend.as<double>() + o->p_pad;
        t_dev = dt.as<double>();
        AA_CHECK_HIP(ctx_memcpy(c, dtrend.p, icpt, used, hipMemcpyHostToDevice));
        AA_CHECK_HIP(ctx_memcpy(c, dtrend.as<double>() + o->p_pad, slope, used, hipMemcpyHostToDevice));
        AA_CHECK_HIP(ctx_memcpy(c, dt.p, t, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    }
    AA_CHECK(install_begin(c, install_rows(n, o->p, o->p_pad)));
    AA_CHECK(launch_model_rows(c, o->X.p, row0, g_dev, shift_dev, icpt_dev, slope_dev, t_dev, scale_dev));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    install_commit(c);
    return AA_OK;
}

// a GroupPlan on the device, one buffer of ints: rows | (slot, begin, len) per chunk | chunk_first
static int upload_group_plan(Ctx *c, const GroupPlan &pl, ScopedDevBuf &buf, SlotPlanDev *pd)
{
    const size_t nr = pl.rows.size(), nc = (size_t)pl.chunks();
    std::vector<int> host(nr + 3 * nc + pl.chunk_first.size());
    std::copy(pl.rows.begin(), pl.rows.end(), host.begin());
    for (size_t i = 0; i < nc; ++i) {
        host[nr + 3 * i] = pl.chunk_slot[i];
        host[nr + 3 * i + 1] = pl.chunk_begin[i];
        host[nr + 3 * i + 2] = pl.chunk_len[i];
    }
    std::copy(pl.chunk_first.begin(), pl.chunk_first.end(), host.begin() + (long)(nr + 3 * nc));
    AA_CHECK(buf.alloc(host.size() * sizeof(int)));
    AA_CHECK_HIP(ctx_memcpy(c, buf.p, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
    pd->rows = buf.as<int>();
    pd->chunks = pd->rows + nr;
    pd->chunk_first = pd->chunks + 3 * nc;
    pd->nchunk = (long)nc;
    pd->G = pl.G;
    return AA_OK;
}

// Every entry of the rows of `table` (G x p) whose slot holds a row of the plan is finite (and, is_scale, not
// zero); the other rows are not read.
static int check_slot_table(const char *who, const char *name, const double *table, const GroupPlan &pl, long p,
                            bool is_scale)
{
    for (int g = 0; table && g < pl.G; ++g) {
        if (pl.start[(size_t)g + 1] == pl.start[(size_t)g]) continue;
        const double *row = table + (size_t)g * p;
        for (long j = 0; j < p; ++j)
            AA_REQUIRE(row[j] - row[j] == 0.0 && !(is_scale && row[j] == 0.0), AA_ERR_ARG, "%s: %s[%d][%ld] = %g is %snot finite",
                       who, name, g, j, row[j], is_scale ? "zero or " : "");
    }
    return AA_OK;
}

int aa_data_slot_sums(aa_ctx *h, int G, const int *slot, const double *centre, double *out, long *counts)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(has_stored_data(c), AA_ERR_STATE, "aa_data_slot_sums: no stored data matrix (data form)");
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_ARG, "aa_data_slot_sums is single-rank");
    AA_REQUIRE(G >= 1 && G <= AA_MAX_SLOTS, AA_ERR_ARG, "aa_data_slot_sums: %d slots (1 to %d are supported)", G,
               AA_MAX_SLOTS);
    AA_REQUIRE(slot && out, AA_ERR_ARG, "null argument");
    AA_REQUIRE(c->n < (1L << 31), AA_ERR_ARG, "aa_data_slot_sums: %ld rows (fewer than 2^31 are supported)", c->n);
    const long bad = group_plan_first_bad_label(slot, c->n, G, -1);
    AA_REQUIRE(bad < 0, AA_ERR_ARG, "aa_data_slot_sums: slot[%ld] = %d is outside [-1, %d)", bad, slot[bad], G);
    const GroupPlan pl = group_plan(slot, c->n, G, AA_SLOT_CHUNK_ROWS);
    AA_CHECK(check_slot_table("aa_data_slot_sums", "centre", centre, pl, c->p, false));
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(join_side(c));
    ScopedDevBuf meta, dcen, partial, sums;
    SlotPlanDev pd;
    AA_CHECK(upload_group_plan(c, pl, meta, &pd));
    AA_CHECK(partial.alloc((size_t)pl.chunks() * c->p_pad * sizeof(double)));
    AA_CHECK(sums.alloc((size_t)G * c->p_pad * sizeof(double)));
    if (centre) {
        AA_CHECK(dcen.alloc((size_t)G * c->p_pad * sizeof(double)));      // zero filled: the padding columns stay zero
        AA_CHECK_HIP(ctx_memcpy2d(c, dcen.p, (size_t)c->p_pad * sizeof(double), centre, (size_t)c->p * sizeof(double),
                                  (size_t)c->p * sizeof(double), (size_t)G, hipMemcpyHostToDevice));
    }
    AA_CHECK(launch_slot_sums(c, pd, centre ? dcen.as<double>() : (const double *)nullptr, partial.as<double>(),
                              sums.as<double>()));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy2d(c, out, (size_t)c->p * sizeof(double), sums.p, (size_t)c->p_pad * sizeof(double),
                              (size_t)c->p * sizeof(double), (size_t)G, hipMemcpyDeviceToHost));
    for (int g = 0; counts && g < G; ++g) counts[g] = (long)pl.start[(size_t)g + 1] - pl.start[(size_t)g];
    return AA_OK;
}

int aa_set_data_rows_slots(aa_ctx *h, const aa_ctx *owner, long row0, long n, int G, const int *slot,
                           const double *shift, const double *scale)
{
    AA_CHECK(check_owner(h, owner, "aa_set_data_rows_slots", AA_ERR_ARG, DTYPE_SAME));
    Ctx *c = &h->c;
    const Ctx *o = &owner->c;
    AA_REQUIRE(row0 >= 0 && n >= 1 && n <= o->n && row0 <= o->n - n, AA_ERR_ARG, "bad row block [%ld, %ld) of %ld", row0,
               row0 + n, o->n);
    // refused before anything of ctx is released: too many slots, no table, a label without a table row, a
    // non-finite shift or a zero or non-finite divisor in a slot that a row of the block uses
    AA_REQUIRE(slot, AA_ERR_ARG, "null argument");
    AA_REQUIRE(G >= 1 && G <= AA_MAX_SLOTS, AA_ERR_ARG, "aa_set_data_rows_slots: %d slots (1 to %d are supported)", G,
               AA_MAX_SLOTS);
    AA_REQUIRE(shift || scale, AA_ERR_ARG, "aa_set_data_rows_slots: a shift table, a scale table or both are needed");
    AA_REQUIRE(n < (1L << 31), AA_ERR_ARG, "aa_set_data_rows_slots: %ld rows (fewer than 2^31 are supported)", n);
    const long bad = group_plan_first_bad_label(slot, n, G, 0);
    AA_REQUIRE(bad < 0, AA_ERR_ARG, "aa_set_data_rows_slots: slot[%ld] = %d is outside [0, %d)", bad, slot[bad], G);
    const GroupPlan pl = group_plan(slot, n, G, AA_SLOT_CHUNK_ROWS);
    AA_CHECK(check_slot_table("aa_set_data_rows_slots", "shift", shift, pl, o->p, false));
    AA_CHECK(check_slot_table("aa_set_data_rows_slots", "scale", scale, pl, o->p, true));
    AA_CHECK_HIP(hipSetDevice(c->device));
    const size_t row = (size_t)o->p_pad * sizeof(double), used = (size_t)o->p * sizeof(double);
    ScopedDevBuf meta, dtab;                              // dtab: shift | scale, G x p_pad each
    SlotPlanDev pd;
    AA_CHECK(upload_group_plan(c, pl, meta, &pd));
    AA_CHECK(dtab.alloc((size_t)2 * G * row));
    double *shift_dev = shift ? dtab.as<double>() : nullptr;
    double *scale_dev = scale ? dtab.as<double>() + (size_t)G * o->p_pad : nullptr;
    if (shift) AA_CHECK_HIP(ctx_memcpy2d(c, shift_dev, row, shift, used, used, (size_t)G, hipMemcpyHostToDevice));
    if (scale) AA_CHECK_HIP(ctx_memcpy2d(c, scale_dev, row, scale, used, used, (size_t)G, hipMemcpyHostToDevice));
    AA_CHECK(install_begin(c, install_rows(n, o->p, o->p_pad)));
    AA_CHECK(launch_slot_rows(c, o->X.p, row0, pd, shift_dev, scale_dev));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    install_commit(c);
    return AA_OK;
}

int aa_set_data_weighted(aa_ctx *h, const void *raw, int host_dtype, long n_total, long p_full, long ld,
                         const double *col_weight, long row0, long n, unsigned char *valid, long *p_valid)
{
    AA_REQUIRE(h && raw && valid && p_valid, AA_ERR_ARG, "null argument");
    AA_REQUIRE(host_dtype == AA_F32 || host_dtype == AA_F64, AA_ERR_ARG, "bad host dtype");
    AA_REQUIRE(n_total >= 1 && p_full >= 1 && ld >= p_full && p_full < (1L << 31), AA_ERR_ARG,
               "bad shape n_total=%ld p_full=%ld ld=%ld", n_total, p_full, ld);
    AA_REQUIRE(row0 >= 0 && n >= 1 && row0 + n <= n_total, AA_ERR_ARG, "bad row block [%ld, %ld) of %ld", row0,
               row0 + n, n_total);
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_ARG, "preprocessing entry point is single-rank");
    const size_t hes = host_dtype == AA_F32 ? 4 : 8;
    ScopedDevBuf draw, dflag, didx, dw;
    AA_CHECK(draw.alloc((size_t)n_total * p_full * hes));
    AA_CHECK(dflag.alloc((size_t)p_full));
    if (col_weight) AA_CHECK(dw.alloc((size_t)p_full * sizeof(double)));
    AA_CHECK_HIP(ctx_memcpy2d(c, draw.p, (size_t)p_full * hes, raw, (size_t)ld * hes, (size_t)p_full * hes,
                              (size_t)n_total, hipMemcpyHostToDevice));
    if (col_weight) AA_CHECK_HIP(ctx_memcpy(c, dw.p, col_weight, (size_t)p_full * sizeof(double), hipMemcpyHostToDevice));
    const double *w = col_weight ? dw.as<double>() : nullptr;
    // the mask is taken on the weighted field (run_hadisst_aa.py:133,201)
    AA_CHECK(launch_col_has_nan(c, draw.p, host_dtype, p_full, n_total, p_full, w, dflag.as<unsigned char>()));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned char> flags((size_t)p_full);
    AA_CHECK_HIP(ctx_memcpy(c, flags.data(), dflag.p, (size_t)p_full, hipMemcpyDeviceToHost));
    std::vector<int> idx;
    idx.reserve((size_t)p_full);
    for (long q = 0; q < p_full; ++q) {
        valid[q] = flags[(size_t)q] ? 0 : 1;
        if (!flags[(size_t)q]) idx.push_back((int)q);
    }
    const long p = (long)idx.size();
    *p_valid = p;
    AA_REQUIRE(p > 0, AA_ERR_ARG, "every column of the field holds a NaN");
    AA_CHECK(didx.alloc(idx.size() * sizeof(int)));
    AA_CHECK_HIP(ctx_memcpy(c, didx.p, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
    AA_CHECK(install_begin(c, install_rows(n, p, round_up(p, 128))));
    AA_CHECK(launch_gather_weight(c, draw.p, host_dtype, p_full, row0, n, didx.as<int>(), p, w));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    install_commit(c);
    return AA_OK;
}

int aa_get_data(aa_ctx *h, double *out, long ld)
{
    AA_REQUIRE(h && out, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    // any stored matrix, the kernel form's too (not has_stored_data)
    AA_REQUIRE(!c->kernel.kind, AA_ERR_STATE, "aa_get_data: no stored matrix behind an implicit kernel");
    AA_REQUIRE(c->have_data, AA_ERR_STATE, "no data");
    AA_REQUIRE(ld >= c->p, AA_ERR_ARG, "ld < p");
    AA_CHECK_HIP(hipSetDevice(c->device));
    ScopedDevBuf tmp;
    AA_CHECK(tmp.alloc((size_t)c->n * c->p * sizeof(double)));
    AA_CHECK(launch_data_to_double(c, tmp.as<double>()));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy2d(c, out, (size_t)ld * sizeof(double), tmp.p, (size_t)c->p * sizeof(double),
                              (size_t)c->p * sizeof(double), (size_t)c->n, hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_data_trace(aa_ctx *h, double *trace)
{
    AA_REQUIRE(h && trace, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_data, AA_ERR_STATE, "no data");
    AA_CHECK_HIP(hipSetDevice(c->device));
    if (!c->redPartial.p) {   // trace asked before any factors: set up minimal scratch
        AA_CHECK(c->redPartial.alloc(8192 * sizeof(double)));
        AA_CHECK(c->redOut.alloc(512 * sizeof(double)));
    }
    AA_CHECK(ensure_trace(c));
    *trace = c->trace;
    return AA_OK;
}

int aa_set_state(aa_ctx *h, int k, const double *C, long ldc, const double *Z, const double *alpha)
{
    AA_REQUIRE(h && C && Z, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(join_side(c));
    AA_CHECK(ensure_problem(c, k));
    AA_REQUIRE(ldc >= c->n, AA_ERR_ARG, "ldc < n");
    AA_CHECK(upload_tall(c, c->Ct, C, 1, ldc, c->n, k));     // Ct[r][i] = C[i][r]
    AA_CHECK(upload_tall(c, c->Zt, Z, k, 1, c->n, k));
    for (int i = 0; i < k; ++i) c->alpha[i] = alpha ? alpha[i] : 1.0;
    AA_CHECK(upload_alpha(c));
    c->have_state = true;
    c->qp_iters_valid = false;
    c->grams_valid = false;
    c->dict_inputs_overridden = false;
    c->x_feasible = false;
    c->products_valid = false;
    c->ckz_valid = false;
    for (int m = 0; m < 4; ++m) {
        c->projWarm[m] = c->projWarm2[m] = false;
        c->projPassHint[m] = c->projPassHint2[m] = 0;
        c->projListShort[m] = false;
    }
    return AA_OK;
}

int aa_get_state(aa_ctx *h, double *C, long ldc, double *Z, double *alpha)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state, AA_ERR_STATE, "no state");
    AA_CHECK_HIP(hipSetDevice(c->device));
    if (C) AA_CHECK(download_tall(c, c->Ct, C, 1, ldc, c->n, c->k));
    if (Z) AA_CHECK(download_tall(c, c->Zt, Z, c->k, 1, c->n, c->k));
    if (alpha)
        for (int i = 0; i < c->k; ++i) alpha[i] = c->alpha[i];
    return AA_OK;
}

int aa_set_alpha(aa_ctx *h, const double *alpha)
{
    AA_REQUIRE(h && alpha, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->k > 0, AA_ERR_STATE, "no problem");
    AA_CHECK_HIP(hipSetDevice(c->device));
    for (int i = 0; i < c->k; ++i) c->alpha[i] = alpha[i];
    return upload_alpha(c);
}

int aa_prepare(aa_ctx *h, double *cost)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    AA_CHECK_HIP(hipSetDevice(h->c.device));
    return prepare(&h->c, cost);
}

int aa_cost(aa_ctx *h, double *cost)
{
    AA_REQUIRE(h && cost, AA_ERR_ARG, "null argument");
    AA_REQUIRE(h->c.grams_valid, AA_ERR_STATE, "Gram products not valid");
    AA_CHECK_HIP(hipSetDevice(h->c.device));
    return device_cost(&h->c, cost);
}

int aa_get_grams(aa_ctx *h, double *ZtZ, double *CKCt, double *CKZ, double *trace)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_REQUIRE(c->grams_valid, AA_ERR_STATE, "Gram products not valid");
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(sync_host_grams(c));
    const size_t kk = (size_t)c->k * c->k;
    if (ZtZ) memcpy(ZtZ, c->ZtZ.data(), kk * sizeof(double));
    if (CKCt) memcpy(CKCt, c->CKCt.data(), kk * sizeof(double));
    if (CKZ) memcpy(CKZ, c->CKZ.data(), kk * sizeof(double));
    if (trace) *trace = c->trace;
    return AA_OK;
}

int aa_set_dictionary_inputs(aa_ctx *h, const double *KZ, const double *ZtZ, double trace)
{
    AA_REQUIRE(h && KZ && ZtZ, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state, AA_ERR_STATE, "set_state first");
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(upload_tall(c, c->H, KZ, c->k, 1, c->n, c->k));
    {   // Z'Z goes to the device Gram state (padded to KP x KP)
        std::vector<double> pad((size_t)c->KP * c->KP, 0.0);
        for (int i = 0; i < c->k; ++i)
            for (int j = 0; j < c->k; ++j) pad[(size_t)i * c->KP + j] = ZtZ[(size_t)i * c->k + j];
        AA_CHECK_HIP(ctx_memcpy(c, dev_ZtZ(c), pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    c->host_grams_valid = false;
    c->trace = trace;
    c->have_trace = true;
    c->dict_inputs_overridden = true;
    return AA_OK;
}

int aa_dictionary_update(aa_ctx *h, const aa_spg_params *params, aa_spg_stats *stats)
{
    AA_REQUIRE(h && params, AA_ERR_ARG, "null argument");
    AA_CHECK_HIP(hipSetDevice(h->c.device));
    return dictionary_update(&h->c, params, stats, DictCall{});
}

int aa_weights_update(aa_ctx *h, const aa_qp_params *params, aa_qp_stats *stats)
{
    AA_REQUIRE(h && params, AA_ERR_ARG, "null argument");
    AA_CHECK_HIP(hipSetDevice(h->c.device));
    return weights_update(&h->c, params, stats);
}

// One outer iteration of AA, enqueued: the scale-factor stage (scale_spg set), the dictionary update or
// the carry of its cost, the weights update or the carry of its cost.  cd == nullptr: no cost is
// recorded.  jd: the iteration's judge -- it rides in the kernel of the iteration's last cost, or
// stands alone behind the carry -- and the snapshot behind it; nullptr (aa_outer_iterations: both
// updates, no loop control): neither.
static int aa_enqueue_iteration(Ctx *c, const aa_spg_params *spg, const aa_qp_params *qp,
                                const aa_spg_params *scale_spg, double delta, bool upd_dict, bool upd_w,
                                double *cd, int *slot, const LoopJudge *jd)
{
    AA_REQUIRE(jd || (upd_dict && upd_w && !scale_spg), AA_ERR_ARG,
               "an AA iteration without a judge runs both updates and no scale-factor stage");
    if (scale_spg) {
        // archetypal_analysis.py:590-609: the Gram state of the previous weights refresh
        // (Z'Z, C K C', C K Z) is what the k-vector problem is made of
        AA_CHECK(ensure_ckz(c));
        AA_CHECK(launch_scale_factors(c, scale_spg, delta, *jd, cd, slot));
    }
    if (upd_dict) {
        bool recorded = false;
        DictCall call;
        call.cost_out = cd;
        call.cost_slot = slot;
        call.cost_recorded = &recorded;
        call.weights_follow = upd_w;
        call.loop_update = true;                   // who reads the SPG tail: dict_tail_needed
        call.loop_judged = jd != nullptr;
        AA_CHECK(dictionary_update(c, spg, nullptr, call));
        if (cd && !recorded) {
            AA_CHECK(ensure_ckz(c));
            AA_CHECK(launch_aa_cost(c, cd, slot));
        }
    } else {
        AA_CHECK(launch_cost_carry(c, cd, slot, jd->cost0));
    }
    if (upd_w) {
        AA_CHECK(weights_update(c, qp, nullptr));
        if (cd) AA_CHECK(launch_aa_cost(c, cd, slot, jd));
        if (jd) AA_CHECK(launch_iter_judge(c, *jd, cd, true, false));
    } else {
        AA_CHECK(join_side(c));                    // the snapshot reads the dictionary the side stream steps
        AA_CHECK(launch_cost_carry(c, cd, slot, jd->cost0));
        AA_CHECK(launch_iter_judge(c, *jd, cd, false, false));
    }
    return AA_OK;
}

int aa_outer_iterations(aa_ctx *h, int n_outer, const aa_spg_params *spg, const aa_qp_params *qp,
                        double *costs)
{
    AA_REQUIRE(h && spg && qp, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    // costs are evaluated and kept on the device; the host waits once, at the end
    AA_CHECK(c->costDev.alloc((size_t)(2 * n_outer + 64) * sizeof(double)));
    AA_CHECK(c->costSlot.alloc(64));
    int *slot = c->costSlot.as<int>();
    double *cd = c->costDev.as<double>();
    AA_CHECK_HIP(hipMemsetAsync(slot, 0, sizeof(int), c->stream));
    auto one_iteration = [&]() -> int {
        return aa_enqueue_iteration(c, spg, qp, nullptr, 0.0, true, true, costs ? cd : nullptr, slot, nullptr);
    };
    // An outer iteration with one SPG iteration per dictionary update is a fixed sequence
    // of ~56 launches without host decisions, two thirds of them small dependent kernels:
    // after two eager iterations (warm state, every lazy allocation done) TWO iterations --
    // the gradient / Gram buffer pairs swap once per iteration -- are captured into a
    // hipGraph and replayed.  Single rank only (RCCL stays outside graphs).
    const bool graph = g_use_graph && c->world <= 1 && !c->force_comm && c->form == AA_FORM_DATA &&
                       spg->max_iterations == 1 && n_outer >= 8 && !g_qp_overlap_tail && !g_qp_live &&
                       !c->time_gemm;      // (timing events recorded inside a capture cannot be read)
    int i = 0;
    const int eager = graph ? 2 : n_outer;
    for (; i < eager; ++i) AA_CHECK(one_iteration());
    if (graph) {
        const int pairs = (n_outer - i) / 2;
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        AA_CHECK_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        int rc = one_iteration();
        if (rc == AA_OK) rc = one_iteration();
        hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (rc != AA_OK || e != hipSuccess || !g) {
            if (rc == AA_OK) set_error("hipStreamEndCapture: %s (set option use_graph=0)", hipGetErrorString(e));
            if (g) (void)hipGraphDestroy(g);
            return rc != AA_OK ? rc : AA_ERR_HIP;   // host state has advanced: not recoverable
        }
        e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        for (int p = 0; p < pairs && e == hipSuccess; ++p) e = hipGraphLaunch(ge, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);    // the replays are still in flight
        if (ge) (void)hipGraphExecDestroy(ge);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) {
            set_error("hipGraph: %s (set option use_graph=0)", hipGetErrorString(e));
            return AA_ERR_HIP;
        }
        i += 2 * pairs;
        for (; i < n_outer; ++i) AA_CHECK(one_iteration());
    }
    // measurement only (tools/interleave_probe.py: several contexts enqueued round-robin by one host
    // thread): return with the work in flight; the next blocking call of this context waits for it
    if (g_outer_nosync && !costs) return AA_OK;
    if (costs && n_outer > 0)
        AA_CHECK_HIP(hipMemcpyAsync(costs, c->costDev.p, (size_t)2 * n_outer * sizeof(double),
                                    hipMemcpyDeviceToHost, c->stream));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK(proj_poll_multirank(c));
    return AA_OK;
}

// ------------------------------------------------------------------ the device loop of a single fit
// (aa_iterate, aa_gpnh_iterate.)  The host enqueues check_every iterations at a time; every iteration
// ends with its judge and the conditional snapshot (launch_iter_judge), and the host reads the status
// record once per batch.
struct LoopRecords {
    double *cd;             // costDev: two costs per iteration (64 spare entries behind them)
    int *slot;              // costSlot: the next free entry of cd
    IterState *st;
};

// the records of a loop of at most n_max iterations; counter and status zeroed on the stream.  Apart from
// run_device_loop because a family may have launches of its own between the two (GPNH: its initial cost)
static int loop_records_begin(Ctx *c, int n_max, LoopRecords *rec)
{
    AA_CHECK(c->costDev.alloc((size_t)(2 * n_max + 64) * sizeof(double)));
    AA_CHECK(c->costSlot.alloc(64));
    AA_CHECK(c->iterState.alloc(sizeof(IterState)));
    rec->cd = c->costDev.as<double>();
    rec->slot = c->costSlot.as<int>();
    rec->st = c->iterState.as<IterState>();
    AA_CHECK_HIP(hipMemsetAsync(rec->slot, 0, sizeof(int), c->stream));
    AA_CHECK_HIP(hipMemsetAsync(rec->st, 0, sizeof(IterState), c->stream));
    c->loop_spg_flags = 0;                       // the host's view of the zeroed record
    return AA_OK;
}

// enqueue(it): one outer iteration, judge and snapshot included.  restore(): the loop stopped behind the
// last iteration enqueued -- put the kept factors back and rebuild what depends on them.
// poll_multirank: every poll also reads the projections' deferred overflow state (AA).
// stop_not_definite: a set IterState::not_definite ends the loop as error stage 3 -- nothing is kept, the
// caller takes another route (GPNH).  *restored (nullable): whether restore() ran.
static int run_device_loop(Ctx *c, const LoopRecords &rec, const aa_iter_params *ip, double cost0, double *costs,
                           aa_iter_stats *stats, bool poll_multirank, bool stop_not_definite,
                           const std::function<int(int)> &enqueue, const std::function<int()> &restore,
                           bool *restored = nullptr)
{
    const int n_max = ip->max_outer;
    if (restored) *restored = false;
    IterState hs;
    memset(&hs, 0, sizeof(hs));
    int done = 0;
    while (done < n_max) {
        const int batch = n_max - done < ip->check_every ? n_max - done : ip->check_every;
        for (int b = 0; b < batch; ++b) AA_CHECK(enqueue(done + b));
        done += batch;
        AA_CHECK_HIP(hipMemcpyAsync(&hs, rec.st, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
        AA_CHECK_HIP(hipStreamSynchronize(c->stream));
        c->loop_spg_flags = hs.spg_flags;        // the next batch's dictionary updates consult it (dict_tail_needed)
        if (poll_multirank) AA_CHECK(proj_poll_multirank(c));
        if (hs.stop || (stop_not_definite && hs.not_definite)) break;
    }
    memset(stats, 0, sizeof(*stats));
    stats->reserved = done;                      /* iterations enqueued (>= n_iter + 1) */
    if (stop_not_definite && hs.not_definite) {
        stats->error_stage = 3;
        stats->n_iter = -1;
        stats->cost = cost0;
        return AA_OK;
    }
    const int last = hs.stop ? hs.stop_iter : n_max - 1;
    AA_CHECK_HIP(ctx_memcpy(c, costs, rec.cd, (size_t)2 * (last + 1) * sizeof(double), hipMemcpyDeviceToHost));
    stats->n_iter = last;
    stats->converged = hs.converged;
    stats->error_stage = hs.error_stage;
    stats->error_iter = hs.error_stage ? hs.stop_iter : -1;
    stats->spg_flags = hs.spg_flags;
    stats->cost = costs[2 * last + 1];
    // iterations behind the stopping one have run: their factors give way to the kept ones
    if (hs.stop && hs.stop_iter < done - 1 && !hs.error_stage) {
        AA_CHECK(restore());
        if (restored) *restored = true;
    }
    return AA_OK;
}

int aa_iterate(aa_ctx *h, const aa_iter_params *ip, const aa_spg_params *spg, const aa_qp_params *qp,
               const aa_spg_params *scale_spg, double cost0, double *costs, aa_iter_stats *stats)
{
    AA_REQUIRE(h && ip && spg && qp && costs && stats, AA_ERR_ARG, "null argument");
    AA_REQUIRE(ip->max_outer >= 1 && ip->check_every >= 1, AA_ERR_ARG, "bad iteration counts");
    AA_REQUIRE(ip->criterion == 0 || ip->criterion == 1, AA_ERR_ARG, "bad stopping criterion");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->have_state && c->grams_valid, AA_ERR_STATE, "aa_iterate needs aa_prepare first");
    const size_t tall_bytes = (size_t)c->n_pad * c->KP * sizeof(double);
    AA_CHECK(c->snapC.alloc(tall_bytes));
    AA_CHECK(c->snapZ.alloc(tall_bytes));
    AA_CHECK(c->snapAlpha.alloc(64 * sizeof(double)));
    LoopRecords rec;
    AA_CHECK(loop_records_begin(c, ip->max_outer, &rec));
    const bool scale = scale_spg != nullptr && ip->delta != 0.0;
    if (scale) AA_REQUIRE(scale_spg->memory <= 16, AA_ERR_ARG, "spg memory > 16 unsupported");
    auto enqueue = [&](int it) -> int {
        const LoopJudge jd = loop_judge(ip, it, cost0, rec.st, 1);
        return aa_enqueue_iteration(c, spg, qp, scale ? scale_spg : nullptr, ip->delta, ip->update_dictionary != 0,
                                    ip->update_weights != 0, rec.cd, rec.slot, &jd);
    };
    auto read_alpha = [&](const DevBuf &src) -> int {    // the host copy of alpha follows the device's
        std::vector<double> a(c->KP, 1.0);
        AA_CHECK_HIP(ctx_memcpy(c, a.data(), src.p, (size_t)c->KP * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < c->k; ++i) c->alpha[i] = a[i];
        return AA_OK;
    };
    auto restore = [&]() -> int {
        // the kept factors, and the products rebuilt from them (four passes over the data, once per fit)
        if (scale) AA_CHECK(read_alpha(c->snapAlpha));
        AA_CHECK_HIP(ctx_memcpy(c, c->Ct.p, c->snapC.p, tall_bytes, hipMemcpyDeviceToDevice));
        AA_CHECK_HIP(ctx_memcpy(c, c->Zt.p, c->snapZ.p, tall_bytes, hipMemcpyDeviceToDevice));
        c->products_valid = false;
        c->grams_valid = false;
        c->qp_iters_valid = false;
        AA_CHECK(prepare(c, nullptr));
        c->x_feasible = true;                    // came out of our own update
        return AA_OK;
    };
    bool restored = false;
    AA_CHECK(run_device_loop(c, rec, ip, cost0, costs, stats, true, false, enqueue, restore, &restored));
    if (scale && !restored) AA_CHECK(read_alpha(c->alphaDev));
    return AA_OK;
}

int aa_reconstruction_cost(aa_ctx *h, double *cost)
{
    AA_REQUIRE(h && cost, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state && c->grams_valid && c->form == AA_FORM_DATA, AA_ERR_STATE,
               "reconstruction cost needs prepared data-form state");
    AA_CHECK_HIP(hipSetDevice(c->device));
    double s = 0.0;
    AA_CHECK(launch_residual_cost(c, c->Zt.as<double>(), c->P.as<double>(), c->alphaDev.as<double>(), &s));
    *cost = 0.5 * s / (double)c->n_global;
    return AA_OK;
}

int aa_get_archetypes(aa_ctx *h, double *CX, long ld)
{
    AA_REQUIRE(h && CX, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->grams_valid && c->form == AA_FORM_DATA, AA_ERR_STATE, "no C X available");
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy2d(c, CX, (size_t)ld * sizeof(double), c->P.p, (size_t)c->p_pad * sizeof(double),
                             (size_t)c->p * sizeof(double), (size_t)c->k, hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_distance_column(aa_ctx *h, long j, double *d)
{
    AA_REQUIRE(h && d, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_data, AA_ERR_STATE, "no data");
    AA_REQUIRE(j >= 0 && j < c->n_global, AA_ERR_ARG, "row %ld out of range", j);
    AA_CHECK_HIP(hipSetDevice(c->device));
    const size_t es = esize(c);
    if (!c->tmpTall.p || c->tmpTall.bytes < (size_t)c->n * sizeof(double))
        AA_CHECK(c->tmpTall.alloc((size_t)c->n_pad * 32 * sizeof(double)));
    if (c->form == AA_FORM_DATA) {
        if (!c->wideScratch.p || c->wideScratch.bytes < (size_t)c->p_pad * sizeof(double))
            AA_CHECK(c->wideScratch.alloc((size_t)32 * c->p_pad * sizeof(double)));
        const long jl = j - c->row_offset;
        const bool own = jl >= 0 && jl < c->n;
        if ((c->world == 1 && !c->force_comm)) {
            AA_CHECK_HIP(hipMemcpyAsync(c->wideScratch.p,
                                        reinterpret_cast<unsigned char *>(c->X.p) + (size_t)jl * c->p_pad * es,
                                        (size_t)c->p_pad * es, hipMemcpyDeviceToDevice, c->stream));
        } else {
            // the owner publishes the row through a sum all-reduce of zero-filled buffers, all
            // on the device (no host staging)
            AA_CHECK(launch_row_broadcast(c, jl, own));
        }
        return launch_distance_column(c, jl, own ? 1 : 0, nullptr, d);
    }
    return launch_distance_column(c, j, 1, nullptr, d);
}

int aa_furthest_sum(aa_ctx *h, int k, long start_index, const int *exclude, int n_exclude, int extra_steps,
                    int *selected, int *tie)
{
    AA_REQUIRE(h && selected && tie, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_data, AA_ERR_STATE, "no data");
    AA_REQUIRE(c->world <= 1 && !c->force_comm, AA_ERR_STATE,
               "aa_furthest_sum is single-rank (row-sharded runs pull distance columns: aa_distance_column)");
    AA_REQUIRE(!c->kernel.kind, AA_ERR_STATE, "aa_furthest_sum: implicit kernels pull distance columns (aa_distance_column)");
    AA_REQUIRE(k >= 1 && k <= AA_MAX_K, AA_ERR_ARG, "k = %d out of range", k);
    AA_REQUIRE(start_index >= 0 && start_index < c->n, AA_ERR_ARG, "start index %ld out of range", start_index);
    AA_REQUIRE(n_exclude >= 0 && (n_exclude == 0 || exclude), AA_ERR_ARG, "bad exclude list");
    for (int e = 0; e < n_exclude; ++e)
        AA_REQUIRE(exclude[e] >= 0 && exclude[e] < c->n && exclude[e] != start_index, AA_ERR_ARG,
                   "excluded index %d out of range or equal to the start index", exclude[e]);
    AA_REQUIRE((long)k <= c->n - n_exclude, AA_ERR_ARG, "too few points for %d components", k);
    AA_CHECK_HIP(hipSetDevice(c->device));
    return launch_furthest_sum(c, k, (int)start_index, exclude, n_exclude, extra_steps < 0 ? 0 : extra_steps,
                               selected, tie);
}

int aa_get_furthest_sum_state(aa_ctx *h, long *n, int *k, double *sums, unsigned char *alive, double *column,
                              int *cur, int *tie, int *selected)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_data && c->fs_k > 0 && c->fsScratch.p, AA_ERR_STATE,
               "aa_get_furthest_sum_state: no selection has run on this data");
    if (n) *n = c->n;
    if (k) *k = c->fs_k;
    AA_CHECK_HIP(hipSetDevice(c->device));
    return fetch_furthest_sum_state(c, sums, alive, column, cur, tie, selected);
}

// ------------------------------------------------------------------ GPNH
int aa_gpnh_set_factors(aa_ctx *h, int k, const double *Wt, long ld, const double *Z)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(has_stored_data(c), AA_ERR_STATE, "GPNH needs a data matrix");
    AA_CHECK(ensure_problem(c, k));
    if (Wt) {
        AA_REQUIRE(ld >= c->p, AA_ERR_ARG, "ld < p");
        std::vector<double> tmp((size_t)c->KP * c->p_pad, 0.0);
        for (int i = 0; i < k; ++i)
            for (long q = 0; q < c->p; ++q) tmp[(size_t)i * c->p_pad + q] = Wt[(size_t)i * ld + q];
        AA_CHECK_HIP(ctx_memcpy(c, c->P.p, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
        AA_CHECK(launch_wide_to_T(c, c->P.as<double>(), operandT(c, c->P, c->Pw)));
        AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gr.as<double>()));   // XW
        c->gpnh_valid = true;
    }
    if (Z) {
        AA_CHECK(upload_tall(c, c->Zt, Z, k, 1, c->n, k));
        c->have_state = true;
    }
    return AA_OK;
}

int aa_gpnh_get_weights(aa_ctx *h, double *Z)
{
    AA_REQUIRE(h && Z, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state, AA_ERR_STATE, "no weights");
    AA_CHECK_HIP(hipSetDevice(c->device));
    return download_tall(c, c->Zt, Z, c->k, 1, c->n, c->k);
}

int aa_gpnh_reduce(aa_ctx *h, double *ZtX, long ld, double *ZtZ, double *trace_WtXtZ)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state, AA_ERR_STATE, "no weights");
    AA_CHECK_HIP(hipSetDevice(c->device));
    if (ZtX) {
        AA_CHECK(launch_reduce_rows(c, c->Zt.as<double>(), c->ZtX.as<double>(), nullptr));
        AA_CHECK_HIP(hipStreamSynchronize(c->stream));
        AA_CHECK_HIP(ctx_memcpy2d(c, ZtX, (size_t)ld * sizeof(double), c->ZtX.p, (size_t)c->p_pad * sizeof(double),
                                 (size_t)c->p * sizeof(double), (size_t)c->k, hipMemcpyDeviceToHost));
    }
    if (ZtZ) {
        AA_CHECK(launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), c->gramOut.as<double>()));
        std::vector<double> g;
        AA_CHECK(fetch_gram(c, c->gramOut.as<double>(), g));
        memcpy(ZtZ, g.data(), g.size() * sizeof(double));
    }
    if (trace_WtXtZ) {
        AA_REQUIRE(c->gpnh_valid, AA_ERR_STATE, "no dictionary");
        AA_CHECK(launch_tall_dot_scaled(c, c->Gr.as<double>(), c->Zt.as<double>(), nullptr, SC_S1));
        AA_CHECK_HIP(hipMemcpyAsync(trace_WtXtZ, c->scalars.as<double>() + SC_S1, sizeof(double),
                                    hipMemcpyDeviceToHost, c->stream));
        AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    }
    return AA_OK;
}

int aa_gpnh_weights_update(aa_ctx *h, const double *WtW, const aa_qp_params *params, aa_qp_stats *stats)
{
    AA_REQUIRE(h && WtW && params, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state && c->gpnh_valid, AA_ERR_STATE, "set_factors first");
    AA_CHECK_HIP(hipSetDevice(c->device));
    return launch_qp(c, WtW, c->Gr.as<double>(), 1, c->KP, nullptr, c->Zt.as<double>(), c->KP, c->n, c->k,
                     params, nullptr, stats);
}

int aa_gpnh_get_dictionary(aa_ctx *h, double *Wt, long ld)
{
    AA_REQUIRE(h && Wt, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->gpnh_valid, AA_ERR_STATE, "no dictionary");
    AA_REQUIRE(ld >= c->p, AA_ERR_ARG, "ld < p");
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy2d(c, Wt, (size_t)ld * sizeof(double), c->P.p, (size_t)c->p_pad * sizeof(double),
                             (size_t)c->p * sizeof(double), (size_t)c->k, hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_gpnh_iterate(aa_ctx *h, const aa_gpnh_params *gp, const aa_qp_params *qp, double *cost0_out,
                    double *costs, aa_iter_stats *stats)
{
    AA_REQUIRE(h && gp && qp && costs && stats, AA_ERR_ARG, "null argument");
    const aa_iter_params *ip = &gp->loop;
    AA_REQUIRE(ip->max_outer >= 1 && ip->check_every >= 1, AA_ERR_ARG, "bad iteration counts");
    AA_REQUIRE(ip->criterion == 0 || ip->criterion == 1, AA_ERR_ARG, "bad stopping criterion");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->have_state && c->gpnh_valid && c->form == AA_FORM_DATA, AA_ERR_STATE,
               "aa_gpnh_iterate needs aa_gpnh_set_factors (dictionary and weights) first");
    const int n_max = ip->max_outer, KP = c->KP;
    const double lambda = gp->lambda_W;
    size_t snap_bytes = (size_t)c->n_pad * KP * sizeof(double);
    if ((size_t)KP * c->p_pad * sizeof(double) > snap_bytes) snap_bytes = (size_t)KP * c->p_pad * sizeof(double);
    AA_CHECK(c->snapC.alloc(snap_bytes));
    AA_CHECK(c->snapZ.alloc(snap_bytes));
    AA_CHECK(c->qpIters.alloc((size_t)c->n * sizeof(int)));
    AA_CHECK(ensure_trace(c));
    for (int i = 0; i < c->k; ++i) c->alpha[i] = 1.0;            // the QP set-up scales by alpha
    AA_CHECK(upload_alpha(c));
    LoopRecords rec;
    AA_CHECK(loop_records_begin(c, n_max, &rec));
    double *cd = rec.cd;
    int *slot = rec.slot;
    // Gram state: [0] = Z'Z, [1] = W'W; scal[SC_S1] = tr(W'X'Z) = <XW, Z>
    AA_CHECK(launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), dev_ZtZ(c)));
    AA_CHECK(launch_gram_wide(c, c->P.as<double>(), c->P.as<double>(), dev_CKCt(c)));
    // tr(W'X'Z) = <Z'X, W'>: with Z'X of the current weights at hand (the dictionary solve needs it
    // anyway) the cost takes no pass over the n rows at all
    AA_CHECK(launch_reduce_rows(c, c->Zt.as<double>(), c->ZtX.as<double>(), nullptr));
    bool ztx_current = true;
    AA_CHECK(launch_gpnh_cost(c, lambda, cd + 2 * n_max + 8, nullptr, true));
    double cost0 = 0.0;
    AA_CHECK_HIP(hipMemcpyAsync(&cost0, cd + 2 * n_max + 8, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    if (cost0_out) *cost0_out = cost0;
    c->grams_valid = false;          // the Gram state now holds GPNH products, not AA ones
    c->ckz_valid = false;
    c->host_grams_valid = false;

    auto enqueue = [&](int it) -> int {
        const LoopJudge jd = loop_judge(ip, it, cost0, rec.st, 0 /* no SPG behind the dictionary */);
        if (ip->update_dictionary) {
            if (!ztx_current) AA_CHECK(launch_reduce_rows(c, c->Zt.as<double>(), c->ZtX.as<double>(), nullptr));
            ztx_current = true;
            AA_CHECK(launch_gpnh_solve(c, lambda, &rec.st->not_definite));              // W'
            AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gr.as<double>()));   // X W
            const bool gram_in_cost = gpnh_cost_can_gram(c);
            if (!gram_in_cost) AA_CHECK(launch_gram_wide(c, c->P.as<double>(), c->P.as<double>(), dev_CKCt(c)));
            AA_CHECK(launch_gpnh_cost(c, lambda, cd, slot, true, gram_in_cost));
        } else {
            AA_CHECK(launch_cost_carry(c, cd, slot, cost0));
        }
        if (ip->update_weights) {
            AA_CHECK(launch_qp(c, nullptr, c->Gr.as<double>(), 1, KP, nullptr, c->Zt.as<double>(), KP, c->n,
                               c->k, qp, c->qpIters.as<int>(), nullptr, dev_CKCt(c)));
            c->qp_iters_valid = true;
            AA_CHECK(launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), dev_ZtZ(c)));
            AA_CHECK(launch_reduce_rows(c, c->Zt.as<double>(), c->ZtX.as<double>(), nullptr));   // also the next solve's
            ztx_current = true;
            AA_CHECK(launch_gpnh_cost(c, lambda, cd, slot, true, false, &jd));   // the judge rides in the cost kernel
            AA_CHECK(launch_iter_judge(c, jd, cd, true, true));
        } else {
            AA_CHECK(launch_cost_carry(c, cd, slot, cost0));
            AA_CHECK(launch_iter_judge(c, jd, cd, false, true));
        }
        return AA_OK;
    };
    auto restore = [&]() -> int {
        // the kept factors, X W rebuilt from them
        AA_CHECK_HIP(ctx_memcpy(c, c->Zt.p, c->snapZ.p, (size_t)c->n_pad * KP * sizeof(double), hipMemcpyDeviceToDevice));
        AA_CHECK_HIP(ctx_memcpy(c, c->P.p, c->snapC.p, (size_t)KP * c->p_pad * sizeof(double), hipMemcpyDeviceToDevice));
        AA_CHECK(launch_wide_to_T(c, c->P.as<double>(), operandT(c, c->P, c->Pw)));
        AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gr.as<double>()));
        c->qp_iters_valid = false;
        AA_CHECK_HIP(hipStreamSynchronize(c->stream));
        return AA_OK;
    };
    // the normal equations not positive definite: the loop ends, the caller solves them another way
    return run_device_loop(c, rec, ip, cost0, costs, stats, false, true, enqueue, restore);
}

// ------------------------------------------------------------------ restart slots: the host steps both families share
// (AA: aa_slots_*, GPNH: aa_gpnh_slots_*.)  Restart r lives in columns [r k, (r + 1) k) of the tall arrays
// and rows [r k, (r + 1) k) of the wide ones; per slot there is a cost record, a counter, an IterState
// and an initial cost (Ctx::slot*).

// begin, the common part: whatever an earlier slot run of either family left -- ended or not -- gives way
// to fresh, zeroed factor arrays of R k components; trace, unit scale factors, the slot geometry, the
// per-slot records allocated.  The callers check their arguments and do everything family-specific.
static int slots_begin_common(Ctx *c, int R, int k, int max_outer)
{
    c->slots_aa = false;
    c->slots_started = false;
    c->products_valid = false;
    c->k = 0;                                         // force fresh, zeroed factor arrays
    AA_CHECK(ensure_problem(c, R * k));
    AA_CHECK(ensure_trace(c));
    for (int i = 0; i < c->k; ++i) c->alpha[i] = 1.0;
    AA_CHECK(upload_alpha(c));
    c->slots_R = R;
    c->slots_k = k;
    c->slots_max_outer = max_outer;
    c->slots_stride = 2 * max_outer + 64;
    AA_CHECK(c->slotCosts.alloc((size_t)R * c->slots_stride * sizeof(double)));
    AA_CHECK(c->slotCounters.alloc(64 * sizeof(int)));
    AA_CHECK(c->slotStates.alloc(32 * sizeof(IterState)));
    AA_CHECK(c->slotCost0.alloc(32 * sizeof(double)));
    return AA_OK;
}

// every slot empty (stop = 1: the judge leaves it alone), every counter zero
static int slots_empty_records(Ctx *c)
{
    std::vector<IterState> st(32);
    memset(st.data(), 0, st.size() * sizeof(IterState));
    for (int r = 0; r < 32; ++r) st[r].stop = 1;
    AA_CHECK_HIP(ctx_memcpy(c, c->slotStates.p, st.data(), st.size() * sizeof(IterState), hipMemcpyHostToDevice));
    AA_CHECK_HIP(ctx_memset(c, c->slotCounters.p, 0, 64 * sizeof(int)));
    return AA_OK;
}

// slot r takes a new restart: running state, no iteration counted
static int slot_clear_record(Ctx *c, int r)
{
    IterState zero;
    memset(&zero, 0, sizeof(zero));
    AA_CHECK_HIP(ctx_memcpy(c, c->slotStates.as<IterState>() + r, &zero, sizeof(zero), hipMemcpyHostToDevice));
    AA_CHECK_HIP(ctx_memset(c, c->slotCounters.as<int>() + r, 0, sizeof(int)));
    return AA_OK;
}

// columns [o, o + slots_k) of a tall device array (row stride KP) <-> a dense n x slots_k host array
static int slot_put_tall(Ctx *c, DevBuf &dst, int o, const double *src)
{
    const size_t w = (size_t)c->slots_k * sizeof(double);
    AA_CHECK_HIP(ctx_memcpy2d(c, dst.as<double>() + o, (size_t)c->KP * sizeof(double), src, w, w, (size_t)c->n,
                             hipMemcpyHostToDevice));
    return AA_OK;
}

static int slot_get_tall(Ctx *c, const DevBuf &src, int o, double *dst)
{
    const size_t w = (size_t)c->slots_k * sizeof(double);
    AA_CHECK_HIP(ctx_memcpy2d(c, dst, w, src.as<double>() + o, (size_t)c->KP * sizeof(double), w, (size_t)c->n,
                             hipMemcpyDeviceToHost));
    return AA_OK;
}

// the same columns <-> the caller's slots_k x n array C (leading dimension ldc): transposed on the host
static int slot_put_tall_T(Ctx *c, DevBuf &dst, int o, const double *C, long ldc)
{
    const int k = c->slots_k;
    std::vector<double> ct((size_t)c->n * k);
    for (long row = 0; row < c->n; ++row)
        for (int i = 0; i < k; ++i) ct[(size_t)row * k + i] = C[(size_t)i * ldc + row];
    return slot_put_tall(c, dst, o, ct.data());
}

static int slot_get_tall_T(Ctx *c, const DevBuf &src, int o, double *C, long ldc)
{
    const int k = c->slots_k;
    std::vector<double> ct((size_t)c->n * k);
    AA_CHECK(slot_get_tall(c, src, o, ct.data()));
    for (long row = 0; row < c->n; ++row)
        for (int i = 0; i < k; ++i) C[(size_t)i * ldc + row] = ct[(size_t)row * k + i];
    return AA_OK;
}

// rows [o, o + slots_k) of a wide device array (row stride p_pad) <-> a slots_k x p host array (leading dimension ld)
static int slot_put_wide(Ctx *c, DevBuf &dst, int o, const double *src, long ld)
{
    AA_CHECK_HIP(ctx_memcpy2d(c, dst.as<double>() + (size_t)o * c->p_pad, (size_t)c->p_pad * sizeof(double), src,
                             (size_t)ld * sizeof(double), (size_t)c->p * sizeof(double), (size_t)c->slots_k,
                             hipMemcpyHostToDevice));
    return AA_OK;
}

static int slot_get_wide(Ctx *c, const DevBuf &src, int o, double *dst, long ld)
{
    AA_CHECK_HIP(ctx_memcpy2d(c, dst, (size_t)ld * sizeof(double), src.as<double>() + (size_t)o * c->p_pad,
                             (size_t)c->p_pad * sizeof(double), (size_t)c->p * sizeof(double), (size_t)c->slots_k,
                             hipMemcpyDeviceToHost));
    return AA_OK;
}

// cost record (2 (stop_iter + 1) values) and initial cost of slot r, which must have stopped
static int slot_fetch_record(Ctx *c, int r, double *costs, double *cost0)
{
    IterState st;
    AA_CHECK_HIP(ctx_memcpy(c, &st, c->slotStates.as<IterState>() + r, sizeof(st), hipMemcpyDeviceToHost));
    AA_REQUIRE(st.stop, AA_ERR_STATE, "slot %d has not stopped", r);
    AA_CHECK_HIP(ctx_memcpy(c, costs, c->slotCosts.as<double>() + (size_t)r * c->slots_stride,
                           (size_t)2 * (st.stop_iter + 1) * sizeof(double), hipMemcpyDeviceToHost));
    AA_CHECK_HIP(ctx_memcpy(c, cost0, c->slotCost0.as<double>() + r, sizeof(double), hipMemcpyDeviceToHost));
    return AA_OK;
}

// the tail of a run call: waits for the iterations, status of every slot out.  flags: the SPG warning
// flags of the slot (AA) or "normal equations not positive definite" (GPNH: IterState::not_definite)
static int slots_read_status(Ctx *c, aa_slot_status *status, bool aa)
{
    const int R = c->slots_R;
    std::vector<IterState> st(R);
    std::vector<int> cnt(R);
    AA_CHECK_HIP(hipMemcpyAsync(st.data(), c->slotStates.p, (size_t)R * sizeof(IterState), hipMemcpyDeviceToHost, c->stream));
    AA_CHECK_HIP(hipMemcpyAsync(cnt.data(), c->slotCounters.p, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    for (int r = 0; r < R; ++r) {
        status[r].stop = st[r].stop;
        status[r].converged = st[r].converged;
        status[r].error_stage = st[r].error_stage;
        status[r].stop_iter = st[r].stop_iter;
        status[r].flags = aa ? st[r].spg_flags : st[r].not_definite;
        status[r].iterations_run = cnt[r] / 2;
    }
    return AA_OK;
}

// ------------------------------------------------------------------ AA restarts side by side
// (bin/run_hadisst_aa.py:149-174).  R independent fits of k components each in the
// component slots of ONE set of device arrays (restart r: columns [r k, (r + 1) k) of C' and Z): the
// passes over X, the Gram kernels, the gradient kernel (block-diagonal M) and the column
// projections are the single fit's launches on the stacked arrays -- an output column of theirs
// depends on its own column only -- and everything that couples the components of a fit (the SPG
// scalars, the line search, the QP Hessian, the cost, the judge) exists once per slot (ctx->slots_aa
// makes the launchers pick those forms; dictionary_update / weights_update themselves are the
// single fit's).  Every slot gets the bits it gets from aa_iterate on its own.  Production
// settings only: data form, one SPG iteration per dictionary update, delta = 0, single rank,
// fewer than 65 536 samples, k <= 16.
int aa_slots_begin(aa_ctx *h, int R, int k, const aa_iter_params *ip, const aa_spg_params *spg,
                   const aa_qp_params *qp, const aa_spg_params *scale_spg)
{
    AA_REQUIRE(h && ip && spg && qp, AA_ERR_ARG, "null argument");
    AA_REQUIRE(ip->delta == 0.0 || (scale_spg && scale_spg->memory <= 16), AA_ERR_ARG,
               "slots: delta != 0 needs the scale-factor SPG parameters (memory <= 16)");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(has_stored_data(c) && !c->linear_kernel, AA_ERR_STATE, "AA slots need a data matrix");
    AA_REQUIRE(c->world <= 1 && !c->force_comm, AA_ERR_STATE, "restart slots are single-rank");
    // R k <= 32: the tall kernels sum a column's rows in KP-dependent interleaved chains, so the slots
    // must run the kernels a single fit of k <= 16 components runs (KP = 32) to get its bits
    AA_REQUIRE(R >= 1 && k >= 1 && k <= 16 && R * k <= 32, AA_ERR_ARG,
               "slots: R = %d restarts of k = %d components do not fit 32 component slots", R, k);
    AA_REQUIRE(c->n < 65536, AA_ERR_ARG, "AA slots: fewer than 65 536 samples");
    AA_REQUIRE(ip->max_outer >= 1 && ip->update_dictionary && ip->update_weights, AA_ERR_ARG, "slots: both updates");
    AA_REQUIRE(spg->max_iterations == 1 && spg->memory <= 16, AA_ERR_ARG, "slots: one SPG iteration per dictionary update");
    AA_REQUIRE(g_fuse_finalize && g_proj_mode == 0, AA_ERR_STATE, "slots: default projection options");
    AA_CHECK(slots_begin_common(c, R, k, ip->max_outer));
    c->slots_ip = *ip;
    c->slots_sp = *spg;
    c->slots_qp = *qp;
    if (scale_spg) c->slots_scale_sp = *scale_spg;
    AA_CHECK(c->snapAlpha.alloc(64 * sizeof(double)));
    c->scalars.release();
    AA_CHECK(c->scalars.alloc((size_t)(R + 1) * AA_SC_STRIDE * sizeof(double)));      // one block per slot
    const size_t tall_bytes = (size_t)c->n_pad * c->KP * sizeof(double);
    AA_CHECK(c->snapC.alloc(tall_bytes));
    AA_CHECK(c->snapZ.alloc(tall_bytes));
    AA_CHECK(c->slotSnapP.alloc((size_t)c->KP * c->p_pad * sizeof(double)));
    AA_CHECK_HIP(ctx_memset(c, c->snapC.p, 0, tall_bytes));
    AA_CHECK_HIP(ctx_memset(c, c->snapZ.p, 0, tall_bytes));
    AA_CHECK(slots_empty_records(c));
    AA_CHECK_HIP(ctx_memset(c, c->Ct.p, 0, tall_bytes));
    AA_CHECK_HIP(ctx_memset(c, c->Zt.p, 0, tall_bytes));
    AA_CHECK_HIP(ctx_memset(c, c->Mdev.p, 0, (size_t)c->KP * c->KP * sizeof(double)));
    AA_CHECK_HIP(ctx_memset(c, c->gramOut.p, 0, (size_t)4 * c->KP * c->KP * sizeof(double)));
    c->slots_aa = true;
    c->have_state = true;
    c->grams_valid = false;
    c->products_valid = false;
    c->ckz_valid = false;
    c->dict_inputs_overridden = false;
    c->x_feasible = false;
    c->qp_iters_valid = false;
    for (int m = 0; m < 4; ++m) {                     // as aa_set_state: every fit starts its projections cold
        c->projWarm[m] = c->projWarm2[m] = false;
        c->projPassHint[m] = c->projPassHint2[m] = 0;
        c->projListShort[m] = false;
    }
    return AA_OK;
}

// the head of a load and of a reload: the caller's factors into slot r's columns of C' and Z (C: k x n,
// leading dimension ldc; Z: n x k), its record cleared, its scale factors set (null: ones)
static int slot_upload_aa(Ctx *c, int r, const double *C, long ldc, const double *Z, const double *alpha, bool running)
{
    const int o = r * c->slots_k;
    AA_CHECK(join_side(c));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK(slot_put_tall_T(c, c->Ct, o, C, ldc));
    AA_CHECK(slot_put_tall(c, c->Zt, o, Z));
    AA_CHECK(slot_clear_record(c, r));
    if (running) {   // the host copy follows the device's (the scale-factor kernel moves the running slots' factors)
        std::vector<double> a(c->KP, 1.0);
        AA_CHECK_HIP(ctx_memcpy(c, a.data(), c->alphaDev.p, (size_t)c->KP * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < c->k; ++i) c->alpha[i] = a[i];
    }
    for (int i = 0; i < c->slots_k; ++i) c->alpha[o + i] = alpha ? alpha[i] : 1.0;
    return upload_alpha(c);
}

// start factors of a restart into slot r; the first run call rebuilds the products of the stacked
// state (aa_prepare's passes) and forms the slots' initial costs
int aa_slots_load(aa_ctx *h, int r, const double *C, long ldc, const double *Z, const double *alpha)
{
    AA_REQUIRE(h && C && Z, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->slots_aa && r >= 0 && r < c->slots_R, AA_ERR_ARG, "slot %d out of range", r);
    AA_REQUIRE(ldc >= c->n, AA_ERR_ARG, "ldc < n");
    AA_CHECK(slot_upload_aa(c, r, C, ldc, Z, alpha, false));
    c->products_valid = false;
    c->grams_valid = false;
    c->slots_started = false;
    return AA_OK;
}

// a new restart into slot r of a RUNNING group (its previous occupant has stopped and been fetched):
// the factors, the products aa_prepare computes -- for this slot; the other slots keep the products
// they carry -- its initial cost; its next dictionary update is the cold one of a fit.
int aa_slots_reload(aa_ctx *h, int r, const double *C, long ldc, const double *Z, const double *alpha)
{
    AA_REQUIRE(h && C && Z, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->slots_aa && c->slots_started && r >= 0 && r < c->slots_R, AA_ERR_ARG, "slot %d out of range", r);
    AA_REQUIRE(ldc >= c->n, AA_ERR_ARG, "ldc < n");
    const int k = c->slots_k, o = r * k, KP = c->KP;
    AA_CHECK(slot_upload_aa(c, r, C, ldc, Z, alpha, true));
    // a fit starts its projections cold (aa_set_state): a warm threshold of +inf selects nothing, which
    // is the cold start of k_proj_small -- for this slot's columns, in both projection states
    {
        std::vector<double> inf(k, INFINITY);
        DevBuf *states[2] = {&c->proj, &c->proj2};
        for (DevBuf *b : states) {
            if (!b->p) continue;
            ProjState *ps = b->as<ProjState>();
            for (int m = 1; m < 4; ++m)
                AA_CHECK_HIP(ctx_memcpy(c, &ps->warm[m][o], inf.data(), (size_t)k * sizeof(double), hipMemcpyHostToDevice));
        }
    }
    // products: aa_prepare's passes on the stacked state; what the RUNNING slots carry (C X, (C X X')',
    // (C X)(C X)') is put back afterwards -- the rest (Z'Z, X X'Z, C X X'Z) comes out as it was
    const size_t wide = (size_t)KP * c->p_pad * sizeof(double), tall = (size_t)c->n_pad * KP * sizeof(double);
    const size_t GS = (size_t)KP * KP;
    AA_CHECK(c->slotSaveP.alloc(wide));
    AA_CHECK(c->slotSaveGr.alloc(tall + GS * sizeof(double)));
    AA_CHECK_HIP(ctx_memcpy(c, c->slotSaveP.p, c->P.p, wide, hipMemcpyDeviceToDevice));
    AA_CHECK_HIP(ctx_memcpy(c, c->slotSaveGr.p, c->Gr.p, tall, hipMemcpyDeviceToDevice));
    double *saveCKCt = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(c->slotSaveGr.p) + tall);
    AA_CHECK_HIP(ctx_memcpy(c, saveCKCt, dev_CKCt(c), GS * sizeof(double), hipMemcpyDeviceToDevice));
    c->products_valid = false;
    c->grams_valid = false;
    AA_CHECK(prepare(c, nullptr));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    const unsigned loaded = c->slots_cold | (1u << r);
    for (int q = 0; q < c->slots_R; ++q) {
        if ((loaded >> q) & 1u) continue;                 // freshly loaded slots keep what prepare computed
        const int oq = q * k;
        AA_CHECK_HIP(ctx_memcpy(c, c->P.as<double>() + (size_t)oq * c->p_pad, c->slotSaveP.as<double>() + (size_t)oq * c->p_pad,
                               (size_t)k * c->p_pad * sizeof(double), hipMemcpyDeviceToDevice));
        AA_CHECK_HIP(ctx_memcpy2d(c, c->Gr.as<double>() + oq, (size_t)KP * sizeof(double),
                                 c->slotSaveGr.as<double>() + oq, (size_t)KP * sizeof(double),
                                 (size_t)k * sizeof(double), (size_t)c->n_pad, hipMemcpyDeviceToDevice));
        AA_CHECK_HIP(ctx_memcpy2d(c, dev_CKCt(c) + (size_t)oq * KP + oq, (size_t)KP * sizeof(double),
                                 saveCKCt + (size_t)oq * KP + oq, (size_t)KP * sizeof(double),
                                 (size_t)k * sizeof(double), (size_t)k, hipMemcpyDeviceToDevice));
    }
    if (c->dtype == AA_F32) AA_CHECK(launch_wide_to_T(c, c->P.as<double>(), operandT(c, c->P, c->Pw)));
    c->slots_cold = loaded;
    c->slots_cold_cols = 0u;
    for (int q = 0; q < c->slots_R; ++q)
        if ((loaded >> q) & 1u)
            for (int i = 0; i < k; ++i) c->slots_cold_cols |= 1u << (q * k + i);
    // initial cost of the new slot only (launch_aa_cost_slots takes all slots: the others' cost0 is
    // rewritten with the same bits -- their Gram blocks are what they were)
    std::vector<double> c0(32);
    AA_CHECK_HIP(ctx_memcpy(c, c0.data(), c->slotCost0.p, 32 * sizeof(double), hipMemcpyDeviceToHost));
    AA_CHECK(launch_aa_cost_slots(c, 0, JudgeRule{}));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    for (int q = 0; q < c->slots_R; ++q)
        if (q != r)
            AA_CHECK_HIP(ctx_memcpy(c, c->slotCost0.as<double>() + q, &c0[q], sizeof(double), hipMemcpyHostToDevice));
    return AA_OK;
}

// n_iters outer iterations of every slot; status[R] out.  The first call after the loads prepares the
// stacked state the way aa_set_state + aa_prepare prepare a single fit: the slots of the first group
// start together, with the cold dictionary update of a fit (the caller's factors projected, the products
// recomputed).  A slot freed later is refilled while the others run (aa_slots_reload): slots_cold marks
// it, and the next update is cold for its columns only.
int aa_slots_run(aa_ctx *h, int n_iters, aa_slot_status *status)
{
    AA_REQUIRE(h && status && n_iters >= 1, AA_ERR_ARG, "bad argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->slots_aa && c->slots_R > 0, AA_ERR_STATE, "aa_slots_begin first");
    if (!c->slots_started) {
        c->x_feasible = false;
        AA_CHECK(prepare(c, nullptr));
        AA_CHECK(launch_aa_cost_slots(c, 0, JudgeRule{}));
        c->slots_started = true;
        c->slots_cold = slots_all_mask(c);
        c->slots_cold_cols = 0xffffffffu;
    }
    // the rule of every slot's judge; iteration, initial cost and status are the slot's own
    const LoopJudge slots_judge = loop_judge(&c->slots_ip, 0, 0.0, nullptr, 1);
    bool recorded = false;
    DictCall call;
    call.cost_out = c->slotCosts.as<double>();
    call.cost_slot = c->slotCounters.as<int>();
    call.cost_recorded = &recorded;
    for (int it = 0; it < n_iters; ++it) {
        if (c->slots_ip.delta != 0.0) {           // archetypal_analysis.py:590-609, once per slot
            AA_CHECK(ensure_ckz(c));
            AA_CHECK(launch_scale_factors(c, &c->slots_scale_sp, c->slots_ip.delta, slots_judge, nullptr, nullptr));
        }
        if (c->slots_cold) {                      // (aa_slots_reload) the cold update of the freshly loaded slots
            c->x_feasible = false;
            c->products_valid = false;
        }
        AA_CHECK(dictionary_update(c, &c->slots_sp, nullptr, call));
        AA_REQUIRE(recorded, AA_ERR_STATE, "AA slots: the fused line search did not record the cost");
        c->slots_cold = 0;
        c->slots_cold_cols = 0xffffffffu;
        AA_CHECK(weights_update(c, &c->slots_qp, nullptr));
        AA_CHECK(launch_aa_cost_slots(c, 2, slots_judge.rule));
        AA_CHECK(launch_aa_snap_slots(c));
    }
    return slots_read_status(c, status, true);
}

// factors (C: k x n with leading dimension ldc, Z: n x k), C X (k x p, leading dimension ldx: recomputed
// from the fetched C, or -- carried != 0 -- as the loop carried it at the stopping iteration), cost record
// and initial cost of a stopped slot
int aa_slots_fetch(aa_ctx *h, int r, double *C, long ldc, double *Z, double *CX, long ldx, int carried,
                   double *costs, double *cost0, double *alpha)
{
    AA_REQUIRE(h && C && Z && costs && cost0 && CX, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->slots_aa && r >= 0 && r < c->slots_R, AA_ERR_ARG, "slot %d out of range", r);
    AA_REQUIRE(ldc >= c->n, AA_ERR_ARG, "ldc < n");
    AA_REQUIRE(ldx >= c->p, AA_ERR_ARG, "ldx < p");
    AA_CHECK(join_side(c));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK(slot_fetch_record(c, r, costs, cost0));
    const int k = c->slots_k, o = r * k;
    AA_CHECK(slot_get_tall_T(c, c->snapC, o, C, ldc));        // the factors of the stopping iteration
    AA_CHECK(slot_get_tall(c, c->snapZ, o, Z));
    if (alpha)                                                // ... and its scale factors
        AA_CHECK_HIP(ctx_memcpy(c, alpha, c->snapAlpha.as<double>() + o, (size_t)k * sizeof(double), hipMemcpyDeviceToHost));
    if (!carried) {
        // C X recomputed from the stopping iteration's dictionary: the pass aa_prepare runs (on the
        // scratch arrays of the dictionary update, free between iterations)
        AA_CHECK_HIP(ctx_memcpy(c, c->Dt.p, c->snapC.p, (size_t)c->n_pad * c->KP * sizeof(double), hipMemcpyDeviceToDevice));
        AA_CHECK(launch_reduce_rows(c, c->Dt.as<double>(), c->Q.as<double>(), nullptr));
        AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    }
    return slot_get_wide(c, carried ? c->slotSnapP : c->Q, o, CX, ldx);
}

// leaves the slot mode (the context can be used for single fits again)
int aa_slots_end(aa_ctx *h)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(join_side(c));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    c->slots_aa = false;
    c->slots_R = 0;
    c->slots_started = false;
    c->k = 0;                                         // the next aa_set_state sizes the arrays afresh
    c->have_state = false;
    c->gpnh_valid = false;                            // (the GPNH slot mode ends here too)
    c->grams_valid = false;
    c->ckz_valid = false;
    c->products_valid = false;
    c->qp_iters_valid = false;
    return AA_OK;
}

// ------------------------------------------------------------------ GPNH restarts side by side
// (kernels_tall.hip: RestartSlots; convex_dim_red/restarts.py drives it).  begin: R empty slots of k
// components each in one set of arrays; load: a restart's start factors into a slot, its initial
// cost; run: outer iterations for all slots, status of every slot back; fetch: factors and cost
// record of a slot that has stopped.  Single rank.
int aa_gpnh_slots_begin(aa_ctx *h, int R, int k, const aa_gpnh_params *gp, const aa_qp_params *qp)
{
    AA_REQUIRE(h && gp && qp, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(has_stored_data(c), AA_ERR_STATE, "GPNH needs a data matrix");
    AA_REQUIRE(c->world <= 1 && !c->force_comm, AA_ERR_STATE, "restart slots are single-rank");
    AA_REQUIRE(R >= 1 && k >= 1 && k <= 32 && R * k <= AA_MAX_K && R <= 32, AA_ERR_ARG,
               "slots: R = %d restarts of k = %d components do not fit", R, k);
    const aa_iter_params *ip = &gp->loop;
    AA_REQUIRE(ip->max_outer >= 1 && ip->update_dictionary && ip->update_weights, AA_ERR_ARG,
               "slots: both updates, max_outer >= 1");
    AA_REQUIRE(ip->criterion == 0 || ip->criterion == 1, AA_ERR_ARG, "bad stopping criterion");
    AA_REQUIRE(qp->max_iterations >= 1 && qp->memory <= 8, AA_ERR_ARG, "slots: QP max_iterations >= 1, memory <= 8");
    AA_REQUIRE(qp->max_iterations <= 4 || (qp->memory <= 1 && k <= 16 && c->n < 65536), AA_ERR_ARG,
               "slots: QPs of more than four passes need memory 1, k <= 16, fewer than 65 536 samples");
    AA_CHECK(slots_begin_common(c, R, k, ip->max_outer));
    c->slots_gp = *gp;
    c->slots_qp = *qp;
    size_t snap_bytes = (size_t)c->n_pad * c->KP * sizeof(double);
    if ((size_t)c->KP * c->p_pad * sizeof(double) > snap_bytes) snap_bytes = (size_t)c->KP * c->p_pad * sizeof(double);
    AA_CHECK(c->snapC.alloc(snap_bytes));
    AA_CHECK(c->snapZ.alloc(snap_bytes));
    AA_CHECK(slots_empty_records(c));
    AA_CHECK_HIP(ctx_memset(c, c->Zt.p, 0, (size_t)c->n_pad * c->KP * sizeof(double)));
    AA_CHECK_HIP(ctx_memset(c, c->P.p, 0, (size_t)c->KP * c->p_pad * sizeof(double)));
    AA_CHECK_HIP(ctx_memset(c, c->gramState.p, 0, (size_t)3 * c->KP * c->KP * sizeof(double)));
    c->gpnh_valid = true;
    c->have_state = true;
    c->grams_valid = false;
    c->ckz_valid = false;
    c->host_grams_valid = false;
    c->qp_iters_valid = false;
    return AA_OK;
}

int aa_gpnh_slots_load(aa_ctx *h, int r, const double *Wt, long ld, const double *Z)
{
    AA_REQUIRE(h && Wt && Z, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->slots_R > 0 && r >= 0 && r < c->slots_R, AA_ERR_ARG, "slot %d out of range", r);
    AA_REQUIRE(ld >= c->p, AA_ERR_ARG, "ld < p");
    const int o = r * c->slots_k;
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK(slot_put_wide(c, c->P, o, Wt, ld));
    AA_CHECK(slot_put_tall(c, c->Zt, o, Z));
    AA_CHECK(slot_clear_record(c, r));
    // the products of the stacked factors (the other slots' parts come out as they were) and this
    // slot's initial cost, the way aa_gpnh_iterate forms it
    AA_CHECK(launch_wide_to_T(c, c->P.as<double>(), operandT(c, c->P, c->Pw)));
    AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gr.as<double>()));          // X W
    AA_CHECK(launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), dev_ZtZ(c)));
    AA_CHECK(launch_gram_wide(c, c->P.as<double>(), c->P.as<double>(), dev_CKCt(c)));
    AA_CHECK(launch_reduce_rows(c, c->Zt.as<double>(), c->ZtX.as<double>(), nullptr));
    AA_CHECK(launch_gpnh_cost_slots(c, c->slots_gp.lambda_W, 1u << r, 0, JudgeRule{}, false));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    return AA_OK;
}

int aa_gpnh_slots_run(aa_ctx *h, int n_iters, aa_slot_status *status)
{
    AA_REQUIRE(h && status && n_iters >= 1, AA_ERR_ARG, "bad argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->slots_R > 0, AA_ERR_STATE, "aa_gpnh_slots_begin first");
    const int R = c->slots_R, k = c->slots_k;
    const double lambda = c->slots_gp.lambda_W;
    const JudgeRule rule = loop_judge(&c->slots_gp.loop, 0, 0.0, nullptr, 0).rule;   // of every slot's judge
    const unsigned all = slots_all_mask(c);
    // the single fit forms W'W inside its cost kernel when the factor is small (gpnh_cost_can_gram
    // with ITS k); the slots follow the same rule so that every restart sees the same bits
    const bool gram_in_cost = k * k <= 256 && (long)k * c->p_pad <= 4096;
    for (int it = 0; it < n_iters; ++it) {
        AA_CHECK(launch_gpnh_solve_slots(c, lambda));                                      // W'
        AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gr.as<double>()));       // X W
        if (!gram_in_cost) AA_CHECK(launch_gram_wide(c, c->P.as<double>(), c->P.as<double>(), dev_CKCt(c)));
        AA_CHECK(launch_gpnh_cost_slots(c, lambda, all, 1, rule, gram_in_cost));
        // at most four SPG passes per QP: the lane-per-sample kernel, as in a single fit; more: the
        // four-lane and wave-per-sample kernels of the AA slots (the Hessian blocks are W'W's)
        if (c->slots_qp.max_iterations <= 4) AA_CHECK(launch_qp_slots(c, R, k, dev_CKCt(c), &c->slots_qp));
        else AA_CHECK(launch_qp_slots_aa(c, &c->slots_qp));
        AA_CHECK(launch_gram_tall(c, c->Zt.as<double>(), c->Zt.as<double>(), dev_ZtZ(c)));
        AA_CHECK(launch_reduce_rows(c, c->Zt.as<double>(), c->ZtX.as<double>(), nullptr));
        AA_CHECK(launch_gpnh_cost_slots(c, lambda, all, 2, rule, false));
        AA_CHECK(launch_gpnh_snap_slots(c));
    }
    return slots_read_status(c, status, false);
}

int aa_gpnh_slots_fetch(aa_ctx *h, int r, double *Wt, long ld, double *Z, double *costs, double *cost0)
{
    AA_REQUIRE(h && Wt && Z && costs && cost0, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_REQUIRE(c->slots_R > 0 && r >= 0 && r < c->slots_R, AA_ERR_ARG, "slot %d out of range", r);
    AA_REQUIRE(ld >= c->p, AA_ERR_ARG, "ld < p");
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK(slot_fetch_record(c, r, costs, cost0));
    const int o = r * c->slots_k;
    AA_CHECK(slot_get_wide(c, c->snapC, o, Wt, ld));          // the factors of the stopping iteration (k_gpnh_snap_slots)
    return slot_get_tall(c, c->snapZ, o, Z);
}

int aa_gpnh_residual_cost(aa_ctx *h, double *cost)
{
    AA_REQUIRE(h && cost, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state && c->gpnh_valid, AA_ERR_STATE, "set_factors first");
    AA_CHECK_HIP(hipSetDevice(c->device));
    double s = 0.0;
    AA_CHECK(launch_residual_cost(c, c->Zt.as<double>(), c->P.as<double>(), nullptr, &s));
    *cost = 0.5 * s / (double)c->n_global;
    return AA_OK;
}

int aa_gpnh_residual_scores(aa_ctx *h, double *col_sse, double *row_sse, double *sse)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_ARG,
               "aa_gpnh_residual_scores is single-rank (the multi-rank form needs an all-reduce of the column sums)");
    AA_REQUIRE(has_stored_data(c), AA_ERR_STATE, "aa_gpnh_residual_scores needs a stored data matrix (data form)");
    AA_REQUIRE(c->have_state && c->gpnh_valid, AA_ERR_STATE, "set_factors first");
    AA_CHECK_HIP(hipSetDevice(c->device));
    return launch_residual_scores(c, col_sse, row_sse, sse);
}

// ------------------------------------------------------------------ KernelAA.transform
// the reference rows X_S and V = D' on them for the cross product of kernel `spec` against the resident rows, and
// the squared norms where the kind's product reads them.  The context names the reference set (cross, cross_s)
// once everything of it is in place; until then it has none
static int set_kernel_reference(aa_ctx *h, const KernelSpec &spec, int k, const double *XS, long s, long p, long ld,
                                const double *V, long ldv)
{
    AA_REQUIRE(h && XS && V, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_STATE, "the implicit %s kernel is single-rank", spec.name());
    AA_REQUIRE(has_stored_data(c) && c->dtype == AA_F64, AA_ERR_STATE,
               "aa_set_%s_reference needs the new samples as a float64 data matrix (aa_set_data)", spec.stem());
    AA_REQUIRE(s >= 1 && p == c->p && ld >= p && ldv >= k, AA_ERR_ARG, "bad shape s=%ld p=%ld (data p=%ld) ld=%ld ldv=%ld",
               s, p, c->p, ld, ldv);
    AA_CHECK(kernel_spec_check(spec));
    c->cross_s = 0;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(ensure_problem(c, k));
    const long s_pad = round_up(s, 64);
    AA_CHECK(c->crossX.alloc((size_t)s_pad * c->p_pad * sizeof(double)));
    AA_CHECK_HIP(ctx_memset(c, c->crossX.p, 0, c->crossX.bytes));
    AA_CHECK_HIP(ctx_memcpy2d(c, c->crossX.p, (size_t)c->p_pad * sizeof(double), XS, (size_t)ld * sizeof(double),
                              (size_t)p * sizeof(double), (size_t)s, hipMemcpyHostToDevice));
    std::vector<double> v((size_t)s_pad * c->KP, 0.0);
    for (long j = 0; j < s; ++j)
        for (int i = 0; i < k; ++i) v[(size_t)j * c->KP + i] = V[j * ldv + i];
    AA_CHECK(c->crossV.alloc(v.size() * sizeof(double)));
    AA_CHECK_HIP(ctx_memcpy(c, c->crossV.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    c->gpnh_valid = false;
    if (spec.cross_reads_norms()) {
        AA_CHECK(c->crossNorm.alloc((size_t)s_pad * sizeof(double)));
        AA_CHECK(launch_row_norms(c, c->crossX.as<double>(), c->p_pad, p, s_pad, c->crossNorm.as<double>()));
        AA_CHECK(c->rowNorm.alloc((size_t)c->n_pad * sizeof(double)));
        AA_CHECK(launch_row_norms(c, c->X.as<double>(), c->p_pad, p, c->n_pad, c->rowNorm.as<double>()));
    }
    c->cross = spec;
    c->cross_s = s;
    c->cross_s_pad = s_pad;
    c->cross_k = k;
    return AA_OK;
}

// XW = kappa(Y, X_S) V into Gr (and to the host), for the entry point of kernel `kind`
static int kernel_cross_product(aa_ctx *h, int kind, double *XW)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_REQUIRE(has_stored_data(c) && c->cross_s > 0 && c->cross_k == c->k && c->cross.kind == kind, AA_ERR_STATE,
               "aa_set_%s_reference first", KernelSpec{kind}.stem());
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(kernel_cross(c));
    c->gpnh_valid = true;                        // the QP's linear term, as after aa_gpnh_set_factors
    if (XW) AA_CHECK(download_tall(c, c->Gr, XW, c->k, 1, c->n, c->k));
    return AA_OK;
}

int aa_set_rbf_reference(aa_ctx *h, int k, const double *XS, long s, long p, long ld, const double *V, long ldv,
                         double gamma)
{
    return set_kernel_reference(h, KernelSpec{IMPLICIT_RBF, gamma}, k, XS, s, p, ld, V, ldv);
}

int aa_set_poly_reference(aa_ctx *h, int k, const double *XS, long s, long p, long ld, const double *V, long ldv,
                          double gamma, double coef0, int degree)
{
    return set_kernel_reference(h, KernelSpec{IMPLICIT_POLY, gamma, coef0, degree}, k, XS, s, p, ld, V, ldv);
}

int aa_rbf_cross(aa_ctx *h, double *XW) { return kernel_cross_product(h, IMPLICIT_RBF, XW); }

int aa_poly_cross(aa_ctx *h, double *XW) { return kernel_cross_product(h, IMPLICIT_POLY, XW); }

int aa_kernel_transform_cost(aa_ctx *h, const double *A, const double *diag, double *cost)
{
    AA_REQUIRE(h && A && cost, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state && c->gpnh_valid, AA_ERR_STATE, "weights and linear terms first");
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_STATE, "the kernel-form transform cost is single-rank");
    AA_CHECK_HIP(hipSetDevice(c->device));
    const size_t GS = (size_t)c->KP * c->KP;
    const long nb = (c->n + 255) / 256;
    AA_CHECK(c->xformCost.alloc((GS + (size_t)c->n_pad + (size_t)nb + 1) * sizeof(double)));
    double *base = c->xformCost.as<double>();
    std::vector<double> a(GS, 0.0);
    for (int i = 0; i < c->k; ++i)
        for (int j = 0; j < c->k; ++j) a[(size_t)i * c->KP + j] = A[(size_t)i * c->k + j];
    AA_CHECK_HIP(ctx_memcpy(c, base, a.data(), GS * sizeof(double), hipMemcpyHostToDevice));
    if (diag) AA_CHECK_HIP(ctx_memcpy(c, base + GS, diag, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice));
    double s = 0.0;
    AA_CHECK(launch_kernel_transform_cost(c, base, diag ? base + GS : nullptr, base + GS + c->n_pad, &s));
    *cost = 0.5 * s / (double)c->n;
    return AA_OK;
}

int aa_kernel_sample_residuals(aa_ctx *h, const double *A, int diag_kind, const double *diag, double *sample_sse,
                               double *diag_out, double sums[2])
{
    AA_REQUIRE(h && A && sums, AA_ERR_ARG, "null argument");
    AA_REQUIRE(diag_kind >= AA_DIAG_GIVEN && diag_kind <= AA_DIAG_LINEAR, AA_ERR_ARG, "bad diag_kind %d", diag_kind);
    AA_REQUIRE((diag_kind == AA_DIAG_GIVEN) == (diag != nullptr), AA_ERR_ARG,
               "a diagonal vector goes with AA_DIAG_GIVEN, and with nothing else");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state && c->gpnh_valid, AA_ERR_STATE, "weights and linear terms first");
    AA_REQUIRE(c->world == 1 && !c->force_comm, AA_ERR_STATE, "the kernel-form residuals are single-rank");
    const bool from_norms = diag_kind == AA_DIAG_POLY || diag_kind == AA_DIAG_LINEAR;
    AA_REQUIRE(!from_norms || (has_stored_data(c) && c->dtype == AA_F64), AA_ERR_STATE,
               "this diagonal is computed from a stored float64 data matrix");
    AA_REQUIRE(diag_kind != AA_DIAG_POLY || (c->cross_s > 0 && c->cross.kind == IMPLICIT_POLY), AA_ERR_STATE,
               "aa_set_poly_reference first");
    AA_CHECK_HIP(hipSetDevice(c->device));
    const size_t GS = (size_t)c->KP * c->KP;
    const long nb = (c->n + 255) / 256;
    // A | d (given) | r | d (out) | block partials of r, of d | the two sums
    AA_CHECK(c->xformCost.alloc((GS + (size_t)3 * c->n_pad + (size_t)2 * nb + 2) * sizeof(double)));
    double *base = c->xformCost.as<double>();
    double *d_in = base + GS, *r_dev = d_in + c->n_pad, *d_dev = r_dev + c->n_pad, *part = d_dev + c->n_pad;
    std::vector<double> a(GS, 0.0);
    for (int i = 0; i < c->k; ++i)
        for (int j = 0; j < c->k; ++j) a[(size_t)i * c->KP + j] = A[(size_t)i * c->k + j];
    AA_CHECK_HIP(ctx_memcpy(c, base, a.data(), GS * sizeof(double), hipMemcpyHostToDevice));
    if (diag) AA_CHECK_HIP(ctx_memcpy(c, d_in, diag, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice));
    if (from_norms) {
        AA_CHECK(c->rowNorm.alloc((size_t)c->n_pad * sizeof(double)));
        AA_CHECK(launch_row_norms(c, c->X.as<double>(), c->p_pad, c->p, c->n_pad, c->rowNorm.as<double>()));
    }
    AA_CHECK(launch_kernel_sample_residuals(c, base, diag_kind, diag ? d_in : nullptr,
                                            from_norms ? c->rowNorm.as<double>() : nullptr, r_dev, d_dev, part));
    AA_CHECK_HIP(ctx_memcpy(c, sums, part + 2 * nb, 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (sample_sse) AA_CHECK_HIP(ctx_memcpy(c, sample_sse, r_dev, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost));
    if (diag_out) AA_CHECK_HIP(ctx_memcpy(c, diag_out, d_dev, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost));
    return AA_OK;
}

// ------------------------------------------------------------------ stateless ops
int aa_simplex_project_rows(int device, const double *in, double *out, long rows, long cols)
{
    AA_REQUIRE(in && out && rows >= 0 && cols >= 0, AA_ERR_ARG, "bad arguments");
    if (rows == 0 || cols == 0) return AA_OK;
    int n = 0;
    AA_CHECK_HIP(hipGetDeviceCount(&n));
    AA_REQUIRE(n > 0 && device >= 0 && device < n, AA_ERR_HIP, "no usable HIP device");
    AA_CHECK_HIP(hipSetDevice(device));
    ScopedDevBuf a, b;
    const size_t bytes = (size_t)rows * cols * sizeof(double);
    AA_CHECK(a.alloc(bytes));
    AA_CHECK(b.alloc(bytes));
    // (everything of this stateless entry point runs on the null stream, waited for by the host)
    AA_CHECK_HIP(hipMemcpy(a.p, in, bytes, hipMemcpyHostToDevice));
    AA_CHECK(launch_simplex_rows_generic(nullptr, a.as<double>(), b.as<double>(), rows, cols));
    AA_CHECK_HIP(hipDeviceSynchronize());
    AA_CHECK_HIP(hipMemcpy(out, b.p, bytes, hipMemcpyDeviceToHost));
    return AA_OK;
}

// the scratch contexts of the stateless QP entry, one per device (aa_quad_simplex_spg_batch, aa_qp_kernels)
static aa_ctx *g_qp_scratch[64] = {nullptr};
static std::mutex g_qp_scratch_mu;

int aa_quad_simplex_spg_batch(int device, const double *A, const double *B, long stride_j, long stride_t,
                              const double *Z0, double *Zout, long n, int k, const aa_qp_params *params,
                              int *iters)
{
    AA_REQUIRE(A && B && Z0 && Zout && params, AA_ERR_ARG, "null argument");
    AA_REQUIRE(n >= 0 && k >= 1 && k <= AA_MAX_K, AA_ERR_ARG, "bad n=%ld k=%d", n, k);
    AA_REQUIRE(stride_j >= 1 && stride_t >= 1, AA_ERR_ARG, "bad strides");
    if (n == 0) return AA_OK;
    // one scratch context per device for the stateless entry points, kept for the life of the
    // process: creating and destroying a context (two streams, events, allocations) per call
    // cost 8 ms -- more than the QPs of every unit-test-sized problem
    // (ctypes releases the GIL: calls from several threads take turns on the scratch context; it
    // is never destroyed -- HIP may already be gone when static destructors run)
    AA_REQUIRE(device >= 0 && device < 64, AA_ERR_ARG, "device %d out of range", device);
    std::lock_guard<std::mutex> hold(g_qp_scratch_mu);
    if (!g_qp_scratch[device]) AA_CHECK(aa_ctx_create(&g_qp_scratch[device], device, AA_F64));
    aa_ctx *h = g_qp_scratch[device];
    AA_CHECK_HIP(hipSetDevice(device));
    Ctx *c = &h->c;
    c->qp_iters_valid = false;
    ScopedDevBuf dB, dZ, dI;
    const size_t extent = (size_t)((k - 1) * stride_j + (n - 1) * stride_t + 1);
    AA_CHECK(dB.alloc(extent * sizeof(double)));
    AA_CHECK(dZ.alloc((size_t)n * k * sizeof(double)));
    AA_CHECK(dI.alloc((size_t)n * sizeof(int)));
    AA_CHECK_HIP(ctx_memcpy(c, dB.p, B, extent * sizeof(double), hipMemcpyHostToDevice));
    AA_CHECK_HIP(ctx_memcpy(c, dZ.p, Z0, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice));
    AA_CHECK(launch_qp(c, A, dB.as<double>(), stride_j, stride_t, nullptr, dZ.as<double>(), k, n, k, params, dI.as<int>(),
                       (aa_qp_stats *)nullptr));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy(c, Zout, dZ.p, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost));
    if (iters) AA_CHECK_HIP(ctx_memcpy(c, iters, dI.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_get_spg_scalars(aa_ctx *h, double *out)
{
    AA_REQUIRE(h && out, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->scalars.p, AA_ERR_STATE, "no solver state");
    AA_CHECK(join_side(c));
    static_assert(AA_SPG_SCALARS == SC_FMEM0, "include/aa_hip.h documents the ScalarSlot layout");
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy(c, out, c->scalars.p, AA_SPG_SCALARS * sizeof(double), hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_get_spg_array(aa_ctx *h, int which, double *out)
{
    AA_REQUIRE(h && out, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    AA_REQUIRE(c->have_state && c->scalars.p, AA_ERR_STATE, "no solver state");
    const DevBuf *tall[] = {&c->gk, &c->gn, &c->Dt, &c->Gr, &c->Gn, &c->H};
    AA_REQUIRE(which >= 0 && which <= AA_SPG_ARRAY_FMEM, AA_ERR_ARG, "aa_get_spg_array: which = %d out of range", which);
    AA_CHECK_HIP(hipSetDevice(c->device));
    if (which == AA_SPG_ARRAY_FMEM) {
        AA_CHECK_HIP(hipStreamSynchronize(c->stream));
        AA_CHECK_HIP(ctx_memcpy(c, out, c->scalars.as<double>() + SC_FMEM0, 16 * sizeof(double), hipMemcpyDeviceToHost));
        return AA_OK;
    }
    if (which <= AA_SPG_ARRAY_H) {                 // tall [n_pad][KP] -> n x k (download_tall joins the side stream)
        AA_REQUIRE(tall[which]->p, AA_ERR_STATE, "aa_get_spg_array: array %d not allocated", which);
        return download_tall(c, *tall[which], out, c->k, 1, c->n, c->k);
    }
    const bool wide = which == AA_SPG_ARRAY_Q;
    const DevBuf &src = wide ? c->Q : c->Mdev;
    const size_t ld = wide ? (size_t)c->p_pad : (size_t)c->KP, cols = wide ? (size_t)c->p : (size_t)c->k;
    AA_REQUIRE(src.p && (!wide || c->form == AA_FORM_DATA), AA_ERR_STATE,
               "aa_get_spg_array: array %d does not exist in this form", which);
    AA_CHECK_HIP(ctx_memcpy2d(c, out, cols * sizeof(double), src.p, ld * sizeof(double), cols * sizeof(double),
                             (size_t)c->k, hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_spg_path(aa_ctx *h, char *buf, int len)
{
    AA_REQUIRE(h && buf && len > 0, AA_ERR_ARG, "null argument");
    const char *path = h->c.spg_path;
    AA_REQUIRE((size_t)len > strlen(path), AA_ERR_ARG, "aa_spg_path: buffer of %d bytes, %zu needed", len,
               strlen(path) + 1);
    strcpy(buf, path);
    return AA_OK;
}

// ------------------------------------------------------------------ the two passes, on their own
static int invalidate_solver_state(Ctx *c)
{
    c->have_state = false;
    c->grams_valid = false;
    c->products_valid = false;
    c->ckz_valid = false;
    c->gpnh_valid = false;
    c->x_feasible = false;
    c->qp_iters_valid = false;
    return AA_OK;
}

// A' X for a host operand through launch_reduce_rows; flagged: by the path of a mostly-zero operand
static int pass_reduce_rows(aa_ctx *h, int k, const double *A, double *out, long ldo, bool flagged)
{
    AA_REQUIRE(h && A && out, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    // the stored kernel form is served too (not has_stored_data); ensure_problem asks for the data
    AA_REQUIRE(!c->kernel.kind, AA_ERR_STATE, "aa_pass_reduce_rows: no stored matrix behind an implicit kernel");
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(ensure_problem(c, k));
    AA_REQUIRE(ldo >= (c->form == AA_FORM_KERNEL ? c->n : c->p), AA_ERR_ARG, "ldo too small");
    AA_CHECK(invalidate_solver_state(c));
    AA_CHECK(upload_tall(c, c->Dt, A, k, 1, c->n, k));
    AA_CHECK(launch_reduce_rows(c, c->Dt.as<double>(), c->Q.as<double>(), nullptr, false,
                                flagged ? &c->groupFlags : nullptr));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy2d(c, out, (size_t)ldo * sizeof(double), c->Q.p, (size_t)c->p_pad * sizeof(double),
                             (size_t)c->p * sizeof(double), (size_t)k, hipMemcpyDeviceToHost));
    return AA_OK;
}

int aa_pass_reduce_rows(aa_ctx *h, int k, const double *A, double *out, long ldo)
{
    return pass_reduce_rows(h, k, A, out, ldo, false);
}

int aa_pass_reduce_rows_flagged(aa_ctx *h, int k, const double *A, double *out, long ldo)
{
    return pass_reduce_rows(h, k, A, out, ldo, true);
}

int aa_reduce_sparse_counts(aa_ctx *h, long out[2])
{
    AA_REQUIRE(h && out, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    out[0] = out[1] = 0;
    if (!c->slabMode.p) return AA_OK;              // no problem size yet: no flagged call either
    AA_CHECK_HIP(hipSetDevice(c->device));
    unsigned int v[2] = {0u, 0u};
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    AA_CHECK_HIP(ctx_memcpy(c, v, c->slabMode.as<unsigned char>() + AA_SLAB_MODE_BYTES, sizeof(v), hipMemcpyDeviceToHost));
    out[0] = (long)v[0];
    out[1] = (long)v[1];
    return AA_OK;
}

int aa_pass_row_local(aa_ctx *h, int k, const double *B, long ldb, double *out)
{
    AA_REQUIRE(h && B && out, AA_ERR_ARG, "null argument");
    Ctx *c = &h->c;
    // as aa_pass_reduce_rows: either stored form
    AA_REQUIRE(!c->kernel.kind, AA_ERR_STATE, "aa_pass_row_local: no stored matrix behind an implicit kernel");
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK(ensure_problem(c, k));
    AA_REQUIRE(ldb >= c->p, AA_ERR_ARG, "ldb < p");
    AA_CHECK(invalidate_solver_state(c));
    std::vector<double> tmp((size_t)c->KP * c->p_pad, 0.0);
    for (int i = 0; i < k; ++i)
        for (long q = 0; q < c->p; ++q) tmp[(size_t)i * c->p_pad + q] = B[(size_t)i * ldb + q];
    AA_CHECK_HIP(ctx_memcpy(c, c->P.p, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    AA_CHECK(launch_wide_to_T(c, c->P.as<double>(), operandT(c, c->P, c->Pw)));
    AA_CHECK(launch_row_local(c, operandT(c, c->P, c->Pw), c->Gn.as<double>()));
    return download_tall(c, c->Gn, out, k, 1, c->n, k);
}

// ------------------------------------------------------------------ measurement
int aa_pass_kernels(aa_ctx *h, char *buf, int len)
{
    AA_REQUIRE(h && buf, AA_ERR_ARG, "null argument");
    const Ctx *c = &h->c;
    const int need = snprintf(nullptr, 0, "%s;%s", c->pass_names[0], c->pass_names[1]) + 1;
    AA_REQUIRE(len >= need, AA_ERR_ARG, "aa_pass_kernels: buffer of %d bytes, %d needed", len, need);
    snprintf(buf, (size_t)len, "%s;%s", c->pass_names[0], c->pass_names[1]);
    return AA_OK;
}

int aa_qp_kernels(aa_ctx *h, int device, char *buf, int len)
{
    AA_REQUIRE(buf && len > 0, AA_ERR_ARG, "null argument");
    AA_REQUIRE(h || (device >= 0 && device < 64), AA_ERR_ARG, "device %d out of range", device);
    std::lock_guard<std::mutex> hold(g_qp_scratch_mu);
    if (!h) h = g_qp_scratch[device];
    const char *names = h ? h->c.qp_names : "";
    AA_REQUIRE((size_t)len > strlen(names), AA_ERR_ARG, "aa_qp_kernels: buffer of %d bytes, %zu needed", len,
               strlen(names) + 1);
    strcpy(buf, names);
    return AA_OK;
}

int aa_proj_counts(aa_ctx *h, long *out)
{
    AA_REQUIRE(h && out, AA_ERR_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = h->c.projCounts[i];
    return AA_OK;
}

int aa_gemm_timing(aa_ctx *h, int enable, double *ms_reduce_rows, int *n_reduce_rows,
                   double *ms_row_local, int *n_row_local)
{
    AA_REQUIRE(h, AA_ERR_ARG, "null ctx");
    Ctx *c = &h->c;
    AA_CHECK_HIP(hipSetDevice(c->device));
    AA_CHECK_HIP(hipStreamSynchronize(c->stream));
    double *ms_out[2] = {ms_reduce_rows, ms_row_local};
    int *n_out[2] = {n_reduce_rows, n_row_local};
    for (int w = 0; w < 2; ++w) {
        std::vector<hipEvent_t> &ev = c->gemmEvents[w];
        double total = 0.0;
        int n = 0;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) {
                total += ms;
                ++n;
            }
        }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
        if (ms_out[w]) *ms_out[w] = n ? total / n : 0.0;
        if (n_out[w]) *n_out[w] = n;
    }
    c->time_gemm = enable != 0;
    return AA_OK;
}

int aa_time_kernel(aa_ctx *h, int which, int reps, double *ms_avg)
{
    AA_REQUIRE(h && ms_avg && reps >= 1, AA_ERR_ARG, "bad arguments");
    Ctx *c = &h->c;
    if (which == 8)
        AA_REQUIRE(c->kernel.kind && c->have_state, AA_ERR_STATE, "aa_time_kernel 8: an implicit kernel with state");
    else if (which == 9)
        AA_REQUIRE(c->cross_s > 0 && c->cross_k == c->k, AA_ERR_STATE,
                   "aa_time_kernel 9: aa_set_rbf_reference or aa_set_poly_reference first");
    else if (which == 10 || which == 11)
        AA_REQUIRE(has_stored_data(c) && c->have_state && c->gpnh_valid && c->world == 1 && !c->force_comm, AA_ERR_STATE,
                   "aa_time_kernel 10 / 11: aa_gpnh_set_factors (dictionary and weights) first, single rank");
    else if (which == 12)                        // either stored form (not has_stored_data), like aa_pass_reduce_rows
        AA_REQUIRE(c->have_data && !c->kernel.kind && c->Dt.p && c->groupFlags.p, AA_ERR_STATE,
                   "aa_time_kernel 12: a stored matrix and a problem size (aa_set_state or aa_pass_reduce_rows_flagged) first");
    else if (which >= 13 && which <= 23)
        AA_REQUIRE(has_stored_data(c) && c->world == 1 && !c->force_comm, AA_ERR_STATE,
                   "aa_time_kernel 13 .. 23: a stored data matrix (data form), single rank");
    else
        AA_REQUIRE(has_stored_data(c) && c->have_state, AA_ERR_STATE, "aa_time_kernel: needs data-form state on a stored matrix");
    AA_CHECK_HIP(hipSetDevice(c->device));
    hipEvent_t e0, e1;
    AA_CHECK_HIP(hipEventCreate(&e0));
    AA_CHECK_HIP(hipEventCreate(&e1));
    int rc = AA_OK;
    // 13 / 14: a scratch destination of the layout the entry point fills, and a seeded permutation of the rows
    ScopedDevBuf scratch, perm;
    const long scratch_ld = which == 14 ? round_up(c->p, 32) : c->p_pad;
    if (which == 13 || which == 14)
        rc = scratch.alloc((size_t)(c->n_pad + AA_SLACK_ROWS) * scratch_ld * (which == 14 ? sizeof(double) : esize(c)));
    if (which == 13 && rc == AA_OK) {
        std::vector<long> idx((size_t)c->n);
        for (long r = 0; r < c->n; ++r) idx[(size_t)r] = r;
        unsigned long long state = 0x9e3779b97f4a7c15ull;
        for (long r = c->n - 1; r > 0; --r) {            // Fisher-Yates on a 64-bit LCG
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(idx[(size_t)r], idx[(size_t)((state >> 33) % (unsigned long long)(r + 1))]);
        }
        rc = perm.alloc(idx.size() * sizeof(long));
        if (rc == AA_OK && ctx_memcpy(c, perm.p, idx.data(), idx.size() * sizeof(long), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("aa_time_kernel 13: upload of the permutation failed");
            rc = AA_ERR_HIP;
        }
    }
    // 15 / 16: 16 coefficient rows (the values do not matter to the time), 16: rows labelled r mod 12 and a zero
    // centre table; 17: the anomalies form of the model copy (12 x p_pad shift table, trend) into a scratch copy
    ScopedDevBuf coef, labels, tables, partial;
    long nslab = 0;
    (void)moment_slab_rows(c->n, c->p_pad, &nslab);
    if (which >= 15 && which <= 17 && rc == AA_OK) {
        std::vector<int> grp((size_t)c->n);
        for (long r = 0; r < c->n; ++r) grp[(size_t)r] = (int)(r % 12);
        rc = labels.alloc(grp.size() * sizeof(int));
        if (rc == AA_OK) rc = coef.alloc((size_t)c->n * AA_MAX_COEF_ROWS * sizeof(double));      // At, or t in its first n
        if (rc == AA_OK) rc = tables.alloc((size_t)(2 * AA_MAX_COEF_ROWS + 2) * c->p_pad * sizeof(double));
        if (rc == AA_OK && which != 17)
            rc = partial.alloc((size_t)(nslab + 1) * AA_MAX_COEF_ROWS * c->p_pad * sizeof(double));
        if (rc == AA_OK && which == 17) rc = scratch.alloc((size_t)(c->n_pad + AA_SLACK_ROWS) * c->p_pad * esize(c));
        if (rc == AA_OK && ctx_memcpy(c, labels.p, grp.data(), grp.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("aa_time_kernel 15 .. 17: upload of the row labels failed");
            rc = AA_ERR_HIP;
        }
    }
    // 18 / 19: the Gram matrix by rows / by columns as gram_plan cuts it, uncentred; 20: the projection onto
    // AA_TIME_PROJECTED components (a zero V: the values do not matter to the time) into a scratch block
    enum { AA_TIME_PROJECTED = 167 };
    GramPlan gpl = {};
    ScopedDevBuf zshift, gram_partial, gram_out, proj_v;
    const long proj_ld = round_up(AA_TIME_PROJECTED, 128);
    if (which >= 18 && which <= 20 && rc == AA_OK) rc = zshift.alloc((size_t)c->p_pad * sizeof(double));
    if ((which == 18 || which == 19) && rc == AA_OK) {
        int cus = 0;
        rc = device_cus(c, &cus);
        gpl = gram_plan(which == 18 ? GRAM_ROWS : GRAM_COLS, c->n, c->p, (int)esize(c), cus);
        if (rc == AA_OK && gpl.d > GRAM_MAX_D) {
            set_error("aa_time_kernel %d: a %ld x %ld Gram matrix (at most %ld x %ld are formed)", which, gpl.d, gpl.d,
                      GRAM_MAX_D, GRAM_MAX_D);
            rc = AA_ERR_ARG;
        }
        if (rc == AA_OK) rc = gram_partial.alloc((size_t)gpl.partial_bytes);
        if (rc == AA_OK) rc = gram_out.alloc((size_t)gpl.g_ld * gpl.g_ld * sizeof(double));
    }
    if (which == 20 && rc == AA_OK) {
        rc = proj_v.alloc((size_t)project_v_rows(AA_TIME_PROJECTED) * c->p_pad * sizeof(double));
        if (rc == AA_OK) rc = scratch.alloc((size_t)(c->n_pad + AA_SLACK_ROWS) * proj_ld * esize(c));
    }
    // 21 .. 23: the slot-major kernels with the rows labelled r mod 366; 22: a zero centre table; 23: a zero shift
    // table, into a scratch copy
    enum { AA_TIME_SLOTS = 366 };
    ScopedDevBuf slot_meta, slot_tab, slot_partial;
    SlotPlanDev spd = {};
    if (which >= 21 && which <= 23 && rc == AA_OK) {
        if (c->n >= (1L << 31)) {
            set_error("aa_time_kernel %d: %ld rows (fewer than 2^31 are supported)", which, c->n);
            rc = AA_ERR_ARG;
        }
        std::vector<int> lab(rc == AA_OK ? (size_t)c->n : 0);
        for (size_t r = 0; r < lab.size(); ++r) lab[r] = (int)(r % AA_TIME_SLOTS);
        const GroupPlan pl = group_plan(lab.data(), (long)lab.size(), AA_TIME_SLOTS, AA_SLOT_CHUNK_ROWS);
        if (rc == AA_OK) rc = upload_group_plan(c, pl, slot_meta, &spd);
        if (rc == AA_OK) rc = slot_tab.alloc((size_t)AA_TIME_SLOTS * c->p_pad * sizeof(double));
        if (rc == AA_OK && which != 23)
            rc = slot_partial.alloc((size_t)(pl.chunks() + AA_TIME_SLOTS) * c->p_pad * sizeof(double));
        if (rc == AA_OK && which == 23) rc = scratch.alloc((size_t)(c->n_pad + AA_SLACK_ROWS) * c->p_pad * esize(c));
    }
    // one untimed launch first
    for (int phase = 0; phase < 2 && rc == AA_OK; ++phase) {
        const int nrep = phase == 0 ? 1 : reps;
        if (phase == 1) (void)hipEventRecord(e0, c->stream);
        for (int r = 0; r < nrep && rc == AA_OK; ++r) {
            if (which == 0)
                rc = launch_reduce_rows(c, c->Ct.as<double>(), c->Q.as<double>(), nullptr, true);
            else if (which == 1)
                rc = launch_row_local(c, operandT(c, c->P, c->Pw), c->Gn.as<double>());
            else if (which >= 2 && which <= 7)
                rc = launch_stream_probe(c, which - 2);
            else if (which == 8)
                rc = kernel_kv(c, c->Zt.as<double>(), c->H.as<double>());
            else if (which == 9)
                rc = kernel_cross(c);
            else if (which == 10)
                rc = launch_residual_scores(c, nullptr, nullptr, nullptr, false);
            else if (which == 11)
                rc = launch_residual_cost(c, c->Zt.as<double>(), c->P.as<double>(), nullptr, nullptr);
            else if (which == 12)
                rc = launch_reduce_rows(c, c->Dt.as<double>(), c->Q.as<double>(), nullptr, true, &c->groupFlags);
            else if (which == 13)
                rc = launch_gather_rows(c, c->X.p, c->dtype, c->p_pad, perm.as<long>(), scratch.p);
            else if (which == 14)
                rc = launch_features_from_data(c, c->X.p, c->dtype, c->p_pad, c->n, c->p, scratch.as<double>(), scratch_ld);
            else if (which == 15 || which == 16)
                rc = launch_col_weighted_sums(c, AA_MAX_COEF_ROWS, coef.as<double>(), which == 16 ? labels.as<int>() : nullptr,
                                              which == 16 ? tables.as<double>() : nullptr, partial.as<double>(),
                                              partial.as<double>() + (size_t)nslab * AA_MAX_COEF_ROWS * c->p_pad);
            else if (which == 17)
                rc = launch_model_rows(c, c->X.p, 0, labels.as<int>(), tables.as<double>(),
                                       tables.as<double>() + (size_t)2 * AA_MAX_COEF_ROWS * c->p_pad,
                                       tables.as<double>() + (size_t)(2 * AA_MAX_COEF_ROWS + 1) * c->p_pad, coef.as<double>(),
                                       nullptr, scratch.p);
            else if (which == 18 || which == 19)
                rc = launch_gram(c, gpl, zshift.as<double>(), gram_partial.as<double>(), gram_out.as<double>());
            else if (which == 20)
                rc = launch_project_rows(c, c->X.p, c->dtype, c->p_pad, c->p, 0, c->n, AA_TIME_PROJECTED,
                                         proj_v.as<double>(), zshift.as<double>(), scratch.p, proj_ld, c->dtype);
            else if (which == 21 || which == 22)
                rc = launch_slot_sums(c, spd, which == 22 ? slot_tab.as<double>() : nullptr, slot_partial.as<double>(),
                                      slot_partial.as<double>() + (size_t)spd.nchunk * c->p_pad);
            else if (which == 23)
                rc = launch_slot_rows(c, c->X.p, 0, spd, slot_tab.as<double>(), nullptr, scratch.p);
            else {
                set_error("aa_time_kernel: unknown kernel %d", which);
                rc = AA_ERR_ARG;
            }
        }
        if (phase == 1) (void)hipEventRecord(e1, c->stream);
    }
    if (rc == AA_OK) {
        hipError_t e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) {
            set_error("aa_time_kernel: %s", hipGetErrorString(e));
            rc = AA_ERR_HIP;
        }
        *ms_avg = (double)ms / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (which >= 13 && which <= 23) (void)hipStreamSynchronize(c->stream);   // the scratch buffers go
    return rc;
}

}  // extern "C"

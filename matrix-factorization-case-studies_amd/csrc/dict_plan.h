// dict_plan.h -- what dictionary_update (solver.hip) launches, decided apart from launching it: a pure function
// of the knobs and of the facts of the call.  Plain C++17, no HIP and no Ctx: a host compiler builds it alone
// (tests/dict_plan_dump.cpp sweeps it on a CPU over the cross product of the facts).
#pragma once

namespace aa {

// the most evaluations one SPG iteration makes: the start, and 1 + 200 in linesearch_thread0
constexpr int SPG_MAX_FEVAL_PER_ITERATION = 202;

// the g_* values (aa_set_option) at the time of a call
struct DictKnobs { int fuse_finalize, setup_in_grad, grad_side, spg_tail, pack_comm, proj_mode, proj_res_side; };

// data_as_kernel: a data matrix standing in for the kernel K = X X' (aa_set_linear_kernel): launched as the data
// form, scaled as the kernel form.  kernel_matrix: K stored; implicit_kernel: K = kappa(x_i, x_j) of features.
enum class DictForm { data, data_as_kernel, kernel_matrix, implicit_kernel };

// The facts of a call.  slots_mixed: restart slots of which some, not all, were just loaded.  multi: world > 1 or
// a forced communicator.  stats / cost_dst: the caller gave a stats record / a place for the cost after the
// update.  weights_follow: a weights update follows in the same outer iteration; loop_update: the update belongs
// to aa_outer_iterations / aa_iterate (not to the step-by-step entry, whose scalars and arrays are read back);
// loop_judged: a judge reads the SPG flags behind it; max_iter_seen: the host has seen MAX_ITER in the status
// record.  side_resources: the side stream, its scratch set and its fork event exist.  flags_operand: the D'X
// pass leaves the group flags of d behind (reduce_rows_flags_operand).
struct DictPlanIn {
    DictForm form;
    bool slots_aa, slots_mixed, multi;
    bool x_feasible, products_valid, grams_valid, ckz_valid, dict_inputs_overridden;
    bool stats, cost_dst;
    int max_iterations, max_feval;
    bool alpha0_negative;
    bool weights_follow, loop_update, loop_judged, max_iter_seen;
    bool side_resources, flags_operand;
};

// the first entry of aa_spg_path.  cold: factors projected where needed, C X, its Gram and C XX' (C K)
// recomputed; warm: the products of the previous update's refresh reused; fast_*: everything the update needs is
// in the Gram state and one block sets up M, the scalars and f(x) -- k_dict_setup, or block 0 of the gradient launch
enum class DictStart { cold, warm, fast_setup, fast_in_grad };
// fused: (P Q'), (Q Q'), the line search and the Gram of the accepted point in one launch
enum class DictLineSearch { fused, wide_x2, tall_x3 };
// The tail of an SPG iteration (see dict_tail_needed).  skip_*: x += lambda d alone, on the main stream, on the
// row groups the D'X pass flagged in d / on every row; side_whole: g_new, the step, the BB stage and the residual
// projection on the side stream, beside the weights QP; side_proj: the residual projection alone there
enum class DictTail { skip_flagged, skip_dense, main, side_whole, side_proj };

// data / implicit: the launch forms (data or data_as_kernel / implicit_kernel).  project_start: spg.py:148, for
// factors not known to be feasible.  save_restore_P: mixed slots, the warm slots keep the C X they carry;
// warm_slots_setup: ... and start the update through k_dict_setup.  scale_by_n: the gradient is divided by
// n_global (data form, :297), else by k (:288).  alpha_first: no alpha0 given, the first step length comes from
// PROJ_ALPHA (spg.py:178-189).  record_cost: the fused line search writes the cost after the update.
// ride_*, multi-rank (pack_comm): closing sums that ride in the tail of the next all-reduce -- ride_dir: of the
// direction projection, behind Q = D'X; ride_grad: <d, g_new>, with the first reduction of the residual
// projection; ride_res: of the residual projection, behind Z'X / Z'Z of the weights refresh.
// ckct_done: the line search left C K C' of the accepted point in the Gram state (refresh_after_dictionary).
struct DictPlan {
    bool data, implicit;
    DictStart start;
    bool project_start, save_restore_P, warm_slots_setup, scale_by_n, alpha_first;
    DictLineSearch line_search;
    bool record_cost;
    DictTail tail;
    bool ride_dir, ride_grad, ride_res;
    bool stats;
    int max_iterations;
    bool ckct_done;
    bool tail_skipped() const { return tail == DictTail::skip_flagged || tail == DictTail::skip_dense; }
    // the host needs the flags only to decide on a further iteration or to report
    bool read_back(int it) const { return stats || it + 1 < max_iterations; }
};

// launched as the data form (AA_FORM_DATA)
inline bool dict_data_form(DictForm f) { return f == DictForm::data || f == DictForm::data_as_kernel; }

// side stream + second scratch set usable: single rank, candidate-list projection, fused stages
inline bool dict_side_available(const DictKnobs &o, bool side_resources, bool multi)
{
    return o.proj_res_side && side_resources && !multi && o.proj_mode == 0 && o.fuse_finalize;
}

// The tail of an SPG iteration: g_new and <d, g_new>, the BB step (spg.py:232-244), the residual projection with
// ||res|| and the CONVERGED / MAX_FEVAL flags (spg.py:250-276).  A further SPG iteration reads all of it.  With
// one iteration per update the next update forms its gradient from the new H and takes its first step length
// from PROJ_ALPHA, so what is left are the readers outside the update: the caller's stats, the step-by-step
// entries whose scalars and arrays are read back (aa_dictionary_update; updates behind
// aa_set_dictionary_inputs), the collectives that ride with the tail (multi-rank), and the judge of a loop.  The
// judge (iter_judge_thread0) masks CONVERGED out and ORs the rest into the sticky IterState::spg_flags, MAX_ITER
// unless the update converged: once the host has seen MAX_ITER in the status record, a later tail can add
// MAX_FEVAL only -- impossible while max_feval >= SPG_MAX_FEVAL_PER_ITERATION -- and the projection's own
// PROJ_UNCONV, which then reports on a projection nothing needed.  aa_outer_iterations has no judge at all.
inline bool dict_tail_needed(const DictKnobs &o, const DictPlanIn &in)
{
    if (o.spg_tail || in.stats || in.max_iterations > 1) return true;
    if (!dict_data_form(in.form) || in.slots_aa || in.multi) return true;
    if (!in.loop_update || in.dict_inputs_overridden) return true;
    if (in.loop_judged && (in.max_feval < SPG_MAX_FEVAL_PER_ITERATION || !in.max_iter_seen)) return true;
    return false;
}

inline DictPlan dict_plan(const DictKnobs &o, const DictPlanIn &in)
{
    const bool data = dict_data_form(in.form);
    // spg.py:148 projects the start point.  A dictionary that came out of our own update (x_old + lambda d, a
    // convex combination of simplex points) is feasible to rounding, and projecting it would move it by ~1e-17:
    // skipped.  Caller-supplied factors are always projected.  The same holds for its products: CX (P) and
    // C XX' / C K (Gr) computed by the previous update's refresh (archetypal_analysis.py:618-619) are the f /
    // gradient ingredients of this one (spg.py:156,176) -- the weights update in between does not touch the
    // dictionary -- so two passes over X are saved (warm).
    const bool warm = in.x_feasible && in.products_valid;
    // fused small stages (fewer, fatter launches; aa_set_option("fuse_finalize", 0) restores the one-kernel-per-
    // step sequence): with everything the update needs already in the Gram state, one block sets up M, the
    // scalars and f(x) -- for a single fit inside the gradient launch, beside its row blocks
    const bool fused = data && o.fuse_finalize;
    const bool fast = fused && warm && in.grams_valid && in.ckz_valid && !in.dict_inputs_overridden;
    const bool in_grad = fast && o.setup_in_grad && !in.slots_aa;
    // one SPG iteration and nobody to report to: nothing on the main stream waits for the tail before the
    // weights update has run
    const bool single_quiet = in.max_iterations == 1 && !in.stats;
    const bool side = single_quiet && dict_side_available(o, in.side_resources, in.multi);
    const bool pack = in.multi && o.pack_comm && data && !in.slots_aa;

    DictPlan p{};
    p.data = data;
    p.implicit = in.form == DictForm::implicit_kernel;
    p.start = in_grad ? DictStart::fast_in_grad : fast ? DictStart::fast_setup
              : warm ? DictStart::warm : DictStart::cold;
    p.project_start = !fast && !in.x_feasible;
    p.save_restore_P = !fast && !warm && data && in.slots_mixed;
    p.warm_slots_setup = !fast && in.slots_mixed;
    p.scale_by_n = in.form == DictForm::data;
    p.alpha_first = in.alpha0_negative;
    p.line_search = fused ? DictLineSearch::fused : data ? DictLineSearch::wide_x2 : DictLineSearch::tall_x3;
    p.record_cost = fused && in.cost_dst && in.max_iterations == 1;
    p.tail = !data ? DictTail::main
             : !dict_tail_needed(o, in) ? (in.flags_operand ? DictTail::skip_flagged : DictTail::skip_dense)
             : side && o.grad_side ? DictTail::side_whole : side ? DictTail::side_proj : DictTail::main;
    p.ride_dir = pack;
    p.ride_grad = pack && o.proj_mode == 0 && o.fuse_finalize;
    p.ride_res = pack && in.weights_follow && single_quiet && o.fuse_finalize;
    p.stats = in.stats;
    p.max_iterations = in.max_iterations;
    p.ckct_done = fused;
    return p;
}

}  // namespace aa

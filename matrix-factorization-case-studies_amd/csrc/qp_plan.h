// qp_plan.h -- what launch_qp launches, decided apart from launching it: a pure function of the
// knobs and of a few facts about the call.  Plain C++17, no HIP and no Ctx: a host compiler builds
// it alone (tests/qp_plan_dump.cpp sweeps it on a CPU at every edge of the dispatch).
#pragma once

namespace aa {

constexpr int QP_MAXMEM = 8;          // f_mem entries the lane / quad kernels keep in registers (spg.py:310)
constexpr int QW_MAXMEM = 32;         // ... and the wave-per-sample kernel, which takes over for memory > 8
constexpr int QR_MAXMEM = 16;         // ... and the row kernel
// Launch shapes; the measurements behind the values are in DESIGN.md sections 8.2 and 9.
constexpr int QP_WAVES = 1024;        // most waves of the lane-per-sample kernel: one per SIMD
constexpr int QP_QUAD_WAVES = 8192;   // most waves of k_qp_quad_w3: up to 131 072 samples every wave takes ONE batch of 16
                                      // and the hardware hands the batches (longest first) to SIMDs as they free up
constexpr int QP_ROW_WAVES = 2048;    // most waves of the row kernel (k_qp_row): 2 per SIMD, all resident
constexpr int QP_WAVE_BLOCKS = 1024;  // blocks (4 waves each) of the wave-per-sample kernel when it finishes parked samples
constexpr int QP_TAIL_CAP = 96;       // qp_overlap_tail: only samples beyond this many passes go to the side stream
constexpr int QP_SORT_ROWS_PER_BLOCK = 1024;   // samples an ordering block takes
constexpr int QP_ORDER_MAX_BLOCKS = 256;       // most ordering blocks in front of k_qp_wave_ord

// the g_qp_* values (aa_set_option) at the time of a call
struct QpKnobs { int mode, pass_cap, quad_cap, live, quad_lazy, fused_order, wave_lazy, overlap_tail, sort; };

// host_hessian: A_host given (else k_qp_setup builds D G D on the device).  own_iters: iters_dev is the context's
// own pass-count list, iters_valid: which holds the counts of the previous update.  perm_ready: that update left a
// permutation of this n (k_qp_wave_ord).  defer_possible: the caller asked for a deferred tail and there are no
// statistics to read, a side stream, ldz == KP, float32 data and room in tmpTall.  live_stream: a stream for the
// live consumers exists and no deferred tail was asked for.
struct QpPlanIn {
    long n;
    int k, memory, max_iterations;
    bool host_hessian, own_iters, iters_valid, perm_ready, defer_possible, live_stream;
};

enum class QpMap { project_only, row, quad, wave_only, lane };
// sort_now: qp_order_rows in front of the first phase; prefetched: the previous update's k_qp_wave_ord left it;
// forms_next: this update runs unordered and its k_qp_wave_ord forms the next one (as a prefetched one does)
enum class QpSampleOrder { none, sort_now, prefetched, forms_next };
// main: k_qp_wave on the main stream; deferred: on the side stream, results by slot; two_stage: up to
// park_at passes on the main stream, the rest deferred; live: consumers beside k_qp_quad, then a clean-up
enum class QpTail { none, main, deferred, two_stage, live };

// KQ / KW: A padded for the lane kernel / for the wave, row and quad kernels.  sel: MT of k_qp_quad_w3, CPL of
// k_qp_row; mem1: MEM1 (memory <= 1); full: FULL (k == KQ); quad_lazy: LAZYQ.  cap, grid, max_trips: passes and
// blocks of the first phase and the four-lane kernel's watchdog.  sort_hist: the set-up kernel zeroes the ordering
// area; setup_order: its last argument, -1, 0 or order_blocks.  tail_ord: the continuation is k_qp_wave_ord, with
// order_blocks blocks in front; park_at: where a two-stage tail parks (else never).
struct QpPlan {
    QpMap mapping;
    int KQ, KW, sel, cap, setup_order, order_blocks, park_at;
    bool mem1, full, quad_lazy, sort_hist, tail_ord;
    long grid, max_trips;
    QpSampleOrder order;
    QpTail tail;
};

inline int qp_pad_k(int k) { int KQ = 4; while (KQ < k) KQ *= 2; return KQ; }

// passes of the first phase: everything when nothing would be left over, and with memory > 1 (the
// continuation kernels are the memory-1 instantiation)
inline int qp_cap(int cap, int memory, int maxit) { return (memory > 1 || maxit <= cap) ? maxit : cap; }

// the four-lane kernel's: 32 from 65 536 samples per GPU (100 000: 1.985 against 2.010 ms per outer
// iteration), 24 below (12 500: 0.572 against 0.582)
inline int qp_quad_cap(int knob, long n, int memory, int maxit)
{
    return qp_cap(knob > 0 ? knob : (n >= 65536 ? 32 : 24), memory, maxit);
}

// blocks for n samples at `per` each, `most` at the most (the kernels stride over the rest)
inline long qp_grid(long n, long per, long most) { return (n + per - 1) / per < most ? (n + per - 1) / per : most; }

// watchdog only: a wave's slots take their samples one after the other, each at most cap passes
// and a start-up trip
struct QpQuadShape { long waves, max_trips; };
inline QpQuadShape qp_quad_shape(long n, int cap)
{
    const long waves = qp_grid(n, 16, QP_QUAD_WAVES), rounds = (n + 16 * waves - 1) / (16 * waves);
    return {waves, 16 * rounds * ((long)cap + 2) + 16};
}

// default (qp_mode 0), k <= 32: four lanes per sample in the matrix-core operand layout
// (k_qp_quad) followed by the wave-per-sample kernel for the samples that reach its pass cap --
// ahead of the other mappings at every size measured (1 600 .. 100 000 samples per GPU:
// 0.63 ms per outer iteration at 12 500 rows against 0.69 for the row kernel and 0.81 for
// lane + wave; 1.99 against 2.21 ms at 100 000) -- except when every sample gets the same
// one or two passes (GPNH's weights QP with max_iterations = 1): nothing diverges then and
// the lane-per-sample kernel, 64 samples per wave, is cheaper (0.175 against 0.188 ms on the
// C3 stand-in).  k > 32: one wave per sample.
// spg.py:310 allocates f_mem of any length; the kernels keep it in registers: 8 entries in the
// throughput kernels, 16 in the row kernel, 32 in the wave-per-sample kernel, which therefore
// takes the whole update when memory > 8 (a setting the reference's callers never use)
inline QpPlan qp_plan(const QpKnobs &o, const QpPlanIn &in)
{
    const int maxit = in.max_iterations, KQ = qp_pad_k(in.k), KW = KQ > 32 ? 64 : 32;
    const bool mem1 = in.memory <= 1, big_mem = in.memory > QP_MAXMEM;
    const bool row = KQ <= 32 && o.mode == 3 && in.memory <= QR_MAXMEM;
    const bool quad = !big_mem && KQ <= 32 && (o.mode == 4 || (o.mode == 0 && maxit > 4));
    const bool wave_only = !row && !quad && (big_mem || KQ > 32 || o.mode == 1 || o.mode == 3);
    const QpMap m = maxit <= 0 ? QpMap::project_only : row ? QpMap::row : quad ? QpMap::quad
                    : wave_only ? QpMap::wave_only : QpMap::lane;
    // samples in the order of their pass counts in the previous update of this context; pointless
    // when everybody gets the same one or two passes, for the kernel that takes a wave per sample
    // anyway and for a few thousand samples (measured: 1610 and 3000 rows 2 % faster unordered,
    // 12 500 rows 3 % slower)
    const bool will_sort = o.sort && maxit > 2 && in.n > 4096 && !wave_only && in.own_iters && in.iters_valid;
    // (deferred stragglers of the four-lane kernel: only the two-stage form, whose first stage is an
    // ordinary launch on the main stream.  The knob is asked here too: launch_qp's one caller that
    // passes defer_tail passes it by this knob, see aa_internal.h)
    const bool defer_ok = o.overlap_tail && in.defer_possible && KW == 32;
    const int quad_cap = qp_quad_cap(o.quad_cap, in.n, in.memory, maxit);
    const bool two_stage = defer_ok && QP_TAIL_CAP > quad_cap && QP_TAIL_CAP < maxit;
    // four-lane kernel: the order is formed by extra blocks of the PREVIOUS update's continuation launch
    // (k_qp_wave_ord) and this update's launch forms the next one; an update without a predecessor runs
    // unordered
    const bool fused = o.fused_order && o.sort && quad && !in.host_hessian && KW == 32 && mem1 && !o.live &&
                       (!defer_ok || two_stage) && quad_cap < maxit && maxit > 2 && in.n > 4096 &&
                       in.n <= (long)QP_ORDER_MAX_BLOCKS * QP_SORT_ROWS_PER_BLOCK && in.own_iters;
    const bool live = o.live && quad_cap < maxit && in.live_stream && KW == 32;
    const QpQuadShape shape = qp_quad_shape(in.n, quad_cap);
    const int cap = m == QpMap::quad ? quad_cap
                    : m == QpMap::lane ? qp_cap(o.pass_cap < 1 ? 1 : o.pass_cap, in.memory, maxit) : 0;
    // (lane kernel, one wave per SIMD: lanes that finish early pull further samples, so a wave's
    // trip count is the sum over ~n/65536 samples per lane instead of two full rounds)
    const long grid = m == QpMap::project_only ? (in.n + 255) / 256 : m == QpMap::row ? qp_grid(in.n, 4, QP_ROW_WAVES)
                      : m == QpMap::quad ? shape.waves : m == QpMap::lane ? qp_grid(in.n, 64, QP_WAVES)
                      : qp_grid(in.n, 4, 2048);
    const int order_blocks = (int)((in.n + QP_SORT_ROWS_PER_BLOCK - 1) / QP_SORT_ROWS_PER_BLOCK);
    const QpSampleOrder order = fused ? (in.perm_ready ? QpSampleOrder::prefetched : QpSampleOrder::forms_next)
                                      : will_sort ? QpSampleOrder::sort_now : QpSampleOrder::none;
    // a continuation follows a first phase that stops at a cap (the row kernel runs every sample to completion)
    const QpTail parked = defer_ok ? QpTail::deferred : QpTail::main;
    const QpTail tail = cap >= maxit ? QpTail::none : m == QpMap::lane ? parked
                        : m != QpMap::quad ? QpTail::none : live ? QpTail::live : two_stage ? QpTail::two_stage : parked;
    return QpPlan{m, KQ, KW, /*sel*/ in.k <= 16 ? 1 : 2, cap, /*setup_order*/ fused ? (in.perm_ready ? order_blocks : 0) : -1,
                  order_blocks, /*park_at*/ tail == QpTail::two_stage ? QP_TAIL_CAP : 1 << 30,
                  mem1, /*full*/ in.k == KQ, /*quad_lazy*/ m == QpMap::quad && o.quad_lazy && !live,
                  /*sort_hist*/ !in.host_hessian && (will_sort || fused), /*tail_ord*/ fused,
                  grid, /*max_trips*/ m == QpMap::quad ? shape.max_trips : 0, order, tail};
}

}  // namespace aa

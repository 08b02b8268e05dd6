// pass_plan.h -- what the two X-pass launchers of kernels_gemm.hip launch (reduce-over-rows A'X, row-local X B'),
// and the slab decomposition ensure_problem (solver.hip) gives the first, decided apart from launching: pure
// functions of the knobs and of the shapes.  Plain C++17, no HIP and no Ctx: a host compiler builds it alone
// (tests/pass_plan_dump.cpp sweeps it on a CPU at every edge of the dispatch).
#pragma once
#include <cstddef>
#include <cstdio>

namespace aa {

constexpr int ROW_LOCAL_RING = 8;          // X pieces in a wave's ring of k_row_local_f32_dma: two tiles, one of them in flight
constexpr long PASS_LDS_LIMIT = 160 * 1024;   // dynamic LDS a block may ask for once the limit is raised (a CU's LDS)

// the g_* values (aa_set_option) at the time of a call
struct PassKnobs { int row_local_variant, row_local_acc64, row_local_split, f64_mfma, reduce_sparse, reduce_sparse_max; };

inline long pass_ceil_div(long a, long b) { return (a + b - 1) / b; }
inline long pass_round_up(long a, long b) { return pass_ceil_div(a, b) * b; }

// ------------------------------------------------------------------ reduce-over-rows: slabs
// columns a block of the reduce-over-rows kernels owns
inline long reduce_rows_block_cols(bool f32) { return f32 ? 512 : 256; }
constexpr long REDUCE_ROWS_BLOCKS = 512;       // target block count, 2 per CU: 64 slabs at p = 4096
constexpr long REDUCE_ROWS_MAX_SLABS = 256;    // (a mode byte per slab: AA_SLAB_MODE_BYTES)

// split-row decomposition of the reduce-over-rows GEMM: slabs of whole 32-row tiles
struct PassSlabs { long colgroups, nslab, rows_per_slab; };
inline PassSlabs pass_slabs(bool f32, long n_pad, long p_pad)
{
    PassSlabs s{};
    s.colgroups = pass_ceil_div(p_pad, reduce_rows_block_cols(f32));
    long nslab = pass_ceil_div(REDUCE_ROWS_BLOCKS, s.colgroups);
    if (nslab > REDUCE_ROWS_MAX_SLABS) nslab = REDUCE_ROWS_MAX_SLABS;
    if (nslab < 1) nslab = 1;
    s.rows_per_slab = pass_round_up(pass_ceil_div(n_pad, nslab), 32);
    s.nslab = pass_ceil_div(n_pad, s.rows_per_slab);
    return s;
}

// ------------------------------------------------------------------ reduce-over-rows: the launch
enum class ReduceRowsFamily { f32, f64_mfma, f64_valu };

// flag_buf: the caller gave a flag buffer (it expects a mostly-zero operand); time_gemm: aa_gemm_timing is on
struct ReduceRowsIn {
    bool f32;
    int KP;
    long p_pad, nslab, rows_per_slab;
    bool flag_buf, time_gemm;
};

// targ: the family's template argument -- NCT (f32), NT (f64 matrix cores), KP (f64 VALU).  flagged: group flags of
// the operand -> gather kernel -> gated dense kernel, in place of the dense kernel alone.  gather_limit: flagged
// groups of 4 rows per slab up to which the gather kernel takes the slab.
struct ReduceRowsPlan {
    ReduceRowsFamily family;
    int targ;
    bool flagged;
    long grid_x, grid_y;
    long gather_limit;
};

// A call with a flag buffer takes the flagged sequence, and so leaves the group flags of its operand in that buffer.
// The float64 VALU kernel (f64_mfma = 0) has no gather twin: it stays dense.  So does every call while
// aa_gemm_timing is on: its event pairs time full passes (bench.py's roofline, two per outer iteration), and the
// dense pass gives the same bits.
inline bool reduce_rows_takes_flags(const PassKnobs &o, bool f32, bool time_gemm)
{
    return o.reduce_sparse && !time_gemm && (f32 || o.f64_mfma);
}

// default reduce_sparse_max: a quarter (float32) / half (float64) of a slab's groups, the largest swept fraction at
// which the flagged sequence beat the dense pass at the headline shape (profiles/reduce_sparse_ab.txt, section 5)
inline long reduce_sparse_default_den(bool f32) { return f32 ? 4 : 2; }

inline ReduceRowsPlan reduce_rows_plan(const PassKnobs &o, const ReduceRowsIn &in)
{
    ReduceRowsPlan p{};
    p.family = in.f32 ? ReduceRowsFamily::f32 : o.f64_mfma ? ReduceRowsFamily::f64_mfma : ReduceRowsFamily::f64_valu;
    p.targ = in.f32 ? in.KP / 32 : o.f64_mfma ? in.KP / 16 : in.KP;
    p.flagged = in.flag_buf && reduce_rows_takes_flags(o, in.f32, in.time_gemm);
    p.grid_x = pass_ceil_div(in.p_pad, reduce_rows_block_cols(in.f32));
    p.grid_y = in.nslab;
    const long gps = in.rows_per_slab / 4;                   // groups per (full) slab
    p.gather_limit = o.reduce_sparse_max < 0 ? gps / reduce_sparse_default_den(in.f32) : (long)o.reduce_sparse_max;
    if (p.gather_limit > gps) p.gather_limit = gps;
    return p;
}

// ------------------------------------------------------------------ row-local: the launch
// float32 -- global: operands straight from global memory (variant 0); lds: X staged in wave-private LDS (1);
// blk: block-tiled, B shared through LDS (2..7); ws: wave-streaming, wave-private X tiles and B slabs shared per
// block (8); dma: the same with LDS-DMA staging and float64 sums of 32-column pieces, k <= 32 (9).
// float64 -- ws: wave-streaming on the f64 matrix cores; mfma: block-tiled on them; valu.
enum class RowLocalFamily { f32_global, f32_lds, f32_blk, f32_ws, f32_dma, f64_ws, f64_mfma, f64_valu };
constexpr int ROW_LOCAL_FAMILIES = 8;

// The per-family constants.  Column split of the block-tiled kernels when there are few row blocks (short shards):
// with fewer than `below` row blocks of `rows` rows, about `target` blocks in all (three per CU), in chunks of at
// least `min_chunk` columns, a multiple of `granule` (every tile width of the family).
struct RowLocalSplit { long rows, below, target, min_chunk, granule; };
constexpr RowLocalSplit ROW_LOCAL_SPLIT_F32_BLK = {128, 384, 768, 512, 128};
constexpr RowLocalSplit ROW_LOCAL_SPLIT_F64_MFMA = {64, 192, 512, 256, 32};
// Most waves per block of the wave-streaming kernels, [KP == 64]: what 160 KB of LDS hold, and with float64 sums in
// the register-staged float32 kernel 3 (2) waves per SIMD.
constexpr int ROW_LOCAL_MIN_WAVES = 8;                             // the B slab loaders assume >= 512 threads
constexpr int ROW_LOCAL_WMAX_F32_DMA = 16;
constexpr int ROW_LOCAL_WMAX_F32_WS[2][2] = {{16, 12}, {12, 8}};   // [acc64][KP == 64]
constexpr int ROW_LOCAL_WMAX_F64_WS[2] = {14, 10};
// block-tiled float32 kernel at KP = 32, variants 2..7: tile width, double-buffered.  Every other variant that
// lands there takes variant 2's; KP = 64 has the 64-column tile alone and keeps the buffering.
struct RowLocalTile { int width; bool dbuf; };
constexpr RowLocalTile ROW_LOCAL_BLK_TILES[6] = {{64, false}, {64, true}, {128, false}, {32, true}, {128, true}, {32, false}};
// rows a thread of k_row_local_f32<NCT, RT> takes
constexpr int row_local_global_rt(int nct) { return nct == 1 ? 2 : 1; }
// shards from this many 32-row tiles on take the wave-streaming kernels by default (32 768 rows per GPU)
constexpr long ROW_LOCAL_STREAM_TILES = 8 * 128;

// targ: the family's first template argument -- NCT = KP / 32 (float32), NT = KP / 16 (f64 matrix cores), KP (f64
// VALU).  tile / dbuf: block-tiled float32 kernel.  acc64: float64 sums of 32-column pieces (blk, ws; dma has no other form).  variant: the
// resolved row_local_variant, float32 only (-1 for float64).  W: waves per block of the streaming kernels, else 0.
// lds: dynamic LDS bytes; raise_lds: the family needs PASS_LDS_LIMIT set on its kernels.  nsplit / chunk: column
// chunks of the contraction (1 / p_pad when unsplit); partial_bytes: of rlPartial, 0 when unsplit.
struct RowLocalPlan {
    RowLocalFamily family;
    int targ, tile;
    bool dbuf, acc64;
    int variant;
    int W;
    long grid_x, grid_y;
    int block;
    size_t lds;
    bool raise_lds;
    int nsplit, chunk;
    size_t partial_bytes;
};

// W waves per block: one block per CU (256) where possible
inline int row_local_waves(long tiles, int wmax)
{
    long W = pass_ceil_div(tiles, 256);
    if (W < ROW_LOCAL_MIN_WAVES) W = ROW_LOCAL_MIN_WAVES;
    if (W > wmax) W = wmax;
    return (int)W;
}

// the streaming families: W waves, one 32-row tile per wave, `lds` bytes
inline void row_local_streaming(RowLocalPlan &p, long n_pad, int wmax, size_t shared_elems, size_t wave_elems,
                                size_t elem_size)
{
    const long tiles = n_pad / 32;
    p.W = row_local_waves(tiles, wmax);
    p.grid_x = pass_ceil_div(tiles, p.W);
    p.block = 64 * p.W;
    p.lds = (shared_elems + (size_t)p.W * wave_elems) * elem_size;
    p.raise_lds = true;
}

// the block-tiled families: one block per rule.rows rows and column chunk
inline void row_local_split(RowLocalPlan &p, const RowLocalSplit &rule, bool split, long n_pad, long p_pad, int KP)
{
    const long rblocks = n_pad / rule.rows;
    long nsplit = 1;
    if (rblocks < rule.below && split) {
        nsplit = pass_ceil_div(rule.target, rblocks);
        if (nsplit > p_pad / rule.min_chunk) nsplit = p_pad / rule.min_chunk;
        if (nsplit < 1) nsplit = 1;
    }
    if (nsplit > 1) {
        p.chunk = (int)pass_round_up(pass_ceil_div(p_pad, nsplit), rule.granule);
        nsplit = pass_ceil_div(p_pad, p.chunk);
    }
    p.nsplit = (int)nsplit;
    p.grid_x = rblocks;
    p.grid_y = nsplit;
    p.partial_bytes = nsplit > 1 ? (size_t)nsplit * n_pad * KP * sizeof(double) : 0;
}

// row_local_variant = -1 is by size: large shards stream; k <= 32 with float64 sums of 32-column pieces through the
// LDS-DMA kernel (1 % slower than the register-staged kernel with one fp32 chain per row, 86 x closer to the exact
// product: rms error 3.5e-9 against 3.1e-7 of sum |x||b| at p = 4096)
inline int row_local_variant(const PassKnobs &o, int KP, long n_pad)
{
    if (o.row_local_variant >= 0) return o.row_local_variant;
    if (n_pad / 32 < ROW_LOCAL_STREAM_TILES) return 4;
    return (KP == 32 && o.row_local_acc64 >= 1) ? 9 : 8;
}

inline RowLocalPlan row_local_plan(const PassKnobs &o, bool f32, int KP, long n_pad, long p_pad)
{
    RowLocalPlan p{};
    p.variant = -1;
    p.grid_y = 1;
    p.block = 256;
    p.nsplit = 1;
    p.chunk = (int)p_pad;
    const bool kp64 = KP == 64;
    if (f32) {
        const int v = p.variant = row_local_variant(o, KP, n_pad);
        p.targ = KP / 32;
        if (v == 9 && !kp64) {
            p.family = RowLocalFamily::f32_dma;
            p.acc64 = true;
            row_local_streaming(p, n_pad, ROW_LOCAL_WMAX_F32_DMA, 2 * 32 * 64, ROW_LOCAL_RING * 256, sizeof(float));
        } else if (v == 8) {
            p.family = RowLocalFamily::f32_ws;
            p.acc64 = o.row_local_acc64 >= 2;
            row_local_streaming(p, n_pad, ROW_LOCAL_WMAX_F32_WS[p.acc64][kp64], (size_t)2 * KP * 128, 32 * 64,
                                sizeof(float));
        } else if (v >= 2) {                       // (a forced 9 at KP = 64 too: it has no kernel of its own there)
            p.family = RowLocalFamily::f32_blk;
            const RowLocalTile t = v <= 7 ? ROW_LOCAL_BLK_TILES[v - 2] : ROW_LOCAL_BLK_TILES[0];
            p.tile = kp64 ? 64 : t.width;
            p.dbuf = t.dbuf;
            p.acc64 = o.row_local_acc64 != 0;      // (2 is the same instantiation as 1)
            row_local_split(p, ROW_LOCAL_SPLIT_F32_BLK, o.row_local_split != 0, n_pad, p_pad, KP);
        } else if (v == 1) {
            p.family = RowLocalFamily::f32_lds;
            p.grid_x = n_pad / 128;
        } else {
            p.family = RowLocalFamily::f32_global;
            p.grid_x = pass_ceil_div(n_pad, 128 * row_local_global_rt(p.targ));
        }
    } else if (o.f64_mfma == 2 || (o.f64_mfma == 1 && n_pad / 32 >= ROW_LOCAL_STREAM_TILES)) {
        p.family = RowLocalFamily::f64_ws;
        p.targ = KP / 16;
        row_local_streaming(p, n_pad, ROW_LOCAL_WMAX_F64_WS[kp64], (size_t)2 * KP * 66, 32 * 34, sizeof(double));
    } else if (o.f64_mfma) {
        p.family = RowLocalFamily::f64_mfma;
        p.targ = KP / 16;
        row_local_split(p, ROW_LOCAL_SPLIT_F64_MFMA, o.row_local_split != 0, n_pad, p_pad, KP);
    } else {
        p.family = RowLocalFamily::f64_valu;
        p.targ = KP;
        p.grid_x = n_pad / 64;
    }
    return p;
}

// ------------------------------------------------------------------ the names aa_pass_kernels reports
// Every format that names a pass kernel is here and nowhere else (tests/test_gpu_pass_kernels.py reads them).
#define PASS_NAME(WHICH, ...) return std::snprintf(buf, len, __VA_ARGS__)
inline int pass_name(const ReduceRowsPlan &p, char *buf, size_t len)
{
    switch (p.family) {
        case ReduceRowsFamily::f32: PASS_NAME(0, "k_reduce_rows_f32<%d,4>", p.targ);
        case ReduceRowsFamily::f64_mfma: PASS_NAME(0, "k_reduce_rows_f64_mfma<%d>", p.targ);
        case ReduceRowsFamily::f64_valu: PASS_NAME(0, "k_reduce_rows_f64<%d>", p.targ);
    }
    return -1;
}

inline int pass_name(const RowLocalPlan &p, char *buf, size_t len)
{
    switch (p.family) {
        case RowLocalFamily::f32_global: PASS_NAME(1, "k_row_local_f32<%d>", p.targ);
        case RowLocalFamily::f32_lds: PASS_NAME(1, "k_row_local_f32_lds<%d>", p.targ);
        case RowLocalFamily::f32_blk:
            PASS_NAME(1, "k_row_local_f32_blk[v%d,acc64=%d,split=%d]", p.variant, (int)p.acc64, p.nsplit);
        case RowLocalFamily::f32_ws: PASS_NAME(1, "k_row_local_f32_ws<%d,%d>", p.targ, (int)p.acc64);
        case RowLocalFamily::f32_dma: PASS_NAME(1, "k_row_local_f32_dma<%d>", ROW_LOCAL_RING);
        case RowLocalFamily::f64_ws: PASS_NAME(1, "k_row_local_f64_ws<%d>", p.targ);
        case RowLocalFamily::f64_mfma: PASS_NAME(1, "k_row_local_f64_mfma<%d>[split=%d]", p.targ, p.nsplit);
        case RowLocalFamily::f64_valu: PASS_NAME(1, "k_row_local_f64<%d>", p.targ);
    }
    return -1;
}
#undef PASS_NAME

}  // namespace aa

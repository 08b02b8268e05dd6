// gram_plan.h -- how aa_data_gram cuts its work, decided apart from launching it: a pure function of the side,
// the shape, the element size and the number of compute units.  Plain C++17 and no Ctx (the one HIP word,
// the host / device mark of gram_pair_tile, is there only under hipcc): a host compiler builds it alone
// (tests/gram_plan_dump.cpp sweeps it on a CPU at the tile, chunk and pad edges).
//
// The Gram matrix G (d x d; d = n by rows, p by columns) is formed in 64 x 64 tiles, the tile pairs (ti, tj) with
// tj >= ti only: gram_pairs(tiles) blocks along grid.x, in the order gram_pair_tile names.  The contraction (over
// the p features by rows, over the n rows by columns) is cut into `nsplit` runs of `split_len` indices along
// grid.y, split_len a multiple of the kernel's K chunk; split s takes [s split_len, min((s + 1) split_len, K)).
// With one split the kernel writes G itself; with more, every block leaves its tile in
// partial[split][pair][64 x 64] and a finish kernel adds the splits in ascending order (no atomics).
#pragma once

namespace aa {

enum { GRAM_ROWS = 0, GRAM_COLS = 1 };          // AA_GRAM_ROWS / AA_GRAM_COLS (include/aa_hip.h)

constexpr long GRAM_TILE = 64;                  // rows and columns of an output tile
constexpr long GRAM_CHUNK = 32;                 // contraction indices a block stages through LDS at a time (both sides)
constexpr long GRAM_MAX_D = 8192;               // largest d: the d x d result goes through one host eigen-solve
constexpr long GRAM_PARTIAL_BUDGET = 64L << 20; // most bytes of partial tiles
constexpr long GRAM_BLOCKS_PER_CU = 2;          // blocks aimed at when the tile pairs alone do not fill the device

struct GramPlan {
    int side;
    long d;                 // order of G
    long tiles;             // 64-wide tiles along one side: ceil(d / 64)
    long pairs;             // tile pairs with tj >= ti: grid.x
    long K;                 // contraction length: p by rows, n by columns
    long nsplit;            // grid.y
    long split_len;         // contraction indices per split, a multiple of GRAM_CHUNK
    long partial_bytes;     // nsplit pairs 64 x 64 doubles, 0 with one split
    long g_ld;              // leading dimension of the device result: 64 tiles (whole tiles are written)
};

inline long gram_pairs(long tiles) { return tiles * (tiles + 1) / 2; }

// pair index -> (ti, tj), tj >= ti: row ti of the upper triangle holds tiles - ti pairs, rows in ascending order.
// The one function the host sweep tests and the kernels call.
#ifdef __HIPCC__
#define GRAM_HOST_DEVICE __host__ __device__
#else
#define GRAM_HOST_DEVICE
#endif
GRAM_HOST_DEVICE inline void gram_pair_tile(long idx, long tiles, long *ti, long *tj)
{
    long i = 0;
    while (idx >= tiles - i) {
        idx -= tiles - i;
        ++i;
    }
    *ti = i;
    *tj = i + idx;
}

// From `cus` tile pairs on, every compute unit has a tile of its own: one split, no partials (1610 x 25 000 by
// rows: 351 pairs; 100 000 x 4096 by columns: 2080).  Below, the contraction is split until about
// GRAM_BLOCKS_PER_CU blocks per compute unit run (89 120 x 167 by columns: 6 pairs over 89 120 rows; 64 x 25 000
// by rows: one pair), never finer than one chunk per split and never beyond the byte budget of the partials.
// elem_size does not enter today (both element types are widened into the same float64 LDS tiles); it is part of
// the signature because the chunk may come to depend on it.
inline GramPlan gram_plan(int side, long n, long p, int elem_size, int cus)
{
    (void)elem_size;
    GramPlan g;
    g.side = side;
    g.d = side == GRAM_ROWS ? n : p;
    g.K = side == GRAM_ROWS ? p : n;
    g.tiles = (g.d + GRAM_TILE - 1) / GRAM_TILE;
    g.pairs = gram_pairs(g.tiles);
    g.g_ld = g.tiles * GRAM_TILE;
    const long chunks = (g.K + GRAM_CHUNK - 1) / GRAM_CHUNK;
    if (cus < 1) cus = 1;
    long want = 1;
    if (g.pairs < cus) {
        want = (GRAM_BLOCKS_PER_CU * cus + g.pairs - 1) / g.pairs;
        const long fit = GRAM_PARTIAL_BUDGET / (g.pairs * GRAM_TILE * GRAM_TILE * 8);
        if (want > fit) want = fit;
        if (want > chunks) want = chunks;
        if (want < 1) want = 1;
    }
    const long chunks_per_split = (chunks + want - 1) / want;
    g.split_len = chunks_per_split * GRAM_CHUNK;
    g.nsplit = (chunks + chunks_per_split - 1) / chunks_per_split;    // <= want: the last split may be short
    g.partial_bytes = g.nsplit > 1 ? g.nsplit * g.pairs * GRAM_TILE * GRAM_TILE * 8 : 0;
    return g;
}

}  // namespace aa

// kernels_pca.hip -- PCA of resident data (gfx950): the Gram matrix of the centred data matrix with itself, by
// rows or by columns, and the row-local projection onto up to 256 directions that installs its result as a new
// block (aa_data_gram, aa_set_data_projected).  Every contraction runs on v_mfma_f64_16x16x4_f64 in float64,
// whatever the element type of the stored matrix: elements are widened on load and the centring
// xc = (double)x - shift[column] is ONE float64 subtraction made on the way into LDS, the rounding NumPy's
// `Xd - m` makes.  No atomics anywhere: splits of a contraction are added by a finish kernel in ascending order.
//
// Operand maps of v_mfma_f64_16x16x4_f64 (as in kernels_gemm.hip): A lane l = A[m = l&15][k = l>>4],
// B lane l = B[k = l>>4][n = l&15], D lane l, reg q = D[m = (l>>4) + 4 q][n = l&15].
#include "aa_internal.h"
#include "gram_plan.h"

namespace aa {

typedef double f64x4p __attribute__((ext_vector_type(4)));

// two adjacent elements of a row, widened
__device__ __forceinline__ void load_pair(const float *p, double &a, double &b)
{
    const float2 v = *reinterpret_cast<const float2 *>(p);
    a = (double)v.x;
    b = (double)v.y;
}
__device__ __forceinline__ void load_pair(const double *p, double &a, double &b)
{
    const double2 v = *reinterpret_cast<const double2 *>(p);
    a = v.x;
    b = v.y;
}

// One value of the tile (ti, tj) at (a, b) into G, both places from the one value.  On a diagonal tile only the
// entries with a <= b are written, so that G[i][j] and G[j][i] never come from two accumulation chains.
__device__ __forceinline__ void gram_put(double *__restrict__ G, long g_ld, long ti, long tj, int a, int b, double v)
{
    if (ti != tj || a <= b) {
        G[(ti * 64 + a) * g_ld + tj * 64 + b] = v;
        G[(tj * 64 + b) * g_ld + ti * 64 + a] = v;
    }
}

// where a block leaves its 64 x 64 tile: G itself (one split) or its slot of the partials
__device__ __forceinline__ void gram_store(const f64x4p (&acc)[4], double *__restrict__ G, long g_ld,
                                           double *__restrict__ partial, long ti, long tj)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lr = lane >> 4;
    double *slot = partial ? partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4096 : nullptr;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int a = 16 * mt + lr + 4 * q, b = 16 * wave + lc;
            if (slot)
                slot[a * 64 + b] = acc[mt][q];
            else
                gram_put(G, g_ld, ti, tj, a, b, acc[mt][q]);
        }
}

// ---------------------------------------------------------------------------
// G = Xc Xc' by rows (NT product, contraction over the contiguous feature axis), in 64 x 64 tiles staged through
// LDS in 32-feature chunks -- the S stage of kernel_tile_product (kernels_gemm.hip) with three differences: T is
// float or double, the shift is applied on the way into LDS, and rows >= n come out as zeros, not -shift (the
// padding rows of X hold zeros; centring them would be the bug).  A wave owns 16 columns of the tile (rows of the
// tj block) against all 64 rows of the ti block: 4 accumulator tiles.  The chunks run to p rounded up to 32,
// inside the zero-padded row (ld is a multiple of 128); the shift table is zero-padded to ld, so padding features
// contribute 0 - 0.  grid = (tile pairs, splits); split s takes the features [s split_len, (s + 1) split_len).
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_gram_rows(const T *__restrict__ X, long ld, long n,
                                                   const double *__restrict__ shift, long tiles, long k_end,
                                                   long split_len, double *__restrict__ G, long g_ld,
                                                   double *__restrict__ partial)
{
    constexpr int TC = 32, LS = 34;
    __shared__ __attribute__((aligned(16))) double as[64 * LS];
    __shared__ __attribute__((aligned(16))) double bs[64 * LS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, lc = lane & 15, lr = lane >> 4;
    long ti, tj;
    gram_pair_tile(blockIdx.x, tiles, &ti, &tj);   // the block's tile pair (gram_plan.h)
    const long i0 = ti * 64, j0 = tj * 64;
    const long k0 = (long)blockIdx.y * split_len;
    const long k1 = k0 + split_len < k_end ? k0 + split_len : k_end;
    f64x4p acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = (f64x4p){0.0, 0.0, 0.0, 0.0};
    for (long q0 = k0; q0 < k1; q0 += TC) {
        __syncthreads();                                  // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cid = t + 256 * e, row = cid >> 4, col = 2 * (cid & 15);
            const double s0 = shift[q0 + col], s1 = shift[q0 + col + 1];
            double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
            if (i0 + row < n) {
                load_pair(X + (i0 + row) * ld + q0 + col, a0, a1);
                a0 -= s0;
                a1 -= s1;
            }
            if (j0 + row < n) {
                load_pair(X + (j0 + row) * ld + q0 + col, b0, b1);
                b0 -= s0;
                b1 -= s1;
            }
            as[row * LS + col] = a0;
            as[row * LS + col + 1] = a1;
            bs[row * LS + col] = b0;
            bs[row * LS + col + 1] = b1;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < TC / 4; ++s) {
            const double b = bs[(16 * wave + lc) * LS + 4 * s + lr];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[(16 * mt + lc) * LS + 4 * s + lr], b, acc[mt], 0, 0, 0);
        }
    }
    gram_store(acc, G, g_ld, partial, ti, tj);
}

// ---------------------------------------------------------------------------
// G = Xc' Xc by columns (TN product, contraction over rows).  Operand maps of k_col_weighted_sums and
// k_residual_scores (kernels_tall.hip): A lane l = xc[t0 + (l>>4)][i0 + (l&15)], B lane likewise for the j block.
// Both 64-column blocks are staged through LDS in chunks of 32 rows, so that a block's waves share the loads
// (row stride 80 doubles: the four rows a half-wave reads fall into disjoint banks).  Rows >= n enter as zeros;
// the shift table is zero-padded to ld, so padding columns stay zero.  The chunks run to n rounded up to 32,
// inside the padded rows of the allocation.  grid = (tile pairs, splits) over the rows.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_gram_cols(const T *__restrict__ X, long ld, long n,
                                                   const double *__restrict__ shift, long tiles, long k_end,
                                                   long split_len, double *__restrict__ G, long g_ld,
                                                   double *__restrict__ partial)
{
    constexpr int RC = 32, LS = 80;
    __shared__ __attribute__((aligned(16))) double as[RC * LS];
    __shared__ __attribute__((aligned(16))) double bs[RC * LS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, lc = lane & 15, lr = lane >> 4;
    long ti, tj;
    gram_pair_tile(blockIdx.x, tiles, &ti, &tj);   // the block's tile pair (gram_plan.h)
    const long i0 = ti * 64, j0 = tj * 64;
    const long k0 = (long)blockIdx.y * split_len;
    const long k1 = k0 + split_len < k_end ? k0 + split_len : k_end;
    // the columns a thread stages are the same in every chunk: so are their shifts
    const int scol = 2 * (t & 31);
    const double sa0 = shift[i0 + scol], sa1 = shift[i0 + scol + 1];
    const double sb0 = shift[j0 + scol], sb1 = shift[j0 + scol + 1];
    f64x4p acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = (f64x4p){0.0, 0.0, 0.0, 0.0};
    for (long t0 = k0; t0 < k1; t0 += RC) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = (t >> 5) + 8 * e;             // cid = t + 256 e: row = cid >> 5, column pair = cid & 31
            const long r = t0 + row;
            double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
            if (r < n) {
                load_pair(X + r * ld + i0 + scol, a0, a1);
                load_pair(X + r * ld + j0 + scol, b0, b1);
                a0 -= sa0;
                a1 -= sa1;
                b0 -= sb0;
                b1 -= sb1;
            }
            as[row * LS + scol] = a0;
            as[row * LS + scol + 1] = a1;
            bs[row * LS + scol] = b0;
            bs[row * LS + scol + 1] = b1;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < RC / 4; ++s) {
            const double b = bs[(4 * s + lr) * LS + 16 * wave + lc];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[(4 * s + lr) * LS + 16 * mt + lc], b, acc[mt], 0, 0, 0);
        }
    }
    gram_store(acc, G, g_ld, partial, ti, tj);
}

// G from the partial tiles: every entry is the sum of its splits in ascending order (k_sum_chunks is the
// precedent), written to both places.  One thread per entry of a tile, 16 blocks per tile pair.
__global__ __launch_bounds__(256) void k_gram_finish(const double *__restrict__ partial, long pairs, long tiles,
                                                     int nsplit, double *__restrict__ G, long g_ld)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long pair = idx >> 12;
    const int e = (int)(idx & 4095);
    if (pair >= pairs) return;
    double s = partial[pair * 4096 + e];
    for (int q = 1; q < nsplit; ++q) s += partial[((size_t)q * pairs + pair) * 4096 + e];
    long ti, tj;
    gram_pair_tile(pair, tiles, &ti, &tj);
    gram_put(G, g_ld, ti, tj, e >> 6, e & 63, s);
}

// G_dev ([g_ld][g_ld], whole tiles) = the Gram matrix of c's centred matrix as the plan cuts it; shift_dev: p_pad
// doubles, zero padded (zeros: no centring); partial_dev: plan.partial_bytes, unused with one split
int launch_gram(Ctx *c, const GramPlan &pl, const double *shift_dev, double *partial_dev, double *G_dev)
{
    const dim3 grid((unsigned)pl.pairs, (unsigned)pl.nsplit);
    const long k_end = round_up(pl.K, GRAM_CHUNK);
    double *part = pl.nsplit > 1 ? partial_dev : nullptr;
#define GRAM(KERNEL, T)                                                                                           \
    hipLaunchKernelGGL((KERNEL<T>), grid, dim3(256), 0, c->stream, (const T *)c->X.as<T>(), c->p_pad, c->n, shift_dev, \
                       pl.tiles, k_end, pl.split_len, G_dev, pl.g_ld, part)
    if (pl.side == GRAM_ROWS) {
        if (c->dtype == AA_F32) GRAM(k_gram_rows, float); else GRAM(k_gram_rows, double);
    } else {
        if (c->dtype == AA_F32) GRAM(k_gram_cols, float); else GRAM(k_gram_cols, double);
    }
#undef GRAM
    AA_CHECK_HIP(hipGetLastError());
    if (pl.nsplit > 1) {
        hipLaunchKernelGGL(k_gram_finish, dim3((unsigned)(pl.pairs * 16)), dim3(256), 0, c->stream,
                           (const double *)partial_dev, pl.pairs, pl.tiles, (int)pl.nsplit, G_dev, pl.g_ld);
        AA_CHECK_HIP(hipGetLastError());
    }
    return AA_OK;
}

// ---------------------------------------------------------------------------
// Y[r][i] = (TO) sum_j ((double)X[row0 + r][j] - shift[j]) V[i][j], row-local: a wave owns 16 rows, a block 64,
// and keeps NT component tiles of 16 x 16 accumulators per wave (NT <= 16: 256 components, 64 accumulator
// registers per lane).  A = the centred rows, B = V, four features per K step; both are streamed through LDS in
// chunks of 16 features (row stride 18 doubles: the 16 rows a half-wave reads fall into disjoint banks), the
// features in ascending order, so every output is one accumulation chain over j.  V is [16 NT][ldv] float64 on the
// device, zero padded in both directions; the chunks run to p rounded up to 16, inside the zero-padded rows of X
// (ld is a multiple of 128) where x - shift is 0 - 0.  Only rows r < n and components i < q are written, once,
// rounded to TO: the rest of the destination keeps the zeros of its allocation.
// ---------------------------------------------------------------------------
template <typename T, typename TO, int NT>
__global__ __launch_bounds__(256) void k_project_rows(const T *__restrict__ X, long ldx, long row0, long n, long k_end,
                                                      const double *__restrict__ V, long ldv,
                                                      const double *__restrict__ shift, int q, TO *__restrict__ Y,
                                                      long ldy)
{
    constexpr int FC = 16, LS = 18;
    __shared__ __attribute__((aligned(16))) double xs[64 * LS];
    __shared__ __attribute__((aligned(16))) double vs[16 * NT * LS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, lc = lane & 15, lr = lane >> 4;
    const long r0 = (long)blockIdx.x * 64;
    f64x4p acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f64x4p){0.0, 0.0, 0.0, 0.0};
    for (long j0 = 0; j0 < k_end; j0 += FC) {
        __syncthreads();                                  // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int cid = t + 256 * e, row = cid >> 3, col = 2 * (cid & 7);
            double a0 = 0.0, a1 = 0.0;
            if (r0 + row < n) {
                load_pair(X + (row0 + r0 + row) * ldx + j0 + col, a0, a1);
                a0 -= shift[j0 + col];
                a1 -= shift[j0 + col + 1];
            }
            xs[row * LS + col] = a0;
            xs[row * LS + col + 1] = a1;
        }
        for (int cid = t; cid < 16 * NT * 8; cid += 256) {
            const int row = cid >> 3, col = 2 * (cid & 7);
            const double2 v = *reinterpret_cast<const double2 *>(V + (long)row * ldv + j0 + col);
            vs[row * LS + col] = v.x;
            vs[row * LS + col + 1] = v.y;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < FC / 4; ++s) {
            const double a = xs[(16 * wave + lc) * LS + 4 * s + lr];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vs[(16 * nt + lc) * LS + 4 * s + lr], acc[nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const long r = r0 + 16 * wave + lr + 4 * qq;
            const int i = 16 * nt + lc;
            if (r < n && i < q) Y[r * ldy + i] = (TO)acc[nt][qq];
        }
}

// component tiles per wave the projection is instantiated for, and the rows of V that instantiation reads
static int project_tiles(int q)
{
    static const int sizes[] = {1, 2, 4, 8, 12, 16};
    for (int nt : sizes)
        if (16 * nt >= q) return nt;
    return 0;
}
int project_v_rows(int q) { return 16 * project_tiles(q); }

// dst ([.][dst_ld] of dst_dtype; rows [0, n), columns [0, q) are written) = the projection of rows
// [row0, row0 + n) of owner_X ([.][owner_ld] of owner_dtype, p features) onto the q rows of V_dev
// ([project_v_rows(q)][owner_ld] float64, zero padded); shift_dev: owner_ld doubles, zero padded
int launch_project_rows(Ctx *c, const void *owner_X, int owner_dtype, long owner_ld, long p, long row0, long n, int q,
                        const double *V_dev, const double *shift_dev, void *dst, long dst_ld, int dst_dtype)
{
    const int nt = project_tiles(q);
    AA_REQUIRE(q >= 1 && nt, AA_ERR_ARG, "projection onto %d components (1 to 256 are supported)", q);
    AA_REQUIRE(dst_dtype == owner_dtype || (owner_dtype == AA_F32 && dst_dtype == AA_F64), AA_ERR_ARG,
               "projection: equal element types, or float32 rows into a float64 block");
    const dim3 grid((unsigned)((n + 63) / 64));
    const long k_end = round_up(p, 16);
#define PROJECT(T, TO, NT)                                                                                        \
    hipLaunchKernelGGL((k_project_rows<T, TO, NT>), grid, dim3(256), 0, c->stream, (const T *)owner_X, owner_ld, row0, \
                       n, k_end, V_dev, owner_ld, shift_dev, q, (TO *)dst, dst_ld)
#define PROJECT_NT(T, TO)                                                                                         \
    switch (nt) {                                                                                                 \
    case 1: PROJECT(T, TO, 1); break;                                                                             \
    case 2: PROJECT(T, TO, 2); break;                                                                             \
    case 4: PROJECT(T, TO, 4); break;                                                                             \
    case 8: PROJECT(T, TO, 8); break;                                                                             \
    case 12: PROJECT(T, TO, 12); break;                                                                           \
    default: PROJECT(T, TO, 16); break;                                                                           \
    }
    if (owner_dtype == AA_F64) {
        PROJECT_NT(double, double)
    } else if (dst_dtype == AA_F64) {
        PROJECT_NT(float, double)
    } else {
        PROJECT_NT(float, float)
    }
#undef PROJECT_NT
#undef PROJECT
    AA_CHECK_HIP(hipGetLastError());
    return AA_OK;
}

}  // namespace aa

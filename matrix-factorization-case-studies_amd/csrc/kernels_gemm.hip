// kernels_gemm.hip -- the two skinny-GEMM shapes of the AA/GPNH solver against the
// resident data matrix X [n_pad][ldx] (gfx950 / CDNA4 only).
//
//   reduce-over-rows  out[i][c] = sum_r A[r][i] * X[r][c]      (k x p result)
//       C X   archetypal_analysis.py:262,297,544,618     (A = C', tall)
//       D X   (search direction; gives (C + lambda D) X by linearity)
//       Z'X   archetypal_analysis.py:548,641; gpnh_convex_coding.py:219
//       C K   archetypal_analysis.py:208,288,409,484     (kernel form)
//   row-local         out[r][i] = sum_c X[r][c] * B[i][c]      (n x k result)
//       (CX) X'   archetypal_analysis.py:299,545,619
//       X (X'Z)   archetypal_analysis.py:549,642
//       X W       gpnh_convex_coding.py:270,292,352
//       K Z       archetypal_analysis.py:411,502             (kernel form)
//
// float32 (v_mfma_f32_32x32x2_f32): every X element is read exactly once per pass.
// Algorithmic traffic per pass = n*p*4 bytes; 2*k*n*p flop; at k = 32 the intensity is
// 16 flop/B (< the 19.7 flop/B ridge) => HBM-bound.  reduce-over-rows loads X straight
// from HBM into the MFMA operand layout; row-local contracts along the contiguous axis and
// stages X through wave-private LDS tiles ("wave-streaming", k_row_local_f32_ws; older
// variants stay selectable).
// float64, the reference dtype (v_mfma_f64_16x16x4_f64): the same two structures,
// k_reduce_rows_f64_mfma and k_row_local_f64_ws / _mfma; the f64 VALU kernels they replaced
// remain behind aa_set_option("f64_mfma", 0).
#include "aa_internal.h"

namespace aa {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// XCD-aware (column group, row slab) of a block.  Workgroups are dealt round-robin over the 8
// XCDs (blocks b and b + 8 share one; MI355X_MICROARCH.md, Workgroup dispatch), and every XCD
// has its own L2.  With the natural map (column group = blockIdx.x) all blocks of a column
// group sit on one XCD, so each of the 8 XCDs pulls the WHOLE tall operand through its L2
// (8 x 25.6 MB at the headline size: the 1.19x traffic of round 1).  Here the blocks of one row
// slab -- which read the same rows of the tall operand -- are given linear ids that agree
// modulo 8, so every slab of the tall operand is fetched by one XCD only.  Placement is a speed
// matter only: any map that is a bijection is correct.
__device__ __forceinline__ void xcd_aware_block(int &colgroup, int &slab)
{
    const int ncg = (int)gridDim.x, nsl = (int)gridDim.y;
    colgroup = (int)blockIdx.x;
    slab = (int)blockIdx.y;
    if (nsl % 8 == 0) {
        const int b = (int)blockIdx.x + ncg * (int)blockIdx.y;   // dispatch order: x fastest
        const int q = b >> 3, r = b & 7;
        slab = r + 8 * (q / ncg);
        colgroup = q % ncg;
    }
}

// ---------------------------------------------------------------------------
// reduce over rows, float32 MFMA.
// grid = (ceil(p_pad/512), nslab); block = 4 waves; wave w owns the 128-column
// strip c0 = (4*blockIdx.x + w)*128 and rows [slab*rows_per_slab, +rows_per_slab).
// MFMA 32x32x2: A-operand lane l = A[row r0+2u+(l>>5)][component l&31],
// B-operand lane l = X[row r0+2u+(l>>5)][c0 + 4*(l&31) + m]  (one dwordx4 load feeds
// the four MFMAs m = 0..3, whose output columns are c0 + 4*j + m).
// ---------------------------------------------------------------------------
// GATED: the launch behind k_reduce_rows_gather_f32 -- a slab whose mode byte says that the gather
// kernel has written its partial block is left alone (slab_mode is not read otherwise).
template <int NCT, int U, bool GATED = false>
__global__ __launch_bounds__(256) void k_reduce_rows_f32(const float *__restrict__ X, long ldx,
                                                         const double *__restrict__ A,
                                                         long rows_per_slab, long n_pad, int p_pad,
                                                         float *__restrict__ partial,
                                                         const unsigned char *__restrict__ slab_mode)
{
    constexpr int KP = 32 * NCT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int colgroup, slab;
    xcd_aware_block(colgroup, slab);
    if constexpr (GATED)
        if (slab_mode[slab]) return;   // block-uniform
    const int c0 = (colgroup * 4 + wave) * 128;
    if (c0 >= p_pad) return;   // wave-uniform; the kernel has no barriers
    const int h = lane >> 5, j = lane & 31;
    const long r_begin = (long)slab * rows_per_slab;
    long r_end = r_begin + rows_per_slab;
    if (r_end > n_pad) r_end = n_pad;

    f32x16 acc[NCT][4];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ct][m][e] = 0.f;

    // Two register sets, software-pipelined one half-step (2*U rows) ahead: while the
    // MFMAs of one set run, the U dwordx4 loads of the other are in flight.  The
    // sched_barriers keep hipcc from sinking the loads down to their first use.
    const float *xp = X + (r_begin + h) * ldx + c0 + 4 * j;
    const double *ap = A + (r_begin + h) * KP + j;
    f32x4 xa[U], xb[U];
    double aa[U][NCT], ab[U][NCT];
#define RR_LOAD(XV, AV, ROWOFF)                                                              \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                                           \
        XV[u] = *reinterpret_cast<const f32x4 *>(xp + (long)((ROWOFF) + 2 * u) * ldx);        \
        _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct)                                    \
            AV[u][ct] = ap[((ROWOFF) + 2 * u) * KP + ct * 32];                                \
    }
#define RR_COMPUTE(XV, AV)                                                                   \
    _Pragma("unroll") for (int u = 0; u < U; ++u)                                             \
        _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) {                                  \
            const float af = (float)AV[u][ct];                                                \
            _Pragma("unroll") for (int m = 0; m < 4; ++m)                                     \
                acc[ct][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, XV[u][m], acc[ct][m],  \
                                                                  0, 0, 0);                   \
        }
    RR_LOAD(xa, aa, 0)
    for (long r = r_begin; r < r_end; r += 4 * U) {
        RR_LOAD(xb, ab, 2 * U)      // may run past r_end: X and A carry AA_SLACK_ROWS zero rows
        __builtin_amdgcn_sched_barrier(0);
        RR_COMPUTE(xa, aa)
        __builtin_amdgcn_sched_barrier(0);
        RR_LOAD(xa, aa, 4 * U)
        __builtin_amdgcn_sched_barrier(0);
        RR_COMPUTE(xb, ab)          // the row range is a multiple of 4*U
        __builtin_amdgcn_sched_barrier(0);
        xp += (long)(4 * U) * ldx;
        ap += (4 * U) * KP;
    }
#undef RR_LOAD
#undef RR_COMPUTE

    // D layout (32x32): column = lane&31 (-> 4 data columns c0+4j+m), row (component)
    // = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
    float *out = partial + (size_t)slab * KP * p_pad;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int comp = ct * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            f32x4 v = {acc[ct][0][reg], acc[ct][1][reg], acc[ct][2][reg], acc[ct][3][reg]};
            *reinterpret_cast<f32x4 *>(out + (size_t)comp * p_pad + c0 + 4 * j) = v;
        }
}

// reduce over rows, float64 VALU: thread = data column, KP accumulators in registers,
// A[r][*] is wave-uniform (scalar loads).
template <int KP>
__global__ __launch_bounds__(256) void k_reduce_rows_f64(const double *__restrict__ X, long ldx,
                                                         const double *__restrict__ A,
                                                         long rows_per_slab, long n_pad, int p_pad,
                                                         double *__restrict__ partial)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p_pad) return;
    const long r_begin = (long)blockIdx.y * rows_per_slab;
    long r_end = r_begin + rows_per_slab;
    if (r_end > n_pad) r_end = n_pad;
    double acc[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) acc[i] = 0.0;
    for (long r = r_begin; r < r_end; ++r) {
        const double x = X[r * ldx + c];
        const double *a = A + r * KP;
#pragma unroll
        for (int i = 0; i < KP; ++i) acc[i] = fma(a[i], x, acc[i]);
    }
    double *out = partial + (size_t)blockIdx.y * KP * p_pad;
#pragma unroll
    for (int i = 0; i < KP; ++i) out[(size_t)i * p_pad + c] = acc[i];
}

// ---------------------------------------------------------------------------
// float64 data (the reference dtype) on the f64 matrix cores, v_mfma_f64_16x16x4_f64:
// A-operand lane l = Aop[m = l&15][k = l>>4], B-operand lane l = Bop[n = l&15][k = l>>4],
// D lane l, reg r = D[m = (l>>4) + 4r][n = l&15]   (D = Aop * Bop').
// ---------------------------------------------------------------------------
typedef double f64x4g __attribute__((ext_vector_type(4)));
typedef double f64x2g __attribute__((ext_vector_type(2)));

// reduce over rows: D[m = component][n = column] += sum over 4 rows.  A wave owns a
// 64-column strip and a row slab; per 4 rows a lane loads NT doubles of the tall operand and
// two 16-byte pieces of X (columns c0 + 32u + 2*(l&15) + e: the two doubles of a piece feed
// the B operands of two different column tiles, so the loads are 256 contiguous bytes per
// row and quarter-wave).  Two register sets, software-pipelined as in k_reduce_rows_f32.
// GATED: as in k_reduce_rows_f32.
template <int NT, bool GATED = false>
__global__ __launch_bounds__(256) void k_reduce_rows_f64_mfma(const double *__restrict__ X, long ldx,
                                                              const double *__restrict__ A,
                                                              long rows_per_slab, long n_pad,
                                                              int p_pad, double *__restrict__ partial,
                                                              const unsigned char *__restrict__ slab_mode)
{
    constexpr int KP = 16 * NT, U = 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int colgroup, slab;
    xcd_aware_block(colgroup, slab);
    if constexpr (GATED)
        if (slab_mode[slab]) return;   // block-uniform
    const int c0 = (colgroup * 4 + wave) * 64;
    if (c0 >= p_pad) return;   // wave-uniform; the kernel has no barriers
    const int lc = lane & 15, lr = lane >> 4;
    const long r_begin = (long)slab * rows_per_slab;
    long r_end = r_begin + rows_per_slab;
    if (r_end > n_pad) r_end = n_pad;

    f64x4g acc[NT][2][2];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 2; ++e) acc[ti][u][e] = (f64x4g){0.0, 0.0, 0.0, 0.0};

    const double *xp = X + (r_begin + lr) * ldx + c0 + 2 * lc;
    const double *ap = A + (r_begin + lr) * KP + lc;
    f64x2g xa[U][2], xb[U][2];
    double aa[U][NT], ab[U][NT];
#define RD_LOAD(XV, AV, ROWOFF)                                                              \
    _Pragma("unroll") for (int q = 0; q < U; ++q) {                                           \
        _Pragma("unroll") for (int u = 0; u < 2; ++u)                                         \
            XV[q][u] = *reinterpret_cast<const f64x2g *>(xp + (long)((ROWOFF) + 4 * q) * ldx + 32 * u); \
        _Pragma("unroll") for (int ti = 0; ti < NT; ++ti)                                     \
            AV[q][ti] = ap[((ROWOFF) + 4 * q) * KP + 16 * ti];                                \
    }
#define RD_COMPUTE(XV, AV)                                                                   \
    _Pragma("unroll") for (int q = 0; q < U; ++q)                                             \
        _Pragma("unroll") for (int ti = 0; ti < NT; ++ti)                                     \
            _Pragma("unroll") for (int u = 0; u < 2; ++u)                                     \
                _Pragma("unroll") for (int e = 0; e < 2; ++e)                                 \
                    acc[ti][u][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(AV[q][ti], XV[q][u][e],   \
                                                                         acc[ti][u][e], 0, 0, 0);
    RD_LOAD(xa, aa, 0)
    for (long r = r_begin; r < r_end; r += 8 * U) {
        RD_LOAD(xb, ab, 4 * U)      // may run past r_end: X and A carry AA_SLACK_ROWS zero rows
        __builtin_amdgcn_sched_barrier(0);
        RD_COMPUTE(xa, aa)
        __builtin_amdgcn_sched_barrier(0);
        RD_LOAD(xa, aa, 8 * U)
        __builtin_amdgcn_sched_barrier(0);
        RD_COMPUTE(xb, ab)          // the row range is a multiple of 8*U
        __builtin_amdgcn_sched_barrier(0);
        xp += (long)(8 * U) * ldx;
        ap += (8 * U) * KP;
    }
#undef RD_LOAD
#undef RD_COMPUTE
    double *out = partial + (size_t)slab * KP * p_pad;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int comp = 16 * ti + lr + 4 * reg;
                f64x2g v = {acc[ti][u][0][reg], acc[ti][u][1][reg]};
                *reinterpret_cast<f64x2g *>(out + (size_t)comp * p_pad + c0 + 32 * u + 2 * lc) = v;
            }
}

// row-local: D[m = row][n = component].  Block = 64 rows (a wave per 16), both operands
// staged through LDS in 32-column tiles with coalesced 16-byte loads, register-prefetched one
// tile ahead; LDS row stride 34 doubles => conflict-free fragment reads.
// Short, wide matrices (n = 1610, p = 25 000: the HadISST shape) have too few 64-row blocks to
// fill the chip (26 of them: 0.7 ms per pass for 322 MB), so the contraction is also split over
// blockIdx.y: chunk `col_chunk` columns per block, partial results to out + blockIdx.y * n_pad *
// KP, summed in a fixed order by k_sum_chunks.  col_chunk = p_pad and gridDim.y = 1: unsplit.
template <int NT>
__global__ __launch_bounds__(256) void k_row_local_f64_mfma(const double *__restrict__ X, long ldx,
                                                            const double *__restrict__ B, int p_pad,
                                                            double *__restrict__ out, long n_pad,
                                                            int col_chunk)
{
    constexpr int KP = 16 * NT, TC = 32, LS = 34;
    const int c_begin = (int)blockIdx.y * col_chunk;
    int c_end = c_begin + col_chunk;
    if (c_end > p_pad) c_end = p_pad;
    out += (size_t)blockIdx.y * n_pad * KP;
    constexpr int NB = KP * 16 / 256;                 // B chunks per thread and tile
    __shared__ __attribute__((aligned(16))) double xs[64 * LS];
    __shared__ __attribute__((aligned(16))) double bs[KP * LS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int lc = lane & 15, lr = lane >> 4;
    const long r0 = (long)blockIdx.x * 64;            // grid = n_pad / 64 exactly
    f64x4g acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f64x4g){0.0, 0.0, 0.0, 0.0};

    f64x2g sx[4], sb[NB];
    auto load_tile = [&](int c0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cid = t + 256 * e;
            sx[e] = *reinterpret_cast<const f64x2g *>(X + (r0 + (cid >> 4)) * ldx + c0 + 2 * (cid & 15));
        }
#pragma unroll
        for (int e = 0; e < NB; ++e) {
            const int cid = t + 256 * e;
            sb[e] = *reinterpret_cast<const f64x2g *>(B + (long)(cid >> 4) * p_pad + c0 + 2 * (cid & 15));
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cid = t + 256 * e;
            *reinterpret_cast<f64x2g *>(xs + (cid >> 4) * LS + 2 * (cid & 15)) = sx[e];
        }
#pragma unroll
        for (int e = 0; e < NB; ++e) {
            const int cid = t + 256 * e;
            *reinterpret_cast<f64x2g *>(bs + (cid >> 4) * LS + 2 * (cid & 15)) = sb[e];
        }
    };
    if (c_begin < c_end) load_tile(c_begin);
    for (int c0 = c_begin; c0 < c_end; c0 += TC) {
        store_tile();
        __syncthreads();
        if (c0 + TC < c_end) load_tile(c0 + TC);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < TC / 4; ++s) {
            const double a = xs[(wave * 16 + lc) * LS + 4 * s + lr];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bs[(16 * nt + lc) * LS + 4 * s + lr],
                                                               acc[nt], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            out[(r0 + wave * 16 + lr + 4 * reg) * KP + 16 * nt + lc] = acc[nt][reg];
}

// out[e] = sum over the column chunks of partial[s][e], s in increasing order (deterministic)
__global__ __launch_bounds__(256) void k_sum_chunks(const double *__restrict__ partial, long elems,
                                                    int nsplit, double *__restrict__ out)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    double s = partial[e];
    for (int q = 1; q < nsplit; ++q) s += partial[(size_t)q * elems + e];
    out[e] = s;
}

// row-local, float64, "wave-streaming" form (the structure of k_row_local_f32_ws): a block is
// W waves on one CU, every wave owns 32 rows (two 16-row MFMA tiles) for the whole kernel
// and streams them through a wave-private LDS tile of 32 columns (256-byte row segments in,
// fragments out, no barrier), one tile register-prefetched ahead; the small operand is shared
// as double-buffered 64-column slabs (one barrier per slab).  Row strides of 34 / 66 doubles
// make the fragment reads conflict free.  Dynamic LDS = 2 * KP * 66 * 8 + W * 32 * 34 * 8 B.
template <int NT>
__global__ __launch_bounds__(NT == 2 ? 1024 : 768) void k_row_local_f64_ws(const double *__restrict__ X, long ldx,
                                                                             const double *__restrict__ B,
                                                                             int p_pad, double *__restrict__ out,
                                                                             long n_pad, int W)
{
    constexpr int KP = 16 * NT, SB = 64, TC = 32, XS = 34, BS = 66;
    constexpr int NBI = NT;                          // B chunks per thread and slab at >= 512 threads
    extern __shared__ __attribute__((aligned(16))) double wsd_smem[];
    const int t = threadIdx.x, lane = t & 63, nthreads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    double *bs = wsd_smem;
    double *xs = wsd_smem + 2 * KP * BS + wave * (32 * XS);
    const long r0 = ((long)blockIdx.x * W + wave) * 32;
    const bool active = r0 < n_pad;
    const long r0c = active ? r0 : n_pad - 32;       // surplus waves recompute the last tile
    const int lc = lane & 15, lr = lane >> 4;

    f64x4g acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f64x4g){0.0, 0.0, 0.0, 0.0};

    f64x2g sb[NBI], sx[8];
    auto load_b = [&](int c0) {
#pragma unroll
        for (int e = 0; e < NBI; ++e) {
            const int cid = (t + e * nthreads) & (KP * 32 - 1);     // 32 chunks of 16 B per component
            sb[e] = *reinterpret_cast<const f64x2g *>(B + (long)(cid >> 5) * p_pad + c0 + 2 * (cid & 31));
        }
    };
    auto store_b = [&](int buf) {
#pragma unroll
        for (int e = 0; e < NBI; ++e) {
            const int cid = (t + e * nthreads) & (KP * 32 - 1);
            *reinterpret_cast<f64x2g *>(bs + buf * (KP * BS) + (cid >> 5) * BS + 2 * (cid & 31)) = sb[e];
        }
    };
    const int xr = lane >> 4, xc = lane & 15;
    const double *gx = X + (r0c + xr) * ldx + 2 * xc;
    auto load_x = [&](int c0) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            sx[e] = *reinterpret_cast<const f64x2g *>(gx + (long)(4 * e) * ldx + c0);
    };
    auto store_x = [&]() {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            *reinterpret_cast<f64x2g *>(xs + (4 * e + xr) * XS + 2 * xc) = sx[e];
    };
    auto compute = [&](int buf, int half) {
        const double *bb = bs + buf * (KP * BS) + half * TC;
#pragma unroll
        for (int s = 0; s < TC / 4; ++s) {
            double bv[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = bb[(16 * nt + lc) * BS + 4 * s + lr];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const double a = xs[(16 * mt + lc) * XS + 4 * s + lr];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv[nt], acc[mt][nt], 0, 0, 0);
            }
        }
    };

    const int nslab = p_pad / SB;
    load_b(0);
    load_x(0);
    store_b(0);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
        const int c0 = s * SB;
        const int snext = s + 1 < nslab ? s + 1 : s;       // last slab: harmless reload
        store_x();                                // wave-private: LDS is in order per wave
        load_x(c0 + TC);
        load_b(snext * SB);
        __builtin_amdgcn_sched_barrier(0);
        compute(s & 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        store_x();
        store_b((s + 1) & 1);                     // that buffer was last read before the previous barrier
        load_x(snext * SB);
        __builtin_amdgcn_sched_barrier(0);
        compute(s & 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
    }
    if (active) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    out[(r0 + 16 * mt + lr + 4 * reg) * KP + 16 * nt + lc] = acc[mt][nt][reg];
    }
}

// second stage of the split-row reduction: fixed summation order => deterministic.
template <typename TP, typename TO>
__global__ __launch_bounds__(256) void k_reduce_partials(const TP *__restrict__ partial, long nslab,
                                                         long elems, double *__restrict__ out,
                                                         TO *__restrict__ outT)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= elems) return;
    double s = 0.0;
#pragma unroll 16
    for (long sl = 0; sl < nslab; ++sl) s += (double)partial[sl * elems + idx];
    out[idx] = s;
    if (outT) outT[idx] = (TO)s;
}

// ---------------------------------------------------------------------------
// row-local, float32 MFMA.  wave owns 32*RT rows; contraction over the columns.
// A-operand lane l = X[r0 + 32*rt + (l&31)][c + 8u + 4*(l>>5) + m]
// B-operand lane l = B[32*ct + (l&31)][c + 8u + 4*(l>>5) + m]      (m = 0..3 from one
// dwordx4 load each); D[row][component]: component = lane&31, row = (reg&3)+8*(reg>>2)+4*(l>>5).
// ---------------------------------------------------------------------------
template <int NCT, int RT>
__global__ __launch_bounds__(256) void k_row_local_f32(const float *__restrict__ X, long ldx,
                                                       const float *__restrict__ B, int p_pad,
                                                       double *__restrict__ out, long n_pad)
{
    constexpr int KP = 32 * NCT;
    constexpr int U = 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long r0 = ((long)blockIdx.x * 4 + wave) * (32 * RT);
    if (r0 >= n_pad) return;
    const int h = lane >> 5, j = lane & 31;

    f32x16 acc[RT][NCT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rt][ct][e] = 0.f;

    const float *xp = X + (r0 + j) * ldx + 4 * h;
    const float *bp = B + (long)j * p_pad + 4 * h;
    for (int c = 0; c < p_pad; c += 8 * U) {
        f32x4 xv[U][RT], bv[U][NCT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                xv[u][rt] = *reinterpret_cast<const f32x4 *>(xp + (long)(rt * 32) * ldx + c + 8 * u);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                bv[u][ct] = *reinterpret_cast<const f32x4 *>(bp + (long)(ct * 32) * p_pad + c + 8 * u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                            xv[u][rt][m], bv[u][ct][m], acc[rt][ct], 0, 0, 0);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const long row = r0 + rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                out[row * KP + ct * 32 + j] = (double)acc[rt][ct][reg];
            }
}

// row-local, float32 MFMA, X staged through wave-private LDS.
// Each wave owns 32 rows and streams them in [32 rows][128 columns] tiles (16 KB): the
// HBM side is 16 fully coalesced loads (two 512-byte row segments per wave-instruction,
// register-prefetched one tile ahead), the MFMA side reads its A fragments from LDS with
// ds_read_b128.  16-byte chunk c of row r is stored at chunk c ^ (r & 15), so the 16
// lanes of a ds_read_b128 group (16 different rows, same logical chunk) hit 16 different
// bank groups.  The tile is private to the wave: no barriers.
template <int NCT>
__global__ __launch_bounds__(256) void k_row_local_f32_lds(const float *__restrict__ X, long ldx,
                                                           const float *__restrict__ B, int p_pad,
                                                           double *__restrict__ out, long n_pad)
{
    constexpr int KP = 32 * NCT;
    __shared__ __attribute__((aligned(16))) float tiles[4][32 * 128];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long r0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (r0 >= n_pad) return;
    const int h = lane >> 5, j = lane & 31;
    float *my = tiles[wave];

    f32x16 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ct][e] = 0.f;

    const float *gbase = X + (r0 + h) * ldx + 4 * j;       // lane: row 2e + h, chunk j
    const float *bp = B + (long)j * p_pad + 4 * h;
    f32x4 stage[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) stage[e] = *reinterpret_cast<const f32x4 *>(gbase + (long)(2 * e) * ldx);

    for (int c0 = 0; c0 < p_pad; c0 += 128) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = 2 * e + h;
            *reinterpret_cast<f32x4 *>(my + row * 128 + ((j ^ (row & 15)) << 2)) = stage[e];
        }
        if (c0 + 128 < p_pad) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                stage[e] = *reinterpret_cast<const f32x4 *>(gbase + (long)(2 * e) * ldx + c0 + 128);
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead of the MFMA block
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(my + j * 128 + (((2 * q + h) ^ (j & 15)) << 2));
            f32x4 bv[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                bv[ct] = *reinterpret_cast<const f32x4 *>(bp + (long)(ct * 32) * p_pad + c0 + 8 * q);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bv[ct][m], acc[ct], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long row = r0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            out[row * KP + ct * 32 + j] = (double)acc[ct][reg];
        }
}

// row-local, float32 MFMA, classic block-tiled form: the 4 waves of a block own 32 rows
// each (X tiles wave-private in LDS) and SHARE the [KP][TC] tile of the small operand B
// through LDS, so B crosses L2->L1 once per block instead of once per wave (in the
// wave-private kernels B traffic equals the X traffic).  Both tiles are register-
// prefetched one step ahead.  TC = tile columns (32/64/128); DB = double-buffered LDS
// (one barrier per tile instead of two).  16-byte chunk c of row r sits at a swizzled
// chunk so that the 16 lanes of a ds_read_b128 group (16 rows, same logical chunk) hit 16
// different bank groups: c ^ (r & 15) for rows >= 256 B, c ^ ((r >> 1) & 7) for 128-B rows.
template <int TC>
__device__ __forceinline__ int rl_phys_chunk(int row, int chunk)
{
    if constexpr (TC >= 64) return chunk ^ (row & 15);
    else return chunk ^ ((row >> 1) & 7);
}

// blockIdx.y: column chunk of `col_chunk` columns (a multiple of TC), partial result to
// out + blockIdx.y * n_pad * KP, summed in a fixed order by k_sum_chunks -- short shards (the
// 12 500 rows of an 8-GPU run are 98 row blocks) otherwise leave most CUs idle.
template <int NCT, int TC, bool DB, bool ACC64 = false>
__global__ __launch_bounds__(256) void k_row_local_f32_blk(const float *__restrict__ X, long ldx,
                                                           const float *__restrict__ B, int p_pad,
                                                           double *__restrict__ out, long n_pad,
                                                           int col_chunk)
{
    constexpr int KP = 32 * NCT;
    constexpr int CPR = TC / 4;                  // 16-byte chunks per tile row
    constexpr int RPI = 64 / CPR;                // tile rows covered by one wave-instruction
    constexpr int NXI = 32 / RPI;                // X load instructions per wave per tile
    constexpr int NBI = KP * CPR / 256;          // B load instructions per thread per tile
    constexpr int NBUF = DB ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float xs[NBUF][4][32 * TC];
    __shared__ __attribute__((aligned(16))) float bs[NBUF][KP * TC];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long r0 = ((long)blockIdx.x * 4 + wave) * 32;      // grid = n_pad / 128 exactly
    const int h = lane >> 5, j = lane & 31;

    f32x16 acc[NCT];
    double accd[ACC64 ? NCT : 1][16];            // ACC64: see k_row_local_f32_ws
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ct][e] = 0.f;
#pragma unroll
    for (int ct = 0; ct < (ACC64 ? NCT : 1); ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) accd[ct][e] = 0.0;

    const int xr = lane / CPR, xc = lane % CPR;
    const float *gx = X + (r0 + xr) * ldx + 4 * xc;
    f32x4 sx[NXI], sb[NBI];
    auto load_tile = [&](int c0) {
#pragma unroll
        for (int e = 0; e < NXI; ++e)
            sx[e] = *reinterpret_cast<const f32x4 *>(gx + (long)(RPI * e) * ldx + c0);
#pragma unroll
        for (int e = 0; e < NBI; ++e) {
            const int cid = t + 256 * e;
            sb[e] = *reinterpret_cast<const f32x4 *>(B + (long)(cid / CPR) * p_pad + c0 + 4 * (cid % CPR));
        }
    };
    auto store_tile = [&](int buf) {
        float *myx = xs[buf][wave];
#pragma unroll
        for (int e = 0; e < NXI; ++e) {
            const int row = RPI * e + xr;
            *reinterpret_cast<f32x4 *>(myx + ((row * CPR + rl_phys_chunk<TC>(row, xc)) << 2)) = sx[e];
        }
#pragma unroll
        for (int e = 0; e < NBI; ++e) {
            const int cid = t + 256 * e, comp = cid / CPR, ch = cid % CPR;
            *reinterpret_cast<f32x4 *>(bs[buf] + ((comp * CPR + rl_phys_chunk<TC>(comp, ch)) << 2)) = sb[e];
        }
    };
    auto compute_tile = [&](int buf) {
        const float *myx = xs[buf][wave];
#pragma unroll
        for (int q = 0; q < TC / 8; ++q) {
            const int pc = rl_phys_chunk<TC>(j, 2 * q + h) << 2;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(myx + j * TC + pc);
            f32x4 bv[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                bv[ct] = *reinterpret_cast<const f32x4 *>(bs[buf] + (ct * 32 + j) * TC + pc);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bv[ct][m], acc[ct], 0, 0, 0);
            if constexpr (ACC64) {
                if ((q & 3) == 3) {                 // 32 columns done: the fp32 chain ends here
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            accd[ct][e] += (double)acc[ct][e];
                            acc[ct][e] = 0.f;
                        }
                }
            }
        }
    };

    const int c_begin = (int)blockIdx.y * col_chunk;
    const int c_end = c_begin + col_chunk < p_pad ? c_begin + col_chunk : p_pad;
    out += (size_t)blockIdx.y * (size_t)n_pad * KP;
    load_tile(c_begin);
    if constexpr (DB) {
        store_tile(0);
        __syncthreads();
        int buf = 0;
        for (int c0 = c_begin; c0 < c_end; c0 += TC) {
            const bool more = c0 + TC < c_end;
            if (more) load_tile(c0 + TC);
            __builtin_amdgcn_sched_barrier(0);
            compute_tile(buf);
            if (more) store_tile(buf ^ 1);     // last read two barriers ago
            __syncthreads();
            buf ^= 1;
        }
    } else {
        for (int c0 = c_begin; c0 < c_end; c0 += TC) {
            store_tile(0);
            __syncthreads();
            if (c0 + TC < c_end) load_tile(c0 + TC);
            __builtin_amdgcn_sched_barrier(0);
            compute_tile(0);
            __syncthreads();
        }
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long row = r0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            if constexpr (ACC64) out[row * KP + ct * 32 + j] = accd[ct][reg];
            else out[row * KP + ct * 32 + j] = (double)acc[ct][reg];
        }
}

// row-local, float32 MFMA, "wave-streaming" form.  The block-tiled kernel above spends
// its time at block barriers (two per 64..128 columns), so HBM time and MFMA time add up
// instead of overlapping.  Here a block is W waves on one CU; every wave owns one 32-row
// tile for the whole kernel and streams its X through a WAVE-PRIVATE LDS tile (coalesced
// 256-byte row segments in, MFMA fragment layout out; only s_waitcnt, no barrier), one
// tile register-prefetched ahead.  The small operand B is shared by the whole block as
// double-buffered 128-column slabs in LDS: one barrier per 128 columns, B crosses
// L2->LDS once per W*32 rows.  Dynamic LDS = 2 slabs (KP*512 B each) + W * 8 KB.
// ACC64: the fp32 accumulation chain is cut after every 32 columns (16 matrix instructions) and
// the partial sums are added up in float64 (VALU, 32 more registers => 3 waves per SIMD, W <= 12).
// x_r . p_i is a COHERENT sum (a sample against an archetype built from samples like it), so the
// fp32 rounding of a long running sum is systematic: relative error ~ eps32 * L / 400 for chains of
// L columns -- 6.9e-7 unchained (measured, p = 4096), 8.8e-8 at L = 512, 5e-9 at L = 32.  On
// bench.py's parity_converged problem that difference decides whether a float32 run stays on
// the reference's trajectory.
template <int NCT, bool ACC64>
__global__ __launch_bounds__(!ACC64 ? (NCT == 1 ? 1024 : 768) : (NCT == 1 ? 768 : 512)) void k_row_local_f32_ws(const float *__restrict__ X, long ldx,
                                                           const float *__restrict__ B, int p_pad,
                                                           double *__restrict__ out, long n_pad,
                                                           int W)
{
    constexpr int KP = 32 * NCT;
    constexpr int SB = 128, TC = 64;
    constexpr int NBI = 2 * NCT;                 // B chunks per thread per slab at >= 512 threads
    extern __shared__ __attribute__((aligned(16))) float ws_smem[];
    const int t = threadIdx.x, lane = t & 63, nthreads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // scalar: uniform row base
    float *bs = ws_smem;
    float *xs = ws_smem + 2 * KP * SB + wave * (32 * TC);
    const long r0 = ((long)blockIdx.x * W + wave) * 32;
    const bool active = r0 < n_pad;              // wave-uniform
    // surplus waves of the last block recompute the last tile (no branches in the loop)
    const long r0c = active ? r0 : n_pad - 32;
    const int h = lane >> 5, j = lane & 31;

    f32x16 acc[NCT];
    double accd[ACC64 ? NCT : 1][16];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ct][e] = 0.f;
#pragma unroll
    for (int ct = 0; ct < (ACC64 ? NCT : 1); ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) accd[ct][e] = 0.0;

    f32x4 sb[NBI], sx[8];
    auto load_b = [&](int c0) {
#pragma unroll
        for (int e = 0; e < NBI; ++e) {
            const int cid = (t + e * nthreads) & (KP * 32 - 1);   // >= 512 threads: wraps only
            sb[e] = *reinterpret_cast<const f32x4 *>(B + (long)(cid >> 5) * p_pad + c0 + 4 * (cid & 31));
        }                                                          // onto identical data
    };
    auto store_b = [&](int buf) {
#pragma unroll
        for (int e = 0; e < NBI; ++e) {
            const int cid = (t + e * nthreads) & (KP * 32 - 1);
            const int comp = cid >> 5, ch = cid & 31;
            *reinterpret_cast<f32x4 *>(bs + buf * (KP * SB) + ((comp * 32 + (ch ^ (comp & 15))) << 2)) = sb[e];
        }
    };
    const int xr = lane >> 4, xc = lane & 15;
    const float *gx = X + (r0c + xr) * ldx + 4 * xc;
    auto load_x = [&](int c0) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            sx[e] = *reinterpret_cast<const f32x4 *>(gx + (long)(4 * e) * ldx + c0);
    };
    auto store_x = [&]() {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int row = 4 * e + xr;
            *reinterpret_cast<f32x4 *>(xs + ((row * 16 + (xc ^ (row & 15))) << 2)) = sx[e];
        }
    };
    auto compute = [&](int buf, int half) {
        const float *bb = bs + buf * (KP * SB);
        f32x4 a, bv[NCT], an, bn[NCT];
        auto frag = [&](int q, f32x4 &fa, f32x4 (&fb)[NCT]) {
            const int pcx = ((2 * q + h) ^ (j & 15)) << 2;
            const int pcb = ((half * 16 + 2 * q + h) ^ (j & 15)) << 2;
            fa = *reinterpret_cast<const f32x4 *>(xs + j * TC + pcx);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                fb[ct] = *reinterpret_cast<const f32x4 *>(bb + (ct * 32 + j) * SB + pcb);
        };
        if constexpr (!ACC64 || NCT == 1) frag(0, a, bv);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if constexpr (!ACC64 || NCT == 1) {
                if (q + 1 < 8) frag(q + 1, an, bn);     // fragments of the next step in flight
            } else {
                frag(q, a, bv);                         // k > 32 with float64 sums: no second fragment set
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bv[ct][m], acc[ct], 0, 0, 0);
            if constexpr (!ACC64 || NCT == 1) {
                a = an;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) bv[ct] = bn[ct];
            }
            if constexpr (ACC64) {
                if ((q & 3) == 3) {                 // 32 columns done: the chain ends here
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            accd[ct][e] += (double)acc[ct][e];
                            acc[ct][e] = 0.f;
                        }
                }
            }
        }
    };

    const int nslab = p_pad / SB;
    load_b(0);
    load_x(0);
    store_b(0);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
        const int c0 = s * SB;
        const int snext = s + 1 < nslab ? s + 1 : s;       // last slab: harmless reload
        store_x();                                // wave-private: LDS is in order per wave
        load_x(c0 + TC);
        load_b(snext * SB);
        __builtin_amdgcn_sched_barrier(0);
        compute(s & 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        store_x();
        store_b((s + 1) & 1);                     // that buffer was last read before the previous barrier
        load_x(snext * SB);
        __builtin_amdgcn_sched_barrier(0);
        compute(s & 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
    }
    if (active) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const long row = r0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if constexpr (ACC64) out[row * KP + ct * 32 + j] = accd[ct][reg];
                else out[row * KP + ct * 32 + j] = (double)acc[ct][reg];
            }
    }
}

// row-local, float32 MFMA, wave-streaming with LDS-DMA staging (k <= 32).  The structure of
// k_row_local_f32_ws -- a block is W waves on one CU, every wave owns one 32-row tile and sweeps
// the columns -- with both operands brought in by `global_load_lds_dwordx4`: no staging registers
// (32 fewer than the register-staged kernel, which is what makes room for the float64 sums at four
// waves per SIMD), no ds_write instructions.  A wave-instruction writes 64 x 16 B = 1 KiB of LDS
// in lane order (a "piece"), so the XOR swizzle that keeps the fragment reads conflict free sits
// on the SOURCE address: lane l of a piece fetches the chunk whose swizzled position is l.
//   X: a tile is 32 rows x 32 columns = 4 pieces (8 rows x 128 B each); every wave owns a RING of
//      R = 8 pieces (one tile in flight per wave; longer rings measured no faster): tile t's pieces sit in ring
//      slots (4t + i) mod R, and R - 4 pieces of the tiles behind it are in flight while it is
//      multiplied (the register-staged kernel keeps 8 KB per wave in flight).
//   B: 64-column slabs (8 pieces: 4 components x 256 B each), two buffers shared by the block;
//      every wave issues one piece per slab (waves past the eighth repeat earlier pieces:
//      identical bytes).
// Every wave issues the same number of DMA instructions per step, so the waits are counted
// (`s_waitcnt vmcnt(N)`: hipcc does not track what lands in LDS; LDS-DMA data is ordered for a
// ds_read only by the issuing wave's covering vmcnt, plus a barrier for other waves' reads) and the
// block barrier is the raw s_barrier (a __syncthreads would drain the DMAs in flight).  The fp32
// accumulation chain ends after every tile (32 columns); the pieces are summed in float64 (see
// k_row_local_f32_ws).
// (ROW_LOCAL_RING, the X pieces in a wave's ring, is pass_plan.h's: the plan sizes the LDS by it and names the kernel)
__device__ __forceinline__ void dma16(const float *src, float *lds_uniform)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)lds_uniform, 16, 0, 0);
}

__global__ __launch_bounds__(1024) void k_row_local_f32_dma(const float *__restrict__ X, long ldx,
                                                            const float *__restrict__ B, int p_pad,
                                                            double *__restrict__ out, long n_pad, int W)
{
    constexpr int KP = 32, SB = 64, TC = 32, R = ROW_LOCAL_RING;
    extern __shared__ __attribute__((aligned(16))) float dma_smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    float *bs = dma_smem;                                   // [2][KP * SB]
    float *xs = dma_smem + 2 * KP * SB + wave * (R * 256);  // R pieces of 256 floats, wave-private
    const long r0 = ((long)blockIdx.x * W + wave) * 32;
    const bool active = r0 < n_pad;
    const long r0c = active ? r0 : n_pad - 32;
    const int h = lane >> 5, j = lane & 31;

    // X piece i of a tile (rows 8i .. 8i+7): lane -> row 8i + (lane >> 3), swizzled position lane & 7
    int xoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 8 * i + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);
        xoff[i] = (int)(row * ldx) + 4 * chunk;
    }
    const float *gx = X + r0c * ldx;
    // B piece of this wave: components 4 pb .. 4 pb + 3 of the slab, lane -> component 4 pb + (lane >> 4)
    const int pb = wave & 7;
    const int bcomp = 4 * pb + (lane >> 4);
    const int boff = bcomp * p_pad + 4 * ((lane & 15) ^ (bcomp & 15));
    const int ntile = p_pad / TC, nslab = p_pad / SB;
    int issued = 0;                                          // X pieces issued so far (uniform)
    auto issue_piece = [&]() {                               // next piece of the sweep into its ring slot
        int tl = issued >> 2;
        if (tl >= ntile) tl = ntile - 1;                     // past the end: harmless reloads
        const int i = issued & 3;
        const int slot = issued % R;
        const int off = i == 0 ? xoff[0] : (i == 1 ? xoff[1] : (i == 2 ? xoff[2] : xoff[3]));
        dma16(gx + off + tl * TC, xs + slot * 256);
        ++issued;
    };
    auto issue_b = [&](int sl, int buf) { dma16(B + boff + sl * SB, bs + buf * (KP * SB) + pb * 256); };

    // two fp32 accumulator sets, alternating tile by tile: the float64 flush of one set runs in the
    // shadow of the matrix instructions that fill the other (the flush needs the LAST instruction of
    // its chain to have retired: 16 passes)
    f32x16 acc0, acc1;
    double accd[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        acc0[e] = 0.f;
        acc1[e] = 0.f;
        accd[e] = 0.0;
    }
    auto tile_mfma = [&](int tl, f32x16 &acc) {
        const int s = tl >> 1, ts = tl & 1;
        if (ts == 0) {
            // pieces 4 tl .. 4 tl + 3 and (older) this wave's B(s) piece have landed when at most the
            // R - 4 younger X pieces are outstanding
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(R - 4) : "memory");
            __builtin_amdgcn_s_barrier();                    // all waves: B(s) complete, slab s-1 read
            issue_b(s + 1 < nslab ? s + 1 : s, (s + 1) & 1);
        } else {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(R - 3) : "memory");   // + the B piece issued one tile ago
        }
        const int base = (4 * tl) % R;                       // ring slot of this tile's first piece
        int slot = base + (j >> 3);
        slot = slot >= R ? slot - R : slot;
        const float *xb = xs + slot * 256 + (j & 7) * TC;
        const float *bb = bs + (s & 1) * (KP * SB) + j * SB;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pcx = ((2 * q + h) ^ ((j >> 1) & 7)) << 2;
            const int pcb = ((ts * 8 + 2 * q + h) ^ (j & 15)) << 2;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(xb + pcx);
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(bb + pcb);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bv[m], acc, 0, 0, 0);
        }
        // the four slots of this tile are free again (their reads were waited for before the MFMAs)
#pragma unroll
        for (int i = 0; i < 4; ++i) issue_piece();
    };
    auto flush = [&](f32x16 &acc) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            accd[e] += (double)acc[e];
            acc[e] = 0.f;
        }
    };

    issue_b(0, 0);
#pragma unroll
    for (int i = 0; i < R; ++i) issue_piece();
    for (int tl = 0; tl < ntile; tl += 2) {                  // p_pad is a multiple of 128: ntile is even
        tile_mfma(tl, acc0);
        flush(acc1);                                         // the previous tile's sums (zeros at tl = 0)
        tile_mfma(tl + 1, acc1);
        flush(acc0);
    }
    flush(acc1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the trailing reloads
    if (active) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long row = r0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            out[row * KP + j] = accd[reg];
        }
    }
}

// row-local, float64 VALU: block = 64 rows, X tile staged through LDS with coalesced
// loads; thread (row = t&63, q = t>>6) accumulates the components [q*KP/4, (q+1)*KP/4).
template <int KP>
__global__ __launch_bounds__(256) void k_row_local_f64(const double *__restrict__ X, long ldx,
                                                       const double *__restrict__ B, int p_pad,
                                                       double *__restrict__ out, long n_pad)
{
    constexpr int KQ = KP / 4;
    __shared__ double tile[64][65];
    const int t = threadIdx.x, row = t & 63, q = t >> 6;
    const long r0 = (long)blockIdx.x * 64;
    if (r0 >= n_pad) return;
    double acc[KQ];
#pragma unroll
    for (int i = 0; i < KQ; ++i) acc[i] = 0.0;
    for (int c0 = 0; c0 < p_pad; c0 += 64) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int idx = e * 256 + t;
            tile[idx >> 6][idx & 63] = X[(r0 + (idx >> 6)) * ldx + c0 + (idx & 63)];
        }
        __syncthreads();
        const double *bq = B + (long)(q * KQ) * p_pad + c0;
        for (int cc = 0; cc < 64; ++cc) {
            const double x = tile[row][cc];
#pragma unroll
            for (int i = 0; i < KQ; ++i) acc[i] = fma(x, bq[(long)i * p_pad + cc], acc[i]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < KQ; ++i) out[(r0 + row) * KP + q * KQ + i] = acc[i];
}

// rank-m correction of a reduce-over-rows result whose tall operand changed in m rows after
// the pass had read it (the QP's stragglers finish while Z'X is being accumulated):
//   extra[g][i][c] = sum over the slots s of slab g of (znew[s][i] - Z[rows[s]][i]) * X[rows[s]][c]
// written as G = gridDim.y further slabs of the split-row partials.  The slot count lives on
// the device; slab g takes the contiguous slot range [g*chunk, (g+1)*chunk).  Same MFMA
// mapping as k_reduce_rows_f32 (a wave owns a 128-column strip), with the rows gathered: a
// wave reads 64 row indices at a time (one coalesced load) and hands them out with
// ds_bpermute, so a step of 2*U slots costs one memory latency (X rows and z rows together).
__global__ __launch_bounds__(256) void k_reduce_rows_fixup_f32(const float *__restrict__ X, long ldx,
                                                               const unsigned int *__restrict__ count_dev,
                                                               const int *__restrict__ rows,
                                                               const double *__restrict__ zslot,
                                                               const double *__restrict__ Ztall,
                                                               int p_pad, float *__restrict__ extra)
{
    constexpr int KP = 32, U = 8;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c0 = (blockIdx.x * 4 + wave) * 128;
    if (c0 >= p_pad) return;   // wave-uniform; the kernel has no barriers
    const int h = lane >> 5, j = lane & 31;
    const long count = (long)*count_dev, G = gridDim.y;
    long chunk = (count + G - 1) / G;
    chunk = (chunk + 2 * U - 1) / (2 * U) * (2 * U);
    const long s_begin = (long)blockIdx.y * chunk;
    long s_end = s_begin + chunk;
    if (s_end > count) s_end = count;

    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;

    for (long b = s_begin; b < s_end; b += 64) {
        const int mine = (b + lane < s_end) ? rows[b + lane] : 0;
        for (int q = 0; q < 64 && b + q < s_end; q += 2 * U) {
            f32x4 xv[U];
            float av[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int sl = q + 2 * u + h;                 // slot of this lane's half
                const long slot = b + sl;
                const bool valid = slot < s_end;
                const long row = __shfl(mine, sl & 63, 64);   // 0 for slots past the end
                xv[u] = *reinterpret_cast<const f32x4 *>(X + row * ldx + c0 + 4 * j);
                av[u] = valid ? (float)(zslot[slot * KP + j] - Ztall[row * KP + j]) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], xv[u][m], acc[m], 0, 0, 0);
        }
    }
    float *out = extra + (size_t)blockIdx.y * KP * p_pad;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int comp = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        f32x4 v = {acc[0][reg], acc[1][reg], acc[2][reg], acc[3][reg]};
        *reinterpret_cast<f32x4 *>(out + (size_t)comp * p_pad + c0 + 4 * j) = v;
    }
}

// ---------------------------------------------------------------------------
// reduce over rows for a tall operand that is zero in almost all of its rows (the SPG direction of
// the dictionary update: about 200 non-zero rows of 100 000).  k_group_flags (kernels_tall.hip) has
// written one byte per aligned group of 4 rows: 1 if any entry of the group compares != 0.0.  The
// gather kernels below run on the grid of their dense twins, with the same block map and strip
// ownership, and write the same block of `partial`; a wave issues, for every FLAGGED group of its
// slab in ascending order, exactly the MFMA steps the dense kernel issues for those four rows (same
// lane-to-row mapping, same conversion of the tall operand).  The steps left out have a tall operand
// of +-0 in every lane: for finite X they add exact zeros to accumulators that never hold -0 (they
// start at +0, and x + (-0) = x), so every accumulator chain sees the same sequence of non-trivial
// steps on the same operands and ends in the same bits, whatever the matrix core does inside a step.
// A slab with more than `limit` flagged groups is left to the gated dense launch that follows
// (slab_mode[slab] = 0); the decision is taken per slab on the device, by every wave of the slab
// alike, and recorded by wave 0 of column group 0 together with the two counters
// counters[0] (slabs gathered) and counters[1] (slabs left to the dense kernel).
// ---------------------------------------------------------------------------
constexpr int GATHER_CHUNK = 512;   // groups per round of flag bytes: 8 per lane, one 8-byte load

// bit b: group g0 + 8 * lane + b of the slab is flagged (ngroups and g0 are multiples of 8)
__device__ __forceinline__ unsigned gather_flag_mask(const unsigned char *__restrict__ fl, int g0,
                                                     int ngroups, int lane)
{
    const int g = g0 + 8 * lane;
    if (g >= ngroups) return 0u;
    const uint2 w = *reinterpret_cast<const uint2 *>(fl + g);
    unsigned m = 0u;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const unsigned byte = ((b < 4 ? w.x : w.y) >> (8 * (b & 3))) & 0xffu;
        m |= (byte != 0u ? 1u : 0u) << b;
    }
    return m;
}

// Number of flagged groups of the slab (the same value in every lane); m0 = the mask of the first
// round, which the walk reuses.
__device__ __forceinline__ int gather_count(const unsigned char *__restrict__ fl, int ngroups, int lane,
                                            unsigned &m0)
{
    m0 = gather_flag_mask(fl, 0, ngroups, lane);
    int cnt = __popc(m0);
    for (int g0 = GATHER_CHUNK; g0 < ngroups; g0 += GATHER_CHUNK)
        cnt += __popc(gather_flag_mask(fl, g0, ngroups, lane));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    return cnt;
}

// The flagged groups of one round, in ascending order, into the wave's list (offsets from g0 in
// groups); returns how many.  The list is private to the wave: LDS operations of a wave complete in
// order, so no barrier is needed around it.
__device__ __forceinline__ int gather_list(unsigned m, int lane, unsigned short *list)
{
    const int c = __popc(m);
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    const int total = __shfl(incl, 63, 64);
    int o = incl - c;
    while (m) {
        const int b = __ffs((int)m) - 1;
        list[o++] = (unsigned short)(8 * lane + b);
        m &= m - 1u;
    }
    __builtin_amdgcn_wave_barrier();
    return total;
}

// NG flagged groups of k_reduce_rows_gather_f32: the 2 * NG loads first, then their MFMA steps in
// ascending row order -- per group the two steps (rows 4g + {0,1} and 4g + {2,3}) of the dense kernel
template <int NCT, int NG>
__device__ __forceinline__ void gather_groups_f32(const float *__restrict__ xp, long ldx,
                                                  const double *__restrict__ ap, const long *rows,
                                                  f32x16 (&acc)[NCT][4])
{
    constexpr int KP = 32 * NCT;
    f32x4 xv[NG][2];
    double av[NG][2][NCT];
#pragma unroll
    for (int t = 0; t < NG; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const long row = rows[t] + 2 * s;
            xv[t][s] = *reinterpret_cast<const f32x4 *>(xp + row * ldx);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) av[t][s][ct] = ap[row * KP + ct * 32];
        }
#pragma unroll
    for (int t = 0; t < NG; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const float af = (float)av[t][s][ct];
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc[ct][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, xv[t][s][m], acc[ct][m], 0, 0, 0);
            }
}

template <int NCT>
__global__ __launch_bounds__(256) void k_reduce_rows_gather_f32(const float *__restrict__ X, long ldx,
                                                                const double *__restrict__ A,
                                                                long rows_per_slab, long n_pad, int p_pad,
                                                                float *__restrict__ partial,
                                                                const unsigned char *__restrict__ flags,
                                                                int limit, unsigned char *__restrict__ slab_mode,
                                                                unsigned int *__restrict__ counters)
{
    constexpr int KP = 32 * NCT, NG = 4;
    __shared__ unsigned short lists[4][GATHER_CHUNK];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int colgroup, slab;
    xcd_aware_block(colgroup, slab);
    const int c0 = (colgroup * 4 + wave) * 128;
    if (c0 >= p_pad) return;   // wave-uniform; the kernel has no barriers
    const int h = lane >> 5, j = lane & 31;
    const long r_begin = (long)slab * rows_per_slab;
    long r_end = r_begin + rows_per_slab;
    if (r_end > n_pad) r_end = n_pad;
    const int ngroups = (int)((r_end - r_begin) >> 2);       // a multiple of 8
    const unsigned char *fl = flags + (r_begin >> 2);

    unsigned m0;
    const int cnt = gather_count(fl, ngroups, lane, m0);
    const bool take = cnt <= limit;
    if (colgroup == 0 && wave == 0 && lane == 0) {
        slab_mode[slab] = take ? 1 : 0;
        atomicAdd(counters + (take ? 0 : 1), 1u);
    }
    if (!take) return;         // the gated dense launch serves this slab

    f32x16 acc[NCT][4];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ct][m][e] = 0.f;

    const float *xp = X + (r_begin + h) * ldx + c0 + 4 * j;
    const double *ap = A + (r_begin + h) * KP + j;
    unsigned short *list = lists[wave];
    if (cnt > 0)
        for (int g0 = 0; g0 < ngroups; g0 += GATHER_CHUNK) {
            const int total = gather_list(g0 == 0 ? m0 : gather_flag_mask(fl, g0, ngroups, lane), lane, list);
            int q = 0;
            long rows[NG];
            for (; q + NG <= total; q += NG) {
#pragma unroll
                for (int t = 0; t < NG; ++t)
                    rows[t] = 4L * (g0 + __builtin_amdgcn_readfirstlane((int)list[q + t]));
                gather_groups_f32<NCT, NG>(xp, ldx, ap, rows, acc);
            }
            for (; q < total; ++q) {
                rows[0] = 4L * (g0 + __builtin_amdgcn_readfirstlane((int)list[q]));
                gather_groups_f32<NCT, 1>(xp, ldx, ap, rows, acc);
            }
            __builtin_amdgcn_wave_barrier();   // the next round overwrites the list
        }

    float *out = partial + (size_t)slab * KP * p_pad;      // as in k_reduce_rows_f32
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int comp = ct * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            f32x4 v = {acc[ct][0][reg], acc[ct][1][reg], acc[ct][2][reg], acc[ct][3][reg]};
            *reinterpret_cast<f32x4 *>(out + (size_t)comp * p_pad + c0 + 4 * j) = v;
        }
}

// NG flagged groups of k_reduce_rows_gather_f64_mfma: one MFMA step of the dense kernel per group
template <int NT, int NG>
__device__ __forceinline__ void gather_groups_f64(const double *__restrict__ xp, long ldx,
                                                  const double *__restrict__ ap, const long *rows,
                                                  f64x4g (&acc)[NT][2][2])
{
    constexpr int KP = 16 * NT;
    f64x2g xv[NG][2];
    double av[NG][NT];
#pragma unroll
    for (int t = 0; t < NG; ++t) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
            xv[t][u] = *reinterpret_cast<const f64x2g *>(xp + rows[t] * ldx + 32 * u);
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) av[t][ti] = ap[rows[t] * KP + 16 * ti];
    }
#pragma unroll
    for (int t = 0; t < NG; ++t)
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    acc[ti][u][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t][ti], xv[t][u][e], acc[ti][u][e],
                                                                         0, 0, 0);
}

template <int NT>
__global__ __launch_bounds__(256) void k_reduce_rows_gather_f64_mfma(const double *__restrict__ X, long ldx,
                                                                     const double *__restrict__ A,
                                                                     long rows_per_slab, long n_pad, int p_pad,
                                                                     double *__restrict__ partial,
                                                                     const unsigned char *__restrict__ flags,
                                                                     int limit,
                                                                     unsigned char *__restrict__ slab_mode,
                                                                     unsigned int *__restrict__ counters)
{
    constexpr int KP = 16 * NT, NG = 4;
    __shared__ unsigned short lists[4][GATHER_CHUNK];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int colgroup, slab;
    xcd_aware_block(colgroup, slab);
    const int c0 = (colgroup * 4 + wave) * 64;
    if (c0 >= p_pad) return;   // wave-uniform; the kernel has no barriers
    const int lc = lane & 15, lr = lane >> 4;
    const long r_begin = (long)slab * rows_per_slab;
    long r_end = r_begin + rows_per_slab;
    if (r_end > n_pad) r_end = n_pad;
    const int ngroups = (int)((r_end - r_begin) >> 2);       // a multiple of 8
    const unsigned char *fl = flags + (r_begin >> 2);

    unsigned m0;
    const int cnt = gather_count(fl, ngroups, lane, m0);
    const bool take = cnt <= limit;
    if (colgroup == 0 && wave == 0 && lane == 0) {
        slab_mode[slab] = take ? 1 : 0;
        atomicAdd(counters + (take ? 0 : 1), 1u);
    }
    if (!take) return;         // the gated dense launch serves this slab

    f64x4g acc[NT][2][2];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 2; ++e) acc[ti][u][e] = (f64x4g){0.0, 0.0, 0.0, 0.0};

    const double *xp = X + (r_begin + lr) * ldx + c0 + 2 * lc;
    const double *ap = A + (r_begin + lr) * KP + lc;
    unsigned short *list = lists[wave];
    if (cnt > 0)
        for (int g0 = 0; g0 < ngroups; g0 += GATHER_CHUNK) {
            const int total = gather_list(g0 == 0 ? m0 : gather_flag_mask(fl, g0, ngroups, lane), lane, list);
            int q = 0;
            long rows[NG];
            for (; q + NG <= total; q += NG) {
#pragma unroll
                for (int t = 0; t < NG; ++t)
                    rows[t] = 4L * (g0 + __builtin_amdgcn_readfirstlane((int)list[q + t]));
                gather_groups_f64<NT, NG>(xp, ldx, ap, rows, acc);
            }
            for (; q < total; ++q) {
                rows[0] = 4L * (g0 + __builtin_amdgcn_readfirstlane((int)list[q]));
                gather_groups_f64<NT, 1>(xp, ldx, ap, rows, acc);
            }
            __builtin_amdgcn_wave_barrier();   // the next round overwrites the list
        }

    double *out = partial + (size_t)slab * KP * p_pad;     // as in k_reduce_rows_f64_mfma
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int comp = 16 * ti + lr + 4 * reg;
                f64x2g v = {acc[ti][u][0][reg], acc[ti][u][1][reg]};
                *reinterpret_cast<f64x2g *>(out + (size_t)comp * p_pad + c0 + 32 * u + 2 * lc) = v;
            }
}

// measurement only: stream X once with 16-byte loads, no arithmetic to speak of -- the
// read bandwidth the memory system delivers to a kernel of this shape (aa_time_kernel 2)
template <int UNROLL>
__global__ __launch_bounds__(256) void k_stream_probe(const f32x4 *__restrict__ x, long n16,
                                                      float *__restrict__ sink)
{
    const long stride = (long)gridDim.x * 256;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (; i + (UNROLL - 1) * stride < n16; i += UNROLL * stride) {
        f32x4 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) v[u] = x[i + u * stride];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) acc += v[u];
    }
    for (; i < n16; i += stride) acc += x[i];
    if (acc[0] + acc[1] + acc[2] + acc[3] == 123.456f) sink[0] = 1.f;   // keeps the loads alive
}

// the load pattern of k_row_local_f32_ws without its LDS / MFMA work: a wave owns 32 rows and
// walks the columns in 64-column tiles (TILED = false: 32 pieces of 256 B, 16 KB apart, per
// tile, as in the row-major matrix; TILED = true: the same bytes as one contiguous 8 KB chunk,
// i.e. what a [32 x 64]-tiled storage of X would give)
template <bool TILED>
__global__ __launch_bounds__(832) void k_stream_probe_rows(const float *__restrict__ X, long ldx,
                                                           long n_pad, int p_pad,
                                                           float *__restrict__ sink)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long r0 = ((long)blockIdx.x * 13 + wave) * 32;
    if (r0 >= n_pad) return;
    const int xr = lane >> 4, xc = lane & 15;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < p_pad; c0 += 128) {
        f32x4 v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tile = e >> 3, ee = e & 7;
            const long off = TILED ? (r0 * ldx + (long)(c0 / 64 + tile) * 2048 + (4 * ee + xr) * 64 + 4 * xc)
                                   : ((r0 + 4 * ee + xr) * ldx + c0 + 64 * tile + 4 * xc);
            v[e] = *reinterpret_cast<const f32x4 *>(X + off);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc += v[e];
    }
    if (acc[0] + acc[1] + acc[2] + acc[3] == 123.456f) sink[0] = 1.f;
}

// variant: 0 = 4 loads in flight per thread x 4096 blocks; 1 = 8 x 2048; 2 = 16 x 1024; 3 = 8 x 8192
int launch_stream_probe(Ctx *c, int variant)
{
    const long bytes = (long)c->n_pad * c->p_pad * (c->dtype == AA_F32 ? 4 : 8);
    const f32x4 *x = reinterpret_cast<const f32x4 *>(c->X.p);
    float *sink = c->partial.as<float>();
    const long tiles = c->n_pad / 32;
    switch (variant) {
        case 4: hipLaunchKernelGGL(k_stream_probe_rows<false>, dim3((unsigned)((tiles + 12) / 13)), dim3(832), 0, c->stream, c->X.as<float>(), c->p_pad, c->n_pad, (int)c->p_pad, sink); break;
        case 5: hipLaunchKernelGGL(k_stream_probe_rows<true>, dim3((unsigned)((tiles + 12) / 13)), dim3(832), 0, c->stream, c->X.as<float>(), c->p_pad, c->n_pad, (int)c->p_pad, sink); break;
        case 1: hipLaunchKernelGGL(k_stream_probe<8>, dim3(2048), dim3(256), 0, c->stream, x, bytes / 16, sink); break;
        case 2: hipLaunchKernelGGL(k_stream_probe<16>, dim3(1024), dim3(256), 0, c->stream, x, bytes / 16, sink); break;
        case 3: hipLaunchKernelGGL(k_stream_probe<8>, dim3(8192), dim3(256), 0, c->stream, x, bytes / 16, sink); break;
        default: hipLaunchKernelGGL(k_stream_probe<4>, dim3(4096), dim3(256), 0, c->stream, x, bytes / 16, sink); break;
    }
    AA_CHECK_HIP(hipGetLastError());
    return AA_OK;
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
static void gemm_event(Ctx *c, int which)
{
    if (!c->time_gemm) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) == hipSuccess) {
        (void)hipEventRecord(e, c->stream);
        c->gemmEvents[which].push_back(e);
    }
}

// The reduce-over-rows kernels on element type T (float32; float64 on the matrix cores) share two signatures: the
// dense kernel, gated by a mode byte per slab when it runs behind its gather twin, and the gather kernel.
template <typename T>
using ReduceRowsFn = void (*)(const T *, long, const double *, long, long, int, T *, const unsigned char *);
template <typename T>
struct ReduceRowsGather {
    void (*gather)(const T *, long, const double *, long, long, int, T *, const unsigned char *, int, unsigned char *,
                   unsigned int *);
    ReduceRowsFn<T> gated;
};

template <typename T>
static void reduce_rows_dense(Ctx *c, const ReduceRowsPlan &pl, ReduceRowsFn<T> dense, const double *A_tall,
                              const unsigned char *mode)
{
    hipLaunchKernelGGL(dense, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3(256), 0, c->stream, c->X.as<T>(),
                       c->p_pad, A_tall, c->rows_per_slab, c->n_pad, (int)c->p_pad, c->partial.as<T>(), mode);
}

// The flagged sequence: group flags of the tall operand -> gather kernel -> gated dense kernel.
// Three launches with the per-slab decision on the device: nothing here waits for the device, and
// the sequence can be captured in a graph.
template <typename T>
static int reduce_rows_flagged(Ctx *c, const ReduceRowsPlan &pl, const ReduceRowsGather<T> &k, const double *A_tall,
                               DevBuf *flag_buf)
{
    unsigned char *flags = flag_buf->as<unsigned char>();
    unsigned char *mode = c->slabMode.as<unsigned char>();
    unsigned int *counters = reinterpret_cast<unsigned int *>(mode + AA_SLAB_MODE_BYTES);
    AA_CHECK(launch_group_flags(c, A_tall, flags, counters));
    hipLaunchKernelGGL(k.gather, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3(256), 0, c->stream, c->X.as<T>(),
                       c->p_pad, A_tall, c->rows_per_slab, c->n_pad, (int)c->p_pad, c->partial.as<T>(),
                       (const unsigned char *)flags, (int)pl.gather_limit, mode, counters);
    reduce_rows_dense<T>(c, pl, k.gated, A_tall, mode);
    return AA_OK;
}

int launch_reduce_rows(Ctx *c, const double *A_tall, double *out_wide, void *outT, bool main_only,
                       DevBuf *flag_buf)
{
    // every instantiation, [KP == 64]
    static const ReduceRowsGather<float> gather32[2] = {{k_reduce_rows_gather_f32<1>, k_reduce_rows_f32<1, 4, true>},
                                                        {k_reduce_rows_gather_f32<2>, k_reduce_rows_f32<2, 4, true>}};
    static const ReduceRowsGather<double> gather64[2] = {
        {k_reduce_rows_gather_f64_mfma<2>, k_reduce_rows_f64_mfma<2, true>},
        {k_reduce_rows_gather_f64_mfma<4>, k_reduce_rows_f64_mfma<4, true>}};
    static const ReduceRowsFn<float> dense32[2] = {k_reduce_rows_f32<1, 4>, k_reduce_rows_f32<2, 4>};
    static const ReduceRowsFn<double> dense64[2] = {k_reduce_rows_f64_mfma<2>, k_reduce_rows_f64_mfma<4>};
    static void (*const valu[2])(const double *, long, const double *, long, long, int, double *) = {
        k_reduce_rows_f64<32>, k_reduce_rows_f64<64>};

    const ReduceRowsPlan pl = reduce_rows_plan(
        pass_knobs(), ReduceRowsIn{c->dtype == AA_F32, c->KP, c->p_pad, c->nslab, c->rows_per_slab, flag_buf != nullptr,
                                   c->time_gemm});
    const int kp64 = c->KP == 64;
    pass_name(pl, c->pass_names[0], sizeof(c->pass_names[0]));
    if (!pl.flagged) gemm_event(c, 0);
    switch (pl.family) {
        case ReduceRowsFamily::f32:
            if (pl.flagged) AA_CHECK(reduce_rows_flagged<float>(c, pl, gather32[kp64], A_tall, flag_buf));
            else reduce_rows_dense<float>(c, pl, dense32[kp64], A_tall, nullptr);
            break;
        case ReduceRowsFamily::f64_mfma:
            if (pl.flagged) AA_CHECK(reduce_rows_flagged<double>(c, pl, gather64[kp64], A_tall, flag_buf));
            else reduce_rows_dense<double>(c, pl, dense64[kp64], A_tall, nullptr);
            break;
        case ReduceRowsFamily::f64_valu:                    // (no gather twin: the plan never flags it)
            hipLaunchKernelGGL(valu[kp64], dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3(256), 0, c->stream,
                               c->X.as<double>(), c->p_pad, A_tall, c->rows_per_slab, c->n_pad, (int)c->p_pad,
                               c->partial.as<double>());
            break;
    }
    AA_CHECK_HIP(hipGetLastError());
    if (!pl.flagged) gemm_event(c, 0);
    if (main_only) return AA_OK;
    return launch_reduce_rows_finish(c, out_wide, outT, 0);
}

int launch_reduce_rows_finish(Ctx *c, double *out_wide, void *outT, int extra_slabs)
{
    const long elems = (long)c->KP * c->p_pad;
    const long slabs = c->nslab + extra_slabs;
    dim3 block(256), grid((unsigned)((elems + 255) / 256));
    if (c->dtype == AA_F32) {
        float *oT = ((c->world > 1 || c->force_comm)) ? nullptr : reinterpret_cast<float *>(outT);
        hipLaunchKernelGGL((k_reduce_partials<float, float>), grid, block, 0, c->stream,
                           (const float *)c->partial.as<float>(), slabs, elems, out_wide, oT);
    } else {
        double *oT = ((c->world > 1 || c->force_comm) || outT == (void *)out_wide) ? nullptr
                                                                : reinterpret_cast<double *>(outT);
        hipLaunchKernelGGL((k_reduce_partials<double, double>), grid, block, 0, c->stream,
                           (const double *)c->partial.as<double>(), slabs, elems, out_wide, oT);
    }
    AA_CHECK_HIP(hipGetLastError());
    if ((c->world > 1 || c->force_comm)) {
        // riders in the buffer's tail (Ctx::ride*): one all-reduce for the lot
        double *tail = out_wide + elems;
        long extra = 0;
        if (c->ride_dst == tail) extra = c->ride_count;
        if (c->ride.on) {
            AA_REQUIRE(c->ride.gather >= tail && c->ride.gather + c->ride.count <= tail + AA_WIDE_TAIL(c->KP), AA_ERR_STATE,
                       "a reduction was left waiting for an all-reduce that did not come");
            const long end = (long)(c->ride.gather - tail) + c->ride.count;
            if (end > extra) extra = end;
        }
        AA_CHECK(comm_allreduce(c, out_wide, elems + extra, 0));
        if (c->ride.on) AA_CHECK(launch_ride_post(c, &c->ride, c->ride.gather));
        c->ride_dst = nullptr;
        c->ride_count = 0;
        if (outT && outT != (void *)out_wide) AA_CHECK(launch_wide_to_T(c, out_wide, outT));
    }
    return AA_OK;
}

int launch_reduce_rows_fixup(Ctx *c, const unsigned int *count_dev, const int *rows_dev,
                             const double *zslot, const double *Ztall)
{
    AA_REQUIRE(c->KP == 32 && c->dtype == AA_F32, AA_ERR_STATE, "tail fix-up: float32 data, k <= 32");
    const size_t slab_elems = (size_t)c->KP * c->p_pad;
    dim3 grid((unsigned)((c->p_pad + 511) / 512), QP_FIX_SLABS), block(256);
    hipLaunchKernelGGL(k_reduce_rows_fixup_f32, grid, block, 0, c->stream, c->X.as<float>(), c->p_pad,
                       count_dev, rows_dev, zslot, Ztall, (int)c->p_pad,
                       c->partial.as<float>() + (size_t)c->nslab * slab_elems);
    AA_CHECK_HIP(hipGetLastError());
    return AA_OK;
}

// ---------------------------------------------------------------------------
// Implicit RBF kernel (archetypal_analysis.py:673-910 with K never formed):
//   out[r][i] = sum_c exp(-gamma ||x_r - x_c||^2) V[c][i]        (V, out tall [n_pad][KP], float64)
// Both pass shapes of the kernel form reduce to this product (K is symmetric: C K = (K C')').  A block
// owns 64 rows and walks over 64-column tiles of K: S = X_R X_C' through LDS in chunks of 16 features
// (a thread holds a 4 x 4 patch), E = exp(-gamma max(|x_r|^2 + |x_c|^2 - 2 S, 0)) goes to LDS, then
// out_R += E V_C (a thread holds KP / 4 components of one row).  float64 VALU throughout: the
// per-sample QPs behind it need a float64 gradient.  n^2 (2 p + 2 KP) flop per
// product: for n up to a few ten thousand; grid.y splits the columns so that the chip is full.
// ---------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void k_rbf_kv(const double *__restrict__ F, long ldf, int pf,
                                                const double *__restrict__ nrm, double gamma,
                                                const double *__restrict__ V, long n, long n_pad,
                                                long tiles_per_split, double *__restrict__ out)
{
    constexpr int PC = 16, CPT = KP / 4;
    extern __shared__ __attribute__((aligned(16))) double rbf_smem[];     // 67 KB (KP = 32) / 83 KB (KP = 64)
    double (*es)[65] = reinterpret_cast<double (*)[65]>(rbf_smem);
    double (*vs)[KP] = reinterpret_cast<double (*)[KP]>(rbf_smem + 64 * 65);
    double (*xr)[PC + 1] = reinterpret_cast<double (*)[PC + 1]>(rbf_smem + 64 * 65 + 64 * KP);
    double (*xc)[PC + 1] = reinterpret_cast<double (*)[PC + 1]>(rbf_smem + 64 * 65 + 64 * KP + 64 * (PC + 1));
    const int t = threadIdx.x;
    const long r0 = (long)blockIdx.x * 64;
    const int tr = t >> 4, tc = t & 15;                  // 4 x 4 patch of S
    const int orow = t >> 2, oc0 = (t & 3) * CPT;        // one row, CPT components of the output
    double acc[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) acc[i] = 0.0;
    const long ntile = n_pad / 64;
    long ct0 = (long)blockIdx.y * tiles_per_split, ct1 = ct0 + tiles_per_split;
    if (ct1 > ntile) ct1 = ntile;
    for (long ct = ct0; ct < ct1; ++ct) {
        const long c0 = ct * 64;
        if (c0 >= n) break;                              // columns past n carry zero rows of V
        double sv[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) sv[a][b] = 0.0;
        for (int q0 = 0; q0 < pf; q0 += PC) {
            __syncthreads();
            for (int e = t; e < 64 * PC; e += 256) {
                const int rr = e / PC, qq = e % PC;
                const bool ok = q0 + qq < pf;
                xr[rr][qq] = ok ? F[(r0 + rr) * ldf + q0 + qq] : 0.0;      // rows < n_pad exist (zero padded)
                xc[rr][qq] = ok ? F[(c0 + rr) * ldf + q0 + qq] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int qq = 0; qq < PC; ++qq) {
                double ra[4], cb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) ra[a] = xr[4 * tr + a][qq];
#pragma unroll
                for (int b = 0; b < 4; ++b) cb[b] = xc[4 * tc + b][qq];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) sv[a][b] = fma(ra[a], cb[b], sv[a][b]);
            }
        }
        __syncthreads();                                 // the previous tile's E and V have been consumed
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long r = r0 + 4 * tr + a, cc = c0 + 4 * tc + b;
                const double d2 = fmax(nrm[r] + nrm[cc] - 2.0 * sv[a][b], 0.0);
                es[4 * tr + a][4 * tc + b] = (r == cc) ? 1.0 : exp(-gamma * d2);
            }
        for (int e = t; e < 64 * KP; e += 256) vs[e / KP][e % KP] = V[(c0 + e / KP) * KP + e % KP];
        __syncthreads();
        for (int cc = 0; cc < 64; ++cc) {
            const double ev = es[orow][cc];
#pragma unroll
            for (int i = 0; i < CPT; ++i) acc[i] = fma(ev, vs[cc][oc0 + i], acc[i]);
        }
    }
    double *dst = out + (size_t)blockIdx.y * n_pad * KP;
    const long r = r0 + orow;
#pragma unroll
    for (int i = 0; i < CPT; ++i) dst[r * KP + oc0 + i] = r < n ? acc[i] : 0.0;     // padding rows stay zero
}

__global__ __launch_bounds__(256) void k_rbf_norms(const double *__restrict__ F, long ldf, int pf, long n_pad,
                                                   double *__restrict__ nrm)
{
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_pad) return;
    double s = 0.0;
    for (int q = 0; q < pf; ++q) s = fma(F[r * ldf + q], F[r * ldf + q], s);
    nrm[r] = s;
}

// ---------------------------------------------------------------------------
// Cross RBF product of KernelAA.transform (archetypal_analysis.py:1151-1199 in kernel form):
//   out[r][i] = sum_c exp(-gamma max(|y_r|^2 + |x_c|^2 - 2 y_r.x_c, 0)) V[c][i]
// for the rows y_r of the resident data matrix Y ([n_pad][ld], the rows of the new samples) against a
// reference set X_S ([s_pad][ld], the training rows in the support of the dictionary) and V = D'
// restricted to them ([s_pad][KP]).  Both products run on v_mfma_f64_16x16x4_f64 (operand / result maps
// at the head of the f64 section above).  A block owns 64 rows of Y, a wave 16 of them, and walks over
// 64-column tiles of X_S:
//   * S' = X_C Y_R' with the column index c as the MFMA row (A = X_C, B = Y_R, both staged through LDS
//     in 32-feature chunks): lane l, reg q holds S[r = l&15][c = 16 mt + (l>>4) + 4 q];
//   * that is the A-operand map of the second product (row r = l&15, contraction index c = l>>4 in the
//     k-step (mt, q)), so E = exp(...) is formed in the registers it was computed in and
//     out_R += E V_C is one MFMA per k-step and 16-component tile, with no LDS round trip of E.
// Rows and columns are different sets: no diagonal shortcut.  Padding columns (c >= s) have zero rows
// of V, padding rows (r >= m) are written as zeros.  grid.y splits the column tiles; the splits are
// summed in a fixed order by k_sum_chunks, so the result is deterministic.
// m s (2 p + 2 KP) flop (p rounded up to 4, s to 64, KP = 32 / 64).  The 32-feature chunks are read from
// the zero-padded rows (ld = p rounded up to 128); the MFMAs stop at p rounded up to 4.
// ---------------------------------------------------------------------------
// The element-wise step is a functor of the dot product s and the two squared norms; the tile body is shared
// by the RBF cross product and the polynomial products below (k_poly_kv_mfma).
struct RbfTile {
    static constexpr bool needs_norms = true;
    double gamma;
    __device__ __forceinline__ double operator()(double s, double nyr, double nsc) const
    {
        const double d2 = fmax(nyr + nsc - 2.0 * s, 0.0);
        return exp(-gamma * d2);
    }
};
struct PolyTile {
    static constexpr bool needs_norms = false;
    PolyKernel pk;
    __device__ __forceinline__ double operator()(double s, double, double) const { return poly_kappa(s, pk); }
};

template <int KP, class Fn>
__device__ __forceinline__ void kernel_tile_product(const double *__restrict__ Y, const double *__restrict__ ny,
                                                    const double *__restrict__ XS, const double *__restrict__ ns,
                                                    const double *__restrict__ V, long ld, int pk, long m,
                                                    long m_pad, long s_tiles, long tiles_per_split, const Fn fn,
                                                    double *__restrict__ out)
{
    constexpr int NT = KP / 16, TC = 32, LS = 34, VS = KP + 16;
    __shared__ __attribute__((aligned(16))) double ys[64 * LS];
    __shared__ __attribute__((aligned(16))) double xs[64 * LS];
    __shared__ __attribute__((aligned(16))) double vs[64 * VS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int lc = lane & 15, lr = lane >> 4;
    const long r0 = (long)blockIdx.x * 64;                // grid.x = m_pad / 64 exactly
    double nyr = 0.0;                                     // |y_r|^2 of the row this lane's S values belong to
    if constexpr (Fn::needs_norms) nyr = ny[r0 + 16 * wave + lc];
    f64x4g o[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) o[nt] = (f64x4g){0.0, 0.0, 0.0, 0.0};

    long ct0 = (long)blockIdx.y * tiles_per_split, ct1 = ct0 + tiles_per_split;
    if (ct1 > s_tiles) ct1 = s_tiles;
    for (long ct = ct0; ct < ct1; ++ct) {
        const long c0 = ct * 64;
        f64x4g sacc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) sacc[mt] = (f64x4g){0.0, 0.0, 0.0, 0.0};
        for (int q0 = 0; q0 < pk; q0 += TC) {
            __syncthreads();                              // the previous chunk has been read
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int cid = t + 256 * e, row = cid >> 4, col = 2 * (cid & 15);
                *reinterpret_cast<f64x2g *>(ys + row * LS + col) =
                    *reinterpret_cast<const f64x2g *>(Y + (r0 + row) * ld + q0 + col);
                *reinterpret_cast<f64x2g *>(xs + row * LS + col) =
                    *reinterpret_cast<const f64x2g *>(XS + (c0 + row) * ld + q0 + col);
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < TC / 4; ++s) {
                if (q0 + 4 * s >= pk) break;              // block-uniform: the last chunk ends at p rounded up to 4
                const double b = ys[(16 * wave + lc) * LS + 4 * s + lr];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    sacc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[(16 * mt + lc) * LS + 4 * s + lr], b, sacc[mt],
                                                                    0, 0, 0);
            }
        }
        // the V rows of this tile (vs was last read before the barriers of the chunk loop)
        for (int e = t; e < 64 * KP; e += 256) vs[(e / KP) * VS + e % KP] = V[(c0 + e / KP) * KP + e % KP];
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cl = 16 * mt + lr + 4 * q;      // column of the tile this lane's value belongs to
                double nsc = 0.0;
                if constexpr (Fn::needs_norms) nsc = ns[c0 + cl];
                const double ev = fn(sacc[mt][q], nyr, nsc);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    o[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ev, vs[cl * VS + 16 * nt + lc], o[nt], 0, 0, 0);
            }
    }
    double *dst = out + (size_t)blockIdx.y * m_pad * KP;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long r = r0 + 16 * wave + lr + 4 * q;
            dst[r * KP + 16 * nt + lc] = r < m ? o[nt][q] : 0.0;
        }
}

template <int KP>
__global__ __launch_bounds__(256) void k_rbf_cross_mfma(const double *__restrict__ Y, const double *__restrict__ ny,
                                                        const double *__restrict__ XS, const double *__restrict__ ns,
                                                        const double *__restrict__ V, long ld, int pk, long m,
                                                        long m_pad, long s_tiles, long tiles_per_split, double gamma,
                                                        double *__restrict__ out)
{
    kernel_tile_product<KP>(Y, ny, XS, ns, V, ld, pk, m, m_pad, s_tiles, tiles_per_split, RbfTile{gamma}, out);
}

// ---------------------------------------------------------------------------
// Implicit polynomial kernel kappa(x, y) = (gamma x.y + coef0)^degree (poly_kappa, aa_internal.h), K never
// formed:   out[r][i] = sum_c kappa(y_r, x_c) V[c][i]
// on the tile body above, both contractions on v_mfma_f64_16x16x4_f64 and kappa(S) formed in the registers S
// was computed in.  One kernel serves both products:
//   * the fit (kernel_kv): Y = X_S = the features of aa_set_poly_features ([n_pad][feat_ld], feat_ld =
//     p rounded up to 32, so that the last 32-feature chunk of a row stays inside the row; zero padded),
//     V = C' or Z.  Rows and columns are the same set and the diagonal is simply what the tile computes;
//   * KernelAA.transform (kernel_cross): Y = the resident rows, X_S = the reference rows, ld = p_pad.
// No norms are read.  Padding columns have zero rows of V (a padding column's kappa is coef0^degree, times
// zero); padding rows are written as zeros.  n^2 (2 p + 2 KP) flop (p rounded up to 4, n to 64).
// Per block: 64 x 34 doubles of Y and of X_S and 64 x (KP + 16) of V in LDS (58 KB at KP = 32, 74 KB at 64);
// per lane 16 accumulators of S and KP / 4 of the output (180 / 184 VGPRs, no spills).
// ---------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void k_poly_kv_mfma(const double *__restrict__ Y, const double *__restrict__ XS,
                                                      const double *__restrict__ V, long ld, int pk, long m,
                                                      long m_pad, long s_tiles, long tiles_per_split,
                                                      const PolyKernel poly, double *__restrict__ out)
{
    kernel_tile_product<KP>(Y, nullptr, XS, nullptr, V, ld, pk, m, m_pad, s_tiles, tiles_per_split, PolyTile{poly},
                            out);
}

// out_tall = kappa(Y, X_S) V for the kernel `spec`, the one launcher of the three product kernels: rows [0, m) of
// Y ([m_pad][ld], m_pad / 64 row tiles = grid.x) against s_pad / 64 column tiles of X_S ([s_pad][ld]) and V
// ([s_pad][KP]); ny / ns: the squared row norms of Y / X_S (RBF; POLY reads none); p: the features of a row.  The
// column tiles are split over grid.y so that about 1024 blocks run (~4 per CU); with more than one split the
// kernel writes [nsplit][m_pad][KP] partials that k_sum_chunks adds in a fixed order.  RBF with Y == X_S (the
// fit: rows and columns are the same set, the diagonal is exactly 1) is k_rbf_kv, RBF otherwise
// k_rbf_cross_mfma, POLY k_poly_kv_mfma for both.
static int launch_kernel_product(Ctx *c, const KernelSpec &spec, const double *Y, const double *ny, const double *XS,
                                 const double *ns, const double *V, long ld, long p, long m, long m_pad, long s_pad,
                                 double *out_tall)
{
    const long rtiles = m_pad / 64, stiles = s_pad / 64;
    long nsplit = (1024 + rtiles - 1) / rtiles;
    if (nsplit > stiles) nsplit = stiles;
    if (nsplit < 1) nsplit = 1;
    const long tps = (stiles + nsplit - 1) / nsplit;
    nsplit = (stiles + tps - 1) / tps;
    double *dst = out_tall;
    if (nsplit > 1) {
        AA_CHECK(c->rlPartial.alloc((size_t)nsplit * m_pad * c->KP * sizeof(double)));
        dst = c->rlPartial.as<double>();
    }
    const dim3 grid((unsigned)rtiles, (unsigned)nsplit);
    const bool rbf_fit = spec.kind == IMPLICIT_RBF && Y == XS;
    const size_t lds_fit = (size_t)(64 * 65 + 64 * c->KP + 2 * 64 * 17) * sizeof(double);   // k_rbf_kv's dynamic LDS
    static bool attr_rbf[64] = {false};
    if (rbf_fit && !attr_rbf[c->device & 63]) {
        AA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rbf_kv<32>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        AA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rbf_kv<64>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr_rbf[c->device & 63] = true;
    }
    const int pk = (int)round_up(p, 4);                  // the MFMAs of the tile body stop here
#define PRODUCT(KPV)                                                                                              \
    do {                                                                                                          \
        if (rbf_fit)                                                                                              \
            hipLaunchKernelGGL(k_rbf_kv<KPV>, grid, dim3(256), lds_fit, c->stream, Y, ld, (int)p, ny, spec.gamma, V, m, \
                               m_pad, tps, dst);                                                                  \
        else if (spec.kind == IMPLICIT_RBF)                                                                       \
            hipLaunchKernelGGL(k_rbf_cross_mfma<KPV>, grid, dim3(256), 0, c->stream, Y, ny, XS, ns, V, ld, pk, m, \
                               m_pad, stiles, tps, spec.gamma, dst);                                              \
        else                                                                                                      \
            hipLaunchKernelGGL(k_poly_kv_mfma<KPV>, grid, dim3(256), 0, c->stream, Y, XS, V, ld, pk, m, m_pad,    \
                               stiles, tps, spec.poly(), dst);                                                    \
    } while (0)
    if (c->KP == 32) PRODUCT(32); else PRODUCT(64);
#undef PRODUCT
    if (nsplit > 1) {
        const long elems = m_pad * c->KP;
        hipLaunchKernelGGL(k_sum_chunks, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, c->stream,
                           (const double *)dst, elems, (int)nsplit, out_tall);
    }
    AA_CHECK_HIP(hipGetLastError());
    return AA_OK;
}

// the fit: K V on the features (rows = columns = the n samples padded to 128)
int kernel_kv(Ctx *c, const double *V_tall, double *out_tall)
{
    AA_REQUIRE(c->kernel.kind && c->feat.p, AA_ERR_STATE, "no implicit kernel set");
    const double *F = c->feat.as<double>(), *nrm = c->featNorm.as<double>();
    return launch_kernel_product(c, c->kernel, F, nrm, F, nrm, V_tall, c->feat_ld, c->feat_p, c->n, c->n_pad, c->n_pad,
                                 out_tall);
}

// KernelAA.transform: Gr (XW) = kappa(Y, X_S) V, the resident rows against the reference set
int kernel_cross(Ctx *c)
{
    AA_REQUIRE(c->cross_s > 0 && c->cross_k == c->k && c->dtype == AA_F64, AA_ERR_STATE, "no %s reference set",
               c->cross.name());
    return launch_kernel_product(c, c->cross, c->X.as<double>(), c->rowNorm.as<double>(), c->crossX.as<double>(),
                                 c->crossNorm.as<double>(), c->crossV.as<double>(), c->p_pad, c->p, c->n, c->n_pad,
                                 c->cross_s_pad, c->Gr.as<double>());
}

// tr K = sum_i kappa(x_i, x_i) from the squared row norms: one block, each thread a strided sum, then a tree
// over the threads -- the same order, hence the same bits, on every call
__global__ __launch_bounds__(256) void k_poly_trace(const double *__restrict__ nrm, long n, const PolyKernel poly,
                                                    double *__restrict__ out)
{
    __shared__ double part[256];
    double s = 0.0;
    for (long r = threadIdx.x; r < n; r += 256) s += poly_kappa(nrm[r], poly);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

int launch_poly_trace(Ctx *c, double *trace_out_host)
{
    AA_REQUIRE(c->kernel.kind == IMPLICIT_POLY && c->featNorm.p, AA_ERR_STATE, "no implicit polynomial kernel set");
    double *out = c->featNorm.as<double>() + c->n_pad;   // the first slack entry behind the norms (never read as one)
    hipLaunchKernelGGL(k_poly_trace, dim3(1), dim3(256), 0, c->stream, (const double *)c->featNorm.as<double>(), c->n,
                       c->kernel.poly(), out);
    AA_CHECK_HIP(hipGetLastError());
    AA_CHECK_HIP(ctx_memcpy(c, trace_out_host, out, sizeof(double), hipMemcpyDeviceToHost));
    return AA_OK;
}

int launch_row_norms(Ctx *c, const double *F, long ld, long p, long rows, double *nrm)
{
    hipLaunchKernelGGL(k_rbf_norms, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->stream, F, ld, (int)p, rows,
                       nrm);
    AA_CHECK_HIP(hipGetLastError());
    return AA_OK;
}

// 0: operands straight from global memory; 1: X staged in wave-private LDS;
// >= 2: block-tiled, B shared through LDS: 2 = 64-column tiles, 3 = 64 double-buffered,
// 4 (default) = 128, 5 = 32 double-buffered, 6 = 128 double-buffered, 7 = 32;
// 8: wave-streaming (wave-private X tiles, B slabs shared per block); 9: the same with LDS-DMA staging
// and float64 sums of 32-column pieces (k <= 32).  aa_set_option.
int g_row_local_variant = -1;   // -1: by size (wave-streaming from 32768 rows per GPU -- 9 for k <= 32, 8 above -- else 4)
int g_reduce_sparse = 1;       // the flagged reduce-over-rows calls (the SPG direction) gather their non-zero row groups
int g_reduce_sparse_max = -1;  // flagged groups per slab up to which the gather kernel takes the slab; -1: a quarter (float32) / half (float64) of a slab's groups
int g_f64_mfma = 1;            // float64 data: pass kernels on the f64 matrix cores (0: f64 VALU;
                               // row-local: 1 = wave-streaming from 32768 rows, else block-tiled;
                               // 2 / 3 = always wave-streaming / always block-tiled)
int g_row_local_acc64 = 1;     // float32 row-local kernels: cut the fp32 accumulation chain every 32 columns and sum the
                               // pieces in float64 -- 0: never (row_local_variant 8 for large shards), 1: in the
                               // block-tiled kernel and, for large shards with k <= 32, through the LDS-DMA kernel
                               // (variant 9), 2: in the register-staged wave-streaming kernel too (k > 32; costs
                               // it a wave per SIMD: 0.31 -> 0.6 ms)
int g_row_local_split = 1;     // block-tiled kernels: split the contraction over column chunks when there are few row blocks

// The row-local kernels on element type T share two signatures: the plain one, and one with a trailing int -- W, the
// waves per block (streaming families), or the column chunk (block-tiled families).
template <typename T>
using RowLocalFn = void (*)(const T *, long, const T *, int, double *, long);
template <typename T>
using RowLocalArgFn = void (*)(const T *, long, const T *, int, double *, long, int);

template <typename T>
static void row_local_launch(Ctx *c, const RowLocalPlan &pl, RowLocalFn<T> kernel, const void *B, double *dst)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3((unsigned)pl.block), pl.lds,
                       c->stream, c->X.as<T>(), c->p_pad, reinterpret_cast<const T *>(B), (int)c->p_pad, dst, c->n_pad);
}

template <typename T>
static void row_local_launch(Ctx *c, const RowLocalPlan &pl, RowLocalArgFn<T> kernel, const void *B, double *dst,
                             int arg)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3((unsigned)pl.block), pl.lds,
                       c->stream, c->X.as<T>(), c->p_pad, reinterpret_cast<const T *>(B), (int)c->p_pad, dst, c->n_pad,
                       arg);
}

// A streaming family: kernels[which] with W waves per block, behind the raised dynamic-LDS limit -- set on all the
// family's kernels, once per device, before its first launch there.
static bool &row_local_lds_raised(const Ctx *c, RowLocalFamily family)
{
    static bool raised[ROW_LOCAL_FAMILIES][64] = {{false}};          // the attribute is per device
    return raised[(int)family][c->device & 63];
}

template <typename T, int N>
static int row_local_stream(Ctx *c, const RowLocalPlan &pl, const RowLocalArgFn<T> (&kernels)[N], int which,
                            const void *B, double *dst)
{
    bool &raised = row_local_lds_raised(c, pl.family);
    if (pl.raise_lds && !raised) {
        for (const RowLocalArgFn<T> kernel : kernels)
            AA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)PASS_LDS_LIMIT));
        raised = true;
    }
    row_local_launch<T>(c, pl, kernels[which], B, dst, pl.W);
    return AA_OK;
}

int launch_row_local(Ctx *c, const void *B_wideT, double *out_tall)
{
    // every instantiation a family has; [KP == 64] where nothing else is said
    static const RowLocalArgFn<float> dma[1] = {k_row_local_f32_dma};
    static const RowLocalArgFn<float> ws32[4] = {k_row_local_f32_ws<1, false>, k_row_local_f32_ws<2, false>,
                                                 k_row_local_f32_ws<1, true>, k_row_local_f32_ws<2, true>};   // [2 acc64 + (KP == 64)]
    struct Blk { int nct, tile; bool dbuf; RowLocalArgFn<float> acc64, chain; };
#define RLB(NCTV, TCV, DBV) \
    {NCTV, TCV, DBV, k_row_local_f32_blk<NCTV, TCV, DBV, true>, k_row_local_f32_blk<NCTV, TCV, DBV, false>}
    static const Blk blk[] = {RLB(1, 64, true),  RLB(1, 128, false), RLB(1, 32, true),  RLB(1, 128, true),
                              RLB(1, 32, false), RLB(1, 64, false),  RLB(2, 64, true),  RLB(2, 64, false)};
#undef RLB
    static const RowLocalFn<float> lds[2] = {k_row_local_f32_lds<1>, k_row_local_f32_lds<2>};
    static const RowLocalFn<float> global[2] = {k_row_local_f32<1, row_local_global_rt(1)>,
                                                k_row_local_f32<2, row_local_global_rt(2)>};
    static const RowLocalArgFn<double> ws64[2] = {k_row_local_f64_ws<2>, k_row_local_f64_ws<4>};
    static const RowLocalArgFn<double> mfma[2] = {k_row_local_f64_mfma<2>, k_row_local_f64_mfma<4>};
    static const RowLocalFn<double> valu[2] = {k_row_local_f64<32>, k_row_local_f64<64>};

    const RowLocalPlan pl = row_local_plan(pass_knobs(), c->dtype == AA_F32, c->KP, c->n_pad, c->p_pad);
    const int kp64 = c->KP == 64;
    pass_name(pl, c->pass_names[1], sizeof(c->pass_names[1]));
    gemm_event(c, 1);
    // split over column chunks: a partial per chunk, summed behind the kernel
    double *dst = out_tall;
    if (pl.nsplit > 1) {
        AA_CHECK(c->rlPartial.alloc(pl.partial_bytes));
        dst = c->rlPartial.as<double>();
    }
    switch (pl.family) {
        case RowLocalFamily::f32_dma: AA_CHECK(row_local_stream<float>(c, pl, dma, 0, B_wideT, dst)); break;
        case RowLocalFamily::f32_ws: AA_CHECK(row_local_stream<float>(c, pl, ws32, 2 * pl.acc64 + kp64, B_wideT, dst)); break;
        case RowLocalFamily::f32_blk: {
            RowLocalArgFn<float> kernel = nullptr;
            for (const Blk &k : blk)
                if (k.nct == pl.targ && k.tile == pl.tile && k.dbuf == pl.dbuf) kernel = pl.acc64 ? k.acc64 : k.chain;
            AA_REQUIRE(kernel, AA_ERR_STATE, "row-local pass: no block-tiled kernel of the planned shape");
            row_local_launch<float>(c, pl, kernel, B_wideT, dst, pl.chunk);
            break;
        }
        case RowLocalFamily::f32_lds: row_local_launch<float>(c, pl, lds[kp64], B_wideT, dst); break;
        case RowLocalFamily::f32_global: row_local_launch<float>(c, pl, global[kp64], B_wideT, dst); break;
        case RowLocalFamily::f64_ws: AA_CHECK(row_local_stream<double>(c, pl, ws64, kp64, B_wideT, dst)); break;
        case RowLocalFamily::f64_mfma: row_local_launch<double>(c, pl, mfma[kp64], B_wideT, dst, pl.chunk); break;
        case RowLocalFamily::f64_valu: row_local_launch<double>(c, pl, valu[kp64], B_wideT, dst); break;
    }
    if (pl.nsplit > 1) {
        const long elems = c->n_pad * c->KP;
        hipLaunchKernelGGL(k_sum_chunks, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, c->stream,
                           (const double *)dst, elems, pl.nsplit, out_tall);
    }
    AA_CHECK_HIP(hipGetLastError());
    gemm_event(c, 1);
    return AA_OK;
}

}  // namespace aa

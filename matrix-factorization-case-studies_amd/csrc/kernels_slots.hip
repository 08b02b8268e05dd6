// kernels_slots.hip -- calendar-slot climatology and anomalies of resident data (aa_data_slot_sums,
// aa_set_data_rows_slots): per-slot column sums, per-slot squared deviations and the per-slot affine copy for
// hundreds of slots (366 days, 1464 six-hourly steps of a year), where the coefficient matrix of
// k_col_weighted_sums would be a sparse indicator and its dense MFMA contraction the wrong tool.
//
// The kernels are slot-major.  group_plan.h sorts the rows by slot and cuts every slot's member list into chunks of
// at most AA_SLOT_CHUNK_ROWS rows; a WORK ITEM is one chunk and one tile of AA_SLOT_TILE_COLS = 256 adjacent
// columns, and one wave owns it: it keeps the slot's table row(s) in registers and walks the chunk's member rows.
// The members of a chunk are a year apart, so every row is a gather of its own; a lane reads 16-byte vectors,
//   float32: one float4,   columns cw + 4 l + e            (the wave reads one 1024-byte run of the row),
//   float64: two double2,  columns cw + 128 i + 2 l + e    (two 1024-byte runs),
// so a lane holds four columns of a tile in both element types, and SLOT_U member rows are loaded before they are
// used (SLOT_U x 16 or 32 bytes per lane in flight).  There is no LDS and no barrier; the four waves of a block take
// four consecutive work items (column tiles of one chunk first), and the row indices, chunk records and table rows
// are read through wave-uniform addresses.  Items are laid along grid.x: chunks x tiles has no 65 535 limit there.
#include "aa_internal.h"

namespace aa {

template <typename T> struct SlotVec;
template <> struct SlotVec<float>  { typedef float4  vec; enum { V = 4, NV = 1 }; };
template <> struct SlotVec<double> { typedef double2 vec; enum { V = 2, NV = 2 }; };
__device__ __forceinline__ void slotvec_get(const float4 &v, double *x) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
__device__ __forceinline__ void slotvec_get(const double2 &v, double *x) { x[0] = v.x; x[1] = v.y; }
__device__ __forceinline__ float4 slotvec_put(const double *x, float)
{
    return make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
}
__device__ __forceinline__ double2 slotvec_put(const double *x, double) { return make_double2(x[0], x[1]); }

constexpr int SLOT_U = 8;                    // member rows a lane has in flight

// the wave's work item: chunk record and first column of its tile; false: past the last item (wave-uniform)
struct SlotItem {
    long chunk, cw;
    int slot, begin, len;
};
__device__ __forceinline__ bool slot_item(const int *__restrict__ chunks, long nchunk, int ntile, SlotItem *it)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long item = (long)blockIdx.x * 4 + wave;
    if (item >= nchunk * ntile) return false;
    it->chunk = item / ntile;
    it->cw = (item % ntile) * AA_SLOT_TILE_COLS;
    it->slot = chunks[3 * it->chunk];
    it->begin = chunks[3 * it->chunk + 1];
    it->len = chunks[3 * it->chunk + 2];
    return true;
}

// partial[chunk][j] = sum over the chunk's member rows t of x[t][j] (SQ = false) or of (x[t][j] - centre[g][j])^2
// (SQ = true, g the chunk's slot; the centre row is loaded once per work item), all in float64, elements widened
// on load.  Summation order: a lane adds the member rows of its columns one after the other in member order, which
// is ascending row index -- one chain per column, the same on every call; no atomics.  Padding columns (p .. ld):
// x = 0 and centre = 0 there (zero-filled allocations), so their sums are zero.  rows: the plan's row list;
// chunks: (slot, begin, len) per chunk.
template <typename T, bool SQ>
__global__ __launch_bounds__(256) void k_slot_sums(const T *__restrict__ X, long ld, const int *__restrict__ rows,
                                                   const int *__restrict__ chunks, long nchunk, int ntile,
                                                   const double *__restrict__ centre, double *__restrict__ partial)
{
    typedef SlotVec<T> SV;
    typedef typename SV::vec vec;
    constexpr int V = SV::V, NV = SV::NV;
    SlotItem it;
    if (!slot_item(chunks, nchunk, ntile, &it)) return;        // wave-uniform, and the kernel has no barrier
    const int lane = threadIdx.x & 63;
    long col[NV];
    bool on[NV];
    double m[4], acc[4];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        col[i] = it.cw + (long)i * 64 * V + lane * V;
        on[i] = col[i] < ld;                                    // ld is a multiple of 128: whole vectors
#pragma unroll
        for (int e = 0; e < V; ++e) {
            m[i * V + e] = (SQ && on[i]) ? centre[(long)it.slot * ld + col[i] + e] : 0.0;
            acc[i * V + e] = 0.0;
        }
    }
    const int *mine = rows + it.begin;
    auto add = [&](const vec &q, int i) {
        double x[V];
        slotvec_get(q, x);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const double d = x[e] - m[i * V + e];
            acc[i * V + e] += SQ ? d * d : d;
        }
    };
    int t = 0;
    for (; t + SLOT_U <= it.len; t += SLOT_U) {
        vec q[SLOT_U][NV];
#pragma unroll
        for (int u = 0; u < SLOT_U; ++u) {
            const long row = mine[t + u];
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (on[i]) q[u][i] = *reinterpret_cast<const vec *>(X + row * ld + col[i]);
        }
#pragma unroll
        for (int u = 0; u < SLOT_U; ++u)
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (on[i]) add(q[u][i], i);
    }
    for (; t < it.len; ++t) {
        const long row = mine[t];
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (on[i]) add(*reinterpret_cast<const vec *>(X + row * ld + col[i]), i);
    }
    double *dst = partial + it.chunk * ld;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (on[i]) {
#pragma unroll
            for (int e = 0; e < V; e += 2)
                *reinterpret_cast<double2 *>(dst + col[i] + e) = make_double2(acc[i * V + e], acc[i * V + e + 1]);
        }
}

// out[g][j] = the partials of slot g's chunks added in ascending chunk order (four loads in flight, one chain of
// additions): the same bits on every call.  A slot without chunks gives exactly 0.0.  One thread per column, 128
// columns per block, grid (ld / 128, G).  k_col_moment_finish does not fit: its slabs are a fixed stride apart and
// equally many per output, a slot's chunks are neither.
__global__ __launch_bounds__(128) void k_slot_finish(const double *__restrict__ partial, long ld,
                                                     const int *__restrict__ chunk_first, double *__restrict__ out)
{
    const long col = (long)blockIdx.x * 128 + threadIdx.x;     // < ld: the grid is ld / 128
    const int g = blockIdx.y;
    const long c1 = chunk_first[g + 1];
    const double *src = partial + col;
    double s = 0.0;
    long c = chunk_first[g];
    for (; c + 4 <= c1; c += 4) {
        const double a0 = src[c * ld], a1 = src[(c + 1) * ld], a2 = src[(c + 2) * ld], a3 = src[(c + 3) * ld];
        s += a0;
        s += a1;
        s += a2;
        s += a3;
    }
    for (; c < c1; ++c) s += src[c * ld];
    out[(long)g * ld + col] = s;
}

// Y[r][j] = (T)(((double)X[row0 + r][j] - shift[g][j]) / scale[g][j]) for the member rows r of the chunk (g its
// slot), j < p; either part is left out when its table is null.  Slot-major: the shift / scale entries of the
// lane's four columns sit in registers for the whole chunk.  Exactly the float64 roundings of the NumPy expression
// (X - shift[g]) / scale[g]: one subtraction and one true division -- there is no product next to a sum here, so the
// build's contraction (-ffp-contract=on; k_model_rows keeps it out of its trend term) has nothing to fuse -- and one
// rounding to T.  Column mapping and padding are k_affine_rows' rules: a vector that straddles p stores zeros in its
// tail, vectors beyond p are not written, and only rows of the plan (every row of the block once) are written; Y is
// the zero-filled allocation of install_begin.  rows: block-relative row indices by slot.
template <typename T>
__global__ __launch_bounds__(256) void k_slot_rows(const T *__restrict__ X, long ld, long row0, long p,
                                                   const int *__restrict__ rows, const int *__restrict__ chunks,
                                                   long nchunk, int ntile, const double *__restrict__ shift,
                                                   const double *__restrict__ scale, T *__restrict__ Y)
{
    typedef SlotVec<T> SV;
    typedef typename SV::vec vec;
    constexpr int V = SV::V, NV = SV::NV;
    SlotItem it;
    if (!slot_item(chunks, nchunk, ntile, &it)) return;
    const int lane = threadIdx.x & 63;
    long col[NV];
    bool on[NV];
    double sh[4], sc[4];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        col[i] = it.cw + (long)i * 64 * V + lane * V;
        on[i] = col[i] < p;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const bool in = col[i] + e < p;
            sh[i * V + e] = (shift && in) ? shift[(long)it.slot * ld + col[i] + e] : 0.0;
            sc[i * V + e] = (scale && in) ? scale[(long)it.slot * ld + col[i] + e] : 1.0;
        }
    }
    const int *mine = rows + it.begin;
    auto put = [&](const vec &q, int i, long r) {
        double x[V];
        slotvec_get(q, x);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            double y = 0.0;
            if (col[i] + e < p) {
                y = x[e];
                if (shift) y = y - sh[i * V + e];
                if (scale) y = y / sc[i * V + e];
            }
            x[e] = y;
        }
        *reinterpret_cast<vec *>(Y + r * ld + col[i]) = slotvec_put(x, T());
    };
    int t = 0;
    for (; t + SLOT_U <= it.len; t += SLOT_U) {
        vec q[SLOT_U][NV];
        long r[SLOT_U];
#pragma unroll
        for (int u = 0; u < SLOT_U; ++u) {
            r[u] = mine[t + u];
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (on[i]) q[u][i] = *reinterpret_cast<const vec *>(X + (row0 + r[u]) * ld + col[i]);
        }
#pragma unroll
        for (int u = 0; u < SLOT_U; ++u)
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (on[i]) put(q[u][i], i, r[u]);
    }
    for (; t < it.len; ++t) {
        const long r = mine[t];
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (on[i]) put(*reinterpret_cast<const vec *>(X + (row0 + r) * ld + col[i]), i, r);
    }
}

static int slot_grid(long nchunk, long ntile, unsigned *blocks)
{
    const long items = nchunk * ntile;
    AA_REQUIRE(items > 0 && (items + 3) / 4 < (1L << 31), AA_ERR_ARG, "%ld chunks x %ld column tiles do not fit one grid",
               nchunk, ntile);
    *blocks = (unsigned)((items + 3) / 4);
    return AA_OK;
}

// out_dev (G x p_pad) = the per-slot sums of c's matrix; centre_dev (G x p_pad, padding columns zero): null for the
// plain sums; partial_dev: nchunk x p_pad doubles.  Rows of centre_dev whose slot has no chunk are not read.
int launch_slot_sums(Ctx *c, const SlotPlanDev &pd, const double *centre_dev, double *partial_dev, double *out_dev)
{
    const long ntile = (c->p_pad + AA_SLOT_TILE_COLS - 1) / AA_SLOT_TILE_COLS;
    if (pd.nchunk > 0) {
        unsigned blocks = 0;
        AA_CHECK(slot_grid(pd.nchunk, ntile, &blocks));
#define SSUMS(T, SQ)                                                                                              \
    hipLaunchKernelGGL((k_slot_sums<T, SQ>), dim3(blocks), dim3(256), 0, c->stream, (const T *)c->X.as<T>(),      \
                       c->p_pad, pd.rows, pd.chunks, pd.nchunk, (int)ntile, centre_dev, partial_dev)
        if (c->dtype == AA_F32) {
            if (centre_dev) SSUMS(float, true); else SSUMS(float, false);
        } else {
            if (centre_dev) SSUMS(double, true); else SSUMS(double, false);
        }
#undef SSUMS
        AA_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_slot_finish, dim3((unsigned)(c->p_pad / 128), (unsigned)pd.G), dim3(128), 0, c->stream,
                       (const double *)partial_dev, c->p_pad, pd.chunk_first, out_dev);
    AA_CHECK_HIP(hipGetLastError());
    return AA_OK;
}

// c->X (zero filled, c->n x c->p_pad) from rows [row0, row0 + c->n) of the owner's matrix of the same p_pad; pd: the
// plan of the block's c->n labels (every row counted); shift_dev / scale_dev: G x p_pad, nullable; dst: null for
// c->X, or a buffer of its layout (aa_time_kernel)
int launch_slot_rows(Ctx *c, const void *owner_X, long row0, const SlotPlanDev &pd, const double *shift_dev,
                     const double *scale_dev, void *dst)
{
    if (!dst) dst = c->X.p;
    const long ntile = (c->p + AA_SLOT_TILE_COLS - 1) / AA_SLOT_TILE_COLS;
    unsigned blocks = 0;
    AA_CHECK(slot_grid(pd.nchunk, ntile, &blocks));
    if (c->dtype == AA_F32)
        hipLaunchKernelGGL(k_slot_rows<float>, dim3(blocks), dim3(256), 0, c->stream,
                           reinterpret_cast<const float *>(owner_X), c->p_pad, row0, c->p, pd.rows, pd.chunks, pd.nchunk,
                           (int)ntile, shift_dev, scale_dev, reinterpret_cast<float *>(dst));
    else
        hipLaunchKernelGGL(k_slot_rows<double>, dim3(blocks), dim3(256), 0, c->stream,
                           reinterpret_cast<const double *>(owner_X), c->p_pad, row0, c->p, pd.rows, pd.chunks, pd.nchunk,
                           (int)ntile, shift_dev, scale_dev, reinterpret_cast<double *>(dst));
    AA_CHECK_HIP(hipGetLastError());
    return AA_OK;
}

}  // namespace aa

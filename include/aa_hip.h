/*
 * aa_hip.h -- C ABI of libaa_hip.so: the MI355X (gfx950) implementation of the
 * archetypal-analysis / GPNH-convex-coding inner solver of `convex_dim_red`.
 *
 * The reference (azedarach/matrix-factorization-case-studies) has NO native/FFI layer:
 * its hot path is numba-JIT Python behind the module surface of
 * src/convex_dim_red.  This header is therefore the boundary a maintainer would
 * bind with ctypes from that package; every entry point cites
 * the reference code it replaces (paths relative to src/convex_dim_red/).
 *
 * Conventions
 *   - every function returns 0 on success, a negative AA_ERR_* code otherwise;
 *     aa_last_error() returns a message for the calling thread's last failure;
 *   - nothing throws across the ABI; plain pointers and sizes only;
 *   - host buffers are caller-owned, row-major, float64 unless said otherwise,
 *     and are only read or filled during the call; device memory is owned by
 *     the context; a context is NOT thread-safe (one per estimator call);
 *   - "n" = samples (rows of X), "p" = features, "k" = components (k <= 64).
 */
#ifndef AA_HIP_H
#define AA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define AA_OK            0
#define AA_ERR_ARG      -1   /* bad argument / unsupported size                 */
#define AA_ERR_HIP      -2   /* a HIP runtime call failed (no GPU, OOM, fault)   */
#define AA_ERR_STATE    -3   /* call order violated (e.g. update before set_data)*/
#define AA_ERR_COMM     -4   /* RCCL failure                                     */

#define AA_F32 0             /* X stored + contracted in float32 (MFMA f32)      */
#define AA_F64 1             /* X stored + contracted in float64 (reference dtype)*/

#define AA_FORM_DATA   0     /* ArchetypalAnalysis: data matrix X (n x p)        */
#define AA_FORM_KERNEL 1     /* KernelAA: kernel matrix K (n x n)                */

#define AA_MAX_K 64

typedef struct aa_ctx aa_ctx;   /* opaque */

/* Parameters of the per-sample simplex QP solver.
 * Replaces the keyword arguments of quad_simplex_spg (spg.py:286-291) as forwarded
 * by _update_kernel_aa_weights (archetypal_analysis.py:372-383) and
 * _update_gpnh_weights (gpnh_convex_coding.py:257-268). */
typedef struct {
    double gamma;
    int    memory;
    double sigma_one, sigma_two, lambda_min;
    double alpha0, alpha_min, alpha_max;
    double epsilon_one, epsilon_two;
    int    max_iterations, max_feval;
} aa_qp_params;

/* Parameters of the dictionary SPG solver: keyword arguments of spg()
 * (spg.py:46-51).  alpha0 < 0 means "None" (derive from the first projected
 * gradient step, spg.py:178-189). */
typedef struct {
    double gamma;
    int    memory;
    double sigma_one, sigma_two, lambda_min;
    double alpha0, alpha_min, alpha_max;
    double epsilon_one, epsilon_two;
    int    use_infinity_norm;
    int    max_iterations, max_feval;
} aa_spg_params;

#define AA_SPG_FLAG_CONVERGED      1   /* spg.py:259-266                         */
#define AA_SPG_FLAG_LAMBDA_MIN     2   /* warning at spg.py:225-229              */
#define AA_SPG_FLAG_MAX_FEVAL      4   /* warning at spg.py:272-276              */
#define AA_SPG_FLAG_MAX_ITER       8   /* warning at spg.py:278-281              */
#define AA_SPG_FLAG_PROJ_UNCONV   16   /* internal: projection pass cap reached  */

typedef struct {
    double f;          /* spg() return value 2: f at the returned point          */
    int    n_iter;     /* spg() return value 3: 0-based index of the last pass   */
    int    n_feval;    /* spg() return value 4                                   */
    int    flags;      /* AA_SPG_FLAG_*                                          */
    double res_norm;   /* ||P(x - g) - x||_2 at exit                             */
} aa_spg_stats;

typedef struct {
    long   total_passes;   /* sum over samples of SPG loop passes                */
    int    max_passes;     /* largest per-sample pass count                      */
    int    reserved;
} aa_qp_stats;

/* ------------------------------------------------------------------ misc */
const char *aa_last_error(void);
int aa_version(void);
int aa_device_count(int *count);
/* Process-wide tuning knobs (results are identical up to rounding for every setting).  The names below
 * are exactly the rows of the table behind aa_set_option (solver.hip); any other name is an error.
 * A 0|1 knob takes any value and stores value != 0.
 *   "row_local_variant" -1..9  float32 row-local GEMM: -1 (default) chosen by size (from 32768 rows
 *                               per GPU: 9 for k <= 32, 8 for k <= 64; else 4), 0 direct, 1 wave-private
 *                               LDS, 2..7 block-tiled (2: 64-column tiles, 3: 64 double-buffered,
 *                               4: 128, 5: 32 double-buffered, 6: 128 double-buffered, 7: 32),
 *                               8 wave-streaming (wave-private X tiles, shared B slabs, register
 *                               staged), 9 wave-streaming with both operands by LDS-DMA and float64
 *                               sums of 32-column fp32 pieces
 *   "row_local_acc64"   0..2   float32 row-local pass: 1 (default) = every fp32 accumulation chain ends
 *                               after 32 columns and the pieces are summed in float64 (block-tiled
 *                               kernels and variant 9; what keeps long float32 runs on the float64
 *                               trajectory); 2 = also in variant 8 (half speed);
 *                               0 = one fp32 chain per column chunk (round 2)
 *   "row_local_split"   0|1    1 (default): block-tiled kernels split the contraction over column
 *                               chunks when there are few row blocks
 *   "f64_mfma"          0..3   float64 data: pass kernels on the f64 matrix cores (1, default: the
 *                               row-local one wave-streaming from 32768 rows per GPU, else
 *                               block-tiled; 2 / 3 force either) or on the f64 VALU (0)
 *   "reduce_sparse"     0|1    1 (default): the reduce-over-rows pass of the dictionary update's SPG
 *                               direction D'X (D K in the kernel form) reads only the aligned groups of
 *                               4 rows in which D has an entry != 0.0 (a few hundred rows of n; flags ->
 *                               gather kernel -> dense kernel on the slabs the gather kernel left).  The
 *                               same bits as the dense pass for finite X; float32 data and float64 data
 *                               with f64_mfma != 0; while aa_gemm_timing is enabled the pass runs dense,
 *                               so that its event pairs time full passes.  0: the dense pass
 *   "reduce_sparse_max" -1..   flagged groups per row slab up to which the gather kernel takes the slab
 *                               (above: the dense kernel); -1 (default): a quarter (float32 data) or half
 *                               (float64 data) of a slab's groups, where the gather kernel stopped paying
 *                               at 100 000 x 4096 (profiles/reduce_sparse_ab.txt)
 *   "proj_mode"         0|1    column simplex projection: 0 candidate lists, 1 iterative full
 *                               passes (also the fallback of a rank whose list overflows); only 0
 *                               and 1 are accepted
 *   "proj_small"        any    1 (default): columns of at most 8192 entries (single rank) find their
 *                               projection threshold in one kernel, one block each, instead of four
 *                               launches; 2: up to 16 384 entries (slower at 12 500); 0: never
 *   "proj_list_cap"     1..2048 multi-rank: most candidates per rank and column that travel in
 *                               the list all-reduce of a projection (effective: min(this,
 *                               2048 / ranks), so that the union fits the solver's LDS)
 *   "proj_check"        0|1    multi-rank, 1: every list projection is checked for overflow at once (a
 *                               host synchronisation per projection); default 0: the check is deferred
 *   "use_graph"         0|1    1: aa_outer_iterations captures two outer iterations in a
 *                               hipGraph and replays it (single rank, data form, one SPG
 *                               iteration per dictionary update, >= 8 iterations).  Default 0:
 *                               bit-identical and measured neutral on ROCm 7.2
 *   "qp_mode"           0..4   0 (default), k <= 32: four lanes per sample in the matrix-core operand
 *                               layout (16 samples per wave) followed by the wave-per-sample kernel
 *                               for the stragglers; one lane per sample when max_iterations <= 4
 *                               (nothing diverges); k > 32: one wave per sample.
 *                               1: one wave per sample; 2: lane-per-sample + wave; 3: row kernel
 *                               (16 lanes per sample, samples run to completion); 4: four lanes per
 *                               sample + wave
 *   "qp_pass_cap"       >= 1   SPG passes a sample spends in the lane-per-sample QP kernel
 *                               before it moves to the wave-per-sample kernel
 *   "qp_quad_cap"       >= 0   SPG passes after which the four-lane kernel parks a sample for the
 *                               wave-per-sample kernel (default 0: 32 from 65 536 samples per GPU,
 *                               24 below)
 *   "qp_sort"           0|1    1 (default): the QP kernels take the samples in the order of their
 *                               pass counts in the previous weights update, longest first
 *   "qp_overlap_tail"   0|1    1: the wave-per-sample kernel of the stragglers runs on a side
 *                               stream while Z'X is accumulated (float32 data); the rows it
 *                               changes enter Z'X as a rank-m correction; the weights carry the
 *                               bits of the serial order.  Default 0: measured
 *                               neutral, the stragglers run 2x slower next to the GEMM
 *   "qp_live"           0|1    1: the four-lane kernel hands parked samples to a consumer launch of the
 *                               wave-per-sample kernel that is resident beside it on CUs of its own
 *                               (bit-identical results; default 0: measured slower)
 *   "proj_res_side"     0|1    1 (default): the residual projection of a one-iteration dictionary SPG
 *                               (convergence flags only) runs on a side stream beside the weights QP
 *   "grad_side"         0|1    1 (default): the tail of a one-iteration dictionary SPG (g_new, x += lambda d,
 *                               BB stage, residual projection) on the side stream beside the weights QP
 *   "fuse_finalize"     0|1    1 (default): fewer, fatter launches in the dictionary update (set-up
 *                               kernel, scalar stages inside the finalize kernels, two-launch line
 *                               search, x update inside the gradient kernel)
 *   "pack_comm"         0|1    multi-rank, 1 (default): four small reductions ride in the tail of the
 *                               all-reduce that follows them (10 collectives per outer iteration, not 14)
 *   "outer_nosync"      0|1    measurement only (tools/interleave_probe.py): aa_outer_iterations called
 *                               WITHOUT a cost buffer returns with its work in flight
 * Changes results at rounding level (another summation order):
 *   "pq_mfma"           0|1    1 (default): the two wide Grams of the line search on the f64 matrix cores;
 *                               0: the LDS / VALU kernel
 * None of the following seven changes a bit of any result; tests/test_gpu_longrun.py:
 * test_schedule_knobs_do_not_change_a_bit pins that for the first six, tests/test_gpu_spg_tail.py for the last:
 *   "qp_fused_order"    0|1    1 (default): the sample order of the NEXT weights update is formed by extra
 *                               blocks of this update's continuation launch instead of two launches in
 *                               front of the four-lane kernel
 *   "qp_wave_lazy"      0|1    1 (default): the wave-per-sample kernel decides the stopping test of a pass at
 *                               the top of the next one and skips it when <d, d> proves it negative
 *   "qp_quad_lazy"      0|1    the same in the four-lane kernel (default 0: no gain there)
 *   "fin_in_last"       0|1    1 (default): the two reductions of a projection are finalized by the last
 *                               block of their pass (write-through partials), not by a launch of their own
 *   "setup_in_grad"     0|1    1 (default): the dictionary update's set-up block is block 0 of its first
 *                               gradient launch
 *   "gram_side"         0|1    Z'Z of the refresh after a weights update on the side stream (default 0)
 *   "spg_tail"          0|1    1: every one-iteration dictionary update runs the whole tail of its SPG iteration
 *                               (g_new, <d, g_new>, the BB step, the residual projection with ||res|| and the
 *                               CONVERGED / MAX_FEVAL flags).  0 (default): the updates of aa_outer_iterations,
 *                               and those of aa_iterate once the status record shows AA_SPG_FLAG_MAX_ITER, run
 *                               x += lambda d alone -- nothing reads the rest there (csrc/solver.hip:
 *                               spg_tail_needed).  Updates with stats, with more than one SPG iteration, behind
 *                               aa_set_dictionary_inputs, of aa_dictionary_update, of the kernel form, of the
 *                               restart slots and of multi-rank runs keep the tail whatever the value;
 *                               aa_iterate with spg max_feval < 202 too.  (A PROJ_UNCONV of a skipped
 *                               residual projection is, naturally, not reported.) */
int aa_set_option(const char *name, int value);

/* -------------------------------------------- stateless ops (unit-test surface) */

/* Euclidean projection of every row of `in` (rows x cols) onto the unit simplex.
 * Replaces simplex_project_rows (simplex_projection.py:40-47) /
 * simplex_project_vector (:13-27). */
int aa_simplex_project_rows(int device, const double *in, double *out, long rows, long cols);

/* Z[t] = argmin_{z in simplex} 0.5 z'Az + b_t'z,  b_t[j] = -B[j*stride_j + t*stride_t],
 * started from Z0[t]; t = 0..n-1.  A: k x k.  iters (nullable): loop passes per sample.
 * Replaces _gu_update_kernel_aa_weights (archetypal_analysis.py:344-366; stride_j = n,
 * stride_t = 1) and _gu_update_gpnh_weights (gpnh_convex_coding.py:229-251; stride_j = 1,
 * stride_t = k), i.e. n calls of quad_simplex_spg (spg.py:286-398). */
int aa_quad_simplex_spg_batch(int device, const double *A, const double *B,
                              long stride_j, long stride_t,
                              const double *Z0, double *Zout, long n, int k,
                              const aa_qp_params *params, int *iters);

/* ------------------------------------------------------ resident solver context */
int aa_ctx_create(aa_ctx **ctx, int device, int dtype);
int aa_ctx_destroy(aa_ctx *ctx);

/* Multi-GPU (one process per GPU, rows of X sharded): rank 0 calls
 * aa_comm_get_unique_id and hands the 128 bytes to the other ranks out of band;
 * every rank then calls aa_ctx_comm_init.  Collectives (RCCL all-reduce, sum/max)
 * run only on the small k x k / k x p Gram products and packed scalars. */
int aa_comm_get_unique_id(void *id128);
int aa_ctx_comm_init(aa_ctx *ctx, const void *id128, int rank, int world);
/* The second transport: a one-shot peer-to-peer all-reduce for the path's
 * latency-bound messages (<= 1 MiB; larger ones go in pieces) -- every rank stores its vector
 * straight into a receive buffer of every peer (mapped with hipIpcOpenMemHandle), raises a flag per
 * block, and reduces the world slots in rank order once the peers' flags are up: one kernel per rank
 * and collective, identical bits on every rank, no RCCL (csrc/comm.hip).  Every rank calls
 * aa_ctx_p2p_export (allocates the buffer; 64-byte IPC handle out), the handles travel out of band
 * like the RCCL unique id, then every rank calls aa_ctx_p2p_init with all `world` handles in rank
 * order; all collectives of the context then use this transport.  At most 8 ranks (one node). */
int aa_ctx_p2p_export(aa_ctx *ctx, int world, void *handle64);
int aa_ctx_p2p_init(aa_ctx *ctx, const void *handles, int rank, int world);
/* all-reduce of a small host vector through the context's communicator (used by
 * bench.py for the barrier + max-over-ranks timing); op: 0 = sum, 1 = max. */
int aa_ctx_allreduce_host(aa_ctx *ctx, double *buf, int count, int op);

/* Installing data.  Thirteen entry points give a context its matrix: aa_set_data, aa_share_data, aa_set_data_rows,
 * aa_set_data_rows_affine, aa_set_data_rows_model, aa_set_data_rows_slots, aa_set_data_take, aa_set_data_projected, aa_set_data_weighted, aa_set_rbf_features, aa_set_poly_features and
 * the _resident forms of the last two.  Every one of them ("an install") first checks its arguments -- a call it
 * refuses has not touched ctx, which keeps the data it had -- and then replaces everything that belonged to the
 * previous matrix: the form and the kind of implicit kernel (none for a stored matrix), aa_set_linear_kernel, the
 * reference set of aa_set_{rbf,poly}_reference, the sizes and the shard, the cached trace, the factors and their
 * Gram products (the next aa_set_state / aa_gpnh_set_factors sizes the arrays afresh), and the pass counts and
 * sample order the QP keeps from one weights update to the next.  The matrix goes into a fresh zero-filled
 * allocation, rows and columns padded to multiples of 128 (aa_share_data aliases the owner's instead; an implicit
 * kernel keeps its float64 features and their squared norms, and no matrix).  What ctx does afterwards depends
 * only on this install, not on the ones before it.  An install that fails after its argument checks (an
 * allocation, a copy, a kernel) leaves ctx WITHOUT data (AA_ERR_STATE from whatever needs some), never with half
 * of it.
 *
 * aa_set_data: upload this rank's row block of the data matrix (form DATA: n x p) or kernel
 * matrix (form KERNEL: n x n, p == n; single rank only).  host_dtype: AA_F32/AA_F64
 * element type of `X` (converted to the context dtype on upload).  The matrix stays
 * resident across restarts.  `n_global`/`row_offset` describe the shard.
 * Replaces the `X`/`K` argument of _iterate_aa / _iterate_kernel_aa
 * (archetypal_analysis.py:534, :399) and `X` of _iterate_gpnh_convex_coding
 * (gpnh_convex_coding.py:282). */
int aa_set_data(aa_ctx *ctx, const void *X, int host_dtype, long n, long p, long ld,
                int form, long n_global, long row_offset);
/* ||X||_F^2 (form DATA; = trace(X X'), archetypal_analysis.py:552 without the n x n
 * temporary) or trace(K) (form KERNEL, :412), summed over all ranks. */
int aa_data_trace(aa_ctx *ctx, double *trace);

/* Factors: C (k x n, this rank's COLUMN block k x n_local, row-major with leading
 * dimension ldc), Z (n_local x k), alpha (k).  Replaces the weights/dictionary/alpha
 * arguments and return values of _iterate_aa (archetypal_analysis.py:534-536,669). */
int aa_set_state(aa_ctx *ctx, int k, const double *C, long ldc, const double *Z, const double *alpha);
int aa_get_state(aa_ctx *ctx, double *C, long ldc, double *Z, double *alpha);
int aa_set_alpha(aa_ctx *ctx, const double *alpha);

/* Recompute every Gram product from (X, C, Z, alpha) and return the cost
 * 0.5 (tr XX' - 2 tr(D C XX' Z) + tr(D Z'Z D C XX' C')) / n.
 * Replaces archetypal_analysis.py:543-558 (:403-418 for the kernel form). */
int aa_prepare(aa_ctx *ctx, double *cost);
/* Cost from the current Gram products and alpha (archetypal_analysis.py:623-627). */
int aa_cost(aa_ctx *ctx, double *cost);
/* k x k Gram products for the host-side scale-factor update
 * (archetypal_analysis.py:243-258): ZtZ, C XX' C', C XX' Z, and the data trace. */
int aa_get_grams(aa_ctx *ctx, double *ZtZ, double *CKCt, double *CKZ, double *trace);
/* Override the dictionary-update inputs with caller-supplied values:
 * KZ = XX'Z or KZ (n_local x k), ZtZ (k x k), trace.  Needed to mirror the
 * test-visible _update_kernel_aa_dictionary(K, C, alpha, trace_K, KZ, ZtZ)
 * (archetypal_analysis.py:304) / _update_aa_dictionary (:324). */
int aa_set_dictionary_inputs(aa_ctx *ctx, const double *KZ, const double *ZtZ, double trace);

/* SPG update of the dictionary with row-simplex constraint, then refresh of
 * CX, C XX', C XX' C', C XX' Z.  Replaces _update_aa_dictionary
 * (archetypal_analysis.py:324-341, cost :261-270, gradient :293-301), or
 * _update_kernel_aa_dictionary (:304-321, :273-290) in the kernel form, plus the
 * refresh at :618-621 (:484-486). */
int aa_dictionary_update(aa_ctx *ctx, const aa_spg_params *params, aa_spg_stats *stats);
/* Per-sample QP update of the weights, then refresh of Z'Z, X'Z, XX'Z, C XX' Z.
 * Replaces _update_kernel_aa_weights (archetypal_analysis.py:369-396) plus the
 * refresh at :640-643 (:501-503). */
int aa_weights_update(aa_ctx *ctx, const aa_qp_params *params, aa_qp_stats *stats);

/* Restarts (bin/run_hadisst_aa.py:158-172 fits n_init models on the same data):
 * `ctx` takes the resident data matrix of `owner` (same device, same dtype, single rank) without
 * a copy -- the solver only reads it -- so several contexts, each with its own factors, streams
 * and scratch, work on ONE copy of X concurrently.  `owner` must outlive `ctx` or give it new
 * data first (any install releases the alias, never the owner's memory).  An install like the others
 * ("installing data" above), of the owner's form (DATA or a stored KERNEL matrix), except that ctx also takes
 * over the owner's cached trace, so that restart contexts do not each run a trace pass. */
int aa_share_data(aa_ctx *ctx, const aa_ctx *owner);

/* Cross-validation on resident data (bin/run_hadisst_aa.py:213-245: TimeSeriesSplit fits on growing
 * prefixes of the training rows and transforms the block behind each, `training_data[train_index]` /
 * `training_data[test_index]` being fresh host slices): rows [row0, row0 + n) of owner's resident DATA
 * matrix become ctx's data matrix -- an install ("installing data" above) of the same values by a
 * device-to-device copy, the host is not involved.  owner is another context on the same device with the same
 * dtype, holding a stored matrix in data form (no kernel matrix, no implicit kernel), both single rank.  Unlike
 * aa_share_data the copy owns its memory: the owner may be destroyed afterwards. */
int aa_set_data_rows(aa_ctx *ctx, const aa_ctx *owner, long row0, long n);

/* Column statistics and standardisation of resident data (the --standardize step of
 * bin/run_jra55_pca_aa.py:165-166 / bin/run_jra55_pca_gpnh.py:162-163,
 * `valid_data / np.std(valid_data, axis=0, keepdims=True)`, without a round trip through the host).
 *
 * aa_data_column_moments: mean[j] = sum_r X[r][j] / n and var[j] = sum_r (X[r][j] - mean[j])^2 / n (ddof 0,
 *   as np.var) of the n resident rows, p values each, either output may be NULL.  Two sweeps over the matrix
 *   (csrc/kernels_tall.hip: k_col_moment_sweep), float64 arithmetic in both context dtypes (elements converted
 *   on load), row-slab partials combined in a fixed order: two calls return the same bits.  Data form with a
 *   stored matrix (AA_ERR_STATE otherwise), single rank.
 * aa_set_data_rows_affine: aa_set_data_rows with Y[r][j] = (X[row0 + r][j] - shift[j]) / scale[j]: float64
 *   subtraction and a true float64 division, rounded once to the context's element type.  shift / scale: host
 *   arrays of owner's p values; NULL: 0 / 1.  A scale[j] that is zero or not finite, or a shift[j] that is not
 *   finite, is refused with AA_ERR_ARG like any other bad argument of an install.  Otherwise the
 *   preconditions and refusals of aa_set_data_rows. */
int aa_data_column_moments(aa_ctx *ctx, double *mean, double *var);
int aa_set_data_rows_affine(aa_ctx *ctx, const aa_ctx *owner, long row0, long n, const double *shift,
                            const double *scale);

/* Seasonal anomalies and per-group standardisation of resident data (the reference notebook
 * hadisst_sst_anom.ipynb: calculate_monthly_anomalies and the per-month (x - mean_month) / std_month behind it).
 * Every quantity of the anomaly model -- the values of the seasonal cycle, the trend's slope and intercept -- is
 * a fixed linear functional of a column, so the model is ONE pass over the matrix with a small coefficient
 * matrix built on the host, and the anomalies one read-and-write pass.
 *
 * aa_data_weighted_column_sums: out[g][j] = sum_t A[g][t] X[t][j] for g < G <= 16, j < p.  A: G x n host doubles
 *   (row-major, n the resident rows), out: G x p host doubles.  float64 arithmetic in both context dtypes
 *   (elements widened on load), the contraction over rows on v_mfma_f64_16x16x4_f64 (csrc/kernels_tall.hip:
 *   k_col_weighted_sums), row-slab partials added in a fixed order, no atomics: two calls return the same bits.
 *   Data form with a stored matrix (AA_ERR_STATE otherwise), single rank.
 * aa_data_grouped_sqdev: out[g][j] = sum_t A[g][t] (X[t][j] - centre[group[t]][j])^2, the second sweep of
 *   per-group variances.  group: n host ints in [-1, Gc), -1: the row is not counted (it contributes 0 whatever
 *   A holds); centre: Gc x p host doubles, Gc <= 16.  Otherwise as above.
 * aa_set_data_rows_model: aa_set_data_rows with
 *     Y[r][j] = ((X[row0 + r][j] - shift[group[r]][j]) - (icpt[j] + slope[j] t[r])) / scale[group[r]][j],
 *   exactly the float64 roundings of that expression as written (a subtraction, a product, a sum, a subtraction,
 *   a true division; nothing fused), rounded once to the context's element type.  shift / scale: G x p host
 *   doubles or NULL (part left out), G <= 16; group: n host ints in [0, G), one per row of the block (NULL with
 *   G == 1: row 0 for every row); icpt / slope: p host doubles, t: n host doubles, all three or none.  G > 16, a
 *   label outside [0, G), a zero or non-finite scale and a non-finite shift, slope, intercept or t are refused
 *   with AA_ERR_ARG like any other bad argument of an install.  Otherwise the preconditions and refusals of
 *   aa_set_data_rows. */
int aa_data_weighted_column_sums(aa_ctx *ctx, int G, const double *A, double *out);
int aa_data_grouped_sqdev(aa_ctx *ctx, int G, const double *A, const int *group, const double *centre, int Gc,
                          double *out);
int aa_set_data_rows_model(aa_ctx *ctx, const aa_ctx *owner, long row0, long n, int G, const int *group,
                           const double *shift, const double *icpt, const double *slope, const double *t,
                           const double *scale);

/* Calendar-slot climatology and anomalies of resident sub-monthly data (the .anom. / .std_anom. inputs of
 * bin/run_jra55_*: deviations from a climatology per calendar slot -- 366 days, 1464 six-hourly steps of a year).
 * A slot is an integer label 0 .. G - 1 per row, taken from the driver's time axis (leap days and irregular
 * calendars are the driver's labels).  With hundreds of slots the coefficient matrix of
 * aa_data_weighted_column_sums would be a sparse indicator, so these entry points are slot-major
 * (csrc/kernels_slots.hip): the host sorts the rows by slot and cuts every slot's rows into chunks of at most
 * AA_SLOT_CHUNK_ROWS (csrc/group_plan.h); one wave takes one chunk and AA_SLOT_TILE_COLS adjacent columns, keeps the
 * slot's table row in registers and walks the chunk's rows.  The <= 16-group entry points above stay what they are.
 *
 * aa_data_slot_sums: out[g][j] = sum of X[t][j] over the rows t with slot[t] == g (centre NULL), or of
 *   (X[t][j] - centre[g][j])^2 (centre: G x p host doubles).  slot: n host ints in [-1, G), n the resident rows, -1:
 *   the row is not counted; out: G x p host doubles; counts (nullable): G host longs, the rows counted per slot.
 *   float64 arithmetic in both context dtypes (elements widened on load).  Summation order: within a chunk the rows
 *   are added one after the other in ascending row index, one chain per column; a finish kernel adds a slot's
 *   chunks in ascending order; no atomics: two calls return the same bits.  A slot without counted rows gives
 *   exactly 0.0 and count 0, and its row of centre is not read (it may hold NaN).  Data form with a stored matrix
 *   (AA_ERR_STATE otherwise), single rank.  AA_ERR_ARG, the first offender named: G < 1 or G > AA_MAX_SLOTS, a
 *   label outside [-1, G), a non-finite centre entry in a slot that a counted row uses.
 * aa_set_data_rows_slots: aa_set_data_rows with Y[r][j] = (X[row0 + r][j] - shift[slot[r]][j]) / scale[slot[r]][j]:
 *   one float64 subtraction and one true float64 division, nothing fused or approximated, rounded once to the
 *   context's element type; either part is left out when its table is NULL, both NULL is refused.  slot: n host ints
 *   in [0, G), one per row of the block; shift / scale: G x p host doubles.  Rows of the tables whose slot no row of
 *   the block uses are not read (they may hold NaN).  AA_ERR_ARG like any other bad argument of an install, before
 *   anything of ctx is released or launched: G < 1 or G > AA_MAX_SLOTS, a label outside [0, G), both tables NULL, a
 *   non-finite shift or a zero or non-finite scale in a slot that a row of the block uses.  Otherwise the
 *   preconditions and refusals of aa_set_data_rows. */
#define AA_MAX_SLOTS 1464            /* 366 x 4: six-hourly steps of a leap year */
#define AA_SLOT_CHUNK_ROWS 64        /* most rows of one slot a work item walks */
#define AA_SLOT_TILE_COLS 256        /* adjacent columns of a work item: one 1024-byte run per row and vector */
int aa_data_slot_sums(aa_ctx *ctx, int G, const int *slot, const double *centre, double *out, long *counts);
int aa_set_data_rows_slots(aa_ctx *ctx, const aa_ctx *owner, long row0, long n, int G, const int *slot,
                           const double *shift, const double *scale);

/* Row gather on the device (seasonal subsets, k-fold splits, bootstrap resamples of a resident block, and the
 * support rows KernelAA.transform keeps, `X[support]`): rows idx[0..n) of owner's resident DATA matrix, in any
 * order and with duplicates, become ctx's data matrix -- an install ("installing data" above) by a gather
 * kernel (csrc/kernels_tall.hip: k_gather_rows); the owner may be destroyed afterwards.  idx == NULL: rows
 * 0..n-1 in order (n <= owner's n).  Preconditions of aa_set_data_rows (same device, data form, both single rank, no
 * implicit kernel behind the owner); the data types are equal, or the owner is float32 and ctx float64 -- an exact
 * widening, the only mixed case.  EVERY index is checked on the host against [0, owner's n) before anything is
 * launched or released: a bad one is AA_ERR_ARG like any other bad argument of an install, and the message names
 * the first. */
int aa_set_data_take(aa_ctx *ctx, const aa_ctx *owner, const long *idx, long n);

/* PCA of resident data (the EOF / PC input of bin/run_jra55_pca_gpnh.py and bin/run_jra55_pca_aa.py, which
 * `run_pca` of notebooks/hadisst_pca.ipynb computes with sklearn.decomposition.PCA on the host): the Gram matrix of
 * the centred matrix with itself, for one host eigen-solve of the smaller side, and the projection of row blocks
 * onto the components, installed as a new block.  Both contractions on v_mfma_f64_16x16x4_f64
 * (csrc/kernels_pca.hip), float64 arithmetic in both context dtypes: elements are widened on load and
 * Xc[r][j] = (double)X[r][j] - shift[j] is one float64 subtraction, the rounding `Xd - m` makes in NumPy.
 *
 * aa_data_gram: side AA_GRAM_ROWS: G = Xc Xc' (n x n, k_gram_rows); AA_GRAM_COLS: G = Xc' Xc (p x p, k_gram_cols).
 *   shift: p host doubles, or NULL for no centring.  out: d x d host doubles with leading dimension ldo, the whole
 *   matrix; out[i][j] and out[j][i] are the same bits (only the 64 x 64 tiles with j >= i are computed, and both
 *   places are written from the one value).  How the contraction is split is decided by csrc/gram_plan.h from the
 *   side, the shape and the compute units; the splits are added in ascending order by a finish kernel, no atomics:
 *   two calls return the same bits.  Data form with a stored matrix (AA_ERR_STATE otherwise), single rank,
 *   d <= 8192 (AA_ERR_ARG above: the result goes through one dense eigen-solve on the host).
 * aa_set_data_projected: an install ("installing data" above): ctx receives the n x q matrix
 *     Y[r][i] = sum_j ((double)X[row0 + r][j] - shift[j]) V[i][j]
 *   from owner's resident DATA matrix (k_project_rows).  V: q x p host doubles (leading dimension ldv),
 *   1 <= q <= AA_MAX_PROJECTED; shift: p host doubles or NULL.  Sums in float64 over ascending j, rounded once to
 *   ctx's element type.  The data types are equal, or the owner is float32 and ctx float64.  Otherwise the
 *   preconditions and refusals of aa_set_data_rows; a non-finite entry of V or shift is AA_ERR_ARG before anything
 *   of ctx is released. */
#define AA_GRAM_ROWS 0
#define AA_GRAM_COLS 1
#define AA_MAX_PROJECTED 256
int aa_data_gram(aa_ctx *ctx, int side, const double *shift, double *out, long ldo);
int aa_set_data_projected(aa_ctx *ctx, const aa_ctx *owner, long row0, long n, int q, const double *V, long ldv,
                          const double *shift);

/* KernelAA on the implicit linear kernel K = X X' (SURVEY 8(f4)): with `on` != 0 the resident
 * DATA matrix X (n x p) stands in for the n x n kernel matrix of _iterate_kernel_aa
 * (archetypal_analysis.py:399-531), which is never formed: every product with K runs as two
 * skinny passes over X, exactly as in the data form, and the dictionary gradient follows the
 * kernel form's convention (divided by n_components, _kernel_aa_dictionary_gradient :281-288,
 * where _aa_dictionary_gradient :291-300 divides by n_samples) -- the one place where the two
 * forms of the reference differ for K = X X'.  Reset by every install. */
int aa_set_linear_kernel(aa_ctx *ctx, int on);
/* KernelAA on an implicit RBF kernel (archetypal_analysis.py:673-910 with the n x n kernel
 * matrix K_ij = exp(-gamma ||x_i - x_j||^2) NEVER formed): uploads the n x p feature matrix (float64) and
 * switches the context to the kernel form of the algorithm; every product C K / K Z is one fused
 * distance + exp + multiply pass over the features (csrc/kernels_gemm.hip: k_rbf_kv), tr K = n, and
 * aa_distance_column returns sqrt(2 - 2 K_ij).  AA_ERR_ARG unless gamma > 0 and finite; single rank and a
 * float64 context, AA_ERR_STATE otherwise (a float32 context is refused here, not only by the binding).  An install
 * ("installing data" above); everything downstream (aa_set_state, aa_prepare, aa_iterate, aa_get_state ...) is the explicit kernel form's. */
int aa_set_rbf_features(aa_ctx *ctx, const double *X, long n, long p, long ld, double gamma);
/* The same for the polynomial kernel K_ij = (gamma x_i.x_j + coef0)^degree (scikit-learn's polynomial_kernel),
 * never formed.  The power is degree - 1 multiplications in a fixed order, evaluated by one device function
 * everywhere (csrc/aa_internal.h: poly_kappa).  Every product C K / K Z runs on the f64 matrix cores
 * (csrc/kernels_gemm.hip: k_poly_kv_mfma), tr K = sum_i (gamma |x_i|^2 + coef0)^degree is summed in a fixed
 * order, and aa_distance_column returns sqrt(max(K_ii - 2 K_ij + K_jj, 0)) with exactly 0 at i = j.
 * AA_ERR_ARG unless gamma > 0, coef0 >= 0 (so that K is positive semi-definite), degree >= 1, all finite.
 * Single rank, float64 context (AA_ERR_STATE).  Both kinds share one body (csrc/solver.hip: set_kernel_features)
 * and one launcher of their products (csrc/kernels_gemm.hip: launch_kernel_product); a refused call has not
 * touched ctx, and ctx names its kernel only once the features are in place. */
int aa_set_poly_features(aa_ctx *ctx, const double *X, long n, long p, long ld, double gamma, double coef0,
                         int degree);
/* aa_set_rbf_features / aa_set_poly_features with the features taken from owner's resident DATA matrix instead of
 * a host array: the zero-padded float64 feature buffer is filled on the device (csrc/kernels_tall.hip:
 * k_features_from_data, which reads owner's element type and leading dimension; float32 widens exactly), so it
 * holds the bits the host entry points give for owner's aa_get_data, and everything downstream is unchanged.
 * owner (another context on the same device, data form with a stored matrix, single rank) is only read and may be
 * destroyed afterwards.  Parameter checks and refusals of the host entry points (float64 ctx, single rank). */
int aa_set_rbf_features_resident(aa_ctx *ctx, const aa_ctx *owner, double gamma);
int aa_set_poly_features_resident(aa_ctx *ctx, const aa_ctx *owner, double gamma, double coef0, int degree);

/* Driver-side preprocessing on the device (bin/run_hadisst_aa.py:133-146 weight_and_flatten_data,
 * :196-209 NaN-column removal and training / validation split; the same steps in
 * bin/run_jra55_pca_gpnh.py).  `raw` is the flattened field, n_total x p_full, row-major
 * (float64 or float32, NaN = missing), `col_weight[p_full]` the latitude weight of every flattened
 * column (NULL: 1).  Columns with a NaN in ANY of the n_total rows are dropped, the others are
 * multiplied by their weight, and rows [row0, row0 + n) become the context's data matrix (data
 * form): an install ("installing data" above), refused with AA_ERR_ARG when no column is left.
 * valid[p_full] receives 1 / 0 per column, *p_valid the number of columns kept.  The raw field crosses PCIe once; weighting, the NaN scan and the
 * compaction run on the GPU. */
int aa_set_data_weighted(aa_ctx *ctx, const void *raw, int host_dtype, long n_total, long p_full,
                         long ld, const double *col_weight, long row0, long n,
                         unsigned char *valid, long *p_valid);
/* The resident data matrix back on the host as float64 (n x p, row stride ld): tests, and the
 * few host-side uses of the data the estimators have (GPNH 'random' initialisation). */
int aa_get_data(aa_ctx *ctx, double *out, long ld);

/* The alternating loop of _iterate_aa / _iterate_kernel_aa (archetypal_analysis.py:586-663,
 * :455-524) for delta == 0, with the monotonicity check (:167-174) and the stopping rule
 * (:177-197, :663) evaluated ON THE DEVICE after every iteration: the host enqueues
 * `check_every` iterations at a time and reads one small status record per batch instead of
 * synchronising three times per iteration (delta != 0 included: the k-vector scale-factor
 * update of :243-258 is one more small kernel).  When the rule fires at iteration j the factors of
 * iteration j are kept (a conditional device-side snapshot), the iterations that were already
 * enqueued behind it are discarded, and the context is left consistent with iteration j. */
typedef struct {
    int    max_outer;          /* archetypal_analysis.py:586 `max_iterations`             */
    double tolerance;
    int    criterion;          /* 0: abs_delta_f, 1: rel_delta_f (:177-197)                */
    int    require_monotonic;  /* :167-174                                                 */
    double mono_tolerance;     /* tolerance of the monotonicity check: the reference uses
                                  `tolerance`; float32 data pass max(tolerance, the float32
                                  noise floor of the trace-form cost)                       */
    int    update_dictionary, update_weights;
    int    check_every;        /* iterations per host poll (>= 1)                          */
    double delta;              /* != 0 (with a scale-factor solver passed to aa_iterate): the
                                  scale-factor update of archetypal_analysis.py:590-609 opens
                                  every iteration, as a k-dimensional SPG in one small kernel  */
} aa_iter_params;

typedef struct {
    int    n_iter;             /* 0-based index of the last iteration (reference n_iter)   */
    int    converged;          /* the stopping rule fired                                  */
    int    error_stage;        /* 0 none, 1 / 2 / 3: cost increased after the dictionary / weights /
                                  scale-factor update                                        */
    int    error_iter;
    int    spg_flags;          /* OR of the dictionary SPG's AA_SPG_FLAG_* over iterations */
    int    reserved;           /* iterations enqueued: >= n_iter + 1 and < n_iter + 1 + check_every
                                  (the ones behind n_iter ran and were discarded)           */
    double cost;               /* cost after the last iteration kept                       */
} aa_iter_stats;

/* cost0: cost of the prepared state (aa_prepare); costs: 2 * max_outer entries, filled for the
 * iterations kept.  Returns AA_OK also when error_stage != 0 (the caller raises). */
int aa_iterate(aa_ctx *ctx, const aa_iter_params *it, const aa_spg_params *spg,
               const aa_qp_params *qp, const aa_spg_params *scale_spg /* NULL: no scale factors */,
               double cost0, double *costs, aa_iter_stats *stats);

/* The alternating loop of _iterate_gpnh_convex_coding (gpnh_convex_coding.py:282-402) on the
 * device, same loop control as aa_iterate.  Per iteration: Z'X (reduce-over-rows GEMM), the
 * regularised normal equations (Z'Z/n + lambda_W GW) W' = Z'X/n (:213-226) solved by a Cholesky
 * factorisation in one small kernel (the reference calls lstsq on the same k x k system; when
 * the factorisation meets a pivot below 1e-13 of the largest diagonal entry the call returns
 * with stats->error_stage = 3 and the caller falls back to its host lstsq path), X W
 * (row-local GEMM), W'W, the GPNH penalty (:179-196), the cost (:317-330) and the n per-sample
 * QPs (:254-279).  Factors set with aa_gpnh_set_factors; the dictionary is read back with
 * aa_gpnh_get_dictionary. */
typedef struct {
    double lambda_W;
    aa_iter_params loop;
} aa_gpnh_params;
int aa_gpnh_iterate(aa_ctx *ctx, const aa_gpnh_params *params, const aa_qp_params *qp,
                    double *cost0, double *costs, aa_iter_stats *stats);
int aa_gpnh_get_dictionary(aa_ctx *ctx, double *Wt /* k x p, row-major */, long ld);

/* n_outer full outer iterations (dictionary, weights) without returning to the
 * caller; costs[2*i], costs[2*i+1] = cost after the dictionary / weights update of
 * iteration i.  delta == 0 only (no scale-factor update).  Replaces the loop body
 * archetypal_analysis.py:586-657 for benchmarking. */
int aa_outer_iterations(aa_ctx *ctx, int n_outer, const aa_spg_params *spg,
                        const aa_qp_params *qp, double *costs);

/* 0.5 ||X - Z diag(alpha) C X||_F^2 / n evaluated in residual form (no trace
 * cancellation); the reconstruction error reported by bench.py. */
int aa_reconstruction_cost(aa_ctx *ctx, double *cost);

/* archetypes = diag(alpha?) C X (k x p): archetypal_analysis.py:1144. */
int aa_get_archetypes(aa_ctx *ctx, double *CX, long ld);

/* FurthestSum support (furthest_sum.py:23-127 needs column j of the n x n
 * dissimilarity matrix, archetypal_analysis.py:95-100): d[i] =
 * sqrt(max(K_ii - 2 K_ij + K_jj, 0)) for this rank's rows i, K = XX' never formed
 * (form DATA) or the stored K (form KERNEL).  j is a GLOBAL row index.  Every form clamps
 * at 0 (the reference does not: where rounding puts K_ii - 2 K_ij + K_jj below zero -- two
 * nearly equal samples of a kernel matrix stored in float32 -- it has NaN and its selection
 * fails; here the entry is 0); where the reference's value is finite the bits are the same.
 * d[j] is exactly 0. */
int aa_distance_column(aa_ctx *ctx, long j, double *d);
/* The whole FurthestSum selection (furthest_sum.py:23-127) on the device, single rank: running
 * distance sums and the candidate flags stay in device memory, every pick is one distance-column
 * kernel and one single-block step, the picked index is passed on in device memory -- no host
 * round trip per pick.  selected[k] out.  *tie != 0: at some pick the largest running sum was
 * shared by several candidates; the reference then takes the one its stable sorts left last, a rule
 * that depends on the history of the list -- the caller repeats the selection through
 * aa_distance_column and the host's list logic (convex_dim_red/furthest_sum.py).  The flag is also raised
 * when a live running sum is NaN (inf - inf behind a non-finite entry of the matrix: no comparison sees
 * it), and the host's logic refuses that selection by name.  Distances in the
 * arithmetic of aa_distance_column, sums updated in the same order: the same picks. */
int aa_furthest_sum(aa_ctx *ctx, int k, long start_index, const int *exclude, int n_exclude, int extra_steps,
                    int *selected, int *tie);
/* What the latest aa_furthest_sum of this context left in its device scratch, copied out: the running sums
 * (n doubles; the entry of a candidate that is not alive keeps the sum it was picked with, that of a point
 * that never was a candidate is unspecified), the alive flags (n bytes, 1: a candidate), the last distance
 * column the chain computed (n doubles: that of the last point picked), cur (the index that column belongs
 * to), tie and selected[0 .. k).  *n and *k: the sizes of that selection; every pointer may be NULL, so a
 * first call can ask for the sizes alone.  Waits for the context's stream, launches nothing and steers
 * nothing.  A test of the chain has to see every pick, not only the last (tests/test_gpu_furthest_sum.py
 * calls aa_furthest_sum with extra_steps = 0, 1, 2, ... and reads the state after each).  The reference has
 * no counterpart (its list is a local of furthest_sum).  AA_ERR_STATE when no selection has run since the
 * last install. */
int aa_get_furthest_sum_state(aa_ctx *ctx, long *n, int *k, double *sums, unsigned char *alive, double *column,
                              int *cur, int *tie, int *selected);

/* GPNH restarts side by side (the drivers' n_init loop, bin/run_jra55_pca_gpnh.py:112-138):
 * R independent fits of k components each share one set of device arrays (R k <= 64) and every launch
 * of an outer iteration -- restart r lives in component slots [r k, (r + 1) k).  Every restart gets
 * the bits it gets from aa_gpnh_iterate on its own.
 *   aa_gpnh_slots_begin   R empty slots; gp / qp as for aa_gpnh_iterate (both updates on)
 *   aa_gpnh_slots_load    start factors of a restart into slot r (W': k x p, leading dimension ld;
 *                         Z: n x k), its initial cost
 *   aa_gpnh_slots_run     n_iters outer iterations of every slot; status[R] out.  A slot stops by its
 *                         own stopping rule / monotonicity check / iteration cap; its factors of that
 *                         iteration are kept while the others go on
 *   aa_gpnh_slots_fetch   factors, cost record (2 (stop_iter + 1) values) and initial cost of a
 *                         stopped slot; the slot can then be loaded again
 *   aa_slots_end          (shared with the AA slots below) leaves the slot mode: the context must be
 *                         ended -- or destroyed -- before it is used for single fits again; a begin
 *                         call of either slot mode resets whatever an earlier, un-ended one left */
typedef struct {
    int stop, converged, error_stage, stop_iter;
    int flags;              /* GPNH slots: nonzero when the slot's normal equations were not positive definite;
                             * AA slots: the slot's SPG warning flags (AA_SPG_FLAG_* bits) */
    int iterations_run;     /* outer iterations this slot has been through since it was loaded */
} aa_slot_status;
int aa_gpnh_slots_begin(aa_ctx *ctx, int R, int k, const aa_gpnh_params *gp, const aa_qp_params *qp);
int aa_gpnh_slots_load(aa_ctx *ctx, int r, const double *Wt, long ld, const double *Z);
int aa_gpnh_slots_run(aa_ctx *ctx, int n_iters, aa_slot_status *status);
int aa_gpnh_slots_fetch(aa_ctx *ctx, int r, double *Wt, long ld, double *Z, double *costs, double *cost0);

/* The same for archetypal analysis (bin/run_hadisst_aa.py:149-174; archetypal_analysis.py:534-670 per
 * restart): R fits of k components in the component slots of one set of arrays (R k <= 32), production
 * settings only (data form, one SPG iteration per dictionary update, fewer than 65 536 samples,
 * k <= 16, single rank).  aa_slots_begin + aa_slots_load x R start the first restarts together;
 * aa_slots_run iterates every slot and reports its status (a stopped slot's factors of that iteration
 * are kept while the others go on); aa_slots_fetch returns a stopped slot's factors, cost record and
 * C X -- recomputed from the fetched C, or (carried != 0) as the loop carried it at the stopping
 * iteration, which is what aa_get_archetypes returns after an aa_iterate that stopped on the last
 * iteration of a batch; aa_slots_reload puts the next restart into the freed slot (its first dictionary
 * update is the cold one of a fit, the running slots keep the products they carry);
 * aa_slots_end returns the context to single fits (from either slot mode: it also ends a run begun with
 * aa_gpnh_slots_begin).  status[r].flags carries the slot's SPG warning flags (AA_SPG_FLAG_*).  Every
 * restart gets the bits aa_iterate gives it on its own. */
int aa_slots_begin(aa_ctx *ctx, int R, int k, const aa_iter_params *loop, const aa_spg_params *spg,
                   const aa_qp_params *qp, const aa_spg_params *scale_spg /* loop->delta != 0 */);
int aa_slots_load(aa_ctx *ctx, int r, const double *C, long ldc, const double *Z, const double *alpha /* k, or NULL: ones */);
int aa_slots_run(aa_ctx *ctx, int n_iters, aa_slot_status *status);
/* a new restart into slot r of a RUNNING group (its previous occupant has stopped and been fetched): the
 * other slots keep the products they carry; the slot's next dictionary update is the cold one of a fit */
int aa_slots_reload(aa_ctx *ctx, int r, const double *C, long ldc, const double *Z, const double *alpha);
int aa_slots_fetch(aa_ctx *ctx, int r, double *C, long ldc, double *Z, double *CX, long ldx, int carried,
                   double *costs, double *cost0, double *alpha /* k scale factors out, nullable */);
int aa_slots_end(aa_ctx *ctx);

/* ------------------------------------------------------------------ GPNH */
/* Dictionary W (p x k) is passed transposed, Wt (k x p, leading dimension ld).
 * aa_gpnh_set_factors uploads Wt and/or Z (either may be NULL to keep the current
 * one) and, when Wt is given, computes XW = X W (n x k).
 * Replaces gpnh_convex_coding.py:292,352 (WtXt) and :270 (XW). */
int aa_gpnh_set_factors(aa_ctx *ctx, int k, const double *Wt, long ld, const double *Z);
int aa_gpnh_get_weights(aa_ctx *ctx, double *Z);
/* Z'X (k x p, summed over ranks), Z'Z (k x k), and tr(W'X'Z) = sum(XW * Z).
 * Replaces gpnh_convex_coding.py:219 (ZtX), :293,:374 (ZtZ), :303,:355,:376. */
int aa_gpnh_reduce(aa_ctx *ctx, double *ZtX, long ld, double *ZtZ, double *trace_WtXtZ);
/* QP update of the weights: A = WtW (k x k, host-supplied), b_t = -XW[t].
 * Replaces _update_gpnh_weights (gpnh_convex_coding.py:254-279). */
int aa_gpnh_weights_update(aa_ctx *ctx, const double *WtW, const aa_qp_params *params,
                           aa_qp_stats *stats);
/* 0.5 ||X - Z W'||_F^2 / n in residual form: _gpnh_cost (gpnh_convex_coding.py:199-210)
 * without the penalty term (added on the host). */
int aa_gpnh_residual_cost(aa_ctx *ctx, double *cost);

/* Reconstruction scores of the drivers' validation branch (bin/run_hadisst_aa.py:235-241, :285-290,
 * :325-366: inverse_transform, then mean_squared_error(data, reconstruction, squared=False) on the host):
 * with R = X - Z W' on the resident matrix (never stored),
 *   col_sse[q] = sum_t R[t][q]^2 (p values), row_sse[t] = sum_q R[t][q]^2 (n values), *sse = sum of all;
 * every output is nullable, float64.  One pass over X with the product on the f64 matrix cores
 * (csrc/kernels_tall.hip: k_residual_scores), float64 arithmetic in both context dtypes, fixed summation
 * orders (two calls return the same bits).  Preconditions of aa_gpnh_residual_cost (data form,
 * aa_gpnh_set_factors has set Wt and Z -- the state ArchetypalAnalysis.transform leaves behind), whose
 * value is 0.5 * sse / n.  Single rank: a context with a communicator is refused with AA_ERR_ARG. */
int aa_gpnh_residual_scores(aa_ctx *ctx, double *col_sse, double *row_sse, double *sse);

/* ------------------------------------------------------------ KernelAA.transform */
/* Weights of new samples y for a fitted kernel model (dictionary C, scale factors alpha, D = diag(alpha) C):
 * the per-sample simplex QPs of ArchetypalAnalysis.transform (archetypal_analysis.py:1151-1199) in kernel
 * form, A = D K D' and b_y = -D kappa(X_train, y).  The context's data matrix (aa_set_data, data form) holds
 * what the linear terms are computed from, the weights go through aa_gpnh_set_factors (Z only) and
 * aa_gpnh_weights_update (A), and the cost is aa_kernel_transform_cost.
 *
 * aa_set_rbf_reference: the implicit RBF kernel exp(-gamma ||y - x||^2).  The data matrix holds the new
 *   samples Y (m x p, float64 context); XS (s x p, leading dimension ld) are the training rows in the support
 *   of D, V (s x k, leading dimension ldv) = D' restricted to them.  Sizes the factor buffers for k
 *   components (like aa_gpnh_set_factors).  Single rank, as aa_set_rbf_features.
 * aa_rbf_cross: XW[r][i] = sum_c exp(-gamma max(|y_r|^2 + |x_c|^2 - 2 y_r.x_c, 0)) V[c][i] into the buffer
 *   aa_gpnh_weights_update reads (b = -XW), never forming the m x s kernel: both products on the f64
 *   matrix cores (csrc/kernels_gemm.hip: k_rbf_cross_mfma), column splits summed in a fixed order;
 *   XW (nullable) receives a copy.
 *   Replaces the kernel evaluation behind B = D kappa(X, Y) of the reference's transform (:1180-1190).
 * aa_kernel_transform_cost: 0.5 sum_t (d_t + 2 w_t.b_t + w_t' A w_t) / m from the resident weights and
 *   linear terms, A (k x k, host), d = kappa(y_t, y_t) (m values, host; NULL: 1 for every row, the RBF
 *   kernel); one deterministic reduction.  The transform analogue of the kernel-form cost
 *   (archetypal_analysis.py:200-217, :411-422), which aa_gpnh_residual_cost (data space) is not. */
int aa_set_rbf_reference(aa_ctx *ctx, int k, const double *XS, long s, long p, long ld, const double *V, long ldv,
                         double gamma);
int aa_rbf_cross(aa_ctx *ctx, double *XW /* nullable: m x k copy of the result, row-major */);
/* aa_set_poly_reference / aa_poly_cross: the same pair for the polynomial kernel of aa_set_poly_features,
 *   XW[r][i] = sum_c (gamma y_r.x_c + coef0)^degree V[c][i] (k_poly_kv_mfma, the kernel of the fit).  The
 *   diagonal aa_kernel_transform_cost needs is d_t = (gamma |y_t|^2 + coef0)^degree.  Argument checks as
 *   aa_set_poly_features. */
int aa_set_poly_reference(aa_ctx *ctx, int k, const double *XS, long s, long p, long ld, const double *V, long ldv,
                          double gamma, double coef0, int degree);
int aa_poly_cross(aa_ctx *ctx, double *XW /* nullable: m x k copy of the result, row-major */);
int aa_kernel_transform_cost(aa_ctx *ctx, const double *A, const double *diag, double *cost);
/* aa_kernel_sample_residuals: the terms of that cost per sample (csrc/kernels_tall.hip:
 *   k_kernel_sample_residuals, A in LDS): r_t = d_t - 2 w_t.XW_t + w_t' A w_t for every resident sample t, the
 *   squared feature-space distance of kappa(y_t, .) from its reconstruction; XW is the linear-term buffer the cross
 *   product or aa_gpnh_set_factors left behind.  sample_sse (n values, nullable) receives r_t -- not clamped, it
 *   may be negative at rounding level --, diag_out (n values, nullable) d_t, sums[0] = sum_t r_t and sums[1] =
 *   sum_t d_t, both reduced in a fixed order (a tree per block of 256 samples, the block partials in block order,
 *   no atomics: two calls return the same bits).  diag_kind says where d_t comes from:
 *     AA_DIAG_GIVEN   diag[t], a host vector of n values (explicit kernels);
 *     AA_DIAG_ONES    1 (RBF);
 *     AA_DIAG_POLY    (gamma |y_t|^2 + coef0)^degree with the parameters of aa_set_poly_reference, evaluated by
 *                     the device's one polynomial function on row norms computed on the device;
 *     AA_DIAG_LINEAR  |y_t|^2.
 *   `diag` must be NULL unless diag_kind is AA_DIAG_GIVEN.  POLY and LINEAR read the stored float64 data matrix
 *   (AA_ERR_STATE otherwise).  Preconditions of aa_kernel_transform_cost, which stays what it is. */
#define AA_DIAG_GIVEN  0
#define AA_DIAG_ONES   1
#define AA_DIAG_POLY   2
#define AA_DIAG_LINEAR 3
int aa_kernel_sample_residuals(aa_ctx *ctx, const double *A, int diag_kind, const double *diag, double *sample_sse,
                               double *diag_out, double sums[2]);

/* ------------------------------------------------------------ the two passes, on their own */
/* The two contractions against the resident matrix that every update is built from, callable
 * with caller-supplied small operands (unit tests of the pass kernels against X.dot(...) in
 * float64; the reference's C.dot(X), X.T.dot(Z) at archetypal_analysis.py:614,627 and
 * CX.dot(X.T), X.dot(XtZ) at :615,628):
 *   aa_pass_reduce_rows: out[k][p] (ld = ldo) = A' X,  A host n x k row-major (tall operand);
 *   aa_pass_row_local:   out[n][k]            = X B',  B host k x p row-major (ld = ldb).
 * Both size the context's factor buffers for k components (like aa_set_state) and leave the
 * solver state invalid (aa_set_state / aa_prepare must follow before any update). */
int aa_pass_reduce_rows(aa_ctx *ctx, int k, const double *A, double *out, long ldo);
int aa_pass_row_local(aa_ctx *ctx, int k, const double *B, long ldb, double *out);
/* aa_pass_reduce_rows through the path of an operand that is expected to be zero in most rows (what
 * the dictionary update does with its search direction, option "reduce_sparse"): for finite X the result
 * equals aa_pass_reduce_rows(A) bit for bit, whatever A holds -- an entry of X that is Inf or NaN
 * contributes NaN to the dense pass even against a zero row of A and nothing here (and the equality
 * assumes that the matrix cores keep a subnormal accumulator through a step with a zero operand, as
 * measured: profiles/reduce_sparse_ab.txt).  With
 * reduce_sparse = 0, or float64 data with f64_mfma = 0, this IS the dense pass. */
int aa_pass_reduce_rows_flagged(aa_ctx *ctx, int k, const double *A, double *out, long ldo);
/* The row slabs of the context's most recent flagged reduce-over-rows call (aa_pass_reduce_rows_flagged,
 * or the D'X pass of the latest dictionary update): out[0] = slabs served by the gather kernel, out[1] =
 * slabs left to the dense kernel.  Waits for the context's stream.  Both 0 before the first such call. */
int aa_reduce_sparse_counts(aa_ctx *ctx, long out[2]);

/* Diagnostics: the scalar state of the latest dictionary SPG iteration (device-resident, see
 * csrc/aa_internal.h: ScalarSlot), copied to out[0..AA_SPG_SCALARS).  Layout: 0 tr, 1 tr(C HD),
 * 2 tr(M C K C'), 3 f_old, 4 f_new, 5 alpha (BB / first step), 6 alpha_set, 7 lambda,
 * 8 <d,g>, 9 <d,d>, 10 tr(D HD), 11 a1, 12 a2, 13 <d,g_new>, 14 ||res||^2, 15 ||res||_inf,
 * 16 n_feval, 17 flags, 18 projection multiplier, 19 max|P(x-g)-x|, 20 divisor of f.
 * After an update that skipped the SPG tail (option "spg_tail"; aa_spg_path ends in "tail:skip") 13, 14, 15
 * and 19 are STALE -- what the latest update with a tail left --, 5 is the step length the update used, not the
 * BB step behind it, and 17 lacks CONVERGED / MAX_FEVAL. */
#define AA_SPG_SCALARS 21
int aa_get_spg_scalars(aa_ctx *ctx, double *out);

/* ------------------------------------------------------------ measurement */
/* Time `reps` launches of one hot-path GEMM kernel with HIP events on the
 * context's stream.  which: 0 = reduce-over-rows (C X, X'Z; k x p out),
 * 1 = row-local (CX X', X X'Z; n x k out), 2..5 = a plain streaming read of X (the read
 * bandwidth the memory system delivers; reference point for the roofline) with 4 / 8 / 16 / 8
 * loads in flight per thread on 4096 / 2048 / 1024 / 8192 blocks; 6 / 7 = the load pattern
 * of the row-local kernel alone, from the row-major matrix / from a tiled view of the same bytes;
 * 8 = K Z of the implicit kernel (k_rbf_kv after aa_set_rbf_features, k_poly_kv_mfma after
 * aa_set_poly_features; + aa_set_state),
 * 9 = the cross product of aa_rbf_cross / aa_poly_cross (a context after aa_set_rbf_reference /
 * aa_set_poly_reference),
 * 10 = the scores pass of aa_gpnh_residual_scores, 11 = the residual pass of aa_gpnh_residual_cost (both
 * without the copy to the host; a context after aa_gpnh_set_factors with dictionary and weights),
 * 12 = the flagged reduce-over-rows sequence (flags, gather, gated dense; no finish) on whatever the
 * direction buffer holds (after aa_pass_reduce_rows_flagged or an update; with reduce_sparse = 0 the
 * dense kernel on the same operand),
 * 13 = the row gather of aa_set_data_take on the context's own matrix (a seeded permutation of all its rows, into a
 * scratch copy), 14 = the feature build of aa_set_poly_features_resident from it (into a scratch buffer); both
 * need only a stored data matrix.  15 = the weighted column sums of aa_data_weighted_column_sums with 16 coefficient
 * rows, 16 = the squared-deviation form of aa_data_grouped_sqdev (rows labelled r mod 12), both with their finish
 * kernel and without the copies; 17 = the model copy of aa_set_data_rows_model in its anomalies form (a 12-row shift
 * table and the trend) from the context's own matrix into a scratch copy; a stored data matrix is all they need.
 * 18 / 19 = the Gram matrix of aa_data_gram by rows / by columns (uncentred: a zero shift table costs the same) with
 * its finish kernel where gram_plan splits, without the copy to the host (the side's d <= 8192); 20 = the projection
 * of aa_set_data_projected onto 167 components (a zero V) from the context's own matrix into a scratch block of the
 * context's element type; a stored data matrix is all they need.
 * 21 = the per-slot sums of aa_data_slot_sums, 22 = their squared-deviation form (a zero centre table), both with
 * their finish kernel and without the copies; 23 = the copy of aa_set_data_rows_slots with a shift table from the
 * context's own matrix into a scratch copy; all three with the rows labelled r mod 366, and a stored data matrix is
 * all they need.
 * ms_avg = average duration of one launch in milliseconds. */
int aa_time_kernel(aa_ctx *ctx, int which, int reps, double *ms_avg);
/* In-context timing of the two pass kernels: while enabled, every launch of the
 * reduce-over-rows / row-local GEMM kernel is bracketed by a HIP event pair on the
 * context's stream.  Each call returns the average duration (ms) and the number of
 * launches recorded since the previous call, clears them, and sets the mode to `enable`. */
int aa_gemm_timing(aa_ctx *ctx, int enable, double *ms_reduce_rows, int *n_reduce_rows,
                   double *ms_row_local, int *n_row_local);
/* Names of the kernels the context's most recent reduce-over-rows and row-local passes were
 * launched with, as "reduce;row_local" (e.g. "k_reduce_rows_f32<1,4>;k_row_local_f32_dma<8>"):
 * the kernels are picked by shard size and dtype (csrc/kernels_gemm.hip: launch_reduce_rows,
 * launch_row_local), and a parity test has to know that it exercised the ones a benchmark times
 * (tests/test_gpu_headline.py).  The reference has no counterpart (NumPy picks its BLAS kernels
 * silently).  Empty names before the first pass.  Returns AA_ERR_ARG if `len` is too small. */
int aa_pass_kernels(aa_ctx *ctx, char *buf, int len);
/* Column simplex projections the context has launched since it was created, by the strategy the
 * launcher picked for each (csrc/kernels_tall.hip: launch_proj): out[0] one kernel with 32 entries
 * per thread (n <= 8192), out[1] the same with 64 (option proj_small = 2, n <= 16 384), out[2]
 * candidate lists, out[3] iterative full passes (option proj_mode = 1, and the multi-rank fallback
 * counts as the list projection it belongs to).  Host-side counters: reading them launches nothing
 * and they steer nothing.  A test of one strategy has to know that it ran that strategy
 * (tests/test_gpu_projection.py).  The reference has no counterpart (one sorted projection). */
int aa_proj_counts(aa_ctx *ctx, long out[4]);
/* The kernels the most recent per-sample QP of a context was launched with (csrc/kernels_qp.hip:
 * launch_qp), in launch order and separated by ';': the first-phase kernel with its template
 * arguments and the pass cap it ran with, then every continuation launch of the wave-per-sample
 * kernel, with ":park=N" where it parks samples beyond N passes for a later stage.  Examples:
 * "k_qp_quad_w3<2,1,0>:cap=24;k_qp_wave<32,1,1>", "k_qp<8,0>:cap=1;k_qp_wave<32,1,1>",
 * "k_qp_quad_w3<1,1,0>:cap=24;k_qp_wave_ord<1>:park=96;k_qp_wave<32,1,1>", "k_qp_row<2>",
 * "k_qp_wave<64,0,1>", "k_qp_project_only<16>".  (A first phase whose cap is max_iterations has
 * no continuation.)  `ctx` NULL: the scratch context that aa_quad_simplex_spg_batch keeps for
 * `device`, which the stateless entry hides.  Empty before the first QP.  A host-side string:
 * reading it launches nothing and it steers nothing.  A test of one mapping has to know that it
 * ran that mapping (tests/test_gpu_qp_kernels.py).  The restart-slot launches are not recorded.
 * Returns AA_ERR_ARG if `len` is too small. */
int aa_qp_kernels(aa_ctx *ctx, int device, char *buf, int len);
/* One device array of the context's latest dictionary update (csrc/solver.hip: dictionary_update), copied
 * to `out` row-major over its valid extent: n x k for the tall arrays, k x k for M, k x p for Q, 16 for f_mem.  `which`:
 *   AA_SPG_ARRAY_G       the current gradient: after an update, that of the point it returned (g_new)
 *   AA_SPG_ARRAY_G_PREV  the gradient before it (g_old of the update's last iteration)
 *   AA_SPG_ARRAY_D       the search direction d of the last iteration
 *   AA_SPG_ARRAY_GR      the raw product behind AA_SPG_ARRAY_G: (C X X')' or (C K)' of the returned point
 *   AA_SPG_ARRAY_GR_PREV the other product buffer: data form, the product behind AA_SPG_ARRAY_G_PREV;
 *                        kernel form, K d (the returned product is the previous one + lambda times this)
 *   AA_SPG_ARRAY_H       X X' Z or K Z, as the update read it
 *   AA_SPG_ARRAY_M       M = D Z'Z D as the set-up formed it (k x k)
 *   AA_SPG_ARRAY_Q       d' X of the last iteration (k x p; data form only)
 *   AA_SPG_ARRAY_FMEM    the line search's history f_mem[0 .. 15] (spg.py:153,198-199; entry 0 is f at the
 *                        start of the last iteration, entries beyond `memory` stay 0)
 * After an update that skipped the SPG tail (option "spg_tail"; aa_spg_path ends in "tail:skip") AA_SPG_ARRAY_G
 * is STALE: the buffer holds an older update's gradient, not that of the returned point (AA_SPG_ARRAY_G_PREV, _D,
 * _GR and the others are the update's own).
 * Waits for the context's stream and side stream, launches nothing and steers nothing.  The element-wise
 * suite of the SPG step compares every kernel's output with the arrays it read
 * (tests/test_gpu_spg_step.py).  The reference has no counterpart (its arrays are NumPy locals of spg()). */
enum { AA_SPG_ARRAY_G = 0, AA_SPG_ARRAY_G_PREV, AA_SPG_ARRAY_D, AA_SPG_ARRAY_GR, AA_SPG_ARRAY_GR_PREV,
       AA_SPG_ARRAY_H, AA_SPG_ARRAY_M, AA_SPG_ARRAY_Q, AA_SPG_ARRAY_FMEM };
int aa_get_spg_array(aa_ctx *ctx, int which, double *out);
/* What the context's latest dictionary update ran, in launch order and separated by ';': the set-up
 * ("cold": factors projected and products recomputed; "warm": products kept, one kernel per step;
 * "fast:k_dict_setup" / "fast:in_grad": one block, on its own or as block 0 of the first gradient launch),
 * then every gradient launch ("k_grad<KP>:nb=blocks:rpb=rows per block") and every line search with its
 * template argument and grid: "k_gram_wide_pq_mfma<32>:nb=17:cpb=128;k_linesearch_fin" (fused; also
 * "k_gram_wide_pq<KP>"), "k_gram_wide<32>x2;k_scalar_stage" (data form, fuse_finalize = 0),
 * "k_gram_tall<64>x3;k_scalar_stage" (kernel form).  An iteration that ran its tail ends with the gradient launch
 * of g_new; one that skipped it (option "spg_tail") ends with "tail:skip" in that place.  The string holds 511 characters: from the first entry
 * that does not fit on, entries are dropped.  A host-side string: reading it launches nothing and it steers
 * nothing.  A test of one path has to know that it ran that path (tests/test_gpu_spg_step.py).  The
 * restart-slot launches are not recorded.  The reference has no counterpart (one code path).  Empty before
 * the first update.  Returns AA_ERR_ARG if `len` is too small. */
int aa_spg_path(aa_ctx *ctx, char *buf, int len);

#ifdef __cplusplus
}
#endif
#endif /* AA_HIP_H */

/* daliid.h -- C ABI of libdaliid_hip.so: the MI355X (gfx950) kernels under the DaliID Person-ReID
 * hot path (embedding train step + gallery distance / CMC-mAP evaluation).
 *
 * The reference (Gabrielcb/DaliID) is pure Python and has NO FFI of its own; its "plugin interface"
 * for this path is the Python module surface mainKIT.py consumes.  Each entry point
 * below cites the reference call it stands under (paths relative to Person-ReID/).  The Python mirror
 * in daliid_amd/ binds these with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (DALI_OK) or a negative dali_status; dali_last_error() gives the
 *     message of the calling thread's last failure.  Nothing throws across the boundary.
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller (PyTorch) owns every
 *     buffer.  The library only owns the opaque dali_ctx (a grow-only device workspace) and net plans.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued there, nothing synchronises.
 *   - bf16 tensors are passed as uint16_t* (raw bits).  Activations are NHWC.
 */
#ifndef DALIID_H
#define DALIID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DALI_OK = 0,
    DALI_ERR_INVALID = -1,   /* null pointer, bad shape / alignment / enum */
    DALI_ERR_HIP = -2,       /* a HIP runtime call failed */
    DALI_ERR_NOMEM = -3,     /* workspace allocation failed */
    DALI_ERR_LIMIT = -4,     /* a documented capacity limit was exceeded */
    DALI_ERR_UNSUPPORTED = -5
} dali_status;

typedef struct dali_ctx dali_ctx;

/* ---- context ---------------------------------------------------------------------------------- */
int dali_version(void);
const char* dali_last_error(void);
/* One context per process / GPU and per stream that may run beside another: `device` is the HIP device ordinal.  A context owns one
 * grow-only workspace block that its calls use from offset 0 (Adam's partial sums, the resize's intermediate image, the distance
 * pre-pass, the class targets), so two calls on the SAME context must not overlap in time: enqueue them on one stream, or give the
 * second stream its own context (the Python side does: `_lib.ctx(device, lane="side")` for the input pipeline's side stream). */
int dali_ctx_create(int device, dali_ctx** out);
int dali_ctx_destroy(dali_ctx* ctx);
/* Pre-size the workspace (hipMalloc happens here, not inside later calls / graph captures). */
int dali_ctx_reserve(dali_ctx* ctx, size_t bytes);

/* ---- evaluation path: validateModels.validate (validateModels.py:35-58) ------------------------- */
typedef enum { DALI_METRIC_COSINE = 0,   /* 1 - q.g         validateModels.py:47, evaluate.py:291 */
               DALI_METRIC_L2SQ = 1,     /* |q|^2+|g|^2-2q.g  (square of the commented cdist, :45) */
               DALI_METRIC_DOT = 2       /* q.g : the similarity GEMMs of the loss heads (losses.py:62, :277) */
} dali_metric;
typedef enum { DALI_PREC_BF16X3 = 0,     /* split-bf16 (hi*hi+hi*lo+lo*hi), fp32 accumulate: ~1e-6 abs */
               DALI_PREC_BF16 = 1        /* single bf16 product, fp32 accumulate: ~1e-4 abs on unit rows */
} dali_precision;
/* pooling of the embedding head: the `feature` attribute eval scripts set through model.module
 * (evaluateCleanATModels.py:249-256, :335-340); training always uses BOTH (Encoders.py:341-345). */
typedef enum { DALI_FEATURE_BOTH = 0, DALI_FEATURE_GAP = 1, DALI_FEATURE_GMP = 2 } dali_feature;

/* y = x / (|x|_2 + eps), rows of an fp32 [n,d] matrix.
 * validateModels.py:41-42 (eps = 0) and train_encodersKIT.py:198 (eps = 1e-9).
 * y may alias x.  norms (nullable) receives |x|_2 per row. */
int dali_l2norm_rows(dali_ctx* ctx, void* stream, const float* x, int n, int d, float eps,
                     float* y, float* norms);
/* Backward of the above: dx = dy/(n+eps) - x*(x.dy)/(n*(n+eps)^2); needs the forward INPUT x. */
int dali_l2norm_rows_bwd(dali_ctx* ctx, void* stream, const float* x, const float* dy, int n, int d,
                         float eps, float* dx);

/* out[nq,ng] (fp32, row-major) = metric(Q[nq,d], G[ng,d]); fp32 inputs.
 * normalize != 0 fuses the row normalisation of validateModels.py:41-42 into the operand pre-pass
 * (the reference sequence normalise -> 1 - q@g.T becomes one call).
 * Workspace: the two operand images (dali_pairdist_operand_bytes) + (nq+ng)*4.
 * DALI_METRIC_DOT at DALI_PREC_BF16X3 without normalisation on a problem that would fill at most a quarter of the CUs with 128 x 256 tiles
 * (the loss heads' similarity GEMMs, losses.py:62, :277) runs on the fp32 matrix cores instead: exact fp32 products, no operand images, no
 * workspace; Q and G need 4-byte alignment only (any d). */
int dali_pairdist(dali_ctx* ctx, void* stream, const float* Q, const float* G, int nq, int ng, int d,
                  int metric, int precision, int normalize, float* out);

/* The two halves of dali_pairdist, for callers that reuse a prepared gallery against many query sets:
 * prepare: X[n,d] fp32 -> the bf16 operand image the distance kernel reads (dali_pairdist_operand_bytes(n, d, precision) bytes,
 * 16-byte aligned; opaque: DALI_PREC_BF16X3 interleaves the bf16 hi part and the bf16 residual per 32 columns so that one
 * k-step of a row is one 128-byte cache line, DALI_PREC_BF16 pads the row to 64 columns) plus |row|^2 (after the optional
 * normalisation).  Both sides of dali_pairdist_prepared must have been prepared with the same precision. */
size_t dali_pairdist_operand_bytes(int n, int d, int precision);
int dali_pairdist_prepare(dali_ctx* ctx, void* stream, const float* X, int n, int d, int normalize, int precision,
                          void* image, float* sq);
int dali_pairdist_prepared(dali_ctx* ctx, void* stream, const void* q_image, const float* q_sq, const void* g_image,
                           const float* g_sq, int nq, int ng, int d, int metric, int precision, float* out);

/* Two-model distance fusion (evaluateCleanATModels.py:103-160): with inout holding the first model's distmat d1
 * (dali_pairdist), computes the second model's d2 = 1 - q.g on the fly and stores
 *   inout = (w1*d1 + w2*d2) / (w1 + w2),  w_m[q,g] = max(q_mag_m[q], g_mag_m[g])            (:154-157)
 * where the magnitudes are the embedding norms under the chosen pooling (getWeightsByMagnitude :249-256);
 * q_mag_prev/g_mag_prev belong to the first model, q_mag/g_mag to this one.  All four null: w = 1, i.e. the
 * "simple ensemble" (d1 + d2)/2 (:126).  One extra read of the matrix instead of a second matrix + a blend pass. */
int dali_pairdist_blend(dali_ctx* ctx, void* stream, const float* Q, const float* G, int nq, int ng, int d,
                        int precision, int normalize, const float* q_mag_prev, const float* g_mag_prev,
                        const float* q_mag, const float* g_mag, float* inout);

/* market1501-protocol CMC / mAP: the arithmetic of torchreid.metrics.evaluate_rank(distmat, q_pids,
 * g_pids, q_camids, g_camids, use_metric_cuhk03=False) called at validateModels.py:68.
 * ids are int32 codes (the Python mirror factorises the reference's string columns).
 * Exact distance ties are ordered by ascending gallery index.
 * Outputs (device): cmc[max_rank] fp32, mAP[1] fp32 (+ fp64 copy in map64[1], nullable),
 * num_valid[1] int32 (queries with at least one match after junk removal),
 * per-query ap[nq] fp32 and first_rank[nq] int32 (-1 = invalid query) -- both nullable.
 * The gallery is indexed by identity on the device first (counting sort), so the ids are read once per evaluation, not once per
 * query.  Limits, reported through status[0] (device): 1 = a query's identity has more than 4096 gallery entries; 2 = the gallery
 * identity codes span more than 2^20 values (pass dense codes, as the mirror's factorize_ids does). */
int dali_rank_eval(dali_ctx* ctx, void* stream, const float* distmat, const int32_t* q_pids,
                   const int32_t* g_pids, const int32_t* q_camids, const int32_t* g_camids, int nq, int ng,
                   int max_rank, float* cmc, float* mAP, double* map64, int32_t* num_valid,
                   float* ap, int32_t* first_rank, int32_t* status);

/* mINP, the mean inverse negative penalty that AGW / fast-reid style evaluations report next to mAP and Rank-1, under the protocol,
 * key order (distance, gallery index), limits and status codes of dali_rank_eval, whose inputs it takes.  Per query, among the kept
 * gallery entries (junk removed):
 *   n_rel[q]     int32: the number of matches;                 last_rank[q]  int32: 0-based position of the LAST match, -1 = invalid query
 *   inp[q]       fp32 : (float)n_rel / (float)(last_rank + 1), one IEEE fp32 division; 0 for an invalid query
 *   minp64[1]    fp64 : the mean over the valid queries of n_rel / (last_rank + 1) with the quotient taken in fp64 (not of the rounded
 *                       fp32 inp), summed by one workgroup in a fixed order; 0 without a valid query
 *   num_valid[1] int32: queries with at least one match after junk removal.
 * The same two-tier query kernels as dali_rank_eval (which this call leaves bit for bit what it was), keeping the position on which
 * their scan ends.  status[0] as for dali_rank_eval.  Nothing synchronises.  One GPU only: the sharded path has no such entry. */
int dali_rank_eval_inp(dali_ctx* ctx, void* stream, const float* distmat, const int32_t* q_pids, const int32_t* g_pids,
                       const int32_t* q_camids, const int32_t* g_camids, int nq, int ng, float* inp, int32_t* last_rank,
                       int32_t* n_rel, double* minp64, int32_t* num_valid, int32_t* status);

/* Gallery-sharded evaluation over N ranks (validateModels.py:41-47,61-69 with the gallery split across GPUs): each rank holds
 * dist_shard [nq][ng] = the distances of ALL queries to ITS gallery slice, whose first entry has global index g_offset.  Three calls with
 * two collectives of the caller's between them (the mirror: ops_eval.rank_eval_sharded over torch.distributed):
 *   dali_rank_shard_matches -> keys [nq][cap] int64 ((orderable distance bits << 32) | global gallery index; unused slots ~0) and counts [nq]
 *                              of the query's matches inside this shard;            [all-gather keys and counts: rank-major]
 *   dali_rank_shard_bins    -> bins [nq][bins_cap + 1] int32: this shard's kept entries binned by the number of matches (of all shards) with a
 *                              smaller key;                                         [all-reduce SUM of bins]
 *   dali_rank_shard_finish  -> cmc / mAP / per-query ap + first_rank from the summed bins; bit-identical to dali_rank_eval on the whole matrix.
 * cap: an upper bound of a query's matches inside one shard, the same on every rank; bins_cap >= a query's matches over all shards
 * (<= 4096).  status[0] = 1 when either bound is exceeded, 2 as for dali_rank_eval. */
int dali_rank_shard_matches(dali_ctx* ctx, void* stream, const float* dist_shard, const int32_t* q_pids, const int32_t* g_pids,
                            const int32_t* q_camids, const int32_t* g_camids, int nq, int ng, int g_offset, int cap,
                            int64_t* keys, int32_t* counts, int32_t* status);
int dali_rank_shard_bins(dali_ctx* ctx, void* stream, const float* dist_shard, const int32_t* q_pids, const int32_t* g_pids,
                         const int32_t* q_camids, const int32_t* g_camids, int nq, int ng, int g_offset, const int64_t* keys_all,
                         const int32_t* counts_all, int world, int cap, int32_t* bins, int bins_cap, int32_t* status);
int dali_rank_shard_finish(dali_ctx* ctx, void* stream, const int32_t* bins, const int32_t* counts_all, int world, int nq, int bins_cap,
                           int max_rank, float* cmc, float* mAP, double* map64, int32_t* num_valid, float* ap, int32_t* first_rank);

/* k-reciprocal re-ranking (Zhong et al., CVPR 2017; torchreid.utils.re_ranking(q_g_dist, q_q_dist, g_g_dist, k1, k2, lambda_value)),
 * the block validateModels.py:49-53 leaves commented out.  Inputs: the fp32 distance blocks q_g [nq][ng], q_q [nq][nq], g_g [ng][ng]
 * (row-major, device); output: out [nq][ng] fp32 (device).  Enqueued on `stream`, nothing synchronises; scratch in the workspace.
 * With N = nq + ng and A = [[q_q, q_g], [q_g^T, g_g]]^2 (elementwise, fp32):
 *   C = (A / max(A, axis=0))^T                  row i of C = column i of A over its maximum (IEEE fp32 division; the transposed
 *                                               reading is followed literally: the blocks need not be bitwise symmetric)
 *   R[i] = stable argsort of row i of C         exact ties by ascending index; only R[i][:k1+1] is used
 *   KR(i) = {f in R[i][:k1+1] : i in R[f][:k1+1]},  KRh(c) the same with h + 1 neighbours, h = round_half_even(k1 / 2)
 *   E(i) = sorted union of KR(i) and every KRh(c), c in KR(i), with |KRh(c) & KR(i)| > (2.0/3.0) * |KRh(c)| (in double)
 *   V[i, e] = w_e / sum(w), w_e = expf(-C[i, e]) for e in E(i) (sum accumulated in fp64, rounded to fp32 once), 0 elsewhere
 *   k2 != 1: V[i] <- mean of V[R[i][:k2]] (fp32, summed in R order, divided by k2), from the un-expanded V
 *   t = sum_c min(V[i,c], V[j,c]) over ascending c (fp32);  out[i][j-nq] = (1 - t / (2 - t)) * (float)(1 - lambda) + C[i, j] * (float)lambda
 * Preconditions: nq, ng >= 1, 1 <= k1, k1 + 1 <= N, 1 <= k2 <= k1 + 1, 0 <= lambda_value <= 1 (DALI_ERR_INVALID otherwise);
 * k1 <= 63 and ng * (row capacity of V) < 2^31 (DALI_ERR_LIMIT otherwise), where the row capacity is min(N, (k1+1)(h+2)), times k2
 * when k2 != 1.  Workspace: about (2 N + 2 ng) * capacity * 4 bytes.  Bitwise identical results run to run. */
int dali_rerank(dali_ctx* ctx, void* stream, const float* q_g, const float* q_q, const float* g_g, int nq, int ng, int k1, int k2,
                double lambda_value, float* out);

/* Exact ROC curve over every query-gallery pair: sklearn.metrics.roc_curve(labels, scores, pos_label=1) of
 * evaluateCleanATModels.calculateMetrics(pooling=...) (evaluateCleanATModels.py:276-292), by counting (no sort, no vendor library).
 * Inputs (device): distmat [nq][ng] fp32, 16-byte aligned; q_ids [nq], g_ids [ng] int32 codes.  For every pair (i, j):
 *   score s = fl32(1 - fl32(distmat[i][j] / 2)), label y = (q_ids[i] == g_ids[j]); every pair counts (no camera or junk filter).
 * The curve: the distinct scores in descending order (-0 and +0 are one score), with fps / tps = the cumulative negative / positive
 * counts up to and including each score.  drop_intermediate (applied when there are more than 2 points) keeps the first and the last
 * point and every point j where the next point's increment (negatives, positives) differs from point j's, i.e. where np.diff(fps, 2)
 * or np.diff(tps, 2) is non-zero.  The leading (0, 0, +inf) point and the division into rates are the caller's (bitwise sklearn 1.7.2).
 *   dali_roc_scratch_bytes(nq, ng): bytes of the caller-owned scratch, 12 * nq * ng + 16 MiB + min(256, nq * ng, 4096) * 8 MiB (about
 *                            14.1 GB at 1e9 pairs); 0 when the shape is not supported.  256-byte aligned; the library keeps none of it.
 *   dali_roc_build  -> out[5] int64 (device): n_points with drop_intermediate, n_points without, n_pos, n_neg, status (0 ok, 1 = a
 *                      non-finite score, 2 = internal count mismatch).  Nothing synchronises; the scratch then holds the curve.
 *   dali_roc_emit   -> thresholds [n_points] fp32, fps / tps [n_points] int64 of the curve the build left in the scratch (the same
 *                      scratch, unchanged), with or without drop_intermediate; n_points = out[0] or out[1] (writes stop there).
 * Limits: nq, ng >= 1 (DALI_ERR_INVALID); nq * ng <= 2^31 - 1 (DALI_ERR_LIMIT).  Bitwise identical results run to run. */
size_t dali_roc_scratch_bytes(int nq, int ng);
int dali_roc_build(dali_ctx* ctx, void* stream, const float* distmat, const int32_t* q_ids, const int32_t* g_ids, int nq, int ng,
                   void* scratch, size_t scratch_bytes, int64_t* out);
int dali_roc_emit(dali_ctx* ctx, void* stream, const void* scratch, int nq, int ng, int drop_intermediate, int64_t n_points,
                  float* thresholds, int64_t* fps, int64_t* tps);

/* Exact top-k retrieval: the k best entries of every row, the question behind validateBRIAR.calculateMetrics (validateModels.py:79-105,
 * argsort[:, :20]), MSMT17_validator (:179-180, torch.topk) and get_subset_one_encoder (getFeatures.py:337-348).
 * THE ORDER (everything below uses it): ascending by value, exact ties by ascending index; -0.0 equals +0.0; a NaN of either sign comes
 * after +inf, as numpy and torch sort it.  largest != 0 reverses the value order only: ties still go by ascending index and NaN still
 * comes last.  A list is kept as k int64 keys per row, best first: (ordered value bits << 32) | global column index, compared as
 * unsigned; a slot that no column has filled yet (k larger than the columns seen) holds the all-ones key.
 *   dali_topk_rows   x [nq][ncols] fp32 with row pitch ld >= ncols elements (a column slice of a wider matrix; 4-byte alignment is
 *                    enough, 16-byte aligned rows are read faster); column j has global index col_offset + j (< 2^31).  accumulate == 0
 *                    starts keys [nq][k]; accumulate != 0 merges the block into the lists an earlier call left there, so a matrix may
 *                    be fed in column blocks of any widths and gives the lists of the whole.  One read of the block.
 *   dali_topk_decode keys -> values [nq][k] fp32, indices [nq][k] int32.  Values are the selected entries' bits, except -0.0 -> +0.0
 *                    and every NaN -> the quiet NaN 0x7fc00000; an unfilled slot gives index -1 and value +inf (-inf for largest).
 *   dali_pairdist_topk  the same lists for the rows of D = dali_pairdist_prepared(q_image, g_image, metric, precision) WITHOUT the
 *                    matrix: gallery row g has global index g_offset + g, values are bitwise those of D (same kernel, same
 *                    accumulators, same metric arithmetic; its epilogue selects instead of storing).  accumulate as above, so a
 *                    gallery may be fed in slices; slices and images of any size are accepted (images beyond the kernel's 32-bit
 *                    offsets are walked in row ranges).  Method: the first boot_cols gallery rows go through a [nq][boot_cols] block
 *                    of D and dali_topk_rows, which gives every query a threshold (its k-th key); the rest is walked in rounds of
 *                    chunk_cols, 2 chunk_cols, 4 chunk_cols, ... rows, never more than the rows already seen (so that a gallery in
 *                    random order leaves at most k survivors per query and round on average), whose distances are compared with the thresholds in the
 *                    distance kernel's epilogue; the survivors (a fraction k / rows_seen of a gallery in random order) are appended
 *                    to per-query candidate lists of cand_cap keys and merged after the round.  A round in which a list overflows is
 *                    dropped and redone through the block, on the device, so any gallery order gives the exact result.
 *                    boot_cols / chunk_cols (rounded up to multiples of 128) / cand_cap: 0 = defaults (4096, 4096, max(64, 4 k)).
 *                    stats [3] int32 (device, written by this call): gallery rows selected in the epilogue, gallery rows taken through
 *                    the block (the bootstrap included), overflow events.
 *   dali_pairdist_topk_scratch_bytes  the workspace the call takes from the context: the block, the candidate lists and counters;
 *                    independent of ng (its argument is kept for symmetry); 0 for an unsupported shape.
 * Limits: 1 <= k <= 128 and cand_cap <= 1920 (DALI_ERR_LIMIT); indices < 2^31.  Nothing synchronises.  The only atomics are integer slot
 * counters whose order of arrival cannot reach a result (lists are sorted by unique keys): bitwise identical results run to run. */
int dali_topk_rows(dali_ctx* ctx, void* stream, const float* x, int nq, int ncols, int64_t ld, int col_offset, int k, int largest,
                   int accumulate, int64_t* keys);
int dali_topk_decode(dali_ctx* ctx, void* stream, const int64_t* keys, int nq, int k, int largest, float* values, int32_t* indices);
size_t dali_pairdist_topk_scratch_bytes(int nq, int ng, int d, int k, int boot_cols, int chunk_cols, int cand_cap);
int dali_pairdist_topk(dali_ctx* ctx, void* stream, const void* q_image, const float* q_sq, const void* g_image, const float* g_sq,
                       int nq, int ng, int d, int metric, int precision, int k, int largest, int g_offset, int accumulate,
                       int64_t* keys, int boot_cols, int chunk_cols, int cand_cap, int32_t* stats);

/* Query expansion (AQE / alpha-QE) and database augmentation (DBA): the gather-and-combine step.  Every output row is the weighted mean
 * of k pool rows, the neighbour lists being those of dali_pairdist_topk (so no similarity matrix exists at any size); the mirror's
 * ops_eval.query_expansion composes prepare -> top-k -> combine, `times` times.
 *   pool [n_pool][d] fp32   the rows that are gathered (the un-normalised current features)
 *   idx  [n][k] int32, val [n][k] fp32   row-major neighbour lists; val is a similarity, or a cosine distance when val_is_distance != 0
 *   out  [n][d] fp32        must not overlap pool (address ranges are compared: DALI_ERR_INVALID)
 * THE ARITHMETIC, every operation an IEEE fp32 operation rounded to nearest, no fused multiply-add, in this order (a numpy float32
 * emulation reproduces it bit for bit).  For row i, element c:
 *   s_j = val_is_distance ? 1.0f - val[i][j] : val[i][j]
 *   w_j = 1.0f when alpha == 0, else ((s_j * s_j) * s_j) ...         alpha - 1 multiplications, left to right (a negative similarity
 *                                                                    keeps its sign for odd alpha: no clamp, no powf)
 *   acc = 0.0f;  for j = 0 .. k-1 ascending:  acc = acc + (w_j * pool[idx[i][j]][c])
 *   out[i][c] = acc * (1.0f / (float)k)                              the reciprocal rounded once
 * An index < 0 or >= n_pool is never dereferenced: its term is skipped (the divisor stays k) and status[0] (device int32) is raised to 1
 * with atomicMax.  The call never clears status: the caller zeroes it, and one word may collect several calls.
 * Refused before any launch (DALI_ERR_INVALID, the message names the value): k < 1, k > 128, alpha outside 0..16, d < 1, a null
 * pointer, out overlapping pool, and n_pool < 1 with n > 0.  n == 0 launches nothing.  Rows are read 16 bytes per lane when d % 4 == 0
 * and pool and out are 16-byte aligned, 4 bytes per lane otherwise (4-byte alignment is required).  No atomics on out: bitwise
 * identical results run to run.  Nothing synchronises; no workspace. */
int dali_qe_combine(dali_ctx* ctx, void* stream, const float* pool, int n_pool, int d, const int32_t* idx, const float* val, int n, int k,
                    int val_is_distance, int alpha, float* out, int32_t* status);

/* Template (set) evaluation: a set of rows -- the frames of a tracklet, the media of a subject, the images of a multi-query -- stands for
 * one search unit (BRIAR templates, MARS tracklets, Market-1501 multi-query).  Three kernels that read their input once; the mirror's
 * ops_eval.pool_templates / link_templates / open_set_metrics compose them.  All pointers are device pointers, 4-byte aligned; nothing
 * synchronises; no workspace; no atomics on floats: bitwise identical results run to run, whatever the launch geometry.
 * order / bounds are device data these entries cannot inspect.  The kernels compare every row number and bound with its range before it
 * becomes an address; what lies outside is skipped and reported in status[0] (device int32, OR-ed with 1 = a row number outside [0, n),
 * 2 = bounds that do not increase inside their range).  The calls never clear status: the caller zeroes it.
 *
 *   dali_pool_rows   feature-level pooling.  fvs [n][d] fp32; order [n] int32 row numbers grouped by template and bounds [n_templates + 1]
 *                    int32, strictly increasing from 0 to n (the convention of dali_class_targets): template t owns
 *                    order[bounds[t] .. bounds[t+1]), its members in that order; weights (nullable; mode 0 only) fp32 [n] indexed by ROW
 *                    number; out [n_templates][d] fp32, not overlapping fvs.  Every operation is an IEEE fp32 operation rounded to nearest,
 *                    no fused multiply-add.  For template t, element c, members r_0, r_1, ... in member order:
 *                      mode 0 (weighted mean)  acc = 0.0f; wsum = 0.0f;
 *                                              for i ascending:  acc = acc + (w_i * fvs[r_i][c]);  wsum = wsum + w_i      (w_i = weights[r_i])
 *                                              out[t][c] = acc / wsum
 *                                              without weights every w_i is 1.0f and the divisor is (float)count.  ONE running sum per
 *                                              element over the whole template, however long: the order depends on neither the launch
 *                                              geometry nor n_templates.
 *                      mode 1 (max)            acc = -inf;  for i ascending:  acc = fvs[r_i][c] > acc ? fvs[r_i][c] : acc   (a NaN is never
 *                                              taken; of +0.0 and -0.0 the one met first stays)
 *                    Rows are read 16 bytes per lane when d % 4 == 0 and fvs and out are 16-byte aligned, 4 bytes per lane otherwise.
 *                    A template with bad bounds gets a zero row.  Refused before any launch (DALI_ERR_INVALID): a mode other than 0 / 1,
 *                    d < 1, n < 1, n_templates outside 1 .. n (an empty template cannot exist then), weights with mode 1, a null or
 *                    misaligned pointer, out overlapping fvs.
 *   dali_segment_reduce2d  score-level linkage.  x: rows x cols fp32 read by its pitch ld >= cols; row_bounds [n_row_segs + 1] and
 *                    col_bounds [n_col_segs + 1] int32: contiguous segments, strictly increasing, covering 0 .. rows and 0 .. cols.
 *                    out[out_row0 + a][out_col0 + b] (out: out_rows rows of pitch out_ld; entries outside the block are not touched) =
 *                    the min (mode 0) / max (mode 1) / mean (mode 2) of the sub-matrix rows(a) x cols(b).
 *                      min / max  in the total order of the bit patterns: -0.0 below +0.0, a NaN beyond the infinity of its sign.  No
 *                                 result depends on the order of the entries; the result is one of the entries, bit for bit.
 *                      mean       for every column j of cols(b):  p_j = x[r_0][j];  for the further rows r ascending:  p_j = p_j + x[r][j]
 *                                 acc = p_{j_0};  for the further columns j ascending:  acc = acc + p_j
 *                                 out = acc / (float)(|rows(a)| * |cols(b)|)        (fp32, rounded to nearest, as above)
 *                    Refused before any launch: a mode other than 0 / 1 / 2, rows or cols < 1, ld < cols, a segment count outside
 *                    1 .. rows / 1 .. cols, an output block that does not lie inside out, a null or misaligned pointer.
 *   dali_open_set_search   per-probe open-set search of a distance matrix distmat [nq][ng] fp32 read by its pitch ld >= ng; q_subj [nq],
 *                    g_subj [ng] int32 subject codes.  For probe i with mates M = {j : g_subj[j] == q_subj[i]}:
 *                      mate_dist[i]    = min of distmat[i][j] over M; mate_col[i] = the smallest j that attains it.  +inf and -1 for an
 *                                        empty M (a probe that is not mated)
 *                      nonmate_dist[i], nonmate_col[i]   the same over the complement of M; +inf and -1 when it is empty
 *                      rank[i]         = the number of non-mates j with distmat[i][j] < mate_dist[i], or distmat[i][j] == mate_dist[i] and
 *                                        j < mate_col[i]: the 0-based position of the best mate in a stable ascending sort of the row
 *                                        with the other mates removed.  -1 for a probe that is not mated
 *                    Comparisons are IEEE (-0.0 == +0.0); a NaN entry is never a minimum and is never counted.  One pass over the row for
 *                    the minima, a second for the count; no sort.  The row and g_subj are read 16 bytes per lane when distmat and g_subj
 *                    are 16-byte aligned and ld % 4 == 0.  Refused before any launch: nq or ng < 1, ld < ng, a null or misaligned pointer. */
int dali_pool_rows(dali_ctx* ctx, void* stream, const float* fvs, int n, int d, const int32_t* order, const int32_t* bounds, int n_templates,
                   const float* weights, int mode, float* out, int32_t* status);
int dali_segment_reduce2d(dali_ctx* ctx, void* stream, const float* x, int rows, int cols, int64_t ld, const int32_t* row_bounds,
                          int n_row_segs, const int32_t* col_bounds, int n_col_segs, int mode, float* out, int out_rows, int64_t out_ld,
                          int out_row0, int out_col0, int32_t* status);
int dali_open_set_search(dali_ctx* ctx, void* stream, const float* distmat, int nq, int ng, int64_t ld, const int32_t* q_subj,
                         const int32_t* g_subj, float* mate_dist, int32_t* mate_col, float* nonmate_dist, int32_t* nonmate_col, int32_t* rank);

/* Weibull meta-recognition score fusion: libmr.FitHigh / libmr.wscore and Meta_Recognition.metarec / mrfuse (evaluate.py:394-627), the
 * `1.0 - meta_rec.mrfuse(1 - d_backbone, 1 - d_head01, 1 - d_head02)` line evaluate.py:277 leaves commented out.  Every gallery column of a
 * similarity matrix gets a Weibull fitted by maximum likelihood to the tail of its scores, a score becomes its w-score (the Weibull CDF),
 * and up to three models' matrices are blended by w-score weight.  Inputs are fp32 device matrices of FINITE scores, larger = more
 * similar, row-major S [nq][ng].  A non-finite score sets status[0] = 1 in the two calls that take a status (results are then
 * unspecified; nothing faults).  fl32(.) is one rounding to fp32; everything else below is fp64.
 *   dali_mr_kill_transpose  (metarec :597-618) use_columns == 0: in every row of S the topk largest entries -- THE ORDER of dali_topk_rows
 *                    with `largest`: descending value, exact ties by ascending index -- become fl32(s - fl32((float)killscale * s)), +0 at
 *                    killscale = 1.  use_columns != 0: the same for every column over its nq rows (dali_topk_rows on the rows of the
 *                    transposed copy).  Either way the result is written transposed, KT [ng][nq]: a gallery column is a contiguous row.
 *                    S is left unchanged.  status [1] int32.
 *   dali_mr_fit_rows (FitHigh -> _weibullFitting -> _fit :444-447, :487-505, :541-590, translateAmount = 1) for every row of x [nrows][n]
 *                    and a tail size T (metarec: x = KT, n = nq, T = nq - topk - 1):
 *                      tail: the n - T + 1 smallest keys of the row (dali_topk_rows, largest = 0); the last of them is the boundary key,
 *                            small_r its element's value (the T-th largest value), and the tail is every element whose (value, index)
 *                            key is >= the boundary key: exactly T elements, ties included;
 *                      terms: x_t = fl32(fl32(v_t + 1) - small_r), L_t = log((double)x_t), l_t = (double)fl32(L_t)  (the reference takes
 *                            the logarithm in fp32 and the power in fp64);
 *                      Newton: k = 1; at most 100 times: e_t = exp(k L_t), fg = sum e_t, ff = sum e_t l_t, ff' = sum (e_t l_t) l_t,
 *                            f = ff/fg - (sum l_t)/T - 1/k, f' = ff'/fg - (ff/fg)^2 + 1/k^2, k_new = k - f/f'; if |k_new - k| < 1e-6:
 *                            shape = k_new, scale = ((sum exp(k_new L_t))/T)^(1/k_new), stop; else k = k_new.
 *                    Every row stops on its own (the reference's global loop keeps stepping finished rows, which by quadratic convergence
 *                    moves k by less than 1e-11).  A row that does not stop within 100 steps, or meets a non-finite f, f' or k_new, is
 *                    UNFIT: (shape, scale) = (NaN, NaN), counted in status[1].  The reference leaves such rows with (0, 0) or NaN and
 *                    their w-score is then an accident of pow (0.5 for a constant column); here an unfit column has w-score 0, i.e. no
 *                    weight in the fusion.  Outputs: fits [nrows][2] fp64 (shape, scale), small [nrows] fp32, iters [nrows] int32
 *                    (nullable: Newton steps taken), status [2] int32 = {non-finite input, unfit rows}.
 *   dali_mr_wscore   (wscore :449-485) out [nq][ng] fp64: d = max(fl32(fl32(S[i][j] + 1) - small_j), 0),
 *                    w = 1 - exp(-pow((double)d / scale_j, shape_j)); d == 0 gives exactly 0 and so does an unfit column.
 *   dali_mr_fuse     (mrfuse :620-637) m = 1 .. 3 models; scores_host / fits_host / small_host are HOST arrays of m device pointers
 *                    (S_a [nq][ng], fits_a [ng][2], small_a [ng]).  out[i][j] = (sum_a w_a (double)s_a) / (sum_a w_a), summed in model
 *                    order, the w-scores computed in the same kernel and never stored; written as fp64 (out_fp64 != 0) or rounded once
 *                    to fp32.  Where sum_a w_a == 0 exactly the output is the plain mean (sum_a (double)s_a) / m: the reference gives
 *                    0/0 = NaN there, which would poison a ranking.
 * Preconditions (DALI_ERR_INVALID otherwise): topk >= 1, nq >= topk + 2, ng >= topk when use_columns == 0; 1 <= T <= n.  Limits
 * (DALI_ERR_LIMIT): topk <= 128; n - T + 1 <= 128 (the dali_topk_rows cap; metarec: topk <= 126); n <= 16384 (a row's L_t stay in LDS
 * across the Newton steps: 128 KiB of the CU's 160).  Workspace, from the context: the selections' keys only, max(nq or ng rows) * topk
 * * 8 bytes for the kill and nrows * (n - T + 1) * 8 for the fit; KT is the caller's.  Enqueued on `stream`, nothing synchronises; all
 * sums run in a fixed order and the only atomic is the integer count of unfit rows: bitwise identical results run to run. */
int dali_mr_kill_transpose(dali_ctx* ctx, void* stream, const float* S, int nq, int ng, int topk, int use_columns, double killscale,
                           float* KT, int32_t* status);
int dali_mr_fit_rows(dali_ctx* ctx, void* stream, const float* x, int nrows, int n, int tail, double* fits, float* small_out,
                     int32_t* iters, int32_t* status);
int dali_mr_wscore(dali_ctx* ctx, void* stream, const float* S, int nq, int ng, const double* fits, const float* small_in, double* out);
int dali_mr_fuse(dali_ctx* ctx, void* stream, const float* const* scores_host, const double* const* fits_host,
                 const float* const* small_host, int m, int nq, int ng, int out_fp64, void* out);

/* ---- training path: Encoders.ResNet50ReID trunk (Encoders.py:330-339) ----------------------------- *
 * Single-op entry points (the parity tests call these; the net plan below chains the same kernels).
 * Layouts: activations NHWC bf16; forward weights [cout][r][s][cin] bf16; dgrad weights
 * [cin][r][s][cout] bf16; weight gradients [cout][r][s][cin] fp32.  stride in {1,2}.
 * These stand under torch.nn.Conv2d forward/backward of torchvision's resnet50 as wrapped by
 * Encoders.py:312-322. */

/* y[n,ho,wo,cout] = conv(x).  If in_scale/in_shift (fp32 [cin]) are given, x is read as
 * relu?(x*in_scale+in_shift) (the preceding BatchNorm(+ReLU) fused into the operand load; padding stays 0).
 * stats (nullable): fp32 [dali_conv2d_stat_tiles(...)][cout][2] per-tile partial (sum, sum of squares) of the
 * fp32 results -- the batch statistics training-mode BatchNorm needs.  cin % 32 == 0, cout % 4 == 0. */
int dali_conv2d_fwd(dali_ctx* ctx, void* stream, const uint16_t* x, const uint16_t* w, uint16_t* y,
                    int n, int h, int wd, int cin, int cout, int r, int s, int stride, int pad,
                    const float* in_scale, const float* in_shift, int in_relu, float* stats);
/* y = relu?( conv(x) * out_scale[c] + out_shift[c] ): the convolution with the BatchNorm (+ ReLU) that follows it folded into the GEMM's output
 * stage -- the fp32 accumulators are scaled, shifted, clamped and rounded to bf16 once; no raw output, no separate BatchNorm pass.  The inference
 * forward of torchvision's Bottleneck conv1 / conv2 (under Encoders.py:336-339) with scale = gamma / sqrt(running_var + eps),
 * shift = beta - running_mean * scale (getFeatures.py:56-67 forwards in eval mode).  cin % 32 == 0, cout % 8 == 0, stride 1 or 2. */
int dali_conv2d_bn_act(dali_ctx* ctx, void* stream, const uint16_t* x, const uint16_t* w, uint16_t* y, int n, int h, int wd, int cin, int cout,
                       int r, int s, int stride, int pad, const float* out_scale, const float* out_shift, int out_relu);
/* The inference stem in one launch: y = maxpool3x3/2( conv7x7/2(images) * scale[c] + shift[c] ), images fp32 NCHW [n,3,h,w], weight fp32
 * [64][7][7][3] (the net's storage order of the logical OIHW tensor), scale / shift fp32 [64] (bn1 by running statistics; NO ReLU between them and
 * the pool: Encoders.py:321-322, :334), y bf16 NHWC [n, h/4, w/4, 64].  torchvision's conv1 / bn1 / maxpool under Encoders.py:33,36 as
 * getFeatures.py:56-67 forwards them (eval mode): the convolution's output is never stored; rounding points as if it were (bf16 of the
 * convolution's output, fp32 affine, bf16 of the pooled value), so the result equals conv -> bf16 -> affine -> max-pool -> bf16 bit for bit.
 * h % 32 == 0, w in {32, 64, 128} (dali_stem_fused_supported; DALI_ERR_INVALID otherwise -- the net plan then runs the three-launch form). */
int dali_stem_fused_supported(int n, int h, int w);
int dali_stem_conv_bn_maxpool(dali_ctx* ctx, void* stream, const float* images, int n, int h, int w, const float* weight, const float* scale,
                              const float* shift, uint16_t* y);
/* 1x1 convolution (a [pixels][cin] x [cout][cin]^T GEMM) with the fused output stage:
 *   y = gate_{out_mask}( relu?( acc * out_scale[c] + out_shift[c] + bias[c] + res_scale[c] * residual ) ),  bits_out = (y > 0), 1 bit per
 *   element (res_scale: the downsample branch's BatchNorm scale when the residual is its raw convolution output).
 * Forward use: bn3 + identity + ReLU of a bottleneck inside conv3 (Encoders.py:330-339 over torchvision's Bottleneck), with the batch
 * statistics from dali_bnlin_fwd.  Backward use: the masked gradient dz = dy * (y > 0) leaves the data-gradient GEMM directly.
 * Every pointer after `cout` is nullable; cin % 32 == 0, cout % 8 == 0. */
int dali_conv1x1_fused(dali_ctx* ctx, void* stream, const uint16_t* x, const uint16_t* w, uint16_t* y, int pixels, int cin, int cout,
                       const float* out_scale, const float* out_shift, const float* bias, const uint16_t* residual, int out_relu,
                       uint8_t* bits_out, const uint8_t* out_mask, const float* res_scale);
/* y [pixels][cout] = [x1 | x2] @ w^T (+ bias): a 1x1 GEMM whose reduction runs over the c1 channels of x1 followed by the c2 channels of a SECOND
 * tensor x2 (both plain [pixels][c] bf16; w [cout][c1 + c2]).  Two chained data gradients that accumulate into one output become one launch and the
 * partial result is never stored: the conv3 backward of a Gram-scheme bottleneck, d_a2 = dz (A.W3) + W3^T Kc - a2 (W3^T diag(Q) W3)
 * (autograd of torchvision's Bottleneck tail under Encoders.py:330-339).  c1 % 32 == 0, c2 % 32 == 0, cout % 8 == 0; bias nullable. */
int dali_conv1x1_cat(dali_ctx* ctx, void* stream, const uint16_t* x1, int c1, const uint16_t* x2, int c2, const uint16_t* w, const float* bias,
                     uint16_t* y, int pixels, int cout);
/* The same two-operand GEMM with the scale / shift / ReLU output stage: y = relu?( ([x1 | x2] @ w^T) * out_scale[c] + out_shift[c] ) (out_scale
 * nullable = 1).  The inference forward of a bottleneck with a stride-1 downsample branch as ONE launch: with the two BatchNorms' scales folded
 * into the weight image w = [s3.W3 | sd.Wd] and out_shift = shift3 + shift_d this is relu(bn3(conv3(a2)) + bnd(convd(x))) (torchvision Bottleneck
 * under Encoders.py:336-339, eval mode: getFeatures.py:56-67).  c1 % 64 == 0, c2 % 64 == 0, cout % 128 == 0; c1 + c2 <= 256 (any pixel count
 * with at least two 128 x 128 tiles per CU) or c1 + c2 >= 1024 with cout >= 512 and >= 16384 pixels.
 * weight_parts = 2: w is [cout][2 (c1 + c2)] = [W1 hi | W1 lo | W2 hi | W2 lo] with hi = bf16(v), lo = bf16(v - hi): folded fp32 weights to ~2^-17
 * (a single bf16 image of scale-folded weights is a coherent 2^-9 perturbation that the ranking notices); 2 (c1 + c2) <= 256 only. */
int dali_conv1x1_cat_act(dali_ctx* ctx, void* stream, const uint16_t* x1, int c1, const uint16_t* x2, int c2, const uint16_t* w, int weight_parts,
                         const float* out_scale, const float* out_shift, int out_relu, uint16_t* y, int pixels, int cout);
/* Training-mode BatchNorm behind a 1x1 convolution WITHOUT the convolution's output (csrc/bnlin.hip): raw = a W^T is linear in
 * a [P][w] (bf16), so its batch statistics follow from gram = a^T a [w][w] and m2 = colsum(a) [w] (returned, fp32):
 * mean = W m2 / P, E[raw^2] = diag(W gram W^T) / P; ut = (W gram)^T [w][C] (fp32) is returned for the backward, with m2.  Outputs scale = gamma*invstd, shift = beta - mean*scale,
 * mean, invstd [C]; running statistics updated like torch (nullable).  W bf16 [C][w]; C % 8 == 0, w % 32 == 0. */
int dali_bnlin_fwd(dali_ctx* ctx, void* stream, const uint16_t* a, const uint16_t* W, int P, int C, int w, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* gram, float* m2,
                   float* ut, float* scale, float* shift, float* mean, float* invstd);
/* Its backward from the gradient dz [P][C] in front of the BatchNorm output: dW [C][w], dgamma, dbeta, and the two weight images of the
 * data gradient  d_a = dz wd1^T + a wd2^T + bvec  (wd1 = (scale.W)^T [w][C], wd2 = -(W^T diag(Q) W) [w][w], bvec = W^T Kc [w];
 * d_raw = scale dz + Kc - Q raw is nnops.hip's folded form of the BatchNorm backward). */
int dali_bnlin_bwd(dali_ctx* ctx, void* stream, const uint16_t* dz, const uint16_t* a, const uint16_t* W, int P, int C, int w,
                   const float* ut, const float* m2, const float* scale, const float* mean, const float* invstd, float* dW,
                   float* dgamma, float* dbeta, uint16_t* wd1, uint16_t* wd2, float* bvec);
/* rows of the `stats` buffer for a given problem (depends on the tile configuration the launcher will pick). */
int dali_conv2d_stat_tiles(int cout, int cin, int r, int s, int stride, int pad, int n, int ho, int wo, int fused_operand);
/* dx[n,h,w,cin] = conv_transpose(dy, w) (+ residual[n,h,w,cin] if given).  cout % 32 == 0, cin % 4 == 0.
 * residual_mask (nullable; needs cin % 8 == 0): 1 bit per residual element, bit e & 7 of byte e >> 3 over the flat
 * [n,h,w,cin] index, as dali_bn_act writes it for a block output: the residual is added only where the bit is set, i.e.
 * the identity path's dy * (y > 0) of a bottleneck (Encoders.py:330-351 autograd) is formed here, not stored. */
int dali_conv2d_dgrad(dali_ctx* ctx, void* stream, const uint16_t* dy, const uint16_t* wt, uint16_t* dx,
                      const uint16_t* residual, const uint8_t* residual_mask, int n, int h, int wd, int cin, int cout, int r, int s,
                      int stride, int pad);
/* dw[cout][r][s][cin] (fp32) = (accumulate ? dw : 0) + sum_p dy[p][cout] * x_gathered[p][r,s,cin]; x may carry
 * the same fused affine(+ReLU) as the forward.  Deterministic split-K (fixed-order slab reduction). */
int dali_conv2d_wgrad(dali_ctx* ctx, void* stream, const uint16_t* x, const uint16_t* dy, float* dw,
                      int n, int h, int wd, int cin, int cout, int r, int s, int stride, int pad,
                      const float* in_scale, const float* in_shift, int in_relu, int accumulate);

/* BatchNorm2d pieces (torch.nn.BatchNorm2d inside torchvision's Bottleneck, and Encoders.py:333).  Training-mode
 * statistics come from the conv epilogue partials; finalize turns them into scale = gamma/sqrt(var+eps),
 * shift = beta - mean*scale and updates the running statistics exactly like torch (momentum, unbiased var). */
int dali_bn_finalize(dali_ctx* ctx, void* stream, const float* partial, int tiles, int C, double count,
                     const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float momentum, float eps, float* scale, float* shift, float* mean, float* invstd);
/* y = relu?(raw*scale+shift + identity) with identity = identity tensor | raw2*scale2+shift2 | nothing (bottleneck tail).
 * mask_out (nullable, [pixels*C/8] bytes): bit t of byte i = (y[8i+t] > 0), the ReLU mask the backward needs, at 1/16 of
 * y's bytes. */
int dali_bn_act(dali_ctx* ctx, void* stream, const uint16_t* raw, const float* scale, const float* shift,
                const uint16_t* identity, const uint16_t* raw2, const float* scale2, const float* shift2, int relu,
                int64_t pixels, int C, uint16_t* y, uint8_t* mask_out);
/* IBN-a's bn1 + ReLU on an NHWC map (IBN-Net IBN.forward; Bottleneck_IBN: conv1 -> bn1 -> relu).
 * x, y bf16 [n][hw][C]; y may be x.  Channels [0, c_in): per (sample, channel) over the hw pixels
 *   mean = sum x / hw, var = sum (x - mean)^2 / hw (biased), invstd = 1 / sqrt(var + eps),
 *   y = fma(x - mean, invstd * gamma[c], beta[c])     (fp32, then one rounding to bf16)
 * Channels [c_in, C): y = x (the BatchNorm half arrives already affine from the convolution's output stage).
 * relu != 0: max(y, 0) on every channel.  mean, invstd: optional fp32 [n][c_in] outputs (may be NULL).
 * C % 8 == 0, c_in % 8 == 0, 0 < c_in <= C, n >= 1, hw >= 1; anything else DALI_ERR_INVALID before any launch.
 * One launch, no atomics: bitwise reproducible, and a sample's result depends neither on n nor on its place in the batch.  The tensor
 * is read once and written once while hw * min(C, 32) <= 65536 (up to 2048 pixels at 32 channels and more); larger maps are read three times. */
int dali_ibn_act(dali_ctx* ctx, void* stream, const uint16_t* x, int n, int hw, int C, int c_in, const float* gamma, const float* beta,
                 float eps, int relu, uint16_t* y, float* mean, float* invstd);
/* Backward of z = bn(raw) followed by an optional ReLU whose mask is the bit mask ybits (dali_bn_act's mask_out) or
 * (ymask > 0) if one of them is given (they are exclusive), else (raw*scale+shift > 0).  g = gradient after the ReLU.  Writes d(raw) (bf16), dgamma, dbeta; with a second side
 * (raw_b...) the same masked gradient also flows through a second BatchNorm (the downsample branch).  dz_out
 * (nullable, may alias g) receives the masked gradient.  draw_a may alias g when dz_out is null. */
int dali_bn_bwd(dali_ctx* ctx, void* stream, const uint16_t* g, const uint16_t* ymask, const uint8_t* ybits, int relu,
                int64_t pixels, int C,
                const uint16_t* raw_a, const float* mean_a, const float* invstd_a, const float* scale_a, const float* shift_a,
                const uint16_t* raw_b, const float* mean_b, const float* invstd_b, const float* scale_b,
                float* dgamma_a, float* dbeta_a, float* dgamma_b, float* dbeta_b, uint16_t* draw_a, uint16_t* draw_b,
                uint16_t* dz_out);
/* Stem tail (Encoders.py:333-335): out = maxpool3x3/2,pad1( raw*scale+shift ), no ReLU; arg = winning tap 0..8. */
int dali_maxpool_bn_fwd(dali_ctx* ctx, void* stream, const uint16_t* raw, const float* scale, const float* shift, int n, int h,
                        int w, int C, uint16_t* out, uint8_t* arg);
int dali_maxpool_bn_bwd(dali_ctx* ctx, void* stream, const uint16_t* dpool, const uint8_t* arg, const uint16_t* raw,
                        const float* mean, const float* invstd, const float* scale, int n, int h, int w, int C,
                        float* dgamma, float* dbeta, uint16_t* draw);
/* Head (Encoders.py:341-345): f[n,c] = mean_hw x + max_hw x (fp32), and its backward; mode = dali_feature
 * (GAP: mean only, GMP: max only -- evaluateCleanATModels.py:335-340). */
int dali_head_pool_fwd(dali_ctx* ctx, void* stream, const uint16_t* x, int n, int hw, int C, int mode, float* f, int16_t* arg);
int dali_head_pool_bwd(dali_ctx* ctx, void* stream, const float* df, const int16_t* arg, int n, int hw, int C, int mode,
                       uint16_t* dx);
/* Several heads from ONE read of the map (inference outputs: no argmax is kept).  x bf16 [n][h][w][C]; head i pools rows
 * [row_begin, row_end) of the map -- 0,0 = every row -- by mode (dali_feature: mean + max, mean or max) into f[i] of f fp32 [n_heads][n][C].
 * The body parts of mainKIT.ResNet50ReID.forward(multipart=True) (mainKIT.py:251-292) are max heads over rows :8, 4:12 and 8: of the 16-row
 * map.  A head over every row is bitwise what dali_head_pool_fwd writes for the same mode.  heads is a HOST array.
 * DALI_ERR_INVALID: n_heads outside 1..DALI_MAX_HEADS, row_end > h, row_begin >= row_end (unless both 0), a bad mode, C % 8 != 0,
 * h * w >= 32768. */
typedef struct { int32_t mode; int32_t row_begin; int32_t row_end; } dali_head_spec;
#define DALI_MAX_HEADS 8
int dali_head_pool_multi(dali_ctx* ctx, void* stream, const uint16_t* x, int n, int h, int w, int C, const dali_head_spec* heads, int n_heads,
                         float* f);
/* out[r] = sum_c x[r][c], fp32: `torch.sum(x, dim=1)` over an NHWC map, one value per pixel (the activation map of mainKIT.py:294-298).
 * x bf16 [rows][C], C % 8 == 0.  No atomics: bitwise identical run to run. */
int dali_channel_sum(dali_ctx* ctx, void* stream, const uint16_t* x, int64_t rows, int C, float* out);
/* BatchNorm1d neck (Encoders.py:350) on fp32 [n,C]. */
int dali_bn1d_fwd(dali_ctx* ctx, void* stream, const float* x, int n, int C, const float* gamma, const float* beta,
                  float* running_mean, float* running_var, int training, float momentum, float eps, float* y, float* mean,
                  float* invstd);
int dali_bn1d_bwd(dali_ctx* ctx, void* stream, const float* x, const float* dy, int n, int C, const float* gamma,
                  const float* mean, const float* invstd, float* dx, float* dgamma, float* dbeta);

/* ---- TransReID ViT encoder pieces (vit_pytorch.py:120-184, 251-288, 375-408; make_models.py:184-205) -------- *
 * Tokens are [rows = B*T][C] bf16.  Linear layers (nn.Linear / the patch-embedding conv) run on the implicit-GEMM
 * engine: weights bf16 [N][K] (torch layout), the dgrad image is the transpose [K][N]. */
/* y = act(x @ w^T + bias) (+ residual); act 0 none / 1 exact-erf GELU (Mlp, vit_pytorch.py:120-136); pre (nullable)
 * receives the pre-activation.  K % 32 == 0, N % 4 == 0. */
int dali_linear_fwd(dali_ctx* ctx, void* stream, const uint16_t* x, const uint16_t* w, const float* bias, int act,
                    const uint16_t* residual, uint16_t* y, uint16_t* pre, int rows, int K, int N);
/* y = row_scale[row] * act(x @ w^T + bias) (+ residual): a residual branch under DropPath (vit_pytorch.py:45-62, applied at :338),
 * row_scale = the per-sample keep / (1 - p) factors expanded to token rows. */
int dali_linear_fwd_scaled(dali_ctx* ctx, void* stream, const uint16_t* x, const uint16_t* w, const float* bias, int act,
                           const uint16_t* residual, const float* row_scale, uint16_t* y, int rows, int K, int N);
/* dx = (dy @ wt^T) * gelu'(gelu_pre) (+ residual). */
int dali_linear_dgrad(dali_ctx* ctx, void* stream, const uint16_t* dy, const uint16_t* wt, const uint16_t* gelu_pre,
                      const uint16_t* residual, uint16_t* dx, int rows, int K, int N);
/* dw[N][K] fp32 = dy^T @ x; dbias[N] fp32 (nullable) = column sums of dy. */
int dali_linear_wgrad(dali_ctx* ctx, void* stream, const uint16_t* x, const uint16_t* dy, float* dw, float* dbias, int rows,
                      int K, int N);
/* PatchEmbed_overlap (vit_pytorch.py:251-288): images fp32 NCHW -> patches bf16 [B*ny*nx][3*patch*patch] in (c,r,s) order. */
int dali_vit_patchify(dali_ctx* ctx, void* stream, const float* img, int B, int H, int W, int patch, int stride, uint16_t* out);
/* x[b,0] = cls + pos[0]; x[b,1+i] = patch_emb[b,i] + pos[1+i] (vit_pytorch.py:379-391, camera = view = 0), and backward. */
int dali_vit_assemble_tokens(dali_ctx* ctx, void* stream, const uint16_t* patch_emb, const float* cls, const float* pos, int B, int T,
                             int C, uint16_t* x);
int dali_vit_assemble_tokens_bwd(dali_ctx* ctx, void* stream, const uint16_t* dx, int B, int T, int C, float* dpos, float* dcls,
                                 uint16_t* dpatch_emb);
/* SIE (vit_pytorch.py:316-331, 382-387): the token assembly with the side-information term, x[b,t] = (tok + pos[t]) + coef * sie[idx[b]]
 * (fp32, one rounding to bf16); sie fp32 [n_sie][C], idx int32 [B] on the device; an index outside [0, n_sie) adds nothing.
 * sie_grad: dsie[i] = coef * sum over the samples with idx[b] == i (ascending b) and their tokens of dx[b,t], fp32, fixed order (no atomics:
 * bit-identical run to run); unused rows get 0. */
int dali_vit_assemble_tokens_sie(dali_ctx* ctx, void* stream, const uint16_t* patch_emb, const float* cls, const float* pos, const float* sie,
                                 const int32_t* idx, int n_sie, float coef, int B, int T, int C, uint16_t* x);
int dali_vit_sie_grad(dali_ctx* ctx, void* stream, const uint16_t* dx, const int32_t* idx, int B, int T, int C, int n_sie, float coef,
                      float* dsie);
/* JPM (make_models.py:314-377).  gather: features bf16 [B][T][C] + map int32 [G][L] of token indices (device) -> out [G*B][1+L][C], sequence
 * g*B + b, row 0 = the sample's cls token; C % 8 == 0.  head: global fp32 [B][C] and local fp32 [4*B][C] (sequence g*B + b) ->
 * out [B][5C] = cat(global, local_1 / 4, .., local_4 / 4); after != 0: every branch first through its BatchNorm1d by running statistics
 * (gamma / beta / running_mean / running_var fp32 [5][C], eps 1e-5), after == 0: the raw features (the four arrays may be NULL). */
int dali_vit_jpm_gather(dali_ctx* ctx, void* stream, const uint16_t* features, const int32_t* map, int B, int T, int C, int G, int L,
                        uint16_t* out);
int dali_vit_jpm_head(dali_ctx* ctx, void* stream, const float* global_feat, const float* local_feat, const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var, int B, int C, int after, float* out);
/* nn.LayerNorm over C (eps 1e-6 in TransReID); backward optionally adds the residual-stream gradient `add`. */
int dali_layernorm_fwd(dali_ctx* ctx, void* stream, const uint16_t* x, const float* gamma, const float* beta, int rows, int C,
                       float eps, uint16_t* y, float* mean, float* rstd);
int dali_layernorm_bwd(dali_ctx* ctx, void* stream, const uint16_t* g, const uint16_t* x, const float* gamma, const float* mean,
                       const float* rstd, const uint16_t* add, int rows, int C, uint16_t* dx, float* dgamma, float* dbeta);
/* Attention (vit_pytorch.py:152-164): qkv [B*T][3*H*64] -> out [B*T][H*64] = softmax(q k^T * scale) v per head, scores on chip;
 * lse [B*H][T] (row log-sum-exp, natural log; nullable in the forward) feeds the backward, which recomputes the probabilities.
 * head_dim 64 (forward and backward) or 96 (forward only: 64 above stands for head_dim); any other width is refused before a launch
 * ("head_dim must be 64 or 96 (got N)").
 * Forward: 1 <= T <= 1024.  T <= 256 keeps a head's K and V in LDS (one workgroup per batch and head); 256 < T <= 1024 goes to the chunked
 * kernel of dali_attention_fwd_long; beyond 1024 DALI_ERR_LIMIT, nothing launched.  At head_dim 96 every length, through any of the three
 * forward entries, runs the chunked kernel's 96-wide instance (key chunks of 128).  Backward: head_dim 64 and T <= 256 only. */
int dali_attention_fwd(dali_ctx* ctx, void* stream, const uint16_t* qkv, int B, int T, int H, int head_dim, float scale,
                       uint16_t* out, float* lse);
/* The chunked forward on its own, 1 <= T <= 1024 (DALI_ERR_LIMIT beyond): one workgroup per (batch, head, 128 queries) walks the keys in
 * chunks of 256 under an online softmax (running maximum and sum in fp32, probabilities rounded to bf16 unnormalised, one division at the
 * end).  Same operands and layouts as dali_attention_fwd; lse may be NULL.  Not bitwise equal to the T <= 256 kernels.  head_dim 96: chunks
 * of 128. */
int dali_attention_fwd_long(dali_ctx* ctx, void* stream, const uint16_t* qkv, int B, int T, int H, int head_dim, float scale,
                            uint16_t* out, float* lse);
int dali_attention_bwd(dali_ctx* ctx, void* stream, const uint16_t* qkv, const uint16_t* out, const uint16_t* d_out, const float* lse,
                       int B, int T, int H, int head_dim, float scale, uint16_t* dqkv);
/* The forward for short sequences, T <= 64 (the JPM local runs: 33 / 53 / 50 tokens): a 4-tile instance of the same kernel (head_dim 96:
 * the chunked kernel, under the same limit). */
int dali_attention_fwd_short(dali_ctx* ctx, void* stream, const uint16_t* qkv, int B, int T, int H, int head_dim, float scale,
                             uint16_t* out, float* lse);

/* ---- loss heads (train_encodersKIT.py:200-208), fp32 --------------------------------------------------- *
 * S is the similarity matrix fn @ C^T (dali_pairdist with DALI_METRIC_DOT).  labels are int32 codes shared between
 * the batch and the center / proxy label arrays; w[i] is the distortion weight table[samples_distortion[i]]
 * (losses.py:42-52).  Both losses are  sum_i num_i / sum_i den_i  with batch-global sums: *_fwd returns the local
 * sums[2] = {sum num, sum den} (all-reduce them across data-parallel ranks), *_bwd takes the global denominator. */

/* BatchWeightedCenterLoss (losses.py:39-88).  rowstat[nb][4] = {num_i, den_i, argmax_j, max_j softmax}. */
int dali_center_loss_fwd(dali_ctx* ctx, void* stream, const float* S, const int32_t* labels, const int32_t* center_labels,
                         const float* w, float tau, int nb, int NC, float* rowstat, float* sums);
/* dS[nb][NC] = gscale * d(sum num / denom)/dS. */
int dali_center_loss_bwd(dali_ctx* ctx, void* stream, const float* S, const int32_t* labels, const int32_t* center_labels,
                         const float* w, float tau, int nb, int NC, const float* denom, float gscale, float* dS);
/* BatchWeightedProxyLoss (losses.py:273-341).  rowstat[nb][2] = {num_i, den_i}; sel_idx / sel_coef [nb][2*K] hold the
 * selected proxies (K positives then K negatives, -1 padded, K = dali_proxy_kmax()) and d num_i / d S_ij.
 * status[0] != 0 if some row had more than K positives (they are truncated: treat as an error). */
int dali_proxy_loss_fwd(dali_ctx* ctx, void* stream, const float* S, const int32_t* labels, const int32_t* proxy_labels,
                        const float* w, float tau, int nb, int NP, float* rowstat, float* sums, int32_t* sel_idx,
                        float* sel_coef, int32_t* status);
/* dfn[nb][D] (= or +=) gscale/denom * sum_sel coef * proxies[sel][:]. */
int dali_proxy_loss_bwd(dali_ctx* ctx, void* stream, const int32_t* sel_idx, const float* sel_coef, const float* proxies, int nb,
                        int D, const float* denom, float gscale, int accumulate, float* dfn);
int dali_proxy_kmax(void);

/* ---- data parallel: gradient all-reduce over RCCL (xGMI), one communicator per context = per process = per GPU --------------------
 * Replaces nn.DataParallel's reduce of all gradients to GPU 0 (Encoders.py:39-40).  Rank 0 creates the 128-byte id
 * (dali_comm_unique_id) and the host program hands it to the other ranks; every rank then calls dali_ctx_comm_init with the
 * context's device current.  dali_allreduce_bucket: in-place SUM over all ranks of buf[0..count) fp32, enqueued on `stream`
 * (reduce-scatter + all-gather when count divides by the world size, else ncclAllReduce).  RCCL is bound at run time: without it
 * these return DALI_ERR_UNSUPPORTED and everything else works. */
int dali_comm_unique_id(void* id128);
int dali_ctx_comm_init(dali_ctx* ctx, const void* id128, int rank, int world);
int dali_ctx_comm_destroy(dali_ctx* ctx);
int dali_allreduce_bucket(dali_ctx* ctx, void* stream, float* buf, int64_t count);

/* ---- optimizer side of the hot loop, on the flat fp32 storages ------------------------------------------- */
/* torch.optim.Adam step (L2 weight decay added to the gradient; mainKIT.py:99, train_encodersKIT.py:214-216):
 * g' = grad_scale*g + wd*p; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 * p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).  weights_sqsum (nullable, device) receives sum p^2 of the
 * updated parameters (the trainer's "weights_sum", train_encodersKIT.py:229-231). */
int dali_adam_step(dali_ctx* ctx, void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                   float* weights_sqsum);
/* momentum = beta*momentum + (1-beta)*online  (train_encodersKIT.py:218-226), flat. */
int dali_ema_update(dali_ctx* ctx, void* stream, float* momentum, const float* online, int64_t n, float beta);

/* ---- optional in-batch triplet head: BatchWeightedSoftmaxTripletLoss (losses.py:607-654) ------------------- *
 * S [nb,nb] = fn @ fn^T (dali_pairdist, DOT); labels int32 codes; w [nb] = the 13-entry distortion table
 * (losses.py:613-627) gathered per row.  Forward: rowstat [nb,2] = {w_i*softplus((s_neg - s_pos)/tau), w_i},
 * sums[2] = {numerator, denominator} (loss = sums[0]/sums[1]), sel_idx [nb,2] = {hardest positive, hardest
 * negative}, sel_coef [nb] = d row/d s_neg (= -d row/d s_pos); status[0] = 1 when some row has no negative (the
 * reference's topk raises there; such rows are skipped).  Backward: dS_sym [nb,nb] = (dS + dS^T) * gscale/denom,
 * so that d loss / d fn = dS_sym @ fn. */
int dali_triplet_loss_fwd(dali_ctx* ctx, void* stream, const float* S, const int32_t* labels, const float* w, float tau, int nb,
                          float* rowstat, float* sums, int32_t* sel_idx, float* sel_coef, int32_t* status);
int dali_triplet_loss_bwd(dali_ctx* ctx, void* stream, const int32_t* sel_idx, const float* sel_coef, int nb, const float* denom,
                          float gscale, float* dS_sym);

/* ---- epoch targets: class centers + farthest-point proxies (train_encodersKIT.py:113-156, :252-284) -------- *
 * fvs [n,d] fp32 un-normalised embeddings.  order [n]: row indices sorted by identity; bounds [n_classes+1]:
 * identity c owns order[bounds[c] .. bounds[c+1]).  first_pick [n_classes]: position (0 .. n_c-1, within the
 * identity's slice) of the first proxy -- the reference draws it with np.random.choice(n) (:257), so the host
 * keeps that stream.  Outputs: centers [n_classes,d] = L2-normalised class means (:131-137); proxies
 * [n_classes*num_proxies,d] = the chosen rows, L2-normalised (:139-141), zero rows where an identity has fewer than
 * num_proxies images; proxy_rows [n_classes*num_proxies] = chosen row of fvs or -1; max_dist [n_classes] = largest
 * pairwise distance among an identity's chosen rows (:278).  All pointers are device pointers.  Ties in the
 * arg-max go to the highest row position (the reference's argsort(...)[-1] leaves them unspecified). */
int dali_class_targets(dali_ctx* ctx, void* stream, const float* fvs, int n, int d, const int32_t* order,
                       const int32_t* bounds, int n_classes, const int32_t* first_pick, int num_proxies,
                       float* centers, float* proxies, int32_t* proxy_rows, float* max_dist);

/* ---- input pipeline on decoded uint8 images (decode stays on the host) -------------------------- *
 * Resize((H,W), bicubic) of getFeatures.py:18 / train_encodersKIT.py:313 = Pillow's two-pass ImagingResample on 8-bit
 * data, reproduced bit for bit: src = n packed RGB images [in_h][in_w][3] at byte offsets src_off; table_of[n] selects
 * the coefficient table of the image's size; bounds_* [tables][out][2] = (first input index, tap count) and coefs_*
 * [tables][out][ksize] = 22-bit fixed-point taps, built by the host as Pillow's precompute_coeffs does
 * (daliid_amd/transforms.py).  out = [n][out_h][out_w][3] uint8.  All pointers are device pointers. */
int dali_resize_bicubic_u8(dali_ctx* ctx, void* stream, const uint8_t* src, const int64_t* src_off, const int32_t* in_h,
                           const int32_t* in_w, const int32_t* table_of, int n, int max_in_h, const int32_t* bounds_h,
                           const int32_t* coefs_h, int ksize_h, const int32_t* bounds_v, const int32_t* coefs_v, int ksize_v,
                           int out_h, int out_w, uint8_t* out);
/* RandomCrop(padding) -> RandomHorizontalFlip -> ColorJitter(brightness, contrast, saturation) -> ToTensor ->
 * RandomErasing(value 0) -> Normalize (train_encodersKIT.py:313-320) of n resized uint8 images [n][h][w][3] with the
 * per-image parameters drawn by the host in torchvision's order: params [n][16] int32 words = crop top, crop left,
 * flip, 4 x op order (0 brightness, 1 contrast, 2 saturation, 3 hue = no-op), erase i, j, h, w (h = 0: none), the
 * three factors as float bits, crop padding, augment flag (0 = eval path: ToTensor + Normalize only,
 * getFeatures.py:18-19).  The enhancers follow PIL.ImageEnhance on 8-bit data exactly.  mean3 / std3 are HOST pointers
 * to 3 floats; out = fp32 [n][3][h][w].  One workgroup per image, the image lives in LDS (h*w*3 <= 150 KiB). */
int dali_augment_batch(dali_ctx* ctx, void* stream, const uint8_t* images, const int32_t* params, int n, int h, int w,
                       const float* mean3, const float* std3, float* out);
/* The same transform, by the same kernel, on images picked from a device-resident store (transforms.ImageStore): store =
 * [store_rows][h][w][3] uint8, rows [n] int32 DEVICE array, image i of out = dali_augment_batch applied to store[rows[i]]
 * with params[i], bit for bit.  rows may come in any order and may repeat; byte offsets into the store are 64-bit (the
 * store may exceed 2 GiB).  rows is device data this entry cannot inspect: whatever it holds, the kernel does not read
 * outside the store -- a row outside [0, store_rows) is treated as an ALL-BLACK image (every byte 0) and the rest of the
 * pipeline (crop, flip, jitter, erase, normalise) runs on it.  Same limits as dali_augment_batch, and store_rows >= 1. */
int dali_augment_gather(dali_ctx* ctx, void* stream, const uint8_t* store, int64_t store_rows, const int32_t* rows,
                        const int32_t* params, int n, int h, int w, const float* mean3, const float* std3, float* out);

/* ---- measurement aid (bench.py roofline leg; no reference counterpart) ------------------------------- *
 * Between _begin and _end every MFMA GEMM kernel launch of the conv / linear path (class 0: igemm_conv_*
 * forward + dgrad, class 1: igemm_wgrad_*) is bracketed by two HIP events on the stream it is launched on.
 * _end waits for them and returns, per class, the summed kernel duration [ms], the summed 2*M*N*K FLOPs
 * and the launch count (arrays of 2).  Process-wide, not re-entrant; launches beyond max_launches are
 * not recorded. */
int dali_gemm_profile_begin(dali_ctx* ctx, int max_launches);
int dali_gemm_profile_end(dali_ctx* ctx, double* total_ms, double* total_flops, long long* launches);

/* ---- net plan: Encoders.ResNet50ReID forward / backward (Encoders.py:306-351) ------------------------ *
 * The plan owns topology + launch order; the caller owns storage: flat fp32 params / grads / BN running
 * statistics, and one byte arena (activations, bf16 weight images, scratch).  Tensor names and order follow
 * torchvision's state_dict ("conv1.weight", "bn1.weight", "layer1.0.conv1.weight", ..., "last_bn.bias"),
 * conv weights are stored [cout][r][s][cin] (the channels_last storage of a logical OIHW tensor). */
typedef struct dali_resnet dali_resnet;
typedef struct {
    int batch, height, width;   /* images: fp32 NCHW [batch,3,height,width]; height % 32 == 0, width % 16 == 0 */
    int layers[4];              /* bottlenecks per stage: {3,4,6,3} for ResNet-50 */
    int width_base;             /* 64 for ResNet-50 (32 allowed for test-size nets) */
} dali_resnet_cfg;

/* IBN-a (IBN-Net resnet50_ibn_a / resnet101_ibn_a under Encoders.ResNet50IBNReID / ResNet101IBNReID, Encoders.py:462-603): ibn[s] != 0 makes
 * every bottleneck of stage s (layer s+1) an IBN-a block, whose bn1 is InstanceNorm2d (affine) on the first width / 2 channels and BatchNorm2d
 * on the rest.  Its tensors are "layerL.B.bn1.IN.weight", ".IN.bias" [w/2], ".bn1.BN.weight", ".BN.bias" [w - w/2] and the buffers
 * ".bn1.BN.running_mean", ".running_var"; IBN-a proper is {1,1,1,0}.  All zero (or a null ext) = dali_resnet_create, size for size.
 * A plan with an IBN stage is an EVAL plan: conv1 writes its output through the output stage (identity on the IN half, the running
 * statistics' coefficients on the BN half), then one dali_ibn_act launch in place.  It reserves none of the backward's buffers, and
 * dali_resnet_forward with training != 0 and dali_resnet_backward return DALI_ERR_LIMIT before any launch ("... eval only"). */
typedef struct { int ibn[4]; } dali_resnet_ext;
int dali_resnet_create(dali_ctx* ctx, const dali_resnet_cfg* cfg, dali_resnet** out);
int dali_resnet_create_ex(dali_ctx* ctx, const dali_resnet_cfg* cfg, const dali_resnet_ext* ext, dali_resnet** out);
int dali_resnet_destroy(dali_resnet* net);
int dali_resnet_sizes(const dali_resnet* net, int64_t* param_elems, int64_t* buffer_elems, int64_t* arena_bytes,
                      int* feat_dim, int* n_params, int* n_buffers);
/* kind 0: parameter, 1: buffer (running_mean / running_var).  offset/numel in fp32 elements of the flat storage. */
int dali_resnet_tensor_info(const dali_resnet* net, int kind, int index, char* name, int name_cap, int64_t* offset,
                            int64_t* numel, int* shape4, int* ndim);
int dali_resnet_stage_param_range(const dali_resnet* net, int stage, int64_t* begin, int64_t* end);
/* All storages 256-byte aligned; grads may be null for inference-only use. */
int dali_resnet_bind(dali_resnet* net, float* params, float* grads, float* buffers, void* arena, size_t arena_bytes);
/* Rebuild the bf16 operand images from the fp32 master weights (call after every optimizer step / state load). */
int dali_resnet_refresh_weights(dali_resnet* net, void* stream);
/* Pooling of the embedding head for the next forward/backward calls (dali_feature; default BOTH).  Mirrors
 * `model.module.feature = pooling` of evaluateCleanATModels.getWeightsByMagnitude (:249-256). */
int dali_resnet_set_feature(dali_resnet* net, int mode);
/* images fp32 NCHW -> emb fp32 [batch, feat_dim].  training != 0: batch statistics + running-stat update
 * (model.train()); else running statistics (model.eval()).  Stands under `model_online(batch_imgs)`
 * (train_encodersKIT.py:197) and `model(batch_gpu)` (getFeatures.py:61). */
int dali_resnet_forward(dali_resnet* net, void* stream, const float* images, int training, float* emb);
/* Height and width of the layer4 map of this plan (the rows a dali_head_spec counts). */
int dali_resnet_head_map(dali_resnet* net, int* h, int* w);
/* Inference with several heads from ONE trunk pass (model.eval(): running statistics, nothing is updated): emb fp32
 * [n_heads][batch][feat_dim], head i = last_bn(pool_i(layer4 map)) (dali_head_pool_multi); a head over every row is bitwise what
 * dali_resnet_forward(training = 0) gives under dali_resnet_set_feature(mode_i).  heat (nullable) fp32 [batch][h * w]: the channel sum of
 * the map (dali_channel_sum).  The plan's own feature mode is neither read nor changed.  Stands under
 * `model(x, multipart=True)` / `model(x, attention_map=True)` (mainKIT.py:239-298) and the three poolings of
 * evaluateCleanATModels.getWeightsByMagnitude (:249-256). */
int dali_resnet_forward_heads(dali_resnet* net, void* stream, const float* images, const dali_head_spec* heads, int n_heads, float* emb,
                              float* heat);
/* Backward of the last training forward, stages stage_begin..stage_end (0: neck+head+layer4, 1: layer3,
 * 2: layer2, 3: layer1+stem); fills the flat gradient buffer (overwrites, no accumulation).
 * Stands under `batch_loss.backward()` (train_encodersKIT.py:215). */
int dali_resnet_backward(dali_resnet* net, void* stream, const float* d_emb, int stage_begin, int stage_end);

int dali_resnet_debug_tensor(dali_resnet* net, const char* name, void** ptr, int64_t* bytes);

/* ---- net plan: TransReID ViT + BN neck (make_models.build_transformer.forward, make_models.py:184-205) ----- *
 * Same storage contract as dali_resnet_*.  forward: images fp32 NCHW -> feat fp32 [batch, dim] (after the
 * BatchNorm1d neck); global_feat (nullable) receives the pre-neck cls feature.  Dropout is the identity (rate 0).
 * Limits: head_dim = dim / heads is 64 or 96, at most 1024 tokens (DALI_ERR_LIMIT beyond).  A plan with more than 256 tokens is an EVAL plan:
 * it reserves none of the backward's buffers, refresh_weights only casts, and dali_vit_forward_ex with training != 0, dali_vit_backward and
 * dali_vit_backward_stages return DALI_ERR_LIMIT before any launch ("training needs at most 256 tokens (this plan has N); eval mode only").
 * A plan with head_dim 96 (ViT-Small: dim 768, 8 heads) is an eval plan in the same way -- only the attention forward exists at that width --
 * and its refusal reads "training needs head_dim 64 (this plan has 96); eval mode only"; the token check comes first.  Plans with at most 256
 * tokens and head_dim 64 are what they were, size for size. */
typedef struct dali_vit dali_vit;
typedef struct {
    int batch, height, width;   /* images fp32 NCHW [batch,3,height,width] */
    int patch, stride;          /* 16, 16 for ViT-B/16; stride < patch = overlapping patches (PatchEmbed_overlap) */
    int dim, depth, heads;      /* 768, 12, 12 */
    int mlp_hidden;             /* 3072 */
    int num_classes;            /* size of the unused `base.fc` head kept for state_dict compatibility (1000) */
} dali_vit_cfg;
/* What a TransReID checkpoint normally carries on top of the baseline; all zero = dali_vit_create.
 *   SIE: "base.sie_embed" [n_sie,1,dim] after pos_embed; forward_ex takes the per-sample index (cam*view_num + view, cam, or view).
 *   local_feature (vit_pytorch.py:393-396): blocks[:-1], all tokens, no final norm; eval only.
 *   jpm (make_models.build_transformer_local, make_models.py:221-377; implies local_feature; eval only): parameters "b1.0.*", "b1.1.*",
 *   "b2.0.*", "b2.1.*", "classifier*.weight" [id_classes, dim] (unused), "bottleneck", "bottleneck_1..4"; feat is [batch, 5*dim].
 *   The shift + group shuffle of the patch tokens (shuffle_unit, make_models.py:8-25) does not depend on the data: the caller computes it once
 *   (daliid_amd.make_models.jpm_token_map) and hands it in as token_map; the plan copies it.
 *   no_qkv_bias / qk_scale: ViT-Small's Attention (vit_pytorch.py:461-468: no qkv bias, scale 768 ** -0.5); independent of head_dim, they
 *   train at head_dim 64. */
typedef struct {
    int n_sie;                  /* rows of sie_embed; 0 = no SIE */
    float sie_coef;             /* cfg.MODEL.SIE_COE */
    int local_feature, jpm;
    int divide;                 /* cfg.MODEL.DEVIDE_LENGTH (must be 4: the reference's forward cuts four runs) */
    const int32_t* token_map;   /* jpm: host int32 [divide][L], L = n_patches / divide: the token (1 .. n_patches; 0 is cls) at place j of run i */
    int neck_after;             /* cfg.TEST.NECK_FEAT == 'after' */
    int id_classes;             /* rows of the unused classifier weights (the training set's identities) */
    int no_qkv_bias;            /* qkv_bias=False (vit_pytorch.py:147): no "attn.qkv.bias" parameter in any block, b1.0 / b2.0 included */
    float qk_scale;             /* the attention scale (vit_pytorch.py:145), forward and backward; 0 = head_dim ** -0.5 */
} dali_vit_ext;
int dali_vit_create(dali_ctx* ctx, const dali_vit_cfg* cfg, dali_vit** out);
int dali_vit_create_ex(dali_ctx* ctx, const dali_vit_cfg* cfg, const dali_vit_ext* ext, dali_vit** out);
int dali_vit_destroy(dali_vit* net);
int dali_vit_sizes(const dali_vit* net, int64_t* param_elems, int64_t* buffer_elems, int64_t* arena_bytes, int* feat_dim,
                   int* n_params, int* n_buffers);
int dali_vit_tensor_info(const dali_vit* net, int kind, int index, char* name, int name_cap, int64_t* offset, int64_t* numel,
                         int* shape4, int* ndim);
int dali_vit_bind(dali_vit* net, float* params, float* grads, float* buffers, void* arena, size_t arena_bytes);
int dali_vit_refresh_weights(dali_vit* net, void* stream);
int dali_vit_forward(dali_vit* net, void* stream, const float* images, int training, float* feat, float* global_feat);
/* sie_idx: device int32 [batch] (required when n_sie > 0; must outlive the backward of a training forward); tokens_out (nullable, local_feature
 * nets): the tokens after blocks[:-1] as fp32 [batch][T][dim].  A local_feature net without jpm writes only tokens_out: it requires
 * tokens_out and refuses a non-null feat or global_feat (the reference has no cls feature or neck output for such a base). */
int dali_vit_forward_ex(dali_vit* net, void* stream, const float* images, const int32_t* sie_idx, int training, float* feat, float* global_feat,
                        float* tokens_out);
int dali_vit_backward(dali_vit* net, void* stream, const float* d_feat);
/* Backward in stages = gradient buckets of the data-parallel reducer (daliid_amd/parallel.py): stage 0 = neck + final norm + the
 * last group of blocks (consumes d_feat), ..., the last stage also holds cls / pos / patch embedding.  Replaces the autograd
 * graph nn.DataParallel reduces as a whole (Encoders.py:39-40). */
int dali_vit_num_stages(const dali_vit* net);
int dali_vit_stage_param_range(const dali_vit* net, int stage, int64_t* begin, int64_t* end);
int dali_vit_backward_stages(dali_vit* net, void* stream, const float* d_feat, int stage_begin, int stage_end);
/* DropPath (vit_pytorch.py:45-62; per block rate linspace(0, drop_path_rate, depth), :338): scales = device fp32 [2*depth][batch],
 * row 2i = attention branch of block i, row 2i+1 = its MLP branch, each entry floor(keep + u)/keep in {0, 1/keep}.  Applied by
 * training-mode forwards (and mirrored by the backward) until reset with NULL; the buffer must outlive the backward. */
int dali_vit_set_drop_path(dali_vit* net, const float* scales);

#ifdef __cplusplus
}
#endif
#endif /* DALIID_H */

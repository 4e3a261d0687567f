// topk.hip -- exact top-k retrieval (include/daliid.h: dali_topk_rows, dali_topk_decode, dali_pairdist_topk): the k best entries of every
//   row under the order of topk_key.h, as sorted lists of 64-bit keys that later calls merge into; the lists are sorted in LDS by
//   block_pad_sort (block_prims.h, shared with the ranking).  dali_pairdist_topk takes the rows from the distance kernel's accumulators
//   (pairdist_epilogue_topk, eval.hip) and never holds more than a [nq, boot_cols] block of them.
#include "kernels.h"
#include "topk_key.h"

namespace dali {

constexpr int TOPK_BUF = 2048;                  // keys a row's workgroup holds in LDS (16 KiB: 8+ workgroups per CU, the scan is HBM-bound)
constexpr int TOPK_BATCH = 1024;                // elements scanned between two looks at the fill level (4 per thread)
constexpr int TOPK_CAND_MAX = TOPK_BUF - TOPK_K_MAX;

// ------------------------------------------------------------------------------------------------
// Row selection: one 256-thread workgroup per row, one read of the row (4 bytes per element, 16-byte loads where the row is aligned).
// An element enters the LDS list only if its key is below the row's threshold; the threshold is the k-th key of the last compaction
// (sort, keep k), and a compaction runs only when the list could not take another batch.  Until the first one the threshold is the
// sentinel (everything enters: 2 batches); after it a fraction k / columns_seen of a row in random order enters, so a row of 100k
// entries is compacted a handful of times and nearly every element costs one compare.  The compaction points depend on counts only,
// and the counts on the thresholds only: the same input gives the same keys.
// gate (nullable): the launch does nothing when gate[0] == 0.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ x, long long ld, int ncols, int col_offset, int k, int largest,
                                                         int accumulate, unsigned long long* __restrict__ keys, const int* __restrict__ gate) {
    __shared__ unsigned long long s_key[TOPK_BUF];
    __shared__ int s_n;
    if (gate && gate[0] == 0) return;
    const int tid = threadIdx.x;
    unsigned long long* krow = keys + (size_t)blockIdx.x * k;
    const float* xr = x + (size_t)blockIdx.x * ld;
    unsigned long long thr = TOPK_SENTINEL;
    if (accumulate) {
        for (int t = tid; t < k; t += 256) s_key[t] = krow[t];
        thr = krow[k - 1];
    }
    if (tid == 0) s_n = accumulate ? k : 0;
    __syncthreads();
    const bool vec = (reinterpret_cast<uintptr_t>(xr) & 15) == 0;
    auto load = [&](int base, float (&v)[4]) {
        const int c = base + tid * 4;
        if (vec && c + 3 < ncols) {
            const float4 f = *reinterpret_cast<const float4*>(xr + c);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = (c + t < ncols) ? xr[c + t] : 0.f;
        }
    };
    float cur[4], nxt[4];
    load(0, cur);
    for (int base = 0; base < ncols; base += TOPK_BATCH) {
        if (base + TOPK_BATCH < ncols) load(base + TOPK_BATCH, nxt);          // the next batch is in flight across this one's barriers
        const int c = base + tid * 4;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (c + t < ncols) {
                const unsigned long long key = topk_key(cur[t], col_offset + c + t, largest);
                if (key < thr) s_key[atomicAdd(&s_n, 1)] = key;               // at most TOPK_BATCH entries on top of <= TOPK_BUF - TOPK_BATCH
            }
        }
        __syncthreads();
        const int n = s_n;
        __syncthreads();                                                     // every thread has read the fill level before the next batch raises it
        if (n > TOPK_BUF - TOPK_BATCH) {
            block_pad_sort(s_key, n, k, tid);
            thr = s_key[k - 1];                                              // n > 1024 >= k: the list is full from here on
            if (tid == 0) s_n = k;
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) cur[t] = nxt[t];
    }
    block_pad_sort(s_key, s_n, k, tid);
    for (int t = tid; t < k; t += 256) krow[t] = s_key[t];
}

// Folds a query's candidate list (the survivors of one selecting launch) into its running list and empties it.  After an overflow
// (flag[0] != 0) the lists of that launch are incomplete: they are dropped and the launch's columns come again through the matrix.
__global__ __launch_bounds__(256) void topk_merge_kernel(unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ cand,
                                                          int* __restrict__ cnt, int cap, int k, const int* __restrict__ flag) {
    __shared__ unsigned long long s_key[TOPK_BUF];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int n = cnt[q];
    __syncthreads();
    if (tid == 0) cnt[q] = 0;
    if (flag[0] != 0 || n == 0) return;
    unsigned long long* krow = keys + (size_t)q * k;
    for (int t = tid; t < k; t += 256) s_key[t] = krow[t];
    for (int t = tid; t < n; t += 256) s_key[k + t] = cand[(size_t)q * cap + t];
    __syncthreads();
    block_pad_sort(s_key, k + n, k, tid);
    for (int t = tid; t < k; t += 256) krow[t] = s_key[t];
}

// End of a round over `cols` gallery rows: stats = {columns selected in the epilogue, columns through the matrix, overflow events}
__global__ void topk_round_end_kernel(int* __restrict__ flag, int32_t* __restrict__ stats, int cols) {
    if (flag[0] != 0) { stats[1] += cols; stats[2] += 1; } else stats[0] += cols;
    flag[0] = 0;
}
__global__ void topk_stats_add_kernel(int32_t* __restrict__ stats, int which, int cols) { stats[which] += cols; }

__global__ __launch_bounds__(256) void topk_decode_kernel(const unsigned long long* __restrict__ keys, long long n, int largest,
                                                           float* __restrict__ values, int32_t* __restrict__ indices) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v; int idx;
    topk_key_decode(keys[i], largest, v, idx);
    values[i] = v;
    indices[i] = idx;
}

static int launch_topk_rows(hipStream_t st, const float* x, int nq, int ncols, long long ld, int col_offset, int k, int largest, int accumulate,
                            unsigned long long* keys, const int* gate) {
    hipLaunchKernelGGL(topk_rows_kernel, dim3(nq), dim3(256), 0, st, x, ld, ncols, col_offset, k, largest, accumulate, keys, gate);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

static int check_k(const char* who, int k) {
    if (k < 1) { set_error("%s: k=%d", who, k); return DALI_ERR_INVALID; }
    if (k > TOPK_K_MAX) { set_error("%s: k=%d above the documented cap %d", who, k, TOPK_K_MAX); return DALI_ERR_LIMIT; }
    return DALI_OK;
}

// tuning of dali_pairdist_topk with the defaults filled in: boot / chunk in whole gallery tiles of 128 rows
struct TopkPlan {
    int boot, chunk, cap;
    size_t b_block, b_cand, b_cnt;
    size_t bytes() const { return b_block + b_cand + b_cnt + 256; }
};
static TopkPlan topk_plan(int nq, int d, bool split, int k, int boot_cols, int chunk_cols, int cand_cap) {
    TopkPlan p;
    const int up = 1 << 24;
    p.boot = boot_cols > 0 ? boot_cols : 4096;
    p.chunk = chunk_cols > 0 ? chunk_cols : 4096;
    p.boot = ((p.boot < up ? p.boot : up) + 127) / 128 * 128;
    p.chunk = ((p.chunk < up ? p.chunk : up) + 127) / 128 * 128;
    // The thresholds of a round are fixed, the k-th keys of the s rows seen; of n new rows in random order n k / (s + 1) beat them on
    // average (negative binomial: variance (1 + n / s) times the mean).  A round takes at most as many rows as were seen, so the mean is at
    // most k and 4 k (at least 64) slots are many standard deviations away for every k.
    p.cap = cand_cap > 0 ? cand_cap : (4 * k > 64 ? 4 * k : 64);
    if (p.cap > TOPK_CAND_MAX) p.cap = TOPK_CAND_MAX;
    const int qmax = pairdist_dma_max_rows(d, split) / 256 * 256;
    const size_t rows = (size_t)(nq < qmax ? nq : qmax);
    p.b_block = align_up(rows * p.boot * sizeof(float), 256);
    p.b_cand = align_up(rows * p.cap * sizeof(unsigned long long), 256);
    p.b_cnt = align_up(rows * sizeof(int), 256);
    return p;
}

}  // namespace dali

using namespace dali;

extern "C" int dali_topk_rows(dali_ctx* ctx, void* stream, const float* x, int nq, int ncols, int64_t ld, int col_offset, int k, int largest,
                              int accumulate, int64_t* keys) {
    DALI_REQUIRE(ctx && x && keys, "dali_topk_rows: null argument");
    DALI_REQUIRE(nq >= 0 && ncols >= 0 && ld >= ncols, "dali_topk_rows: bad shape nq=%d ncols=%d ld=%lld", nq, ncols, (long long)ld);
    DALI_REQUIRE(col_offset >= 0 && (long long)col_offset + ncols <= 0x7fffffffll, "dali_topk_rows: column indices %d + %d leave int32", col_offset, ncols);
    DALI_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(keys) & 7) == 0, "dali_topk_rows: misaligned pointer");
    if (int rc = check_k("dali_topk_rows", k)) return rc;
    if (nq == 0) return DALI_OK;
    return launch_topk_rows((hipStream_t)stream, x, nq, ncols, ld, col_offset, k, largest ? 1 : 0, accumulate ? 1 : 0,
                            reinterpret_cast<unsigned long long*>(keys), nullptr);
}

extern "C" int dali_topk_decode(dali_ctx* ctx, void* stream, const int64_t* keys, int nq, int k, int largest, float* values, int32_t* indices) {
    DALI_REQUIRE(ctx && keys && values && indices, "dali_topk_decode: null argument");
    DALI_REQUIRE(nq >= 0 && k >= 1, "dali_topk_decode: bad shape nq=%d k=%d", nq, k);
    const long long n = (long long)nq * k;
    if (n == 0) return DALI_OK;
    hipLaunchKernelGGL(topk_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long*>(keys), n, largest ? 1 : 0, values, indices);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" size_t dali_pairdist_topk_scratch_bytes(int nq, int ng, int d, int k, int boot_cols, int chunk_cols, int cand_cap) {
    if (nq <= 0 || ng <= 0 || d <= 0 || k < 1 || k > TOPK_K_MAX) return 0;
    size_t a = topk_plan(nq, d, true, k, boot_cols, chunk_cols, cand_cap).bytes(), b = topk_plan(nq, d, false, k, boot_cols, chunk_cols, cand_cap).bytes();
    return a > b ? a : b;
}

extern "C" int dali_pairdist_topk(dali_ctx* ctx, void* stream, const void* q_image, const float* q_sq, const void* g_image, const float* g_sq,
                                  int nq, int ng, int d, int metric, int precision, int k, int largest, int g_offset, int accumulate,
                                  int64_t* keys, int boot_cols, int chunk_cols, int cand_cap, int32_t* stats) {
    DALI_REQUIRE(ctx && q_image && g_image && q_sq && g_sq && keys && stats, "dali_pairdist_topk: null argument");
    DALI_REQUIRE(nq >= 0 && ng >= 0 && d > 0, "dali_pairdist_topk: bad shape nq=%d ng=%d d=%d", nq, ng, d);
    DALI_REQUIRE(metric == DALI_METRIC_COSINE || metric == DALI_METRIC_L2SQ || metric == DALI_METRIC_DOT, "dali_pairdist_topk: bad metric %d", metric);
    DALI_REQUIRE(precision == DALI_PREC_BF16X3 || precision == DALI_PREC_BF16, "dali_pairdist_topk: bad precision %d", precision);
    DALI_REQUIRE(g_offset >= 0 && (long long)g_offset + ng <= 0x7fffffffll, "dali_pairdist_topk: gallery indices %d + %d leave int32", g_offset, ng);
    DALI_REQUIRE(boot_cols >= 0 && chunk_cols >= 0 && cand_cap >= 0, "dali_pairdist_topk: negative tuning value");
    DALI_REQUIRE((reinterpret_cast<uintptr_t>(keys) & 7) == 0, "dali_pairdist_topk: keys must be 8-byte aligned");
    if (int rc = check_k("dali_pairdist_topk", k)) return rc;
    if (cand_cap > TOPK_CAND_MAX) {
        set_error("dali_pairdist_topk: cand_cap=%d above the documented cap %d", cand_cap, TOPK_CAND_MAX);
        return DALI_ERR_LIMIT;
    }
    hipStream_t st = (hipStream_t)stream;
    DALI_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(int32_t), st));
    if (nq == 0) return DALI_OK;
    const bool split = precision == DALI_PREC_BF16X3;
    largest = largest ? 1 : 0;
    const TopkPlan plan = topk_plan(nq, d, split, k, boot_cols, chunk_cols, cand_cap);
    char* ws = static_cast<char*>(workspace(ctx, plan.bytes()));
    if (!ws) return DALI_ERR_NOMEM;
    float* block = reinterpret_cast<float*>(ws);
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(ws + plan.b_block);
    int* cnt = reinterpret_cast<int*>(ws + plan.b_block + plan.b_cand);
    int* flag = reinterpret_cast<int*>(ws + plan.b_block + plan.b_cand + plan.b_cnt);
    DALI_HIP(hipMemsetAsync(cnt, 0, plan.b_cnt + 256, st));
    const size_t pitch_bytes = dali_pairdist_operand_bytes(1, d, precision);
    const int max_rows = pairdist_dma_max_rows(d, split);
    const int q_step = max_rows / 256 * 256, g_step = max_rows / 128 * 128;
    DALI_REQUIRE(q_step > 0 && g_step > 0, "dali_pairdist_topk: d=%d leaves no room for a tile in the 32-bit offsets", d);
    const char* qi = static_cast<const char*>(q_image);
    const char* gi = static_cast<const char*>(g_image);
    unsigned long long* ukeys = reinterpret_cast<unsigned long long*>(keys);
    if (ng == 0) {
        if (!accumulate) DALI_HIP(hipMemsetAsync(keys, 0xff, (size_t)nq * k * 8, st));
        return DALI_OK;
    }
    // Operand images beyond the DMA kernel's offsets are walked in row ranges below it; a range is addressed exactly as a caller would
    // address it with g_offset.  Query ranges are independent problems.
    for (int q0 = 0; q0 < nq; q0 += q_step) {
        const int nqr = nq - q0 < q_step ? nq - q0 : q_step;
        const uint16_t* qimg = reinterpret_cast<const uint16_t*>(qi + (size_t)q0 * pitch_bytes);
        unsigned long long* kq = ukeys + (size_t)q0 * k;
        // the columns [p, p + n) of these queries through the matrix block, in pieces of plan.boot; gate as for launch_pairdist_matrix
        auto through_matrix = [&](int p, int n, int acc, const int* gate) -> int {
            for (int c = 0; c < n; c += plan.boot) {
                const int m = n - c < plan.boot ? n - c : plan.boot;
                const uint16_t* gimg = reinterpret_cast<const uint16_t*>(gi + (size_t)(p + c) * pitch_bytes);
                if (int rc = launch_pairdist_matrix(ctx->num_cus, st, gimg, g_sq + p + c, qimg, q_sq + q0, nqr, m, d, metric, split, block, gate)) return rc;
                if (int rc = launch_topk_rows(st, block, nqr, m, m, g_offset + p + c, k, largest, (acc || c > 0) ? 1 : 0, kq, gate)) return rc;
            }
            return DALI_OK;
        };
        int p = 0;
        if (!accumulate) {                       // bootstrap: the first columns give every query a threshold
            p = ng < plan.boot ? ng : plan.boot;
            if (int rc = through_matrix(0, p, 0, nullptr)) return rc;
            hipLaunchKernelGGL(topk_stats_add_kernel, dim3(1), dim3(1), 0, st, stats, 1, q0 == 0 ? p : 0);
            DALI_LAUNCH_CHECK();
        }
        long long chunk = plan.chunk;
        while (p < ng) {
            int n = (long long)(ng - p) < chunk ? ng - p : (int)chunk;
            const int seen = p > plan.boot ? p : plan.boot;            // (a continued list has seen at least a bootstrap's worth of rows)
            if (n > seen) n = seen;                                    // a round never outgrows what its thresholds were drawn from
            const int range_end = (p / g_step + 1) * g_step;          // a launch stays inside one row range of the gallery image
            if (p + n > range_end) n = range_end - p;
            const uint16_t* gimg = reinterpret_cast<const uint16_t*>(gi + (size_t)p * pitch_bytes);
            const PairTopk sel{kq, cand, cnt, flag, k, plan.cap, g_offset + p, largest};
            if (int rc = launch_pairdist_select(ctx->num_cus, st, gimg, g_sq + p, qimg, q_sq + q0, nqr, n, d, metric, split, sel)) return rc;
            hipLaunchKernelGGL(topk_merge_kernel, dim3(nqr), dim3(256), 0, st, kq, cand, cnt, plan.cap, k, flag);
            DALI_LAUNCH_CHECK();
            if (int rc = through_matrix(p, n, 1, flag)) return rc;
            hipLaunchKernelGGL(topk_round_end_kernel, dim3(1), dim3(1), 0, st, flag, stats, q0 == 0 ? n : 0);
            DALI_LAUNCH_CHECK();
            p += n;
            if (chunk < (1ll << 30)) chunk *= 2;
        }
    }
    return DALI_OK;
}

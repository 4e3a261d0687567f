// rerank.hip -- k-reciprocal re-ranking (Zhong et al., CVPR 2017; torchreid.utils.re_ranking) of a query-gallery distance matrix, the
// block validateModels.py:49-53 leaves commented out.  Definition and numerics: include/daliid.h (dali_rerank) and DESIGN.md §5.
//
// Notation: N = nq + ng; full = [[q_q, q_g], [q_g^T, g_g]] (never materialised: rr_full reads the right block); A = full^2;
// colmax[i] = max_j A[j][i]; C[i][j] = A[j][i] / colmax[i] (row i of C is column i of A); K = k1 + 1.
//
//   1. rr_columns_kernel<false>  colmax: one streaming pass over the blocks, 32 columns of A per workgroup, tiled transposed reads
//   2. rr_columns_kernel<true>   R[i][0..K): the first K entries of the stable argsort of row i of C (a second pass, now dividing)
//   3. rr_recip_kernel           per row: bit masks of the positions l of R[i] with i in R[R[i][l]][:K] (KR) and [:h+1] (KRh)
//   4. rr_vrow_kernel            per row: expansion set E(i) (sorted, deduplicated) and V[i] = exp(-C[i,E]) / sum, padded sparse row
//   5. rr_qe_kernel              (k2 != 1) per row: mean of the k2 V rows of R[i][:k2], a k2-way merge of sorted sparse rows
//   6. rr_inv_*                  inverted index of the gallery rows of V: column -> (gallery row, value), count / scan / scatter
//   7. rr_jaccard_kernel<LDS>    per query: t[j] = sum_c min(V[i,c], V[j,c]) over c ascending, then the blend into out[i][:]
//
// Every float sum has a fixed order, so the result is bitwise identical run to run: the only atomics are integer counters of the
// inverted index, whose slot order inside a column cannot reach a sum (a column's rows are distinct, so each accumulator t[j] receives
// at most one term per column, and the columns are walked in ascending order with a barrier between them).
#include "block_prims.h"
#include <climits>

namespace {

constexpr int RR_TI = 32;          // columns of A (= rows of C) per workgroup of rr_columns_kernel
constexpr int RR_TJ = 64;          // rows of A per tile: one per lane
constexpr int RR_COL_THREADS = 512;
constexpr int RR_KMAX = 64;        // K = k1 + 1 <= 64: one neighbour per lane
constexpr int RR_LDS_ACC_MAX = 128 * 1024 / 4;   // galleries up to 32,768 keep the Jaccard accumulator in LDS (one 128 KiB block per CU)

typedef unsigned long long u64;
using dali::shfl_u64;
using dali::shfl_up_u64;

// full[j][i], every offset 64-bit (ng * ng exceeds 2^31 once ng > 46,340)
__device__ __forceinline__ float rr_full(const float* __restrict__ q_g, const float* __restrict__ q_q, const float* __restrict__ g_g,
                                         int nq, int ng, int j, int i) {
    if (j < nq) return i < nq ? q_q[(size_t)j * nq + i] : q_g[(size_t)j * ng + (i - nq)];
    return i < nq ? q_g[(size_t)i * ng + (j - nq)] : g_g[(size_t)(j - nq) * ng + (i - nq)];
}

__device__ __forceinline__ int rr_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double rr_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 rr_lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// ---- 1 + 2: one streaming pass over the blocks per template instance ----
// A workgroup owns RR_TI consecutive columns of A and walks all N rows in tiles of RR_TJ x RR_TI, staged in LDS.  Each tile row is
// read coalesced from its source: rows of q_q / q_g / g_g for most of the matrix, and for the query columns' gallery rows (q_g read
// down a row = a column of A) the tile is loaded transposed, consecutive lanes reading consecutive j of one q_g row.  Wave w then owns
// columns 4w..4w+3 of the tile and reads them down the tile, one row (j) per lane.
// SELECT = false: colmax.  SELECT = true: per column a sorted list of the K smallest keys (C value bits << 32 | j), one key per lane;
// C >= 0 (or NaN, which sorts last like numpy's), so the float bits order like the values and ties go by ascending index.
template <bool SELECT>
__global__ __launch_bounds__(RR_COL_THREADS) void rr_columns_kernel(const float* __restrict__ q_g, const float* __restrict__ q_q,
                                                                    const float* __restrict__ g_g, int nq, int ng,
                                                                    float* __restrict__ colmax, int K, int32_t* __restrict__ R) {
    __shared__ float tile[RR_TJ][RR_TI + 1];
    const int N = nq + ng, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i0 = blockIdx.x * RR_TI;
    float cm[4], mx[4];
    u64 key[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = i0 + w * 4 + t;
        cm[t] = (SELECT && i < N) ? colmax[i] : 1.f;
        mx[t] = 0.f;
        key[t] = ~0ull;
    }
    for (int j0 = 0; j0 < N; j0 += RR_TJ) {
        const bool transposed = j0 >= nq && i0 < nq;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RR_TJ * RR_TI / RR_COL_THREADS; ++k) {
            const int e = tid + k * RR_COL_THREADS;
            const int jj = transposed ? (e & (RR_TJ - 1)) : e / RR_TI, ii = transposed ? e / RR_TJ : (e & (RR_TI - 1));
            const int j = j0 + jj, i = i0 + ii;
            tile[jj][ii] = (j < N && i < N) ? rr_full(q_g, q_q, g_g, nq, ng, j, i) : 0.f;
        }
        __syncthreads();
        const int j = j0 + lane;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float x = tile[lane][w * 4 + t];
            const float a = x * x;
            if (!SELECT) {
                mx[t] = fmaxf(mx[t], a);
            } else if (i0 + w * 4 + t < N) {                                     // wave-uniform
                const float v = a / cm[t];                                       // IEEE division (no fast reciprocal)
                const u64 kv = ((u64)__float_as_uint(v) << 32) | (unsigned)j;
                const u64 th = shfl_u64(key[t], K - 1);
                u64 m = __ballot(j < N && kv < th);
                while (m) {                                                       // insert into the sorted per-lane list
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const u64 kc = shfl_u64(kv, b);
                    const u64 prev = shfl_up_u64(key[t], 1);
                    key[t] = key[t] < kc ? key[t] : ((lane == 0 || prev < kc) ? kc : prev);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = i0 + w * 4 + t;
        if (i >= N) continue;
        if (!SELECT) {
            float v = mx[t];
            for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
            if (lane == 0) colmax[i] = v;
        } else if (lane < K) {
            R[(size_t)i * K + lane] = (int32_t)(unsigned)key[t];
        }
    }
}

// ---- 3: reciprocity masks, one wave per row ----
__global__ __launch_bounds__(256) void rr_recip_kernel(const int32_t* __restrict__ R, int N, int K, int h, u64* __restrict__ krmask,
                                                       u64* __restrict__ khmask) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    int p = K;                                            // position of i in R[f][:K], K = absent
    if (lane < K) {
        const int32_t* rf = R + (size_t)R[(size_t)i * K + lane] * K;
        for (int m = 0; m < K; ++m)
            if (rf[m] == i) { p = m; break; }
    }
    const u64 kr = __ballot(lane < K && p < K), kh = __ballot(lane <= h && p <= h);
    if (lane == 0) { krmask[i] = kr; khmask[i] = kh; }
}

// ---- 4: expansion set and the V row, one wave per row ----
// s_cand (dynamic LDS, P2MAX ints): KR(i), then every accepted KRh(c) appended; bitonic-sorted, then deduplicated on the way out.
__global__ __launch_bounds__(64) void rr_vrow_kernel(const float* __restrict__ q_g, const float* __restrict__ q_q, const float* __restrict__ g_g,
                                                     int nq, int ng, const float* __restrict__ colmax, const int32_t* __restrict__ R, int K,
                                                     const u64* __restrict__ krmask, const u64* __restrict__ khmask, int cap,
                                                     int32_t* __restrict__ vidx, float* __restrict__ vval, int32_t* __restrict__ vcnt) {
    __shared__ int s_kr[RR_KMAX];
    extern __shared__ int s_cand[];
    const int i = blockIdx.x, lane = threadIdx.x;
    const u64 below = rr_lanes_below(lane);
    const u64 krm = krmask[i];
    const int nkr = __popcll(krm);
    if ((krm >> lane) & 1) {
        const int pos = __popcll(krm & below), v = R[(size_t)i * K + lane];
        s_kr[pos] = v;
        s_cand[pos] = v;
    }
    __syncthreads();
    int ncand = nkr;
    for (int t = 0; t < nkr; ++t) {
        const int c = s_kr[t];
        const u64 khm = khmask[c];
        const bool bit = (khm >> lane) & 1;
        const int x = bit ? R[(size_t)c * K + lane] : -1;
        bool in = false;
        if (bit)
            for (int u = 0; u < nkr; ++u) in |= s_kr[u] == x;
        const int n = __popcll(khm), inter = __popcll(__ballot(in));
        if ((double)inter > (2.0 / 3.0) * (double)n) {          // in double, as written in the definition
            if (bit) s_cand[ncand + __popcll(khm & below)] = x;
            ncand += n;
        }
    }
    int p2 = 1;
    while (p2 < ncand) p2 <<= 1;
    for (int k = ncand + lane; k < p2; k += 64) s_cand[k] = INT_MAX;
    __syncthreads();
    // (a network of its own, not an instance of block_sort_keys: one wave, ints, one compare pair per lane and pass, where the shared form
    //  walks every element with 256 threads and idles the upper partner -- another schedule for this kernel, not measured, so not taken)
    for (int size = 2; size <= p2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (p2 >> 1); t += 64) {
                const int lo = 2 * stride * (t / stride) + (t % stride), hi = lo + stride;
                const int a = s_cand[lo], b = s_cand[hi];
                if ((a > b) == ((lo & size) == 0)) { s_cand[lo] = b; s_cand[hi] = a; }
            }
            __syncthreads();
        }
    // two passes over the sorted candidates: the weight sum (fp64, fixed order), then w / sum (w recomputed bit for bit)
    const float cmi = colmax[i];
    double part = 0.0;
    int n_e = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const float sum = (float)rr_wave_sum_d(part);
        n_e = 0;
        for (int k0 = 0; k0 < ncand; k0 += 64) {
            const int k = k0 + lane;
            const int e = k < ncand ? s_cand[k] : INT_MAX;
            const bool first = k < ncand && (k == 0 || s_cand[k - 1] != e);
            const u64 m = __ballot(first);
            if (first) {
                const float x = rr_full(q_g, q_q, g_g, nq, ng, e, i);
                const float wgt = expf(-((x * x) / cmi));
                const size_t o = (size_t)i * cap + n_e + __popcll(m & below);
                if (pass == 0) { part += (double)wgt; vidx[o] = e; }
                else vval[o] = wgt / sum;
            }
            n_e += __popcll(m);
        }
    }
    if (lane == 0) vcnt[i] = n_e;
}

// ---- 5: query expansion, one wave per row: lane r < k2 walks the sorted row R[i][r]; each output column is the smallest current
// index, its value the fp32 sum of the matching lanes in ascending r (numpy's order along axis 0) divided by k2 ----
__global__ __launch_bounds__(64) void rr_qe_kernel(const int32_t* __restrict__ R, int K, int k2, const int32_t* __restrict__ vidx,
                                                   const float* __restrict__ vval, const int32_t* __restrict__ vcnt, int cap,
                                                   int32_t* __restrict__ qidx, float* __restrict__ qval, int32_t* __restrict__ qcnt, int qcap) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int src = lane < k2 ? R[(size_t)i * K + lane] : 0;
    const int len = lane < k2 ? vcnt[src] : 0;
    const int32_t* ip = vidx + (size_t)src * cap;
    const float* vp = vval + (size_t)src * cap;
    int ptr = 0, cur = len > 0 ? ip[0] : INT_MAX;
    float cv = len > 0 ? vp[0] : 0.f;
    const float fk2 = (float)k2;
    int n = 0, oi = 0;
    float ov = 0.f;
    int32_t* qi = qidx + (size_t)i * qcap;
    float* qv = qval + (size_t)i * qcap;
    for (;;) {
        const int m = rr_wave_min(cur);
        if (m == INT_MAX) break;
        u64 mask = __ballot(cur == m);
        float s = 0.f;
        while (mask) {
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            s += __shfl(cv, b, 64);
        }
        if (lane == (n & 63)) { oi = m; ov = s / fk2; }
        if ((n & 63) == 63) { qi[n - 63 + lane] = oi; qv[n - 63 + lane] = ov; }     // flush 64 outputs, coalesced
        ++n;
        if (cur == m) {
            ++ptr;
            cur = ptr < len ? ip[ptr] : INT_MAX;
            cv = ptr < len ? vp[ptr] : 0.f;
        }
    }
    if (lane < (n & 63)) { qi[(n & ~63) + lane] = oi; qv[(n & ~63) + lane] = ov; }
    if (lane == 0) qcnt[i] = n;
}

// ---- 6: inverted index of the gallery rows (count, scan, scatter), one wave per gallery row ----
__global__ __launch_bounds__(256) void rr_inv_count_kernel(const int32_t* __restrict__ vidx, const int32_t* __restrict__ vcnt, int cap, int nq,
                                                           int ng, int32_t* __restrict__ colcnt) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= ng) return;
    const int j = nq + g, n = vcnt[j];
    for (int k = lane; k < n; k += 64) atomicAdd(&colcnt[vidx[(size_t)j * cap + k]], 1);
}
// one block: off[c] = exclusive prefix of colcnt over N columns (off[N] = total), cursors zeroed
__global__ __launch_bounds__(1024) void rr_inv_scan_kernel(const int32_t* __restrict__ colcnt, int N, int32_t* __restrict__ off,
                                                           int32_t* __restrict__ cursor) {
    dali::block_counts_to_offsets_1024(colcnt, N, off, cursor);
}
__global__ __launch_bounds__(256) void rr_inv_scatter_kernel(const int32_t* __restrict__ vidx, const float* __restrict__ vval,
                                                             const int32_t* __restrict__ vcnt, int cap, int nq, int ng,
                                                             const int32_t* __restrict__ off, int32_t* __restrict__ cursor,
                                                             int32_t* __restrict__ inv_row, float* __restrict__ inv_val) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= ng) return;
    const int j = nq + g, n = vcnt[j];
    for (int k = lane; k < n; k += 64) {
        const size_t o = (size_t)j * cap + k;
        const int c = vidx[o];
        const int pos = off[c] + atomicAdd(&cursor[c], 1);     // slot order inside a column never reaches a sum (file comment)
        inv_row[pos] = g;
        inv_val[pos] = vval[o];
    }
}

// ---- 7: Jaccard + blend, one workgroup per query.  The accumulator t[0..ng) lives in LDS (LDS = true) or in the query's own output
// row (LDS = false, any gallery size); either way one column at a time, a barrier between columns ----
template <bool LDS>
__global__ __launch_bounds__(256) void rr_jaccard_kernel(const float* __restrict__ q_g, int nq, int ng, const float* __restrict__ colmax,
                                                         const int32_t* __restrict__ vidx, const float* __restrict__ vval,
                                                         const int32_t* __restrict__ vcnt, int cap, const int32_t* __restrict__ off,
                                                         const int32_t* __restrict__ inv_row, const float* __restrict__ inv_val, float w_jac,
                                                         float w_orig, float* __restrict__ out) {
    extern __shared__ float s_acc[];
    const int i = blockIdx.x, tid = threadIdx.x;
    float* orow = out + (size_t)i * ng;
    float* acc = LDS ? s_acc : orow;
    for (int j = tid; j < ng; j += 256) acc[j] = 0.f;
    __syncthreads();
    const int n = vcnt[i];
    for (int k = 0; k < n; ++k) {
        const size_t o = (size_t)i * cap + k;
        const int c = vidx[o];
        const float v = vval[o];
        const int e = off[c + 1];
        for (int p = off[c] + tid; p < e; p += 256) {
            const int g = inv_row[p];
            acc[g] = acc[g] + fminf(v, inv_val[p]);
        }
        __syncthreads();
    }
    const float cmi = colmax[i];
    const float* qrow = q_g + (size_t)i * ng;
    for (int j = tid; j < ng; j += 256) {
        const float t = acc[j];
        const float jac = 1.f - t / (2.f - t);
        const float x = qrow[j];
        orow[j] = jac * w_jac + ((x * x) / cmi) * w_orig;
    }
}

}  // namespace

using dali::align_up;

extern "C" int dali_rerank(dali_ctx* ctx, void* stream, const float* q_g, const float* q_q, const float* g_g, int nq, int ng, int k1, int k2,
                           double lambda_value, float* out) {
    DALI_REQUIRE(ctx && q_g && q_q && g_g && out, "dali_rerank: null argument");
    DALI_REQUIRE(nq > 0 && ng > 0 && (long long)nq + ng <= INT_MAX, "dali_rerank: bad shape nq=%d ng=%d", nq, ng);
    const int N = nq + ng;
    DALI_REQUIRE(k1 >= 1 && k1 + 1 <= N, "dali_rerank: k1=%d needs 1 <= k1 and k1 + 1 <= nq + ng = %d", k1, N);
    DALI_REQUIRE(k2 >= 1 && k2 <= k1 + 1, "dali_rerank: k2=%d outside 1..k1+1=%d", k2, k1 + 1);
    DALI_REQUIRE(lambda_value >= 0.0 && lambda_value <= 1.0, "dali_rerank: lambda_value %g outside [0, 1]", lambda_value);
    if (k1 + 1 > RR_KMAX) {
        dali::set_error("dali_rerank: k1=%d above the documented cap %d", k1, RR_KMAX - 1);
        return DALI_ERR_LIMIT;
    }
    const int K = k1 + 1;
    const int h = (k1 / 2) + ((k1 & 1) && ((k1 / 2) & 1) ? 1 : 0);        // round half to even of k1 / 2 (np.around)
    const int cand_cap = K * (h + 2);                                        // |KR(i)| + sum of the accepted |KRh(c)|
    const int cap1 = cand_cap < N ? cand_cap : N;
    const long long qe_cap = (long long)k2 * cap1;
    const int cap = k2 == 1 ? cap1 : (int)(qe_cap < N ? qe_cap : N);         // row capacity of the final V
    if ((long long)ng * cap > INT_MAX) {
        dali::set_error("dali_rerank: ng * row capacity = %lld exceeds 2^31 (inverted index offsets are int32)", (long long)ng * cap);
        return DALI_ERR_LIMIT;
    }
    int p2max = 1;
    while (p2max < cand_cap) p2max <<= 1;

    const size_t b_cm = align_up((size_t)N * 4, 256), b_R = align_up((size_t)N * K * 4, 256), b_mask = align_up((size_t)N * 8, 256);
    const size_t b_v1 = align_up((size_t)N * cap1 * 4, 256), b_cnt = align_up((size_t)N * 4, 256);
    const size_t b_v2 = k2 == 1 ? 0 : align_up((size_t)N * cap * 4, 256);
    const size_t b_col = align_up(((size_t)N + 1) * 4, 256), b_inv = align_up((size_t)ng * cap * 4, 256);
    const size_t total = b_cm + b_R + 2 * b_mask + 2 * b_v1 + b_cnt + (k2 == 1 ? 0 : 2 * b_v2 + b_cnt) + 3 * b_col + 2 * b_inv;
    char* ws = static_cast<char*>(dali::workspace(ctx, total));
    if (!ws) return DALI_ERR_NOMEM;
    size_t o = 0;
    auto take = [&](size_t b) { char* p = ws + o; o += b; return p; };
    float* colmax = reinterpret_cast<float*>(take(b_cm));
    int32_t* R = reinterpret_cast<int32_t*>(take(b_R));
    u64* krmask = reinterpret_cast<u64*>(take(b_mask));
    u64* khmask = reinterpret_cast<u64*>(take(b_mask));
    int32_t* v1idx = reinterpret_cast<int32_t*>(take(b_v1));
    float* v1val = reinterpret_cast<float*>(take(b_v1));
    int32_t* v1cnt = reinterpret_cast<int32_t*>(take(b_cnt));
    int32_t *vidx = v1idx, *vcnt = v1cnt;
    float* vval = v1val;
    if (k2 != 1) {
        vidx = reinterpret_cast<int32_t*>(take(b_v2));
        vval = reinterpret_cast<float*>(take(b_v2));
        vcnt = reinterpret_cast<int32_t*>(take(b_cnt));
    }
    int32_t* colcnt = reinterpret_cast<int32_t*>(take(b_col));
    int32_t* off = reinterpret_cast<int32_t*>(take(b_col));
    int32_t* cursor = reinterpret_cast<int32_t*>(take(b_col));
    int32_t* inv_row = reinterpret_cast<int32_t*>(take(b_inv));
    float* inv_val = reinterpret_cast<float*>(take(b_inv));

    hipStream_t st = (hipStream_t)stream;
    const int col_blocks = (N + RR_TI - 1) / RR_TI, row_blocks = (N + 3) / 4, gal_blocks = (ng + 3) / 4;
    hipLaunchKernelGGL((rr_columns_kernel<false>), dim3(col_blocks), dim3(RR_COL_THREADS), 0, st, q_g, q_q, g_g, nq, ng, colmax, K, R);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL((rr_columns_kernel<true>), dim3(col_blocks), dim3(RR_COL_THREADS), 0, st, q_g, q_q, g_g, nq, ng, colmax, K, R);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL(rr_recip_kernel, dim3(row_blocks), dim3(256), 0, st, R, N, K, h, krmask, khmask);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL(rr_vrow_kernel, dim3(N), dim3(64), (size_t)p2max * 4, st, q_g, q_q, g_g, nq, ng, colmax, R, K, krmask, khmask, cap1,
                       v1idx, v1val, v1cnt);
    DALI_LAUNCH_CHECK();
    if (k2 != 1) {
        hipLaunchKernelGGL(rr_qe_kernel, dim3(N), dim3(64), 0, st, R, K, k2, v1idx, v1val, v1cnt, cap1, vidx, vval, vcnt, cap);
        DALI_LAUNCH_CHECK();
    }
    DALI_HIP(hipMemsetAsync(colcnt, 0, ((size_t)N + 1) * 4, st));
    hipLaunchKernelGGL(rr_inv_count_kernel, dim3(gal_blocks), dim3(256), 0, st, vidx, vcnt, cap, nq, ng, colcnt);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL(rr_inv_scan_kernel, dim3(1), dim3(1024), 0, st, colcnt, N, off, cursor);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL(rr_inv_scatter_kernel, dim3(gal_blocks), dim3(256), 0, st, vidx, vval, vcnt, cap, nq, ng, off, cursor, inv_row, inv_val);
    DALI_LAUNCH_CHECK();
    const float w_jac = (float)(1.0 - lambda_value), w_orig = (float)lambda_value;
    if (ng <= RR_LDS_ACC_MAX) {
        DALI_ONCE_PER_DEVICE(DALI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&rr_jaccard_kernel<true>),
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, RR_LDS_ACC_MAX * 4)));
        hipLaunchKernelGGL((rr_jaccard_kernel<true>), dim3(nq), dim3(256), (size_t)ng * 4, st, q_g, nq, ng, colmax, vidx, vval, vcnt, cap, off,
                           inv_row, inv_val, w_jac, w_orig, out);
    } else {
        hipLaunchKernelGGL((rr_jaccard_kernel<false>), dim3(nq), dim3(256), 0, st, q_g, nq, ng, colmax, vidx, vval, vcnt, cap, off,
                           inv_row, inv_val, w_jac, w_orig, out);
    }
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

// qe.hip -- query expansion / database augmentation (include/daliid.h: dali_qe_combine): every output row is the weighted mean of k
//   gathered pool rows, the weights being an integer power of the neighbours' similarities.  The neighbour lists come from
//   dali_pairdist_topk (topk.hip), so no similarity matrix exists at any size.  The kernel is a pure gather: n k d 4 bytes of scattered
//   row reads (whole rows, 16 bytes per lane where the rows are aligned), n d 4 bytes written, no atomics on the output, no scratch.
//   The arithmetic order is the header's and is spelled with __fmul_rn / __fadd_rn / __fsub_rn: no contraction, whatever the flags.
#include "common.h"

namespace dali {

constexpr int QE_K_MAX = 128;                   // = TOPK_K_MAX: a row's whole neighbour list, as dali_pairdist_topk returns it
constexpr int QE_ALPHA_MAX = 16;
constexpr int QE_ROWS = 4;                      // output rows per 256-thread workgroup: one wave each
constexpr int QE_UNROLL = 8;                    // gathered rows in flight per lane

// 16-byte elements are the native vector type (f32x4_t, common.h): loads, selects and copies of it stay in registers
__device__ __forceinline__ f32x4_t qe_zero(const f32x4_t*) { return f32x4_t{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ float qe_zero(const float*) { return 0.f; }
// acc + (w * x): the product rounded, then the sum rounded
__device__ __forceinline__ float qe_madd(float acc, float w, float x) { return __fadd_rn(acc, __fmul_rn(w, x)); }
__device__ __forceinline__ f32x4_t qe_madd(f32x4_t acc, float w, f32x4_t x) {
    return f32x4_t{qe_madd(acc[0], w, x[0]), qe_madd(acc[1], w, x[1]), qe_madd(acc[2], w, x[2]), qe_madd(acc[3], w, x[3])};
}
__device__ __forceinline__ float qe_scale(float a, float r) { return __fmul_rn(a, r); }
__device__ __forceinline__ f32x4_t qe_scale(f32x4_t a, float r) {
    return f32x4_t{__fmul_rn(a[0], r), __fmul_rn(a[1], r), __fmul_rn(a[2], r), __fmul_rn(a[3], r)};
}

// U neighbours j .. j + U - 1 of one output element (or 4 of them, for the 16-byte V): all U loads are issued before the first use.  A skipped neighbour (index -1)
// loads row 0 (n_pool >= 1: always inside the pool) and is left out of the sum by a select, so that no load sits behind a branch.
template <int U, class V>
__device__ __forceinline__ void qe_step(const V* __restrict__ pool, size_t row_elems, int c, const int* s_idx, const float* s_w, int j, V& acc) {
    int g[U];
    float w[U];
    V x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { g[u] = s_idx[j + u]; w[u] = s_w[j + u]; }
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = pool[(size_t)(g[u] < 0 ? 0 : g[u]) * row_elems + c];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const V a = qe_madd(acc, w[u], x[u]);
        acc = g[u] < 0 ? acc : a;
    }
}

// One output row by one wave: lanes stride over the row's elements (V = f32x4_t or float), the j loop runs in ascending order per element.
template <class V>
__device__ __forceinline__ void qe_row(const V* __restrict__ pool, int row_elems, const int* s_idx, const float* s_w, int k, float rk,
                                        V* __restrict__ orow, int lane) {
    for (int c = lane; c < row_elems; c += 64) {
        V acc = qe_zero(pool);
        int j = 0;
        for (; j + QE_UNROLL <= k; j += QE_UNROLL) qe_step<QE_UNROLL>(pool, (size_t)row_elems, c, s_idx, s_w, j, acc);
        if (j + 4 <= k) { qe_step<4>(pool, (size_t)row_elems, c, s_idx, s_w, j, acc); j += 4; }
        if (j + 2 <= k) { qe_step<2>(pool, (size_t)row_elems, c, s_idx, s_w, j, acc); j += 2; }
        if (j < k) qe_step<1>(pool, (size_t)row_elems, c, s_idx, s_w, j, acc);
        orow[c] = qe_scale(acc, rk);
    }
}

__global__ __launch_bounds__(256) void qe_combine_kernel(const float* __restrict__ pool, int n_pool, int d, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ val, int n, int k, int val_is_distance, int alpha, float rk,
                                                          int vec, float* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ int s_idx[QE_ROWS][QE_K_MAX];
    __shared__ float s_w[QE_ROWS][QE_K_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * QE_ROWS + wave;
    // the row's k (index, weight) pairs, read once; an index outside the pool becomes -1 here and is never turned into an address
    if (row < n) {
        for (int j = lane; j < k; j += 64) {
            int g = idx[(size_t)row * k + j];
            const float v = val[(size_t)row * k + j];
            const float s = val_is_distance ? __fsub_rn(1.0f, v) : v;
            float w = 1.0f;
            if (alpha > 0) {
                w = s;
                for (int a = 1; a < alpha; ++a) w = __fmul_rn(w, s);
            }
            if (g < 0 || g >= n_pool) { g = -1; atomicMax(status, 1); }
            s_idx[wave][j] = g;
            s_w[wave][j] = w;
        }
    }
    __syncthreads();
    if (row >= n) return;
    if (vec) qe_row(reinterpret_cast<const f32x4_t*>(pool), d >> 2, s_idx[wave], s_w[wave], k, rk, reinterpret_cast<f32x4_t*>(out + (size_t)row * d), lane);
    else qe_row(pool, d, s_idx[wave], s_w[wave], k, rk, out + (size_t)row * d, lane);
}

}  // namespace dali

using namespace dali;

extern "C" int dali_qe_combine(dali_ctx* ctx, void* stream, const float* pool, int n_pool, int d, const int32_t* idx, const float* val, int n,
                               int k, int val_is_distance, int alpha, float* out, int32_t* status) {
    DALI_REQUIRE(k >= 1 && k <= QE_K_MAX, "dali_qe_combine: k=%d outside 1..%d", k, QE_K_MAX);
    DALI_REQUIRE(alpha >= 0 && alpha <= QE_ALPHA_MAX, "dali_qe_combine: alpha=%d outside 0..%d (integer exponents only)", alpha, QE_ALPHA_MAX);
    DALI_REQUIRE(d >= 1, "dali_qe_combine: d=%d", d);
    DALI_REQUIRE(n >= 0 && n_pool >= 0, "dali_qe_combine: bad shape n=%d n_pool=%d", n, n_pool);
    DALI_REQUIRE(ctx && pool && idx && val && out && status, "dali_qe_combine: null argument");
    if (n == 0) return DALI_OK;
    DALI_REQUIRE(n_pool >= 1, "dali_qe_combine: n_pool=%d: nothing to gather %d rows from", n_pool, n);
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(pool), p1 = p0 + (size_t)n_pool * d * sizeof(float);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (size_t)n * d * sizeof(float);
    DALI_REQUIRE(o1 <= p0 || p1 <= o0, "dali_qe_combine: out overlaps pool (rows are gathered while others are written)");
    DALI_REQUIRE(((p0 | o0 | reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(val)) & 3) == 0, "dali_qe_combine: misaligned pointer");
    const int vec = (d & 3) == 0 && ((p0 | o0) & 15) == 0;
    const float rk = 1.0f / (float)k;            // rounded once, on the host (IEEE division)
    hipLaunchKernelGGL(qe_combine_kernel, dim3((unsigned)((n + QE_ROWS - 1) / QE_ROWS)), dim3(256), 0, (hipStream_t)stream, pool, n_pool, d, idx, val,
                       n, k, val_is_distance ? 1 : 0, alpha, rk, vec, out, status);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

// templates.hip -- template (set) evaluation (include/daliid.h: dali_pool_rows, dali_segment_reduce2d, dali_open_set_search): a set of
//   frames stands for one search unit.  Three memory-bound kernels that read their input once: feature rows pooled per template, a
//   frame-level distance block reduced to template-level entries, and the per-probe open-set search of a distance matrix.
//   The arithmetic orders are the header's and are spelled with __fmul_rn / __fadd_rn / __fdiv_rn: no contraction, whatever the flags.
//   order / bounds are device data the entries cannot inspect: the kernels compare every index and bound with its range before it
//   becomes an address, skip what lies outside and report it in a status word (integer atomicOr; no atomics on floats).
#include "common.h"

namespace dali {

constexpr int TPL_THREADS = 256;
constexpr int POOL_UNROLL = 8;                  // gathered rows in flight per lane
constexpr int POOL_MEAN = 0, POOL_MAX = 1;
constexpr int SEG_MIN = 0, SEG_MAX = 1, SEG_MEAN = 2;
constexpr int TPL_BAD_INDEX = 1, TPL_BAD_BOUNDS = 2;

// ---- dali_pool_rows ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float pool_fill(const float*, float v) { return v; }
__device__ __forceinline__ f32x4_t pool_fill(const f32x4_t*, float v) { return f32x4_t{v, v, v, v}; }
// MEAN: acc + (w * x), the product rounded, then the sum rounded.  MAX: x where x > acc (a NaN is never taken, the first of equal zeros stays).
template <int MODE>
__device__ __forceinline__ float pool_step(float acc, float w, float x) {
    if (MODE == POOL_MEAN) return __fadd_rn(acc, __fmul_rn(w, x));
    return x > acc ? x : acc;
}
template <int MODE>
__device__ __forceinline__ f32x4_t pool_step(f32x4_t acc, float w, f32x4_t x) {
    return f32x4_t{pool_step<MODE>(acc[0], w, x[0]), pool_step<MODE>(acc[1], w, x[1]), pool_step<MODE>(acc[2], w, x[2]), pool_step<MODE>(acc[3], w, x[3])};
}
__device__ __forceinline__ float pool_div(float a, float s) { return __fdiv_rn(a, s); }
__device__ __forceinline__ f32x4_t pool_div(f32x4_t a, float s) {
    return f32x4_t{__fdiv_rn(a[0], s), __fdiv_rn(a[1], s), __fdiv_rn(a[2], s), __fdiv_rn(a[3], s)};
}

// U members i .. i + U - 1 of one output element (or 4 of them, for the 16-byte V): all U loads are issued before the first use.  A row
// number outside [0, n) loads row 0 (n >= 1) and is left out by a select, so that no load sits behind a branch.
template <int MODE, int U, class V>
__device__ __forceinline__ void pool_members(const V* __restrict__ fvs, int n, size_t row_elems, int c, const int32_t* __restrict__ order,
                                              const float* __restrict__ weights, int i, V& acc, float& wsum, int& bad) {
    int g[U];
    float w[U];
    V x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        g[u] = order[i + u];
        if (g[u] < 0 || g[u] >= n) { g[u] = -1; bad = 1; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        w[u] = (MODE == POOL_MEAN && weights) ? weights[g[u] < 0 ? 0 : g[u]] : 1.0f;
        x[u] = fvs[(size_t)(g[u] < 0 ? 0 : g[u]) * row_elems + c];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const V a = pool_step<MODE>(acc, w[u], x[u]);
        const float s = __fadd_rn(wsum, w[u]);
        acc = g[u] < 0 ? acc : a;
        wsum = g[u] < 0 ? wsum : s;
    }
}

// One thread per output element (V = float) or per 4 of them (V = f32x4_t); the threads of a wave that share a template read one
// contiguous stretch of every member row.  Every thread walks its template's members in member order.
template <int MODE, class V>
__global__ __launch_bounds__(TPL_THREADS) void pool_rows_kernel(const V* __restrict__ fvs, int n, int row_elems, const int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ bounds, int n_templates,
                                                                const float* __restrict__ weights, V* __restrict__ out, int32_t* __restrict__ status) {
    const size_t gid = (size_t)blockIdx.x * TPL_THREADS + threadIdx.x;
    if (gid >= (size_t)n_templates * row_elems) return;
    const int t = (int)(gid / (size_t)row_elems), c = (int)(gid % (size_t)row_elems);
    const int b0 = bounds[t], b1 = bounds[t + 1];
    if (b0 < 0 || b1 > n || b1 <= b0) {          // never an address: the template's row is zeroed and the call reports it
        if (c == 0) atomicOr(status, TPL_BAD_BOUNDS);
        out[gid] = pool_fill(fvs, 0.0f);
        return;
    }
    V acc = pool_fill(fvs, MODE == POOL_MEAN ? 0.0f : -__builtin_inff());
    float wsum = 0.0f;
    int bad = 0, i = b0;
    for (; i + POOL_UNROLL <= b1; i += POOL_UNROLL) pool_members<MODE, POOL_UNROLL>(fvs, n, (size_t)row_elems, c, order, weights, i, acc, wsum, bad);
    for (; i < b1; ++i) pool_members<MODE, 1>(fvs, n, (size_t)row_elems, c, order, weights, i, acc, wsum, bad);
    if (bad && c == 0) atomicOr(status, TPL_BAD_INDEX);
    if (MODE == POOL_MEAN) acc = pool_div(acc, weights ? wsum : (float)(b1 - b0));
    out[gid] = acc;
}

// ---- dali_segment_reduce2d -----------------------------------------------------------------------------------------------------

// min / max in the total order of the bits (-0.0 below +0.0; a NaN beyond the infinity of its sign): no result depends on the order
// in which the entries are met.  mean: the rounded sum.
__device__ __forceinline__ int seg_key(float x) {
    const int k = __float_as_int(x);
    return k ^ ((k >> 31) & 0x7fffffff);
}
template <int MODE>
__device__ __forceinline__ float seg_op(float a, float b) {
    if (MODE == SEG_MIN) return seg_key(b) < seg_key(a) ? b : a;
    if (MODE == SEG_MAX) return seg_key(b) > seg_key(a) ? b : a;
    return __fadd_rn(a, b);
}

__device__ __forceinline__ int seg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Workgroup (a, ct): row segment a and the column segments that START inside the 256-column window ct.  Their columns are walked in
// chunks of 256: thread j reduces column c + j over the rows of a (coalesced, ascending row) into LDS, then thread s folds the column
// results of segment b_lo + s in ascending column order, carrying its accumulator from chunk to chunk.  Every entry is read once.
template <int MODE>
__global__ __launch_bounds__(TPL_THREADS) void segment_reduce2d_kernel(const float* __restrict__ x, int rows, int cols, size_t ld,
                                                                       const int32_t* __restrict__ row_bounds, const int32_t* __restrict__ col_bounds,
                                                                       int n_col_segs, int n_windows, float* __restrict__ out, size_t out_ld,
                                                                       int32_t* __restrict__ status) {
    __shared__ float s_col[TPL_THREADS];
    __shared__ int s_seg[2];
    const int a = blockIdx.x / n_windows, ct = blockIdx.x % n_windows;
    const int tid = threadIdx.x;
    if (tid < 2) {                               // the first segment whose start is >= (ct + tid) * 256, or n_col_segs
        const long long want = (long long)(ct + tid) * TPL_THREADS;
        int lo = 0, hi = n_col_segs;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((long long)col_bounds[mid] >= want) hi = mid; else lo = mid + 1;
        }
        s_seg[tid] = lo;
    }
    __syncthreads();
    const int b_lo = s_seg[0];
    int b_hi = s_seg[1];
    if (b_hi <= b_lo) return;                    // no segment starts in this window (uniform over the workgroup)
    if (b_hi - b_lo > TPL_THREADS) {             // more starts than columns: the bounds do not increase
        if (tid == 0) atomicOr(status, TPL_BAD_BOUNDS);
        b_hi = b_lo + TPL_THREADS;
    }
    const int r0 = row_bounds[a], r1 = row_bounds[a + 1];
    if (r0 < 0 || r1 > rows || r1 <= r0) {
        if (tid == 0) atomicOr(status, TPL_BAD_BOUNDS);
        return;
    }
    const int cs = seg_clamp(col_bounds[b_lo], 0, cols), ce = seg_clamp(col_bounds[b_hi], 0, cols);
    const bool mine = b_lo + tid < b_hi;
    const int s0 = mine ? col_bounds[b_lo + tid] : 0, s1 = mine ? col_bounds[b_lo + tid + 1] : 0;
    float acc = 0.0f;
    bool have = false;
    for (int c = cs; c < ce; c += TPL_THREADS) {
        const int j = c + tid;
        if (j < ce) {
            const float* p = x + (size_t)r0 * ld + j;
            float v = p[0];
            int r = r0 + 1;
            for (; r + 4 <= r1; r += 4) {
                const size_t o = (size_t)(r - r0) * ld;
                const float v0 = p[o], v1 = p[o + ld], v2 = p[o + 2 * ld], v3 = p[o + 3 * ld];
                v = seg_op<MODE>(seg_op<MODE>(seg_op<MODE>(seg_op<MODE>(v, v0), v1), v2), v3);
            }
            for (; r < r1; ++r) v = seg_op<MODE>(v, p[(size_t)(r - r0) * ld]);
            s_col[tid] = v;
        }
        __syncthreads();
        if (mine) {
            const int lo = s0 > c ? s0 : c;
            int hi = s1 < c + TPL_THREADS ? s1 : c + TPL_THREADS;
            hi = hi < ce ? hi : ce;
            for (int jj = lo; jj < hi; ++jj) {
                const float v = s_col[jj - c];
                acc = have ? seg_op<MODE>(acc, v) : v;
                have = true;
            }
        }
        __syncthreads();
    }
    if (!mine) return;
    if (!have || s0 < cs || s1 > ce || s1 <= s0) {
        atomicOr(status, TPL_BAD_BOUNDS);
        return;
    }
    if (MODE == SEG_MEAN) acc = __fdiv_rn(acc, (float)((long long)(r1 - r0) * (long long)(s1 - s0)));
    out[(size_t)a * out_ld + (size_t)(b_lo + tid)] = acc;
}

// ---- dali_open_set_search ------------------------------------------------------------------------------------------------------

struct OsBest {                                  // the smallest distance met and the smallest column that holds it; col == INT_MAX: none yet
    float d;
    int col;
};
__device__ __forceinline__ void os_take(OsBest& b, float d, int col) {
    if (d < b.d || (d == b.d && col < b.col)) { b.d = d; b.col = col; }
}
__device__ __forceinline__ OsBest os_wave_min(OsBest b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float d = __shfl_xor(b.d, o, 64);
        const int col = __shfl_xor(b.col, o, 64);
        os_take(b, d, col);
    }
    return b;
}

// One workgroup per probe.  Pass 1: (min, first column) over the mates and over the non-mates.  Pass 2 (mated probes): the non-mates
// that sort before the best mate.  VEC: the row and the subject codes are read 16 bytes per lane; the last ng % 4 columns one by one.
template <int VEC>
__global__ __launch_bounds__(TPL_THREADS) void open_set_search_kernel(const float* __restrict__ x, int nq, int ng, size_t ld, const int32_t* __restrict__ q_subj,
                                                                      const int32_t* __restrict__ g_subj, float* __restrict__ mate_dist,
                                                                      int32_t* __restrict__ mate_col, float* __restrict__ nonmate_dist,
                                                                      int32_t* __restrict__ nonmate_col, int32_t* __restrict__ rank) {
    __shared__ float s_d[2][TPL_THREADS / 64];
    __shared__ int s_c[2][TPL_THREADS / 64];
    __shared__ int s_n[TPL_THREADS / 64];
    const int i = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* row = x + (size_t)i * ld;
    const int me = q_subj[i];
    const float inf = __builtin_inff();
    const int none = 0x7fffffff;
    const int nvec = VEC ? (ng >> 2) : 0;
    OsBest m{inf, none}, u{inf, none};
    for (int v = tid; v < nvec; v += TPL_THREADS) {
        const f32x4_t d4 = reinterpret_cast<const f32x4_t*>(row)[v];
        const int4 s4 = reinterpret_cast<const int4*>(g_subj)[v];
        const int j = v << 2;
        if (s4.x == me) os_take(m, d4[0], j); else os_take(u, d4[0], j);
        if (s4.y == me) os_take(m, d4[1], j + 1); else os_take(u, d4[1], j + 1);
        if (s4.z == me) os_take(m, d4[2], j + 2); else os_take(u, d4[2], j + 2);
        if (s4.w == me) os_take(m, d4[3], j + 3); else os_take(u, d4[3], j + 3);
    }
    for (int j = (nvec << 2) + tid; j < ng; j += TPL_THREADS) {
        if (g_subj[j] == me) os_take(m, row[j], j); else os_take(u, row[j], j);
    }
    m = os_wave_min(m);
    u = os_wave_min(u);
    if (lane == 0) { s_d[0][wave] = m.d; s_c[0][wave] = m.col; s_d[1][wave] = u.d; s_c[1][wave] = u.col; }
    __syncthreads();
    m = OsBest{s_d[0][0], s_c[0][0]};
    u = OsBest{s_d[1][0], s_c[1][0]};
#pragma unroll
    for (int w = 1; w < TPL_THREADS / 64; ++w) { os_take(m, s_d[0][w], s_c[0][w]); os_take(u, s_d[1][w], s_c[1][w]); }
    const bool mated = m.col != none;
    if (tid == 0) {
        mate_dist[i] = m.d;
        mate_col[i] = mated ? m.col : -1;
        nonmate_dist[i] = u.d;
        nonmate_col[i] = u.col != none ? u.col : -1;
        if (!mated) rank[i] = -1;
    }
    if (!mated) return;                          // uniform over the workgroup
    int cnt = 0;
    for (int v = tid; v < nvec; v += TPL_THREADS) {
        const f32x4_t d4 = reinterpret_cast<const f32x4_t*>(row)[v];
        const int4 s4 = reinterpret_cast<const int4*>(g_subj)[v];
        const int j = v << 2;
        cnt += (s4.x != me) && (d4[0] < m.d || (d4[0] == m.d && j < m.col));
        cnt += (s4.y != me) && (d4[1] < m.d || (d4[1] == m.d && j + 1 < m.col));
        cnt += (s4.z != me) && (d4[2] < m.d || (d4[2] == m.d && j + 2 < m.col));
        cnt += (s4.w != me) && (d4[3] < m.d || (d4[3] == m.d && j + 3 < m.col));
    }
    for (int j = (nvec << 2) + tid; j < ng; j += TPL_THREADS) {
        const float d = row[j];
        cnt += (g_subj[j] != me) && (d < m.d || (d == m.d && j < m.col));
    }
    cnt = wave_sum_i(cnt);
    if (lane == 0) s_n[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < TPL_THREADS / 64; ++w) total += s_n[w];
        rank[i] = total;
    }
}

template <class V>
static void pool_launch(int mode, unsigned grid, hipStream_t st, const float* fvs, int n, int row_elems, const int32_t* order, const int32_t* bounds,
                        int n_templates, const float* weights, float* out, int32_t* status) {
    if (mode == POOL_MEAN)
        hipLaunchKernelGGL((pool_rows_kernel<POOL_MEAN, V>), dim3(grid), dim3(TPL_THREADS), 0, st, reinterpret_cast<const V*>(fvs), n, row_elems, order,
                           bounds, n_templates, weights, reinterpret_cast<V*>(out), status);
    else
        hipLaunchKernelGGL((pool_rows_kernel<POOL_MAX, V>), dim3(grid), dim3(TPL_THREADS), 0, st, reinterpret_cast<const V*>(fvs), n, row_elems, order,
                           bounds, n_templates, weights, reinterpret_cast<V*>(out), status);
}

}  // namespace dali

using namespace dali;

static inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

extern "C" int dali_pool_rows(dali_ctx* ctx, void* stream, const float* fvs, int n, int d, const int32_t* order, const int32_t* bounds,
                              int n_templates, const float* weights, int mode, float* out, int32_t* status) {
    DALI_REQUIRE(mode == POOL_MEAN || mode == POOL_MAX, "dali_pool_rows: mode=%d (0 weighted mean, 1 max)", mode);
    DALI_REQUIRE(d >= 1, "dali_pool_rows: d=%d", d);
    DALI_REQUIRE(n >= 1 && n_templates >= 1 && n_templates <= n, "dali_pool_rows: n=%d rows in n_templates=%d templates (every template holds a row)",
                 n, n_templates);
    DALI_REQUIRE(ctx && fvs && order && bounds && out && status, "dali_pool_rows: null argument");
    DALI_REQUIRE(!(weights && mode == POOL_MAX), "dali_pool_rows: weights with mode=1 (the maximum takes none)");
    DALI_REQUIRE(((addr(fvs) | addr(out) | addr(order) | addr(bounds) | addr(weights) | addr(status)) & 3) == 0, "dali_pool_rows: misaligned pointer");
    const uintptr_t p0 = addr(fvs), p1 = p0 + (size_t)n * d * sizeof(float), o0 = addr(out), o1 = o0 + (size_t)n_templates * d * sizeof(float);
    DALI_REQUIRE(o1 <= p0 || p1 <= o0, "dali_pool_rows: out overlaps fvs (rows are gathered while others are written)");
    const bool vec = (d & 3) == 0 && ((p0 | o0) & 15) == 0;
    const int row_elems = vec ? d >> 2 : d;
    const size_t blocks = ((size_t)n_templates * row_elems + TPL_THREADS - 1) / TPL_THREADS;
    DALI_REQUIRE(blocks <= 0x7fffffffu, "dali_pool_rows: n_templates=%d x d=%d needs more than 2^31 - 1 workgroups", n_templates, d);
    if (vec) pool_launch<f32x4_t>(mode, (unsigned)blocks, (hipStream_t)stream, fvs, n, row_elems, order, bounds, n_templates, weights, out, status);
    else pool_launch<float>(mode, (unsigned)blocks, (hipStream_t)stream, fvs, n, row_elems, order, bounds, n_templates, weights, out, status);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_segment_reduce2d(dali_ctx* ctx, void* stream, const float* x, int rows, int cols, int64_t ld, const int32_t* row_bounds,
                                     int n_row_segs, const int32_t* col_bounds, int n_col_segs, int mode, float* out, int out_rows,
                                     int64_t out_ld, int out_row0, int out_col0, int32_t* status) {
    DALI_REQUIRE(mode == SEG_MIN || mode == SEG_MAX || mode == SEG_MEAN, "dali_segment_reduce2d: mode=%d (0 min, 1 max, 2 mean)", mode);
    DALI_REQUIRE(rows >= 1 && cols >= 1, "dali_segment_reduce2d: bad shape rows=%d cols=%d", rows, cols);
    DALI_REQUIRE(ld >= cols, "dali_segment_reduce2d: ld=%lld below cols=%d", (long long)ld, cols);
    DALI_REQUIRE(n_row_segs >= 1 && n_row_segs <= rows && n_col_segs >= 1 && n_col_segs <= cols,
                 "dali_segment_reduce2d: %d row segments of %d rows, %d column segments of %d columns (every segment holds an entry)", n_row_segs,
                 rows, n_col_segs, cols);
    DALI_REQUIRE(out_row0 >= 0 && out_col0 >= 0 && (long long)out_row0 + n_row_segs <= out_rows && (long long)out_col0 + n_col_segs <= out_ld,
                 "dali_segment_reduce2d: the %d x %d block at (%d, %d) does not lie inside out [%d rows, pitch %lld]", n_row_segs, n_col_segs,
                 out_row0, out_col0, out_rows, (long long)out_ld);
    DALI_REQUIRE(ctx && x && row_bounds && col_bounds && out && status, "dali_segment_reduce2d: null argument");
    DALI_REQUIRE(((addr(x) | addr(out) | addr(row_bounds) | addr(col_bounds) | addr(status)) & 3) == 0, "dali_segment_reduce2d: misaligned pointer");
    const int n_windows = (cols + TPL_THREADS - 1) / TPL_THREADS;
    DALI_REQUIRE((long long)n_row_segs * n_windows <= 0x7fffffffLL, "dali_segment_reduce2d: %d row segments x %d column windows exceed 2^31 - 1 workgroups",
                 n_row_segs, n_windows);
    const dim3 grid((unsigned)(n_row_segs * n_windows));
    out += (size_t)out_row0 * (size_t)out_ld + (size_t)out_col0;
    const hipStream_t st = (hipStream_t)stream;
    if (mode == SEG_MIN)
        hipLaunchKernelGGL(segment_reduce2d_kernel<SEG_MIN>, grid, dim3(TPL_THREADS), 0, st, x, rows, cols, (size_t)ld, row_bounds, col_bounds, n_col_segs,
                           n_windows, out, (size_t)out_ld, status);
    else if (mode == SEG_MAX)
        hipLaunchKernelGGL(segment_reduce2d_kernel<SEG_MAX>, grid, dim3(TPL_THREADS), 0, st, x, rows, cols, (size_t)ld, row_bounds, col_bounds, n_col_segs,
                           n_windows, out, (size_t)out_ld, status);
    else
        hipLaunchKernelGGL(segment_reduce2d_kernel<SEG_MEAN>, grid, dim3(TPL_THREADS), 0, st, x, rows, cols, (size_t)ld, row_bounds, col_bounds, n_col_segs,
                           n_windows, out, (size_t)out_ld, status);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_open_set_search(dali_ctx* ctx, void* stream, const float* distmat, int nq, int ng, int64_t ld, const int32_t* q_subj,
                                    const int32_t* g_subj, float* mate_dist, int32_t* mate_col, float* nonmate_dist, int32_t* nonmate_col,
                                    int32_t* rank) {
    DALI_REQUIRE(nq >= 1 && ng >= 1, "dali_open_set_search: bad shape nq=%d ng=%d", nq, ng);
    DALI_REQUIRE(ld >= ng, "dali_open_set_search: ld=%lld below ng=%d", (long long)ld, ng);
    DALI_REQUIRE(ctx && distmat && q_subj && g_subj && mate_dist && mate_col && nonmate_dist && nonmate_col && rank, "dali_open_set_search: null argument");
    DALI_REQUIRE(((addr(distmat) | addr(q_subj) | addr(g_subj) | addr(mate_dist) | addr(mate_col) | addr(nonmate_dist) | addr(nonmate_col) | addr(rank)) & 3) == 0,
                 "dali_open_set_search: misaligned pointer");
    const bool vec = ((addr(distmat) | addr(g_subj)) & 15) == 0 && (ld & 3) == 0;
    const hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(open_set_search_kernel<1>, dim3((unsigned)nq), dim3(TPL_THREADS), 0, st, distmat, nq, ng, (size_t)ld, q_subj, g_subj, mate_dist,
                           mate_col, nonmate_dist, nonmate_col, rank);
    else
        hipLaunchKernelGGL(open_set_search_kernel<0>, dim3((unsigned)nq), dim3(TPL_THREADS), 0, st, distmat, nq, ng, (size_t)ld, q_subj, g_subj, mate_dist,
                           mate_col, nonmate_dist, nonmate_col, rank);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

// metarec.hip -- Weibull meta-recognition score fusion (include/daliid.h: dali_mr_kill_transpose, dali_mr_fit_rows, dali_mr_wscore,
//   dali_mr_fuse; the reference's libmr / Meta_Recognition, evaluate.py:394-627).  The selections come from dali_topk_rows (topk.hip), so
//   "the topk largest" and "the tail" are THE ORDER of topk_key.h.  The fit keeps a row's log terms in LDS across its Newton steps: a wave
//   per row for short rows, a workgroup of 4 or 16 waves per row beyond; every row stops on its own.  All sums are fp64 in a fixed order.
#include "kernels.h"
#include "topk_key.h"

namespace dali {

constexpr int MR_N_WAVE = 1024;                  // rows up to here: one wave per row, 4 rows per workgroup (<= 16 elements per lane)
constexpr int MR_N_QUAD = 4096;                  // up to here: one 256-thread workgroup per row; beyond: one of 1024 threads
constexpr int MR_N_MAX = 16384;                  // 128 KiB of fp64 log terms: what one workgroup can hold of the CU's 160 KiB
constexpr int MR_ITERS = 100;
constexpr double MR_EPS = 1e-6;
constexpr double MR_SKIP = -1.7976931348623157e308;   // marks an element outside the tail in the LDS row (no logarithm returns it)

// ---- kill + transpose -----------------------------------------------------------------------------------------------------------------
// KT[j][i] = S[i][j] through a 32 x 32 LDS tile: rows of S are read and rows of KT are written in 128-byte runs.
__global__ __launch_bounds__(256) void mr_transpose_kernel(const float* __restrict__ S, int nq, int ng, int tiles_j, float* __restrict__ KT,
                                                            int32_t* __restrict__ status) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = (int)(blockIdx.x / (unsigned)tiles_j) * 32, j0 = (int)(blockIdx.x % (unsigned)tiles_j) * 32;
    bool bad = false;
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, j = j0 + tx;
        if (i < nq && j < ng) {
            const float v = S[(size_t)i * ng + j];
            bad |= !isfinite(v);
            tile[r][tx] = v;
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int j = j0 + r, i = i0 + tx;
        if (i < nq && j < ng) KT[(size_t)j * nq + i] = tile[tx][r];
    }
    if (bad) status[0] = 1;
}

// One thread per selected entry: keys [rows][topk] of the rows of S (by_columns == 0: row = i, index = j) or of the rows of KT
// (row = j, index = i).  Either way the entry is KT[j][i], which holds S[i][j].
__global__ __launch_bounds__(256) void mr_kill_kernel(const unsigned long long* __restrict__ keys, long long n_keys, int topk, int by_columns,
                                                       int nq, int ng, float killscale, float* __restrict__ KT) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_keys) return;
    const unsigned row = (unsigned)(e / topk), idx = (unsigned)keys[e];
    const unsigned i = by_columns ? idx : row, j = by_columns ? row : idx;
    if (i >= (unsigned)nq || j >= (unsigned)ng) return;            // an unfilled slot (cannot happen for topk <= columns)
    float* p = KT + (size_t)j * nq + i;
    const float s = *p;
    *p = s - killscale * s;
}

// ---- fit ------------------------------------------------------------------------------------------------------------------------------
// Sums of three doubles over the W waves of a row, the same value in every lane: xor butterfly inside the wave, then the wave totals in
// wave order through LDS.  W > 1: every thread of the workgroup calls it (two barriers).
template <int W>
__device__ __forceinline__ void mr_row_sum3(double& a, double& b, double& c, double* s_red, int wave, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if constexpr (W > 1) {
        __syncthreads();                                          // the readers of the previous sums are done
        if (lane == 0) { s_red[wave] = a; s_red[W + wave] = b; s_red[2 * W + wave] = c; }
        __syncthreads();
        a = b = c = 0.0;
#pragma unroll
        for (int w = 0; w < W; ++w) { a += s_red[w]; b += s_red[W + w]; c += s_red[2 * W + w]; }
    }
}

// W waves per row; W == 1: 4 rows per 256-thread workgroup and no barrier anywhere, so that each wave leaves when its row is done.
// Dynamic LDS: (rows per workgroup) * n doubles + 3 W doubles.  A thread reads back only the LDS words it wrote itself.
template <int W>
__global__ __launch_bounds__(W == 1 ? 256 : W * 64) void mr_fit_kernel(const float* __restrict__ x, int nrows, int n, int T,
                                                                       const unsigned long long* __restrict__ keys, int kk,
                                                                       double* __restrict__ fits, float* __restrict__ small,
                                                                       int32_t* __restrict__ iters, int32_t* __restrict__ status) {
    extern __shared__ double s_dyn[];
    constexpr int RPB = W == 1 ? 4 : 1, TS = W * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = W == 1 ? wave : 0, t0 = W == 1 ? lane : tid;
    const int r = blockIdx.x * RPB + sub;
    if (r >= nrows) return;                                       // W == 1 only (whole waves); a W > 1 grid has exactly nrows workgroups
    double* sL = s_dyn + (size_t)sub * n;
    double* s_red = s_dyn + (size_t)RPB * n;
    const float* xr = x + (size_t)r * n;
    const unsigned long long bkey = keys[(size_t)r * kk + (kk - 1)];
    const unsigned bidx = (unsigned)bkey;
    const float sm = bidx < (unsigned)n ? xr[bidx] : 0.f;
    const double dT = (double)T;
    double suml = 0.0, z0 = 0.0, z1 = 0.0;
    bool bad = false;
    for (int t = t0; t < n; t += TS) {
        const float v = xr[t];
        bad |= !isfinite(v);
        double L = MR_SKIP;
        if (topk_key(v, t, 0) >= bkey) {
            const float xt = (v + 1.0f) - sm;
            L = log((double)xt);
            suml += (double)(float)L;
        }
        sL[t] = L;
    }
    if (bad) status[0] = 1;
    mr_row_sum3<W>(suml, z0, z1, s_red, wave, lane);
    const double mean_l = suml / dT;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double k = 1.0, shape = nan, scale = nan;
    int it = 0;
    bool fit = false;
    while (it < MR_ITERS) {
        ++it;
        double fg = 0.0, ff = 0.0, ffp = 0.0;
        for (int t = t0; t < n; t += TS) {
            const double L = sL[t];
            if (L != MR_SKIP) {
                const double e = exp(k * L), l = (double)(float)L, el = e * l;
                fg += e; ff += el; ffp += el * l;
            }
        }
        mr_row_sum3<W>(fg, ff, ffp, s_red, wave, lane);
        const double q = ff / fg;
        const double f = q - mean_l - 1.0 / k;
        const double fp = ffp / fg - q * q + 1.0 / (k * k);
        const double kn = k - f / fp;
        if (!(isfinite(f) && isfinite(fp) && isfinite(kn))) break;
        if (fabs(kn - k) < MR_EPS) {
            double g = 0.0, u0 = 0.0, u1 = 0.0;
            for (int t = t0; t < n; t += TS) {
                const double L = sL[t];
                if (L != MR_SKIP) g += exp(kn * L);
            }
            mr_row_sum3<W>(g, u0, u1, s_red, wave, lane);
            shape = kn;
            scale = pow(g / dT, 1.0 / kn);
            fit = true;
            break;
        }
        k = kn;
    }
    if (t0 == 0) {
        fits[2 * (size_t)r] = shape;
        fits[2 * (size_t)r + 1] = scale;
        small[r] = sm;
        if (iters) iters[r] = it;
        if (!fit) atomicAdd(&status[1], 1);
    }
}

// ---- w-score and fusion ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double mr_wscore_one(float s, float sm, double shape, double scale) {
    const float d = (s + 1.0f) - sm;
    if (!(d > 0.f) || shape != shape || scale != scale) return 0.0;
    return 1.0 - exp(-pow((double)d / scale, shape));
}

// grid (column blocks of 256, rows): a thread keeps its column's fit and walks the rows blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(256) void mr_wscore_kernel(const float* __restrict__ S, int nq, int ng, const double* __restrict__ fits,
                                                         const float* __restrict__ small, double* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ng) return;
    const double shape = fits[2 * (size_t)j], scale = fits[2 * (size_t)j + 1];
    const float sm = small[j];
    for (int i = blockIdx.y; i < nq; i += gridDim.y) {
        const size_t e = (size_t)i * ng + j;
        out[e] = mr_wscore_one(S[e], sm, shape, scale);
    }
}

struct MrFuseArgs {
    const float* s[4];
    const double* fits[4];
    const float* small[4];
    int m;
};
template <bool F64>
__global__ __launch_bounds__(256) void mr_fuse_kernel(MrFuseArgs a, int nq, int ng, void* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ng) return;
    double shape[4], scale[4];
    float sm[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c < a.m) { shape[c] = a.fits[c][2 * (size_t)j]; scale[c] = a.fits[c][2 * (size_t)j + 1]; sm[c] = a.small[c][j]; }
    }
    for (int i = blockIdx.y; i < nq; i += gridDim.y) {
        const size_t e = (size_t)i * ng + j;
        double num = 0.0, den = 0.0, sum = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < a.m) {
                const float s = a.s[c][e];
                const double w = mr_wscore_one(s, sm[c], shape[c], scale[c]);
                num += w * (double)s;
                den += w;
                sum += (double)s;
            }
        }
        const double v = den == 0.0 ? sum / (double)a.m : num / den;
        if (F64) static_cast<double*>(out)[e] = v;
        else static_cast<float*>(out)[e] = (float)v;
    }
}

static dim3 mr_grid_cols_rows(int nq, int ng) { return dim3((unsigned)((ng + 255) / 256), (unsigned)(nq < 65535 ? nq : 65535)); }

template <int W>
static int launch_mr_fit(hipStream_t st, const float* x, int nrows, int n, int T, const unsigned long long* keys, int kk, double* fits,
                         float* small, int32_t* iters, int32_t* status) {
    constexpr int RPB = W == 1 ? 4 : 1;
    const size_t lds = ((size_t)RPB * n + 3 * W) * sizeof(double);
    if (W == 16) {
        DALI_ONCE_PER_DEVICE(DALI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mr_fit_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                          (MR_N_MAX + 3 * 16) * (int)sizeof(double))));
    }
    hipLaunchKernelGGL((mr_fit_kernel<W>), dim3((unsigned)((nrows + RPB - 1) / RPB)), dim3(W == 1 ? 256 : W * 64), lds, st, x, nrows, n, T, keys, kk,
                       fits, small, iters, status);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

}  // namespace dali

using namespace dali;

extern "C" int dali_mr_kill_transpose(dali_ctx* ctx, void* stream, const float* S, int nq, int ng, int topk, int use_columns, double killscale,
                                      float* KT, int32_t* status) {
    DALI_REQUIRE(ctx && S && KT && status, "dali_mr_kill_transpose: null argument");
    DALI_REQUIRE(nq >= 1 && ng >= 1, "dali_mr_kill_transpose: bad shape nq=%d ng=%d", nq, ng);
    DALI_REQUIRE(topk >= 1 && (long long)nq >= (long long)topk + 2, "dali_mr_kill_transpose: topk=%d needs nq >= topk + 2, nq=%d", topk, nq);
    DALI_REQUIRE(use_columns || ng >= topk, "dali_mr_kill_transpose: topk=%d entries per row of ng=%d", topk, ng);
    if (topk > TOPK_K_MAX) { set_error("dali_mr_kill_transpose: topk=%d above the documented cap %d", topk, TOPK_K_MAX); return DALI_ERR_LIMIT; }
    hipStream_t st = (hipStream_t)stream;
    const int rows = use_columns ? ng : nq;
    const long long n_keys = (long long)rows * topk;
    unsigned long long* keys = static_cast<unsigned long long*>(workspace(ctx, (size_t)n_keys * 8));
    if (!keys) return DALI_ERR_NOMEM;
    DALI_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    const int tiles_j = (ng + 31) / 32;
    const long long tiles = (long long)((nq + 31) / 32) * tiles_j;
    if (tiles > 0x7fffffffll) { set_error("dali_mr_kill_transpose: %d x %d has too many tiles", nq, ng); return DALI_ERR_LIMIT; }
    if (!use_columns) {
        if (int rc = dali_topk_rows(ctx, stream, S, nq, ng, ng, 0, topk, 1, 0, reinterpret_cast<int64_t*>(keys))) return rc;
    }
    hipLaunchKernelGGL(mr_transpose_kernel, dim3((unsigned)tiles), dim3(256), 0, st, S, nq, ng, tiles_j, KT, status);
    DALI_LAUNCH_CHECK();
    if (use_columns) {
        if (int rc = dali_topk_rows(ctx, stream, KT, ng, nq, nq, 0, topk, 1, 0, reinterpret_cast<int64_t*>(keys))) return rc;
    }
    hipLaunchKernelGGL(mr_kill_kernel, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, st, keys, n_keys, topk, use_columns ? 1 : 0, nq, ng,
                       (float)killscale, KT);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_mr_fit_rows(dali_ctx* ctx, void* stream, const float* x, int nrows, int n, int tail, double* fits, float* small_out,
                                int32_t* iters, int32_t* status) {
    DALI_REQUIRE(ctx && x && fits && small_out && status, "dali_mr_fit_rows: null argument");
    DALI_REQUIRE(nrows >= 0 && n >= 1, "dali_mr_fit_rows: bad shape nrows=%d n=%d", nrows, n);
    DALI_REQUIRE(tail >= 1 && tail <= n, "dali_mr_fit_rows: tail=%d outside 1 .. n=%d", tail, n);
    const int kk = n - tail + 1;
    if (kk > TOPK_K_MAX) { set_error("dali_mr_fit_rows: n - tail + 1 = %d above the documented cap %d", kk, TOPK_K_MAX); return DALI_ERR_LIMIT; }
    if (n > MR_N_MAX) { set_error("dali_mr_fit_rows: n=%d above the documented cap %d", n, MR_N_MAX); return DALI_ERR_LIMIT; }
    hipStream_t st = (hipStream_t)stream;
    DALI_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st));
    if (nrows == 0) return DALI_OK;
    unsigned long long* keys = static_cast<unsigned long long*>(workspace(ctx, (size_t)nrows * kk * 8));
    if (!keys) return DALI_ERR_NOMEM;
    if (int rc = dali_topk_rows(ctx, stream, x, nrows, n, n, 0, kk, 0, 0, reinterpret_cast<int64_t*>(keys))) return rc;
    if (n <= MR_N_WAVE) return launch_mr_fit<1>(st, x, nrows, n, tail, keys, kk, fits, small_out, iters, status);
    if (n <= MR_N_QUAD) return launch_mr_fit<4>(st, x, nrows, n, tail, keys, kk, fits, small_out, iters, status);
    return launch_mr_fit<16>(st, x, nrows, n, tail, keys, kk, fits, small_out, iters, status);
}

extern "C" int dali_mr_wscore(dali_ctx* ctx, void* stream, const float* S, int nq, int ng, const double* fits, const float* small_in, double* out) {
    DALI_REQUIRE(ctx && S && fits && small_in && out, "dali_mr_wscore: null argument");
    DALI_REQUIRE(nq >= 0 && ng >= 0, "dali_mr_wscore: bad shape nq=%d ng=%d", nq, ng);
    if (nq == 0 || ng == 0) return DALI_OK;
    hipLaunchKernelGGL(mr_wscore_kernel, mr_grid_cols_rows(nq, ng), dim3(256), 0, (hipStream_t)stream, S, nq, ng, fits, small_in, out);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_mr_fuse(dali_ctx* ctx, void* stream, const float* const* scores_host, const double* const* fits_host,
                            const float* const* small_host, int m, int nq, int ng, int out_fp64, void* out) {
    DALI_REQUIRE(ctx && scores_host && fits_host && small_host && out, "dali_mr_fuse: null argument");
    DALI_REQUIRE(m >= 1 && m <= 3, "dali_mr_fuse: m=%d models (1 .. 3)", m);
    DALI_REQUIRE(nq >= 0 && ng >= 0, "dali_mr_fuse: bad shape nq=%d ng=%d", nq, ng);
    MrFuseArgs a = {};
    a.m = m;
    for (int c = 0; c < m; ++c) {
        DALI_REQUIRE(scores_host[c] && fits_host[c] && small_host[c], "dali_mr_fuse: null pointer for model %d", c);
        a.s[c] = scores_host[c]; a.fits[c] = fits_host[c]; a.small[c] = small_host[c];
    }
    if (nq == 0 || ng == 0) return DALI_OK;
    if (out_fp64) hipLaunchKernelGGL((mr_fuse_kernel<true>), mr_grid_cols_rows(nq, ng), dim3(256), 0, (hipStream_t)stream, a, nq, ng, out);
    else hipLaunchKernelGGL((mr_fuse_kernel<false>), mr_grid_cols_rows(nq, ng), dim3(256), 0, (hipStream_t)stream, a, nq, ng, out);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

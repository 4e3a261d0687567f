// roc.hip -- exact ROC curve over every query-gallery pair (sklearn.metrics.roc_curve of evaluateCleanATModels.py:276-292) by counting,
// without a sort.  Definition, limits and scratch size: include/daliid.h (dali_roc_build / dali_roc_emit).
//
// key(s) = the 32-bit order-preserving image of the fp32 score s = 1 - D/2 (-0 folded to +0), split 12 / 10 / 10 (hi / mid / lo).
// Buckets (hi) and segments (hi, mid) are laid out in DESCENDING key order, so positions in the scratch run from the highest score down.
//
//   1. roc_hist1_kernel     one read of D: per-workgroup LDS histogram of hi (4096 bins), one atomic per non-empty bin; n_pos / n_neg;
//                           non-finite flag
//   2. roc_scan1_kernel     occupied buckets -> slots (descending), element bases, chunk-task prefix, partition cursors
//   3. roc_part1_kernel     second read of D: payload (low 20 key bits << 1 | label) scattered to its bucket (s1); a tile reserves its
//                           run of every bucket with one atomic, ranks inside the tile come from LDS
//   4. roc_mid_kernel<0>    per chunk of a bucket: LDS histogram of mid -> segment sizes
//   5. roc_scan2_kernel     per slot: segment bases (descending mid)
//   6. roc_mid_kernel<1>    s1 -> s2 grouped by (hi, mid)
//   7. per window of at most ROC_W slots (dense counters cnt[slot][lo20] = pos << 32 | neg, 8 MiB per slot):
//        roc_count_kernel   per chunk: LDS counters over 8 mids x 1024 lo, one 64-bit atomic per (workgroup, non-empty key)
//        roc_cmp*_kernel    reduce-then-scan compaction of the non-empty keys, descending, into the record arrays (key, pos, neg);
//                           the read clears the counters for the next window
//   8. roc_curveA/B         per-range sums of pos / neg / kept points (drop_intermediate marks need only the neighbours' counts) + scan
//   9. roc_emit_kernel      (dali_roc_emit) cumulative fps / tps and thresholds of the kept points
//
// Every count is an integer, so the order in which atomics land cannot change a result: the output is bitwise identical run to run.
// In LDS, a wave whose lanes all hit one bin adds once (the all-tied matrix would otherwise serialise on one address).
#include "block_prims.h"
#include <algorithm>

namespace {

typedef unsigned long long u64;

constexpr int ROC_TPB = 512;                 // threads of the streaming kernels
constexpr int ROC_EPT = 16;                  // elements per thread and tile
constexpr int ROC_TILE = ROC_TPB * ROC_EPT;  // 8192 elements per tile / chunk
constexpr int ROC_NB1 = 4096;                // hi buckets
constexpr int ROC_NMID = 1024;
constexpr int ROC_MSPAN = 8;                 // mids per LDS pass of the count kernel (32 KiB of counters)
constexpr int ROC_KEYS = 1 << 20;            // lo20 keys per bucket
constexpr int ROC_W_MAX = 256;               // slots per window (2 GiB of counters)
constexpr int ROC_GRID = 2048;               // grid of the grid-stride kernels
constexpr int ROC_CURVE_G = 1024;            // ranges of the curve kernels
constexpr int ROC_CMP_BLK = 8192;            // counter entries per compaction block

// meta words (u64) at the head of the scratch
enum { M_NOCC = 0, M_NTASK, M_BAD, M_NPOS, M_NNEG, M_NREC, M_NKEPT, M_COUNT = 8 };

struct Layout {
    size_t meta, bucket_cnt, cursor1, occ_bucket, slot_base, task_prefix, seg, blk, part, s1, s2, s3, cnt, total;
    int W;
};

Layout roc_layout(long long N) {
    Layout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = dali::align_up(o + bytes, 256); return at; };
    L.W = (int)std::min<long long>(ROC_W_MAX, std::min<long long>(ROC_NB1, N));
    L.meta = take(M_COUNT * 8);
    L.bucket_cnt = take(ROC_NB1 * 4);
    L.cursor1 = take(ROC_NB1 * 4);
    L.occ_bucket = take(ROC_NB1 * 4);
    L.slot_base = take((ROC_NB1 + 1) * 4);
    L.task_prefix = take((ROC_NB1 + 1) * 4);
    L.seg = take((size_t)ROC_NB1 * ROC_NMID * 4);
    L.blk = take((size_t)L.W * (ROC_KEYS / ROC_CMP_BLK) * 4);
    L.part = take((size_t)ROC_CURVE_G * 4 * 8);
    L.s1 = take((size_t)N * 4);
    L.s2 = take((size_t)N * 4);
    L.s3 = take((size_t)N * 4);
    L.cnt = take((size_t)L.W * ROC_KEYS * 8);
    L.total = o;
    return L;
}

// The key is dali::ordered_bits(s) for every finite and infinite s (the map agrees bit for bit there, -0 folded onto +0), and its inverse
// below IS ordered_bits_inv.  NaN policy of this file: a non-finite score sets `bad` (status 1 of dali_roc_build) and is still counted
// under its key, so a NaN's key reaches the point counts and the scratch.  The key is therefore taken from the raw bits, folding by
// comparison: ordered_bits folds by `s + 0.0f`, an addition, and what an addition leaves of a NaN's payload is the hardware's choice.
__device__ __forceinline__ unsigned roc_key(float d, bool& bad) {
    const float s = 1.0f - d / 2.0f;                        // numpy's fl32(1 - fl32(d / 2)); the library builds without contraction
    unsigned u = __float_as_uint(s);
    bad = (u & 0x7f800000u) == 0x7f800000u;
    if (u == 0x80000000u) u = 0u;                            // -0 and +0 are one score
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float roc_score(unsigned key) { return dali::ordered_bits_inv(key); }

__device__ __forceinline__ int roc_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ unsigned roc_mbcnt(u64 m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// h[bin] += inc for every valid lane; one LDS add when the wave's valid lanes share a bin.  Returns the old value plus the lane's rank
// among the valid lanes of the wave (only meaningful when every lane adds 1).
__device__ __forceinline__ unsigned roc_lds_add(unsigned* h, unsigned bin, unsigned inc, bool valid) {
    const u64 mv = __ballot(valid);
    if (mv == 0) return 0;
    const int leader = __ffsll((long long)mv) - 1;
    const unsigned b0 = __shfl(bin, leader, 64);
    const u64 ms = __ballot(valid && bin == b0);
    if (ms == mv) {                                          // wave-uniform
        const unsigned inc0 = __shfl(inc, leader, 64);
        const bool same_inc = __ballot(valid && inc == inc0) == mv;
        if (same_inc) {
            unsigned base = 0;
            if (roc_lane() == leader) base = atomicAdd(&h[b0], inc0 * (unsigned)__popcll(mv));
            base = __shfl(base, leader, 64);
            return base + roc_mbcnt(mv) * inc0;
        }
    }
    return valid ? atomicAdd(&h[bin], inc) : 0u;
}

// block-wide exclusive scan of NV u64 values (blockDim.x a multiple of 64, at most 1024); totals[] receive the block sums.
// `sh` holds at least 16 * NV u64.  Ends with a barrier, so `sh` may be reused at once.
template <int NV>
__device__ __forceinline__ void roc_block_scan(u64 (&v)[NV], u64 (&totals)[NV], u64* sh) {
    const int lane = roc_lane(), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u64 inc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        inc[k] = v[k];
        for (int d = 1; d < 64; d <<= 1) {
            const u64 t = dali::shfl_up_u64(inc[k], d);
            if (lane >= d) inc[k] += t;
        }
    }
    __syncthreads();
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < NV; ++k) sh[w * NV + k] = inc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        u64 before = 0, tot = 0;
        for (int x = 0; x < nw; ++x) {
            const u64 s = sh[x * NV + k];
            if (x < w) before += s;
            tot += s;
        }
        v[k] = before + inc[k] - v[k];
        totals[k] = tot;
    }
    __syncthreads();
}

__device__ __forceinline__ int roc_block_max(int v, int* sh) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if (roc_lane() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = sh[0];
    for (int x = 1; x < (int)(blockDim.x >> 6); ++x) m = max(m, sh[x]);
    __syncthreads();
    return m;
}

// the 16 elements of thread `tid` in tile `t`: e = t * TILE + k * (TPB * 4) + tid * 4 + c (float4 loads, 16-B aligned D)
struct RocTile {
    unsigned key[ROC_EPT];
    unsigned lab, valid, bad;
};

__device__ __forceinline__ void roc_load_tile(const float* __restrict__ D, const int32_t* __restrict__ qid, const int32_t* __restrict__ gid,
                                              unsigned ng, unsigned N, unsigned t, RocTile& T) {
    T.lab = T.valid = T.bad = 0;
#pragma unroll
    for (int k = 0; k < ROC_EPT / 4; ++k) {
        const unsigned e0 = t * (unsigned)ROC_TILE + (unsigned)(k * ROC_TPB * 4) + threadIdx.x * 4u;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (e0 + 3 < N) {
            const float4 v = *reinterpret_cast<const float4*>(D + e0);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (e0 + c < N) d[c] = D[e0 + c];
        }
        unsigned i = e0 < N ? e0 / ng : 0u, j = e0 < N ? e0 - i * ng : 0u;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int s = k * 4 + c;
            const bool ok = e0 + c < N;
            while (ok && j >= ng) { j -= ng; ++i; }
            bool b = false;
            T.key[s] = roc_key(d[c], b);
            if (ok) {
                T.valid |= 1u << s;
                if (qid[i] == gid[j]) T.lab |= 1u << s;
                if (b) T.bad = 1;
            }
            ++j;
        }
    }
}

__global__ __launch_bounds__(ROC_TPB) void roc_hist1_kernel(const float* __restrict__ D, const int32_t* __restrict__ qid,
                                                            const int32_t* __restrict__ gid, unsigned ng, unsigned N, u64* meta,
                                                            unsigned* __restrict__ bucket_cnt) {
    __shared__ unsigned h[ROC_NB1];
    __shared__ u64 sh[16];
    for (int b = threadIdx.x; b < ROC_NB1; b += ROC_TPB) h[b] = 0;
    __syncthreads();
    const unsigned ntiles = (N + ROC_TILE - 1) / ROC_TILE;
    unsigned npos = 0, bad = 0;
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
        RocTile T;
        roc_load_tile(D, qid, gid, ng, N, t, T);
        bad |= T.bad;
        npos += __popc(T.lab);
#pragma unroll
        for (int s = 0; s < ROC_EPT; ++s) roc_lds_add(h, T.key[s] >> 20, 1u, (T.valid >> s) & 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < ROC_NB1; b += ROC_TPB)
        if (h[b]) atomicAdd(&bucket_cnt[b], h[b]);
    u64 v[1] = {npos}, tot[1];
    roc_block_scan<1>(v, tot, sh);
    if (__syncthreads_or((int)bad) && threadIdx.x == 0) atomicOr(&meta[M_BAD], 1ull);
    if (threadIdx.x == 0 && tot[0]) atomicAdd(&meta[M_NPOS], tot[0]);
}

// one workgroup of 1024 threads; thread t owns the descending bucket positions 4t..4t+3 (bucket 4095 - p)
__global__ __launch_bounds__(1024) void roc_scan1_kernel(const unsigned* __restrict__ bucket_cnt, u64* meta, unsigned* __restrict__ cursor1,
                                                         int32_t* __restrict__ occ_bucket, unsigned* __restrict__ slot_base,
                                                         unsigned* __restrict__ task_prefix, unsigned N) {
    __shared__ u64 sh[16 * 3];
    unsigned c[4];
    u64 v[3] = {0, 0, 0}, tot[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k] = bucket_cnt[ROC_NB1 - 1 - (threadIdx.x * 4 + k)];
        v[0] += c[k] != 0;
        v[1] += c[k];
        v[2] += (c[k] + ROC_TILE - 1) / ROC_TILE;
    }
    roc_block_scan<3>(v, tot, sh);
    u64 slot = v[0], base = v[1], task = v[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = ROC_NB1 - 1 - (threadIdx.x * 4 + k);
        cursor1[b] = (unsigned)base;
        if (c[k]) {
            occ_bucket[slot] = b;
            slot_base[slot] = (unsigned)base;
            task_prefix[slot] = (unsigned)task;
            ++slot;
        }
        base += c[k];
        task += (c[k] + ROC_TILE - 1) / ROC_TILE;
    }
    if (threadIdx.x == 0) {
        slot_base[tot[0]] = N;
        task_prefix[tot[0]] = (unsigned)tot[2];
        meta[M_NOCC] = tot[0];
        meta[M_NTASK] = tot[2];
        meta[M_NNEG] = (u64)N - meta[M_NPOS];
    }
}

__global__ __launch_bounds__(ROC_TPB) void roc_part1_kernel(const float* __restrict__ D, const int32_t* __restrict__ qid,
                                                            const int32_t* __restrict__ gid, unsigned ng, unsigned N,
                                                            unsigned* __restrict__ cursor1, unsigned* __restrict__ s1) {
    __shared__ unsigned h[ROC_NB1];
    const unsigned ntiles = (N + ROC_TILE - 1) / ROC_TILE;
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (int b = threadIdx.x; b < ROC_NB1; b += ROC_TPB) h[b] = 0;
        __syncthreads();
        RocTile T;
        roc_load_tile(D, qid, gid, ng, N, t, T);
        unsigned rank[ROC_EPT];
#pragma unroll
        for (int s = 0; s < ROC_EPT; ++s) rank[s] = roc_lds_add(h, T.key[s] >> 20, 1u, (T.valid >> s) & 1u);
        __syncthreads();
        for (int b = threadIdx.x; b < ROC_NB1; b += ROC_TPB)
            if (h[b]) h[b] = atomicAdd(&cursor1[b], h[b]);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < ROC_EPT; ++s)
            if ((T.valid >> s) & 1u) s1[h[T.key[s] >> 20] + rank[s]] = ((T.key[s] & 0xfffffu) << 1) | ((T.lab >> s) & 1u);
        __syncthreads();
    }
}

// chunk task t of the slots [slot_lo, slot_hi): its slot and element range
__device__ __forceinline__ bool roc_task(unsigned t, const unsigned* __restrict__ task_prefix, const unsigned* __restrict__ slot_base,
                                         unsigned slot_lo, unsigned slot_hi, unsigned& slot, unsigned& e0, unsigned& e1) {
    unsigned lo = slot_lo, hi = slot_hi;                     // last slot with task_prefix[slot] <= t
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) / 2;
        if (task_prefix[mid] <= t) lo = mid; else hi = mid;
    }
    slot = lo;
    e0 = slot_base[slot] + (t - task_prefix[slot]) * (unsigned)ROC_TILE;
    e1 = min(e0 + (unsigned)ROC_TILE, slot_base[slot + 1]);
    return e0 < e1;
}

template <bool PART>
__global__ __launch_bounds__(ROC_TPB) void roc_mid_kernel(const u64* meta, const unsigned* __restrict__ task_prefix,
                                                          const unsigned* __restrict__ slot_base, unsigned* __restrict__ seg,
                                                          const unsigned* __restrict__ s1, unsigned* __restrict__ s2) {
    __shared__ unsigned h[ROC_NMID];
    const unsigned nocc = (unsigned)meta[M_NOCC], ntask = (unsigned)meta[M_NTASK];
    for (unsigned t = blockIdx.x; t < ntask; t += gridDim.x) {
        unsigned slot, e0, e1;
        const bool any = roc_task(t, task_prefix, slot_base, 0, nocc, slot, e0, e1);
        for (int b = threadIdx.x; b < ROC_NMID; b += ROC_TPB) h[b] = 0;
        __syncthreads();
        unsigned p[ROC_EPT], rank[ROC_EPT];
#pragma unroll
        for (int s = 0; s < ROC_EPT; ++s) {
            const unsigned e = e0 + s * ROC_TPB + threadIdx.x;
            const bool ok = any && e < e1;
            p[s] = ok ? s1[e] : 0u;
            rank[s] = roc_lds_add(h, p[s] >> 11, 1u, ok);
        }
        __syncthreads();
        for (int b = threadIdx.x; b < ROC_NMID; b += ROC_TPB)
            if (h[b]) {
                if (PART) h[b] = atomicAdd(&seg[(size_t)slot * ROC_NMID + b], h[b]);
                else atomicAdd(&seg[(size_t)slot * ROC_NMID + b], h[b]);
            }
        __syncthreads();
        if (PART) {
#pragma unroll
            for (int s = 0; s < ROC_EPT; ++s) {
                const unsigned e = e0 + s * ROC_TPB + threadIdx.x;
                if (any && e < e1) s2[h[p[s] >> 11] + rank[s]] = p[s];
            }
            __syncthreads();
        }
    }
}

// one workgroup (256 threads) per slot: segment sizes -> bases, descending mid
__global__ __launch_bounds__(256) void roc_scan2_kernel(const u64* meta, const unsigned* __restrict__ slot_base, unsigned* __restrict__ seg) {
    __shared__ u64 sh[16];
    const unsigned nocc = (unsigned)meta[M_NOCC];
    for (unsigned slot = blockIdx.x; slot < nocc; slot += gridDim.x) {
        unsigned* sg = seg + (size_t)slot * ROC_NMID;
        unsigned c[4];
        u64 v[1] = {0}, tot[1];
#pragma unroll
        for (int k = 0; k < 4; ++k) { c[k] = sg[ROC_NMID - 1 - (threadIdx.x * 4 + k)]; v[0] += c[k]; }
        roc_block_scan<1>(v, tot, sh);
        unsigned base = slot_base[slot] + (unsigned)v[0];
#pragma unroll
        for (int k = 0; k < 4; ++k) { sg[ROC_NMID - 1 - (threadIdx.x * 4 + k)] = base; base += c[k]; }
    }
}

__global__ void roc_zero_kernel(const u64* meta, int W, u64* __restrict__ cnt) {
    const u64 n = (u64)min((u64)W, meta[M_NOCC]) * ROC_KEYS;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) cnt[i] = 0;
}

// window w: chunks of the slots [w W, min((w + 1) W, nocc)) -> cnt[slot - w W][lo20] += pos << 32 | neg
__global__ __launch_bounds__(ROC_TPB) void roc_count_kernel(const u64* meta, const unsigned* __restrict__ task_prefix,
                                                            const unsigned* __restrict__ slot_base, const unsigned* __restrict__ s2,
                                                            int w, int W, u64* __restrict__ cnt) {
    __shared__ unsigned h[ROC_MSPAN * 1024];
    __shared__ int shm[16];
    const unsigned nocc = (unsigned)meta[M_NOCC];
    const unsigned slo = (unsigned)w * W;
    if (slo >= nocc) return;
    const unsigned shi = min(slo + (unsigned)W, nocc);
    const unsigned t0 = task_prefix[slo], t1 = task_prefix[shi];
    for (unsigned t = t0 + blockIdx.x; t < t1; t += gridDim.x) {
        unsigned slot, e0, e1;
        const bool any = roc_task(t, task_prefix, slot_base, slo, shi, slot, e0, e1);
        unsigned p[ROC_EPT], ok = 0;
        int top = -1;
#pragma unroll
        for (int s = 0; s < ROC_EPT; ++s) {
            const unsigned e = e0 + s * ROC_TPB + threadIdx.x;
            p[s] = 0;
            if (any && e < e1) { p[s] = s2[e]; ok |= 1u << s; top = max(top, (int)(p[s] >> 11)); }
        }
        top = roc_block_max(top, shm);
        u64* c = cnt + (size_t)(slot - slo) * ROC_KEYS;
        while (top >= 0) {
            for (int b = threadIdx.x; b < ROC_MSPAN * 1024; b += ROC_TPB) h[b] = 0;
            __syncthreads();
            int next = -1;
#pragma unroll
            for (int s = 0; s < ROC_EPT; ++s) {
                const int mid = (int)(p[s] >> 11);
                const bool in = ((ok >> s) & 1u) && mid <= top && mid > top - ROC_MSPAN;
                if (((ok >> s) & 1u) && mid <= top - ROC_MSPAN) next = max(next, mid);
                roc_lds_add(h, (unsigned)(top - mid) * 1024u + ((p[s] >> 1) & 1023u), (p[s] & 1u) ? 0x10000u : 1u, in);
            }
            next = roc_block_max(next, shm);                 // (barrier: the histogram is complete)
            for (int b = threadIdx.x; b < ROC_MSPAN * 1024; b += ROC_TPB) {
                const unsigned v = h[b];
                if (v) {
                    const unsigned key20 = ((unsigned)(top - b / 1024) << 10) | (unsigned)(b & 1023);
                    atomicAdd(&c[key20], ((u64)(v >> 16) << 32) | (u64)(v & 0xffffu));
                }
            }
            __syncthreads();
            top = next;
        }
    }
}

// compaction of window w: entry i of the window = (slot_local = i >> 20, lo20 = 0xfffff - (i & 0xfffff)), i.e. descending keys.
// A: non-empty entries per block of ROC_CMP_BLK; thread t reads the 16 entries [blk * 8192 + 16 t, +16)
__global__ __launch_bounds__(ROC_TPB) void roc_cmpA_kernel(const u64* meta, int w, int W, const u64* __restrict__ cnt,
                                                           unsigned* __restrict__ blk) {
    __shared__ u64 sh[16];
    const u64 nocc = meta[M_NOCC];
    if ((u64)w * W >= nocc) return;
    const unsigned ns = (unsigned)min((u64)W, nocc - (u64)w * W);
    const unsigned nblk = ns * (ROC_KEYS / ROC_CMP_BLK);
    for (unsigned bk = blockIdx.x; bk < nblk; bk += gridDim.x) {
        const size_t i0 = (size_t)bk * ROC_CMP_BLK + threadIdx.x * 16;
        const size_t sl = i0 >> 20, k0 = ROC_KEYS - 16 - (i0 & (ROC_KEYS - 1));    // entries lo20 = k0 + 15 .. k0
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(cnt + sl * ROC_KEYS + k0);
        u64 v[1] = {0}, tot[1];
#pragma unroll
        for (int q = 0; q < 8; ++q) { const ulonglong2 x = src[q]; v[0] += (x.x != 0) + (x.y != 0); }
        roc_block_scan<1>(v, tot, sh);
        if (threadIdx.x == 0) blk[bk] = (unsigned)tot[0];
    }
}

// B: one workgroup of 1024 threads: exclusive scan of the block counts, offset by the records so far
__global__ __launch_bounds__(1024) void roc_cmpB_kernel(u64* meta, int w, int W, unsigned* __restrict__ blk) {
    __shared__ u64 sh[16];
    const u64 nocc = meta[M_NOCC];
    if ((u64)w * W >= nocc) return;
    const unsigned nblk = (unsigned)min((u64)W, nocc - (u64)w * W) * (ROC_KEYS / ROC_CMP_BLK);
    const unsigned per = (nblk + 1023) / 1024;
    const unsigned b0 = min(threadIdx.x * per, nblk), b1 = min(b0 + per, nblk);
    u64 v[1] = {0}, tot[1];
    for (unsigned b = b0; b < b1; ++b) v[0] += blk[b];
    roc_block_scan<1>(v, tot, sh);
    u64 base = meta[M_NREC] + v[0];
    for (unsigned b = b0; b < b1; ++b) { const unsigned c = blk[b]; blk[b] = (unsigned)base; base += c; }
    __syncthreads();
    if (threadIdx.x == 0) meta[M_NREC] += tot[0];
}

// C: write the records (key -> s2 in place, pos -> s1, neg -> s3) and clear the counters
__global__ __launch_bounds__(ROC_TPB) void roc_cmpC_kernel(const u64* meta, int w, int W, u64* __restrict__ cnt,
                                                           const unsigned* __restrict__ blk, const int32_t* __restrict__ occ_bucket,
                                                           unsigned* __restrict__ rkey, unsigned* __restrict__ rpos,
                                                           unsigned* __restrict__ rneg) {
    __shared__ u64 sh[16];
    const u64 nocc = meta[M_NOCC];
    if ((u64)w * W >= nocc) return;
    const unsigned ns = (unsigned)min((u64)W, nocc - (u64)w * W);
    const unsigned nblk = ns * (ROC_KEYS / ROC_CMP_BLK);
    for (unsigned bk = blockIdx.x; bk < nblk; bk += gridDim.x) {
        const size_t i0 = (size_t)bk * ROC_CMP_BLK + threadIdx.x * 16;
        const size_t sl = i0 >> 20, k0 = ROC_KEYS - 16 - (i0 & (ROC_KEYS - 1));
        ulonglong2* src = reinterpret_cast<ulonglong2*>(cnt + sl * ROC_KEYS + k0);
        u64 x[16];
        u64 v[1] = {0}, tot[1];
        (void)tot;
#pragma unroll
        for (int q = 0; q < 8; ++q) { const ulonglong2 y = src[q]; x[2 * q] = y.x; x[2 * q + 1] = y.y; v[0] += (y.x != 0) + (y.y != 0); }
        roc_block_scan<1>(v, tot, sh);
        unsigned pos = blk[bk] + (unsigned)v[0];
        const unsigned hi = (unsigned)occ_bucket[(unsigned)w * W + (unsigned)sl] << 20;
#pragma unroll
        for (int r = 15; r >= 0; --r) {                      // descending lo20: entry k0 + r first
            if (x[r]) {
                rkey[pos] = hi | (unsigned)(k0 + r);
                rpos[pos] = (unsigned)(x[r] >> 32);
                rneg[pos] = (unsigned)x[r];
                ++pos;
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (x[2 * q] | x[2 * q + 1]) src[q] = make_ulonglong2(0ull, 0ull);
    }
}

__device__ __forceinline__ bool roc_kept(const unsigned* __restrict__ rpos, const unsigned* __restrict__ rneg, u64 i, u64 R, bool drop) {
    if (!drop || R <= 2 || i == 0 || i + 1 == R) return true;
    return rpos[i + 1] != rpos[i] || rneg[i + 1] != rneg[i];
}

// A: per range g of the records: sums of pos, neg and kept points
__global__ __launch_bounds__(256) void roc_curveA_kernel(const u64* meta, const unsigned* __restrict__ rpos, const unsigned* __restrict__ rneg,
                                                         u64* __restrict__ part) {
    __shared__ u64 sh[16 * 3];
    const u64 R = meta[M_NREC];
    const u64 a = R * blockIdx.x / ROC_CURVE_G, b = R * (blockIdx.x + 1) / ROC_CURVE_G;
    u64 v[3] = {0, 0, 0}, tot[3];
    for (u64 i = a + threadIdx.x; i < b; i += blockDim.x) {
        v[0] += rpos[i];
        v[1] += rneg[i];
        v[2] += roc_kept(rpos, rneg, i, R, true);
    }
    roc_block_scan<3>(v, tot, sh);
    if (threadIdx.x == 0) { part[blockIdx.x * 4 + 0] = tot[0]; part[blockIdx.x * 4 + 1] = tot[1]; part[blockIdx.x * 4 + 2] = tot[2]; }
}

// B: one workgroup of ROC_CURVE_G threads: exclusive offsets of the ranges; the caller's int64 out[5]
__global__ __launch_bounds__(ROC_CURVE_G) void roc_curveB_kernel(u64* meta, u64* __restrict__ part, int64_t* __restrict__ out) {
    __shared__ u64 sh[16 * 3];
    u64 v[3] = {part[threadIdx.x * 4 + 0], part[threadIdx.x * 4 + 1], part[threadIdx.x * 4 + 2]}, tot[3];
    roc_block_scan<3>(v, tot, sh);
    part[threadIdx.x * 4 + 0] = v[0];
    part[threadIdx.x * 4 + 1] = v[1];
    part[threadIdx.x * 4 + 2] = v[2];
    if (threadIdx.x == 0) {
        meta[M_NKEPT] = tot[2];
        out[0] = (int64_t)tot[2];
        out[1] = (int64_t)meta[M_NREC];
        out[2] = (int64_t)tot[0];
        out[3] = (int64_t)tot[1];
        out[4] = meta[M_BAD] ? 1 : ((tot[0] + tot[1] != meta[M_NPOS] + meta[M_NNEG] || tot[0] != meta[M_NPOS]) ? 2 : 0);
    }
}

// dali_roc_emit: range g in chunks of 256 x 4 consecutive records
__global__ __launch_bounds__(256) void roc_emit_kernel(const u64* meta, const unsigned* __restrict__ rkey, const unsigned* __restrict__ rpos,
                                                       const unsigned* __restrict__ rneg, const u64* __restrict__ part, int drop,
                                                       long long cap, float* __restrict__ thr, int64_t* __restrict__ fps,
                                                       int64_t* __restrict__ tps) {
    __shared__ u64 sh[16 * 3];
    const u64 R = meta[M_NREC];
    const u64 a = R * blockIdx.x / ROC_CURVE_G, b = R * (blockIdx.x + 1) / ROC_CURVE_G;
    u64 cp = part[blockIdx.x * 4 + 0], cn = part[blockIdx.x * 4 + 1], ck = drop ? part[blockIdx.x * 4 + 2] : a;
    for (u64 c0 = a; c0 < b; c0 += 256 * 4) {
        const u64 i0 = c0 + threadIdx.x * 4;
        unsigned pp[4], nn[4], kk[4];
        u64 v[3] = {0, 0, 0}, tot[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = i0 + k < b;
            pp[k] = in ? rpos[i0 + k] : 0u;
            nn[k] = in ? rneg[i0 + k] : 0u;
            kk[k] = in ? (unsigned)roc_kept(rpos, rneg, i0 + k, R, drop != 0) : 0u;
            v[0] += pp[k]; v[1] += nn[k]; v[2] += kk[k];
        }
        roc_block_scan<3>(v, tot, sh);
        u64 tp = cp + v[0], fp = cn + v[1], o = ck + v[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tp += pp[k]; fp += nn[k];
            if (kk[k]) {
                if ((long long)o < cap) {
                    thr[o] = roc_score(rkey[i0 + k]);
                    fps[o] = (int64_t)fp;
                    tps[o] = (int64_t)tp;
                }
                ++o;
            }
        }
        cp += tot[0]; cn += tot[1]; ck += tot[2];
    }
}

int roc_check(long long nq, long long ng) {
    if (nq < 1 || ng < 1) { dali::set_error("dali_roc: nq = %lld, ng = %lld (need >= 1)", nq, ng); return DALI_ERR_INVALID; }
    if (nq * ng > 2147483647ll) {
        dali::set_error("dali_roc: nq * ng = %lld exceeds the supported 2^31 - 1 pairs", nq * ng);
        return DALI_ERR_LIMIT;
    }
    return DALI_OK;
}

}  // namespace

extern "C" size_t dali_roc_scratch_bytes(int nq, int ng) {
    if (roc_check(nq, ng) != DALI_OK) return 0;
    return roc_layout((long long)nq * ng).total;
}

extern "C" int dali_roc_build(dali_ctx* ctx, void* stream, const float* distmat, const int32_t* q_ids, const int32_t* g_ids, int nq, int ng,
                              void* scratch, size_t scratch_bytes, int64_t* out) {
    const int st = roc_check(nq, ng);
    if (st != DALI_OK) return st;
    DALI_REQUIRE(ctx && distmat && q_ids && g_ids && scratch && out, "dali_roc_build: null argument");
    DALI_REQUIRE(((uintptr_t)distmat & 15) == 0, "dali_roc_build: distmat must be 16-byte aligned");
    DALI_REQUIRE(((uintptr_t)scratch & 255) == 0, "dali_roc_build: scratch must be 256-byte aligned");
    const unsigned N = (unsigned)((long long)nq * ng);
    const Layout L = roc_layout(N);
    DALI_REQUIRE(scratch_bytes >= L.total, "dali_roc_build: scratch holds %zu bytes, needs %zu (dali_roc_scratch_bytes)", scratch_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    u64* meta = (u64*)(base + L.meta);
    unsigned* bucket_cnt = (unsigned*)(base + L.bucket_cnt);
    unsigned* cursor1 = (unsigned*)(base + L.cursor1);
    int32_t* occ_bucket = (int32_t*)(base + L.occ_bucket);
    unsigned* slot_base = (unsigned*)(base + L.slot_base);
    unsigned* task_prefix = (unsigned*)(base + L.task_prefix);
    unsigned* seg = (unsigned*)(base + L.seg);
    unsigned* blk = (unsigned*)(base + L.blk);
    u64* part = (u64*)(base + L.part);
    unsigned *s1 = (unsigned*)(base + L.s1), *s2 = (unsigned*)(base + L.s2), *s3 = (unsigned*)(base + L.s3);
    u64* cnt = (u64*)(base + L.cnt);

    DALI_HIP(hipMemsetAsync(base, 0, L.seg + (size_t)ROC_NB1 * ROC_NMID * 4, s));    // meta .. seg
    const unsigned ntiles = (N + ROC_TILE - 1) / ROC_TILE;
    const int g1 = (int)std::min<unsigned>(ntiles, ROC_GRID);
    roc_hist1_kernel<<<g1, ROC_TPB, 0, s>>>(distmat, q_ids, g_ids, (unsigned)ng, N, meta, bucket_cnt);
    DALI_LAUNCH_CHECK();
    roc_scan1_kernel<<<1, 1024, 0, s>>>(bucket_cnt, meta, cursor1, occ_bucket, slot_base, task_prefix, N);
    DALI_LAUNCH_CHECK();
    roc_part1_kernel<<<g1, ROC_TPB, 0, s>>>(distmat, q_ids, g_ids, (unsigned)ng, N, cursor1, s1);
    DALI_LAUNCH_CHECK();
    const int gt = (int)std::min<unsigned>(ntiles + std::min<unsigned>(N, ROC_NB1), ROC_GRID);   // chunk tasks <= tiles + slots
    roc_mid_kernel<false><<<gt, ROC_TPB, 0, s>>>(meta, task_prefix, slot_base, seg, s1, s2);
    DALI_LAUNCH_CHECK();
    roc_scan2_kernel<<<(int)std::min<unsigned>(N, ROC_GRID), 256, 0, s>>>(meta, slot_base, seg);
    DALI_LAUNCH_CHECK();
    roc_mid_kernel<true><<<gt, ROC_TPB, 0, s>>>(meta, task_prefix, slot_base, seg, s1, s2);
    DALI_LAUNCH_CHECK();
    roc_zero_kernel<<<ROC_GRID, 256, 0, s>>>(meta, L.W, cnt);
    DALI_LAUNCH_CHECK();
    const int nwin = (int)((std::min<unsigned>(N, ROC_NB1) + L.W - 1) / L.W);
    const int gc = (int)std::min<long long>((long long)L.W * (ROC_KEYS / ROC_CMP_BLK), ROC_GRID);
    for (int w = 0; w < nwin; ++w) {
        roc_count_kernel<<<gt, ROC_TPB, 0, s>>>(meta, task_prefix, slot_base, s2, w, L.W, cnt);
        DALI_LAUNCH_CHECK();
        roc_cmpA_kernel<<<gc, ROC_TPB, 0, s>>>(meta, w, L.W, cnt, blk);
        DALI_LAUNCH_CHECK();
        roc_cmpB_kernel<<<1, 1024, 0, s>>>(meta, w, L.W, blk);
        DALI_LAUNCH_CHECK();
        roc_cmpC_kernel<<<gc, ROC_TPB, 0, s>>>(meta, w, L.W, cnt, blk, occ_bucket, s2, s1, s3);
        DALI_LAUNCH_CHECK();
    }
    roc_curveA_kernel<<<ROC_CURVE_G, 256, 0, s>>>(meta, s1, s3, part);
    DALI_LAUNCH_CHECK();
    roc_curveB_kernel<<<1, ROC_CURVE_G, 0, s>>>(meta, part, out);
    DALI_LAUNCH_CHECK();
    (void)ctx;
    return DALI_OK;
}

extern "C" int dali_roc_emit(dali_ctx* ctx, void* stream, const void* scratch, int nq, int ng, int drop_intermediate, int64_t n_points,
                             float* thresholds, int64_t* fps, int64_t* tps) {
    const int st = roc_check(nq, ng);
    if (st != DALI_OK) return st;
    DALI_REQUIRE(ctx && scratch, "dali_roc_emit: null argument");
    DALI_REQUIRE(n_points >= 0, "dali_roc_emit: n_points < 0");
    if (n_points == 0) return DALI_OK;
    DALI_REQUIRE(thresholds && fps && tps, "dali_roc_emit: null output");
    const Layout L = roc_layout((long long)nq * ng);
    const char* base = (const char*)scratch;
    roc_emit_kernel<<<ROC_CURVE_G, 256, 0, (hipStream_t)stream>>>((const u64*)(base + L.meta), (const unsigned*)(base + L.s2),
                                                                 (const unsigned*)(base + L.s1), (const unsigned*)(base + L.s3),
                                                                 (const u64*)(base + L.part), drop_intermediate ? 1 : 0, (long long)n_points,
                                                                 thresholds, fps, tps);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

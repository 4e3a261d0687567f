// block_prims.h -- the block- and wave-level pieces that the evaluation kernels share (rank.hip, topk.hip + topk_key.h, rerank.hip,
// roc.hip): the order-preserving image of a float, the bitonic sort of 64-bit keys in LDS, the 256-thread inclusive scan, the one-block
// "counts -> exclusive offsets" pass of the counting sorts, and the 64-bit wave shuffles.  Device-only; each exists here once.
#pragma once
#include "common.h"

namespace dali {

// IEEE bits made monotonic: negative values flipped, the sign bit set on the others; -0.0 is folded onto +0.0 first, so that equal
// values get equal bits (and a key built on them compares by its index).  No NaN policy: a NaN's bits are mapped like any other
// (positive NaN above +inf, negative NaN below -inf); a caller that can meet one states what it does with it.
__device__ __forceinline__ unsigned int ordered_bits(float v) {
    unsigned int b = __float_as_uint(v + 0.0f);
    b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
    return b;
}
__device__ __forceinline__ float ordered_bits_inv(unsigned int b) {
    return __uint_as_float((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b);
}

// ascending bitonic sort of s_key[0 .. npad), npad a power of two, by a 256-thread block.  Keys are unique except for the sentinel,
// so the sorted sequence does not depend on the order the keys arrived in.
__device__ __forceinline__ void block_sort_keys(unsigned long long* s_key, int npad, int tid) {
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < npad; t += 256) {
                const int p = t ^ j;
                if (p > t) {
                    const bool up = (t & k) == 0;
                    const unsigned long long ka = s_key[t], kb = s_key[p];
                    if (up ? kb < ka : ka < kb) { s_key[t] = kb; s_key[p] = ka; }
                }
            }
            __syncthreads();
        }
    }
}
// pads s_key[n ..) with the sentinel ~0ull (above every real key) up to the next power of two >= max(n, at_least) and sorts.  All
// threads pass the same n.  One barrier separates the pad from the sort: what a caller writes to LDS just before the call is visible after it.
__device__ __forceinline__ void block_pad_sort(unsigned long long* s_key, int n, int at_least, int tid) {
    int npad = 1;
    while (npad < n || npad < at_least) npad <<= 1;
    for (int t = n + tid; t < npad; t += 256) s_key[t] = ~0ull;
    __syncthreads();
    block_sort_keys(s_key, npad, tid);
}

// inclusive scan of one int per thread over a 256-thread block (Hillis-Steele through s_scan[256]); returns the thread's prefix, and
// s_scan[255] is the block total.  Ends on a barrier after the last write; the caller puts one before it reuses s_scan.
__device__ __forceinline__ int block_scan_incl_256(int* s_scan, int v, int tid) {
    s_scan[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int add = (tid >= o) ? s_scan[tid - o] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    return s_scan[tid];
}

// body of a one-block, 1024-thread kernel: off[c] = exclusive prefix of cnt over n entries (off[n] = total), cursor[0 .. n) zeroed.
// The middle pass of a counting sort (count, this, scatter by atomic cursor).
__device__ __forceinline__ void block_counts_to_offsets_1024(const int32_t* __restrict__ cnt, int n, int32_t* __restrict__ off,
                                                             int32_t* __restrict__ cursor) {
    __shared__ int s_part[1024];
    const int tid = threadIdx.x, per = (n + 1023) / 1024, b = min(tid * per, n), e = min(b + per, n);
    int sum = 0;
    for (int c = b; c < e; ++c) sum += cnt[c];
    s_part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int add = tid >= o ? s_part[tid - o] : 0;
        __syncthreads();
        s_part[tid] += add;
        __syncthreads();
    }
    int run = s_part[tid] - sum;
    for (int c = b; c < e; ++c) { off[c] = run; cursor[c] = 0; run += cnt[c]; }
    if (tid == 1023) off[n] = s_part[1023];
}

// 64-bit values through the 32-bit wave shuffles
__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int d) {
    const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)(v >> 32), d, 64);
    return ((unsigned long long)hi << 32) | lo;
}

}  // namespace dali

// topk_key.h -- the selection order of include/daliid.h (dali_topk_rows) as one unsigned 64-bit key, shared by the row selection
// (topk.hip) and the selecting epilogue of the distance kernel (eval.hip):
//   key = (ordered value bits << 32) | global column index;  smaller key = better entry.
// Ordered value bits: ordered_bits (block_prims.h: monotone, -0.0 folded onto +0.0, so that equal values compare by index), complemented
// for `largest`.  NaN policy of this key, stated here once: a NaN of either sign is 0xffffffff in both directions, i.e. after +inf (-inf
// for largest), where numpy and torch sort it.  No other value maps to 0xffffffff, and indices stay below 2^31, so the all-ones
// key is free: it marks an unfilled slot and sorts after every entry.
#pragma once
#include "block_prims.h"

namespace dali {

constexpr int TOPK_K_MAX = 128;
constexpr unsigned long long TOPK_SENTINEL = ~0ull;

__device__ __forceinline__ unsigned int topk_ordered_bits(float v, int largest) {
    if (v != v) return 0xffffffffu;
    const unsigned int b = ordered_bits(v);
    return largest ? ~b : b;
}
__device__ __forceinline__ unsigned long long topk_key(float v, int index, int largest) {
    return ((unsigned long long)topk_ordered_bits(v, largest) << 32) | (unsigned int)index;
}
// -> value (the canonical quiet NaN for a NaN; +inf / -inf for an unfilled slot) and index (-1 for an unfilled slot)
__device__ __forceinline__ void topk_key_decode(unsigned long long key, int largest, float& v, int& index) {
    const unsigned int hi = (unsigned int)(key >> 32);
    index = (int)(unsigned int)key;
    if (hi == 0xffffffffu) {
        v = (key == TOPK_SENTINEL) ? __uint_as_float(largest ? 0xff800000u : 0x7f800000u) : __uint_as_float(0x7fc00000u);
        return;
    }
    v = ordered_bits_inv(largest ? ~hi : hi);
}

// Selecting epilogue of pairdist_dma_kernel: instead of storing its tile, a consumer lane compares every distance with its query's
// threshold -- the k-th key of the running list, read-only during the launch, so the set of survivors does not depend on timing -- and
// appends the survivors' keys to the query's candidate list.  cnt is the only atomic: it hands out slots, and the merge sorts the list.
struct PairTopk {
    const unsigned long long* keys;   // [nq][k] running lists, ascending
    unsigned long long* cand;         // [nq][cap]
    int* cnt;                         // [nq] survivors of this launch (may exceed cap: then flag[0] = 1 and the launch is redone through the matrix)
    int* flag;
    int k, cap, g_offset, largest;
};
// Matrix epilogue of a launch that only runs when gate[0] != 0 (the overflow fallback: enqueued unconditionally, decided on the device)
struct PairGate {
    const int* gate;
};

}  // namespace dali

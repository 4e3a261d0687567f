// rank.hip -- the market1501 CMC/mAP arithmetic of torchreid.metrics.evaluate_rank (validateModels.py:68) on a distance matrix, without a
//   full row sort: dali_rank_eval on one GPU, dali_rank_shard_matches / _bins / _finish with the gallery sharded over ranks.  The stages
//   the two paths share (identity slice, lower bound among the sorted match keys, bins -> AP) are one function each, below.
//   dali_rank_eval_inp: mINP (mean inverse negative penalty) from the same query kernels on one GPU; the sharded path is out of its scope.
#include "block_prims.h"

namespace dali {

// ------------------------------------------------------------------------------------------------
// market1501 ranking without a row sort.  One 256-thread block per query.
//   kept(g)  = !(g_pid == q_pid && g_cam == q_cam)                  (junk removal)
//   match(g) = kept(g) && g_pid == q_pid
// The gallery is indexed by identity ONCE per evaluation (rank_index_*: counting sort of the gallery positions by pid, on
// the device), so a query finds its same-identity entries -- matches and junk -- as one slice of that index instead of
// scanning all ng ids (10k x 100k: 4 GB of id reads gone; only the distance row is read, 4 bytes per pair).
// Sort the matches by key (dist, index) in LDS (bitonic).  Every kept gallery entry is binned by the
// number of matches with a smaller key (binary search); with c[b] the bin counts,
//   position (1-based, among kept) of the j-th match = c[0] + ... + c[j]
//   AP = mean_j (j+1) / position_j ,  first-hit rank = c[0] - 1.
// LDS is sized in two tiers (the row scan is HBM-bound and needs many workgroups per CU in flight): RANK_PSMALL same-identity
// entries per query in the first launch (16 KiB of LDS: 8+ workgroups per CU); queries with more are flagged and redone by a
// second launch with room for RANK_PMAX; beyond that DALI_ERR_LIMIT through status[0].
// ------------------------------------------------------------------------------------------------
constexpr int RANK_PSMALL = 512, RANK_PMAX = 4096, RANK_BINS = 1024;
constexpr int RANK_MAX_PID_RANGE = 1 << 20;      // identity codes must span at most this range (the mirrors pass dense codes): status 2 otherwise

// (dist, index) as one unsigned 64-bit key ordered like (dist, index): ordered_bits of the distance (equal distances compare by index), then
// the gallery index.  NaN: no policy, the distances are taken as numbers (a NaN sorts by its bits: positive last, negative first).
__device__ __forceinline__ unsigned long long rank_key(float d, int g) {
    return ((unsigned long long)ordered_bits(d) << 32) | (unsigned int)g;
}

// The query's identity slice [sb, se) of the gallery index (empty when the gallery lacks the identity); false, and an empty slice, when
// the identity codes span more than RANK_MAX_PID_RANGE (the index was not built: status 2 set by rank_index_count_kernel).
__device__ __forceinline__ bool rank_identity_slice(const int32_t* __restrict__ info, const int32_t* __restrict__ starts, int qp, int& sb, int& se) {
    const int lo = info[0], hi = info[1];
    sb = se = 0;
    if ((long long)hi - lo + 1 > RANK_MAX_PID_RANGE) return false;
    if (qp >= lo && qp <= hi) { sb = starts[qp - lo]; se = starts[qp - lo + 1]; }
    return true;
}

// p + (number of keys below k among the sorted s_key[p .. p + len))
__device__ __forceinline__ int rank_lower_bound(const unsigned long long* s_key, int p, int len, unsigned long long k) {
    while (len > 0) {
        const int half = len >> 1;
        if (s_key[p + half] < k) { p += half + 1; len -= half + 1; } else len = half;
    }
    return p;
}

// Bins -> AP and first-hit rank of one query, by its 256-thread block: load_bin(j), j < np, is the number of kept entries that have j
// matches with a smaller key, so the (1-based) position of the j-th match is the inclusive prefix sum; taken in sequential chunks of 256
// with a carry.  The float arithmetic and its order -- per-thread partial sums over the chunks, wave_sum, four wave partials added in
// order, one division by np -- exist only here: whatever bins the whole-gallery and the sharded path agree on give the same bits.
// last / n_rel (nullable; compile-time null for CMC / mAP): the 0-based position of the LAST match, where the scan ends, and np.
template <class LoadBin>
__device__ __forceinline__ void rank_ap_tail(LoadBin load_bin, int np, int* s_scan, float* s_red, int tid, float* __restrict__ ap,
                                             int32_t* __restrict__ first, int32_t* __restrict__ last = nullptr,
                                             int32_t* __restrict__ n_rel = nullptr) {
    float ap_part = 0.f;
    int carry = 0;
    for (int base = 0; base < np; base += 256) {
        const int t = base + tid;
        const int pos = carry + block_scan_incl_256(s_scan, (t < np) ? load_bin(t) : 0, tid);
        if (t < np) ap_part += (float)(t + 1) / (float)pos;
        if (t == 0) *first = pos - 1;
        if (last && t == np - 1) *last = pos - 1;
        carry += s_scan[255];
        __syncthreads();
    }
    ap_part = wave_sum(ap_part);
    if ((tid & 63) == 0) s_red[tid >> 6] = ap_part;
    __syncthreads();
    if (tid == 0) *ap = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (float)np;
    if (n_rel && tid == 0) *n_rel = np;
}

// ---- gallery index by identity: info = {min pid, max pid}; counts/starts over [min, max]; order = gallery positions grouped by pid ----
__global__ __launch_bounds__(256) void rank_index_minmax_kernel(const int32_t* __restrict__ g_pids, int ng, int32_t* __restrict__ info) {
    int lo = 0x7fffffff, hi = (int)0x80000000;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < ng; g += gridDim.x * 256) { const int p = g_pids[g]; lo = min(lo, p); hi = max(hi, p); }
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { atomicMin(&info[0], lo); atomicMax(&info[1], hi); }
}
__global__ __launch_bounds__(256) void rank_index_count_kernel(const int32_t* __restrict__ g_pids, int ng, const int32_t* __restrict__ info,
                                                                int32_t* __restrict__ counts, int32_t* __restrict__ status) {
    const int lo = info[0];
    const long long range = (long long)info[1] - lo + 1;
    if (range > RANK_MAX_PID_RANGE) { if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(status, 2); return; }
    for (int g = blockIdx.x * 256 + threadIdx.x; g < ng; g += gridDim.x * 256) atomicAdd(&counts[g_pids[g] - lo], 1);
}
// one block: starts[r] = exclusive prefix of counts (range + 1 entries), cursors zeroed
__global__ __launch_bounds__(1024) void rank_index_scan_kernel(const int32_t* __restrict__ info, const int32_t* __restrict__ counts,
                                                               int32_t* __restrict__ starts, int32_t* __restrict__ cursor) {
    const long long range = (long long)info[1] - info[0] + 1;
    if (range > RANK_MAX_PID_RANGE) return;
    block_counts_to_offsets_1024(counts, (int)range, starts, cursor);
}
__global__ __launch_bounds__(256) void rank_index_scatter_kernel(const int32_t* __restrict__ g_pids, int ng, const int32_t* __restrict__ info,
                                                                  const int32_t* __restrict__ starts, int32_t* __restrict__ cursor,
                                                                  int32_t* __restrict__ order) {
    const int lo = info[0];
    if ((long long)info[1] - lo + 1 > RANK_MAX_PID_RANGE) return;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < ng; g += gridDim.x * 256) {
        const int r = g_pids[g] - lo;
        order[starts[r] + atomicAdd(&cursor[r], 1)] = g;          // order inside an identity is irrelevant: matches are sorted by key below
    }
}

// PASS 0: every query, LDS for PCAP = RANK_PSMALL; larger identities set pending[q].  PASS 1: only the pending queries, PCAP = RANK_PMAX.
// INP (dali_rank_eval_inp): also last_rank[q] / n_rel[q], the position of the query's last match and its number of matches (-1 / 0 for an
// invalid query); without it the two pointers are never read and the kernel is what it was.
template <int PCAP, int PASS, bool INP>
__global__ __launch_bounds__(256) void rank_query_kernel(const float* __restrict__ distmat, const int32_t* __restrict__ q_pids,
                                                          const int32_t* __restrict__ q_cams, const int32_t* __restrict__ g_cams,
                                                          const int32_t* __restrict__ info, const int32_t* __restrict__ starts,
                                                          const int32_t* __restrict__ order, int nq, int ng,
                                                          float* __restrict__ ap_out, int32_t* __restrict__ first_rank,
                                                          int32_t* __restrict__ pending, int32_t* __restrict__ status,
                                                          int32_t* __restrict__ last_rank, int32_t* __restrict__ n_rel) {
    __shared__ unsigned long long s_key[PCAP];    // (orderable distance bits << 32) | gallery index: one 8-byte LDS read per compare
    __shared__ unsigned s_cell[RANK_BINS];
    __shared__ int s_cnt[PCAP + 1];
    __shared__ int s_junk[PCAP];
    __shared__ int s_n, s_nj;
    __shared__ float s_red[4];
    __shared__ int s_scan[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    if (PASS == 1 && pending[q] == 0) return;
    const float* drow = distmat + (size_t)q * ng;
    const int qp = q_pids[q], qc = q_cams[q];
    // 1. this query's identity slice of the gallery index: matches (other camera) and junk (same camera)
    int sb, se;
    auto invalid = [&]() { ap_out[q] = 0.f; first_rank[q] = -1; if constexpr (INP) { last_rank[q] = -1; n_rel[q] = 0; } };
    if (!rank_identity_slice(info, starts, qp, sb, se)) { if (tid == 0) invalid(); return; }
    const int nsame = se - sb;
    if (nsame == 0) {
        if (tid == 0) { invalid(); if (PASS == 0) pending[q] = 0; }
        return;
    }
    if (nsame > PCAP) {
        if (tid == 0) {
            invalid();
            if (PASS == 0) pending[q] = 1; else atomicMax(status, 1);
        }
        return;
    }
    if (tid == 0) { s_n = 0; s_nj = 0; if (PASS == 0) pending[q] = 0; }
    __syncthreads();
    for (int t = tid; t < nsame; t += 256) {
        const int g = order[sb + t];
        if (g_cams[g] != qc) s_key[atomicAdd(&s_n, 1)] = rank_key(drow[g], g);
        else s_junk[atomicAdd(&s_nj, 1)] = g;
    }
    __syncthreads();
    const int np = s_n, nj = s_nj;
    if (np == 0) {
        if (tid == 0) invalid();
        return;
    }
    const bool vec = (ng & 3) == 0 && (reinterpret_cast<uintptr_t>(drow) & 15) == 0;
    // 2. bitonic sort of (dist, idx); the bins are zeroed behind the sort's own barrier between its pad and its passes
    for (int t = tid; t <= np; t += 256) s_cnt[t] = 0;
    block_pad_sort(s_key, np, 0, tid);
    // 3. bin EVERY gallery entry by the number of matches with a smaller key (only the distance row is read: 4 bytes per pair, coalesced
    //    16 B per lane), then take the junk entries back out of their bins.
    //    The lower bound over the sorted matches is NOT searched per entry (7 dependent LDS reads per entry at ~100 matches left the pass
    //    LDS-bound on random distances: 1.7 ms for 10k x 100k against 0.8 ms of HBM time).  The distance axis between the first and the
    //    last match is cut into RANK_BINS uniform cells; s_cell[c] = (matches in lower cells) | (matches in cell c) << 16.  An entry reads
    //    its cell's word: that IS its lower bound unless the cell holds matches itself (about one cell in ten), where a short search
    //    inside the cell's matches finishes it.  floor((d - lo) * scale) is monotone in d, so cells never reorder keys.
    const unsigned long long last_key = s_key[np - 1];
    auto key_dist = [](unsigned long long k) { return ordered_bits_inv((unsigned)(k >> 32)); };
    const float dlo = key_dist(s_key[0]), dhi = key_dist(last_key);
    const float cscale = dhi > dlo ? (float)RANK_BINS / (dhi - dlo) : 0.f;
    auto cell_of = [&](float dn) { const unsigned c = (unsigned)(int)((dn - dlo) * cscale); return (int)(c < (unsigned)RANK_BINS ? c : RANK_BINS - 1); };   // (always in bounds)
    for (int t = tid; t < RANK_BINS; t += 256) s_cell[t] = 0;
    __syncthreads();
    for (int t = tid; t < np; t += 256) atomicAdd(&s_cell[cell_of(key_dist(s_key[t]))], 1u << 16);
    __syncthreads();
    {   // exclusive scan of the per-cell match counts into the low halves (RANK_BINS = 4 * 256: four cells per thread)
        unsigned c4[4], run = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) { c4[u] = s_cell[tid * 4 + u] >> 16; run += c4[u]; }
        unsigned base = (unsigned)block_scan_incl_256(s_scan, (int)run, tid) - run;
#pragma unroll
        for (int u = 0; u < 4; ++u) { s_cell[tid * 4 + u] = base | (c4[u] << 16); base += c4[u]; }
        __syncthreads();
    }
    auto lower_bound_in = [&](unsigned long long k, float dn) {          // number of matches with a key below k, for dlo <= dn and k <= last_key
        const unsigned cw = s_cell[cell_of(dn)];
        return rank_lower_bound(s_key, (int)(cw & 0xffffu), (int)(cw >> 16), k);      // only cells that hold matches: a search among THEIR keys
    };
    auto bin = [&](float d, int g, int delta) {
        const float dn = d + 0.0f;
        const unsigned long long k = rank_key(d, g);
        if (k > last_key) return;                                       // beyond the last match: affects no position
        atomicAdd(&s_cnt[dn < dlo ? 0 : lower_bound_in(k, dn)], delta);
    };
    auto bin4 = [&](const float4 v, int g, int delta) { bin(v.x, g, delta); bin(v.y, g + 1, delta); bin(v.z, g + 2, delta); bin(v.w, g + 3, delta); };
    if (vec) {
        int g = tid * 4;
        for (; g + 3072 < ng; g += 4096) {                            // 4 independent 16-byte loads in flight
            const float4 v0 = *reinterpret_cast<const float4*>(drow + g);
            const float4 v1 = *reinterpret_cast<const float4*>(drow + g + 1024);
            const float4 v2 = *reinterpret_cast<const float4*>(drow + g + 2048);
            const float4 v3 = *reinterpret_cast<const float4*>(drow + g + 3072);
            bin4(v0, g, 1); bin4(v1, g + 1024, 1); bin4(v2, g + 2048, 1); bin4(v3, g + 3072, 1);
        }
        for (; g < ng; g += 1024) bin4(*reinterpret_cast<const float4*>(drow + g), g, 1);
    } else {
        for (int g = tid; g < ng; g += 256) bin(drow[g], g, 1);
    }
    __syncthreads();
    for (int t = tid; t < nj; t += 256) bin(drow[s_junk[t]], s_junk[t], -1);
    __syncthreads();
    // 4. inclusive scan of the bins + AP
    if constexpr (INP) rank_ap_tail([&](int t) { return s_cnt[t]; }, np, s_scan, s_red, tid, &ap_out[q], &first_rank[q], &last_rank[q], &n_rel[q]);
    else rank_ap_tail([&](int t) { return s_cnt[t]; }, np, s_scan, s_red, tid, &ap_out[q], &first_rank[q]);
}

// Single-block deterministic reduction of dali_rank_eval_inp: inp[q] = n_rel / (last_rank + 1), one fp32 division (0 for an invalid
// query), and the mean over the valid queries of the same quotient taken in fp64.
__global__ __launch_bounds__(256) void rank_inp_reduce_kernel(const int32_t* __restrict__ last_rank, const int32_t* __restrict__ n_rel, int nq,
                                                               float* __restrict__ inp, double* __restrict__ minp64, int32_t* __restrict__ num_valid) {
    __shared__ double s_sum[256];
    __shared__ int s_valid[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    int nv = 0;
    for (int q = tid; q < nq; q += 256) {
        const int lr = last_rank[q], nr = n_rel[q];
        if (lr >= 0) {
            inp[q] = __fdiv_rn((float)nr, (float)(lr + 1));
            s += (double)nr / (double)(lr + 1);
            ++nv;
        } else {
            inp[q] = 0.f;
        }
    }
    s_sum[tid] = s; s_valid[tid] = nv;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_valid[tid] += s_valid[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        num_valid[0] = s_valid[0];
        minp64[0] = s_valid[0] > 0 ? s_sum[0] / (double)s_valid[0] : 0.0;
    }
}

// Single-block deterministic reduction: CMC curve + mAP over valid queries.
__global__ __launch_bounds__(256) void rank_reduce_kernel(const float* __restrict__ ap, const int32_t* __restrict__ first_rank,
                                                           int nq, int max_rank, float* __restrict__ cmc, float* __restrict__ mAP,
                                                           double* __restrict__ map64, int32_t* __restrict__ num_valid) {
    __shared__ double s_sum[256];
    __shared__ int s_valid[256];
    __shared__ int s_hist[1024];
    const int tid = threadIdx.x;
    for (int t = tid; t < 1024; t += 256) s_hist[t] = 0;
    __syncthreads();
    double s = 0.0;
    int nv = 0;
    for (int q = tid; q < nq; q += 256) {
        const int fr = first_rank[q];
        if (fr >= 0) {
            s += (double)ap[q];
            ++nv;
            if (fr < max_rank) atomicAdd(&s_hist[fr], 1);
        }
    }
    s_sum[tid] = s; s_valid[tid] = nv;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_valid[tid] += s_valid[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        const int n = s_valid[0];
        num_valid[0] = n;
        const double m = n > 0 ? s_sum[0] / (double)n : 0.0;
        mAP[0] = (float)m;
        if (map64) map64[0] = m;
        int run = 0;
        for (int k = 0; k < max_rank; ++k) {
            run += s_hist[k];
            cmc[k] = n > 0 ? (float)((double)run / (double)n) : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Gallery-sharded ranking (the evaluation path over N GPUs): every rank holds the distances of ALL queries to ITS slice of
// the gallery.  The position of a match in the full ranking is 1 + (kept gallery entries of every shard with a smaller key), keys being
// (distance, GLOBAL gallery index), so the merge is a sum of per-shard counts:
//   (1) rank_shard_matches_kernel: the keys of the query's matches inside this shard (identity slice of the shard's index, other camera);
//   (2) [host: all-gather of the keys]
//   (3) rank_shard_bins_kernel: all shards' match keys sorted in LDS (the same order on every rank: keys are unique); every kept entry of THIS
//       shard is binned by the number of matches with a smaller key, exactly as rank_query_kernel bins the whole row;
//   (4) [host: all-reduce SUM of the integer bins]
//   (5) rank_shard_finish_kernel: positions = inclusive scan of the bins, AP and first-hit rank by rank_ap_tail, the function that ends
//       rank_query_kernel (equal integer bins in, so the single-GPU result's bits out), then rank_reduce_kernel.
// Plain binary search over the sorted keys (no distance cells): this path is bounded by the collectives, not by the bins.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_shard_matches_kernel(const float* __restrict__ dist, const int32_t* __restrict__ q_pids,
                                                                  const int32_t* __restrict__ q_cams, const int32_t* __restrict__ g_cams,
                                                                  const int32_t* __restrict__ info, const int32_t* __restrict__ starts,
                                                                  const int32_t* __restrict__ order, int ng, int g_offset, int cap,
                                                                  unsigned long long* __restrict__ keys, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ status) {
    __shared__ int s_n;
    const int q = blockIdx.x, tid = threadIdx.x;
    unsigned long long* krow = keys + (size_t)q * cap;
    for (int t = tid; t < cap; t += 256) krow[t] = ~0ull;
    const int qp = q_pids[q], qc = q_cams[q];
    int sb, se;
    if (!rank_identity_slice(info, starts, qp, sb, se)) { if (tid == 0) counts[q] = 0; return; }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const float* drow = dist + (size_t)q * ng;
    for (int t = sb + tid; t < se; t += 256) {
        const int g = order[t];
        if (g_cams[g] != qc) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < cap) krow[slot] = rank_key(drow[g], g + g_offset);
        }
    }
    __syncthreads();
    if (tid == 0) {
        counts[q] = s_n < cap ? s_n : cap;
        if (s_n > cap) atomicMax(status, 1);
    }
}

__global__ __launch_bounds__(256) void rank_shard_bins_kernel(const float* __restrict__ dist, const int32_t* __restrict__ q_pids,
                                                               const int32_t* __restrict__ q_cams, const int32_t* __restrict__ g_cams,
                                                               const int32_t* __restrict__ info, const int32_t* __restrict__ starts,
                                                               const int32_t* __restrict__ order, int nq, int ng, int g_offset,
                                                               const unsigned long long* __restrict__ keys_all, const int32_t* __restrict__ counts_all,
                                                               int world, int cap, int32_t* __restrict__ bins, int bins_cap,
                                                               int32_t* __restrict__ status) {
    __shared__ unsigned long long s_key[RANK_PMAX];
    __shared__ int s_cnt[RANK_PMAX + 1];
    const int q = blockIdx.x, tid = threadIdx.x;
    int32_t* brow = bins + (size_t)q * (bins_cap + 1);
    int np = 0;
    for (int r = 0; r < world; ++r) np += counts_all[(size_t)r * nq + q];
    if (np > bins_cap || np > RANK_PMAX) { if (tid == 0) atomicMax(status, 1); np = 0; }
    for (int t = tid; t <= bins_cap; t += 256) brow[t] = 0;
    if (np == 0) return;
    // all shards' match keys of this query, in rank order (any order: they are sorted next)
    int base = 0;
    for (int r = 0; r < world; ++r) {
        const int n = counts_all[(size_t)r * nq + q];
        const unsigned long long* src = keys_all + ((size_t)r * nq + q) * cap;
        for (int t = tid; t < n; t += 256) s_key[base + t] = src[t];
        base += n;
    }
    for (int t = tid; t <= np; t += 256) s_cnt[t] = 0;             // behind the sort's own barrier between its pad and its passes
    block_pad_sort(s_key, np, 0, tid);
    const unsigned long long last_key = s_key[np - 1];
    auto bin = [&](float d, int g, int delta) {
        const unsigned long long k = rank_key(d, g + g_offset);
        if (k > last_key) return;                                     // beyond the last match: affects no position
        atomicAdd(&s_cnt[rank_lower_bound(s_key, 0, np, k)], delta);
    };
    const float* drow = dist + (size_t)q * ng;
    for (int g = tid; g < ng; g += 256) bin(drow[g], g, 1);
    // junk of this shard (same identity, same camera) comes back out; an empty slice where the shard lacks the identity or has no index
    const int qc = q_cams[q];
    int sb, se;
    rank_identity_slice(info, starts, q_pids[q], sb, se);
    __syncthreads();
    for (int t = sb + tid; t < se; t += 256) { const int g = order[t]; if (g_cams[g] == qc) bin(drow[g], g, -1); }
    __syncthreads();
    for (int t = tid; t <= np; t += 256) brow[t] = s_cnt[t];
}

__global__ __launch_bounds__(256) void rank_shard_finish_kernel(const int32_t* __restrict__ bins, const int32_t* __restrict__ counts_all, int world,
                                                                 int nq, int bins_cap, float* __restrict__ ap_out, int32_t* __restrict__ first_rank) {
    __shared__ int s_scan[256];
    __shared__ float s_red[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    int np = 0;
    for (int r = 0; r < world; ++r) np += counts_all[(size_t)r * nq + q];
    if (np == 0 || np > bins_cap) { if (tid == 0) { ap_out[q] = 0.f; first_rank[q] = -1; } return; }
    const int32_t* brow = bins + (size_t)q * (bins_cap + 1);
    rank_ap_tail([&](int t) { return brow[t]; }, np, s_scan, s_red, tid, &ap_out[q], &first_rank[q]);     // rank_query_kernel's step 4, the same function
}

}  // namespace dali

using namespace dali;

// gallery positions counting-sorted by identity (info = {min, max} pid; starts over [min, max]; order = positions grouped by pid)
static int build_gallery_index(hipStream_t st, const int32_t* g_pids, int ng, int32_t* info, int32_t* counts, int32_t* starts, int32_t* cursor,
                               int32_t* order, int32_t* status) {
    const int32_t init[2] = {0x7fffffff, (int32_t)0x80000000};
    DALI_HIP(hipMemcpyAsync(info, init, sizeof(init), hipMemcpyHostToDevice, st));
    const int gb = (ng + 255) / 256 < 1024 ? (ng + 255) / 256 : 1024;
    hipLaunchKernelGGL(rank_index_minmax_kernel, dim3(gb), dim3(256), 0, st, g_pids, ng, info);
    DALI_LAUNCH_CHECK();
    DALI_HIP(hipMemsetAsync(counts, 0, ((size_t)RANK_MAX_PID_RANGE + 1) * 4, st));
    hipLaunchKernelGGL(rank_index_count_kernel, dim3(gb), dim3(256), 0, st, g_pids, ng, info, counts, status);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_index_scan_kernel, dim3(1), dim3(1024), 0, st, info, counts, starts, cursor);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_index_scatter_kernel, dim3(gb), dim3(256), 0, st, g_pids, ng, info, starts, cursor, order);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}
// the index of a gallery (shard) in the context workspace: -> info / starts / order
static int shard_index(dali_ctx* ctx, hipStream_t st, const int32_t* g_pids, int ng, int32_t* status, int32_t*& info, int32_t*& starts, int32_t*& order) {
    const size_t b_info = 256, b_order = align_up((size_t)ng * 4, 256), b_tab = align_up(((size_t)RANK_MAX_PID_RANGE + 1) * 4, 256);
    char* ws = static_cast<char*>(workspace(ctx, b_info + b_order + 3 * b_tab));
    if (!ws) return DALI_ERR_NOMEM;
    info = reinterpret_cast<int32_t*>(ws);
    order = reinterpret_cast<int32_t*>(ws + b_info);
    int32_t* counts = reinterpret_cast<int32_t*>(ws + b_info + b_order);
    starts = counts + b_tab / 4;
    return build_gallery_index(st, g_pids, ng, info, counts, starts, starts + b_tab / 4, order, status);
}

extern "C" int dali_rank_shard_matches(dali_ctx* ctx, void* stream, const float* dist_shard, const int32_t* q_pids, const int32_t* g_pids,
                                       const int32_t* q_camids, const int32_t* g_camids, int nq, int ng, int g_offset, int cap,
                                       int64_t* keys, int32_t* counts, int32_t* status) {
    DALI_REQUIRE(ctx && dist_shard && q_pids && g_pids && q_camids && g_camids && keys && counts && status, "dali_rank_shard_matches: null argument");
    DALI_REQUIRE(nq > 0 && ng > 0 && g_offset >= 0 && cap > 0 && cap <= RANK_PMAX, "dali_rank_shard_matches: bad shape nq=%d ng=%d offset=%d cap=%d", nq, ng, g_offset, cap);
    hipStream_t st = (hipStream_t)stream;
    DALI_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    int32_t *info, *starts, *order;
    if (int rc = shard_index(ctx, st, g_pids, ng, status, info, starts, order)) return rc;
    hipLaunchKernelGGL(rank_shard_matches_kernel, dim3(nq), dim3(256), 0, st, dist_shard, q_pids, q_camids, g_camids, info, starts, order, ng, g_offset, cap,
                       reinterpret_cast<unsigned long long*>(keys), counts, status);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_rank_shard_bins(dali_ctx* ctx, void* stream, const float* dist_shard, const int32_t* q_pids, const int32_t* g_pids,
                                    const int32_t* q_camids, const int32_t* g_camids, int nq, int ng, int g_offset, const int64_t* keys_all,
                                    const int32_t* counts_all, int world, int cap, int32_t* bins, int bins_cap, int32_t* status) {
    DALI_REQUIRE(ctx && dist_shard && q_pids && g_pids && q_camids && g_camids && keys_all && counts_all && bins && status, "dali_rank_shard_bins: null argument");
    DALI_REQUIRE(nq > 0 && ng > 0 && g_offset >= 0 && world > 0 && cap > 0 && bins_cap > 0 && bins_cap <= RANK_PMAX,
                 "dali_rank_shard_bins: bad shape nq=%d ng=%d world=%d cap=%d bins_cap=%d (<= %d)", nq, ng, world, cap, bins_cap, RANK_PMAX);
    hipStream_t st = (hipStream_t)stream;
    DALI_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    int32_t *info, *starts, *order;
    if (int rc = shard_index(ctx, st, g_pids, ng, status, info, starts, order)) return rc;
    hipLaunchKernelGGL(rank_shard_bins_kernel, dim3(nq), dim3(256), 0, st, dist_shard, q_pids, q_camids, g_camids, info, starts, order, nq, ng, g_offset,
                       reinterpret_cast<const unsigned long long*>(keys_all), counts_all, world, cap, bins, bins_cap, status);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_rank_shard_finish(dali_ctx* ctx, void* stream, const int32_t* bins, const int32_t* counts_all, int world, int nq, int bins_cap,
                                      int max_rank, float* cmc, float* mAP, double* map64, int32_t* num_valid, float* ap, int32_t* first_rank) {
    DALI_REQUIRE(ctx && bins && counts_all && cmc && mAP && num_valid && ap && first_rank, "dali_rank_shard_finish: null argument");
    DALI_REQUIRE(nq > 0 && world > 0 && bins_cap > 0 && max_rank > 0 && max_rank <= 1024, "dali_rank_shard_finish: bad shape");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rank_shard_finish_kernel, dim3(nq), dim3(256), 0, st, bins, counts_all, world, nq, bins_cap, ap, first_rank);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_reduce_kernel, dim3(1), dim3(256), 0, st, ap, first_rank, nq, max_rank, cmc, mAP, map64, num_valid);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

// The per-query stage of dali_rank_eval / dali_rank_eval_inp: status cleared, the gallery index by identity (counting sort over [min pid,
// max pid]) in the context workspace behind the ap / first_rank scratch, then the two-tier query launches.
template <bool INP>
static int rank_queries(dali_ctx* ctx, hipStream_t st, const float* distmat, const int32_t* q_pids, const int32_t* g_pids, const int32_t* q_camids,
                        const int32_t* g_camids, int nq, int ng, float* ap, int32_t* first_rank, int32_t* last_rank, int32_t* n_rel,
                        int32_t* status, float*& ap_buf, int32_t*& fr_buf) {
    ap_buf = ap;
    fr_buf = first_rank;
    DALI_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    const size_t head = (!ap || !first_rank) ? align_up((size_t)nq * 4, 256) * 2 : 0;
    const size_t b_info = 256, b_order = align_up((size_t)ng * 4, 256), b_pend = align_up((size_t)nq * 4, 256);
    const size_t b_tab = align_up(((size_t)RANK_MAX_PID_RANGE + 1) * 4, 256);
    char* ws = static_cast<char*>(workspace(ctx, head + b_info + b_order + b_pend + 3 * b_tab));
    if (!ws) return DALI_ERR_NOMEM;
    if (!ap) ap_buf = reinterpret_cast<float*>(ws);
    if (!first_rank) fr_buf = reinterpret_cast<int32_t*>(ws + align_up((size_t)nq * 4, 256));
    int32_t* info = reinterpret_cast<int32_t*>(ws + head);
    int32_t* order = reinterpret_cast<int32_t*>(ws + head + b_info);
    int32_t* pending = reinterpret_cast<int32_t*>(ws + head + b_info + b_order);
    int32_t* counts = reinterpret_cast<int32_t*>(ws + head + b_info + b_order + b_pend);
    int32_t* starts = counts + b_tab / 4;
    int32_t* cursor = starts + b_tab / 4;
    if (int rc = build_gallery_index(st, g_pids, ng, info, counts, starts, cursor, order, status)) return rc;
    hipLaunchKernelGGL((rank_query_kernel<RANK_PSMALL, 0, INP>), dim3(nq), dim3(256), 0, st, distmat, q_pids, q_camids, g_camids, info, starts, order,
                       nq, ng, ap_buf, fr_buf, pending, status, last_rank, n_rel);
    DALI_LAUNCH_CHECK();
    hipLaunchKernelGGL((rank_query_kernel<RANK_PMAX, 1, INP>), dim3(nq), dim3(256), 0, st, distmat, q_pids, q_camids, g_camids, info, starts, order,
                       nq, ng, ap_buf, fr_buf, pending, status, last_rank, n_rel);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_rank_eval(dali_ctx* ctx, void* stream, const float* distmat, const int32_t* q_pids,
                              const int32_t* g_pids, const int32_t* q_camids, const int32_t* g_camids, int nq, int ng,
                              int max_rank, float* cmc, float* mAP, double* map64, int32_t* num_valid, float* ap,
                              int32_t* first_rank, int32_t* status) {
    DALI_REQUIRE(ctx && distmat && q_pids && g_pids && q_camids && g_camids && cmc && mAP && num_valid && status,
                 "dali_rank_eval: null argument");
    DALI_REQUIRE(nq > 0 && ng > 0, "dali_rank_eval: bad shape nq=%d ng=%d", nq, ng);
    DALI_REQUIRE(max_rank > 0 && max_rank <= 1024, "dali_rank_eval: max_rank %d outside 1..1024", max_rank);
    hipStream_t st = (hipStream_t)stream;
    float* ap_buf;
    int32_t* fr_buf;
    if (int rc = rank_queries<false>(ctx, st, distmat, q_pids, g_pids, q_camids, g_camids, nq, ng, ap, first_rank, nullptr, nullptr, status, ap_buf, fr_buf))
        return rc;
    hipLaunchKernelGGL(rank_reduce_kernel, dim3(1), dim3(256), 0, st, ap_buf, fr_buf, nq, max_rank, cmc, mAP, map64, num_valid);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

// mINP beside dali_rank_eval (include/daliid.h): the same query kernels, keeping where the scan of rank_ap_tail ends.  One GPU only:
// the sharded path (dali_rank_shard_*) has no INP entry.
extern "C" int dali_rank_eval_inp(dali_ctx* ctx, void* stream, const float* distmat, const int32_t* q_pids, const int32_t* g_pids,
                                  const int32_t* q_camids, const int32_t* g_camids, int nq, int ng, float* inp, int32_t* last_rank,
                                  int32_t* n_rel, double* minp64, int32_t* num_valid, int32_t* status) {
    DALI_REQUIRE(ctx && distmat && q_pids && g_pids && q_camids && g_camids && inp && last_rank && n_rel && minp64 && num_valid && status,
                 "dali_rank_eval_inp: null argument");
    DALI_REQUIRE(nq > 0 && ng > 0, "dali_rank_eval_inp: bad shape nq=%d ng=%d", nq, ng);
    hipStream_t st = (hipStream_t)stream;
    float* ap_buf;
    int32_t* fr_buf;
    if (int rc = rank_queries<true>(ctx, st, distmat, q_pids, g_pids, q_camids, g_camids, nq, ng, nullptr, nullptr, last_rank, n_rel, status, ap_buf, fr_buf))
        return rc;
    hipLaunchKernelGGL(rank_inp_reduce_kernel, dim3(1), dim3(256), 0, st, last_rank, n_rel, nq, inp, minp64, num_valid);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

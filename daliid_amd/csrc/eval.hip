// eval.hip -- evaluation path of validateModels.validate (validateModels.py:35-76):
//   row L2 normalisation (:41-42) and distmat = 1 - q @ g.T (:47) on MFMA, plus the loss heads' small similarity GEMMs.
//   The market1501 CMC/mAP ranking (:68) that follows them is rank.hip.
#include "gemm_tile.h"
#include "topk_key.h"
#include <cstdlib>
#include <type_traits>

namespace dali {

// ------------------------------------------------------------------------------------------------
// Row pre-pass: one wave64 per row.  Optionally normalises (y = x / (|x| + eps)), emits the bf16 operand image
// (zero-padded to Kp columns), |y|^2, and/or the fp32 row.  Operand image layouts (what the distance kernels DMA):
//   layout 1 (bf16):    [n][Kp] bf16, Kp = roundup(d, 64): a 64-deep k-step of one row is one 128-byte cache line;
//   layout 3 (bf16 x3): [n][Kp/32][hi 32 | lo 32] bf16, Kp = roundup(d, 32), lo = bf16(y - hi): the hi and lo parts of a
//                       32-deep k-step of one row share one 128-byte line (the L2 -> LDS path retires whole lines, see conv.hip).
// HBM-bound: reads 4 B/elem once, writes 2-4 B/elem.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rows_prep_kernel(const float* __restrict__ x, int n, int d, int Kp,
                                                         int normalize, float eps, uint16_t* __restrict__ img,
                                                         int layout, float* __restrict__ sq,
                                                         float* __restrict__ yout, float* __restrict__ norms) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* xr = x + (size_t)row * d;
    float ss = 0.f;
    const bool vec = (d & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
    if (vec && Kp == d && d <= 2048 && !yout && img) {
        // the whole row in registers (<= 8 float4 per lane): all loads in flight at once, one pass over memory.  Same arithmetic, in the same
        // order, as the two-sweep form below (the squares are added chunk by chunk, lane sums by wave_sum).
        float4 v4[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = lane * 4 + k * 256;
            v4[k] = c < d ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (lane * 4 + k * 256 < d) ss += v4[k].x * v4[k].x + v4[k].y * v4[k].y + v4[k].z * v4[k].z + v4[k].w * v4[k].w;
        ss = wave_sum(ss);
        const float nrm1 = sqrtf(ss);
        const float den1 = normalize ? (nrm1 + eps) : 1.0f;
        if (lane == 0) {
            if (norms) norms[row] = nrm1;
            if (sq) sq[row] = normalize ? (ss / (den1 * den1)) : ss;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = lane * 4 + k * 256;
            if (c < d) {
                const float v[4] = {v4[k].x / den1, v4[k].y / den1, v4[k].z / den1, v4[k].w / den1};
                uint16_t h[4], l[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    h[t] = f32_to_bf16_bits(v[t]);
                    l[t] = f32_to_bf16_bits(v[t] - bf16_bits_to_f32(h[t]));
                }
                const uint2 hv = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
                if (layout == 3) {
                    uint16_t* dst = img + (size_t)row * (2 * Kp) + (c >> 5) * 64 + (c & 31);
                    const uint2 lv = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
                    *reinterpret_cast<uint2*>(dst) = hv;
                    *reinterpret_cast<uint2*>(dst + 32) = lv;
                } else {
                    *reinterpret_cast<uint2*>(img + (size_t)row * Kp + c) = hv;
                }
            }
        }
        return;
    }
    if (vec) {
        for (int c = lane * 4; c < d; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(xr + c);
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    } else {
        for (int c = lane; c < d; c += 64) { const float v = xr[c]; ss += v * v; }
    }
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    const float den = normalize ? (nrm + eps) : 1.0f;
    if (lane == 0) {
        if (norms) norms[row] = nrm;
        if (sq) sq[row] = normalize ? (ss / (den * den)) : ss;
    }
    if (vec && Kp == d && (reinterpret_cast<uintptr_t>(yout) & 15) == 0) {
        // second sweep, whole float4 chunks (d % 4 == 0, no column padding): 16-byte loads of the L1 / L2-resident row, no per-element
        // predicates (the scalar form below issued four predicated dword loads per chunk, each behind its own branch)
        for (int c = lane * 4; c < d; c += 256) {
            const float4 x4 = *reinterpret_cast<const float4*>(xr + c);
            const float v[4] = {x4.x / den, x4.y / den, x4.z / den, x4.w / den};
            if (yout) *reinterpret_cast<float4*>(yout + (size_t)row * d + c) = make_float4(v[0], v[1], v[2], v[3]);
            if (img) {
                uint16_t h[4], l[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    h[t] = f32_to_bf16_bits(v[t]);
                    l[t] = f32_to_bf16_bits(v[t] - bf16_bits_to_f32(h[t]));
                }
                const uint2 hv = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
                if (layout == 3) {
                    uint16_t* dst = img + (size_t)row * (2 * Kp) + (c >> 5) * 64 + (c & 31);
                    const uint2 lv = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
                    *reinterpret_cast<uint2*>(dst) = hv;
                    *reinterpret_cast<uint2*>(dst + 32) = lv;
                } else {
                    *reinterpret_cast<uint2*>(img + (size_t)row * Kp + c) = hv;
                }
            }
        }
        return;
    }
    // second sweep (the row is L1/L2 resident): write outputs
    for (int c = lane * 4; c < Kp; c += 256) {
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = (c + t < d) ? xr[c + t] / den : 0.f;
        if (yout) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (c + t < d) yout[(size_t)row * d + c + t] = v[t];
        }
        if (img) {
            uint16_t h[4], l[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                h[t] = f32_to_bf16_bits(v[t]);
                l[t] = f32_to_bf16_bits(v[t] - bf16_bits_to_f32(h[t]));
            }
            const uint2 hv = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
            if (layout == 3) {
                uint16_t* dst = img + (size_t)row * (2 * Kp) + (c >> 5) * 64 + (c & 31);
                const uint2 lv = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
                *reinterpret_cast<uint2*>(dst) = hv;
                *reinterpret_cast<uint2*>(dst + 32) = lv;
            } else {
                *reinterpret_cast<uint2*>(img + (size_t)row * Kp + c) = hv;
            }
        }
    }
}

__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          int n, int d, float eps, float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* xr = x + (size_t)row * d;
    const float* gr = dy + (size_t)row * d;
    float ss = 0.f, xg = 0.f;
#pragma unroll 8
    for (int c = lane; c < d; c += 64) { const float v = xr[c]; ss += v * v; xg += v * gr[c]; }
    ss = wave_sum(ss); xg = wave_sum(xg);
    const float nrm = sqrtf(ss), den = nrm + eps;
    const float a = 1.0f / den;
    const float b = (nrm > 0.f) ? xg / (nrm * den * den) : 0.f;
#pragma unroll 8
    for (int c = lane; c < d; c += 64) dx[(size_t)row * d + c] = gr[c] * a - xr[c] * b;
}

// ------------------------------------------------------------------------------------------------
// Pair distance: out[q][g] = 1 - Q[q].G[g]   (or |q|^2 + |g|^2 - 2 q.g)
// MFMA rows (m) = gallery, MFMA columns (n) = query, so each lane's 4 accumulator registers are 4
// consecutive gallery entries of one query row: one 16-byte store.
// Algorithmic work: 2*d FLOP per pair (x3 MFMA issue in split-bf16 mode); bound: MFMA.
// ------------------------------------------------------------------------------------------------
template <int NPROD>
struct PairCfg { using type = GemmCfg<128, 128, (NPROD == 3 ? 2 : 1), (NPROD == 3 ? 2 : 1), NPROD>; };

struct RowLoader {                       // 32-deep k-tile kt of row `row` of an operand image; arr 1 = the lo part (layout 3)
    const uint16_t* p;
    int row0, nrows, pitch, kstep;
    __device__ __forceinline__ uint4 operator()(int arr, int row, int kt, int kc) const {
        const int r = row0 + row;
        if (r >= nrows) return make_uint4(0, 0, 0, 0);
        return *reinterpret_cast<const uint4*>(p + (size_t)r * pitch + kt * kstep + arr * 32 + kc * 8);
    }
};

// Two-model fusion epilogue (evaluateCleanATModels.py:154-157): with `out` holding the first model's distances d1,
//   out = (w1*d1 + w2*d2) / (w1 + w2),  w_m[q,g] = max(qmag_m[q], gmag_m[g])   (null magnitudes: weight 1 = the
// "simple ensemble" (d1+d2)/2 of :126), d2 = this launch's 1 - q.g.
struct PairBlend {
    const float* qmag1; const float* gmag1;
    const float* qmag2; const float* gmag2;
    int on;
};

// Epilogue shared by the distance kernels: metric, optional two-model blend, fp32 store (4 consecutive gallery entries per lane).
// mb / nb: this lane's first gallery row / query column inside the tile (accumulator layout: rows (lane>>4)*4 + r, column lane&15).
template <int FM, int FN>
__device__ __forceinline__ void pairdist_epilogue(f32x4_t (&acc)[FM][FN], int g_tile0, int q_tile0, int mb, int nb, const float* __restrict__ gsq,
                                                  const float* __restrict__ qsq, int ng, int nq, int metric, float* out, const PairBlend& blend) {
    const bool vec_ok = (ng & 3) == 0;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int q = q_tile0 + nb + j * 16;
        if (q >= nq) continue;
        const float qq = (metric == DALI_METRIC_L2SQ) ? qsq[q] : 0.f;
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int g0 = g_tile0 + mb + i * 16;
            if (g0 >= ng) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dot = acc[i][j][r];
                if (metric == DALI_METRIC_L2SQ) {
                    const float gg = (g0 + r < ng) ? gsq[g0 + r] : 0.f;
                    v[r] = qq + gg - 2.0f * dot;
                } else if (metric == DALI_METRIC_DOT) {
                    v[r] = dot;
                } else {
                    v[r] = 1.0f - dot;
                }
            }
            float* o = out + (size_t)q * ng + g0;
            if (blend.on) {
                const float qm1 = blend.qmag1 ? blend.qmag1[q] : 1.f, qm2 = blend.qmag2 ? blend.qmag2[q] : 1.f;
                float prev[4];
                if (vec_ok && g0 + 3 < ng) {
                    const float4 p4 = *reinterpret_cast<const float4*>(o);
                    prev[0] = p4.x; prev[1] = p4.y; prev[2] = p4.z; prev[3] = p4.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) prev[r] = (g0 + r < ng) ? o[r] : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int g = (g0 + r < ng) ? g0 + r : g0;
                    const float w1 = fmaxf(qm1, blend.gmag1 ? blend.gmag1[g] : 1.f);
                    const float w2 = fmaxf(qm2, blend.gmag2 ? blend.gmag2[g] : 1.f);
                    v[r] = (w1 * prev[r] + w2 * v[r]) / (w1 + w2);
                }
            }
            if (vec_ok && g0 + 3 < ng) {
                // non-temporal: the 4 GB result streams past the Infinity Cache instead of evicting the operand panels every XCD re-reads each round
                // (PMC: 24.7 GB fetched behind the L2 per launch); 10k x 100k x 2048: 9.77 -> 9.44 ms, the ranking kernel behind it unchanged
                typedef float f32x4_nt __attribute__((ext_vector_type(4)));
                const f32x4_nt vv = {v[0], v[1], v[2], v[3]};
                __builtin_nontemporal_store(vv, reinterpret_cast<f32x4_nt*>(o));
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (g0 + r < ng) o[r] = v[r];
            }
        }
    }
}

template <int NPROD>
__global__ __launch_bounds__(256) void pairdist_kernel(const uint16_t* __restrict__ G, const uint16_t* __restrict__ Q,
                                                       const float* __restrict__ gsq, const float* __restrict__ qsq,
                                                       int ng, int nq, int Kp, int metric, float* out,
                                                       int tiles_m, int tiles_n, PairBlend blend) {
    using Cfg = typename PairCfg<NPROD>::type;
    extern __shared__ __attribute__((aligned(16))) uint16_t smem[];
    int tm, tn;
    if (!xcd_tile_map(blockIdx.x, tiles_m, tiles_n, tm, tn)) return;
    f32x4_t acc[Cfg::FM][Cfg::FN];
#pragma unroll
    for (int i = 0; i < Cfg::FM; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    RowLoader la{G, tm * Cfg::TM, ng, NPROD == 3 ? 2 * Kp : Kp, NPROD == 3 ? 64 : 32};
    RowLoader lb{Q, tn * Cfg::TN, nq, NPROD == 3 ? 2 * Kp : Kp, NPROD == 3 ? 64 : 32};
    gemm_mainloop<Cfg>(acc, la, lb, Kp / 32, smem);

    int mb, nb;
    acc_coords<Cfg>(mb, nb);
    pairdist_epilogue<Cfg::FM, Cfg::FN>(acc, tm * Cfg::TM, tn * Cfg::TN, mb, nb, gsq, qsq, ng, nq, metric, out, blend);
}

// Epilogue of the persistent kernel for interior tiles: whole 128-byte lines per store instruction.  In the accumulator layout a store
// instruction covers 16 query rows x 64 bytes (half a line per row); streamed non-temporally past the caches those halves reached memory as
// partial-line writes (PMC WRITE_SIZE 5.50 GB per launch for a 4.00 GB result, round 3).  Here each wave passes its 64 x 64 sub-tile through a
// PRIVATE 2 KiB strip of LDS behind the ring (3 x 48 + 8 x 2 = all 160 KiB of the CU) (the three ring stages are all busy during the epilogue: the producers are already fetching the
// next tile), one block of 16 query rows x 32 gallery entries at a time: two ds_write_b128 per lane in the accumulator layout, two ds_read_b128 in
// which 8 adjacent lanes hold one row's 128 bytes, two 16-byte stores of 8 rows x one full line each.  No workgroup barrier (the strip is the
// wave's own; a wave's LDS operations execute in order), no registers live across the k-loop.
constexpr int PAIR_STRIP_PITCH = 128;                         // bytes per staged row; 16-byte chunk c of row q sits at chunk c ^ (q & 7): the 8 lanes of a
constexpr int PAIR_STRIP_BYTES = 16 * PAIR_STRIP_PITCH;       // ds_write_b128 group (8 rows, one chunk) land on 8 distinct bank quads
__device__ __forceinline__ void pairdist_epilogue_lines(f32x4_t (&acc)[4][4], int g0w, int q0w, int lane, const float* __restrict__ gsq,
                                                        const float* __restrict__ qsq, int ng, int metric, float* out, char* strip) {
    // g0w / q0w: first gallery entry / query row of this wave's 64 x 64 sub-tile
    char* wr = strip + (lane & 15) * PAIR_STRIP_PITCH;                            // + ((ii * 4 + (lane >> 4)) ^ (lane & 7)) * 16
    const int wsw = lane & 7, wch = lane >> 4;
    const char* rd = strip + (lane >> 3) * PAIR_STRIP_PITCH + (((lane & 7) ^ ((lane >> 3) & 7)) << 4);   // + t * 8 * PITCH (rows + 8: same swizzle)
    float* obase = out + (size_t)(q0w + (lane >> 3)) * ng + g0w + (lane & 7) * 4;
    typedef float f32x4_nt __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float qq = 0.f;
        if (metric == DALI_METRIC_L2SQ) qq = qsq[q0w + j * 16 + (lane & 15)];
#pragma unroll
        for (int ih = 0; ih < 2; ++ih) {
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int i = ih * 2 + ii;
                f32x4_t v;
                if (metric == DALI_METRIC_L2SQ) {
                    const float4 gg = *reinterpret_cast<const float4*>(gsq + g0w + i * 16 + (lane >> 4) * 4);
                    v = f32x4_t{qq + gg.x - 2.0f * acc[i][j][0], qq + gg.y - 2.0f * acc[i][j][1], qq + gg.z - 2.0f * acc[i][j][2], qq + gg.w - 2.0f * acc[i][j][3]};
                } else if (metric == DALI_METRIC_DOT) {
                    v = acc[i][j];
                } else {
                    v = f32x4_t{1.0f - acc[i][j][0], 1.0f - acc[i][j][1], 1.0f - acc[i][j][2], 1.0f - acc[i][j][3]};
                }
                *reinterpret_cast<f32x4_t*>(wr + (((ii * 4 + wch) ^ wsw) << 4)) = v;
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f32x4_t v = *reinterpret_cast<const f32x4_t*>(rd + t * 8 * PAIR_STRIP_PITCH);
                const f32x4_nt vv = {v[0], v[1], v[2], v[3]};
                __builtin_nontemporal_store(vv, reinterpret_cast<f32x4_nt*>(obase + (size_t)(j * 16 + t * 8) * ng + ih * 32));
            }
        }
    }
}

// Selecting epilogue (PairTopk, topk_key.h): the metric arithmetic of pairdist_epilogue, then one compare of the ordered value bits against
// the query's threshold rejects almost every element; a survivor takes a slot of its query's candidate list.  Nothing of the tile is stored.
// Edge tiles take the same bounds checks as pairdist_epilogue.
__device__ __forceinline__ void pairdist_epilogue_topk(f32x4_t (&acc)[4][4], int g_tile0, int q_tile0, int mb, int nb, const float* __restrict__ gsq,
                                                       const float* __restrict__ qsq, int ng, int nq, int metric, const PairTopk& t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = q_tile0 + nb + j * 16;
        if (q >= nq) continue;
        const float qq = (metric == DALI_METRIC_L2SQ) ? qsq[q] : 0.f;
        const unsigned long long thr = t.keys[(size_t)q * t.k + t.k - 1];
        const unsigned int thr_hi = (unsigned int)(thr >> 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int g0 = g_tile0 + mb + i * 16;
            if (g0 >= ng) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (g0 + r >= ng) continue;
                const float dot = acc[i][j][r];
                float v;
                if (metric == DALI_METRIC_L2SQ) {
                    const float gg = gsq[g0 + r];
                    v = qq + gg - 2.0f * dot;
                } else if (metric == DALI_METRIC_DOT) {
                    v = dot;
                } else {
                    v = 1.0f - dot;
                }
                const unsigned int hi = topk_ordered_bits(v, t.largest);
                if (hi > thr_hi) continue;
                const unsigned long long key = ((unsigned long long)hi << 32) | (unsigned int)(t.g_offset + g0 + r);
                if (key >= thr) continue;
                const int slot = atomicAdd(&t.cnt[q], 1);
                if (slot < t.cap) t.cand[(size_t)q * t.cap + slot] = key;
                else *t.flag = 1;
            }
        }
    }
}

// LDS-DMA version (what the launcher uses when the operands fit 32-bit buffer offsets): 128 gallery rows x 256 query
// rows per 8-wave block (wave (wm, wn) of the 2 x 4 grid owns 64 x 64).  A k-step takes one 128-byte line of every operand
// row ([hi 32 | lo 32] for NPROD = 3, 64 consecutive k for NPROD = 1) by buffer_load_dwordx4 ... lds (a DMA piece = 8 rows,
// no VGPR staging) into a [rows][64] LDS image (physical 16-byte chunk = logical ^ ((row >> 1) & 7), as the k-tile-64 conv
// kernel); 48 KiB per stage, 3-stage ring with counted vmcnt.  Per k-step a wave reads 16 fragments for 48 (NPROD = 3: hi.hi +
// hi.lo + lo.hi) or 32 MFMAs.
// Wave specialisation: waves 8..15 only issue the DMA pieces (60-185 issue cycles each; 6 per wave and k-step used to sit in
// the MFMA waves' instruction streams and the feed time ADDED to the MFMA time: compute-only 0.89 us per k-step, with the feed
// 1.17 us), waves 0..7 only read fragments and issue MFMAs: 1.03 us per k-step (bf16 x3), 0.45 -> 0.37 us (bf16).
// Persistent: one workgroup per CU walks its tiles; the k-steps of all tiles form one stream through the ring, so the next
// tile's first k-steps are fetched under the stores of the finished one.
// Measured and not kept: the two waves of a SIMD issuing their DMA pieces at different points of the k-step (no change); a
// software-pipelined loop (wait + barrier half way through the k-step, next tile's first fragments fetched under the second
// half of the MFMAs: the DMA lead shrinks from two k-steps to one, +5 % / +18 % time); the tile staged through the free ring
// stage and stored as 512-byte contiguous rows (the stores cost 8 of the 11 us a tile spends outside its k-loop, found by
// removing them; staged they cost 6, but the kernel reaches the 128-VGPR cap, spills 15 registers around the k-loop and the
// k-step slows by 10 %).
// Round 4: the tile now leaves through a private 2 KiB strip per consumer wave behind the ring (pairdist_epilogue_lines: whole 128-byte
// lines per store, no spill: 123 VGPRs): 9.03 -> 8.72 ms (bf16 3.99 -> 3.62).  Measured and removed again: (a) 8 consumer + 4 producer waves
// (3 waves per SIMD, 168 VGPRs): 8.93 against 8.91 ms, so four producers do feed the ring; (b) on that kernel, three of a tile's four query
// columns kept in 48 registers and handed to the store path one (column, half) block every ktiles / 6 k-steps of the NEXT tile, so that
// the stores run under its MFMAs: 9.41 ms (+5 %; bf16 3.64 against 3.51) -- stores issued inside the k-loop delay the LDS-DMA loads of the
// same CU by more than the exposed burst costs; (c) start phases per XCD (blockIdx.x & 7) instead of per workgroup: 8.69-8.73 against 8.72.
// EPI, the type of the last argument, is what a finished tile does: PairBlend (the default) stores it, blended or not; PairGate stores it
// if the launch's gate word is set and ends the launch at once otherwise; PairTopk selects from it and stores nothing
// (pairdist_epilogue_topk).  Resolved with if constexpr: the PairBlend instantiations are the kernels they were before the policy existed.
template <int NPROD, class EPI = PairBlend>
__global__ __launch_bounds__(1024) void pairdist_dma_kernel(const uint16_t* __restrict__ G, const uint16_t* __restrict__ Q,
                                                            const float* __restrict__ gsq, const float* __restrict__ qsq,
                                                            int ng, int nq, int pitch, int ktiles, int metric, float* out,
                                                            int tiles_m, int tiles_n, int vgrid, EPI blend) {
    if constexpr (std::is_same_v<EPI, PairGate>) {
        if (blend.gate[0] == 0) return;
    }
    constexpr int TM = 128, TN = 256;
    constexpr int A_ELEMS = TM * 64, B_ELEMS = TN * 64, STAGE = A_ELEMS + B_ELEMS;
    constexpr int A_PIECES = TM / 8, NDMA = (TM + TN) / 8 / 8;                   // 1 KiB DMA pieces: 16 of A, 6 per producer wave
    static_assert(A_PIECES % 8 == 0, "a producer's piece i is a gallery piece for every producer or for none");
    extern __shared__ __attribute__((aligned(16))) uint16_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Persistent: this workgroup owns the virtual blocks v = blockIdx.x, + gridDim.x, ... (gridDim.x is a multiple of 8, so v
    // stays on this XCD's share of the tile map); the k-steps of all its tiles form one stream through the 3-stage ring, so
    // the producers fetch the next tile's first two k-steps while the consumers store the finished tile.
    int n_tiles = 0;
    for (int v = blockIdx.x; v < vgrid; v += gridDim.x) { int tm, tn; n_tiles += xcd_tile_map(v, tiles_m, tiles_n, tm, tn) ? 1 : 0; }
    if (n_tiles == 0) return;
    // (Measured and removed: a staggered start of the workgroups, in 8 phases an eighth of a tile apart per workgroup -- 9.67 -> 10.1-10.5 ms, it gives up
    // the XCD's L2 panel sharing -- or per XCD, blockIdx.x & 7 -- 8.69-8.73 against 8.72 ms.  The stores' 8 us per tile are not burst contention.)
    if (wave >= 8) {
        // ---- producer waves 8..15 (two per SIMD, next to two consumers): nothing but the DMA ring ----
        const int pw = wave - 8;
        const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(G), 0, ng * pitch * 2, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_q = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(Q), 0, nq * pitch * 2, 0x00020000);
        // pieces q = pw + 8*i; q < 16: rows 8q.. of the gallery tile, else rows 8(q-16).. of the query tile; both piece indices
        // have the parity of pw, so one logical chunk per lane serves all of them
        const int r_in = lane >> 3;
        const int kc = (lane & 7) ^ (((pw & 1) << 2) | (r_in >> 1));
        uint32_t off[NDMA];
        int v_next = blockIdx.x, kt_next = 0, st_fill = 0;            // the step the next issue() fetches
        auto seek_tile = [&]() {                                      // advance v_next to the next valid tile and load its row offsets
            int tm = 0, tn = 0;
            while (!xcd_tile_map(v_next, tiles_m, tiles_n, tm, tn)) v_next += gridDim.x;
#pragma unroll
            for (int i = 0; i < NDMA; ++i) {
                const int q = pw + 8 * i;
                const bool is_a = q < A_PIECES;
                const int row = is_a ? tm * TM + q * 8 + r_in : tn * TN + (q - A_PIECES) * 8 + r_in;
                off[i] = (row < (is_a ? ng : nq)) ? (uint32_t)(row * pitch + kc * 8) * 2u : DMA_OOB;
            }
        };
        auto issue = [&]() {
            if (kt_next == 0) seek_tile();
            uint16_t* base = smem + st_fill * STAGE;
#pragma unroll
            for (int i = 0; i < NDMA; ++i) {
                const uint32_t o = (off[i] == DMA_OOB) ? DMA_OOB : off[i] + (uint32_t)(kt_next * 128);
                uint16_t* dst = base + (pw + 8 * i) * 512;
                if (8 * i + 7 < A_PIECES) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_g, (lds_void_ptr)dst, 16, o, 0, 0, 0);
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_q, (lds_void_ptr)dst, 16, o, 0, 0, 0);
            }
            st_fill = (st_fill == 2) ? 0 : st_fill + 1;
            if (++kt_next == ktiles) { kt_next = 0; v_next += gridDim.x; }
        };
        const int steps = n_tiles * ktiles;
        issue();
        if (steps > 1) { issue(); dma_wait<NDMA>(); } else dma_wait<0>();
        __builtin_amdgcn_s_barrier();                              // step 0 visible
        for (int s = 0; s < steps; ++s) {
            // the stage of step s+2 was last read in step s-1, which every consumer left through the previous barrier
            if (s + 2 < steps) { issue(); dma_wait<NDMA>(); } else dma_wait<0>();     // step s+1 has landed
            __builtin_amdgcn_s_barrier();
        }
        return;
    }
    // ---- consumer waves 0..7: fragments + MFMAs + the tile's stores ----
    const int wm = wave >> 2, wn = wave & 3;
    const int frag_off = (lane & 15) * 64 + (((lane >> 4) ^ ((lane & 15) >> 1)) << 3);   // first half; second half = ^ 32
    __builtin_amdgcn_s_barrier();
    int st_cur = 0;
    for (int v = blockIdx.x; v < vgrid; v += gridDim.x) {
        int tm, tn;
        if (!xcd_tile_map(v, tiles_m, tiles_n, tm, tn)) continue;
        f32x4_t acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < ktiles; ++kt) {
            const uint16_t* sa = smem + st_cur * STAGE;
            const uint16_t* sb = sa + A_ELEMS;
            bf16x8_t a0[4], a1[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a0[i] = *reinterpret_cast<const bf16x8_t*>(sa + (wm * 64 + i * 16) * 64 + frag_off);
                a1[i] = *reinterpret_cast<const bf16x8_t*>(sa + (wm * 64 + i * 16) * 64 + (frag_off ^ 32));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(sb + (wn * 64 + j * 16) * 64 + frag_off);
                const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(sb + (wn * 64 + j * 16) * 64 + (frag_off ^ 32));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0, acc[i][j], 0, 0, 0);
                    if (NPROD == 3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b1, acc[i][j], 0, 0, 0);   // hi . lo
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b0, acc[i][j], 0, 0, 0);   // lo . hi
                    } else {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1, acc[i][j], 0, 0, 0);   // next 32 k
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // my reads of this stage are complete before it can be refilled
            __builtin_amdgcn_s_barrier();
            st_cur = (st_cur == 2) ? 0 : st_cur + 1;
        }
        if constexpr (std::is_same_v<EPI, PairTopk>) {
            pairdist_epilogue_topk(acc, tm * TM, tn * TN, wm * 64 + (lane >> 4) * 4, wn * 64 + (lane & 15), gsq, qsq, ng, nq, metric, blend);
        } else if constexpr (std::is_same_v<EPI, PairGate>) {
            if ((ng & 31) == 0 && (tm + 1) * TM <= ng && (tn + 1) * TN <= nq)
                pairdist_epilogue_lines(acc, tm * TM + wm * 64, tn * TN + wn * 64, lane, gsq, qsq, ng, metric, out,
                                        reinterpret_cast<char*>(smem + 3 * STAGE) + wave * PAIR_STRIP_BYTES);
            else
                pairdist_epilogue<4, 4>(acc, tm * TM, tn * TN, wm * 64 + (lane >> 4) * 4, wn * 64 + (lane & 15), gsq, qsq, ng, nq, metric, out,
                                        PairBlend{nullptr, nullptr, nullptr, nullptr, 0});
        } else {
            if (!blend.on && (ng & 31) == 0 && (tm + 1) * TM <= ng && (tn + 1) * TN <= nq)
                pairdist_epilogue_lines(acc, tm * TM + wm * 64, tn * TN + wn * 64, lane, gsq, qsq, ng, metric, out,
                                        reinterpret_cast<char*>(smem + 3 * STAGE) + wave * PAIR_STRIP_BYTES);
            else
                pairdist_epilogue<4, 4>(acc, tm * TM, tn * TN, wm * 64 + (lane >> 4) * 4, wn * 64 + (lane & 15), gsq, qsq, ng, nq, metric, out, blend);
        }
    }
}

}  // namespace dali

using namespace dali;

extern "C" int dali_l2norm_rows(dali_ctx* ctx, void* stream, const float* x, int n, int d, float eps, float* y,
                                float* norms) {
    DALI_REQUIRE(ctx && x && y, "dali_l2norm_rows: null argument");
    DALI_REQUIRE(n >= 0 && d > 0, "dali_l2norm_rows: bad shape n=%d d=%d", n, d);
    if (n == 0) return DALI_OK;
    hipLaunchKernelGGL(rows_prep_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, n, d, (d + 3) & ~3, 1, eps,
                       (uint16_t*)nullptr, 0, (float*)nullptr, y, norms);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_l2norm_rows_bwd(dali_ctx* ctx, void* stream, const float* x, const float* dy, int n, int d,
                                    float eps, float* dx) {
    DALI_REQUIRE(ctx && x && dy && dx, "dali_l2norm_rows_bwd: null argument");
    DALI_REQUIRE(n >= 0 && d > 0, "dali_l2norm_rows_bwd: bad shape n=%d d=%d", n, d);
    if (n == 0) return DALI_OK;
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, dy, n, d, eps, dx);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

// operand image geometry (rows_prep_kernel): columns padded to Kp, `pitch` bf16 elements per row
static inline int pair_kp(int d, bool split) { return split ? (d + 31) & ~31 : (d + 63) & ~63; }
static inline int pair_pitch(int d, bool split) { return split ? 2 * pair_kp(d, true) : pair_kp(d, false); }

// rows of an operand image the DMA kernel addresses with its 32-bit buffer offsets
static inline bool pair_dma_fits(int n, int pitch) { return (long long)n * pitch * 2 < 0x7ff00000ll; }

// epi: what the DMA kernel does with a finished tile (PairBlend: store; PairGate: store if the gate word is set; PairTopk: select)
template <class EPI>
static int launch_pairdist_dma(int num_cus, hipStream_t st, const uint16_t* g_img, const float* gsq, const uint16_t* q_img, const float* qsq, int nq, int ng,
                               int d, int metric, bool split, float* out, EPI epi) {
    const int Kp = pair_kp(d, split), pitch = pair_pitch(d, split);
    const int tm2 = (ng + 127) / 128, tn2 = (nq + 255) / 256;
    const int grid2 = xcd_tile_grid(tm2, tn2);
    const int lds = 3 * (128 + 256) * 64 * 2 + 8 * PAIR_STRIP_BYTES;         // 3 stages x 48 KiB + the consumers' store strips = 160 KiB
    DALI_ONCE_PER_DEVICE({
        DALI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pairdist_dma_kernel<3, EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        DALI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pairdist_dma_kernel<1, EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    });
    const int cap = num_cus / 8 * 8, grid = grid2 < cap ? grid2 : cap;          // persistent: one workgroup per CU (144 KiB of LDS each)
    const int kt = split ? Kp / 32 : Kp / 64;
    if (split) hipLaunchKernelGGL((pairdist_dma_kernel<3, EPI>), dim3(grid), dim3(1024), lds, st, g_img, q_img, gsq, qsq, ng, nq, pitch, kt, metric, out, tm2, tn2, grid2, epi);
    else hipLaunchKernelGGL((pairdist_dma_kernel<1, EPI>), dim3(grid), dim3(1024), lds, st, g_img, q_img, gsq, qsq, ng, nq, pitch, kt, metric, out, tm2, tn2, grid2, epi);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

static int launch_pairdist(int num_cus, hipStream_t st, const uint16_t* g_img, const float* gsq, const uint16_t* q_img, const float* qsq, int nq, int ng,
                           int d, int metric, bool split, float* out, PairBlend blend = PairBlend{nullptr, nullptr, nullptr, nullptr, 0}) {
    const int Kp = pair_kp(d, split), pitch = pair_pitch(d, split);
    if (pair_dma_fits(ng, pitch) && pair_dma_fits(nq, pitch))
        return launch_pairdist_dma(num_cus, st, g_img, gsq, q_img, qsq, nq, ng, d, metric, split, out, blend);
    const int tiles_m = (ng + 127) / 128, tiles_n = (nq + 127) / 128;
    const int grid = xcd_tile_grid(tiles_m, tiles_n);
    if (split) {
        using Cfg = PairCfg<3>::type;
        DALI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pairdist_kernel<3>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES));
        hipLaunchKernelGGL(pairdist_kernel<3>, dim3(grid), dim3(256), Cfg::LDS_BYTES, st, g_img, q_img, gsq, qsq, ng, nq, Kp, metric, out, tiles_m, tiles_n, blend);
    } else {
        using Cfg = PairCfg<1>::type;
        hipLaunchKernelGGL(pairdist_kernel<1>, dim3(grid), dim3(256), Cfg::LDS_BYTES, st, g_img, q_img, gsq, qsq, ng, nq, Kp, metric, out, tiles_m, tiles_n, blend);
    }
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" size_t dali_pairdist_operand_bytes(int n, int d, int precision) {
    if (n <= 0 || d <= 0) return 0;
    return (size_t)n * pair_pitch(d, precision == DALI_PREC_BF16X3) * sizeof(uint16_t);
}

extern "C" int dali_pairdist_prepare(dali_ctx* ctx, void* stream, const float* X, int n, int d, int normalize, int precision,
                                     void* image, float* sq) {
    DALI_REQUIRE(ctx && X && image && sq, "dali_pairdist_prepare: null argument");
    DALI_REQUIRE(n >= 0 && d > 0, "dali_pairdist_prepare: bad shape n=%d d=%d", n, d);
    DALI_REQUIRE(precision == DALI_PREC_BF16X3 || precision == DALI_PREC_BF16, "dali_pairdist_prepare: bad precision %d", precision);
    DALI_REQUIRE((reinterpret_cast<uintptr_t>(image) & 15) == 0, "dali_pairdist_prepare: the operand image must be 16-byte aligned");
    if (n == 0) return DALI_OK;
    const bool split = precision == DALI_PREC_BF16X3;
    hipLaunchKernelGGL(rows_prep_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, X, n, d, pair_kp(d, split), normalize, 0.0f,
                       static_cast<uint16_t*>(image), split ? 3 : 1, sq, (float*)nullptr, (float*)nullptr);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}

extern "C" int dali_pairdist_prepared(dali_ctx* ctx, void* stream, const void* q_image, const float* q_sq, const void* g_image,
                                      const float* g_sq, int nq, int ng, int d, int metric, int precision, float* out) {
    DALI_REQUIRE(ctx && q_image && g_image && q_sq && g_sq && out, "dali_pairdist_prepared: null argument");
    DALI_REQUIRE(nq >= 0 && ng >= 0 && d > 0, "dali_pairdist_prepared: bad shape nq=%d ng=%d d=%d", nq, ng, d);
    DALI_REQUIRE(metric == DALI_METRIC_COSINE || metric == DALI_METRIC_L2SQ || metric == DALI_METRIC_DOT, "dali_pairdist_prepared: bad metric %d", metric);
    DALI_REQUIRE(precision == DALI_PREC_BF16X3 || precision == DALI_PREC_BF16, "dali_pairdist_prepared: bad precision %d", precision);
    DALI_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "dali_pairdist_prepared: out must be 16-byte aligned");
    if (nq == 0 || ng == 0) return DALI_OK;
    return launch_pairdist(ctx->num_cus, (hipStream_t)stream, static_cast<const uint16_t*>(g_image), g_sq, static_cast<const uint16_t*>(q_image), q_sq, nq, ng, d,
                           metric, precision == DALI_PREC_BF16X3, out);
}

// The distance kernel as topk.hip drives it (kernels.h): operand images whose row counts fit the DMA kernel's offsets (pairdist_dma_max_rows).
namespace dali {
int pairdist_dma_max_rows(int d, bool split) { return (int)((0x7ff00000ll - 1) / ((long long)pair_pitch(d, split) * 2)); }
int launch_pairdist_matrix(int num_cus, hipStream_t st, const uint16_t* g_img, const float* gsq, const uint16_t* q_img, const float* qsq, int nq, int ng,
                           int d, int metric, bool split, float* out, const int* gate) {
    if (!gate) return launch_pairdist(num_cus, st, g_img, gsq, q_img, qsq, nq, ng, d, metric, split, out);
    return launch_pairdist_dma(num_cus, st, g_img, gsq, q_img, qsq, nq, ng, d, metric, split, out, PairGate{gate});
}
int launch_pairdist_select(int num_cus, hipStream_t st, const uint16_t* g_img, const float* gsq, const uint16_t* q_img, const float* qsq, int nq, int ng,
                           int d, int metric, bool split, const PairTopk& sel) {
    return launch_pairdist_dma(num_cus, st, g_img, gsq, q_img, qsq, nq, ng, d, metric, split, (float*)nullptr, sel);
}
}  // namespace dali

// ------------------------------------------------------------------------------------------------
// Small similarity GEMMs (the loss heads' fn @ centers^T, fn @ proxies^T, dS @ centers: 256 x 751 .. 2253 x 2048, losses.py:62, :277) on the fp32
// MFMA: out[m][n] = sum_k Q[m][k] G[n][k], exact fp32 products, no operand pre-pass.  The persistent distance kernel gives a 128 x 256 tile
// to one CU: 6-18 of the 256 CUs worked on these, 46 us per launch + two 8 us operand pre-passes.  Here: one workgroup per 32 x 32 tile
// (192-568 workgroups), its 4 waves split K in 16-deep steps (lane (i, h) takes k = k16 + 8h + t: two 16-byte loads per operand), D steps of
// loads in flight ahead of each wave's MFMA chain, partial tiles summed through LDS in a fixed order.  Rows past nq / ng are clamped onto the
// last row and masked at the store; k-steps past a wave's share are clamped and multiplied by zero; the K % 16 tail is one masked step.
// (Rows are read in 16-byte pieces at 4-byte alignment when ldq / ldg is no multiple of 4 -- d = 751 in the heads' backward: global loads of any
//  width need dword alignment only on gfx950; tests/test_gpu_eval.py covers that shape bit-exactly.)
// ------------------------------------------------------------------------------------------------
namespace dali {
template <int D>
__global__ __launch_bounds__(256) void dot_small_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ G, int ldg, int nq, int ng, int K,
                                                        float* __restrict__ out, int ldo) {
    __shared__ float red[3][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const float* ap = Q + (size_t)min(m0 + i, nq - 1) * ldq + 8 * h;
    const float* bp = G + (size_t)min(n0 + i, ng - 1) * ldg + 8 * h;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nfull = K >> 4;                              // whole 16-deep steps; wave w takes steps w, w + 4, ...
    const int ns = (nfull + 3) >> 2;                       // turns per wave (the last may be past a wave's share: clamped, weight 0)
    struct Raw { float4 a0, a1, b0, b1; };
    auto load = [&](int j, Raw& st) {
        const int sc = min(wave + 4 * j, nfull - 1);
        st.a0 = *reinterpret_cast<const float4*>(ap + 16 * sc); st.a1 = *reinterpret_cast<const float4*>(ap + 16 * sc + 4);
        st.b0 = *reinterpret_cast<const float4*>(bp + 16 * sc); st.b1 = *reinterpret_cast<const float4*>(bp + 16 * sc + 4);
    };
    auto fma = [&](const Raw& st, int j) {
        const float z = wave + 4 * j < nfull ? 1.f : 0.f;
        const float a[8] = {st.a0.x * z, st.a0.y * z, st.a0.z * z, st.a0.w * z, st.a1.x * z, st.a1.y * z, st.a1.z * z, st.a1.w * z};
        const float b[8] = {st.b0.x, st.b0.y, st.b0.z, st.b0.w, st.b1.x, st.b1.y, st.b1.z, st.b1.w};
#pragma unroll
        for (int t = 0; t < 8; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
    };
    if (nfull > 0) {
        Raw ring[D];
#pragma unroll
        for (int d = 0; d < D; ++d) load(d, ring[d]);
        for (int j0 = 0; j0 < ns; j0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                fma(ring[d], j0 + d);
                load(j0 + d + D, ring[d]);
            }
        }
    }
    if ((K & 15) && wave == 0) {                           // the ragged end of K: one masked step
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = 16 * nfull + 8 * h + t;          // (ap / bp already carry the 8h)
            const float a = k < K ? ap[16 * nfull + t] : 0.f, b = k < K ? bp[16 * nfull + t] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
        const int n = n0 + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float v = ((acc[r] + red[0][r][lane]) + red[1][r][lane]) + red[2][r][lane];
            if (m < nq && n < ng) out[(size_t)m * ldo + n] = v;
        }
    }
}
// does dali_pairdist take this problem on the small kernel?  plain dot products at fp32 grade whose 128 x 256 tiles would occupy at most a
// quarter of the CUs (DALI_PAIRDIST_SMALL=0: always the persistent kernel, for A/B)
static bool dot_small_applies(int num_cus, int nq, int ng, int d, int metric, int precision, int normalize) {
    if (metric != DALI_METRIC_DOT || normalize || precision != DALI_PREC_BF16X3 || d < 16) return false;
    const long long big_tiles = (long long)((nq + 127) / 128) * ((ng + 255) / 256);
    return big_tiles * 4 <= num_cus && DALI_ENV_INT("DALI_PAIRDIST_SMALL", 1) != 0;
}
static int launch_dot_small(hipStream_t st, const float* Q, const float* G, int nq, int ng, int d, float* out) {
    const dim3 grid((ng + 31) / 32, (nq + 31) / 32);
    const int turns = ((d >> 4) + 3) >> 2;
    if (turns >= 8) hipLaunchKernelGGL(dot_small_kernel<8>, grid, dim3(256), 0, st, Q, d, G, d, nq, ng, d, out, ng);
    else if (turns >= 4) hipLaunchKernelGGL(dot_small_kernel<4>, grid, dim3(256), 0, st, Q, d, G, d, nq, ng, d, out, ng);
    else hipLaunchKernelGGL(dot_small_kernel<2>, grid, dim3(256), 0, st, Q, d, G, d, nq, ng, d, out, ng);
    DALI_LAUNCH_CHECK();
    return DALI_OK;
}
}  // namespace dali

// gallery image, query image and the squared norms in the context workspace
static int prepare_both(dali_ctx* ctx, void* stream, const float* Q, const float* G, int nq, int ng, int d, int precision, int normalize,
                        uint16_t*& g_img, uint16_t*& q_img, float*& sq) {
    const size_t g_bytes = align_up(dali_pairdist_operand_bytes(ng, d, precision), 256);
    const size_t q_bytes = align_up(dali_pairdist_operand_bytes(nq, d, precision), 256);
    char* ws = static_cast<char*>(workspace(ctx, g_bytes + q_bytes + align_up(((size_t)nq + ng) * sizeof(float), 256)));
    if (!ws) return DALI_ERR_NOMEM;
    g_img = reinterpret_cast<uint16_t*>(ws);
    q_img = reinterpret_cast<uint16_t*>(ws + g_bytes);
    sq = reinterpret_cast<float*>(ws + g_bytes + q_bytes);
    int rc = dali_pairdist_prepare(ctx, stream, G, ng, d, normalize, precision, g_img, sq);          // gallery rows first
    if (rc != DALI_OK) return rc;
    return dali_pairdist_prepare(ctx, stream, Q, nq, d, normalize, precision, q_img, sq + ng);
}

extern "C" int dali_pairdist(dali_ctx* ctx, void* stream, const float* Q, const float* G, int nq, int ng, int d,
                             int metric, int precision, int normalize, float* out) {
    DALI_REQUIRE(ctx && Q && G && out, "dali_pairdist: null argument");
    DALI_REQUIRE(nq >= 0 && ng >= 0 && d > 0, "dali_pairdist: bad shape nq=%d ng=%d d=%d", nq, ng, d);
    DALI_REQUIRE(metric == DALI_METRIC_COSINE || metric == DALI_METRIC_L2SQ || metric == DALI_METRIC_DOT, "dali_pairdist: bad metric %d", metric);
    DALI_REQUIRE(precision == DALI_PREC_BF16X3 || precision == DALI_PREC_BF16, "dali_pairdist: bad precision %d", precision);
    DALI_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "dali_pairdist: out must be 16-byte aligned");
    if (nq == 0 || ng == 0) return DALI_OK;
    if (dot_small_applies(ctx->num_cus, nq, ng, d, metric, precision, normalize)) return launch_dot_small((hipStream_t)stream, Q, G, nq, ng, d, out);
    uint16_t *g_img, *q_img;
    float* sq;
    const int rc = prepare_both(ctx, stream, Q, G, nq, ng, d, precision, normalize, g_img, q_img, sq);
    if (rc != DALI_OK) return rc;
    return launch_pairdist(ctx->num_cus, (hipStream_t)stream, g_img, sq, q_img, sq + ng, nq, ng, d, metric, precision == DALI_PREC_BF16X3, out);
}

extern "C" int dali_pairdist_blend(dali_ctx* ctx, void* stream, const float* Q, const float* G, int nq, int ng, int d,
                                   int precision, int normalize, const float* q_mag_prev, const float* g_mag_prev,
                                   const float* q_mag, const float* g_mag, float* inout) {
    DALI_REQUIRE(ctx && Q && G && inout, "dali_pairdist_blend: null argument");
    DALI_REQUIRE(nq >= 0 && ng >= 0 && d > 0, "dali_pairdist_blend: bad shape nq=%d ng=%d d=%d", nq, ng, d);
    DALI_REQUIRE(precision == DALI_PREC_BF16X3 || precision == DALI_PREC_BF16, "dali_pairdist_blend: bad precision %d", precision);
    DALI_REQUIRE((q_mag_prev == nullptr) == (g_mag_prev == nullptr) && (q_mag == nullptr) == (g_mag == nullptr) &&
                 (q_mag_prev == nullptr) == (q_mag == nullptr),
                 "dali_pairdist_blend: the four magnitude vectors must be all set or all null");
    DALI_REQUIRE((reinterpret_cast<uintptr_t>(inout) & 15) == 0, "dali_pairdist_blend: inout must be 16-byte aligned");
    if (nq == 0 || ng == 0) return DALI_OK;
    uint16_t *g_img, *q_img;
    float* sq;
    const int rc = prepare_both(ctx, stream, Q, G, nq, ng, d, precision, normalize, g_img, q_img, sq);
    if (rc != DALI_OK) return rc;
    return launch_pairdist(ctx->num_cus, (hipStream_t)stream, g_img, sq, q_img, sq + ng, nq, ng, d, DALI_METRIC_COSINE, precision == DALI_PREC_BF16X3, inout,
                           PairBlend{q_mag_prev, g_mag_prev, q_mag, g_mag, 1});
}

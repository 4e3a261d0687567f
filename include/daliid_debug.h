/* daliid_debug.h -- diagnostic entry points of libdaliid_hip.so.  NOT part of the drop-in surface (include/daliid.h):
 * nothing under daliid_amd/ binds them; scripts/ (timing, in-kernel stamps) and tests do, through ctypes: the split plan and the split-K
 * reduce alone, the net plan's backward block by block, and the pieces of the plan that have no single-op entry point in daliid.h (the stem
 * weight gradient on the packed image, the head-pool backward with its ReLU gate).  Named intermediates of a plan (packed image and weight
 * images included) are read through dali_resnet_debug_tensor (daliid.h).
 * Declared here so that the shared library exports nothing that no header names (tests/test_abi.py compares the
 * two headers with `nm -D` of the library).
 */
#ifndef DALIID_DEBUG_H
#define DALIID_DEBUG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the DALI_* switches that select a reference path (DALI_TRAIN_STEM, DALI_EVAL_STEM, DALI_PAIRDIST_SMALL; daliid_amd/csrc/common.h)
 * are re-read from the environment at their next use, so that one process can run both paths back to back */
int dali_debug_reload_env(void);

/* device buffer of 12 x uint64 per workgroup that the convolution / weight-gradient kernels fill with s_memrealtime
 * stamps (100 MHz); null switches the stamps off (scripts/conv_block_timeline.py) */
int dali_debug_set_conv_stamps(void* dev_ptr);

/* the split count the weight-gradient plan picks for a layer (returned as the status value, >= 1) */
int dali_debug_wgrad_splits(int Cm, int Ntot, int P, int taps, int halo_w);

/* the split-K reduce alone: out[e] (+)= sum_k partial[k][e], fixed order (tests/test_gpu_conv.py, scripts/bench_reduce.py) */
int dali_debug_splitk_reduce(void* stream, const float* partial, float* out, long long elems, int splits, int accumulate);

/* the ResNet plan's backward ONE bottleneck at a time (last block first: that call also runs the neck + head backward from d_emb; after
 * block 0, block = -1 runs the stem), so that a test can read the gradient entering every block (`grad_cur` of dali_resnet_debug_tensor); same launches
 * in the same order as dali_resnet_backward (tests/test_gpu_resnet_blocks.py, the batch-256 composition check) */
struct dali_resnet;
int dali_debug_resnet_backward_block(struct dali_resnet* net, void* stream, const float* d_emb, int block);

/* the ViT plan's backward ONE piece at a time: block = depth runs the head only (neck, final LayerNorm on the cls rows, memset + scatter of
 * their gradient into the token gradient), depth-1 .. 0 runs that one transformer block, -1 the token tail (assemble_tokens_bwd, the patch
 * embedding's weight gradient, sie_grad).  The same launches in the same order as dali_vit_backward_stages: both call the same three helpers
 * (tests/test_gpu_vit_plan.py).  d_feat is read by the head call only */
struct dali_vit;
int dali_debug_vit_backward_block(struct dali_vit* net, void* stream, const float* d_feat, int block);
/* device pointer and byte size of a named arena tensor of a bound ViT plan, valid after a forward: patches, pe, x0, cls_rows, gf, dgf, dcls_rows,
 * fin.mean, fin.rstd, neck.mean, neck.invstd, dp_rows, wbf16, grad_cur (the token gradient between two pieces of the backward), dpe (the patch
 * rows of it, as the token tail hands them to the patch weight gradient), block<i>.{h1,qkv,att,x_mid,h2,pre1,act1,x_out,lse,n1.mean,n1.rstd,
 * n2.mean,n2.rstd} and block<i>.{qkv,proj,fc1,fc2}.{w,wt}.  DALI_ERR_INVALID for an unknown name and for one the plan did not reserve (wt,
 * dp_rows, grad_cur, dpe of an eval-only plan) */
int dali_debug_vit_tensor(const struct dali_vit* net, const char* name, void** ptr, int64_t* bytes);

/* pieces that only the net plan reaches, on their own (tests/test_gpu_plan_only.py) */
struct dali_ctx;
/* the stem weight gradient as the plan's backward runs it: pack the image, the split plan of (Cout, 224, P, taps 7), the weight-gradient GEMM on
 * the packed image with the plan's own gather geometry, unpack.  images fp32 [N][3][H][W], d_raw0 bf16 [N][H/2][W/2][Cout] -> dw fp32 [Cout][7][7][3];
 * H % 32 == 0, W % 16 == 0, Cout 32 or 64 (dali_resnet_create's rules); buffers from the context workspace */
int dali_debug_stem_wgrad(struct dali_ctx* ctx, void* stream, const float* images, const unsigned short* d_raw0, int N, int H, int W, int Cout, float* dw);
/* dali_head_pool_bwd with the ReLU mask bits of the tensor the gradient belongs to (bit e & 7 of byte e >> 3, e = pixel * C + c): the store
 * forms dz = dy * (y > 0), as in the plan's backward */
int dali_debug_head_pool_bwd_masked(struct dali_ctx* ctx, void* stream, const float* df, const short* arg, int n, int hw, int C, int mode,
                                    const unsigned char* ybits, unsigned short* dx);

#ifdef __cplusplus
}
#endif
#endif

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

/* Which entries of the kernel table (daliid_amd/csrc/conv.hip, GemmKernel::name) a forward / data-gradient / linear-layer GEMM is launched on:
 * the launcher's parity split of a stride-2 data gradient and the kernel chooser, no launch and no HIP call, so it runs without a GPU.
 * Problem: Cm output channels x P pixels; the geometry as dali_conv2d_fwd (mode 0: h x wd input images of ck channels) or dali_conv2d_dgrad
 * (mode 1: h x wd images of dx, ck channels of dy) takes it, a linear layer of `rows` rows as h = wd = r = s = stride = 1, pad = 0, P = rows,
 * ck = K; flags: what the launch carries; ck1 > 0: a second operand tensor (IGemmArgs::X2: ck1 channels in the first, x_rep weight images);
 * n_cus: the CU count the persistent kernel's grid is sized by (a multiple of 8).  The residual is a tensor of its own (not accumulated in
 * place), and the launcher's check of the statistics slab is not run.
 * -> DALI_OK and the names in `out`, joined by '+' when the split makes several launches; the chooser's refusal status (message:
 * dali_last_error) otherwise */
enum {
    DALI_DEBUG_CONV_STATS = 1,      /* BatchNorm statistics epilogue */
    DALI_DEBUG_CONV_FUSED = 2,      /* fused output stage: scale, shift, ReLU */
    DALI_DEBUG_CONV_RES = 4,        /* residual */
    DALI_DEBUG_CONV_RES_MASK = 8,   /* 1-bit gate of the residual (dali_conv2d_dgrad) */
    DALI_DEBUG_CONV_OUT_MASK = 16,  /* 1-bit gate of the output (fused stage) */
    DALI_DEBUG_CONV_BITS = 32,      /* (value > 0) bits written (fused stage) */
    DALI_DEBUG_CONV_LIN = 64        /* linear-layer extras (GELU) */
};
int dali_debug_conv_kernel_name(int Cm, int P, int h, int wd, int ck, int r, int s, int stride, int pad, int mode, int flags, int ck1, int x_rep,
                                int n_cus, char* out, int cap);

/* the split-K reduce alone: out[e] (+)= sum_k partial[k][e], fixed order (tests/test_gpu_conv.py, scripts/bench_reduce.py) */
int dali_debug_splitk_reduce(void* stream, const float* partial, float* out, long long elems, int splits, int accumulate);

/* the ResNet plan's backward ONE bottleneck at a time (last block first: that call also runs the neck + head backward from d_emb; after
 * block 0, block = -1 runs the stem), so that a test can read the gradient entering every block (`grad_cur` of dali_resnet_debug_tensor); same launches
 * in the same order as dali_resnet_backward (tests/test_gpu_resnet_blocks.py, the batch-256 composition check) */
struct dali_resnet;
int dali_debug_resnet_backward_block(struct dali_resnet* net, void* stream, const float* d_emb, int block);
/* The same call (same helper, same launches, same order) that also KEEPS the intermediates which the backward overwrites in place (d_a2 becomes
 * d_raw2 and then dx; G0 = dz^T a2 is finished inside the gradient slot): each one is copied, device to device on the same stream right after
 * the launch that produces it, into `snap` (device memory, snap_bytes long).  offsets[slot] receives the byte offset of the copy inside snap
 * (256-byte aligned), or -1 where this call does not produce that tensor.  Sizes are those of the tensor: bf16 [pixels][channels] for the
 * activations' gradients, fp32 [cout][cin] for an unfinished G0, fp32 [Cout][224] for the padded stem weight gradient.
 * DALI_ERR_INVALID when snap is too small (nothing after the tensor that did not fit is meaningful) (tests/test_gpu_resnet_plan.py) */
enum {
    DALI_SNAP_D_A2 = 0,         /* output of the [dz | a2] GEMM: the gradient of a2 */
    DALI_SNAP_D_RAW2,           /* after bn2 + ReLU backward */
    DALI_SNAP_D_A1,             /* conv2's data gradient */
    DALI_SNAP_D_RAW1,           /* after bn1 + ReLU backward */
    DALI_SNAP_D_RAWD,           /* downsample BatchNorm backward (blocks with a branch that does not run through the moments of x) */
    DALI_SNAP_DX_CONV1,         /* dx after conv1's data gradient, before the downsample branch accumulates into it (blocks with a branch) */
    DALI_SNAP_G0_CONV3,         /* dz^T a2 as the weight-gradient GEMM leaves it in conv3's gradient slot */
    DALI_SNAP_G0_DS,            /* dz^T x in the downsample convolution's slot (the net's first block: branch through the moments of x) */
    DALI_SNAP_D_RAW0,           /* block = -1: the stem's d(raw0) */
    DALI_SNAP_STEM_DW_PAD,      /* block = -1: the stem weight gradient on the padded [Cout][7][8][4] layout, before the unpack */
    DALI_SNAP_HEAD_DZ,          /* last block: the masked gradient of the last block's output, as the head pooling's backward leaves it */
    DALI_SNAP_COUNT
};
int dali_debug_resnet_backward_block_snap(struct dali_resnet* net, void* stream, const float* d_emb, int block, void* snap, int64_t snap_bytes,
                                          int64_t* offsets);

/* the ViT plan's backward ONE piece at a time: block = depth runs the head only (neck, final LayerNorm on the cls rows, memset + scatter of
 * their gradient into the token gradient), depth-1 .. 0 runs that one transformer block, -1 the token tail (assemble_tokens_bwd, the patch
 * embedding's weight gradient, sie_grad).  The same launches in the same order as dali_vit_backward_stages: both call the same three helpers
 * (tests/test_gpu_vit_plan.py).  d_feat is read by the head call only */
struct dali_vit;
int dali_debug_vit_backward_block(struct dali_vit* net, void* stream, const float* d_feat, int block);
/* device pointer and byte size of a named arena tensor of a bound ViT plan (intermediates: valid after a forward).  The names are those under
 * which dali_vit_create_ex reserves the tensors:
 *   wbf16 (the bf16 cast of the flat parameters), patches, pe, x0, patch.w, cls_rows, dcls_rows, dgf16, gf, dgf, neck.mean, neck.invstd, fin.mean,
 *   fin.rstd, scratch; block<i>.{h1,qkv,att,x_mid,h2,pre1,act1,x_out,lse,n1.mean,n1.rstd,n2.mean,n2.rstd} (qkv: the activation) and the forward
 *   weight images block<i>.{qkv,proj,fc1,fc2}.w (they lie inside wbf16);
 *   of a training plan only: patch.wt and block<i>.{qkv,proj,fc1,fc2}.wt (the transposed images), slab, partial, dp_rows, gbuf0 .. gbuf3,
 *   grad_cur (the token gradient between two pieces of the backward: the head of gbuf0) and dpe (the patch rows of it, as the token tail hands
 *   them to the patch weight gradient: the head of gbuf1);
 *   of a JPM plan: jseq, b2.{h1 .. n2.rstd as a block's}, cls2, gf2, fin2.mean, fin2.rstd, map_dev and {b1,b2}.{qkv,proj,fc1,fc2}.w (b1 works in the
 *   buffers of the idle last block: its activations are block<depth-1>.*).
 * DALI_ERR_INVALID for an unknown name and for one this plan does not hold (wt, dp_rows, grad_cur, dpe of an eval-only plan) */
int dali_debug_vit_tensor(const struct dali_vit* net, const char* name, void** ptr, int64_t* bytes);

/* The arena of a plan as a table, one entry per index 0, 1, ... (DALI_ERR_INVALID past the last): every tensor that dali_*_create_ex reserves,
 * in the order of the arena (reserved = 1: `offset` bytes from the arena's base, 256-byte aligned, `bytes` long; the reservations do not overlap
 * and their 256-aligned sizes add up to the plan's arena_bytes), and every view (reserved = 0, offset = -1): a name for storage inside a
 * reserved tensor (a weight image inside wbf16, grad_cur, dpe, the ResNet's d_raw0 and block<i>.d_raw1 inside the gradient buffers) whose
 * pointer is set later or never.  Every entry's name is what dali_resnet_debug_tensor / dali_debug_vit_tensor answers to, with these bytes; an
 * entry is listed whether or not the plan is bound (tests/test_gpu_plan_arena.py).
 * The ResNet's names (shapes: the comment above dali_resnet_debug_tensor, daliid_amd/csrc/resnet_plan.hip):
 *   wbf16, w_stem, ximg, raw0, pool0, pool_arg, bn1.{scale,shift,mean,invstd,coef}, feat, head_arg, neck.mean, neck.invstd, gbuf0;
 *   block<i>.{a1,a2,y}, .rawd (with a downsample branch), .bn{1,2,3,d}.{scale,shift,mean,invstd,coef}, .conv{1,2,3,d}.w, .in1.{mean,invstd} (an IBN
 *   block), .wcat and .shcat (where the inference forward folds conv3 + downsample into one GEMM);
 *   of a training plan only: d_raw0, dfeat, stat_partial, bwd_partial, wgrad_slab, cs_partial, stem_dw_pad, red_scratch, gbuf1 .. gbuf5,
 *   block<i>.{raw1,raw2,d_raw1,ybits,sdz}, .conv{1,2,3,d}.wt, .l3.{gram,m2,bvec,qk,wd,ut,dot} and, where the downsample branch's backward runs
 *   through the moments of x, .ld.{gram,m2,bvec,qk,wd,ut};
 *   grad_cur, which dali_resnet_debug_tensor also answers, is no entry: it moves and changes its size from block to block */
int dali_debug_resnet_arena_entry(const struct dali_resnet* net, int index, char* name, int name_cap, int64_t* offset, int64_t* bytes, int* reserved);
int dali_debug_vit_arena_entry(const struct dali_vit* net, int index, char* name, int name_cap, int64_t* offset, int64_t* bytes, int* reserved);

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

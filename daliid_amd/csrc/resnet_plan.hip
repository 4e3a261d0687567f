// resnet_plan.hip -- native executor of the ResNet-50-ReID embedding network
// (Encoders.ResNet50ReID, Encoders.py:306-351, over torchvision's ResNet-50 v1.5 bottleneck trunk).
//
// The plan owns the topology and the launch sequence (forward, backward per stage); PyTorch owns the storage:
// one flat fp32 parameter buffer, one flat fp32 gradient buffer, one flat fp32 buffer of BatchNorm running
// statistics and one byte arena for activations / bf16 weight images / scratch.  Tensor order and names follow
// torchvision's state_dict so the Python mirror exposes the reference's keys.
//
// ReID edits reproduced (Encoders.py:321-322, :334, :341-350): no ReLU after the stem BN, layer4 at stride 1,
// head = global avg-pool + global max-pool -> BatchNorm1d.
#include "kernels.h"
#include "plan_table.h"
#include "../../include/daliid_debug.h"
#include <cstring>
#include <memory>
#include <new>

using namespace dali;

namespace {

struct Conv {
    int cin, cout, r, s, stride, pad, hin, win, hout, wout;
    int64_t w_off;            // element offset of the fp32 [cout][r][s][cin] weight in the flat params
    uint16_t* w_bf16;         // [cout][r*s*cin] (arena)
    uint16_t* wt_bf16;        // [cin][r*s*cout] (arena), dgrad image
};
struct Bn {
    int C;
    int lo = 0;               // the BatchNorm covers channels [lo, C) of the coefficient arrays (an IBN block's bn1: lo = C / 2, its tensors have C - lo entries)
    int64_t g_off, b_off;     // flat params
    int64_t rm_off, rv_off;   // flat buffers
    float *scale, *shift, *mean, *invstd, *coef;   // arena, [C] each (coef [C][3])
};
// The BatchNorm behind a 1x1 convolution through the moments of the convolution's INPUT (bnlin.hip): w = the input's channels, C = the outputs'
struct LinBn {
    int w = 0, C = 0;
    bool stats = false;                                        // the forward takes the batch statistics from the moments too (else: ut for the backward only)
    float *gram = nullptr, *m2 = nullptr, *bvec = nullptr, *qk = nullptr;      // [w][w], [w], [w], [2][C]
    float *ut = nullptr, *dot = nullptr;                       // (W gram)^T [w][C] (forward -> backward); with stats: [w/32][C] scratch
    uint16_t* wd = nullptr;                                    // data-gradient image [w][C + w]: (A.W)^T beside -(W^T diag(Q) W)
};
struct Block {
    Conv c1, c2, c3, cd;
    Bn b1, b2, b3, bd;
    bool has_ds;
    int hin, win, hout, wout, cin, width, cout;
    uint8_t* ybits = nullptr;                                  // ReLU mask of y, one bit per element (dali_bn_act mask_out)
    uint16_t *x, *raw1, *a1, *raw2, *a2, *rawd, *y;           // a = relu(bn(raw)), materialised once (fused
                                                                // apply-on-load repeats the VALU work per tap and per M-tile)
    // bn3 behind conv3 through the moments of a2: conv3's raw output is never stored
    LinBn l3;
    float* sdz = nullptr;                                      // colsum(dz) [cout]
    // the downsample BatchNorm's backward through the moments of the block input x (same scheme, backward only: rawd is still what the forward
    // stores and conv3's epilogue reads): no reduce / apply passes over (dz, rawd), d_rawd is never formed
    bool lin_ds = false;
    LinBn ld;
    // inference: conv3 + the (stride-1) downsample convolution as one GEMM over [a2 | x] (dali_conv1x1_cat_act): the folded weight image and shift
    bool cat_eval = false;
    uint16_t* wcat = nullptr;
    float* shcat = nullptr;
    // IBN-a (dali_resnet_ext): bn1 = InstanceNorm2d on channels [0, c_in) | BatchNorm2d on the rest (b1, with b1.lo = c_in)
    bool ibn = false;
    int c_in = 0;
    int64_t in_g_off = 0, in_b_off = 0;                        // IN.weight / IN.bias [c_in], flat params
    float *in_mean = nullptr, *in_invstd = nullptr;            // [N][c_in], what the last forward's dali_ibn_act launch saw
    uint16_t* dbg_d_raw1 = nullptr;                            // where the last backward of this block left d(raw1) (scratch: valid until the next block runs)
};
// f(layer, its name inside the block's arena names)
template <class F> void for_each_conv(Block& b, F f) { f(b.c1, "conv1"); f(b.c2, "conv2"); f(b.c3, "conv3"); if (b.has_ds) f(b.cd, "convd"); }
template <class F> void for_each_bn(Block& b, F f) { f(b.b1, "bn1"); f(b.b2, "bn2"); f(b.b3, "bn3"); if (b.has_ds) f(b.bd, "bnd"); }

}  // namespace

struct dali_resnet : PlanTable {
    dali_ctx* ctx;
    dali_resnet_cfg cfg;
    bool eval_only = false;                  // a plan with an IBN stage: no training forward, no backward, none of the backward's buffers
    int N, H, W;
    Conv stem; Bn stem_bn; Bn neck;
    int stem_h, stem_w, pool_h, pool_w, feat_dim, head_hw;
    std::vector<Block> blocks;
    int stage_first[4], stage_last[4];       // block index ranges per layer
    // arena pointers
    uint16_t *ximg = nullptr, *raw0 = nullptr, *pool0 = nullptr, *w_stem = nullptr;
    uint8_t* pool_arg = nullptr;
    float *feat = nullptr, *emb_in = nullptr, *stat_partial = nullptr, *bwd_partial = nullptr, *wgrad_slab = nullptr, *stem_dw_pad = nullptr;
    float *dfeat = nullptr, *neck_mean = nullptr, *neck_invstd = nullptr, *cs_partial = nullptr;
    double* red_scratch = nullptr;
    int16_t* head_arg = nullptr;
    uint16_t* gbuf[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t gbuf_bytes = 0;                   // of each; they are reserved back to back: gbuf[0] heads one region of 6 * gbuf_bytes
    uint16_t* wbf16_flat = nullptr;          // bf16 cast of the whole flat parameter buffer
    // bound storages
    float *P = nullptr, *G = nullptr, *B = nullptr;
    char* arena = nullptr;
    // backward state
    uint16_t* cur_dy = nullptr;
    int64_t cur_dy_bytes = 0;
    uint16_t* dbg_d_raw0 = nullptr;          // where the last stem backward left d(raw0) (scratch: valid until the next backward runs)
    bool fwd_training = false;
    int feature_mode = DALI_FEATURE_BOTH;
    // diagnostics (dali_debug_resnet_backward_block_snap): where snap_keep copies the backward's intermediates; null in every other call
    char* snap = nullptr;
    int64_t snap_cap = 0, snap_used = 0;
    int64_t* snap_offsets = nullptr;
};

namespace {

void add_conv(dali_resnet* net, Conv& c, const std::string& name, int cin, int cout, int k, int stride, int pad, int hin, int win) {
    c.cin = cin; c.cout = cout; c.r = k; c.s = k; c.stride = stride; c.pad = pad; c.hin = hin; c.win = win;
    c.hout = (hin + 2 * pad - k) / stride + 1;
    c.wout = (win + 2 * pad - k) / stride + 1;
    c.w_off = net->add_param(name + ".weight", {cout, cin, k, k});   // logical OIHW, stored OHWI
    c.w_bf16 = nullptr; c.wt_bf16 = nullptr;
}
void add_bn(dali_resnet* net, Bn& b, const std::string& name, int C) {
    b.C = C;
    b.g_off = net->add_param(name + ".weight", {C});
    b.b_off = net->add_param(name + ".bias", {C});
    b.rm_off = net->add_buffer(name + ".running_mean", {C});
    b.rv_off = net->add_buffer(name + ".running_var", {C});
}
// IBN(planes) as bn1 of block b: IN.weight, IN.bias [C/2], then the BatchNorm half's tensors [C - C/2] (IBN-Net's module order)
void add_ibn(dali_resnet* net, Block& b, const std::string& name, int C) {
    Bn& bn = b.b1;
    b.ibn = true; b.c_in = C / 2;
    bn.C = C; bn.lo = b.c_in;
    b.in_g_off = net->add_param(name + ".IN.weight", {b.c_in});
    b.in_b_off = net->add_param(name + ".IN.bias", {b.c_in});
    bn.g_off = net->add_param(name + ".BN.weight", {C - b.c_in});
    bn.b_off = net->add_param(name + ".BN.bias", {C - b.c_in});
    bn.rm_off = net->add_buffer(name + ".BN.running_mean", {C - b.c_in});
    bn.rv_off = net->add_buffer(name + ".BN.running_var", {C - b.c_in});
}
// The arena tensors of a layer, named `name`.<field> (PlanTable::reserve: what dali_resnet_debug_tensor answers)
void reserve_bn(dali_resnet* net, Bn& b, const std::string& name) {
    net->reserve(name + ".scale", b.scale, b.C * 4); net->reserve(name + ".shift", b.shift, b.C * 4);
    net->reserve(name + ".mean", b.mean, b.C * 4); net->reserve(name + ".invstd", b.invstd, b.C * 4);
    net->reserve(name + ".coef", b.coef, b.C * 12);
}
void reserve_linbn(dali_resnet* net, LinBn& l, const Conv& c, bool stats, const std::string& name) {
    l.w = c.cin; l.C = c.cout; l.stats = stats;
    net->reserve(name + ".gram", l.gram, (size_t)l.w * l.w * 4); net->reserve(name + ".m2", l.m2, (size_t)l.w * 4);
    net->reserve(name + ".bvec", l.bvec, (size_t)l.w * 4); net->reserve(name + ".qk", l.qk, (size_t)l.C * 8);
    net->reserve(name + ".wd", l.wd, (size_t)l.w * (l.C + l.w) * 2);
    net->reserve(name + ".ut", l.ut, (size_t)l.w * l.C * 4);
    if (stats) net->reserve(name + ".dot", l.dot, (size_t)(l.w / 32) * l.C * 12);
}

// (gamma, beta) in the flat parameters, (running_mean, running_var) in the flat buffers
struct BnParams { const float *gamma, *beta; float *rm, *rv; };
BnParams bn_params(const dali_resnet* net, const Bn& b) { return {net->P + b.g_off, net->P + b.b_off, net->B + b.rm_off, net->B + b.rv_off}; }

GatherGeom conv_geom(const Conv& c, int mode) {
    GatherGeom g{};
    if (mode == 0) {
        g.Hout = c.hout; g.Wout = c.wout; g.Hin = c.hin; g.Win = c.win; g.Ck = c.cin;
    } else {
        g.Hout = c.hin; g.Wout = c.win; g.Hin = c.hout; g.Win = c.wout; g.Ck = c.cout;
    }
    g.R = c.r; g.S = c.s; g.stride = c.stride; g.pad = c.pad; g.mode = mode;
    g.pix_pitch = g.Ck; g.row_pitch = g.Win * g.Ck; g.img_pitch = (long long)g.Hin * g.Win * g.Ck;
    g.lw = g.lhw = -1;
    return g;
}

// The plan's weight-gradient GEMMs, out [Cm][R*S*Ck] = dY^T gather(X) over P pixels.  dali_resnet_create sizes the slab and the column-sum
// partials from these descriptions and run_wgrad launches from them.
struct WGradDesc { int Cm, P; GatherGeom g; };
WGradDesc conv_wgrad_desc(const dali_resnet* net, const Conv& c) { return {c.cout, net->N * c.hout * c.wout, conv_geom(c, 0)}; }    // dW = dy^T gather(x)
WGradDesc gram_desc(const dali_resnet* net, const Conv& c) { return {c.cin, net->N * c.hout * c.wout, conv_geom(c, 0)}; }            // x^T x of a 1x1 / stride 1 convolution's input
WGradDesc stem_wgrad_desc(const dali_resnet* net) { return {net->stem.cout, net->N * net->stem_h * net->stem_w, stem_geom(net->H, net->W)}; }
// colsum_out (nullable) = column sums of dy
int run_wgrad(dali_resnet* net, hipStream_t st, const WGradDesc& d, const uint16_t* dy, const uint16_t* x, float* out, float* colsum_out = nullptr) {
    WGradArgs a{};
    a.dY = dy; a.X = x; a.Cm = d.Cm; a.P = d.P; a.g = d.g;
    return launch_wgrad(st, a, WGradBufs{net->wgrad_slab, net->cs_partial, net->red_scratch}, out, 0, colsum_out);
}

}  // namespace

extern "C" int dali_resnet_create(dali_ctx* ctx, const dali_resnet_cfg* cfg, dali_resnet** out) {
    return dali_resnet_create_ex(ctx, cfg, nullptr, out);
}

extern "C" int dali_resnet_create_ex(dali_ctx* ctx, const dali_resnet_cfg* cfg, const dali_resnet_ext* ext, dali_resnet** out) {
    DALI_REQUIRE(ctx && cfg && out, "dali_resnet_create: null argument");
    DALI_REQUIRE(cfg->batch > 0 && cfg->height >= 32 && cfg->width >= 32 && cfg->height % 32 == 0 && cfg->width % 16 == 0,
                 "dali_resnet_create: bad input shape %dx%dx%d (height %% 32, width %% 16)", cfg->batch, cfg->height, cfg->width);
    DALI_REQUIRE(cfg->width_base >= 32 && cfg->width_base % 32 == 0 && cfg->width_base <= 64,
                 "dali_resnet_create: width_base must be 32 or 64 (got %d)", cfg->width_base);
    for (int i = 0; i < 4; ++i) DALI_REQUIRE(cfg->layers[i] >= 1, "dali_resnet_create: layers[%d] < 1", i);
    DALI_REQUIRE(!ext || (cfg->width_base / 2) % 8 == 0, "dali_resnet_create_ex: an IBN block's IN half (width / 2 channels) must be a multiple of 8");
    std::unique_ptr<dali_resnet> owner(new (std::nothrow) dali_resnet());
    dali_resnet* net = owner.get();
    if (!net) { set_error("dali_resnet_create: out of host memory"); return DALI_ERR_NOMEM; }
    net->ctx = ctx; net->cfg = *cfg; net->N = cfg->batch; net->H = cfg->height; net->W = cfg->width;
    const int wb = cfg->width_base;
    for (int i = 0; i < 4; ++i) net->eval_only |= ext && ext->ibn[i] != 0;
    const bool train = !net->eval_only;
    // ---- topology + parameter table (torchvision order) ----
    add_conv(net, net->stem, "conv1", 3, wb, 7, 2, 3, net->H, net->W);
    add_bn(net, net->stem_bn, "bn1", wb);
    net->stem_h = net->stem.hout; net->stem_w = net->stem.wout;
    net->pool_h = (net->stem_h + 2 - 3) / 2 + 1; net->pool_w = (net->stem_w + 2 - 3) / 2 + 1;
    int h = net->pool_h, w = net->pool_w, inpl = wb;
    const int strides[4] = {1, 2, 2, 1};              // layer4 at stride 1 (Encoders.py:321-322)
    for (int li = 0; li < 4; ++li) {
        const int planes = wb << li;
        net->stage_first[li] = (int)net->blocks.size();
        for (int bi = 0; bi < cfg->layers[li]; ++bi) {
            Block b{};
            const int st = bi == 0 ? strides[li] : 1;
            const std::string pre = "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
            b.hin = h; b.win = w; b.cin = inpl; b.width = planes; b.cout = planes * 4;
            add_conv(net, b.c1, pre + ".conv1", inpl, planes, 1, 1, 0, h, w);
            if (ext && ext->ibn[li]) add_ibn(net, b, pre + ".bn1", planes);        // (planes / 2 is a multiple of 8: width_base 32 or 64)
            else add_bn(net, b.b1, pre + ".bn1", planes);
            add_conv(net, b.c2, pre + ".conv2", planes, planes, 3, st, 1, h, w);
            add_bn(net, b.b2, pre + ".bn2", planes);
            add_conv(net, b.c3, pre + ".conv3", planes, planes * 4, 1, 1, 0, b.c2.hout, b.c2.wout);
            add_bn(net, b.b3, pre + ".bn3", planes * 4);
            b.has_ds = (bi == 0);                     // torchvision: stride != 1 or inplanes != planes*4; true for every first block
            if (b.has_ds) {
                add_conv(net, b.cd, pre + ".downsample.0", inpl, planes * 4, 1, st, 0, h, w);
                add_bn(net, b.bd, pre + ".downsample.1", planes * 4);
            }
            b.hout = b.c2.hout; b.wout = b.c2.wout;
            // bn3 through the moments of a2 in every block (bnlin.hip): width_base 32 or 64 keeps every width a multiple of 32 up to 512, and the
            // scheme pays at every width (15.71 ms per step for w <= 128 only, 15.61 for w <= 256, 15.47 for all, same box).  With a downsample
            // branch the identity enters conv3's epilogue as scale_d * rawd + shift_d (res_scale / bias) and the downsample BatchNorm keeps its own
            // two-pass backward, except where the branch is a stride-1 convolution of a narrow input (ResNet-50: layer1's, 64 -> 256 over 524288
            // pixels at batch 256): its Gram matrix costs less than the two passes, so its backward goes through the moments of x as well
            // (block_backward)
            b.lin_ds = b.has_ds && st == 1 && inpl % 32 == 0 && inpl <= 128 && net->blocks.empty();   // (first block of the net: no mask on dx)
            h = b.hout; w = b.wout; inpl = planes * 4;
            net->blocks.push_back(b);
        }
        net->stage_last[li] = (int)net->blocks.size() - 1;
    }
    net->feat_dim = inpl;
    net->head_hw = h * w;
    DALI_REQUIRE(net->head_hw < 32768, "dali_resnet_create: final map too large");
    add_bn(net, net->neck, "last_bn", net->feat_dim);

    // ---- arena layout ----
    const size_t N = net->N;
    net->reserve("wbf16", net->wbf16_flat, (size_t)net->param_elems * 2);
    net->reserve("w_stem", net->w_stem, (size_t)wb * 224 * 2);
    net->reserve("ximg", net->ximg, N * (net->H + 6) * (net->W + 8) * 4 * 2);
    const size_t raw0_bytes = N * net->stem_h * net->stem_w * wb * 2;
    net->reserve("raw0", net->raw0, raw0_bytes);
    net->view("d_raw0", net->dbg_d_raw0, raw0_bytes);
    net->reserve("pool0", net->pool0, N * net->pool_h * net->pool_w * wb * 2);
    net->reserve("pool_arg", net->pool_arg, N * net->pool_h * net->pool_w * wb);
    reserve_bn(net, net->stem_bn, "bn1");
    size_t max_act = raw0_bytes, max_stat = (size_t)igemm_conv_stat_tiles(wb, (int)N * net->stem_h * net->stem_w, 224) * wb * 2 * 4;
    int stem_qpb;
    // (an eval plan reserves what the inference forward touches and nothing else: `train` guards the rest)
    size_t max_bwd_partial = (size_t)maxpool_bn_bwd_blocks((int)N, net->stem_h, net->stem_w, wb, &stem_qpb) * wb * 2 * 4;
    // the weight-gradient slab and column-sum partials: the most any weight-gradient GEMM of the plan asks for (run_wgrad's callers)
    size_t max_slab = 0, max_cs = 256;
    auto size_wgrad = [&](const WGradDesc& d, bool colsum) {
        const WGradNeed need = wgrad_need(d.Cm, d.P, d.g, colsum);
        max_slab = std::max(max_slab, need.slab_bytes);
        max_cs = std::max(max_cs, need.colsum_floats * 4);
    };
    size_wgrad(stem_wgrad_desc(net), false);
    for (size_t bi = 0; bi < net->blocks.size(); ++bi) {
        Block& b = net->blocks[bi];
        const std::string pre = "block" + std::to_string(bi) + ".";
        const size_t pin = N * b.hin * b.win, pout = N * b.hout * b.wout;
        if (train) net->reserve(pre + "raw1", b.raw1, pin * b.width * 2);
        net->view(pre + "d_raw1", b.dbg_d_raw1, pin * b.width * 2);
        net->reserve(pre + "a1", b.a1, pin * b.width * 2);
        if (train) net->reserve(pre + "raw2", b.raw2, pout * b.width * 2);
        net->reserve(pre + "a2", b.a2, pout * b.width * 2);
        if (train) {
            reserve_linbn(net, b.l3, b.c3, true, pre + "l3");
            net->reserve(pre + "sdz", b.sdz, (size_t)b.cout * 4);
            size_wgrad(gram_desc(net, b.c3), true);
        }
        net->reserve(pre + "y", b.y, pout * b.cout * 2);
        if (train) net->reserve(pre + "ybits", b.ybits, pout * b.cout / 8);
        if (b.has_ds) net->reserve(pre + "rawd", b.rawd, pout * b.cout * 2);
        if (b.ibn) { net->reserve(pre + "in1.mean", b.in_mean, N * b.c_in * 4); net->reserve(pre + "in1.invstd", b.in_invstd, N * b.c_in * 4); }
        if (b.lin_ds && train) {
            reserve_linbn(net, b.ld, b.cd, false, pre + "ld");
            size_wgrad(gram_desc(net, b.cd), true);
        }
        // (split weight image, 2 parts: folding the scales into ONE bf16 image is a coherent 2^-9 perturbation of the weights, which moved the mAP of
        //  separated identities by 1.1e-3 against the oracle; hi + lo images are fp32-grade.  K = 2 (w + cin) <= 256: layer1's first block.)
        b.cat_eval = b.has_ds && b.cd.stride == 1 && conv_cat_act_supported(b.cout, b.width, b.cin, (int)pout, 2);
        if (b.cat_eval) { net->reserve(pre + "wcat", b.wcat, (size_t)b.cout * 2 * (b.width + b.cin) * 2); net->reserve(pre + "shcat", b.shcat, (size_t)b.cout * 4); }
        for_each_bn(b, [&](Bn& bn, const char* name) { reserve_bn(net, bn, pre + name); });
        for_each_conv(b, [&](Conv& c, const char* name) {
            const size_t w_bytes = (size_t)c.cin * c.r * c.s * c.cout * 2;
            net->view(pre + name + ".w", c.w_bf16, w_bytes);             // in the flat bf16 cast (bind)
            if (!train) return;
            net->reserve(pre + name + ".wt", c.wt_bf16, w_bytes);
            const int P = (int)N * c.hout * c.wout;
            max_stat = std::max(max_stat, (size_t)igemm_conv_stat_tiles(c.cout, P, c.r * c.s * c.cin) * c.cout * 2 * 4);
            size_wgrad(conv_wgrad_desc(net, c), &c == &b.c3);      // conv3's carries s_dz = colsum(dz)
            max_act = std::max(max_act, (size_t)P * c.cout * 2);
            max_act = std::max(max_act, N * c.hin * c.win * c.cin * 2);
            max_bwd_partial = std::max(max_bwd_partial, bn_bwd_partial_floats(P, c.cout, true) * 4);
        });
    }
    net->reserve("feat", net->feat, N * net->feat_dim * 4);
    if (train) net->reserve("dfeat", net->dfeat, N * net->feat_dim * 4);
    net->reserve("head_arg", net->head_arg, N * net->feat_dim * 2);
    net->reserve("neck.mean", net->neck_mean, net->feat_dim * 4);
    net->reserve("neck.invstd", net->neck_invstd, net->feat_dim * 4);
    if (train) {
        net->reserve("stat_partial", net->stat_partial, max_stat);
        net->reserve("bwd_partial", net->bwd_partial, max_bwd_partial);
        net->reserve("wgrad_slab", net->wgrad_slab, max_slab);
        net->reserve("cs_partial", net->cs_partial, max_cs);
        net->reserve("stem_dw_pad", net->stem_dw_pad, (size_t)wb * 224 * 4);
        net->reserve("red_scratch", net->red_scratch, reduce_scratch_bytes(net->feat_dim, 3));
        net->gbuf_bytes = align_up(max_act, 256);
        for (int i = 0; i < 6; ++i) net->reserve("gbuf" + std::to_string(i), net->gbuf[i], net->gbuf_bytes);
    } else {
        // the one forward that uses the gradient buffers' region: dali_resnet_forward_heads' pooled values, up to DALI_MAX_HEADS heads
        net->gbuf_bytes = align_up((DALI_MAX_HEADS * N * net->feat_dim * 4 + 5) / 6, 256);
        net->reserve("gbuf0", net->gbuf[0], 6 * net->gbuf_bytes);
    }
    *out = owner.release();
    return DALI_OK;
}

extern "C" int dali_resnet_destroy(dali_resnet* net) { delete net; return DALI_OK; }

extern "C" int dali_resnet_sizes(const dali_resnet* net, int64_t* param_elems, int64_t* buffer_elems, int64_t* arena_bytes,
                                 int* feat_dim, int* n_params, int* n_buffers) {
    DALI_REQUIRE(net, "dali_resnet_sizes: null net");
    return net->sizes(net->feat_dim, param_elems, buffer_elems, arena_bytes, feat_dim, n_params, n_buffers);
}

extern "C" int dali_resnet_tensor_info(const dali_resnet* net, int kind, int index, char* name, int name_cap, int64_t* offset,
                                       int64_t* numel, int* shape4, int* ndim) {
    DALI_REQUIRE(net, "dali_resnet_tensor_info: null argument");
    return net->tensor_info("dali_resnet_tensor_info", kind, index, name, name_cap, offset, numel, shape4, ndim);
}

// Stage s (0..3) covers layer(4-s); returns the flat-parameter element range whose gradients are complete once
// dali_resnet_backward has run through that stage (stage 0 also holds last_bn, stage 3 also the stem).
extern "C" int dali_resnet_stage_param_range(const dali_resnet* net, int stage, int64_t* begin, int64_t* end) {
    DALI_REQUIRE(net && begin && end && stage >= 0 && stage < 4, "dali_resnet_stage_param_range: bad argument");
    const int li = 3 - stage;
    const Block& first = net->blocks[net->stage_first[li]];
    *begin = (li == 0) ? 0 : first.c1.w_off;
    if (li == 3) *end = net->param_elems;
    else *end = net->blocks[net->stage_first[li + 1]].c1.w_off;
    return DALI_OK;
}

extern "C" int dali_resnet_bind(dali_resnet* net, float* params, float* grads, float* buffers, void* arena, size_t arena_bytes) {
    DALI_REQUIRE(net && params && buffers && arena, "dali_resnet_bind: null argument");
    DALI_REQUIRE(arena_bytes >= net->arena_bytes, "dali_resnet_bind: arena too small (%zu < %zu)", arena_bytes, net->arena_bytes);
    DALI_REQUIRE((reinterpret_cast<uintptr_t>(arena) & 255) == 0 && (reinterpret_cast<uintptr_t>(params) & 255) == 0 &&
                 (reinterpret_cast<uintptr_t>(grads) & 255) == 0 && (reinterpret_cast<uintptr_t>(buffers) & 255) == 0,
                 "dali_resnet_bind: storages must be 256-byte aligned");
    net->P = params; net->G = grads; net->B = buffers; net->arena = static_cast<char*>(arena);
    net->bind_arena(net->arena);
    // bf16 weight images alias the flat bf16 cast (same offsets as the fp32 flat buffer)
    for (auto& b : net->blocks) for_each_conv(b, [&](Conv& c, const char*) { c.w_bf16 = net->wbf16_flat + c.w_off; });
    return DALI_OK;
}

// fp32 master weights -> bf16 operand images (forward layout = flat cast; dgrad layout = per-tap transpose;
// stem = padded [64][7][8][4]); eval-mode BN coefficients from the running statistics.
extern "C" int dali_resnet_refresh_weights(dali_resnet* net, void* stream) {
    DALI_REQUIRE(net && net->P, "dali_resnet_refresh_weights: net not bound");
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_cast_bf16(st, net->P, (size_t)net->param_elems, net->wbf16_flat);
    if (rc) return rc;
    rc = launch_stem_pack_weight(st, net->P + net->stem.w_off, net->stem.cout, net->w_stem);
    if (rc) return rc;
    if (net->eval_only) {
        // no data-gradient images; the IN half of every IBN block's conv1 output stage is the identity (scale 1, shift 0): constants of the arena
        for (auto& b : net->blocks) {
            if (!b.ibn) continue;
            DALI_HIP(hipMemsetD32Async((hipDeviceptr_t)b.b1.scale, 0x3f800000, (size_t)b.c_in, st));
            DALI_HIP(hipMemsetD32Async((hipDeviceptr_t)b.b1.shift, 0, (size_t)b.c_in, st));
        }
        return DALI_OK;
    }
    std::vector<TransposeJob> jobs;                      // every conv's dgrad image [cin][r*s][cout], one launch
    for (auto& b : net->blocks) for_each_conv(b, [&](Conv& c, const char*) { jobs.push_back(TransposeJob{c.w_bf16, c.wt_bf16, c.cout, c.r * c.s, c.cin, 0}); });
    return launch_weight_transpose_batched(st, jobs.data(), (int)jobs.size());
}

namespace {

int bn_train(dali_resnet* net, hipStream_t st, Bn& b, int tiles, double count) {
    const BnParams p = bn_params(net, b);
    return launch_bn_finalize(st, net->stat_partial, tiles, b.C, count, p.gamma, p.beta, p.rm, p.rv, 0.1f, 1e-5f, b.scale, b.shift, b.mean, b.invstd,
                              net->red_scratch);
}

// conv forward: y(raw) = conv(x); in training the BN of the OUTPUT is finalised right after
int conv_bn_fwd(dali_resnet* net, hipStream_t st, const Conv& c, Bn& out_bn, const uint16_t* x, uint16_t* raw) {
    IGemmArgs a{};
    a.W = c.w_bf16; a.X = x; a.O = raw;
    a.stats = net->fwd_training ? net->stat_partial : nullptr;
    a.Cm = c.cout; a.P = net->N * c.hout * c.wout;
    a.g = conv_geom(c, 0);
    int rc = launch_igemm_conv(st, a);
    if (rc) return rc;
    if (net->fwd_training) return bn_train(net, st, out_bn, igemm_conv_stat_tiles(a.Cm, a.P, a.g.R * a.g.S * a.g.Ck), (double)a.P);
    return DALI_OK;                                          // inference: the coefficients were formed at the top of the forward (one batched launch)
}
// act = relu(bn(raw))
int bn_relu(hipStream_t st, const Bn& bn, const uint16_t* raw, size_t elems, uint16_t* act) {
    return launch_bn_act(st, raw, bn.scale, bn.shift, nullptr, nullptr, nullptr, nullptr, 1, elems, bn.C, act, nullptr);
}

// inference: act = relu(bn(conv(x))) leaves the GEMM directly -- the running-statistics coefficients are known before the convolution runs, so
// they ride in the fused output stage (IGemmArgs::out_scale / out_shift / out_relu) and neither the raw output nor a bn_act pass exists
// (getFeatures.py:56-67 forwards the whole train set this way every epoch, train_encodersKIT.py:104-110; every validate, validateModels.py:38-39)
int conv_bn_relu_eval(dali_resnet* net, hipStream_t st, const Conv& c, const Bn& bn, const uint16_t* x, uint16_t* act, int relu = 1) {
    IGemmArgs a{};
    a.W = c.w_bf16; a.X = x; a.O = act;
    a.out_scale = bn.scale; a.out_shift = bn.shift; a.out_relu = relu;
    a.Cm = c.cout; a.P = net->N * c.hout * c.wout;
    a.g = conv_geom(c, 0);
    return launch_igemm_conv(st, a);
}

int conv_wgrad(dali_resnet* net, hipStream_t st, const Conv& c, const uint16_t* x, const uint16_t* dy) {
    return run_wgrad(net, st, conv_wgrad_desc(net, c), dy, x, net->G + c.w_off);
}

// out_mask: ReLU mask of the block output this gradient belongs to (the masked gradient dz = dy * (y > 0) is what every block stores)
int conv_dgrad(dali_resnet* net, hipStream_t st, const Conv& c, const uint16_t* dy, const uint16_t* residual, uint16_t* dx,
               const uint8_t* out_mask = nullptr) {
    IGemmArgs a{};
    a.W = c.wt_bf16; a.X = dy; a.O = dx; a.Res = residual; a.out_mask = out_mask;
    a.Cm = c.cin; a.P = net->N * c.hin * c.win;
    a.g = conv_geom(c, 1);
    return launch_igemm_conv(st, a);
}

// O [P][Cm] = [X | X2] W^T, X with c1 and X2 with c2 channels per pixel, over the grid of the 1x1 convolution c: its output pixels (mode 0) or,
// as a data gradient, its input pixels (mode 1).  K = (c1 + c2) x stage.x_rep.  stage: what else the site sets (bias, residual, output stage)
int cat_gemm(dali_resnet* net, hipStream_t st, const Conv& c, int mode, const uint16_t* W, const uint16_t* X, int c1, const uint16_t* X2, int c2, int Cm,
             uint16_t* O, IGemmArgs stage = IGemmArgs{}) {
    IGemmArgs& a = stage;
    a.W = W; a.X = X; a.X2 = X2; a.Ck1 = c1; a.O = O;
    a.Cm = Cm; a.P = net->N * (mode == 0 ? c.hout * c.wout : c.hin * c.win);
    Conv cat = c;
    (mode == 0 ? cat.cin : cat.cout) = (a.x_rep ? a.x_rep : 1) * (c1 + c2);
    a.g = conv_geom(cat, mode);
    return launch_igemm_conv(st, a);
}

// Diagnostics: while dali_debug_resnet_backward_block_snap runs, keep a copy of an intermediate that the backward overwrites later (device to
// device, on the launches' own stream, right after the launch that produced it).  In every other call net->snap is null and this returns at once.
int snap_keep(dali_resnet* net, hipStream_t st, int slot, const void* src, size_t bytes) {
    if (!net->snap) return DALI_OK;
    const int64_t off = (int64_t)align_up((size_t)net->snap_used, 256);
    if (off + (int64_t)bytes > net->snap_cap) {
        set_error("dali_debug_resnet_backward_block_snap: snapshot buffer too small (slot %d needs bytes %lld .. %lld of %lld)", slot, (long long)off,
                  (long long)(off + (int64_t)bytes), (long long)net->snap_cap);
        return DALI_ERR_INVALID;
    }
    DALI_HIP(hipMemcpyAsync(net->snap + off, src, bytes, hipMemcpyDeviceToDevice, st));
    net->snap_offsets[slot] = off;
    net->snap_used = off + (int64_t)bytes;
    return DALI_OK;
}

// The moments of x, the input of the 1x1 convolution c: gram = x^T x with m2 = colsum(x) on the same GEMM; from them the batch statistics of
// bn(c(x)) (l.stats) or only Ut for the backward
int linbn_fwd(dali_resnet* net, hipStream_t st, LinBn& l, const Conv& c, Bn& bn, const uint16_t* x) {
    const WGradDesc d = gram_desc(net, c);
    int rc;
    if ((rc = run_wgrad(net, st, d, x, x, l.gram, l.m2))) return rc;
    if (!l.stats) return launch_bnlin_ut(st, c.w_bf16, l.gram, l.C, l.w, l.ut);
    const BnParams p = bn_params(net, bn);
    return launch_bnlin_stats(st, c.w_bf16, c.wt_bf16, l.gram, l.m2, l.C, l.w, (double)d.P, p.gamma, p.beta, p.rm, p.rv, 0.1f, 1e-5f, l.ut, l.dot, bn.scale,
                              bn.shift, bn.mean, bn.invstd);
}
// G0 = dz^T x into c's gradient slot (with s_dz = colsum(dz) on the GEMM when sum_dz, else s_dz is read), finished in place by the row kernel
// together with dgamma / dbeta, the data-gradient image l.wd and l.bvec
int linbn_bwd(dali_resnet* net, hipStream_t st, LinBn& l, const Conv& c, const Bn& bn, const uint16_t* dz, const uint16_t* x, float* s_dz, bool sum_dz,
              int snap_slot) {
    const WGradDesc d = conv_wgrad_desc(net, c);
    int rc;
    if ((rc = run_wgrad(net, st, d, dz, x, net->G + c.w_off, sum_dz ? s_dz : nullptr))) return rc;
    if ((rc = snap_keep(net, st, snap_slot, net->G + c.w_off, (size_t)l.C * l.w * 4))) return rc;
    const int ld = l.C + l.w;
    return launch_bnlin_bwd(st, c.w_bf16, c.wt_bf16, l.ut, l.m2, s_dz, l.C, l.w, (double)d.P, bn.scale, bn.mean, bn.invstd, net->G + c.w_off, net->G + bn.g_off,
                            net->G + bn.b_off, l.wd, l.wd + l.C, l.bvec, l.qk, ld, ld);
}

// BatchNorm (+ ReLU) backward by two passes over (g, raw): dgamma / dbeta into the gradient slots, d(raw) into out (may be g)
int bn_bwd(dali_resnet* net, hipStream_t st, const Bn& bn, const uint16_t* raw, const uint16_t* g, int relu, int P, uint16_t* out) {
    const BnBwdSide s{raw, bn.mean, bn.invstd, bn.scale, bn.shift};
    return launch_bn_bwd(st, g, nullptr, nullptr, s, nullptr, relu, P, bn.C, net->bwd_partial, bn.coef, nullptr, net->G + bn.g_off, net->G + bn.b_off,
                         nullptr, nullptr, out, nullptr, nullptr, net->red_scratch);
}

uint16_t* next_gbuf(dali_resnet* net, const uint16_t* avoid0, const uint16_t* avoid1 = nullptr, const uint16_t* avoid2 = nullptr,
                    const uint16_t* avoid3 = nullptr) {
    for (int i = 0; i < 6; ++i) {
        uint16_t* g = net->gbuf[i];
        if (g != avoid0 && g != avoid1 && g != avoid2 && g != avoid3) return g;
    }
    return nullptr;
}

// conv1 -> bn1 -> (no ReLU) -> maxpool
int stem_forward(dali_resnet* net, hipStream_t st, const float* images, bool tr) {
    const Conv& c = net->stem;
    Bn& bn = net->stem_bn;
    int rc;
    if ((rc = launch_stem_pack_image(st, images, net->N, net->H, net->W, net->ximg))) return rc;
    // inference: one launch, the convolution's output never stored (stem.hip); bn1 acts on the fp32 accumulators
    if (!tr && stem_fused_supported(net->N, net->H, net->W, c.cout))
        return launch_stem_conv_bn_pool(st, net->ximg, net->w_stem, bn.scale, bn.shift, net->N, net->H, net->W, net->pool0);
    if (tr && stem_train_supported(net->N, net->H, net->W, c.cout)) {
        // training: raw0 + the statistics' partial sums from the patch kernel (stem.hip), 256-pixel tiles as the implicit-GEMM kernel's slab
        if ((rc = launch_stem_conv_stats(st, net->ximg, net->w_stem, net->N, net->H, net->W, net->raw0, net->stat_partial))) return rc;
        if ((rc = bn_train(net, st, bn, stem_train_tiles(net->N, net->H), (double)net->N * net->stem_h * net->stem_w))) return rc;
    } else {
        IGemmArgs a{};
        a.W = net->w_stem; a.X = net->ximg; a.O = net->raw0;
        a.stats = tr ? net->stat_partial : nullptr;
        a.Cm = c.cout; a.P = net->N * net->stem_h * net->stem_w;
        a.g = stem_geom(net->H, net->W);
        if ((rc = launch_igemm_conv(st, a))) return rc;
        if (tr && (rc = bn_train(net, st, bn, igemm_conv_stat_tiles(a.Cm, a.P, 224), (double)a.P))) return rc;
    }
    return launch_maxpool_bn_fwd(st, net->raw0, bn.scale, bn.shift, net->N, net->stem_h, net->stem_w, c.cout, net->pool0, net->pool_arg);
}

// one bottleneck: x -> b.y
int block_forward(dali_resnet* net, hipStream_t st, Block& b, const uint16_t* x, bool tr) {
    int rc;
    b.x = const_cast<uint16_t*>(x);
    if (!tr && b.ibn) {
        // IBN-a: the instance statistics of conv1's output are not known before it runs, so a1 leaves the output stage without the ReLU (identity on
        // the IN half, bn1.BN's running-statistics coefficients on the rest) and one launch normalises the IN half and applies the ReLU in place
        // (rounding and ReLU commute: the BN half is bit for bit what conv_bn_relu_eval gives)
        if ((rc = conv_bn_relu_eval(net, st, b.c1, b.b1, x, b.a1, 0))) return rc;
        if ((rc = launch_ibn_act(st, b.a1, net->N, b.hin * b.win, b.width, b.c_in, net->P + b.in_g_off, net->P + b.in_b_off, 1e-5f, 1, b.a1, b.in_mean,
                                 b.in_invstd))) return rc;
        if ((rc = conv_bn_relu_eval(net, st, b.c2, b.b2, b.a1, b.a2))) return rc;
    } else if (!tr) {
        if ((rc = conv_bn_relu_eval(net, st, b.c1, b.b1, x, b.a1))) return rc;
        if ((rc = conv_bn_relu_eval(net, st, b.c2, b.b2, b.a1, b.a2))) return rc;
    } else {
        if ((rc = conv_bn_fwd(net, st, b.c1, b.b1, x, b.raw1))) return rc;
        if ((rc = bn_relu(st, b.b1, b.raw1, (size_t)net->N * b.hin * b.win * b.width, b.a1))) return rc;
        if ((rc = conv_bn_fwd(net, st, b.c2, b.b2, b.a1, b.raw2))) return rc;
        if ((rc = bn_relu(st, b.b2, b.raw2, (size_t)net->N * b.hout * b.wout * b.width, b.a2))) return rc;
        // bn3's batch statistics from the moments of a2 (bnlin.hip), then conv3 writes y = relu(bn3(conv3(a2)) + x) and its ReLU mask itself
        if ((rc = linbn_fwd(net, st, b.l3, b.c3, b.b3, b.a2))) return rc;
    }
    if (!tr && b.cat_eval) {
        // inference, stride-1 downsample branch: y = relu([a2 | x] [s3.W3 | sd.Wd]^T + shift3 + shift_d) in one launch: no raw branch
        // output, no residual read (the scales ride in a split hi + lo weight image: fp32-grade weights, mirrored by the twin)
        if ((rc = launch_fold_cat_weights(st, net->P + b.c3.w_off, net->P + b.cd.w_off, b.b3.scale, b.bd.scale, b.b3.shift, b.bd.shift, b.cout, b.width,
                                          b.cin, 2, b.wcat, b.shcat))) return rc;
        IGemmArgs stage{};
        stage.x_rep = 2; stage.out_shift = b.shcat; stage.out_relu = 1;
        return cat_gemm(net, st, b.c3, 0, b.wcat, b.a2, b.width, x, b.cin, b.cout, b.y, stage);
    }
    IGemmArgs a{};
    a.W = b.c3.w_bf16; a.X = b.a2; a.O = b.y; a.Res = x; a.out_scale = b.b3.scale; a.out_shift = b.b3.shift; a.out_relu = 1;
    if (b.has_ds) {                               // identity = bnd(convd(x)): raw output + its BatchNorm as residual scale / extra shift
        if ((rc = conv_bn_fwd(net, st, b.cd, b.bd, x, b.rawd))) return rc;
        a.Res = b.rawd; a.res_scale = b.bd.scale; a.bias = b.bd.shift;
        // moments of x for the branch's backward: G_x = x^T x, m2 = colsum(x), Ut = (Wd G_x)^T
        if (b.lin_ds && tr && (rc = linbn_fwd(net, st, b.ld, b.cd, b.bd, x))) return rc;
    }
    a.bits_out = tr ? b.ybits : nullptr;
    a.Cm = b.cout; a.P = net->N * b.hout * b.wout; a.g = conv_geom(b.c3, 0);
    return launch_igemm_conv(st, a);
}

}  // namespace

// training an IBN-a net needs half-channel batch statistics and an instance-norm backward, which the plan does not have
static int eval_only_error(const char* who) {
    set_error("%s: a plan with IBN-a stages is eval only (running statistics; no training forward, no backward)", who);
    return DALI_ERR_LIMIT;
}

extern "C" int dali_resnet_set_feature(dali_resnet* net, int mode) {
    DALI_REQUIRE(net, "dali_resnet_set_feature: null net");
    DALI_REQUIRE(mode >= DALI_FEATURE_BOTH && mode <= DALI_FEATURE_GMP, "dali_resnet_set_feature: bad feature mode %d", mode);
    net->feature_mode = mode;
    return DALI_OK;
}

namespace {

// The trunk of a forward: (inference) every BatchNorm's coefficients, the stem and the blocks.  -> the layer4 map, bf16 [N][head_hw][feat_dim]
int trunk_forward(dali_resnet* net, hipStream_t st, const float* images, bool tr, const uint16_t** map) {
    net->fwd_training = tr;
    int rc;
    if (!tr) {                                               // inference: every BatchNorm's scale / shift from the running statistics, one launch
        std::vector<BnEvalJob> jobs;
        auto add = [&](Bn& b, const char* = nullptr) { const BnParams p = bn_params(net, b); jobs.push_back(BnEvalJob{p.gamma, p.beta, p.rm, p.rv, b.scale + b.lo, b.shift + b.lo, b.C - b.lo}); };
        add(net->stem_bn);
        for (auto& b : net->blocks) for_each_bn(b, add);
        if ((rc = launch_bn_eval_coeffs_batched(st, jobs.data(), (int)jobs.size(), 1e-5f))) return rc;
    }
    if ((rc = stem_forward(net, st, images, tr))) return rc;
    const uint16_t* x = net->pool0;
    for (auto& b : net->blocks) {
        if ((rc = block_forward(net, st, b, x, tr))) return rc;
        x = b.y;
    }
    *map = x;
    return DALI_OK;
}

}  // namespace

extern "C" int dali_resnet_forward(dali_resnet* net, void* stream, const float* images, int training, float* emb) {
    DALI_REQUIRE(net && net->P && images && emb, "dali_resnet_forward: null argument or net not bound");
    if (training && net->eval_only) return eval_only_error("dali_resnet_forward(training = 1)");
    hipStream_t st = (hipStream_t)stream;
    const bool tr = training != 0;
    const uint16_t* x;
    int rc;
    if ((rc = trunk_forward(net, st, images, tr, &x))) return rc;
    // ---- head: avg-pool + max-pool, BatchNorm1d ----
    if ((rc = launch_head_pool_fwd(st, x, net->N, net->head_hw, net->feat_dim, net->feature_mode, net->feat, net->head_arg))) return rc;
    const BnParams p = bn_params(net, net->neck);
    return launch_bn1d_fwd(st, net->feat, net->N, net->feat_dim, p.gamma, p.beta, p.rm, p.rv, tr ? 1 : 0, 0.1f, 1e-5f, emb, net->neck_mean, net->neck_invstd);
}

extern "C" int dali_resnet_head_map(dali_resnet* net, int* h, int* w) {
    DALI_REQUIRE(net && h && w, "dali_resnet_head_map: null argument");
    *h = net->blocks.back().hout; *w = net->blocks.back().wout;
    return DALI_OK;
}

// Inference with several heads from one trunk pass: the pooled values of every head in one launch ([n_heads][N][feat_dim]), the neck by the
// running statistics over the n_heads * N rows at once (an affine map per element: each row gets what dali_resnet_forward gives it), and the
// channel sums of the map when asked for.  Neither the neck's saved statistics nor feature_mode are touched.  The pooled values take no
// arena of their own: they lie in the backward's gradient buffers (gbuf[0..5], one region), which no forward uses.
extern "C" int dali_resnet_forward_heads(dali_resnet* net, void* stream, const float* images, const dali_head_spec* heads, int n_heads, float* emb,
                                         float* heat) {
    DALI_REQUIRE(net && net->P && images && heads && emb, "dali_resnet_forward_heads: null argument or net not bound");
    hipStream_t st = (hipStream_t)stream;
    const Block& last = net->blocks.back();
    const uint16_t* x;
    int rc;
    if ((rc = check_head_specs(heads, n_heads, last.hout, last.wout))) return rc;       // before anything runs
    float* pooled = reinterpret_cast<float*>(net->gbuf[0]);
    DALI_REQUIRE((size_t)n_heads * net->N * net->feat_dim * 4 <= 6 * net->gbuf_bytes, "dali_resnet_forward_heads: %d heads do not fit the plan's scratch", n_heads);
    if ((rc = trunk_forward(net, st, images, false, &x))) return rc;
    if ((rc = launch_head_pool_multi(st, x, net->N, last.hout, last.wout, net->feat_dim, heads, n_heads, pooled))) return rc;
    const BnParams p = bn_params(net, net->neck);
    if ((rc = launch_bn1d_fwd(st, pooled, n_heads * net->N, net->feat_dim, p.gamma, p.beta, p.rm, p.rv, 0, 0.1f, 1e-5f, emb, nullptr, nullptr)))
        return rc;
    return heat ? launch_channel_sum(st, x, (int64_t)net->N * net->head_hw, net->feat_dim, heat) : DALI_OK;
}

// Every block receives and hands on the MASKED gradient dz = dL/dy * (y > 0) (the gradient in front of the block's final ReLU): the
// producer (the data-gradient epilogue of the next block's conv1, or the head pooling) applies the mask bits, so that neither the
// BatchNorm backward nor the identity path has to.  prev_bits = ReLU mask of the previous block's output (null for the first block).
static int block_backward(dali_resnet* net, hipStream_t st, Block& b, const uint8_t* prev_bits) {
    int rc;
    uint16_t* dz = net->cur_dy;                                   // masked grad wrt block output y
    const int Pout = net->N * b.hout * b.wout, Pin = net->N * b.hin * b.win;
    uint16_t* d_rawd = nullptr;
    // bn3 + conv3 through the moments of a2 (bnlin.hip): no reduce / apply passes over [P][cout] tensors, conv3's raw output does not exist.
    // G0 = dz^T a2 goes into the gradient slot with s = colsum(dz) riding on the GEMM
    if ((rc = linbn_bwd(net, st, b.l3, b.c3, b.b3, dz, b.a2, b.sdz, true, DALI_SNAP_G0_CONV3))) return rc;
    uint16_t* d_a2 = next_gbuf(net, dz);
    uint16_t* scratch_a = next_gbuf(net, dz, d_a2);
    {   // d_a2 = dz (A.W3) + W3^T Kc - a2 (W3^T diag(Q) W3) as ONE GEMM over K = cout + w: [dz | a2] against the concatenated image
        // (two launches with the partial result stored and re-read before: 190 -> see docs/experiments.md)
        IGemmArgs stage{};
        stage.bias = b.l3.bvec;
        if ((rc = cat_gemm(net, st, b.c3, 1, b.l3.wd, dz, b.cout, b.a2, b.width, b.width, d_a2, stage))) return rc;
        if ((rc = snap_keep(net, st, DALI_SNAP_D_A2, d_a2, (size_t)Pout * b.width * 2))) return rc;
    }
    if (b.lin_ds) {
        // downsample branch through the moments of x: G0d = dz^T x into the gradient slot (s = colsum(dz) is bn3's), finished in place by the row
        // kernel together with dgamma / dbeta and the two data-gradient images; the data gradient itself follows conv1's below
        if ((rc = linbn_bwd(net, st, b.ld, b.cd, b.bd, dz, b.x, b.sdz, false, DALI_SNAP_G0_DS))) return rc;
    } else if (b.has_ds) {                                    // the downsample BatchNorm: its own two passes over (dz, rawd)
        d_rawd = next_gbuf(net, dz, d_a2, scratch_a);
        if ((rc = bn_bwd(net, st, b.bd, b.rawd, dz, 0, Pout, d_rawd))) return rc;
        if ((rc = snap_keep(net, st, DALI_SNAP_D_RAWD, d_rawd, (size_t)Pout * b.cout * 2))) return rc;
    }
    // bn2 + relu, in place.  The ReLU mask is recomputed from raw2 (raw*scale+shift > 0 <=> a2 > 0: bf16 rounding cannot
    // flush a positive fp32 to zero) instead of reading a2: one tensor read less in each of the two passes.
    if ((rc = bn_bwd(net, st, b.b2, b.raw2, d_a2, 1, Pout, d_a2))) return rc;
    if ((rc = snap_keep(net, st, DALI_SNAP_D_RAW2, d_a2, (size_t)Pout * b.width * 2))) return rc;
    // conv2
    if ((rc = conv_wgrad(net, st, b.c2, b.a1, d_a2))) return rc;
    uint16_t* d_a1 = scratch_a;
    if ((rc = conv_dgrad(net, st, b.c2, d_a2, nullptr, d_a1))) return rc;
    if ((rc = snap_keep(net, st, DALI_SNAP_D_A1, d_a1, (size_t)Pin * b.width * 2))) return rc;
    if ((rc = bn_bwd(net, st, b.b1, b.raw1, d_a1, 1, Pin, d_a1))) return rc;
    if ((rc = snap_keep(net, st, DALI_SNAP_D_RAW1, d_a1, (size_t)Pin * b.width * 2))) return rc;
    b.dbg_d_raw1 = d_a1;
    // conv1 (+ identity / downsample branch); the result is masked with the previous block's ReLU bits
    if ((rc = conv_wgrad(net, st, b.c1, b.x, d_a1))) return rc;
    uint16_t* dx = d_a2;                                          // d_a2 is dead now
    if (b.lin_ds) {
        // dx = d_a1 W1 + [dz | x] [(A_d.Wd)^T | -(Wd^T diag(Q_d) Wd)] + Wd^T Kc: conv1's data gradient, then the branch's two-operand GEMM on top of it
        if ((rc = conv_dgrad(net, st, b.c1, d_a1, nullptr, dx, prev_bits))) return rc;
        if ((rc = snap_keep(net, st, DALI_SNAP_DX_CONV1, dx, (size_t)Pin * b.cin * 2))) return rc;
        IGemmArgs stage{};
        stage.Res = dx; stage.bias = b.ld.bvec;
        if ((rc = cat_gemm(net, st, b.cd, 1, b.ld.wd, dz, b.cout, b.x, b.cin, b.cin, dx, stage))) return rc;
    } else if (b.has_ds) {
        if ((rc = conv_wgrad(net, st, b.cd, b.x, d_rawd))) return rc;
        // conv1's data gradient first, then the downsample branch accumulates into it in place: with stride 2 only the
        // even-even quarter of the positions receives a contribution (launch_igemm_conv's parity split).  (a + b) * m = a * m + b * m:
        // both launches apply the mask.
        if ((rc = conv_dgrad(net, st, b.c1, d_a1, nullptr, dx, prev_bits))) return rc;
        if ((rc = snap_keep(net, st, DALI_SNAP_DX_CONV1, dx, (size_t)Pin * b.cin * 2))) return rc;
        if ((rc = conv_dgrad(net, st, b.cd, d_rawd, dx, dx, prev_bits))) return rc;
    } else {
        if ((rc = conv_dgrad(net, st, b.c1, d_a1, dz, dx, prev_bits))) return rc;             // identity path: + dz
    }
    net->cur_dy = dx;
    net->cur_dy_bytes = (int64_t)Pin * b.cin * 2;
    return DALI_OK;
}

// neck + head pooling: d_emb -> the masked gradient of the last block's output in cur_dy
static int head_backward(dali_resnet* net, hipStream_t st, const float* d_emb) {
    int rc;
    if ((rc = launch_bn1d_bwd(st, net->feat, d_emb, net->N, net->feat_dim, net->P + net->neck.g_off, net->neck_mean, net->neck_invstd,
                              net->dfeat, net->G + net->neck.g_off, net->G + net->neck.b_off))) return rc;
    net->cur_dy = net->gbuf[0];
    if ((rc = launch_head_pool_bwd(st, net->dfeat, net->head_arg, net->N, net->head_hw, net->feat_dim, net->feature_mode, net->cur_dy,
                                   net->blocks.back().ybits))) return rc;
    net->cur_dy_bytes = (int64_t)net->N * net->head_hw * net->feat_dim * 2;
    return snap_keep(net, st, DALI_SNAP_HEAD_DZ, net->cur_dy, (size_t)net->cur_dy_bytes);
}

// maxpool + stem BN backward, then the stem weight gradient (no data gradient: images need none)
static int stem_backward(dali_resnet* net, hipStream_t st) {
    int rc;
    uint16_t* d_raw0 = next_gbuf(net, net->cur_dy);
    if ((rc = launch_maxpool_bn_bwd(st, net->cur_dy, net->pool_arg, net->raw0, net->stem_bn.mean, net->stem_bn.invstd, net->stem_bn.scale,
                                    net->N, net->stem_h, net->stem_w, net->stem.cout, net->bwd_partial, net->stem_bn.coef,
                                    net->G + net->stem_bn.g_off, net->G + net->stem_bn.b_off, d_raw0, net->red_scratch))) return rc;
    net->dbg_d_raw0 = d_raw0;
    if ((rc = snap_keep(net, st, DALI_SNAP_D_RAW0, d_raw0, (size_t)net->N * net->stem_h * net->stem_w * net->stem.cout * 2))) return rc;
    if ((rc = run_wgrad(net, st, stem_wgrad_desc(net), d_raw0, net->ximg, net->stem_dw_pad))) return rc;
    if ((rc = snap_keep(net, st, DALI_SNAP_STEM_DW_PAD, net->stem_dw_pad, (size_t)net->stem.cout * 224 * 4))) return rc;
    return launch_stem_unpack_wgrad(st, net->stem_dw_pad, net->stem.cout, net->G + net->stem.w_off);
}

// Runs stages [stage_begin, stage_end] of the backward pass (0: neck+head+layer4, 1: layer3, 2: layer2,
// 3: layer1+stem).  Stage 0 consumes d_emb; later stages continue from the gradient the previous call left.
extern "C" int dali_resnet_backward(dali_resnet* net, void* stream, const float* d_emb, int stage_begin, int stage_end) {
    DALI_REQUIRE(net, "dali_resnet_backward: null net");
    if (net->eval_only) return eval_only_error("dali_resnet_backward");
    DALI_REQUIRE(net->P && net->G, "dali_resnet_backward: net not bound (grads required)");
    DALI_REQUIRE(net->fwd_training, "dali_resnet_backward: the last forward was not in training mode");
    DALI_REQUIRE(stage_begin >= 0 && stage_end <= 3 && stage_begin <= stage_end, "dali_resnet_backward: bad stage range %d..%d", stage_begin, stage_end);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    for (int stage = stage_begin; stage <= stage_end; ++stage) {
        const int li = 3 - stage;
        if (stage == 0) {
            DALI_REQUIRE(d_emb != nullptr, "dali_resnet_backward: d_emb is null");
            if ((rc = head_backward(net, st, d_emb))) return rc;
        }
        for (int bi = net->stage_last[li]; bi >= net->stage_first[li]; --bi)
            if ((rc = block_backward(net, st, net->blocks[bi], bi > 0 ? net->blocks[bi - 1].ybits : nullptr))) return rc;
        if (stage == 3 && (rc = stem_backward(net, st))) return rc;
    }
    return DALI_OK;
}

// Diagnostic (include/daliid_debug.h): the backward pass ONE bottleneck at a time, so that a test can read the gradient entering every block
// (`grad_cur` of dali_resnet_debug_tensor) instead of one per stage.  Call with block = last block first (that call also runs the neck + head
// backward from d_emb), then block - 1, ... down to 0, then -1 (the stem); same launches, same order as dali_resnet_backward.
static int debug_backward_block(dali_resnet* net, void* stream, const float* d_emb, int block) {
    DALI_REQUIRE(net, "dali_debug_resnet_backward_block: null net");
    if (net->eval_only) return eval_only_error("dali_debug_resnet_backward_block");
    DALI_REQUIRE(net->P && net->G, "dali_debug_resnet_backward_block: net not bound (grads required)");
    DALI_REQUIRE(net->fwd_training, "dali_debug_resnet_backward_block: the last forward was not in training mode");
    const int nb = (int)net->blocks.size();
    if (block == -1) return stem_backward(net, (hipStream_t)stream);      // after block 0: the stem (its own call, so that block 0's scratch tensors can be read first)
    DALI_REQUIRE(block >= 0 && block < nb, "dali_debug_resnet_backward_block: block %d out of range", block);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (block == nb - 1) {
        DALI_REQUIRE(d_emb != nullptr, "dali_debug_resnet_backward_block: d_emb is null");
        if ((rc = head_backward(net, st, d_emb))) return rc;
    }
    return block_backward(net, st, net->blocks[block], block > 0 ? net->blocks[block - 1].ybits : nullptr);
}
extern "C" int dali_debug_resnet_backward_block(dali_resnet* net, void* stream, const float* d_emb, int block) {
    return debug_backward_block(net, stream, d_emb, block);
}
// Diagnostic (include/daliid_debug.h): the same call with snap_keep switched on: the backward's in-place intermediates are copied into `snap` as
// they are produced (offsets[DALI_SNAP_*]: where, or -1)
extern "C" int dali_debug_resnet_backward_block_snap(dali_resnet* net, void* stream, const float* d_emb, int block, void* snap, int64_t snap_bytes,
                                                      int64_t* offsets) {
    DALI_REQUIRE(net && snap && offsets && snap_bytes > 0, "dali_debug_resnet_backward_block_snap: null argument");
    for (int i = 0; i < DALI_SNAP_COUNT; ++i) offsets[i] = -1;
    net->snap = static_cast<char*>(snap); net->snap_cap = snap_bytes; net->snap_used = 0; net->snap_offsets = offsets;
    const int rc = debug_backward_block(net, stream, d_emb, block);
    net->snap = nullptr; net->snap_cap = 0; net->snap_offsets = nullptr;
    return rc;
}

// Debug/inspection: device pointer + byte size of a named arena tensor of a bound plan (intermediates: valid after a forward).  Every name is
// declared where dali_resnet_create_ex reserves the tensor; a tensor that this plan does not hold (an eval-only plan reserves none of the
// backward's) is refused like an unknown name.
// Names: wbf16 (the bf16 cast of the flat parameters), ximg (packed image bf16 [N][H+6][W+8][4]), w_stem (bf16 [Cout][7][8][4]), raw0, pool0,
// pool_arg (uint8, the max-pool's tap), bn1.{scale,shift,mean,invstd,coef}, feat, head_arg (int16), neck.{mean,invstd}, gbuf0 (an eval-only plan:
// the whole region dali_resnet_forward_heads pools into); of a training plan dfeat (after a backward's head call), d_raw0 (after a stem backward),
// grad_cur (gradient wrt the input of the last block processed by backward) and the scratch stat_partial, bwd_partial, wgrad_slab, cs_partial,
// stem_dw_pad, red_scratch, gbuf0 .. gbuf5;
// block<i>.{a1,a2,y}, .rawd (with a downsample branch), .bn{1,2,3,d}.{scale,shift,mean,invstd,coef}, the weight images .conv{1,2,3,d}.w (bf16
// [cout][r][s][cin]); for an IBN block .in1.{mean,invstd} (fp32 [N][width / 2], of the last forward); where the inference forward folds conv3 +
// downsample into one GEMM .wcat (bf16 [cout][2 (w + cin)]: W3 hi | W3 lo | Wd hi | Wd lo) and .shcat (fp32 [cout]); of a training plan
// .{raw1,raw2}, .d_raw1 (after the block's backward), .ybits (the ReLU mask of y, one bit per element), .sdz (colsum(dz), after the block's
// backward), .conv{1,2,3,d}.wt (bf16 [cin][r*s][cout]) and the moments scheme's .l3.{gram,m2,ut,wd,bvec,qk,dot} (LinBn; wd, bvec, qk after the
// block's backward), the same without dot under .ld. where the downsample branch's backward runs through the moments of x
extern "C" int dali_resnet_debug_tensor(dali_resnet* net, const char* name, void** ptr, int64_t* bytes) {
    DALI_REQUIRE(net && name && ptr && bytes && net->arena, "dali_resnet_debug_tensor: bad argument / net not bound");
    // the one name that is no fixed tensor: it moves through the gradient buffers and changes its size from block to block
    if (!strcmp(name, "grad_cur") && net->cur_dy) { *ptr = net->cur_dy; *bytes = net->cur_dy_bytes; return DALI_OK; }
    return net->arena_tensor("dali_resnet_debug_tensor", name, ptr, bytes);
}
extern "C" int dali_debug_resnet_arena_entry(const dali_resnet* net, int index, char* name, int name_cap, int64_t* offset, int64_t* bytes, int* reserved) {
    DALI_REQUIRE(net, "dali_debug_resnet_arena_entry: null net");
    return net->arena_entry("dali_debug_resnet_arena_entry", index, name, name_cap, offset, bytes, reserved);
}

// vit_plan.hip -- native executor of the TransReID ViT encoder + BN neck:
//   make_models.build_transformer.forward (make_models.py:184-205) over vit_pytorch.TransReID.forward_features
//   (vit_pytorch.py:375-408; camera = view = 0, local_feature = False; Dropout rate 0).  DropPath (vit_pytorch.py:45-62, wired at
//   :338 and :178-179) is applied in training when the caller hands over the per-sample branch scales (dali_vit_set_drop_path).
// Same contract as resnet_plan.hip: the plan owns topology + launch order, PyTorch owns flat fp32 params / grads /
// buffers and one byte arena.  Parameter names / order follow the reference state_dict ("base.cls_token",
// "base.pos_embed", "base.patch_embed.proj.weight", "base.blocks.N....", "base.norm.*", "base.fc.*", "bottleneck.*").
// `base.fc` (vit_pytorch.py:349) is never used by forward(): it is carried as parameters with zero gradient.
// dali_vit_ext adds what a TransReID checkpoint normally contains (dali_vit_create_ex; all zero = the plan above, byte for byte):
//   SIE (vit_pytorch.py:316-331, 382-387): "base.sie_embed" [n_sie,1,C] right after pos_embed, added to every token as coef * sie[idx[b]];
//   local_feature (vit_pytorch.py:393-396): blocks[:-1] only, all tokens, no final norm; blocks[depth-1], norm and fc stay as unused parameters;
//   JPM (make_models.build_transformer_local, make_models.py:221-377), eval mode only: b1 / b2 = block + norm copies, the shifted and
//   shuffled patch tokens cut into four runs that share b2, five BatchNorm1d necks, output [B][5C].
// A local_feature / JPM plan never runs a backward, so it reserves none of the backward's buffers (dgrad weight images, weight-gradient slab,
// reduction partials, DropPath rows, gradient buffers) and its refresh_weights only casts.  The same holds for any plan with more than 256 tokens
// (up to 1024: 384x128 at stride 12 = 311, 256x256 at stride 16 = 257): only the attention FORWARD exists there, so a training forward and the
// backward entries return DALI_ERR_LIMIT before their first launch.  And for a plan with head_dim 96 (ViT-Small, vit_pytorch.py:461-468: dim 768,
// 8 heads): at that width only the chunked attention forward exists (launch_attention_fwd_hd96), whatever the token count.
//   no_qkv_bias (vit_pytorch.py:147, qkv_bias=False): no block has an "attn.qkv.bias" parameter; the qkv GEMM runs without a bias and its
//   weight gradient without a column sum.  qk_scale (vit_pytorch.py:145): the attention scale, 0 = head_dim ** -0.5; the plan keeps ONE scale
//   (att_scale) for the forward and the backward.  Both are independent of head_dim and train at head_dim 64.
#include "kernels.h"
#include "plan_table.h"
#include <cmath>
#include <cstdio>
#include <memory>
#include <new>
#include <string>
#include <vector>

using namespace dali;

namespace {
struct Lin { int K, N; int64_t w_off, b_off; uint16_t *w, *wt; };
struct Ln { int64_t g_off, b_off; float *mean, *rstd; };
struct VBlock {
    Ln n1, n2; Lin qkv, proj, fc1, fc2;
    uint16_t *x_in, *h1, *qkv_o, *att, *x_mid, *h2, *pre1, *act1, *x_out;
    float* lse;
};
struct Neck { int64_t g, b, rm, rv; };
}  // namespace

struct dali_vit : PlanTable {
    dali_ctx* ctx;
    dali_vit_cfg cfg;
    int B, T, np, C, H, rows, hd;
    float att_scale;                      // vit_pytorch.py:145: qk_scale or head_dim ** -0.5 (exactly 0.125f at head_dim 64), forward and backward
    int64_t cls_off, pos_off, fcw_off, fcb_off;
    Lin patch; Ln fin; std::vector<VBlock> blocks;
    int64_t neck_g, neck_b, neck_rm, neck_rv;
    uint16_t *wbf16 = nullptr, *patches = nullptr, *pe = nullptr, *x0 = nullptr, *cls_rows = nullptr, *dcls_rows = nullptr, *dgf16 = nullptr;
    float *gf = nullptr, *dgf = nullptr, *neck_mean = nullptr, *neck_invstd = nullptr, *slab = nullptr, *partial = nullptr;
    float *fin_mean = nullptr, *fin_rstd = nullptr, *dp_rows = nullptr;        // dp_rows [2*depth][rows]: DropPath factors per output row
    double* scratch = nullptr;
    uint16_t* gbuf[4] = {nullptr, nullptr, nullptr, nullptr};
    float *P = nullptr, *G = nullptr, *Bf = nullptr;
    char* arena = nullptr;
    bool fwd_training = false;
    const float* dp_scale = nullptr;      // device [2*depth][B]: row 2i = attention branch of block i, 2i+1 = its MLP branch; null = no DropPath
    const float* dp_used = nullptr;       // what the last training forward applied (the backward mirrors it)
    // ---- SIE / local_feature / JPM (dali_vit_ext) ----
    dali_vit_ext ext{};
    int64_t sie_off = -1;
    const int32_t* sie_used = nullptr;    // the indices of the last training forward (the backward's sie_grad reads them)
    int L = 0, Tl = 0, rows2 = 0;         // JPM: tokens per run, 1 + L, and the local branch's row count divide * B * Tl
    VBlock b1, b2; Ln fin1, fin2;
    Neck necks[5];                        // bottleneck, bottleneck_1 .. _4 (necks[0] = neck_g .. neck_rv)
    std::vector<int32_t> map_host;        // [divide][L] token indices, copied from dali_vit_ext::token_map
    int32_t* map_dev = nullptr;
    uint16_t *jseq = nullptr, *cls2 = nullptr;
    float *gf2 = nullptr, *fin2_mean = nullptr, *fin2_rstd = nullptr;
    int n_stages = 1;
    std::vector<int> stage_first_block;   // backward stage s runs blocks [stage_first_block[s+1], stage_first_block[s]) downwards
    bool eval_only = false;               // local_feature / JPM, more than VIT_TRAIN_MAX_T tokens, or head_dim 96: none of the backward's buffers
};

namespace {
// The attention forward runs up to 1024 tokens (launch_attention_fwd), its backward up to 256: a longer plan is an eval plan.
// At head_dim 96 only the attention forward exists, at any length: such a plan is an eval plan too.
constexpr int VIT_MAX_T = 1024, VIT_TRAIN_MAX_T = 256, VIT_TRAIN_HD = 64, VIT_EVAL_HD = 96;
// the training forward and every backward entry ask this before their first launch (the token check first)
int refuse_long_training(const dali_vit* n) {
    if (n->T > VIT_TRAIN_MAX_T) {
        set_error("training needs at most %d tokens (this plan has %d); eval mode only", VIT_TRAIN_MAX_T, n->T);
        return DALI_ERR_LIMIT;
    }
    if (n->hd != VIT_TRAIN_HD) {
        set_error("training needs head_dim %d (this plan has %d); eval mode only", VIT_TRAIN_HD, n->hd);
        return DALI_ERR_LIMIT;
    }
    return DALI_OK;
}
void add_lin(dali_vit* n, Lin& l, const std::string& name, int K, int N, bool bias = true) {
    l.K = K; l.N = N;
    l.w_off = n->add_param(name + ".weight", {N, K});
    l.b_off = bias ? n->add_param(name + ".bias", {N}) : -1;          // -1: no such parameter (lin_bias / lin_dbias hand out null)
    l.w = l.wt = nullptr;
}
const float* lin_bias(const dali_vit* n, const Lin& l) { return l.b_off >= 0 ? n->P + l.b_off : nullptr; }
float* lin_dbias(const dali_vit* n, const Lin& l) { return l.b_off >= 0 ? n->G + l.b_off : nullptr; }
void add_ln(dali_vit* n, Ln& l, const std::string& name, int C) {
    l.g_off = n->add_param(name + ".weight", {C});
    l.b_off = n->add_param(name + ".bias", {C});
}
void add_block(dali_vit* n, VBlock& b, const std::string& pre) {
    const int C = n->C;
    add_ln(n, b.n1, pre + ".norm1", C);
    add_lin(n, b.qkv, pre + ".attn.qkv", C, 3 * C, !n->ext.no_qkv_bias);
    add_lin(n, b.proj, pre + ".attn.proj", C, C);
    add_ln(n, b.n2, pre + ".norm2", C);
    add_lin(n, b.fc1, pre + ".mlp.fc1", C, n->cfg.mlp_hidden);
    add_lin(n, b.fc2, pre + ".mlp.fc2", n->cfg.mlp_hidden, C);
}
// f(linear layer, its name inside the block's arena names)
template <class F> void for_each_lin(VBlock& b, F f) { f(b.qkv, "qkv"); f(b.proj, "proj"); f(b.fc1, "fc1"); f(b.fc2, "fc2"); }
// The thirteen activation and statistic tensors of a block that runs on `rows` token rows = seqs sequences of T tokens, as `prefix`<field>
void reserve_block_acts(dali_vit* n, VBlock& b, const std::string& prefix, size_t rows, size_t seqs, size_t T) {
    const size_t C = n->C, Hd = n->cfg.mlp_hidden;
    n->reserve(prefix + "h1", b.h1, rows * C * 2); n->reserve(prefix + "qkv", b.qkv_o, rows * 3 * C * 2); n->reserve(prefix + "att", b.att, rows * C * 2);
    n->reserve(prefix + "x_mid", b.x_mid, rows * C * 2); n->reserve(prefix + "h2", b.h2, rows * C * 2); n->reserve(prefix + "pre1", b.pre1, rows * Hd * 2);
    n->reserve(prefix + "act1", b.act1, rows * Hd * 2); n->reserve(prefix + "x_out", b.x_out, rows * C * 2);
    n->reserve(prefix + "lse", b.lse, seqs * n->H * T * 4);
    n->reserve(prefix + "n1.mean", b.n1.mean, rows * 4); n->reserve(prefix + "n1.rstd", b.n1.rstd, rows * 4);
    n->reserve(prefix + "n2.mean", b.n2.mean, rows * 4); n->reserve(prefix + "n2.rstd", b.n2.rstd, rows * 4);
}
// `prefix`{qkv,proj,fc1,fc2}.w: the block's forward weight images, views into the flat bf16 cast (dali_vit_bind sets them)
void name_block_weights(dali_vit* n, VBlock& b, const std::string& prefix) {
    for_each_lin(b, [&](Lin& l, const char* name) { n->view(prefix + name + ".w", l.w, (size_t)l.K * l.N * 2); });
}
}  // namespace

extern "C" int dali_vit_create(dali_ctx* ctx, const dali_vit_cfg* cfg, dali_vit** out) {
    const dali_vit_ext none{};
    return dali_vit_create_ex(ctx, cfg, &none, out);
}

extern "C" int dali_vit_create_ex(dali_ctx* ctx, const dali_vit_cfg* cfg, const dali_vit_ext* ext, dali_vit** out) {
    DALI_REQUIRE(ctx && cfg && ext && out, "dali_vit_create: null argument");
    DALI_REQUIRE(cfg->batch > 0 && cfg->patch % 8 == 0 && cfg->stride > 0 && cfg->height >= cfg->patch && cfg->width >= cfg->patch,
                 "dali_vit_create: bad geometry");
    DALI_REQUIRE(cfg->heads > 0 && cfg->dim > 0 && cfg->dim <= 2048 && cfg->dim % cfg->heads == 0 &&
                 (cfg->dim / cfg->heads == VIT_TRAIN_HD || cfg->dim / cfg->heads == VIT_EVAL_HD),
                 "dali_vit_create: head_dim = dim / heads must be %d or %d (dim=%d heads=%d)", VIT_TRAIN_HD, VIT_EVAL_HD, cfg->dim, cfg->heads);
    DALI_REQUIRE(ext->qk_scale >= 0.0f && ext->qk_scale < 1e30f, "dali_vit_create: qk_scale must be positive, or 0 for head_dim ** -0.5");
    DALI_REQUIRE(cfg->depth >= 1 && cfg->mlp_hidden % 32 == 0 && cfg->mlp_hidden > 0, "dali_vit_create: bad depth / mlp_hidden");
    std::unique_ptr<dali_vit> owner(new (std::nothrow) dali_vit());
    dali_vit* n = owner.get();
    if (!n) { set_error("dali_vit_create: out of host memory"); return DALI_ERR_NOMEM; }
    n->ctx = ctx; n->cfg = *cfg; n->ext = *ext;
    if (n->ext.jpm) n->ext.local_feature = 1;            // make_models.py:243: the JPM base is built with local_feature = cfg.MODEL.JPM
    const int ny = (cfg->height - cfg->patch) / cfg->stride + 1, nx = (cfg->width - cfg->patch) / cfg->stride + 1;
    n->B = cfg->batch; n->np = ny * nx; n->T = n->np + 1; n->C = cfg->dim; n->H = cfg->heads; n->rows = n->B * n->T;
    n->hd = cfg->dim / cfg->heads;
    n->att_scale = ext->qk_scale > 0.0f ? ext->qk_scale : n->hd == VIT_TRAIN_HD ? 0.125f : 1.0f / sqrtf((float)n->hd);
    if (n->T > VIT_MAX_T) { set_error("dali_vit_create: %d tokens exceed the attention kernel's limit of %d", n->T, VIT_MAX_T); return DALI_ERR_LIMIT; }
    // past VIT_TRAIN_MAX_T tokens, and at head_dim 96, only the attention forward exists: an eval plan, reserved like a local_feature one
    n->eval_only = n->ext.local_feature != 0 || n->T > VIT_TRAIN_MAX_T || n->hd != VIT_TRAIN_HD;
    const int C = n->C, Kp = 3 * cfg->patch * cfg->patch;
    n->cls_off = n->add_param("base.cls_token", {1, 1, C});
    n->pos_off = n->add_param("base.pos_embed", {1, n->T, C});
    DALI_REQUIRE(ext->n_sie >= 0, "dali_vit_create: n_sie = %d", ext->n_sie);
    if (ext->n_sie > 0) n->sie_off = n->add_param("base.sie_embed", {ext->n_sie, 1, C});      // vit_pytorch.py:316-331
    n->patch.K = Kp; n->patch.N = C;
    n->patch.w_off = n->add_param("base.patch_embed.proj.weight", {C, 3, cfg->patch, cfg->patch});
    n->patch.b_off = n->add_param("base.patch_embed.proj.bias", {C});
    n->blocks.resize(cfg->depth);
    for (int i = 0; i < cfg->depth; ++i) add_block(n, n->blocks[i], "base.blocks." + std::to_string(i));
    add_ln(n, n->fin, "base.norm", C);
    n->fcw_off = n->add_param("base.fc.weight", {cfg->num_classes, C});
    n->fcb_off = n->add_param("base.fc.bias", {cfg->num_classes});
    if (n->ext.jpm) {
        // make_models.py:249-258, 279-288: b1 / b2 = (block, norm) copies, then the five unused classifiers, in the state dict's order
        DALI_REQUIRE(n->ext.id_classes >= 1, "dali_vit_create: JPM needs id_classes >= 1 (the classifiers' rows)");
        DALI_REQUIRE(n->ext.divide == 4, "dali_vit_create: JPM needs divide = 4, the reference's forward cuts four runs (got %d)", n->ext.divide);
        // the token map (shift + group shuffle, make_models.jpm_token_map) is the caller's: [divide][L] token indices, each a patch token 1 .. np
        n->L = n->np / n->ext.divide;
        bool map_ok = n->ext.token_map != nullptr && n->L >= 1;
        for (int i = 0; map_ok && i < n->ext.divide * n->L; ++i) map_ok = n->ext.token_map[i] >= 1 && n->ext.token_map[i] <= n->np;
        DALI_REQUIRE(map_ok, "dali_vit_create: JPM needs token_map [%d][%d] with entries in 1 .. %d", n->ext.divide, n->L, n->np);
        n->map_host.assign(n->ext.token_map, n->ext.token_map + (size_t)n->ext.divide * n->L);
        n->ext.token_map = nullptr;                      // copied: the caller's array need not outlive this call
        n->Tl = 1 + n->L; n->rows2 = n->ext.divide * n->B * n->Tl;
        add_block(n, n->b1, "b1.0"); add_ln(n, n->fin1, "b1.1", C);
        add_block(n, n->b2, "b2.0"); add_ln(n, n->fin2, "b2.1", C);
        for (int i = 0; i < 5; ++i) n->add_param(i ? "classifier_" + std::to_string(i) + ".weight" : std::string("classifier.weight"), {n->ext.id_classes, C});
    }
    for (int i = 0; i < (n->ext.jpm ? 5 : 1); ++i) {
        const std::string nm = i ? "bottleneck_" + std::to_string(i) : std::string("bottleneck");
        Neck& k = n->necks[i];
        k.g = n->add_param(nm + ".weight", {C});
        k.b = n->add_param(nm + ".bias", {C});
        k.rm = n->add_buffer(nm + ".running_mean", {C});
        k.rv = n->add_buffer(nm + ".running_var", {C});
    }
    n->neck_g = n->necks[0].g; n->neck_b = n->necks[0].b; n->neck_rm = n->necks[0].rm; n->neck_rv = n->necks[0].rv;
    // backward stages = gradient buckets of the data-parallel reducer: up to 4 groups of consecutive blocks, last blocks first
    n->n_stages = cfg->depth >= 4 ? 4 : cfg->depth;
    n->stage_first_block.resize(n->n_stages + 1);
    for (int s = 0; s <= n->n_stages; ++s) n->stage_first_block[s] = cfg->depth - (int)((int64_t)cfg->depth * s / n->n_stages);

    const size_t rows = n->rows, Hd = cfg->mlp_hidden;
    // ---- arena layout: every tensor under the name dali_debug_vit_tensor answers to ----
    n->reserve("wbf16", n->wbf16, (size_t)n->param_elems * 2);
    n->reserve("patches", n->patches, (size_t)n->B * n->np * Kp * 2);
    n->reserve("pe", n->pe, (size_t)n->B * n->np * C * 2);
    n->reserve("x0", n->x0, rows * C * 2);
    const bool eval_only = n->eval_only;
    n->view("patch.w", n->patch.w, (size_t)Kp * C * 2);
    if (!eval_only) n->reserve("patch.wt", n->patch.wt, (size_t)Kp * C * 2);          // unused (images need no gradient) but keeps Lin uniform
    // the weight-gradient workspace is sized for every linear layer the backward runs (patch embedding, then each block's four)
    WGradNeed need = linear_wgrad_need(n->B * n->np, Kp, C, true);
    size_t part = std::max(layernorm_bwd_partial_floats((int)rows, C), colsum_partial_floats((int)rows, (int)std::max<size_t>(Hd, 3 * C)));
    for (int i = 0; i < cfg->depth; ++i) {
        VBlock& b = n->blocks[i];
        const std::string pre = "block" + std::to_string(i) + ".";
        reserve_block_acts(n, b, pre, rows, n->B, n->T);
        name_block_weights(n, b, pre);
        for_each_lin(b, [&](Lin& l, const char* name) {
            if (!eval_only) n->reserve(pre + name + ".wt", l.wt, (size_t)l.K * l.N * 2);
            const WGradNeed ln = linear_wgrad_need((int)rows, l.K, l.N, true);
            need = WGradNeed{std::max(need.slab_bytes, ln.slab_bytes), std::max(need.colsum_floats, ln.colsum_floats)};
        });
    }
    n->reserve("cls_rows", n->cls_rows, (size_t)n->B * C * 2); n->reserve("dcls_rows", n->dcls_rows, (size_t)n->B * C * 2);
    n->reserve("dgf16", n->dgf16, (size_t)n->B * C * 2);
    n->reserve("gf", n->gf, (size_t)n->B * C * 4); n->reserve("dgf", n->dgf, (size_t)n->B * C * 4);
    n->reserve("neck.mean", n->neck_mean, C * 4); n->reserve("neck.invstd", n->neck_invstd, C * 4);
    n->reserve("fin.mean", n->fin_mean, n->B * 4); n->reserve("fin.rstd", n->fin_rstd, n->B * 4);
    if (!eval_only) {
        n->reserve("slab", n->slab, need.slab_bytes); n->reserve("partial", n->partial, std::max(part, need.colsum_floats) * 4);
        n->reserve("dp_rows", n->dp_rows, (size_t)2 * cfg->depth * rows * 4);
    }
    n->reserve("scratch", n->scratch, reduce_scratch_bytes((int)std::max<size_t>(Hd, 3 * C), 2));
    for (int i = 0; i < 4 && !eval_only; ++i) n->reserve("gbuf" + std::to_string(i), n->gbuf[i], rows * std::max<size_t>(Hd, 3 * C) * 2);
    // between two pieces of the backward the token gradient lies in gbuf[0]; the token tail hands its patch rows to the patch weight gradient in gbuf[1]
    n->view("grad_cur", n->gbuf[0], rows * C * 2);
    n->view("dpe", n->gbuf[1], (size_t)n->B * n->np * C * 2);
    if (n->ext.jpm) {
        // b1 runs on the B*T rows in the buffers of the idle blocks[depth-1] (bind); b2 gets its own for the divide * B sequences of 1 + L tokens
        const size_t seqs = (size_t)n->ext.divide * n->B;
        n->reserve("jseq", n->jseq, (size_t)n->rows2 * C * 2);
        reserve_block_acts(n, n->b2, "b2.", n->rows2, seqs, n->Tl);
        n->reserve("cls2", n->cls2, seqs * C * 2); n->reserve("gf2", n->gf2, seqs * C * 4);
        n->reserve("fin2.mean", n->fin2_mean, seqs * 4); n->reserve("fin2.rstd", n->fin2_rstd, seqs * 4);
        n->reserve("map_dev", n->map_dev, n->map_host.size() * 4);
        name_block_weights(n, n->b1, "b1."); name_block_weights(n, n->b2, "b2.");
    }
    *out = owner.release();
    return DALI_OK;
}

extern "C" int dali_vit_destroy(dali_vit* n) { delete n; return DALI_OK; }

extern "C" int dali_vit_sizes(const dali_vit* n, int64_t* param_elems, int64_t* buffer_elems, int64_t* arena_bytes, int* feat_dim,
                              int* n_params, int* n_buffers) {
    DALI_REQUIRE(n, "dali_vit_sizes: null net");
    return n->sizes(n->ext.jpm ? 5 * n->C : n->C, param_elems, buffer_elems, arena_bytes, feat_dim, n_params, n_buffers);
}
extern "C" int dali_vit_tensor_info(const dali_vit* n, int kind, int index, char* name, int name_cap, int64_t* offset, int64_t* numel,
                                    int* shape4, int* ndim) {
    DALI_REQUIRE(n, "dali_vit_tensor_info: null argument");
    return n->tensor_info("dali_vit_tensor_info", kind, index, name, name_cap, offset, numel, shape4, ndim);
}
extern "C" int dali_vit_bind(dali_vit* n, float* params, float* grads, float* buffers, void* arena, size_t arena_bytes) {
    DALI_REQUIRE(n && params && buffers && arena, "dali_vit_bind: null argument");
    DALI_REQUIRE(arena_bytes >= n->arena_bytes, "dali_vit_bind: arena too small (%zu < %zu)", arena_bytes, n->arena_bytes);
    n->P = params; n->G = grads; n->Bf = buffers; n->arena = static_cast<char*>(arena);
    n->bind_arena(n->arena);
    // the forward weight images lie in the flat bf16 cast, at the offsets of the fp32 parameters
    auto bind_w = [&](Lin& l, const char* = nullptr) { l.w = n->wbf16 + l.w_off; };
    bind_w(n->patch);
    for (auto& b : n->blocks) for_each_lin(b, bind_w);
    if (n->ext.jpm) {
        const VBlock& idle = n->blocks.back();           // local_feature never runs it: b1, its copy, works in its buffers
        VBlock& b = n->b1;
        b.h1 = idle.h1; b.qkv_o = idle.qkv_o; b.att = idle.att; b.x_mid = idle.x_mid; b.h2 = idle.h2; b.pre1 = idle.pre1; b.act1 = idle.act1;
        b.x_out = idle.x_out; b.lse = idle.lse;
        b.n1.mean = idle.n1.mean; b.n1.rstd = idle.n1.rstd; b.n2.mean = idle.n2.mean; b.n2.rstd = idle.n2.rstd;
        for_each_lin(n->b1, bind_w); for_each_lin(n->b2, bind_w);
    }
    return DALI_OK;
}
extern "C" int dali_vit_refresh_weights(dali_vit* n, void* stream) {
    DALI_REQUIRE(n && n->P, "dali_vit_refresh_weights: net not bound");
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_cast_bf16(st, n->P, (size_t)n->param_elems, n->wbf16);
    if (rc) return rc;
    // b1 / b2 read their bf16 weights from the same image (the cast above covers them)
    if (n->ext.jpm) DALI_HIP(hipMemcpyAsync(n->map_dev, n->map_host.data(), n->map_host.size() * 4, hipMemcpyHostToDevice, st));
    if (n->eval_only) return DALI_OK;                    // local_feature / JPM / more than 256 tokens / head_dim 96: no dgrad images
    std::vector<TransposeJob> jobs;                      // every linear's dgrad image [K][N], batched launches (48 single launches cost 0.3 ms)
    for (auto& b : n->blocks) for_each_lin(b, [&](Lin& l, const char*) { jobs.push_back(TransposeJob{l.w, l.wt, l.N, 1, l.K, 0}); });   // [N][K] -> [K][N]
    return launch_weight_transpose_batched(st, jobs.data(), (int)jobs.size());
}

namespace {
// one transformer block (vit_pytorch.py:166-184) on `rows` = seqs * T token rows; dp_att / dp_mlp: DropPath factors per row or null
int run_block(dali_vit* n, hipStream_t st, VBlock& b, const uint16_t* x, int rows, int seqs, int T, const float* dp_att, const float* dp_mlp, bool short_att) {
    const int C = n->C, Hd = n->cfg.mlp_hidden;
    const float eps = 1e-6f, scale = n->att_scale;
    int rc;
    b.x_in = const_cast<uint16_t*>(x);
    if ((rc = launch_layernorm_fwd(st, x, n->P + b.n1.g_off, n->P + b.n1.b_off, rows, C, eps, b.h1, b.n1.mean, b.n1.rstd, nullptr))) return rc;
    if ((rc = launch_linear_fwd(st, b.h1, b.qkv.w, lin_bias(n, b.qkv), 0, nullptr, b.qkv_o, nullptr, nullptr, rows, C, 3 * C))) return rc;
    if ((rc = n->hd == VIT_EVAL_HD ? launch_attention_fwd_hd96(st, b.qkv_o, seqs, T, n->H, scale, b.att, b.lse)
              : short_att        ? launch_attention_fwd_short(st, b.qkv_o, seqs, T, n->H, scale, b.att, b.lse)
                                 : launch_attention_fwd(st, b.qkv_o, seqs, T, n->H, scale, b.att, b.lse))) return rc;
    // x_mid = x + s[b] * proj(...): the per-row factor rides in the GEMM's epilogue (IGemmArgs::row_scale)
    if ((rc = launch_linear_fwd(st, b.att, b.proj.w, n->P + b.proj.b_off, 0, x, b.x_mid, nullptr, nullptr, rows, C, C, dp_att))) return rc;
    if ((rc = launch_layernorm_fwd(st, b.x_mid, n->P + b.n2.g_off, n->P + b.n2.b_off, rows, C, eps, b.h2, b.n2.mean, b.n2.rstd, nullptr))) return rc;
    if ((rc = launch_linear_fwd(st, b.h2, b.fc1.w, n->P + b.fc1.b_off, 1, nullptr, b.act1, b.pre1, nullptr, rows, C, Hd))) return rc;
    return launch_linear_fwd(st, b.act1, b.fc2.w, n->P + b.fc2.b_off, 0, b.x_mid, b.x_out, nullptr, nullptr, rows, Hd, C, dp_mlp);
}
}  // namespace

extern "C" int dali_vit_forward(dali_vit* n, void* stream, const float* images, int training, float* feat, float* global_feat) {
    return dali_vit_forward_ex(n, stream, images, nullptr, training, feat, global_feat, nullptr);
}

extern "C" int dali_vit_forward_ex(dali_vit* n, void* stream, const float* images, const int32_t* sie_idx, int training, float* feat, float* global_feat,
                                   float* tokens_out) {
    DALI_REQUIRE(n && n->P && images, "dali_vit_forward: null argument or net not bound");
    if (training) { const int lim = refuse_long_training(n); if (lim) return lim; }
    const bool local = n->ext.local_feature != 0, jpm = n->ext.jpm != 0;
    if (local && !jpm) {
        // vit_pytorch.py:393-396 returns the tokens and nothing else: there is no cls feature and no neck output to write
        DALI_REQUIRE(tokens_out && !feat && !global_feat, "dali_vit_forward: a local_feature net without JPM writes only tokens_out (feat and global_feat must be null)");
    } else {
        DALI_REQUIRE(feat, "dali_vit_forward: null argument or net not bound");
    }
    DALI_REQUIRE(!tokens_out || local, "dali_vit_forward: tokens_out needs a local_feature net");
    DALI_REQUIRE(!(local && training), "dali_vit_forward: a local_feature / JPM net runs in eval mode only");
    DALI_REQUIRE(n->ext.n_sie == 0 || sie_idx, "dali_vit_forward: this net has SIE embeddings and needs the per-sample indices");
    hipStream_t st = (hipStream_t)stream;
    const int C = n->C, rows = n->rows;
    const float eps = 1e-6f;
    n->fwd_training = training != 0;
    int rc;
    if ((rc = launch_patchify(st, images, n->B, n->cfg.height, n->cfg.width, n->cfg.patch, n->cfg.stride, n->patches))) return rc;
    if ((rc = launch_linear_fwd(st, n->patches, n->patch.w, n->P + n->patch.b_off, 0, nullptr, n->pe, nullptr, nullptr, n->B * n->np, n->patch.K, C))) return rc;
    if (n->ext.n_sie > 0) {
        if ((rc = launch_assemble_tokens_sie(st, n->pe, n->P + n->cls_off, n->P + n->pos_off, n->P + n->sie_off, sie_idx, n->ext.n_sie, n->ext.sie_coef,
                                             n->B, n->T, C, n->x0))) return rc;
        if (training) n->sie_used = sie_idx;
    } else if ((rc = launch_assemble_tokens(st, n->pe, n->P + n->cls_off, n->P + n->pos_off, n->B, n->T, C, n->x0))) return rc;
    const uint16_t* x = n->x0;
    const float* dp = training ? n->dp_scale : nullptr;        // DropPath is the identity in eval mode (vit_pytorch.py:58)
    n->dp_used = dp;
    if (dp && (rc = launch_expand_rowscale(st, dp, 2 * (int)n->blocks.size(), n->B, n->T, n->dp_rows))) return rc;
    const int n_run = (int)n->blocks.size() - (local ? 1 : 0);          // local_feature: blocks[:-1] (vit_pytorch.py:393-396)
    for (int bi = 0; bi < n_run; ++bi) {
        VBlock& b = n->blocks[bi];
        if ((rc = run_block(n, st, b, x, rows, n->B, n->T, dp ? n->dp_rows + (size_t)(2 * bi) * rows : nullptr,
                            dp ? n->dp_rows + (size_t)(2 * bi + 1) * rows : nullptr, false))) return rc;
        x = b.x_out;
    }
    if (tokens_out && (rc = launch_tokens_f32(st, x, (size_t)rows * C, tokens_out))) return rc;
    if (local && !jpm) return DALI_OK;
    if (jpm) {
        // global branch (make_models.py:318-320): b1 on all tokens, its norm on the cls rows only
        if ((rc = run_block(n, st, n->b1, x, rows, n->B, n->T, nullptr, nullptr, false))) return rc;
        DALI_HIP(hipMemcpy2DAsync(n->cls_rows, (size_t)C * 2, n->b1.x_out, (size_t)n->T * C * 2, (size_t)C * 2, n->B, hipMemcpyDeviceToDevice, st));
        if ((rc = launch_layernorm_fwd(st, n->cls_rows, n->P + n->fin1.g_off, n->P + n->fin1.b_off, n->B, C, eps, nullptr, n->fin_mean, n->fin_rstd, n->gf))) return rc;
        if (global_feat) DALI_HIP(hipMemcpyAsync(global_feat, n->gf, (size_t)n->B * C * 4, hipMemcpyDeviceToDevice, st));
        // local branch (make_models.py:322-349): cls + each of the four runs of shuffled patch tokens through the shared b2
        const int seqs = n->ext.divide * n->B;
        if ((rc = launch_jpm_gather(st, x, n->map_dev, n->B, n->T, C, n->ext.divide, n->L, n->jseq))) return rc;
        if ((rc = run_block(n, st, n->b2, n->jseq, n->rows2, seqs, n->Tl, nullptr, nullptr, n->Tl <= 64))) return rc;
        DALI_HIP(hipMemcpy2DAsync(n->cls2, (size_t)C * 2, n->b2.x_out, (size_t)n->Tl * C * 2, (size_t)C * 2, seqs, hipMemcpyDeviceToDevice, st));
        if ((rc = launch_layernorm_fwd(st, n->cls2, n->P + n->fin2.g_off, n->P + n->fin2.b_off, seqs, C, eps, nullptr, n->fin2_mean, n->fin2_rstd, n->gf2))) return rc;
        JpmNecks nk;
        for (int i = 0; i < 5; ++i) { nk.gamma[i] = n->P + n->necks[i].g; nk.beta[i] = n->P + n->necks[i].b; nk.rm[i] = n->Bf + n->necks[i].rm; nk.rv[i] = n->Bf + n->necks[i].rv; }
        return launch_jpm_head(st, n->gf, n->gf2, nk, n->B, C, n->ext.neck_after, 1e-5f, feat);       // make_models.py:351-377
    }
    // final LayerNorm on the cls rows only (x[:, 0], vit_pytorch.py:401-403), then the BN neck (make_models.py:187)
    DALI_HIP(hipMemcpy2DAsync(n->cls_rows, (size_t)C * 2, x, (size_t)n->T * C * 2, (size_t)C * 2, n->B, hipMemcpyDeviceToDevice, st));
    if ((rc = launch_layernorm_fwd(st, n->cls_rows, n->P + n->fin.g_off, n->P + n->fin.b_off, n->B, C, eps, nullptr, n->fin_mean, n->fin_rstd, n->gf))) return rc;
    if (global_feat) DALI_HIP(hipMemcpyAsync(global_feat, n->gf, (size_t)n->B * C * 4, hipMemcpyDeviceToDevice, st));
    return launch_bn1d_fwd(st, n->gf, n->B, C, n->P + n->neck_g, n->P + n->neck_b, n->Bf + n->neck_rm, n->Bf + n->neck_rv, training ? 1 : 0, 0.1f,
                           1e-5f, feat, n->neck_mean, n->neck_invstd);
}

namespace {
int lin_bwd(dali_vit* n, hipStream_t st, const Lin& l, const uint16_t* x, const uint16_t* dy, const uint16_t* gelu_pre, uint16_t* dx, int rows) {
    int rc;
    if ((rc = launch_linear_wgrad(st, x, dy, n->G + l.w_off, rows, l.K, l.N, WGradBufs{n->slab, n->partial, n->scratch}, lin_dbias(n, l)))) return rc;
    if (dx) return launch_linear_fwd(st, dy, l.wt, nullptr, 0, nullptr, dx, nullptr, gelu_pre, rows, l.N, l.K);
    return DALI_OK;
}
}  // namespace

extern "C" int dali_vit_set_drop_path(dali_vit* n, const float* scales) {
    DALI_REQUIRE(n, "dali_vit_set_drop_path: null net");
    n->dp_scale = scales;
    return DALI_OK;
}

extern "C" int dali_vit_num_stages(const dali_vit* n) { return n ? n->n_stages : 0; }

// Flat-parameter element range whose gradients are complete once dali_vit_backward_stages has run through `stage`:
// stage 0 = final norm + fc + neck + the last group of blocks, ..., the last stage also holds cls / pos / patch embedding.
extern "C" int dali_vit_stage_param_range(const dali_vit* n, int stage, int64_t* begin, int64_t* end) {
    DALI_REQUIRE(n && begin && end && stage >= 0 && stage < n->n_stages, "dali_vit_stage_param_range: bad argument");
    const int lo = n->stage_first_block[stage + 1], hi = n->stage_first_block[stage];
    *begin = (stage == n->n_stages - 1) ? 0 : n->blocks[lo].n1.g_off;
    *end = (stage == 0) ? n->param_elems : n->blocks[hi].n1.g_off;
    return DALI_OK;
}

namespace {
// The three pieces of the backward; dali_vit_backward_stages and dali_debug_vit_backward_block both run exactly these, in this order.
// The gradient wrt the tokens entering a piece lives in gbuf[0] throughout.

// neck (bias frozen, make_models.py:181: no dbeta) + final LayerNorm (cls rows) -> gbuf[0] = dcls_rows at token 0 of every sample, 0 elsewhere
int bwd_head(dali_vit* n, hipStream_t st, const float* d_feat) {
    const int C = n->C;
    uint16_t* dx = n->gbuf[0];
    int rc;
    if ((rc = launch_bn1d_bwd(st, n->gf, d_feat, n->B, C, n->P + n->neck_g, n->neck_mean, n->neck_invstd, n->dgf, n->G + n->neck_g, nullptr))) return rc;
    if ((rc = launch_layernorm_bwd(st, nullptr, n->cls_rows, n->P + n->fin.g_off, n->fin_mean, n->fin_rstd, nullptr, n->B, C, n->dcls_rows,
                                   n->G + n->fin.g_off, n->G + n->fin.b_off, n->partial, n->scratch, n->dgf))) return rc;
    DALI_HIP(hipMemsetAsync(dx, 0, (size_t)n->rows * C * 2, st));
    DALI_HIP(hipMemcpy2DAsync(dx, (size_t)n->T * C * 2, n->dcls_rows, (size_t)C * 2, (size_t)C * 2, n->B, hipMemcpyDeviceToDevice, st));
    return DALI_OK;
}

// block i: gbuf[0] = d x_out  ->  gbuf[0] = d x_in, and the block's 12 parameter gradients
int bwd_block(dali_vit* n, hipStream_t st, int i) {
    const int C = n->C, rows = n->rows;
    const float* dp = n->dp_used;
    int rc;
    VBlock& b = n->blocks[i];
    uint16_t* dx = n->gbuf[0]; uint16_t* t1 = n->gbuf[1]; uint16_t* t2 = n->gbuf[2]; uint16_t* t3 = n->gbuf[3];
    const float* s_att = dp ? dp + (size_t)(2 * i) * n->B : nullptr;
    const float* s_mlp = dp ? dp + (size_t)(2 * i + 1) * n->B : nullptr;
    // x_out = x_mid + s_mlp * fc2(gelu(fc1(LN2(x_mid))))
    const uint16_t* d_branch = dx;
    if (dp) { if ((rc = launch_rowscale_add(st, dx, s_mlp, n->B, n->T, C, nullptr, t2))) return rc; d_branch = t2; }
    if ((rc = lin_bwd(n, st, b.fc2, b.act1, d_branch, b.pre1, t1, rows))) return rc;           // t1 = d_pre1 (GELU' fused)
    if ((rc = lin_bwd(n, st, b.fc1, b.h2, t1, nullptr, t2, rows))) return rc;                  // t2 = d_h2
    if ((rc = launch_layernorm_bwd(st, t2, b.x_mid, n->P + b.n2.g_off, b.n2.mean, b.n2.rstd, dx, rows, C, t3, n->G + b.n2.g_off,
                                   n->G + b.n2.b_off, n->partial, n->scratch))) return rc;     // t3 = dx_mid
    // x_mid = x_in + s_att * proj(attn(qkv(LN1(x_in))))
    d_branch = t3;
    if (dp) { if ((rc = launch_rowscale_add(st, t3, s_att, n->B, n->T, C, nullptr, t2))) return rc; d_branch = t2; }
    if ((rc = lin_bwd(n, st, b.proj, b.att, d_branch, nullptr, t1, rows))) return rc;          // t1 = d_att
    if ((rc = launch_attention_bwd(st, b.qkv_o, b.att, t1, b.lse, n->B, n->T, n->H, n->att_scale, t2))) return rc;   // t2 = d_qkv
    if ((rc = lin_bwd(n, st, b.qkv, b.h1, t2, nullptr, t1, rows))) return rc;                  // t1 = d_h1
    return launch_layernorm_bwd(st, t1, b.x_in, n->P + b.n1.g_off, b.n1.mean, b.n1.rstd, t3, rows, C, dx, n->G + b.n1.g_off,
                                n->G + b.n1.b_off, n->partial, n->scratch);                    // dx = dx_in
}

// tokens: d pos_embed, d cls_token, d patch embedding (gbuf[1] = the patch rows of gbuf[0]), d sie_embed
int bwd_tokens(dali_vit* n, hipStream_t st) {
    const int C = n->C;
    uint16_t* dx = n->gbuf[0];
    int rc;
    if ((rc = launch_assemble_tokens_bwd(st, dx, n->B, n->T, C, n->G + n->pos_off, n->G + n->cls_off, n->gbuf[1]))) return rc;
    if ((rc = lin_bwd(n, st, n->patch, n->patches, n->gbuf[1], nullptr, nullptr, n->B * n->np))) return rc;
    // d sie_embed from the same dx (every token of sample b carries coef * sie[idx[b]], vit_pytorch.py:382-387)
    if (n->ext.n_sie > 0) {
        DALI_REQUIRE(n->sie_used != nullptr, "dali_vit_backward: no SIE indices from the last training forward");
        if ((rc = launch_sie_grad(st, dx, n->sie_used, n->B, n->T, C, n->ext.n_sie, n->ext.sie_coef, n->G + n->sie_off))) return rc;
    }
    return DALI_OK;
}
}  // namespace

extern "C" int dali_vit_backward_stages(dali_vit* n, void* stream, const float* d_feat, int stage_begin, int stage_end) {
    DALI_REQUIRE(n, "dali_vit_backward: null argument or net not bound");
    { const int lim = refuse_long_training(n); if (lim) return lim; }
    DALI_REQUIRE(n->P && n->G, "dali_vit_backward: null argument or net not bound");
    DALI_REQUIRE(!n->ext.local_feature, "dali_vit_backward: a local_feature / JPM net is eval only (its train-mode forward feeds an ID loss that is out of scope)");
    DALI_REQUIRE(n->fwd_training, "dali_vit_backward: the last forward was not in training mode");
    DALI_REQUIRE(stage_begin >= 0 && stage_end < n->n_stages && stage_begin <= stage_end, "dali_vit_backward: bad stage range %d..%d", stage_begin, stage_end);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    for (int stage = stage_begin; stage <= stage_end; ++stage) {
        if (stage == 0) {
            DALI_REQUIRE(d_feat != nullptr, "dali_vit_backward: d_feat is null");
            if ((rc = bwd_head(n, st, d_feat))) return rc;
        }
        for (int i = n->stage_first_block[stage] - 1; i >= n->stage_first_block[stage + 1]; --i)
            if ((rc = bwd_block(n, st, i))) return rc;
        if (stage == n->n_stages - 1 && (rc = bwd_tokens(n, st))) return rc;
    }
    return DALI_OK;
}

// ---- diagnostics (include/daliid_debug.h) ----
extern "C" int dali_debug_vit_backward_block(dali_vit* n, void* stream, const float* d_feat, int block) {
    DALI_REQUIRE(n && n->P && n->G, "dali_debug_vit_backward_block: null argument or net not bound");
    { const int lim = refuse_long_training(n); if (lim) return lim; }
    DALI_REQUIRE(!n->ext.local_feature, "dali_debug_vit_backward_block: a local_feature / JPM net is eval only");
    DALI_REQUIRE(n->fwd_training, "dali_debug_vit_backward_block: the last forward was not in training mode");
    const int depth = (int)n->blocks.size();
    DALI_REQUIRE(block >= -1 && block <= depth, "dali_debug_vit_backward_block: block %d not in -1 .. %d", block, depth);
    hipStream_t st = (hipStream_t)stream;
    if (block == depth) {
        DALI_REQUIRE(d_feat != nullptr, "dali_debug_vit_backward_block: d_feat is null");
        return bwd_head(n, st, d_feat);
    }
    return block >= 0 ? bwd_block(n, st, block) : bwd_tokens(n, st);
}

// every name is declared where dali_vit_create_ex reserves the tensor; one that this plan did not reserve (dgrad images, DropPath rows, gradient
// buffers of an eval-only plan) was never bound and is refused like an unknown name
extern "C" int dali_debug_vit_tensor(const dali_vit* n, const char* name, void** ptr, int64_t* bytes) {
    DALI_REQUIRE(n && name && ptr && bytes, "dali_debug_vit_tensor: null argument");
    DALI_REQUIRE(n->arena, "dali_debug_vit_tensor: net not bound");
    return n->arena_tensor("dali_debug_vit_tensor", name, ptr, bytes);
}
extern "C" int dali_debug_vit_arena_entry(const dali_vit* n, int index, char* name, int name_cap, int64_t* offset, int64_t* bytes, int* reserved) {
    DALI_REQUIRE(n, "dali_debug_vit_arena_entry: null net");
    return n->arena_entry("dali_debug_vit_arena_entry", index, name, name_cap, offset, bytes, reserved);
}

extern "C" int dali_vit_backward(dali_vit* n, void* stream, const float* d_feat) {
    DALI_REQUIRE(n && d_feat, "dali_vit_backward: null argument");
    return dali_vit_backward_stages(n, stream, d_feat, 0, n->n_stages - 1);
}

"""GPU parity of the ViT-B/16 train step's kernels at the BENCHMARKED plan's own sizes (configs[3]: batch 128 of 224 x 224 images,
197 tokens, 25216 token rows; the patch embedding at 25088 rows): the five linears (forward in the plan's own epilogue combination,
data gradient as lin_bwd launches it, weight and bias gradient), the GELU / GELU' epilogues over every bf16 input on every epilogue
path, attention at B = 128 and at its NTILE instance boundaries, and the token plumbing (patchify, assemble_tokens and its backward).

Why beside tests/test_gpu_vit_ops.py: that file runs random data against a max-scaled tolerance (2^-7 |ref| + 4e-3 max |ref|), at
16500 rows and one (25216, 1024, 768) case that is not a ViT shape, and attention at B <= 3.  Tile configurations, the epilogue path a
row lands in (staged 256 x 320 column blocks, the half-tile "linear-layer extras" block, the general edge-tile path), the weight
gradient's split count and its column-sum share are functions of the plan's (rows, K, N); a deterministic indexing or epilogue error
confined to some tiles passes every property test of the full-size step.

Inputs of the linears are small integers (|x| <= 3, |w| <= 2 at density 1/2, integer bias and residual): every product and fp32 partial
sum is an integer below 2^24 (the longest: 3072 x 6 in fc2's forward, 25216 x 6 in a weight gradient), so every accumulator is exact in
any order and each output is the exact value rounded once to bf16 -- compared with torch.equal.  Rounding steps that are part of the
design (DropPath's fp32(1/0.9), GELU, GELU', attention's softmax) are emulated in float32 where the kernel's order of operations is
fixed (-ffp-contract=off), or bounded element-wise by the error of the kernel's own formula, derived next to each bound.  References
are integer, float32-on-integers (exact by the argument above) or fp64 host arithmetic, chunked so host memory stays at a few GB."""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
U = 2.0 ** -24                      # fp32 unit roundoff (half an ulp, relative)
U1 = 2.0 ** -23                     # one fp32 ulp, relative: the error of one fp32 operation that is not correctly rounded (v_exp_f32,
                                    # v_rcp_f32, log2f: 1 ulp each) or whose rounding inside an MFMA is not specified (any order, any mode)
HB = 2.0 ** -8                      # bf16 unit roundoff (half an ulp, relative)
ROWS = 128 * 197                    # 25216 token rows (ViT-B/16 at 224 x 224, batch 128): 98 full 256-row tiles + 128, 78 full 320-row tiles + 256
PROWS = 128 * 196                   # 25088 patch rows: 78 full 320-row tiles + 128
CHUNK_ROWS = 4096                   # host fp64 reference chunk (rows of a [rows, <= 3072] tensor)
FP32_INV_KEEP = float(np.float32(1.0 / 0.9))        # DropPath's keep factor as the plan's fp32 factor array holds it (drop rate 0.1)


@pytest.fixture(scope="module")
def V():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import ops_vit
    torch.set_num_threads(min(16, max(torch.get_num_threads(), 8)))
    return ops_vit


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(lo, hi, shape, gen, density=1.0):
    t = torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int8)
    if density < 1.0:
        t = t * (torch.rand(shape, generator=gen) < density).to(torch.int8)
    return t


def _halfulp_bf16(a):
    """half a bf16 ulp at magnitude |a| (float64 tensor in and out; bf16 keeps fp32's exponent range, subnormal spacing 2^-133)"""
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -126))            # |a| = m 2^e, m in [0.5, 1): the binade's ulp is 2^(e - 8)
    return torch.ldexp(torch.ones_like(a), e.to(a.dtype) - 9)


def _assert_within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                                        # NaN counts as bad
    if bad.any():
        i = int(torch.argmax(torch.where(bad, err - bound, torch.zeros_like(err)).flatten().nan_to_num(nan=1e300)))
        raise AssertionError("%s: %d elements off; worst at %d: got %r, ref %r, bound %r" % (
            what, int(bad.sum()), i, float(got.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i])))


def _equal(got, ref, what):
    got = got.cpu()
    if not torch.equal(got, ref):
        diff = got.float() != ref.float()
        i = int(torch.argmax(diff.flatten().int()))
        raise AssertionError("%s: %d elements differ; first at %d: got %r, ref %r" % (
            what, int(diff.sum()), i, float(got.flatten()[i]), float(ref.flatten()[i])))


# ---------------------------------------------------------------------------------------------------------------------------
# GELU / GELU' references and the bound of the kernel's formula (conv.hip gelu_parts)
# ---------------------------------------------------------------------------------------------------------------------------
def _phi_Phi(v):
    """fp64 phi(v), Phi(v) of a float64 tensor"""
    return torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi), 0.5 * torch.erfc(-v / math.sqrt(2.0))


# C_GELU: the absolute error of the kernel's cdf = Phi(v), in units of U (first order; each fp32 operation <= 1 ulp = 2 U):
#  - Abramowitz-Stegun 7.1.26 itself: |erf_AS - erf| <= 1.5e-7, halved in cdf = 0.5 + 0.5 erf:                                  1.3 U
#  - r = poly(t) t e approximates erfc(z) in [0, 1].  z = |v| fl(1/sqrt 2): 2 U relative.  e = exp2(-(z z) fl(log2 e)): the argument
#    carries 2 x 2 U (z^2) + 3 U (square, constant, product) = 7 U relative, i.e. 7 U z^2 absolute in the exponent, plus v_exp's 2 U;
#    r z^2 <= max erfc(z) z^2 < 0.17:                                                                                            r x 3.2 U
#  - t = rcp(fma(p, z, 1)): 2 U (rcp) + 1 U (fma) + 4 U (z) = 7 U relative; poly(t) t has condition number
#    sum k |a_k| t^k / |poly(t) t| <= 16.2 on t in (0, 1] (a_k the five A&S coefficients):                                       113 U
#  - Horner, 4 fmas: gamma_4 x sum |a_k| t^k / |poly t| <= 4 x 4.47 U:                                                            18 U
#  - the products poly t and (poly t) e: 2 x 2 U;  erf_abs = fma(-(poly t), e, 1): 1 U                                             5 U
#    (the bracket, 139.2 U of erf, is halved in the cdf)                                                                         69.6 U
#  - cdf = fma(0.5, erf, 0.5) rounded at |cdf| <= 1:                                                                               1 U
#  total 71.9 U -> 72.  gelu_f = fl(v cdf): |v| (72 + 1) U.  gelu_grad_f = fma(v, pdf, cdf): pdf = fl(fl(1/sqrt(2 pi)) e) carries
#  2 x 2 U + e's 7 U z^2 + 2 U; |v| phi(v) <= 0.242 and |v|^3 phi(v) / 2 <= 0.231 -> 0.242 x 6 U + 0.231 x 7 U = 3.1 U; the fma's
#  rounding at |g'| <= 1.13: 1.2 U.  72 + 3.1 + 1.2 -> 77 U.  Both constants are rounded up to 80 U.
C_GELU = 80.0
C_DGELU = 80.0


def _gelu_bound(v, ref, scale=1.0):
    """|got - ref| for got = bf16(fl(scale x g(v))), ref = scale x g64(v): the formula error E (C_GELU U |v|, at least C_GELU U: a
    product of |v| < 1 keeps the cdf's absolute error) times |scale| (a power of two: exact), plus half a bf16 ulp at |ref| + E
    (the fp32 value rounded to bf16 may sit up to E above |ref|)"""
    E = C_GELU * U * v.abs().clamp_min(1.0) * abs(scale)
    return _halfulp_bf16(ref.abs() + E) + E


def _dgelu_bound(ref, acc):
    """got = bf16(fl(acc x gelu_grad_f(v))), ref = acc x (Phi(v) + v phi(v)) in fp64, acc exact in fp32: |acc| x (C_DGELU U + U)"""
    E = (C_DGELU + 1.0) * U * acc.abs()
    return _halfulp_bf16(ref.abs() + E) + E


# ---------------------------------------------------------------------------------------------------------------------------
# 1: every ViT-B/16 linear at its plan size, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
# (name, rows, K, N).  Tile configuration (conv.hip conv_pick_cfg / conv_prefers_320, default environment) and epilogue paths:
#  patch 25088 x 768 -> 768, bias:  conv_prefers_320 -> 256 x 320 k-tile 64 (table entry K64_320: igemm_conv_ring_kernel, 16 waves of 64 x 80, Epi::LIN), 3 x 79 tiles; interior
#        tiles: the staged column-block store (conv_epilogue_cols), the last row tile (128 of 320 rows): the general path.
#  qkv   25216 x 768 -> 2304, bias:  256 x 256 k-tile 64 without linear extras (K64), 9 x 99 tiles; interior:
#        the lean staged store (bias folded), last row tile (128 of 256 rows): the general path.
#  proj  25216 x 768 -> 768, bias + residual + row_scale:  256 x 320 (as patch); columns store / general path (last tile: 256 of 320 rows).
#  fc1   25216 x 768 -> 3072, bias + GELU + O2:  256 x 256 k-tile 64 with linear extras (K64_LIN), 12 x 99
#        tiles; interior: the half-tile "linear-layer extras" block, last row tile: the general path.
#  fc2   25216 x 3072 -> 768, bias + residual + row_scale:  conv_pick_cfg says 256 x 256 (K >= 1024), conv_prefers_320 overrides it:
#        256 x 320, as proj.
# Data gradients (lin_bwd: dy [rows, N] against wt [K][N], Cm = K, reduction N): fc2 with gelu_pre (Cm 3072, reduction 768): 256 x 256
#  with linear extras, half-tile block + general path; fc1 (768, 3072), proj (768, 768), qkv (768, 2304): 256 x 320, columns store +
#  general path.  The patch embedding has no data gradient in the plan.
# Weight gradients (wgrad_pick_cfg 2: 128 x 256, wgrad_spec -> the pipelined igemm_wgrad_p_kernel<1,4,8,4,4,6,COLSUM>), splits from
#  wgrad_plan: qkv 4 (6304 rows each), proj 14 (13 x 1824 + 1504), fc1 3 (2 x 8416 + 8384), fc2 3 (as fc1), patch 14 (14 x 1792); the
#  slabs and the bias column sums (splits x K / 256 partial rows) reduced in one splitk_reduce_kernel<4> launch.  The bias gradient
#  always rides on the weight-gradient launch at these shapes (wgrad_colsum_supported: tensors below 2 GiB), so the column-sum
#  fallback (launch_colsum) is not reachable through dali_linear_wgrad here; want_bias=False runs the kernel without column sums.
LINEARS = [("patch", PROWS, 768, 768), ("qkv", ROWS, 768, 2304), ("proj", ROWS, 768, 768), ("fc1", ROWS, 768, 3072), ("fc2", ROWS, 3072, 768)]


def _row_factors(rows, T, gen):
    """per-row DropPath factors: one per sample of T rows, drawn from the plan's {0, fp32(1/0.9)} and powers of two"""
    choices = torch.tensor([0.0, FP32_INV_KEEP, FP32_INV_KEEP, 0.5, 1.0, 2.0, 0.25], dtype=torch.float32)
    per_sample = choices[torch.randint(0, len(choices), ((rows + T - 1) // T,), generator=gen)]
    return per_sample.repeat_interleave(T)[:rows].contiguous()


@pytest.mark.parametrize("case", LINEARS, ids=lambda c: c[0])
def test_vit_linear_exact_at_plan_size(V, case):
    name, rows, K, N = case
    gen = _gen("lin", name)
    x = _ints(-3, 3, (rows, K), gen)
    w = _ints(-2, 2, (N, K), gen, density=0.5)
    bias = _ints(-8, 8, (N,), gen).float()
    xg, wg, bg = x.cuda().to(bf16), w.cuda().to(bf16), bias.cuda()
    acc = x.float() @ w.float().t()                   # integers below 2^24: float32 is exact in any summation order
    pre = acc + bias                                  # exact

    # ---- forward, in the plan's epilogue combination ----
    if name in ("patch", "qkv"):
        _equal(V.linear_fwd(xg, wg, bg), pre.to(bf16), name + " forward (bias)")
    elif name == "fc1":
        y, pre_k = V.linear_fwd(xg, wg, bg, act=1, want_pre=True)
        _equal(pre_k, pre.to(bf16), "fc1 pre-activation copy (O2)")
        y = y.cpu()
        for r0 in range(0, rows, CHUNK_ROWS):
            v = pre[r0:r0 + CHUNK_ROWS].double()
            ref = v * _phi_Phi(v)[1]
            _assert_within(y[r0:r0 + CHUNK_ROWS].double(), ref, _gelu_bound(v, ref), "fc1 forward GELU")
        del y, pre_k
    else:                                             # proj / fc2: bias + residual + DropPath row factor (vit_pytorch.py:338)
        res = _ints(-16, 16, (rows, N), gen).float()
        rs = _row_factors(rows, 197, gen)
        y = V.linear_fwd_scaled(xg, wg, rs.cuda(), bias=bg, residual=res.cuda().to(bf16))
        # the documented order, one fp32 rounding per operation (bias add exact): ((acc + bias) x rs) + res, then bf16
        _equal(y, (pre * rs[:, None] + res).to(bf16), name + " forward (bias, row factor, residual)")
        y = V.linear_fwd(xg, wg, bg, residual=res.cuda().to(bf16))          # eval mode: DropPath is the identity
        _equal(y, (pre + res).to(bf16), name + " forward (bias, residual)")
        del y, res
    del pre

    # ---- data gradient, as lin_bwd launches it: dy [rows, N] against the transposed weight image [K][N] ----
    if name != "patch":
        dy = _ints(-2, 2, (rows, N), gen)
        dyg = dy.cuda().to(bf16)
        wt = wg.t().contiguous()
        dacc = dy.float() @ w.float()                 # [rows, K], exact
        if name == "fc2":                             # d h1 = (d o @ W2) x gelu'(pre1): fc1's pre-activation as the GELU' argument
            pre1 = (torch.randn(rows, K, generator=gen) * 2).to(bf16)
            dx = V.linear_dgrad(dyg, wt, gelu_pre=pre1.cuda()).cpu()
            for r0 in range(0, rows, CHUNK_ROWS):
                v, a = pre1[r0:r0 + CHUNK_ROWS].double(), dacc[r0:r0 + CHUNK_ROWS].double()
                phi, Phi = _phi_Phi(v)
                ref = a * (Phi + v * phi)
                _assert_within(dx[r0:r0 + CHUNK_ROWS].double(), ref, _dgelu_bound(ref, a), "fc2 data gradient x GELU'")
            del pre1
        else:
            dx = V.linear_dgrad(dyg, wt)
            _equal(dx, dacc.to(bf16), name + " data gradient")
        del dx, dacc, wt
    else:
        dy = _ints(-2, 2, (rows, N), gen)
        dyg = dy.cuda().to(bf16)

    # ---- weight gradient (fp32) and bias gradient: dw = dy^T x <= 25216 x 6 < 2^24, db = sum dy: exact ----
    dw_ref = dy.float().t() @ x.float()
    db_ref = dy.sum(0, dtype=torch.int64).float()
    dw, db = V.linear_wgrad(xg, dyg)
    _equal(dw, dw_ref, name + " weight gradient (column sums riding)")
    _equal(db, db_ref, name + " bias gradient")
    dw2 = V.linear_wgrad(xg, dyg, want_bias=False)
    _equal(dw2, dw_ref, name + " weight gradient (no column sums)")


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the GELU and GELU' epilogues over every bf16 input on every path
# ---------------------------------------------------------------------------------------------------------------------------
def _sweep_values():
    """every finite bf16 value in [-12, 12] (subnormals and both zeros included), as float32"""
    b = (torch.arange(65536, dtype=torch.int32) << 16).view(torch.float32)
    b = b[torch.isfinite(b) & (b.abs() <= 12)]
    return b


def _sweep_layout(rows, cols, n, gen):
    """[rows, cols] indices into the n sweep values: random, except that the first rows and the last 128 rows each hold every value
    (the last 128 rows are inside the last row tile of both the 256-row and the 320-row configurations: the general path)"""
    idx = torch.randint(0, n, (rows, cols), generator=gen)
    head = (n + cols - 1) // cols
    assert 128 * cols >= n
    idx[:head] = (torch.arange(head * cols) % n).reshape(head, cols)
    idx[-128:] = (torch.randperm(128 * cols, generator=gen) % n).reshape(128, cols)
    return idx


def _same_bits_per_value(keys, vals, n, what):
    """every occurrence of a key carries the same bits (int32 tensors on the device)"""
    canon = torch.zeros(n, dtype=vals.dtype, device=vals.device)
    canon[keys] = vals                                            # one arbitrary occurrence per key
    bad = canon[keys] != vals
    assert not bad.any(), "%s: %d outputs differ from another occurrence of the same input (first at %d)" % (
        what, int(bad.sum()), int(torch.argmax(bad.int())))


def test_gelu_epilogue_every_bf16_input_every_path(V):
    """acc = the swept value exactly (w picks one input column, bias 0): fc1's shape (half-tile extras block + general edge tile) and a
    768-output act=1 launch (256 x 320 columns store + general edge tile).  Each value against the fp64 GELU within the formula's
    bound, and the same bits for the same value on every path"""
    vals = _sweep_values()
    n = vals.numel()
    gen = _gen("gelu-sweep")
    idx = _sweep_layout(ROWS, 768, n, gen)
    x = vals[idx].to(bf16).cuda()                                 # exact: the values are bf16
    v64 = vals.double()
    phi, Phi = _phi_Phi(v64)
    g64 = (v64 * Phi).cuda()
    bound = _gelu_bound(v64, v64 * Phi).cuda()
    idx_g = idx.cuda()
    keys, bits = [], []
    for N in (3072, 768):
        w = torch.zeros(N, 768, dtype=bf16, device="cuda")
        w[torch.arange(N), torch.arange(N) % 768] = 1.0
        y, pre = V.linear_fwd(x, w, torch.zeros(N, device="cuda"), act=1, want_pre=True)
        k = idx_g.repeat(1, N // 768)                             # output channel c carries input column c % 768
        normal = vals.abs().cuda()[k] >= 2.0 ** -126              # (subnormal inputs: the MFMA's handling is not the epilogue's business)
        assert torch.equal(pre.float()[normal], vals.cuda()[k][normal]), "N %d: pre-activation copy is not the input" % N
        _assert_within(y.double(), g64[k], bound[k], "GELU sweep, N %d" % N)
        keys.append(k.flatten())
        bits.append(y.view(torch.int16).flatten().int())
        del y, pre, normal, w
    _same_bits_per_value(torch.cat(keys), torch.cat(bits), n, "GELU across epilogue paths")


def test_gelu_grad_epilogue_every_bf16_input_every_path(V):
    """fc2's data gradient (Cm 3072: half-tile extras block + general edge tile) and a 768-output one (256 x 320 columns store + general
    edge tile) with gelu_pre = the sweep and dy wt^T = a power of two per channel (dy's column 0 is 1, wt's column 0 holds +-2^s)"""
    vals = _sweep_values()
    n = vals.numel()
    gen = _gen("dgelu-sweep")
    v64 = vals.double()
    phi, Phi = _phi_Phi(v64)
    d64 = (Phi + v64 * phi).cuda()
    keys, bits = [], []
    for K, Nred in ((3072, 768), (768, 3072)):                   # (output channels, reduction): fc2's dgrad, fc1's dgrad shape
        idx = _sweep_layout(ROWS, K, n, gen).cuda()
        pre = vals.cuda()[idx].to(bf16)
        dy = torch.zeros(ROWS, Nred, dtype=bf16, device="cuda")
        dy[:, 0] = 1.0
        s = (2.0 ** torch.randint(-2, 2, (K,), generator=gen).double()) * (1 - 2 * torch.randint(0, 2, (K,), generator=gen)).double()
        wt = torch.zeros(K, Nred, dtype=bf16, device="cuda")
        wt[:, 0] = s.float().cuda().to(bf16)
        dx = V.linear_dgrad(dy, wt, gelu_pre=pre)
        sg = s.cuda()
        ref = d64[idx] * sg
        _assert_within(dx.double(), ref, _dgelu_bound(ref, sg.expand_as(ref)), "GELU' sweep, %d outputs" % K)
        keys.append(idx.flatten())
        bits.append((dx.float() / sg.float()).view(torch.int32).flatten())      # / +-2^s: exact, so equal values carry equal bits
        del idx, pre, dy, wt, dx, ref
    _same_bits_per_value(torch.cat(keys), torch.cat(bits), n, "GELU' across epilogue paths")


# ---------------------------------------------------------------------------------------------------------------------------
# 3: attention at plan sizes and at its instance boundaries
# ---------------------------------------------------------------------------------------------------------------------------
SCALE = 0.125                       # head_dim 64 -> 64^-0.5, a power of two


def _att_inputs(B, T, H, seed):
    """qkv [B*T, 3C] bf16 and d_out [B*T, C]; the kind of each (sequence, head) problem is (b H + h) % 4:
    0 random; 1 q, k x 3.7 (scaled scores of std ~14, spanning about +-60); 2 every key of the problem equal (a row of equal scores);
    3 one dominant key (q >= 0, k* = 2: score ~13 above the rest, p ~ 1), the last real key on even problems"""
    g = _gen("att", B, T, H, seed)
    q = torch.randn(B, H, T, 64, generator=g)
    k = torch.randn(B, H, T, 64, generator=g)
    v = torch.randn(B, H, T, 64, generator=g)
    kind = (torch.arange(B)[:, None] * H + torch.arange(H)[None, :]) % 4
    wide = kind == 1
    q[wide] *= 3.7
    k[wide] *= 3.7
    eq = kind == 2
    k[eq] = k[eq][:, :1].expand(-1, T, -1).clone()
    dom = (kind == 3).nonzero().tolist()
    for b, h in dom:
        q[b, h] = q[b, h].abs()
        k[b, h] *= 0.5
        j = T - 1 if (b * H + h) % 8 == 3 else int(torch.randint(0, T, (1,), generator=g))
        k[b, h, j] = 2.0
    qkv = torch.stack([q, k, v], 2).to(bf16)                     # [B, H, 3, T, 64]
    qkv = qkv.permute(0, 3, 2, 1, 4).reshape(B * T, 3 * H * 64).contiguous()     # vit_pytorch.py:155 layout
    d_out = torch.randn(B * T, H * 64, generator=g).to(bf16)
    return qkv, d_out


def _heads(t, B, T, H, part):
    """[B*T, 3C] (or [B*T, C] with part None) -> fp64 [B, H, T, 64]"""
    if part is None:
        return t.reshape(B, T, H, 64).permute(0, 2, 1, 3).double()
    return t.reshape(B, T, 3, H, 64)[:, :, part].permute(0, 2, 1, 3).double()


def _check_attention(qkv, d_out, out_k, lse_k, dqkv_k, B, T, H, what, chunk=16):
    """fp64 softmax attention on the same bf16 q, k, v; per-element bounds from the kernels' rounding steps (vit_ops.hip:483-700)."""
    FLOOR = 2.0 ** -100             # flushed subnormals: p < 2^-126 per term, T <= 256 terms, operands < 2^6 -> < 2^-112
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        r0, r1 = b0 * T, b1 * T
        nb = b1 - b0
        q, k, v = (_heads(qkv[r0:r1], nb, T, H, i) for i in range(3))
        dO = _heads(d_out[r0:r1], nb, T, H, None)
        oK = _heads(out_k[r0:r1].float(), nb, T, H, None)
        x = SCALE * (q @ k.transpose(-1, -2))                     # [nb, H, T, T] natural-log scores
        lse = torch.logsumexp(x, -1)
        p = torch.exp(x - lse[..., None])
        o = p @ v
        # Gm_i >= |x_ij| for every j: the score magnitudes that scale the fp32 errors of the scores
        Gm = (SCALE * (q.abs() @ k.abs().transpose(-1, -2))).amax(-1)
        # ---- forward (attention_fwd2_kernel) ----
        # score S = q.k by MFMA: 64 U1 G;  t = fl(S sc2) with sc2 = scale fl(log2 e): U1 |x|;  fl(t - m): U1/2 |t - m| <= U1 Gm (natural
        # units);  v_exp_f32: U1.  -> eta = 66 U1 Gm + U1 per exponential (relative).  p = e / l with l = sum of T positive terms (T U1),
        # 1 / l and e x inv_l (U1 each); the max term cancels in the ratio but each e_j and l carry their own: eps_p = 2 eta + (T + 2) U1.
        eta = 66 * U1 * Gm + U1
        eps_p = 2 * eta + (T + 2) * U1
        # p rounded to bf16 for the PV MFMA (HB relative), T products summed in fp32 (T U1); the output rounded once to bf16.
        # 1.01 covers the second-order products of these relative errors (each < 2^-7).
        E_o = 1.01 * (HB + eps_p + T * U1)[..., None] * (p @ v.abs()) + FLOOR
        ok = oK.double()
        _assert_within(ok, o, E_o + _halfulp_bf16(o.abs() + E_o), "%s: attention output" % what)
        # lse = fl(fl(m + fl(log2f(l))) ln2): m = t_max carries 65 U1 Gm (score, scaling); l's relative error (each e_j vs the exact
        # exp(x_j - x_max): 2 x 65 U1 Gm + U1 Gm + U1, plus T U1 for the sum) enters as itself; log2f: 1 ulp of <= 8 -> 8 U1; the add and
        # the product with fl(ln 2): U1 (|lse| + 8) together.  -> U1 (197 Gm + T + 17 + |lse|), rounded up below.
        lse_b = U1 * (200 * Gm + T + 20 + 2 * lse.abs())
        lk = lse_k[b0 * H:b1 * H].double().reshape(nb, H, T)
        _assert_within(lk, lse, lse_b, "%s: attention lse" % what)
        # ---- backward (attention_bwd_dq_kernel / attention_bwd_dkv_kernel), on the kernel's own o (D = rowsum(dO o) is defined on the
        # stored output) and lse ----
        # p = exp2(fl(fl(S sc2) - fl(lse fl(log2 e)))): score 65 U1 G; lse's bound above; lq's rounding U1 |lse|; the subtraction
        # U1/2 |t - lq| <= U1 (Gm + |lse|); v_exp: U1.
        eta_b = (66 * U1 * Gm + lse_b + U1 * (2 * lse.abs() + Gm) + U1)[..., None]
        dP = dO @ v.transpose(-1, -2)
        D = (dO * ok).sum(-1, keepdim=True)
        A = dO.abs() @ v.abs().transpose(-1, -2)                  # dP's MFMA sum of 64 products: 64 U1 A
        Bd = (dO.abs() * ok.abs()).sum(-1, keepdim=True)          # D's fp32 sum of 64 products: 64 U1 B
        dS = SCALE * p * (dP - D)
        # dS = fl(fl(p fl(dP - D)) scale): p's eta_b, the subtraction and the product (U1 together), the sums' 64 U1 (A + B); then
        # rounded to bf16 (HB) as the A operand of dQ = dS K and dK = dS^T Q
        Wd = 1.01 * SCALE * p * ((HB + eta_b + U1) * (dP - D).abs() + 64 * U1 * (A + Bd))
        dSa = dS.abs()
        dq = dS @ k
        E_dq = Wd @ k.abs() + 1.01 * T * U1 * (dSa @ k.abs()) + FLOOR
        dk = dS.transpose(-1, -2) @ q
        E_dk = Wd.transpose(-1, -2) @ q.abs() + 1.01 * T * U1 * (dSa.transpose(-1, -2) @ q.abs()) + FLOOR
        # dV = P^T dO: p (eta_b) rounded to bf16 (HB), T products summed in fp32
        dv = p.transpose(-1, -2) @ dO
        E_dv = 1.01 * ((HB + eta_b) * p).transpose(-1, -2) @ dO.abs() + 1.01 * T * U1 * (p.transpose(-1, -2) @ dO.abs()) + FLOOR
        for part, ref, E, nm in ((0, dq, E_dq, "dq"), (1, dk, E_dk, "dk"), (2, dv, E_dv, "dv")):
            got = _heads(dqkv_k[r0:r1].float(), nb, T, H, part)
            _assert_within(got, ref, E + _halfulp_bf16(ref.abs() + E), "%s: attention %s" % (what, nm))


def _run_attention(V, B, T, H, seed=0):
    qkv, d_out = _att_inputs(B, T, H, seed)
    out, lse = V.attention_fwd(qkv.cuda(), B, T, H)
    dqkv = V.attention_bwd(qkv.cuda(), out, d_out.cuda(), lse, B, T, H)
    _check_attention(qkv, d_out, out.cpu(), lse.cpu(), dqkv.cpu(), B, T, H, "B %d T %d H %d" % (B, T, H))


# 197 tokens = configs[3] (ViT-B/16 at 224 x 224); 211 = TransReID at 256 x 128, stride 12 (vit_pytorch.py:254-267).  At B = 128 the keys
# padded beyond T in each problem's last tile sit next to the following sequence's tokens in memory.
@pytest.mark.parametrize("T", [197, 211])
def test_attention_plan_batch(V, T):
    _run_attention(V, 128, T, 12)


# NTILE instances: T <= 208 -> 13 tiles, 209..224 -> 14, 225..256 -> 16; T = 1, 16, 17: a single (ragged) tile and the first tile edge
@pytest.mark.parametrize("T", [1, 16, 17, 208, 209, 224, 225, 256])
def test_attention_instance_boundaries(V, T):
    _run_attention(V, 2, T, 4, seed=T)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: token plumbing at plan size, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,stride", [((224, 224), 16), ((256, 128), 12)], ids=["224x224_s16", "256x128_s12"])
def test_patchify_plan_batch(V, hw, stride):
    g = _gen("patchify", hw, stride)
    img = torch.randn(128, 3, hw[0], hw[1], generator=g) * 3
    p = V.patchify(img.cuda(), 16, stride)
    ref = F.unfold(img.to(bf16).float(), 16, stride=stride).transpose(1, 2).reshape(-1, 3 * 16 * 16).to(bf16)
    _equal(p, ref, "patchify %s stride %d" % (hw, stride))


@pytest.mark.parametrize("T", [197, 211])
def test_assemble_tokens_plan_batch(V, T):
    B, C = 128, 768
    g = _gen("tokens", T)
    pe = torch.randn(B * (T - 1), C, generator=g).to(bf16)
    cls, pos = torch.randn(C, generator=g), torch.randn(T, C, generator=g)
    x = V.assemble_tokens(pe.cuda(), cls.cuda(), pos.cuda(), B, T)
    # one fp32 add (pe's bf16 value or cls, plus pos), then one rounding to bf16
    ref = (torch.cat((cls.expand(B, 1, C), pe.float().reshape(B, T - 1, C)), 1) + pos).reshape(B * T, C).to(bf16)
    _equal(x, ref, "assemble_tokens T %d" % T)
    # backward on integers: dpos / dcls are sums over 128 images of |dx| <= 8 (exact in fp32), dpe an exact copy
    dx = _ints(-8, 8, (B * T, C), g).to(bf16)
    dpos, dcls, dpe = V.assemble_tokens_bwd(dx.cuda(), B, T)
    s = dx.float().reshape(B, T, C).sum(0)
    _equal(dpos, s, "assemble_tokens_bwd dpos")
    _equal(dcls, s[0], "assemble_tokens_bwd dcls")
    _equal(dpe, dx.reshape(B, T, C)[:, 1:].reshape(B * (T - 1), C), "assemble_tokens_bwd dpe")

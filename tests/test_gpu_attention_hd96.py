"""The chunked attention forward at head_dim 96 (attention_fwd_long_kernel<96, 128>: key chunks of 128 under an online softmax), the one kernel
that serves EVERY head-dim-96 length from 1 to 1024 tokens, through the three forward entries of ops_vit.

Compared with torch CPU fp32 attention on the same bf16-rounded qkv, by the criteria of tests/test_gpu_vit_long.py: output
|err| <= 2^-7 |ref| + 4e-3 max|ref|, lse rtol = atol = 1e-4.  Both scales ViT-Small could be given: 96 ** -0.5 (the head width's) and
768 ** -0.5 (the one the reference uses, vit_pytorch.py:462)."""
import numpy as np
import pytest
import torch

bf16 = torch.bfloat16
pytestmark = pytest.mark.gpu
HD = 96
SCALES = [96 ** -0.5, 768 ** -0.5]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def close(got, ref, rel=2.0 ** -7, abs_frac=4e-3):
    got, ref = got.float().cpu(), ref.float()
    err = (got - ref).abs()
    tol = rel * ref.abs() + abs_frac * ref.abs().max()
    assert (err <= tol).all(), "max err %.4g (ref scale %.4g), worst err / tol %.3f" % (float(err.max()), float(ref.abs().max()), float((err / tol).max()))


def _qkv(B, T, H, hd=HD, seed=None):
    g = torch.Generator().manual_seed(B * 1000 + T + H if seed is None else seed)
    return torch.randn(B * T, 3 * H * hd, generator=g)


def _ref_attention(qkv, B, T, H, scale, hd=HD):
    """fp32 attention and row log-sum-exp on the bf16-rounded qkv (vit_pytorch.py:155 layout)"""
    t = qkv.to(bf16).float().reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (t[0] @ t[1].transpose(-2, -1)) * scale
    out = (s.softmax(dim=-1) @ t[2]).transpose(1, 2).reshape(B * T, H * hd)
    return out, torch.logsumexp(s, dim=-1).reshape(B * H, T)


def _check(fn, qkv, B, T, H, scale, hd=HD):
    ref, ref_lse = _ref_attention(qkv, B, T, H, scale, hd)
    out, lse = fn(qkv.to(bf16).cuda(), B, T, H, scale)
    assert out.shape == (B * T, H * hd) and lse.shape == (B * H, T)
    close(out, ref)
    np.testing.assert_allclose(lse.cpu().numpy(), ref_lse.numpy(), rtol=1e-4, atol=1e-4)


# (2, 1, 2): one live query of 128; 16 / 17: a tile edge; (8, 33, 8): a JPM run; (2, 128, 2): exactly one chunk; (2, 129, 8): ViT-Small at 256x128 /
# stride 16, one key in the second chunk and one query in the second query block; 211: stride 12; 256 / 257: a chunk edge; (2, 311, 8): 384x128 at
# stride 12; (3, 385, 2): three sequences adjacent in memory, one key in the fourth chunk; (1, 1024, 1): the cap, eight full chunks
@pytest.mark.parametrize("scale", SCALES, ids=["hd", "dim"])
@pytest.mark.parametrize("B,T,H", [(2, 1, 2), (2, 16, 2), (2, 17, 2), (8, 33, 8), (2, 128, 2), (2, 129, 8), (2, 211, 2), (2, 256, 2), (2, 257, 2),
                                   (2, 311, 8), (3, 385, 2), (1, 1024, 1)])
def test_attention_fwd_head_dim_96(B, T, H, scale):
    _need_gpu()
    from daliid_amd import ops_vit
    _check(ops_vit.attention_fwd, _qkv(B, T, H), B, T, H, scale)


@pytest.mark.parametrize("scale", SCALES, ids=["hd", "dim"])
@pytest.mark.parametrize("T", [1, 17, 129])
def test_attention_fwd_long_entry_head_dim_96(T, scale):
    _need_gpu()
    from daliid_amd import ops_vit
    _check(ops_vit.attention_fwd_long, _qkv(2, T, 4), 2, T, 4, scale)


@pytest.mark.parametrize("scale", SCALES, ids=["hd", "dim"])
@pytest.mark.parametrize("T", [33, 53, 64])
def test_attention_fwd_short_entry_head_dim_96(T, scale):
    _need_gpu()
    from daliid_amd import ops_vit
    _check(ops_vit.attention_fwd_short, _qkv(8, T, 8), 8, T, 8, scale)


# the running maximum has to move in both directions across a 128-key chunk: keys of the last chunk (rows >= 256) times 4 -> every row's maximum
# moves there and everything accumulated before is scaled down; keys of the first tile times 4 -> the first chunk dominates, alpha = 1 afterwards
@pytest.mark.parametrize("scale", SCALES, ids=["hd", "dim"])
@pytest.mark.parametrize("which", ["last_chunk", "first_tile"])
def test_attention_hd96_rescales_in_both_directions(which, scale):
    _need_gpu()
    from daliid_amd import ops_vit
    B, T, H = 2, 257, 2
    C = H * HD
    qkv = _qkv(B, T, H).reshape(B, T, 3 * C).clone()
    if which == "last_chunk":
        qkv[:, 256:, C:2 * C] *= 4
    else:
        qkv[:, :16, C:2 * C] *= 4
    _check(ops_vit.attention_fwd, qkv.reshape(B * T, 3 * C), B, T, H, scale)


def test_attention_hd96_without_lse_is_bitwise_the_same():
    _need_gpu()
    from daliid_amd import ops_vit
    B, T, H = 2, 211, 2
    qkv = _qkv(B, T, H).to(bf16).cuda()
    out, lse = ops_vit.attention_fwd_long(qkv, B, T, H, 768 ** -0.5)
    out2, none = ops_vit.attention_fwd_long(qkv, B, T, H, 768 ** -0.5, with_lse=False)
    assert none is None and lse is not None
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


def test_other_widths_and_lengths_are_refused_without_a_launch_and_head_dim_64_still_runs():
    _need_gpu()
    from daliid_amd import _lib, ops_vit
    for hd in (32, 128):
        qkv = torch.zeros(16, 3 * hd, dtype=bf16, device="cuda")
        for fn in (ops_vit.attention_fwd, ops_vit.attention_fwd_long, ops_vit.attention_fwd_short):
            with pytest.raises(_lib.DaliError, match=r"head_dim must be 64 or 96 \(got %d\)" % hd):
                fn(qkv, 1, 16, 1)
    qkv = torch.zeros(1025, 3 * HD, dtype=bf16, device="cuda")
    for fn in (ops_vit.attention_fwd, ops_vit.attention_fwd_long):
        with pytest.raises(_lib.DaliError, match="1025 tokens exceed the limit of 1024"):
            fn(qkv, 1, 1025, 1)
    with pytest.raises(_lib.DaliError, match="64"):
        ops_vit.attention_fwd_short(qkv[:65], 1, 65, 1)
    # no backward at head_dim 96
    q = torch.zeros(16, 3 * HD, dtype=bf16, device="cuda")
    o = torch.zeros(16, HD, dtype=bf16, device="cuda")
    with pytest.raises(_lib.DaliError, match="head_dim must be 64"):
        ops_vit.attention_bwd(q, o, o, torch.zeros(1, 16, device="cuda"), 1, 16, 1)
    torch.cuda.synchronize()
    # and the head-dim-64 entries are what they were
    for fn, T in ((ops_vit.attention_fwd, 197), (ops_vit.attention_fwd_long, 257), (ops_vit.attention_fwd_short, 33)):
        _check(fn, _qkv(2, T, 2, hd=64), 2, T, 2, 0.125, hd=64)

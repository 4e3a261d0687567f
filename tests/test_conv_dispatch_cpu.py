"""CPU: which entry of the kernel table (daliid_amd/csrc/conv.hip, GemmKernel::name) each forward / data-gradient / linear-layer GEMM of the GPU
parity tests is launched on, through dali_debug_conv_kernel_name with 256 CUs: the launcher's parity split and conv_choose, no launch.

The problems are the ones the bit-exact GPU tests run -- every convolution of test_gpu_conv_plan_shapes.PLAN (forward with statistics, the
fused BatchNorm + ReLU forward, the data gradient with a masked residual), the ViT linears of test_gpu_vit_plan_shapes.LINEARS in the
plan's epilogue combinations, the cases of test_gpu_conv.py whose comments name a kernel, and test_gpu_conv_ring.CASES -- so the names
below say which kernel instantiation each of those tests proves.  The expected names were recorded from the commit before the three
LDS-DMA kernel templates became igemm_conv_ring_kernel (the same export added to a scratch build of it); a change of the chooser that
moves a problem to another entry has to change this table, and with it the claim of the GPU test's comment.  Together the problems
reach every instantiation of igemm_conv_ring_kernel (RING), so that none of them is launched by the library and proven by no test."""
import ctypes

import pytest

from daliid_amd import _lib
from test_gpu_conv import CASES
from test_gpu_conv_plan_shapes import N, PLAN
from test_gpu_conv_ring import CASES as RING_CASES
from test_gpu_vit_plan_shapes import LINEARS

STATS, FUSED, RES, RES_MASK, OUT_MASK, BITS, LIN = 1, 2, 4, 8, 16, 32, 64           # include/daliid_debug.h
N_CUS = 256

RING = {"DMA128", "DMA128_LIN", "DMA128_FUSED", "DMA128_CLS", "DMA128_SRC2", "DMA64", "DMA64_LEAN", "DMA64_SRC2", "WG128", "WG128_LIN",
        "WG128_FUSED", "WG128_CLS", "WG256", "K64", "K64_LIN", "K64_FUSED", "K64_CLS", "K64_SRC2", "K64_FUSED_SRC2", "K64_320"}


def _out(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


def fwd(n, h, w, cin, cout, r, s, stride, pad, flags=0):
    return dict(Cm=cout, P=n * _out(h, r, stride, pad) * _out(w, s, stride, pad), h=h, wd=w, ck=cin, r=r, s=s, stride=stride, pad=pad, mode=0, flags=flags)


def dgrad(n, h, w, cin, cout, r, s, stride, pad, flags=0):
    return dict(Cm=cin, P=n * h * w, h=h, wd=w, ck=cout, r=r, s=s, stride=stride, pad=pad, mode=1, flags=flags)


def linear(rows, K, Nout, flags=0, ck1=0, x_rep=0):
    return dict(Cm=Nout, P=rows, h=1, wd=1, ck=K, r=1, s=1, stride=1, pad=0, mode=0, flags=flags, ck1=ck1, x_rep=x_rep)


def _problems():
    p = {}
    for h, w, cin, cout, r, stride, pad in PLAN:                      # test_plan_conv_exact_at_batch_256's three GEMM launches
        key = "plan %dx%d_%d-%d_k%d_s%d " % (h, w, cin, cout, r, stride)
        p[key + "fwd+stats"] = fwd(N, h, w, cin, cout, r, r, stride, pad, STATS)
        p[key + "fwd bn_act"] = fwd(N, h, w, cin, cout, r, r, stride, pad, FUSED)
        p[key + "dgrad+masked residual"] = dgrad(N, h, w, cin, cout, r, r, stride, pad, RES | RES_MASK)
    for name, rows, K, Nout in LINEARS:                               # test_vit_linear_exact_at_plan_size
        if name in ("patch", "qkv"):
            p["vit %s fwd" % name] = linear(rows, K, Nout)
        elif name == "fc1":
            p["vit fc1 fwd gelu"] = linear(rows, K, Nout, LIN)
        else:
            p["vit %s fwd row_scale+residual" % name] = linear(rows, K, Nout, LIN | RES)
            p["vit %s fwd residual" % name] = linear(rows, K, Nout, RES)
        if name != "patch":
            p["vit %s dgrad" % name] = linear(rows, Nout, K, LIN if name == "fc2" else 0)
    for i in (1, 14, 15, 16, 17, 18, 19, 20, 21, 22):                 # test_conv_fwd_dgrad_wgrad_exact_integers: the cases whose comments name a kernel
        p["conv case %d fwd+stats" % i] = fwd(*CASES[i], flags=STATS)
        p["conv case %d dgrad" % i] = dgrad(*CASES[i])
        p["conv case %d dgrad+masked residual" % i] = dgrad(*CASES[i], flags=RES | RES_MASK)
    for P, c1, c2, cout in [(777, 256, 64, 64), (1000, 512, 128, 128), (300, 64, 32, 24), (16640, 1024, 256, 256), (16500, 2048, 512, 512),
                            (16384, 1024, 64, 128), (16384, 448, 64, 256), (20000, 512, 256, 512)]:          # test_conv1x1_two_operand_tensors_exact_integers
        p["cat %d_%d+%d-%d" % (P, c1, c2, cout)] = linear(P, c1 + c2, cout, ck1=c1)
    for P, c1, c2, cout in [(524288, 64, 64, 256), (1024000, 64, 64, 256), (40000, 128, 64, 256), (32768, 512, 1024, 2048), (64000, 512, 1024, 2048)]:
        p["cat_act %d_%d+%d-%d" % (P, c1, c2, cout)] = linear(P, c1 + c2, cout, FUSED, ck1=c1, x_rep=1)       # ..._with_output_stage_exact_integers
        if 2 * (c1 + c2) <= 256:
            p["cat_act %d_%d+%d-%d split weights" % (P, c1, c2, cout)] = linear(P, 2 * (c1 + c2), cout, FUSED, ck1=c1, x_rep=2)
    for case in [(3, 9, 5, 64, 64, 3, 3, 1, 1), (3, 7, 5, 128, 136, 3, 3, 1, 1), (2, 9, 8, 256, 64, 1, 1, 1, 0)]:      # test_conv2d_bn_act_edge_tiles_exact_integers
        p["bn_act edge %s" % (case,)] = fwd(*case, flags=FUSED)
    p["dgrad 256x320 masked residual"] = dgrad(257, 16, 8, 512, 512, 1, 1, 1, 0, RES | RES_MASK)          # test_conv_dgrad_masked_residual_on_256x320_tile...
    for name, rows, K, Nout, flags in RING_CASES:                     # test_gpu_conv_ring.py: the entries that nothing above reaches
        p["ring %s" % name] = linear(rows, K, Nout, flags)
    return p


PROBLEMS = _problems()

EXPECTED = {
    "plan 64x32_64-64_k1_s1 fwd+stats": "DMA64",
    "plan 64x32_64-64_k1_s1 fwd bn_act": "DMA64_LEAN",
    "plan 64x32_64-64_k1_s1 dgrad+masked residual": "DMA64",
    "plan 64x32_64-64_k3_s1 fwd+stats": "HALO64",
    "plan 64x32_64-64_k3_s1 fwd bn_act": "HALO64_LEAN",
    "plan 64x32_64-64_k3_s1 dgrad+masked residual": "HALO64",
    "plan 64x32_64-256_k1_s1 fwd+stats": "DMA128",
    "plan 64x32_64-256_k1_s1 fwd bn_act": "DMA128_FUSED",
    "plan 64x32_64-256_k1_s1 dgrad+masked residual": "DMA64",
    "plan 64x32_256-64_k1_s1 fwd+stats": "DMA64",
    "plan 64x32_256-64_k1_s1 fwd bn_act": "DMA64_LEAN",
    "plan 64x32_256-64_k1_s1 dgrad+masked residual": "DMA128",
    "plan 64x32_256-128_k1_s1 fwd+stats": "DMA128",
    "plan 64x32_256-128_k1_s1 fwd bn_act": "DMA128_FUSED",
    "plan 64x32_256-128_k1_s1 dgrad+masked residual": "DMA128",
    "plan 64x32_128-128_k3_s2 fwd+stats": "K64S",
    "plan 64x32_128-128_k3_s2 fwd bn_act": "K64S_LEAN",
    "plan 64x32_128-128_k3_s2 dgrad+masked residual": "DMA128_CLS",
    "plan 32x16_128-512_k1_s1 fwd+stats": "DMA128",
    "plan 32x16_128-512_k1_s1 fwd bn_act": "DMA128_FUSED",
    "plan 32x16_128-512_k1_s1 dgrad+masked residual": "DMA128",
    "plan 64x32_256-512_k1_s2 fwd+stats": "DMA128",
    "plan 64x32_256-512_k1_s2 fwd bn_act": "DMA128_FUSED",
    "plan 64x32_256-512_k1_s2 dgrad+masked residual": "WG128",
    "plan 32x16_512-128_k1_s1 fwd+stats": "DMA128",
    "plan 32x16_512-128_k1_s1 fwd bn_act": "DMA128_FUSED",
    "plan 32x16_512-128_k1_s1 dgrad+masked residual": "DMA128",
    "plan 32x16_128-128_k3_s1 fwd+stats": "K64S",
    "plan 32x16_128-128_k3_s1 fwd bn_act": "K64S_LEAN",
    "plan 32x16_128-128_k3_s1 dgrad+masked residual": "K64S",
    "plan 32x16_512-256_k1_s1 fwd+stats": "WG128",
    "plan 32x16_512-256_k1_s1 fwd bn_act": "WG128_FUSED",
    "plan 32x16_512-256_k1_s1 dgrad+masked residual": "DMA128",
    "plan 32x16_256-256_k3_s2 fwd+stats": "K64S",
    "plan 32x16_256-256_k3_s2 fwd bn_act": "K64S_LEAN",
    "plan 32x16_256-256_k3_s2 dgrad+masked residual": "WG128_CLS",
    "plan 16x8_256-1024_k1_s1 fwd+stats": "DMA128",
    "plan 16x8_256-1024_k1_s1 fwd bn_act": "DMA128_FUSED",
    "plan 16x8_256-1024_k1_s1 dgrad+masked residual": "K64S",
    "plan 32x16_512-1024_k1_s2 fwd+stats": "WG128",
    "plan 32x16_512-1024_k1_s2 fwd bn_act": "WG128_FUSED",
    "plan 32x16_512-1024_k1_s2 dgrad+masked residual": "K64",
    "plan 16x8_1024-256_k1_s1 fwd+stats": "K64S",
    "plan 16x8_1024-256_k1_s1 fwd bn_act": "K64S_LEAN",
    "plan 16x8_1024-256_k1_s1 dgrad+masked residual": "DMA128",
    "plan 16x8_256-256_k3_s1 fwd+stats": "K64S",
    "plan 16x8_256-256_k3_s1 fwd bn_act": "K64S_LEAN",
    "plan 16x8_256-256_k3_s1 dgrad+masked residual": "K64S",
    "plan 16x8_1024-512_k1_s1 fwd+stats": "K64",
    "plan 16x8_1024-512_k1_s1 fwd bn_act": "K64_FUSED",
    "plan 16x8_1024-512_k1_s1 dgrad+masked residual": "WG128",
    "plan 16x8_512-512_k3_s1 fwd+stats": "K64",
    "plan 16x8_512-512_k3_s1 fwd bn_act": "K64_FUSED",
    "plan 16x8_512-512_k3_s1 dgrad+masked residual": "K64",
    "plan 16x8_512-2048_k1_s1 fwd+stats": "WG128",
    "plan 16x8_512-2048_k1_s1 fwd bn_act": "WG128_FUSED",
    "plan 16x8_512-2048_k1_s1 dgrad+masked residual": "K64",
    "plan 16x8_1024-2048_k1_s1 fwd+stats": "K64",
    "plan 16x8_1024-2048_k1_s1 fwd bn_act": "K64_FUSED",
    "plan 16x8_1024-2048_k1_s1 dgrad+masked residual": "K64",
    "plan 16x8_2048-512_k1_s1 fwd+stats": "K64",
    "plan 16x8_2048-512_k1_s1 fwd bn_act": "K64_FUSED",
    "plan 16x8_2048-512_k1_s1 dgrad+masked residual": "WG128",
    "vit patch fwd": "K64_320",
    "vit qkv fwd": "K64",
    "vit qkv dgrad": "K64_320",
    "vit proj fwd row_scale+residual": "K64_320",
    "vit proj fwd residual": "K64_320",
    "vit proj dgrad": "K64_320",
    "vit fc1 fwd gelu": "K64_LIN",
    "vit fc1 dgrad": "K64_320",
    "vit fc2 fwd row_scale+residual": "K64_320",
    "vit fc2 fwd residual": "K64_320",
    "vit fc2 dgrad": "K64_LIN",
    "conv case 1 fwd+stats": "DMA64",
    "conv case 1 dgrad": "DMA128",
    "conv case 1 dgrad+masked residual": "DMA128",
    "conv case 14 fwd+stats": "K64",
    "conv case 14 dgrad": "K64S",
    "conv case 14 dgrad+masked residual": "K64S",
    "conv case 15 fwd+stats": "K64S",
    "conv case 15 dgrad": "DMA128",
    "conv case 15 dgrad+masked residual": "DMA128",
    "conv case 16 fwd+stats": "K64S",
    "conv case 16 dgrad": "DMA128",
    "conv case 16 dgrad+masked residual": "DMA128",
    "conv case 17 fwd+stats": "K64",
    "conv case 17 dgrad": "WG128",
    "conv case 17 dgrad+masked residual": "WG128",
    "conv case 18 fwd+stats": "K64S",
    "conv case 18 dgrad": "WG128_CLS",
    "conv case 18 dgrad+masked residual": "WG128_CLS",
    "conv case 19 fwd+stats": "HALO64",
    "conv case 19 dgrad": "HALO64",
    "conv case 19 dgrad+masked residual": "HALO64",
    "conv case 20 fwd+stats": "HALO64",
    "conv case 20 dgrad": "HALO64",
    "conv case 20 dgrad+masked residual": "HALO64",
    "conv case 21 fwd+stats": "WG256",
    "conv case 21 dgrad": "K64S",
    "conv case 21 dgrad+masked residual": "K64S",
    "conv case 22 fwd+stats": "K64S",
    "conv case 22 dgrad": "K64_CLS",
    "conv case 22 dgrad+masked residual": "K64_CLS",
    "cat 777_256+64-64": "DMA64_SRC2",
    "cat 1000_512+128-128": "DMA128_SRC2",
    "cat 300_64+32-24": "DMA64_SRC2",
    "cat 16640_1024+256-256": "K64S_SRC2",
    "cat 16500_2048+512-512": "K64_SRC2",
    "cat 16384_1024+64-128": "K64S_SRC2",
    "cat 16384_448+64-256": "DMA128_SRC2",
    "cat 20000_512+256-512": "DMA128_SRC2",
    "cat_act 524288_64+64-256": "F1_RB2_SRC2",
    "cat_act 524288_64+64-256 split weights": "F1_RB1_SRC2",
    "cat_act 1024000_64+64-256": "F1_RB2_SRC2",
    "cat_act 1024000_64+64-256 split weights": "F1_RB1_SRC2",
    "cat_act 40000_128+64-256": "F1_RB1_SRC2",
    "cat_act 32768_512+1024-2048": "K64_FUSED_SRC2",
    "cat_act 64000_512+1024-2048": "K64_FUSED_SRC2",
    "bn_act edge (3, 9, 5, 64, 64, 3, 3, 1, 1)": "DMA64_LEAN",
    "bn_act edge (3, 7, 5, 128, 136, 3, 3, 1, 1)": "DMA128_FUSED",
    "bn_act edge (2, 9, 8, 256, 64, 1, 1, 1, 0)": "DMA64_LEAN",
    "dgrad 256x320 masked residual": "K64_320",
    "ring DMA128_LIN": "DMA128_LIN",
    "ring WG128_LIN": "WG128_LIN",
}


@pytest.fixture(scope="module")
def kernel_name():
    L = _lib.lib()
    L.dali_debug_conv_kernel_name.argtypes = [ctypes.c_int] * 14 + [ctypes.c_char_p, ctypes.c_int]
    L.dali_debug_conv_kernel_name.restype = ctypes.c_int

    def name(Cm, P, h, wd, ck, r, s, stride, pad, mode, flags, ck1=0, x_rep=0, n_cus=N_CUS):
        buf = ctypes.create_string_buffer(128)
        rc = L.dali_debug_conv_kernel_name(Cm, P, h, wd, ck, r, s, stride, pad, mode, flags, ck1, x_rep, n_cus, buf, len(buf))
        return buf.value.decode() if rc == 0 else rc
    return name


def test_the_table_lists_every_problem():
    assert sorted(EXPECTED) == sorted(PROBLEMS)


@pytest.mark.parametrize("key", sorted(PROBLEMS))
def test_problem_is_launched_on_the_recorded_entry(kernel_name, key):
    assert kernel_name(**PROBLEMS[key]) == EXPECTED[key]


def test_every_ring_instantiation_is_reached(kernel_name):
    reached = set()
    for prob in PROBLEMS.values():
        got = kernel_name(**prob)
        assert isinstance(got, str), (prob, got, _lib.last_error())
        reached.update(got.split("+"))
    assert RING <= reached, sorted(RING - reached)


def test_refusals_return_the_status_and_need_no_device(kernel_name):
    """test_conv1x1_cat_act_refuses_and_leaves_output's two problems: DALI_ERR_INVALID (-1) from the chooser, nothing written to `out`"""
    assert kernel_name(**linear(1000, 2 * (64 + 64), 256, FUSED, ck1=64, x_rep=2)) == -1
    assert "persistent streaming kernel" in _lib.last_error()
    assert kernel_name(**linear(1000, 256 + 128, 256, FUSED, ck1=256, x_rep=1)) == -1
    # a residual mask goes with neither the fused stage nor the linear extras
    assert kernel_name(**dgrad(2, 8, 8, 64, 128, 1, 1, 1, 0, RES | RES_MASK | LIN)) == -1
    # the persistent kernel's choice depends on the CU count handed in, not on a device: 2 tiles per CU at 64 CUs, not at 256
    small = linear(16384, 128, 256, FUSED | RES)
    assert kernel_name(**small, n_cus=64) == "F1_RB2_RES" and kernel_name(**small) == "DMA128_FUSED"

"""The arena of the two net plans as a table (daliid_amd/csrc/plan_table.h): every tensor is declared once, in dali_*_create_ex, with its name,
pointer and size, and dali_debug_{resnet,vit}_arena_entry lists the declarations.  The wiring suites (test_gpu_resnet_plan.py,
test_gpu_vit_plan.py, ...) read the plans' tensors through dali_resnet_debug_tensor / dali_debug_vit_tensor, which look the name up in that
table; here the table itself is checked, per plan: unique names, aligned reservations that do not overlap and add up to arena_bytes exactly (an
unnamed or doubly counted reservation shows there), views inside reserved tensors, the lookup agreeing with the enumerator entry by entry, and
the plan's sizes against those of the commit before the table existed.  One tiny eval forward per plan binds it.

Plans: a ResNet training plan (a block without a downsample branch, the first block whose downsample backward runs through the moments of x),
the same with IBN stages (eval only), a ViT training plan, the same ViT with JPM + SIE (8 patch tokens in four runs of 1 + 2; eval only) and a
head-dim-96 ViT (eval only).  (At width 32 no block folds conv3 + downsample for inference: wcat / shcat are read by test_gpu_resnet_eval_plan.py.)
"""
import ctypes
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DALI_ERR_INVALID = -1               # include/daliid.h

# (param_elems, buffer_elems, arena_bytes, n_params, n_buffers) of dali_resnet_sizes / dali_vit_sizes for these configurations at commit c14fcaa
# ("Test the ResNet plan's inference forward op by op from its own tensors"), the last one whose create functions reserved unnamed tensors
SIZES = {
    "resnet": (2031360, 12416, 16287488, 62, 42),
    "resnet_ibn": (2031744, 12288, 4949504, 70, 42),
    "vit": (498112, 256, 3161600, 34, 2),
    "vit_jpm": (902976, 1280, 2631424, 76, 10),
    "vit_hd96": (1042048, 384, 3139328, 34, 2),
}
TRAINING = ("resnet", "vit")
# held by a training plan only
GRAD_ONLY = {"resnet": ("block0.raw1", "block0.conv2.wt", "gbuf1"), "vit": ("block0.qkv.wt", "dp_rows", "grad_cur")}


@functools.lru_cache(maxsize=None)
def _dbg():
    """the diagnostic entry points (include/daliid_debug.h), bound here: nothing under daliid_amd/ binds them"""
    from daliid_amd import _lib
    L = _lib.lib()
    vp, i64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)
    for fn in (L.dali_debug_resnet_arena_entry, L.dali_debug_vit_arena_entry):
        fn.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, i64p, i64p, ctypes.POINTER(ctypes.c_int)]
    L.dali_debug_vit_tensor.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), i64p]        # (dali_resnet_debug_tensor: daliid.h, bound by _lib)
    return L


def _build(name):
    """the net in eval mode after one forward of batch 2 at 64 x 32: its last plan is bound"""
    from daliid_amd import Encoders as E
    from daliid_amd import vit_pytorch as V
    from daliid_amd.make_models import jpm_token_map
    x = torch.randn(2, 3, 64, 32, generator=torch.Generator().manual_seed(3)).cuda()
    vit = dict(img_size=(64, 32), patch_size=16, stride_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, num_classes=10, seed=1)
    labels = {}
    if name == "resnet":
        net = E.ResNet50ReID(layers=(2, 1, 1, 1), width=32, seed=1)
    elif name == "resnet_ibn":
        net = E.ResNet50IBNReID(layers=(2, 1, 1, 1), width=32, seed=1)
    elif name == "vit":
        net = V.ViTNeckNet(**vit)
    elif name == "vit_jpm":
        net = V.ViTNeckNet(camera=3, jpm=dict(token_map=jpm_token_map(8, 3, 2, 4, True), neck_after=1, id_classes=10), **vit)
        labels = dict(cam_label=[0, 2])
    else:
        net = V.ViTNeckNet(**dict(vit, embed_dim=192))
    net.eval()
    with torch.no_grad():
        net(x, **labels)
    torch.cuda.synchronize()
    return net


@functools.lru_cache(maxsize=None)
def arena(name):
    net = _build(name)
    L, plan = _dbg(), net._last_plan
    kind = "resnet" if name.startswith("resnet") else "vit"
    entry = L.dali_debug_resnet_arena_entry if kind == "resnet" else L.dali_debug_vit_arena_entry
    lookup = L.dali_resnet_debug_tensor if kind == "resnet" else L.dali_debug_vit_tensor
    entries, buf = [], ctypes.create_string_buffer(128)
    off, nbytes, reserved = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    while entry(plan.h, len(entries), buf, 128, ctypes.byref(off), ctypes.byref(nbytes), ctypes.byref(reserved)) == 0:
        entries.append((buf.value.decode(), off.value, nbytes.value, reserved.value))
        assert len(entries) < 100000
    assert entry(plan.h, len(entries), buf, 128, ctypes.byref(off), ctypes.byref(nbytes), ctypes.byref(reserved)) == DALI_ERR_INVALID
    assert entry(plan.h, -1, buf, 128, ctypes.byref(off), ctypes.byref(nbytes), ctypes.byref(reserved)) == DALI_ERR_INVALID

    def tensor(tensor_name):
        """(status, byte offset from the arena's base, bytes) of the plan's debug-tensor call"""
        ptr, nb = ctypes.c_void_p(), ctypes.c_int64()
        rc = lookup(plan.h, tensor_name.encode(), ctypes.byref(ptr), ctypes.byref(nb))
        return (rc, ptr.value - net._arena.data_ptr(), nb.value) if rc == 0 else (rc, None, None)

    return types.SimpleNamespace(net=net, plan=plan, entries=entries, tensor=tensor)


PLANS = pytest.mark.parametrize("name", list(SIZES))


@PLANS
def test_reservations_tile_the_arena(name):
    a = arena(name)
    names = [e[0] for e in a.entries]
    assert len(set(names)) == len(names), sorted(n for n in set(names) if names.count(n) > 1)
    assert all(names), "an entry without a name"
    reserved = sorted((off, nbytes, n) for n, off, nbytes, r in a.entries if r)
    assert reserved and all(off % 256 == 0 for off, _, _ in reserved)
    assert all(off == -1 for _, off, _, r in a.entries if not r)
    for (o0, b0, n0), (o1, _, n1) in zip(reserved, reserved[1:]):
        assert o0 + b0 <= o1, (n0, o0, b0, n1, o1)
    assert sum((nbytes + 255) // 256 * 256 for _, nbytes, _ in reserved) == a.plan.arena_bytes


@PLANS
def test_lookup_agrees_with_the_table(name):
    a = arena(name)
    reserved = [(off, nbytes) for _, off, nbytes, r in a.entries if r]
    bound = 0
    for n, off, nbytes, r in a.entries:
        rc, got_off, got_bytes = a.tensor(n)
        if r:
            assert (rc, got_off, got_bytes) == (0, off, nbytes), n
        elif rc == 0:
            # a view that is bound: these bytes, wholly inside one reserved tensor
            bound += 1
            assert got_bytes == nbytes and sum(o <= got_off and got_off + nbytes <= o + b for o, b in reserved) == 1, (n, got_off, nbytes)
        else:
            assert rc == DALI_ERR_INVALID, n             # a view that nothing has set: the plan does not hold it
    assert bound >= 4 * 2                                # at least every trunk block's forward weight images, inside the bf16 cast
    for bad in ("nope", "", "block0", "block0.", "block9.a1", "block0.nope", "gbuf9"):
        assert a.tensor(bad)[0] == DALI_ERR_INVALID, bad


@PLANS
def test_sizes_are_those_before_the_table(name):
    p = arena(name).plan
    assert (p.param_elems, p.buffer_elems, p.arena_bytes, p.n_params, p.n_buffers) == SIZES[name]


@PLANS
def test_gradient_only_tensors_are_held_by_training_plans_only(name):
    a = arena(name)
    kind = "resnet" if name.startswith("resnet") else "vit"
    listed = {e[0] for e in a.entries}
    for n in GRAD_ONLY[kind]:
        if name in TRAINING:
            assert n in listed and a.tensor(n)[0] == 0, n
        else:
            assert a.tensor(n)[0] == DALI_ERR_INVALID, n

"""GPU: what the ResNet and the ViT wrapper share on top of their plans -- when a plan is bound and when the weights are re-cast, that an
arena regrowth or a reload changes no result it should not, the refusal of a backward after a forward of another shape, where the
gradients land, how a 4-D parameter is stored, and the refusal of device / dtype moves.  Both nets at the smallest shapes the other suites
train; every expectation is exact (counts, pointers, torch.equal), there is no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ("resnet", "vit")
BACKWARD = {"resnet": "dali_resnet_backward", "vit": "dali_vit_backward_stages"}


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import Encoders, _lib, vit_pytorch
    return dict(E=Encoders, V=vit_pytorch, lib=_lib)


def build(mods, kind, seed=1):
    if kind == "resnet":
        return mods["E"].ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=seed)
    return mods["V"].ViTNeckNet(img_size=(32, 32), patch_size=8, stride_size=8, embed_dim=64, depth=2, num_heads=1, num_classes=10, seed=seed)


def images(kind, batch):
    h, w = (64, 32) if kind == "resnet" else (32, 32)             # the ViT: 4 x 4 patches + cls = 17 tokens
    return torch.randn(batch, 3, h, w, generator=torch.Generator().manual_seed(5)).cuda()


def param_table(net, kind, batch=4):
    """name -> (offset, numel, shape) of the plan's parameter table"""
    plan = net._plan(batch, 64, 32) if kind == "resnet" else net._plan(batch)
    return {name: (off, numel, shape) for name, off, numel, shape in plan.tensor_table(0)}


def count_calls(monkeypatch, mods, names):
    """Wrap entries of the loaded library so that calls are counted; the originals still run."""
    L, counts = mods["lib"].lib(), {name: 0 for name in names}
    for name in names:
        def counted(*args, _name=name, _orig=getattr(L, name)):
            counts[_name] += 1
            return _orig(*args)
        monkeypatch.setattr(L, name, counted)
    return counts


@pytest.mark.parametrize("kind", KINDS)
def test_activation_state_machine(mods, monkeypatch, kind):
    """(bind, refresh_weights) calls per forward: a plan is bound when another one ran last (or none), the weights are re-cast when the plan
    changed or flat_params' version moved, and an arena regrowth forces both."""
    bind, refresh = "dali_%s_bind" % kind, "dali_%s_refresh_weights" % kind
    counts = count_calls(monkeypatch, mods, (bind, refresh))
    net = build(mods, kind).eval()
    x4, x8 = images(kind, 4), images(kind, 8)

    def forward(x):
        before = (counts[bind], counts[refresh])
        with torch.no_grad():
            net(x)
        return counts[bind] - before[0], counts[refresh] - before[1]

    assert forward(x4) == (1, 1)
    assert forward(x4) == (0, 0)
    net.mark_weights_changed()
    assert forward(x4) == (0, 1)
    net.load_state_dict(net.state_dict())
    assert forward(x4) == (0, 1)
    arena = net._arena
    assert forward(x8) == (1, 1) and net._arena is not arena           # the arena regrew
    assert forward(x4) == (1, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_arena_regrowth_keeps_results(mods, kind):
    net = build(mods, kind).eval()
    x4 = images(kind, 4)
    with torch.no_grad():
        first = net(x4)
        twice = net(torch.cat([x4, x4]))
        again = net(x4)
    assert torch.isfinite(first).all() and first.abs().max() > 0
    assert torch.equal(again, first)
    assert torch.equal(twice[:4], first) and torch.equal(twice[4:], first)          # eval features do not depend on the batch


@pytest.mark.parametrize("kind", KINDS)
def test_loaded_weights_are_seen(mods, kind):
    net, other = build(mods, kind, seed=1).eval(), build(mods, kind, seed=2).eval()
    x = images(kind, 4)
    with torch.no_grad():
        own = net(x)
        net.load_state_dict(other.state_dict())
        loaded, expect = net(x), other(x)
    assert torch.equal(loaded, expect) and not torch.equal(loaded, own)


@pytest.mark.parametrize("kind", KINDS)
def test_backward_after_forward_of_another_shape_is_refused(mods, monkeypatch, kind):
    net = build(mods, kind).train()
    out = net._run_forward(images(kind, 4), True)
    net._run_forward(images(kind, 8), False)
    counts = count_calls(monkeypatch, mods, (BACKWARD[kind],))
    with pytest.raises(mods["lib"].DaliError):
        net._backward_stage(torch.ones_like(out), 0)
    assert counts[BACKWARD[kind]] == 0                                 # refused before anything was launched


@pytest.mark.parametrize("kind", KINDS)
def test_gradients_attach_by_name(mods, kind):
    net = build(mods, kind).train()
    net(images(kind, 4)).sum().backward()
    table, base, total = param_table(net, kind), net.flat_grads.data_ptr(), net.flat_grads.numel()
    params = dict(net.named_parameters())
    assert set(params) == set(table)
    for name, p in params.items():
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        off, numel, shape = table[name]
        assert 0 <= off and off + numel <= total, name
        assert p.grad is not None and p.grad.data_ptr() == base + 4 * off, name
        assert p.grad.shape == p.shape == torch.Size(shape) and p.grad.stride() == p.stride(), name       # (a wrong OHWI view shows here)
    if kind == "vit":
        assert not params["bottleneck.bias"].requires_grad and params["bottleneck.bias"].grad is None
    assert net.flat_grads.abs().max() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_4d_parameter_storage(mods, kind):
    """The conv weights of the ResNet are logical OIHW over the OHWI storage its kernels read; the ViT's patch projection is stored as it
    is shaped."""
    net = build(mods, kind)
    table = param_table(net, kind)
    if kind == "resnet":
        name, w = "conv1.weight", net.conv1.weight
        stored = w.permute(0, 2, 3, 1)
    else:
        name, w = "base.patch_embed.proj.weight", net.base.patch_embed.proj.weight
        stored = w
    off, numel, shape = table[name]
    assert w.dim() == 4 and w.shape == torch.Size(shape) and w.numel() == numel
    assert stored.is_contiguous() and w.data_ptr() == net.flat_params.data_ptr() + 4 * off
    assert w.abs().max() > 0 and torch.equal(stored.reshape(-1), net.flat_params[off:off + numel])


@pytest.mark.parametrize("kind", KINDS)
def test_device_and_dtype_moves_are_refused(mods, kind):
    net = build(mods, kind)
    with pytest.raises(mods["lib"].DaliError):
        net.half()
    with pytest.raises(mods["lib"].DaliError):
        net.cpu()
    assert net.cuda() is net and net.float() is net
    assert net.flat_params.dtype == torch.float32 and net.flat_params.is_cuda


def test_ibn_parameters_pair_by_name(mods):
    """ResNet50IBNReID registers four modules the plan does not hold before ``last_bn``: the plan's names still find their own views, the
    other parameters live outside flat_params and never get a gradient, and the net stays eval only."""
    net = mods["E"].ResNet50IBNReID(layers=(1, 1, 1, 1), width=64, seed=1).eval()
    x = torch.randn(2, 3, 64, 32, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        assert torch.isfinite(net(x)).all()
    table = {name: (off, numel, shape) for name, off, numel, shape in net._plan(2, 64, 32).tensor_table(0)}
    params = dict(net.named_parameters())
    base, end = net.flat_params.data_ptr(), net.flat_params.data_ptr() + 4 * net.flat_params.numel()
    for name, (off, numel, shape) in table.items():
        assert params[name].data_ptr() == base + 4 * off and params[name].shape == torch.Size(shape), name
    unplanned = sorted(set(params) - set(table))
    assert unplanned == sorted(m + s for m in ("conv1x1_layer4", "conv1x1_squeeze_layer4", "conv1x1_expand_layer4", "attribute_classifier")
                               for s in (".weight", ".bias"))
    assert list(params).index("conv1x1_layer4.weight") < list(params).index("last_bn.weight")
    for name in unplanned:
        assert not base <= params[name].data_ptr() < end and params[name].grad is None, name
    net.train()
    with pytest.raises(NotImplementedError):
        net(x)

"""CPU: the two small backbones of make_models.py:392-397 -- the restatement tests/vit_small_ref.py pinned to the reference's own outputs
(tests/golden/vit_small.npz, written by tests/golden/make_vit_small_golden.py), and the Python surface that needs no GPU: the factory names,
their parameter lists, the four TRANSFORMER_TYPE names."""
import inspect

import pytest
import torch

from conftest import load_golden
import vit_small_ref as R


@pytest.fixture(scope="module")
def golden():
    return load_golden("vit_small.npz")


# vs16: ViT-Small (8 heads of 96, no qkv bias, scale 768 ** -0.5); ds16: DeiT-Small (6 heads of 64, default scale)
@pytest.mark.parametrize("name,heads,qk_scale", [("vs16", 8, 768 ** -0.5), ("ds16", 6, None)])
def test_restatement_matches_the_reference(golden, name, heads, qk_scale):
    z = golden
    H, W, stride = (int(v) for v in z[name + "/geom"])
    keys, shapes = [str(k) for k in z[name + "/keys"]], [str(s) for s in z[name + "/shapes"]]
    sd = R.seeded_state(keys, shapes, float(z["qkv_std"]) if name.startswith("vs") else 0.02)
    assert any(k.endswith("attn.qkv.bias") for k in keys) == (name == "ds16")
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(int(z["x_seed"])))
    with torch.no_grad():
        y, gf = R.forward(sd, x, heads, stride, qk_scale)
    e_y, e_gf = R.rel_l2(y, torch.from_numpy(z[name + "/y_eval"])), R.rel_l2(gf, torch.from_numpy(z[name + "/global_feat"]))
    print("%s: restatement vs the reference: y_eval rel-L2 %.3e, global_feat rel-L2 %.3e" % (name, e_y, e_gf))
    assert e_y < 1e-5 and e_gf < 1e-5


def test_a_head_width_scale_would_show(golden):
    """the golden's own figure: with qk_scale 96 ** -0.5 the reference's ViT-Small output moves by at least five times the GPU tests' bound,
    and the restatement moves with it"""
    z = golden
    for name in ("vs16", "vs12", "vsjpm"):
        assert float(z[name + "/scale_shift"]) >= 0.1
    keys, shapes = [str(k) for k in z["vs16/keys"]], [str(s) for s in z["vs16/shapes"]]
    sd = R.seeded_state(keys, shapes, float(z["qkv_std"]))
    x = torch.randn(2, 3, 256, 128, generator=torch.Generator().manual_seed(int(z["x_seed"])))
    with torch.no_grad():
        wrong, _ = R.forward(sd, x, 8, 16, 96 ** -0.5)
    assert abs(R.rel_l2(wrong, torch.from_numpy(z["vs16/y_eval"])) - float(z["vs16/scale_shift"])) < 1e-3


@pytest.mark.parametrize("name", sorted(R.FACTORY_PARAMS))
def test_factories_take_the_reference_parameters(name):
    from daliid_amd import vit_pytorch as V
    fn = getattr(V, name)
    params = list(inspect.signature(fn).parameters.values())
    assert params[-1].kind is inspect.Parameter.VAR_KEYWORD
    assert tuple((p.name, p.default) for p in params[:-1]) == R.FACTORY_PARAMS[name]


def test_the_four_transformer_types_are_in_geom():
    from daliid_amd import make_models
    assert tuple(make_models._GEOM) == R.TRANSFORMER_TYPES
    dim, depth, heads, ratio, qkv_bias, qk_scale = make_models._GEOM["vit_small_patch16_224_TransReID"]
    assert (dim, depth, heads, int(dim * ratio), qkv_bias) == (768, 8, 8, 2304, False) and qk_scale == 768 ** -0.5
    assert make_models._GEOM["deit_small_patch16_224_TransReID"] == (384, 12, 6, 4.0, True, None)
    assert make_models._GEOM["vit_base_patch16_224_TransReID"] == make_models._GEOM["deit_base_patch16_224_TransReID"] == (768, 12, 12, 4.0, True, None)

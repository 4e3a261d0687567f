"""CPU: tests/ibn_ref.py (the IBN-a trunk, the reference's wrapper restated, the seeded weights) against tests/golden/ibn.npz, which the
reference's own ResNet50IBNReID / ResNet101IBNReID wrote (tests/golden/make_ibn_golden.py); and the product's export of both classes."""
import numpy as np
import pytest
import torch

import ibn_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("ibn.npz")


def golden_table(gold, pre):
    return list(zip([str(k) for k in gold[pre + "keys"]], [str(s) for s in gold[pre + "shapes"]]))


@pytest.mark.parametrize("pre,layers,wrapper", [("r50/", (3, 4, 6, 3), R.ResNet50IBNReID), ("r101/", (3, 4, 23, 3), R.ResNet101IBNReID),
                                                ("small/", (1, 1, 1, 1), R.ResNet50IBNReID)])
def test_wrapper_keys_equal_the_reference(gold, pre, layers, wrapper):
    mine = [(k, str(s)) for k, s in R.key_shapes(R.build(layers, 64, wrapper=wrapper))]
    assert mine == golden_table(gold, pre)


def test_small_table_is_what_the_issue_counts(gold):
    table = golden_table(gold, "small/")
    assert len(table) == 121
    assert ("layer1.0.bn1.IN.weight", "(32,)") in table and ("layer3.0.bn1.BN.num_batches_tracked", "()") in table
    assert not [k for k, _ in table if k.startswith("layer4.0.bn1.IN")]                       # ibn_cfg = ('a', 'a', 'a', None)
    names = [k for k, _ in table]
    assert names.index("layer4.0.downsample.1.num_batches_tracked") < names.index("conv1x1_layer4.weight") < names.index("last_bn.weight")
    extras = [int(np.prod(eval(s))) for k, s in table if k.split(".")[0] in ("conv1x1_layer4", "conv1x1_squeeze_layer4", "conv1x1_expand_layer4",
                                                                              "attribute_classifier")]
    assert len(extras) == 8 and sum(extras) == 6476889


def test_fp32_forward_matches_the_reference_output(gold):
    n, h, w = [int(v) for v in gold["small/geom"][:3]]
    model = R.build((1, 1, 1, 1), 64)
    model.load_state_dict(R.seeded_state(model.state_dict(), int(gold["small/w_seed"])))
    model.eval()
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(int(gold["small/x_seed"])))
    with torch.no_grad():
        y = model(x).numpy()
    ref = gold["small/y_eval"]
    assert y.shape == ref.shape == (4, 2048)
    # 1e-5 of the largest output: |y| reaches 117, where one fp32 ulp is 7.6e-6, and the convolutions' summation order follows the
    # thread count (0 with the generator's thread count, 3.3e-5 absolute = 2.9e-7 relative with one thread)
    assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max()
    # the twin rounds to bf16 at a dozen points: it stays near, and is not the fp32 forward itself
    twin = R.forward_matched_eval(model, x).numpy()
    rel = np.linalg.norm(twin - ref) / np.linalg.norm(ref)
    assert 0 < rel < 3e-2, rel


def test_ibn_halves():
    m = R.IBN(64)
    assert m.half == 32 and m.IN.weight.shape == (32,) and m.BN.running_var.shape == (32,)
    m.eval()
    x = torch.randn(2, 64, 5, 3, generator=torch.Generator().manual_seed(0)) * 3 + 1
    y = m(x)
    # instance statistics in eval mode too; the BatchNorm half by its running statistics (0 / 1)
    assert torch.allclose(y[:, :32].mean((2, 3)), torch.zeros(2, 32), atol=1e-5)
    assert torch.allclose(y[:, 32:], x[:, 32:] / (1 + 1e-5) ** 0.5, atol=1e-5)
    mean, invstd = R.ibn_stats(x[:, :32])
    assert torch.allclose((x[:, :32] - mean) * invstd, y[:, :32], atol=1e-5)


def test_encoders_exports_both_classes():
    from daliid_amd import Encoders
    assert issubclass(Encoders.ResNet50IBNReID, Encoders.ResNet50ReID) and issubclass(Encoders.ResNet101IBNReID, Encoders.ResNet50IBNReID)
    assert Encoders.ResNet50IBNReID._ibn == (1, 1, 1, 0)
    for cls in (Encoders.ResNet50IBNReID, Encoders.ResNet101IBNReID):
        assert "IGNORED" in cls.forward.__doc__ and "forward_heads" in cls.forward.__doc__

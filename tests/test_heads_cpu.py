"""CPU: the fp64 restatement of the multi-output head (tests/heads_ref.py) against the reference's own classes (tests/golden/heads.npz,
written by tests/golden/make_heads_golden.py), and the row ranges of the body parts."""
import numpy as np
import pytest

import heads_ref as R


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def test_fixture_shapes(gold):
    assert gold["map_bits"].shape == (1, 2048, 16, 8) and gold["map_bits"].dtype == np.uint16
    assert gold["map"].shape == (1, 16, 8, 2048)
    assert (gold["map"].max((1, 2)) < 0).any(), "the fixture keeps channels whose maximum is negative"
    assert gold["heatmap"].shape == (16, 8)
    assert float(gold["last_bn.eps"]) == 1e-5


@pytest.mark.parametrize("key,mode,rows", R.GOLDEN_HEADS)
def test_restatement_matches_reference_classes(gold, key, mode, rows):
    """Pooled values: max exact, the others within 1e-6 relative (the fixture is fp32 torch on the CPU); then through the neck."""
    x = gold["map"]
    f = R.pool(x, mode, rows)
    scale, shift = R.neck_coeffs(*gold["bn"])
    want = gold[key].astype(np.float64)
    # the neck undone: (y - shift) / scale is the pooled value the class fed to last_bn, up to fp32 rounding of y
    got = f * scale + shift
    tol = 1e-6 * (np.abs(f * scale) + np.abs(shift)) + 1e-6 * np.abs(want)
    assert np.all(np.abs(got - want) <= tol), float(np.abs(got - want).max())
    if mode == "gmp":
        # a max head is exact: the class's fp32 neck applied to the exact maximum
        import torch
        bn = torch.nn.BatchNorm1d(x.shape[3]).eval()
        with torch.no_grad():
            for name, v in zip(("weight", "bias", "running_mean", "running_var"), gold["bn"]):
                getattr(bn, name).copy_(torch.from_numpy(v))
            exact = bn(torch.from_numpy(f.astype(np.float32)))
        assert np.array_equal(f.astype(np.float32).astype(np.float64), f), "a maximum of bf16 values is a bf16 value"
        assert np.array_equal(exact.numpy(), gold[key])


def test_channel_sum_matches_attention_map(gold):
    ref = R.channel_sum(gold["map"])[0]
    want = gold["heatmap"].astype(np.float64)
    assert np.all(np.abs(ref - want) <= 1e-6 * np.abs(gold["map"][0]).sum(-1))
    assert np.all(np.abs(ref - want) <= R.heat_bound(gold["map"])[0])


def test_middle_part_is_rows_4_to_12(gold):
    x = gold["map"]
    assert np.array_equal(R.pool(x, "gmp", (4, 12)), x[:, 4:12].max((1, 2)))
    assert not np.array_equal(R.pool(x, "gmp", (4, 12)), R.pool(x, "gmp", (0, 8)))


def test_bounds_are_nonnegative_and_zero_for_max(gold):
    x = gold["map"]
    ref = R.pool(x, "both", (4, 12))
    assert np.all(R.mean_bound(x, ref, "both", (4, 12)) > 0)
    assert not R.mean_bound(x, ref, "gmp", (4, 12)).any()


def test_default_parts():
    from daliid_amd import _lib
    from daliid_amd.Encoders import default_parts
    assert default_parts(16) == ((0, 8), (4, 12), (8, 16))
    assert default_parts(4) == ((0, 2), (1, 3), (2, 4))
    assert default_parts(5) == ((0, 2), (1, 3), (2, 5))
    with pytest.raises(_lib.DaliError):
        default_parts(1)


def test_extract_multipart_refuses_what_is_out_of_scope():
    from daliid_amd import getFeatures
    for kw in ({"eval_mode": False}, {"sobel": True}, {"grayscale": True}, {"BGR": True}):
        with pytest.raises(NotImplementedError):
            getFeatures.extractFeaturesMultiPart([], 256, 128, None, 4, **kw)

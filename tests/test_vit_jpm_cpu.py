"""CPU: the JPM token map (make_models.jpm_token_map) against the reference's own shuffle_unit outputs (tests/golden/vit_jpm.npz), and the
plain torch restatements of tests/vit_jpm_ref.py against the reference's outputs of golden case C (48x48, depth 2, 3 cameras x 2 views)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import vit_jpm_ref as R
from daliid_amd._lib import DaliError
from daliid_amd.make_models import jpm_token_map


@pytest.fixture(scope="module")
def z():
    return load_golden("vit_jpm.npz")


def _stored(z):
    return [tuple(int(v) for v in k.split("/")[1].split("_")) for k in z.files if k.startswith("shuffle/") and k != "shuffle/raises"]


def test_token_map_equals_every_stored_shuffle(z):
    cases = _stored(z)
    assert set(cases) == {(128, 2, 5), (210, 2, 5), (9, 2, 5), (12, 4, 5), (7, 4, 5), (7, 2, 5), (128, 4, 8)}
    for n, groups, shift in cases:
        order = z["shuffle/%d_%d_%d" % (n, groups, shift)]
        L = n // 4
        m = jpm_token_map(n, shift, groups, 4, True)
        assert m.dtype == np.int32 and m.shape == (4, L)
        assert np.array_equal(m.reshape(-1), order[:4 * L]), (n, groups, shift)
        runs, full = R.token_map(n, shift, groups, 4, True)
        assert full == order.tolist() and [t for r in runs for t in r] == m.reshape(-1).tolist()
    # the orders the reference produced, spelled out
    assert z["shuffle/128_2_5"][:4].tolist() == [5, 69, 6, 70] and len(z["shuffle/128_2_5"]) == 128
    assert z["shuffle/210_2_5"][:4].tolist() == [5, 110, 6, 111] and len(z["shuffle/210_2_5"]) == 210
    assert z["shuffle/9_2_5"].tolist() == [5, 1, 6, 2, 7, 3, 8, 4, 9, 3]
    assert z["shuffle/12_4_5"].tolist() == [5, 8, 11, 2, 6, 9, 12, 3, 7, 10, 1, 4]
    assert z["shuffle/7_4_5"].tolist() == [5, 7, 2, 4, 6, 1, 3, 3]
    # 210 tokens in runs of 52: the last two of the shuffled order are dropped; the padded duplicate always lands behind the runs
    assert not set(z["shuffle/210_2_5"][208:].tolist()) & set(jpm_token_map(210, 5, 2).reshape(-1).tolist())
    assert jpm_token_map(9, 5, 2).tolist() == [[5, 1], [6, 2], [7, 3], [8, 4]]


def test_token_map_raises_where_the_reference_raised(z):
    raised = [tuple(int(v) for v in r) for r in z["shuffle/raises"]]
    assert sorted(raised) == [(9, 4), (210, 4)]
    for n, groups in raised:
        with pytest.raises(DaliError):
            jpm_token_map(n, 5, groups, 4, True)
        with pytest.raises(ValueError):
            R.token_map(n, 5, groups, 4, True)
    for n, groups, shift in _stored(z):
        jpm_token_map(n, shift, groups, 4, True)                    # and nowhere else
    for shift in (0, -1, 128, 200):
        with pytest.raises(DaliError):
            jpm_token_map(128, shift, 2, 4, True)
    with pytest.raises(DaliError):
        jpm_token_map(3, 1, 1, 4, True)                              # fewer tokens than runs


def test_token_map_without_rearrange_is_the_identity_runs():
    for n in (128, 210, 9):
        L = n // 4
        assert np.array_equal(jpm_token_map(n, 5, 2, 4, False), np.arange(1, 4 * L + 1, dtype=np.int32).reshape(4, L))
    assert np.array_equal(jpm_token_map(210, 5, 4, 4, False)[3], np.arange(157, 209))      # groups do not matter, tokens 209 and 210 are dropped


def _case(z, name):
    keys, shapes = [str(k) for k in z[name + "/keys"]], [str(s) for s in z[name + "/shapes"]]
    H, W, stride, depth, cams, views, seed = (int(v) for v in z[name + "/geom"])
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(seed))
    return R.seeded_state(keys, shapes), x, stride, cams, views, float(z[name + "/coef"])


def test_restatements_reproduce_case_c(z):
    sd, x, stride, cams, views, coef = _case(z, "C")
    assert len(z["C/keys"]) == 91 and str(z["C/keys"][2]) == "base.sie_embed"
    idx = R.sie_index(z["C/cam"], z["C/view"], cams, views)
    assert idx.tolist() == [2, 5]
    tok = R.local_features(sd, x, 12, stride, idx, coef)
    ref_tok = torch.from_numpy(z["C/tokens"])
    assert tok.shape == ref_tok.shape == (2, 10, 768)
    assert float((tok - ref_tok).abs().max()) < 1e-5
    y = R.jpm_forward(sd, x, 12, stride, 5, 2, True, str(z["C/neck_feat"]) == "after", idx, coef)
    ref_y = torch.from_numpy(z["C/y"])
    assert y.shape == ref_y.shape == (2, 3840)
    assert float((y - ref_y).abs().max()) < 1e-5
    # the SIE term matters: without it the tokens differ by far more than the bound
    assert float((R.local_features(sd, x, 12, stride) - ref_tok).abs().max()) > 1e-2

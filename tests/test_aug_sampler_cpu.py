"""CPU: the batched augmentation-parameter sampler (transforms.sample_train_params_batched) against the sequential, torchvision-ordered
one, and the host side of ImageStore's loaders (lazy plans, slot assignment) -- nothing here touches a GPU."""
import itertools

import numpy as np
import pytest
import torch

from daliid_amd import transforms as T

N_DIST = 20000
JITTER = (0.4, 0.3, 0.4)          # brightness, contrast, saturation of train_encodersKIT.py:313-320 (the samplers' defaults)


def test_same_seed_same_array_other_seed_other_array():
    a = T.sample_train_params_batched(64, 256, 128, np.random.default_rng(5))
    b = T.sample_train_params_batched(64, 256, 128, np.random.default_rng(5))
    c = T.sample_train_params_batched(64, 256, 128, np.random.default_rng(6))
    assert a.dtype == np.int32 and a.shape == (64, T.AUG_WORDS)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


@pytest.mark.parametrize("hw", [(256, 128), (64, 32)])
def test_every_field_lies_in_its_domain(hw):
    H, W = hw
    pad = 10
    p = T.sample_train_params_batched(4000, H, W, np.random.default_rng(H))
    assert p[:, 0:2].min() >= 0 and p[:, 0:2].max() <= 2 * pad
    assert set(np.unique(p[:, 0])) == set(range(2 * pad + 1))                # 4000 draws over 21 values: every one occurs
    assert set(np.unique(p[:, 2])) == {0, 1}
    assert (np.sort(p[:, 3:7], axis=1) == np.arange(4)).all()
    for k, x in enumerate(JITTER):
        f = p[:, 11 + k].copy().view(np.float32)
        assert f.min() >= np.float32(1 - x) and f.max() <= np.float32(1 + x), (k, f.min(), f.max())
    ei, ej, eh, ew = p[:, 7], p[:, 8], p[:, 9], p[:, 10]
    none = (eh == 0) & (ew == 0)
    assert (p[none, 7:11] == 0).all()
    box = ~none
    assert box.any()
    assert (eh[box] > 0).all() and (ew[box] > 0).all() and (eh[box] < H).all() and (ew[box] < W).all()
    assert (ei[box] >= 0).all() and (ej[box] >= 0).all() and (ei[box] + eh[box] <= H).all() and (ej[box] + ew[box] <= W).all()
    assert (p[:, 14] == pad).all() and (p[:, 15] == 1).all()


def test_no_fitting_attempt_gives_no_box():
    # 8 x 8 with scale 0.9..1.0 and a wide aspect range: most images find no attempt with h < H and w < W
    p = T.sample_train_params_batched(500, 8, 8, np.random.default_rng(1), erase_scale=(0.9, 1.0), erase_ratio=(0.3, 3.3))
    none = p[:, 9] == 0
    assert none.any() and (p[none, 7:11] == 0).all()
    assert (p[~none, 9] < 8).all() and (p[~none, 10] < 8).all() and (p[~none, 10] > 0).all()


# the training configuration, where some attempt out of ten practically always fits, and a small image with large erase areas, where
# retries and "no box" are common (the share of images without a box is a live statistic only there)
CASES = {"train": (256, 128, {}), "tight": (64, 32, dict(erase_scale=(0.5, 1.0)))}


@pytest.fixture(scope="module", params=sorted(CASES))
def two_samples(request):
    H, W, kw = CASES[request.param]
    torch_state = torch.get_rng_state()
    torch.manual_seed(101)
    seq = T.sample_train_params(N_DIST, H, W, **kw)
    torch.set_rng_state(torch_state)
    bat = T.sample_train_params_batched(N_DIST, H, W, np.random.default_rng(202), **kw)
    if request.param == "tight":
        assert 0.02 < (seq[:, 9] == 0).mean() < 0.98
    return seq, bat


def _columns(p):
    """name -> float64 [n]: every scalar field, the erase statistics and one indicator per permutation of the four jitter ops."""
    cols = {"word%d" % k: p[:, k].astype(np.float64) for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15)}
    for k in (11, 12, 13):
        cols["factor%d" % k] = p[:, k].copy().view(np.float32).astype(np.float64)
    cols["no_box"] = (p[:, 9] == 0).astype(np.float64)
    cols["box_area"] = p[:, 9].astype(np.float64) * p[:, 10]
    code = p[:, 3] * 64 + p[:, 4] * 16 + p[:, 5] * 4 + p[:, 6]
    for perm in itertools.permutations(range(4)):
        cols["perm%d%d%d%d" % perm] = (code == perm[0] * 64 + perm[1] * 16 + perm[2] * 4 + perm[3]).astype(np.float64)
    return cols


def test_distribution_equals_the_sequential_sampler(two_samples):
    """Two independent samples of 20,000 rows, fixed seeds.  For every statistic (a mean, or a frequency = the mean of an indicator) the
    difference of the two sample means has standard error sqrt(var_a / n + var_b / n), estimated from the samples themselves; the bound is
    5 of those: with ~43 statistics the chance that equal distributions miss it is ~43 * 6e-7, and the seeds are fixed."""
    seq, bat = _columns(two_samples[0]), _columns(two_samples[1])
    assert len(seq) == 13 + 3 + 2 + 24
    bad = []
    for name in seq:
        a, b = seq[name], bat[name]
        se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
        diff = abs(a.mean() - b.mean())
        print("%-10s sequential %.5f batched %.5f diff %.2e = %.2f se" % (name, a.mean(), b.mean(), diff, diff / se if se else 0.0))
        if not diff <= 5 * se:
            bad.append((name, a.mean(), b.mean(), se))
    assert not bad, bad
    # every permutation does occur (a frequency of 0 in both samples would pass the bound above vacuously)
    assert all(seq[k].sum() > 0 and bat[k].sum() > 0 for k in seq if k.startswith("perm"))


def _fake_decode(calls):
    def decode(path):
        calls.append(path)
        return np.zeros((8, 4, 3), np.uint8)
    return decode


def test_batched_loader_plans_are_lazy_and_drawn_once_at_submit(monkeypatch):
    calls, draws = [], []
    real = T.sample_train_params_batched
    monkeypatch.setattr(T, "sample_train_params_batched", lambda n, *a, **k: (draws.append(n), real(n, *a, **k))[1])
    store = T.ImageStore(64, 32, capacity=16, decode=_fake_decode(calls))
    loader = store.train_loader(sampler="batched", seed=3)
    np_state, torch_state = np.random.get_state()[1].copy(), torch.get_rng_state()
    plans = [loader.plan(["a%d" % i, "b%d" % i], 64, 32, None) for i in range(3)]
    assert all(p.params is None and (p.height, p.width) == (64, 32) for p in plans)
    merged = plans[0].concat(plans, order=[5, 4, 3, 2, 1, 0])
    assert merged.params is None and merged.files == ["b2", "a2", "b1", "a1", "b0", "a0"] and (merged.height, merged.width) == (64, 32)
    assert not draws
    ticket = loader.submit(merged)
    assert draws == [6] and ticket.params.shape == (6, T.AUG_WORDS) and (ticket.params[:, 15] == 1).all()
    # neither global generator was touched: this sampler has its own stream
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)
    # the same seed gives the same parameters for the same plan
    again = T.ImageStore(64, 32, capacity=16, decode=_fake_decode([])).train_loader(sampler="batched", seed=3)
    assert np.array_equal(again.submit(again.plan(merged.files, 64, 32, None)).params, ticket.params)
    with pytest.raises(T._lib.DaliError):
        store.eval_loader.submit(merged)                                     # no generator there: a lazy plan is an error, not zeros


def test_torchvision_sampler_draws_at_plan_time_like_the_uncached_loader():
    store = T.ImageStore(64, 32, capacity=4, decode=_fake_decode([]))
    loader = store.train_loader()
    torch.manual_seed(9)
    want = T.plan_train(["x", "y", "z"], 64, 32, None)
    after = torch.get_rng_state()
    torch.manual_seed(9)
    got = loader.plan(["x", "y", "z"], 64, 32, None)
    assert np.array_equal(got.params, want.params) and got.files == want.files and torch.equal(torch.get_rng_state(), after)
    with pytest.raises(T._lib.DaliError):
        loader.plan(["x"], 128, 64, None)                                    # one store, one size
    with pytest.raises(ValueError):
        store.train_loader(sampler="fast")


def test_submit_gives_each_file_one_slot_and_one_decode():
    calls = []
    store = T.ImageStore(64, 32, capacity=4, decode=_fake_decode(calls))
    ev = store.eval_loader
    t1 = ev.submit(ev.plan(["a", "b", "a"], 64, 32, None))
    t2 = ev.submit(ev.plan(["b", "c", "c", "d", "e", "e", "f"], 64, 32, None))          # d fills the store; e, f find it full
    for t in (t1, t2):
        for f in t.temp_futures:
            f.result()
    for fill in store._fills:
        for f in fill.futures:
            f.result()
    assert t1.rows.tolist() == [0, 1, 0] and t2.rows.tolist() == [1, 2, 2, 3, -1, -1, -1]
    assert t2.temp_at == [[4, 5], [6]]
    assert sorted(calls) == ["a", "b", "c", "d", "e", "f"]
    assert store.stats == dict(hits=3, misses=6, decodes=6, uncached=2, rows_used=4)
    store.clear()
    assert store.stats == dict(hits=0, misses=0, decodes=0, uncached=0, rows_used=0)
    with pytest.raises(T._lib.DaliError):
        store._finish(t1)                                                    # a ticket from before clear() is void

"""GPU: dali_augment_gather and transforms.ImageStore (resized images resident in HBM) against the uncached loaders, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ERASED_R = (0.0 - 0.485) / 0.229          # value 0 before Normalize, channel 0


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import transforms
    return transforms


def _images(rng, sizes):
    out = []
    for h, w in sizes:
        yy, xx = np.mgrid[0:h, 0:w]
        base = 127 + 100 * np.sin(yy / 9.0)[..., None] * np.cos(xx / 7.0)[..., None] * np.array([1.0, 0.7, -0.8])
        out.append(np.clip(base + rng.normal(0, 40, size=(h, w, 3)), 0, 255).astype(np.uint8))
    return out


def _write_dataset(tmp_path, n_ids, per_id, hw=(128, 64), turb=True, fmt="jpg"):
    from PIL import Image
    rng = np.random.default_rng(3)
    clean = tmp_path / "clean"; tdir = tmp_path / "turb"
    clean.mkdir(); tdir.mkdir()
    records = []
    for pid in range(n_ids):
        for k, im in enumerate(_images(rng, [hw] * per_id)):
            name = "%04d_c1s1_%06d_00" % (pid, k)
            Image.fromarray(im).save(str(clean / (name + "." + fmt)), quality=95)
            if turb:
                for s in range(1, 6):
                    Image.fromarray(np.roll(im, s, axis=1)).save(str(tdir / ("%s_turbstrength%d.jpg" % (name, s))), quality=95)
            records.append([str(clean / (name + "." + fmt)), str(pid), "0", "person"])
    return np.array(records), str(tdir)


def _write_ragged(tmp_path, n):
    """n files of different sizes, PNG and JPEG alternating."""
    from PIL import Image
    rng = np.random.default_rng(11)
    sizes = [(128, 64), (200, 90), (64, 64), (301, 117), (17, 9), (128, 64), (96, 40), (256, 128), (77, 33), (150, 61), (40, 80), (128, 65)]
    paths = []
    for i, im in enumerate(_images(rng, sizes[:n])):
        p = str(tmp_path / ("%04d_c1s1_%06d_00.%s" % (i, i, "png" if i % 2 else "jpg")))
        Image.fromarray(im).save(p, quality=92)
        paths.append(p)
    return paths


def _counting(T):
    calls = []

    def decode(path):
        calls.append(path)
        return T._decode_one(path)
    return calls, decode


def _gather(T, store, store_rows, rows, params, n, h, w, out):
    from daliid_amd import _lib
    dev = out.device
    m3, s3 = (ctypes.c_float * 3)(*T.IMAGENET_MEAN), (ctypes.c_float * 3)(*T.IMAGENET_STD)
    return _lib.lib().dali_augment_gather(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(store), store_rows, _lib.ptr(rows), _lib.ptr(params), n, h, w,
                                          m3, s3, _lib.ptr(out))


def _params(T, kind, n, h, w, seed=4):
    if kind == "eval":
        return T.eval_params(n)
    torch.manual_seed(seed)
    return T.sample_train_params(n, h, w)


# ---- the kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["eval", "train"])
@pytest.mark.parametrize("hw", [(64, 32), (256, 128), (50, 34)])          # 50 x 34 x 3 bytes is no multiple of 16
def test_gather_equals_augment_of_the_picked_rows(T, hw, kind):
    h, w = hw
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(h)
    store = torch.from_numpy(np.stack(_images(rng, [hw] * 9))).to(dev)
    rows = [5, 2, 8, 2, 0, 7, 3]                                           # out of order, row 2 twice
    params = torch.from_numpy(_params(T, kind, len(rows), h, w)).to(dev)
    want = T.augment(store[torch.tensor(rows, device=dev)].contiguous(), params)
    out = torch.full((len(rows), 3, h, w), float("nan"), device=dev)
    assert _gather(T, store, 9, torch.tensor(rows, dtype=torch.int32, device=dev), params, len(rows), h, w, out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    if kind == "train":
        assert (out[:, 0] == ERASED_R).any()


def test_gather_reaches_rows_past_2_gib(T):
    """22,000 rows of 256 x 128 x 3 bytes = 2.16 GB: row 21,999 starts at byte 2,162,589,696 > 2^31.  Only the two rows read are written."""
    h, w, S = 256, 128, 22000
    dev = torch.device("cuda", 0)
    two = torch.from_numpy(np.stack(_images(np.random.default_rng(8), [(h, w)] * 2))).to(dev)
    store = torch.empty(S, h, w, 3, dtype=torch.uint8, device=dev)
    assert store.numel() > 2 ** 31
    store[S - 1], store[0] = two[0], two[1]
    params = torch.from_numpy(_params(T, "train", 2, h, w)).to(dev)
    want = T.augment(two, params)
    out = torch.full((2, 3, h, w), float("nan"), device=dev)
    assert _gather(T, store, S, torch.tensor([S - 1, 0], dtype=torch.int32, device=dev), params, 2, h, w, out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert not torch.equal(out[0], out[1])


@pytest.mark.parametrize("kind", ["eval", "train"])
def test_rows_outside_the_store_are_black_images(T, kind):
    h, w, S = 64, 32, 5
    dev = torch.device("cuda", 0)
    store = torch.from_numpy(np.stack(_images(np.random.default_rng(2), [(h, w)] * S))).to(dev)
    rows = [-1, S, 3, 2 ** 31 - 1, -2 ** 31]
    params = torch.from_numpy(_params(T, kind, len(rows), h, w)).to(dev)
    picked = torch.zeros(len(rows), h, w, 3, dtype=torch.uint8, device=dev)
    picked[2] = store[3]
    want = T.augment(picked, params)
    out = torch.full((len(rows), 3, h, w), float("nan"), device=dev)
    assert _gather(T, store, S, torch.tensor(rows, dtype=torch.int32, device=dev), params, len(rows), h, w, out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_gather_guards_launch_nothing(T):
    from daliid_amd import _lib
    h, w, S, n = 64, 32, 3, 2
    dev = torch.device("cuda", 0)
    store = torch.zeros(S, h, w, 3, dtype=torch.uint8, device=dev)
    rows = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    params = torch.from_numpy(T.eval_params(n)).to(dev)
    out = torch.full((n, 3, h, w), 7.0, device=dev)                       # poison: a launch would overwrite it
    INVALID = -1
    assert _gather(T, store, 0, rows, params, n, h, w, out) == INVALID     # store_rows >= 1
    assert "store_rows" in _lib.last_error()
    assert _gather(T, store, -4, rows, params, n, h, w, out) == INVALID
    assert _gather(T, None, S, rows, params, n, h, w, out) == INVALID      # null arguments
    assert _gather(T, store, S, None, params, n, h, w, out) == INVALID
    assert _gather(T, store, S, rows, None, n, h, w, out) == INVALID
    assert _gather(T, store, S, rows, params, -1, h, w, out) == INVALID    # sizes
    assert _gather(T, store, S, rows, params, n, 0, w, out) == INVALID
    assert _gather(T, store, S, rows, params, n, h, -2, out) == INVALID
    assert _gather(T, store, S, rows, params, n, 256, 256, out) == INVALID  # 192 KiB > the 150 KiB LDS limit
    assert "LDS" in _lib.last_error()
    m3 = (ctypes.c_float * 3)(*T.IMAGENET_MEAN)
    L = _lib.lib()
    assert L.dali_augment_gather(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(store), S, _lib.ptr(rows), _lib.ptr(params), n, h, w, None, m3,
                                 _lib.ptr(out)) == INVALID
    assert L.dali_augment_gather(None, _lib.stream_ptr(), _lib.ptr(store), S, _lib.ptr(rows), _lib.ptr(params), n, h, w, m3, m3,
                                 _lib.ptr(out)) == INVALID
    assert _gather(T, store, S, rows, params, 0, h, w, out) == 0          # an empty batch is fine and launches nothing either
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- the loaders ---------------------------------------------------------------------------------------------------------
def test_eval_loader_equals_the_uncached_one_cold_and_warm(T, tmp_path):
    paths = _write_ragged(tmp_path, 8)
    want = T.gpu_eval_loader(paths, 64, 32)
    calls, decode = _counting(T)
    store = T.ImageStore(64, 32, capacity=16, decode=decode)
    cold = store.eval_loader(paths, 64, 32)
    assert sorted(calls) == sorted(paths)
    warm = store.eval_loader(paths, 64, 32)
    torch.cuda.synchronize()
    assert len(calls) == len(paths)                                        # the second call decoded nothing
    assert cold.shape == (8, 3, 64, 32) and torch.equal(cold, want) and torch.equal(warm, want)
    assert store.stats == dict(hits=8, misses=8, decodes=8, uncached=0, rows_used=8)
    back = store.eval_loader(paths[::-1], 64, 32)                         # any order
    assert torch.equal(back, want.flip(0))
    with pytest.raises(T._lib.DaliError):
        store.eval_loader(paths, 128, 64)
    store.clear()
    assert store.stats["rows_used"] == 0 and torch.equal(store.eval_loader(paths[:3], 64, 32), want[:3]) and len(calls) == len(paths) + 3


def test_train_loader_torchvision_pk_batch_equals_the_uncached_one(T, tmp_path):
    from daliid_amd import train_encodersKIT as TK
    records, tdir = _write_dataset(tmp_path, 4, 5)
    labels = np.int32(records[:, 1])
    calls, decode = _counting(T)
    store = T.ImageStore(64, 32, capacity=4 * 5 * 6, decode=decode)
    dev = torch.device("cuda", 0)

    def run(loader, seeds=(21, 22)):
        np.random.seed(seeds[0]); torch.manual_seed(seeds[1])
        ds = TK.samplePKBatches("Market", records, labels, 64, 32, tdir, 1, K=3)
        imgs, lab, dist = ds.finish_batch(ds.plan_batch([2, 0, 3], loader), loader, dev)
        torch.cuda.synchronize()
        return imgs.cpu(), lab, dist, np.random.rand(), torch.rand(1).item()       # the generators end in the same state too

    a, b = run(T.gpu_train_loader), run(store.train_loader(sampler="torchvision"))
    assert a[0].shape == (18, 3, 64, 32) and torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]
    assert len(calls) == len(set(calls)) == store.stats["rows_used"] == 18
    c = run(store.train_loader())                                          # warm: the same files
    assert len(calls) == 18 and torch.equal(c[0], a[0]) and c[3] == a[3] and c[4] == a[4]
    # the per-identity __getitem__ path (loader called directly) serves from the store too
    TK.set_train_loader(store.train_loader())
    try:
        np.random.seed(21); torch.manual_seed(22)
        ds = TK.samplePKBatches("Market", records, labels, 64, 32, tdir, 1, K=3)
        direct = torch.cat([ds[i][0] for i in [2, 0, 3]], 0)
    finally:
        TK.set_train_loader(None)
    assert torch.equal(direct.cpu(), a[0]) and len(calls) == 18


@pytest.mark.parametrize("second_first", [False, True])
def test_prefetched_tickets_share_pending_fills(T, tmp_path, second_first):
    paths = _write_ragged(tmp_path, 6)
    a, b, c, d, e, f = paths
    first, second = [a, b, c], [c, d, d, a, e]
    want1, want2 = T.gpu_eval_loader(first, 64, 32), T.gpu_eval_loader(second, 64, 32)
    calls, decode = _counting(T)
    store = T.ImageStore(64, 32, capacity=8, decode=decode)
    ev = store.eval_loader
    t1 = ev.submit(ev.plan(first, 64, 32, None))
    t2 = ev.submit(ev.plan(second, 64, 32, None))                           # before either is finished
    if second_first:
        got2 = ev.finish(t2)                                                # completes ticket 1's fills first
        got1 = ev.finish(t1)
    else:
        got1 = ev.finish(t1)
        got2 = ev.finish(t2)
    torch.cuda.synchronize()
    assert sorted(calls) == sorted([a, b, c, d, e])                         # each distinct file decoded once
    assert store.stats["rows_used"] == 5 and len(set(store._index.values())) == 5
    assert torch.equal(got1, want1) and torch.equal(got2, want2)


def test_full_store_serves_the_overflow_uncached(T, tmp_path):
    paths = _write_ragged(tmp_path, 9)
    want = T.gpu_eval_loader(paths, 64, 32)
    calls, decode = _counting(T)
    store = T.ImageStore(64, 32, capacity=4, decode=decode)
    got = store.eval_loader(paths, 64, 32)
    assert torch.equal(got, want)
    assert store.stats["rows_used"] == 4 and store.stats["uncached"] == 5 and len(calls) == 9
    order = [8, 1, 8, 0, 5, 3, 2, 6, 7, 4]                                   # stored and overflow files mixed, one overflow file twice
    mixed = [paths[i] for i in order]
    torch.manual_seed(5)
    want_train = T.gpu_train_loader(mixed, 64, 32)
    torch.manual_seed(5)
    got_train = store.train_loader()(mixed, 64, 32)
    assert torch.equal(got_train, want_train)
    assert store.stats["rows_used"] == 4 and len(calls) == 9 + 5              # nothing evicted, the overflow decoded again (once each)
    n = len(calls)
    assert torch.equal(store.eval_loader(paths[:4], 64, 32), want[:4]) and len(calls) == n


def test_extract_features_twice_through_the_store(T, tmp_path):
    from daliid_amd import Encoders, getFeatures
    records, _ = _write_dataset(tmp_path, 5, 3, hw=(96, 40), turb=False, fmt="png")
    net = Encoders._DataParallelShim(Encoders.ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=3)).eval()
    calls, decode = _counting(T)
    store = T.ImageStore(64, 32, capacity=15, decode=decode)
    try:
        getFeatures.set_image_loader(T.gpu_eval_loader)
        uncached = getFeatures.extractFeatures(records, 64, 32, net, 4, gpu_index=0, verbose=False)          # batches of 4, 4, 4, 3
        getFeatures.set_image_loader(store.eval_loader)
        one = getFeatures.extractFeatures(records, 64, 32, net, 4, gpu_index=0, verbose=False)
        assert len(calls) == 15
        two = getFeatures.extractFeatures(records, 64, 32, net, 4, gpu_index=0, verbose=False)
    finally:
        getFeatures.set_image_loader(None)
    assert len(calls) == 15
    assert one.shape == (15, 1024) and torch.equal(one, two) and torch.equal(one, uncached)


def test_one_trainer_epoch_equals_the_default_loaders(T, tmp_path):
    """trainer.train (epoch inference, targets, PK steps with prefetch depth 2) on files with turbulence copies: the store with
    sampler="torchvision" against the default loaders from the same seeds -- the same statistics and bitwise the same two models."""
    from daliid_amd import Encoders, getFeatures
    from daliid_amd import train_encodersKIT as TK
    records, tdir = _write_dataset(tmp_path, 8, 6)
    labels = np.int32(records[:, 1])
    calls, decode = _counting(T)
    store = T.ImageStore(64, 32, capacity=8 * 6 * 6, decode=decode)

    def run(use_store):
        online = Encoders._DataParallelShim(Encoders.ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=7))
        momentum = Encoders._DataParallelShim(Encoders.ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=7))
        momentum.load_state_dict(online.state_dict())
        opt = torch.optim.Adam(online.parameters(), lr=3.5e-4, weight_decay=5e-4)
        tr = TK.trainer("Market", records, "resnet50", {}, 64, 32, tdir, False, 1, opt, 4, 4, 0.05, 0.9, 0.4, 250, online.eval(), momentum.eval(),
                        [0], "t")
        try:
            if use_store:
                getFeatures.set_image_loader(store.eval_loader)
                TK.set_train_loader(store.train_loader(sampler="torchvision"))
            np.random.seed(31); torch.manual_seed(32)
            tr.train(records, labels, 1, 1)
        finally:
            getFeatures.set_image_loader(None)
            TK.set_train_loader(None)
        torch.cuda.synchronize()
        return tr.last_epoch_stats, {k: v.clone() for k, v in online.state_dict().items()}, {k: v.clone() for k, v in momentum.state_dict().items()}

    base, cached = run(False), run(True)
    assert base[0]["steps"] == 2 and np.isfinite(base[0]["loss"])
    assert base[0] == cached[0]
    for a, b in ((base[1], cached[1]), (base[2], cached[2])):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert len(calls) == len(set(calls)) and store.stats["uncached"] == 0
    assert store.stats["rows_used"] == len(calls) >= 48


def test_batched_sampler_pk_batch_end_to_end(T, tmp_path):
    from daliid_amd import train_encodersKIT as TK
    records, tdir = _write_dataset(tmp_path, 4, 5)
    labels = np.int32(records[:, 1])
    store = T.ImageStore(64, 32, capacity=4 * 5 * 6)
    dev = torch.device("cuda", 0)

    def run(seed):
        loader = store.train_loader(sampler="batched", seed=seed)
        np.random.seed(21)
        ds = TK.samplePKBatches("Market", records, labels, 64, 32, tdir, 1, K=3)
        imgs, lab, dist = ds.finish_batch(ds.plan_batch([2, 0, 3], loader), loader, dev)
        torch.cuda.synchronize()
        return imgs

    a, b, c = run(1), run(1), run(2)
    assert a.shape == (18, 3, 64, 32) and torch.isfinite(a).all()
    assert (a[:, 0] == ERASED_R).any()                                     # an erased box
    assert torch.equal(a, b) and not torch.equal(a, c)

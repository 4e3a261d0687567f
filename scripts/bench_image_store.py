"""Epochs of ``trainer.train`` on real files: the uncached loaders (host decode + resize + augment per batch) against
``transforms.ImageStore`` (each file decoded and resized once, every later batch one dali_augment_gather launch from HBM).

Writes a Market-1501-shaped JPEG data set into a temporary directory (clean files + their five ``_turbstrength<k>`` copies; default
751 identities x 17 images of 128 x 64), then times, in ONE process and on the same files:
  uncached          gpu_eval_loader / gpu_train_loader                      (what the library did before the store)
  store cold        an empty store, sampler="torchvision"
  store warm tv     every file resident, sampler="torchvision"
  store warm batch  every file resident, sampler="batched"
Per phase: host milliseconds inside samplePKBatches.plan_batch + finish_batch per PK batch (the enqueueing thread's share), epoch-inference
images per second, seconds per epoch (host clock around work that ends in a device synchronise), files decoded.  Then, with HIP events after
warm-up (medians): the device time of one train step and of the gather launch against resize + augment for one PK batch.

    python scripts/bench_image_store.py [--ids 751 --per-id 17 --P 16 --K 12 --height 256 --width 128 --json out.json]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daliid_amd import Encoders, _lib, getFeatures  # noqa: E402
from daliid_amd import train_encodersKIT as TK  # noqa: E402
from daliid_amd import transforms as T  # noqa: E402


def write_dataset(root, n_ids, per_id, src_h, src_w, seed=3):
    """Clean JPEGs under root/clean, the five distorted copies of each under root/turb; encoded on the decode pool (PIL releases the GIL)."""
    from PIL import Image
    clean, tdir = os.path.join(root, "clean"), os.path.join(root, "turb")
    os.makedirs(clean); os.makedirs(tdir)
    yy, xx = np.mgrid[0:src_h, 0:src_w]

    def one(job):
        pid, k = job
        rng = np.random.default_rng(seed * 1000003 + pid * 131 + k)
        base = 127 + 100 * np.sin(yy / (5.0 + pid % 7))[..., None] * np.cos(xx / (4.0 + k % 5))[..., None] * np.array([1.0, 0.7, -0.8])
        im = np.clip(base + rng.normal(0, 30, size=(src_h, src_w, 3)), 0, 255).astype(np.uint8)
        name = "%04d_c%ds1_%06d_00" % (pid, 1 + k % 6, k)
        path = os.path.join(clean, name + ".jpg")
        Image.fromarray(im).save(path, quality=90)
        for s in range(1, 6):
            Image.fromarray(np.roll(im, s, axis=1)).save(os.path.join(tdir, "%s_turbstrength%d.jpg" % (name, s)), quality=90)
        return [path, str(pid), str(k % 6), "person"]
    jobs = [(pid, k) for pid in range(n_ids) for k in range(per_id)]
    return np.array(list(T.decode_pool().map(one, jobs))), tdir


class HostClock:
    """Accumulates the host time the PK loop spends in samplePKBatches.plan_batch and finish_batch."""

    def __init__(self):
        self.seconds, self.batches = 0.0, 0
        self._plan, self._finish = TK.samplePKBatches.plan_batch, TK.samplePKBatches.finish_batch

    def __enter__(self):
        clock, plan, finish = self, self._plan, self._finish

        def plan_batch(ds, ids, loader):
            t0 = time.perf_counter()
            r = plan(ds, ids, loader)
            clock.seconds += time.perf_counter() - t0
            return r

        def finish_batch(planned, loader, dev):
            t0 = time.perf_counter()
            r = finish(planned, loader, dev)
            clock.seconds += time.perf_counter() - t0
            clock.batches += 1
            return r
        TK.samplePKBatches.plan_batch, TK.samplePKBatches.finish_batch = plan_batch, staticmethod(finish_batch)
        return self

    def __exit__(self, *exc):
        TK.samplePKBatches.plan_batch, TK.samplePKBatches.finish_batch = self._plan, staticmethod(self._finish)
        return False


def median_event_ms(fn, warmup=3, reps=15):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ids", type=int, default=751)
    ap.add_argument("--per-id", type=int, default=17)
    ap.add_argument("--src-height", type=int, default=128)
    ap.add_argument("--src-width", type=int, default=64)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--P", type=int, default=16)
    ap.add_argument("--K", type=int, default=12)
    ap.add_argument("--small-net", action="store_true", help="ResNet50ReID(layers=(1,1,1,1), width=32): a quick functional run, not a measurement")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_store.py measures on the GPU; none is visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W = args.height, args.width
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())
    result = {"config": vars(args)}

    with tempfile.TemporaryDirectory(prefix="daliid_store_bench_") as root:
        t0 = time.perf_counter()
        records, tdir = write_dataset(root, args.ids, args.per_id, args.src_height, args.src_width)
        labels = np.int32(records[:, 1])
        n_files = 6 * len(records)
        print("wrote %d clean + %d distorted JPEGs of %d x %d in %.1f s" % (len(records), 5 * len(records), args.src_height, args.src_width,
                                                                           time.perf_counter() - t0), flush=True)
        kw = dict(layers=(1, 1, 1, 1), width=32) if args.small_net else {}
        online = Encoders._DataParallelShim(Encoders.ResNet50ReID(device=dev, seed=12, **kw))
        momentum = Encoders._DataParallelShim(Encoders.ResNet50ReID(device=dev, seed=12, **kw))
        opt = torch.optim.Adam(online.parameters(), lr=3.5e-4, weight_decay=5e-4)
        tr = TK.trainer("Market", records, "resnet50", {}, H, W, tdir, False, 1, opt, args.P, args.K, 0.05, 0.999, 0.4, 250, online, momentum,
                        [dev.index], "bench")
        store = T.ImageStore(H, W, capacity=n_files, device=dev)
        print("store: %d slots x %d x %d x 3 B = %.2f GB" % (n_files, H, W, n_files * H * W * 3 / 1e9), flush=True)

        def phase(name, eval_loader, train_loader, epochs=1):
            getFeatures.set_image_loader(eval_loader); TK.set_train_loader(train_loader)
            rows = []
            try:
                for _ in range(epochs):
                    d0 = store.stats["decodes"]
                    t_inf = [0.0]

                    def timed_inference(images, inner=type(tr).extract_train_features):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fvs = inner(tr, images)
                        torch.cuda.synchronize()
                        t_inf[0] += time.perf_counter() - t0
                        return fvs
                    tr.extract_train_features = timed_inference                        # the epoch's own inference pass, not an extra one
                    torch.cuda.synchronize()
                    with HostClock() as clock, quiet():
                        t0 = time.perf_counter()
                        tr.train(records, labels, 1, 10)
                        torch.cuda.synchronize()
                        t_epoch = time.perf_counter() - t0
                    del tr.extract_train_features
                    t_inf = t_inf[0]
                    rows.append(dict(phase=name, host_ms_per_batch=1e3 * clock.seconds / max(clock.batches, 1), batches=clock.batches,
                                     inference_img_per_s=len(records) / t_inf, epoch_s=t_epoch, decodes=store.stats["decodes"] - d0))
                    print("%-18s host %7.2f ms/batch (%d batches)  inference %8.0f img/s  epoch %6.2f s  store decodes %d"
                          % (name, rows[-1]["host_ms_per_batch"], clock.batches, rows[-1]["inference_img_per_s"], t_epoch, rows[-1]["decodes"]), flush=True)
            finally:
                getFeatures.set_image_loader(None); TK.set_train_loader(None)
            return rows

        table = []
        np.random.seed(12); torch.manual_seed(12)
        phase("warm-up (uncached)", T.gpu_eval_loader, T.gpu_train_loader)            # plan construction for every batch size, allocator, pool threads
        table += phase("uncached", T.gpu_eval_loader, T.gpu_train_loader, epochs=2)
        table += phase("store cold", store.eval_loader, store.train_loader(sampler="torchvision"))
        # make the store fully resident (an epoch touches one random strength per picked image only): every distorted file once
        t0 = time.perf_counter()
        d0 = store.stats["decodes"]
        everything = [getFeatures.turb_path(p, (tdir, s, "Market")) for s in range(1, 6) for p in records[:, 0]]
        for b in range(0, len(everything), 2000):
            store.eval_loader(everything[b:b + 2000], H, W)
        torch.cuda.synchronize()
        t_fill = time.perf_counter() - t0
        result["fill"] = dict(files=store.stats["decodes"] - d0, seconds=t_fill)
        print("filled the rest of the store: %d files in %.1f s (%.0f files/s); rows used %d of %d"
              % (result["fill"]["files"], t_fill, result["fill"]["files"] / t_fill, store.stats["rows_used"], store.capacity), flush=True)
        table += phase("store warm tv", store.eval_loader, store.train_loader(sampler="torchvision"), epochs=2)
        table += phase("store warm batch", store.eval_loader, store.train_loader(sampler="batched", seed=12), epochs=2)
        table += phase("uncached again", T.gpu_eval_loader, T.gpu_train_loader)     # the spread of the first phase, alternated
        result["epochs"] = table

        # ---- device times, HIP events ----
        from daliid_amd.losses import _codes, _sample_weights
        loader = store.train_loader(sampler="torchvision")
        ds = TK.samplePKBatches("Market", records, labels, H, W, tdir, 1, K=args.K)
        planned = ds.plan_batch(range(min(args.P, len(ds))), loader)
        files = list(planned[0].plan.files)                                            # one PK batch: P x K x (clean, distorted)
        n = len(files)
        batch, labels_f, dist = ds.finish_batch(planned, loader, dev)
        heads = tr.last_targets
        codes, w = _codes(labels_f, dev), _sample_weights(torch.from_numpy(dist), 10, 250, dev)
        acc = torch.zeros(6, device=dev)
        online.train()
        step_ms = median_event_ms(lambda: tr.train_step(heads, batch, codes, w, acc), warmup=3, reps=10)
        online.eval()
        arrs = [np.ascontiguousarray(T._decode_one(f)) for f in files]
        torch.manual_seed(1)
        params = torch.from_numpy(T.sample_train_params(n, H, W)).to(dev)
        rows = torch.from_numpy(np.array([store._index[f] for f in files], np.int32)).to(dev)
        u8 = torch.empty(n, H, W, 3, device=dev, dtype=torch.uint8)
        out = torch.empty(n, 3, H, W, device=dev)
        m3, s3 = (ctypes.c_float * 3)(*T.IMAGENET_MEAN), (ctypes.c_float * 3)(*T.IMAGENET_STD)
        L, ctx = _lib.lib(), _lib.ctx(dev)
        resize = T._resize_launcher(arrs, H, W, dev)                                   # inputs uploaded once: the events see the kernels only

        def augment():
            _lib.check(L.dali_augment_batch(ctx, _lib.stream_ptr(), _lib.ptr(u8), _lib.ptr(params), n, H, W, m3, s3, _lib.ptr(out)), "dali_augment_batch")

        def gather():
            _lib.check(L.dali_augment_gather(ctx, _lib.stream_ptr(), _lib.ptr(store._arena), store.capacity, _lib.ptr(rows), _lib.ptr(params), n, H, W,
                                             m3, s3, _lib.ptr(out)), "dali_augment_gather")
        resize_ms = median_event_ms(lambda: resize(u8))
        augment_ms = median_event_ms(augment)
        want = out.clone()
        gather_ms = median_event_ms(gather)
        assert torch.equal(out, want), "gather and resize + augment disagree"
        result["device_ms"] = dict(images=n, train_step=step_ms, resize=resize_ms, augment=augment_ms, gather=gather_ms)
        print("device, %d images: train step %.2f ms | resize %.3f + augment %.3f = %.3f ms | gather %.3f ms"
              % (n, step_ms, resize_ms, augment_ms, resize_ms + augment_ms, gather_ms), flush=True)
    for r in table:
        r["host_bound"] = bool(r["host_ms_per_batch"] >= step_ms)
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

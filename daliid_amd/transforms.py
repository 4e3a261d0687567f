"""The image side of the input pipeline on the GPU: what the reference does per image with
torchvision transforms on PIL images (``getFeatures.sample`` getFeatures.py:18-19; ``samplePKBatches.transform``
train_encodersKIT.py:313-320), batched on HIP kernels (``dali_resize_bicubic_u8``, ``dali_augment_batch``), and ``ImageStore``: the resized
images kept in HBM, every later batch one ``dali_augment_gather`` launch.

JPEG decode stays on the host.  Random parameters are drawn here, per image and in torchvision's call order, from
torch's global CPU generator (the reference's transforms draw from it too); the kernels are deterministic pixel
arithmetic that reproduces PIL's 8-bit results bit for bit.  torchvision is not installed in the build image and the
reference pins no version: the draw order follows torchvision 0.1x's ``RandomCrop.get_params``, ``RandomHorizontalFlip``,
``ColorJitter.get_params`` and ``RandomErasing.get_params``.
"""
import ctypes
import math
from functools import lru_cache

import numpy as np
import torch

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 32 - 8 - 2
AUG_WORDS = 16


# ---- Pillow's resampling coefficients (src/libImaging/Resample.c: bicubic_filter, precompute_coeffs, normalize_coeffs_8bpc)
def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@lru_cache(maxsize=256)
def resize_coeffs(in_size, out_size):
    """-> (ksize, bounds int32 [out,2] = (first input index, taps), coefs int32 [out,ksize] in 22-bit fixed point)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coefs = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        bounds[xx] = (xmin, xmax)
        for x, w in enumerate(k):
            coefs[xx, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
    return ksize, bounds, coefs


def resize_u8_reference(img, out_h, out_w):
    """numpy restatement of the two 8-bit passes with the tables above (CPU check of the table builder against PIL)."""
    def one_pass(a, out_size):                      # resample axis 1 of [rows][n][3]
        ks, bounds, coefs = resize_coeffs(a.shape[1], out_size)
        out = np.empty((a.shape[0], out_size, a.shape[2]), dtype=np.uint8)
        ai = a.astype(np.int64)
        for xx in range(out_size):
            x0, n = bounds[xx]
            ssum = (1 << (PRECISION_BITS - 1)) + (ai[:, x0:x0 + n, :] * coefs[xx, :n].astype(np.int64)[None, :, None]).sum(1)
            out[:, xx, :] = np.clip(ssum >> PRECISION_BITS, 0, 255)
        return out
    tmp = one_pass(np.asarray(img), out_w)                                   # horizontal first
    return one_pass(tmp.transpose(1, 0, 2), out_h).transpose(1, 0, 2)       # then vertical


def _resize_launcher(arrs, out_h, out_w, dev, lane=0):
    """Host share of one resize of the (non-empty) list of contiguous uint8 [h,w,3] arrays: the coefficient tables of the sizes present, ONE packed
    upload of the pixels and the small index arrays.  -> launch(out): enqueues dali_resize_bicubic_u8 into ``out`` [n,out_h,out_w,3] (it keeps
    the uploaded tensors alive; calling it again repeats the launch on the same inputs)."""
    n = len(arrs)
    sizes = sorted({a.shape[:2] for a in arrs})
    tab = {sz: i for i, sz in enumerate(sizes)}
    ks_h = max(resize_coeffs(w, out_w)[0] for _, w in sizes)
    ks_v = max(resize_coeffs(h, out_h)[0] for h, _ in sizes)
    bh = np.zeros((len(sizes), out_w, 2), np.int32); ch = np.zeros((len(sizes), out_w, ks_h), np.int32)
    bv = np.zeros((len(sizes), out_h, 2), np.int32); cv = np.zeros((len(sizes), out_h, ks_v), np.int32)
    for (h, w), i in tab.items():
        k, b, c = resize_coeffs(w, out_w); bh[i] = b; ch[i, :, :k] = c
        k, b, c = resize_coeffs(h, out_h); bv[i] = b; cv[i, :, :k] = c
    offs = np.zeros(n, np.int64)
    pos = 0
    for i, a in enumerate(arrs):
        assert a.ndim == 3 and a.shape[2] == 3, "RGB uint8 images expected"
        offs[i] = pos
        pos += a.size
    packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(dev, non_blocking=True)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
    t_off, t_h, t_w = up(offs), up(np.array([a.shape[0] for a in arrs], np.int32)), up(np.array([a.shape[1] for a in arrs], np.int32))
    t_tab = up(np.array([tab[a.shape[:2]] for a in arrs], np.int32))
    t_bh, t_ch, t_bv, t_cv = up(bh), up(ch), up(bv), up(cv)
    max_in_h = max(a.shape[0] for a in arrs)

    def launch(out):
        _lib.check(_lib.lib().dali_resize_bicubic_u8(_lib.ctx(dev, lane), _lib.stream_ptr(), _lib.ptr(packed), _lib.ptr(t_off), _lib.ptr(t_h), _lib.ptr(t_w),
                                                      _lib.ptr(t_tab), n, max_in_h, _lib.ptr(t_bh), _lib.ptr(t_ch), ks_h, _lib.ptr(t_bv), _lib.ptr(t_cv),
                                                      ks_v, out_h, out_w, _lib.ptr(out)), "dali_resize_bicubic_u8")
    return launch


def resize_bicubic_u8(images, out_h, out_w, device=None, lane=0, out=None):
    """images: sequence of uint8 [h,w,3] arrays (numpy or CPU tensors) of any sizes -> uint8 CUDA tensor [N,out_h,out_w,3]
    = PIL ``img.resize((out_w, out_h), Image.BICUBIC)`` for each.  The horizontally resampled intermediate lives in the workspace of
    the context ``_lib.ctx(device, lane)``: a caller on a stream that runs beside the main one passes its own lane.
    ``out``: a contiguous uint8 CUDA tensor [N,out_h,out_w,3] to write into (ImageStore: N consecutive slots of its arena) instead of a new one."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    arrs = [np.ascontiguousarray(np.asarray(im), dtype=np.uint8) for im in images]
    n = len(arrs)
    if out is None:
        out = torch.empty(n, out_h, out_w, 3, device=dev, dtype=torch.uint8)
    elif tuple(out.shape) != (n, out_h, out_w, 3) or out.dtype != torch.uint8 or out.device != dev:
        raise _lib.DaliError("resize_bicubic_u8: out must be uint8 [%d,%d,%d,3] on %s, got %s %s on %s"
                             % (n, out_h, out_w, dev, out.dtype, tuple(out.shape), out.device))
    if n == 0:
        return out
    launch = _resize_launcher(arrs, out_h, out_w, dev, lane)
    launch(out)
    return out


# ---- random parameters in torchvision's order ------------------------------------------------------------------
def _f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


def sample_train_params(n, height, width, padding=10, brightness=0.4, contrast=0.3, saturation=0.4, erase_p=1.0,
                        erase_scale=(0.05, 0.30), erase_ratio=(0.3, 3.3)):
    """Per image: RandomCrop((H,W), padding) -> RandomHorizontalFlip(0.5) -> ColorJitter(b, c, s, hue=0) ->
    RandomErasing(p, scale, ratio) parameters (train_encodersKIT.py:313-320), int32 [n,16] (layout: dali_augment_batch)."""
    p = np.zeros((n, AUG_WORDS), dtype=np.int32)
    log_ratio = (math.log(erase_ratio[0]), math.log(erase_ratio[1]))
    area = height * width
    for i in range(n):
        # RandomCrop.get_params on the padded image
        top = int(torch.randint(0, 2 * padding + 1, size=(1,)).item())
        left = int(torch.randint(0, 2 * padding + 1, size=(1,)).item())
        flip = int(torch.rand(1).item() < 0.5)
        # ColorJitter.get_params: permutation first, then the factors; hue = 0 -> None (no draw)
        order = torch.randperm(4).tolist()
        b = float(torch.empty(1).uniform_(max(0.0, 1 - brightness), 1 + brightness))
        c = float(torch.empty(1).uniform_(max(0.0, 1 - contrast), 1 + contrast))
        s = float(torch.empty(1).uniform_(max(0.0, 1 - saturation), 1 + saturation))
        # RandomErasing.forward: the p draw, then get_params (up to 10 attempts)
        ei = ej = eh = ew = 0
        if torch.rand(1).item() < erase_p:
            for _ in range(10):
                erase_area = area * torch.empty(1).uniform_(erase_scale[0], erase_scale[1]).item()
                aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
                h = int(round(math.sqrt(erase_area * aspect)))
                w = int(round(math.sqrt(erase_area / aspect)))
                if not (h < height and w < width):
                    continue
                ei = int(torch.randint(0, height - h + 1, size=(1,)).item())
                ej = int(torch.randint(0, width - w + 1, size=(1,)).item())
                eh, ew = h, w
                break
        p[i] = [top, left, flip, *order, ei, ej, eh, ew, _f32_bits(b), _f32_bits(c), _f32_bits(s), padding, 1]
    return p


def sample_train_params_batched(n, height, width, rng, padding=10, brightness=0.4, contrast=0.3, saturation=0.4, erase_p=1.0,
                                erase_scale=(0.05, 0.30), erase_ratio=(0.3, 3.3)):
    """``sample_train_params`` for n images at once from a ``numpy.random.Generator``: the same [n,16] layout and the same per-image
    distributions, drawn in a fixed number of vectorised calls (no per-image loop; the sequential sampler costs more host time per PK batch
    than the device step).  NOT torchvision's random stream, hence opt-in (``ImageStore.train_loader(sampler="batched")``).
    All ten RandomErasing attempts of every image are drawn at once and the first that fits (h < H and w < W) is kept: attempts are
    i.i.d., so drawing the ones after the kept one changes nothing."""
    p = np.zeros((n, AUG_WORDS), dtype=np.int32)
    p[:, 0:2] = rng.integers(0, 2 * padding + 1, size=(n, 2))                # RandomCrop: top, left
    p[:, 2] = rng.random(n) < 0.5                                            # flip
    p[:, 3:7] = np.argsort(rng.random((n, 4)), axis=1)                       # ranks of 4 i.i.d. uniforms: a uniform permutation
    for k, x in enumerate((brightness, contrast, saturation)):
        lo, hi = np.float32(max(0.0, 1 - x)), np.float32(1 + x)
        p[:, 11 + k] = np.clip(rng.uniform(lo, hi, size=n).astype(np.float32), lo, hi).view(np.int32)
    tries = 10
    area = height * width * rng.uniform(erase_scale[0], erase_scale[1], size=(n, tries))
    aspect = np.exp(rng.uniform(math.log(erase_ratio[0]), math.log(erase_ratio[1]), size=(n, tries)))
    eh = np.rint(np.sqrt(area * aspect)).astype(np.int64)
    ew = np.rint(np.sqrt(area / aspect)).astype(np.int64)
    fits = (eh < height) & (ew < width)
    first = np.argmax(fits, axis=1)                                          # first fitting attempt (0 where none fits: masked by `keep`)
    keep = fits.any(axis=1) & (rng.random(n) < erase_p)
    at = np.arange(n)
    eh, ew = np.where(keep, eh[at, first], 0), np.where(keep, ew[at, first], 0)
    ei, ej = rng.integers(0, height - eh + 1), rng.integers(0, width - ew + 1)      # uniform on 0 .. H - h, per image
    p[:, 7], p[:, 8], p[:, 9], p[:, 10] = np.where(keep, ei, 0), np.where(keep, ej, 0), eh, ew
    p[:, 14], p[:, 15] = padding, 1
    return p


def eval_params(n):
    p = np.zeros((n, AUG_WORDS), dtype=np.int32)
    p[:, 3:7] = -1
    return p


def augment(images_u8, params, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """images_u8: uint8 CUDA [N,H,W,3]; params int32 [N,16] (numpy or tensor) -> fp32 CUDA [N,3,H,W]."""
    n, h, w, _ = images_u8.shape
    dev = images_u8.device
    prm = torch.as_tensor(np.ascontiguousarray(params), dtype=torch.int32).to(dev) if not isinstance(params, torch.Tensor) else params.to(dev, torch.int32).contiguous()
    assert tuple(prm.shape) == (n, AUG_WORDS)
    out = torch.empty(n, 3, h, w, device=dev, dtype=torch.float32)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _lib.check(_lib.lib().dali_augment_batch(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(images_u8.contiguous()), _lib.ptr(prm), n, h, w, m3, s3,
                                              _lib.ptr(out)), "dali_augment_batch")
    return out


# ---- loaders that plug into getFeatures.set_image_loader / train_encodersKIT.set_train_loader -------------------------
# Host side of the pipeline (the reference: torch DataLoader with 8 worker processes, train_encodersKIT.py:77-83, getFeatures.py:52).
# JPEG decode is the host's share: PIL releases the GIL while it decodes, so a thread pool scales with the cores, and a batch is
# SUBMITTED (its files start decoding) before the previous batch's GPU work is enqueued and FINISHED (one packed upload, ONE
# dali_resize_bicubic_u8 + ONE dali_augment_batch launch for the whole batch, on a side stream) when it is needed:
#     ticket = loader.submit(plan)   ...   images = loader.finish(ticket)
# Random augmentation parameters are drawn at PLAN time, on the calling thread, in the order the sequential per-call path draws
# them, so the batched path reproduces it bit for bit.
_pool = None
_side = {}


def decode_pool():
    """The process-wide decode pool: DALIID_DECODE_THREADS threads (default: the CPUs this process may run on, at most 16)."""
    global _pool
    if _pool is None:
        import os
        from concurrent.futures import ThreadPoolExecutor
        try:
            ncpu = len(os.sched_getaffinity(0))
        except AttributeError:
            ncpu = os.cpu_count() or 1
        _pool = ThreadPoolExecutor(max_workers=max(1, int(os.environ.get("DALIID_DECODE_THREADS", min(16, ncpu)))), thread_name_prefix="dali-decode")
    return _pool


def _decode_one(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))                        # torchreid.utils.tools.read_image


def _decode(paths):
    if len(paths) <= 2:
        return [_decode_one(p) for p in paths]
    return list(decode_pool().map(_decode_one, paths))


def _turb_path(path, turb):
    from .getFeatures import turb_path
    return turb_path(path, turb)


def _side_stream(dev):
    key = (dev.type, dev.index)
    if key not in _side:
        _side[key] = torch.cuda.Stream(device=dev)
    return _side[key]


class ImagePlan:
    """What one loader call would do, with every random draw already made: files to decode + their [n,16] parameter rows."""
    __slots__ = ("files", "params", "height", "width")

    def __init__(self, files, params, height, width):
        self.files, self.params, self.height, self.width = files, params, height, width

    @staticmethod
    def concat(plans, order=None):
        """One plan for many (all of one output size); ``order``: permutation of the concatenated images (the final batch order)."""
        files = [f for p in plans for f in p.files]
        params = np.concatenate([p.params for p in plans], 0) if plans else np.zeros((0, AUG_WORDS), np.int32)
        if order is not None:
            files, params = [files[i] for i in order], params[np.asarray(order)]
        return ImagePlan(files, params, plans[0].height, plans[0].width)


class _Ticket:
    __slots__ = ("plan", "futures")

    def __init__(self, plan, futures):
        self.plan, self.futures = plan, futures


def submit(plan, decode=None):
    """Start decoding the plan's files on the pool (returns at once)."""
    fn = decode or _decode_one
    return _Ticket(plan, [decode_pool().submit(fn, f) for f in plan.files])


def finish(ticket, device=None, side_stream=True):
    """Wait for the decodes, then ONE resize launch + ONE augment launch for the whole plan.  With ``side_stream`` the upload and the two
    kernels run on the device's side stream (under whatever the current stream is computing) and the current stream waits for them."""
    arrs = [f.result() for f in ticket.futures]
    plan = ticket.plan
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if not side_stream:
        return augment(resize_bicubic_u8(arrs, plan.height, plan.width, dev), plan.params)
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    with torch.cuda.stream(side):
        # the side stream's own context: the resize keeps its intermediate in the context's workspace, and the main stream's kernels (Adam's
        # partial sums, the targets, the distance pre-pass) use THEIR context's workspace at the same time
        u8 = resize_bicubic_u8(arrs, plan.height, plan.width, dev, lane="side")
        out = augment(u8, plan.params)
    main.wait_stream(side)
    out.record_stream(main)
    return out


def plan_eval(paths, img_height, img_width, turb=None):
    files = [_turb_path(p, turb) for p in paths] if turb else list(paths)
    return ImagePlan(files, eval_params(len(files)), img_height, img_width)


def plan_train(paths, img_height, img_width, turb=None):
    files = [_turb_path(p, turb) for p in paths] if turb else list(paths)
    return ImagePlan(files, sample_train_params(len(files), img_height, img_width), img_height, img_width)


def gpu_eval_loader(paths, img_height, img_width, turb=None, decode=_decode):
    """getFeatures.sample.__getitem__ for a list of paths: decode (host) -> bicubic resize -> ToTensor -> Normalize (GPU)."""
    plan = plan_eval(paths, img_height, img_width, turb)
    return augment(resize_bicubic_u8(decode(plan.files), img_height, img_width), plan.params)


def gpu_train_loader(paths, img_height, img_width, turb=None, decode=_decode):
    """samplePKBatches.transform for a list of paths (train_encodersKIT.py:313-320)."""
    plan = plan_train(paths, img_height, img_width, turb)
    return augment(resize_bicubic_u8(decode(plan.files), img_height, img_width), plan.params)


# the batched protocol of the two loaders (train_encodersKIT.samplePKBatches.plan / getFeatures.extractFeatures use it when present)
gpu_eval_loader.plan, gpu_eval_loader.submit, gpu_eval_loader.finish = plan_eval, submit, finish
gpu_train_loader.plan, gpu_train_loader.submit, gpu_train_loader.finish = plan_train, submit, finish


# ---- ImageStore: resized images resident in HBM ---------------------------------------------------------------------------
# A resized uint8 image is a pure function of its file and of (height, width): 96 KiB at 256 x 128, so Market-1501's train set with its
# five turbulence strengths (12,936 x 6 files) is 7.6 GB and MSMT17's about 19 GB -- a small share of the card's HBM.  The store decodes
# and resizes each file ONCE; every later batch is ONE dali_augment_gather launch over the arena, and the host's share per batch is one
# dict lookup per file and one small upload (rows + parameters).
class StorePlan(ImagePlan):
    """An ImagePlan whose ``params`` may be None: the batched sampler draws them at submit, once, for all images in their final order."""
    __slots__ = ()

    @staticmethod
    def concat(plans, order=None):
        files = [f for p in plans for f in p.files]
        lazy = [p.params is None for p in plans]
        if any(lazy) and not all(lazy):
            raise _lib.DaliError("StorePlan.concat: plans with and without drawn parameters cannot be merged")
        params = None if all(lazy) and plans else (np.concatenate([p.params for p in plans], 0) if plans else np.zeros((0, AUG_WORDS), np.int32))
        if order is not None:
            files = [files[i] for i in order]
            params = params if params is None else params[np.asarray(order)]
        return StorePlan(files, params, plans[0].height, plans[0].width)


class _Fill:
    """Files that a submit gave consecutive new slots [slot0, slot0 + len(files)); their decodes run on the pool until a finish resizes them in."""
    __slots__ = ("seq", "slot0", "files", "futures")

    def __init__(self, seq, slot0, files, futures):
        self.seq, self.slot0, self.files, self.futures = seq, slot0, files, futures


class _StoreTicket:
    __slots__ = ("plan", "params", "rows", "seq", "generation", "temp_futures", "temp_at")

    def __init__(self, plan, params, rows, seq, generation, temp_futures, temp_at):
        self.plan, self.params, self.rows, self.seq, self.generation = plan, params, rows, seq, generation
        self.temp_futures, self.temp_at = temp_futures, temp_at


class _StoreLoader:
    """A loader over an ImageStore: callable like ``gpu_eval_loader`` / ``gpu_train_loader`` and with their plan / submit / finish protocol."""

    def __init__(self, store, train, sampler, seed):
        if sampler not in ("torchvision", "batched"):
            raise ValueError("sampler must be 'torchvision' or 'batched', got %r" % (sampler,))
        self.store, self.train, self.sampler = store, train, sampler
        self.rng = np.random.default_rng(seed) if sampler == "batched" else None

    def plan(self, paths, img_height, img_width, turb=None):
        st = self.store
        if (img_height, img_width) != (st.height, st.width):
            raise _lib.DaliError("ImageStore holds %d x %d images, asked for %d x %d (one store per size)" % (st.height, st.width, img_height, img_width))
        files = [_turb_path(p, turb) for p in paths] if turb else list(paths)
        if not self.train:
            params = eval_params(len(files))
        elif self.sampler == "torchvision":
            params = sample_train_params(len(files), img_height, img_width)        # at plan time, in the uncached path's draw order
        else:
            params = None                                                            # drawn at submit
        return StorePlan(files, params, img_height, img_width)

    def submit(self, plan):
        params = plan.params
        if params is None:
            if self.rng is None:
                raise _lib.DaliError("a plan without parameters needs the loader of train_loader(sampler='batched')")
            params = sample_train_params_batched(len(plan.files), plan.height, plan.width, self.rng)
        return self.store._submit(plan, params)

    def finish(self, ticket, device=None):
        return self.store._finish(ticket, device)

    def __call__(self, paths, img_height, img_width, turb=None):
        return self.finish(self.submit(self.plan(paths, img_height, img_width, turb)))


class ImageStore:
    """A device arena of ``capacity`` resized uint8 images of ONE output size (height, width), allocated once at first use
    (capacity x height x width x 3 bytes), and a host dict from file path -- the path actually opened, i.e. after the turbulence mapping
    of ``getFeatures.turb_path`` -- to its slot.

        store = ImageStore(256, 128, capacity=6 * len(train_files))
        getFeatures.set_image_loader(store.eval_loader)
        train_encodersKIT.set_train_loader(store.train_loader())

    A file a plan needs and the store lacks is decoded on ``decode_pool()`` and resized (the Pillow-exact ``dali_resize_bicubic_u8``)
    straight into its slot, so a stored image is bitwise what the uncached loaders compute for that file; every batch is then one
    ``dali_augment_gather`` launch.  Slots are assigned at ``submit``: a file whose fill is still pending in an earlier ticket is neither
    decoded again nor given a second slot, a file listed twice in a plan is decoded once, and ``finish`` of a ticket first completes the
    pending fills of every earlier ticket.  Fills and gathers run on the device's side stream (ordered among themselves); the current
    stream waits for the result.  When the store is full, further new files are served through a temporary, as the uncached path would,
    and are not stored; nothing is evicted.

    A file is ASSUMED NOT TO CHANGE on disk while it is in the store (``clear()`` drops everything).  ``decode``: path -> uint8 [h,w,3]
    array (default: PIL, as the uncached loaders).  Submit / finish are meant for one thread, as the two in-tree callers use them."""

    def __init__(self, height, width, capacity, device=None, decode=None):
        if height <= 0 or width <= 0 or capacity < 1:
            raise ValueError("ImageStore needs positive sizes and capacity >= 1")
        self.height, self.width, self.capacity = int(height), int(width), int(capacity)
        self.device = torch.device(device) if device is not None else None
        self._decode = decode
        self._generation = 0
        self.eval_loader = _StoreLoader(self, False, "torchvision", None)
        self.clear()

    def clear(self):
        """Drop every stored image, the arena and the statistics.  Tickets submitted before are void."""
        self._arena, self._index, self._fills, self._used, self._seq, self._failed = None, {}, [], 0, 0, None
        self._generation += 1
        self._stats = dict(hits=0, misses=0, decodes=0, uncached=0)

    @property
    def stats(self):
        """hits: images served from a slot (filled or pending); misses: images that needed a decode; decodes: files decoded; uncached: files
        served through a temporary because the store was full; rows_used: slots taken."""
        return dict(self._stats, rows_used=self._used)

    def train_loader(self, sampler="torchvision", seed=None):
        """sampler="torchvision": parameters drawn at plan time by ``sample_train_params`` from torch's global generator, in the uncached
        path's order (bitwise the uncached batches, both global generators left in the same state).  sampler="batched": drawn at submit by
        ``sample_train_params_batched`` from ``numpy.random.default_rng(seed)`` -- the same distributions, another random stream."""
        return _StoreLoader(self, True, sampler, seed)

    # -- host side: no GPU work before finish --
    def _submit(self, plan, params):
        if (plan.height, plan.width) != (self.height, self.width):
            raise _lib.DaliError("ImageStore holds %d x %d images, the plan is for %d x %d" % (self.height, self.width, plan.height, plan.width))
        params = np.ascontiguousarray(params, dtype=np.int32)
        n = len(plan.files)
        assert params.shape == (n, AUG_WORDS)
        fn = self._decode or _decode_one
        pool = decode_pool()
        rows = np.empty(n, np.int32)
        new, temp, temp_at = [], {}, []
        for i, f in enumerate(plan.files):
            slot = self._index.get(f)
            if slot is not None:
                self._stats["hits"] += 1
            elif f in temp:                                   # listed twice, store full: one decode serves both
                temp_at[temp[f]].append(i)
                slot = -1
            elif self._used < self.capacity:
                slot = self._index[f] = self._used
                self._used += 1
                new.append(f)
                self._stats["misses"] += 1
            else:
                temp[f] = len(temp_at)
                temp_at.append([i])
                slot = -1
                self._stats["misses"] += 1
                self._stats["uncached"] += 1
            rows[i] = slot
        self._seq += 1
        if new:
            self._fills.append(_Fill(self._seq, self._used - len(new), new, [pool.submit(fn, f) for f in new]))
        temp_futures = [pool.submit(fn, f) for f in temp]      # dict order = temp_at order
        self._stats["decodes"] += len(new) + len(temp)
        return _StoreTicket(plan, params, rows, self._seq, self._generation, temp_futures, temp_at)

    # -- device side --
    def _complete_fills(self, upto_seq, dev):
        """Resize the decoded files of every pending fill up to ticket ``upto_seq`` into their slots (ONE resize launch per fill); on the side stream."""
        while self._fills and self._fills[0].seq <= upto_seq:
            fill = self._fills[0]
            try:
                arrs = [f.result() for f in fill.futures]
                resize_bicubic_u8(arrs, self.height, self.width, dev, lane="side", out=self._arena[fill.slot0:fill.slot0 + len(arrs)])
            except Exception as e:                             # the slots are indexed but hold nothing: refuse to serve until clear()
                self._failed = e
                raise
            self._fills.pop(0)

    def _finish(self, ticket, device=None):
        if ticket.generation != self._generation:
            raise _lib.DaliError("ImageStore: the ticket was submitted before clear()")
        if self._failed is not None:
            raise _lib.DaliError("ImageStore: an earlier fill failed (%r); clear() the store" % (self._failed,))
        here = torch.device("cuda", torch.cuda.current_device())
        whole = lambda d: here if d is None or d.index is None else d          # "cuda" without an ordinal = the current device
        self.device = whole(self.device)
        dev = whole(torch.device(device)) if device is not None else self.device
        if dev != self.device:
            raise _lib.DaliError("ImageStore lives on %s, finish asked for %s" % (self.device, dev))
        n, h, w = len(ticket.plan.files), self.height, self.width
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev)
        with torch.cuda.stream(side):
            if self._arena is None:
                self._arena = torch.empty(self.capacity, h, w, 3, device=dev, dtype=torch.uint8)
            self._complete_fills(ticket.seq, dev)
            out = torch.empty(n, 3, h, w, device=dev, dtype=torch.float32)
            if n:
                m3, s3 = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
                L, ctx = _lib.lib(), _lib.ctx(dev, "side")
                # ONE upload: the n rows, then the n x 16 parameter words
                up = torch.from_numpy(np.concatenate([ticket.rows, ticket.params.reshape(-1)])).to(dev, non_blocking=True)
                if not ticket.temp_futures:
                    _lib.check(L.dali_augment_gather(ctx, _lib.stream_ptr(), _lib.ptr(self._arena), self.capacity, _lib.ptr(up[:n]), _lib.ptr(up[n:]),
                                                     n, h, w, m3, s3, _lib.ptr(out)), "dali_augment_gather")
                else:
                    # store full: the files without a slot are resized into a temporary, as the uncached path does, the stored ones copied
                    # beside them, and the batch goes through dali_augment_batch
                    tmp = resize_bicubic_u8([f.result() for f in ticket.temp_futures], h, w, dev, lane="side")
                    u8 = self._arena.index_select(0, up[:n].clamp(min=0))
                    src = [k for k, at in enumerate(ticket.temp_at) for _ in at]
                    dst = [i for at in ticket.temp_at for i in at]
                    u8[torch.tensor(dst, device=dev)] = tmp[torch.tensor(src, device=dev)]
                    _lib.check(L.dali_augment_batch(ctx, _lib.stream_ptr(), _lib.ptr(u8), _lib.ptr(up[n:]), n, h, w, m3, s3, _lib.ptr(out)),
                               "dali_augment_batch")
        main.wait_stream(side)
        out.record_stream(main)
        return out

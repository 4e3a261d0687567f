"""GPU: template (set) evaluation -- ops_eval.pool_templates / segment_reduce2d / link_templates / open_set_search / open_set_metrics and
validateModels.setTemplates / report_open_set -- against tests/templates_ref.py: the kernels bit for bit against the float32 emulation of
their documented arithmetic order (min / max / the open-set search: exactly), the pooled rows against float64 within a derived bound,
the wiring bit for bit against the composition of the public pieces.  Shapes are the smallest that cross every boundary of the kernels
(the 8-member unroll, the 16-byte and the scalar path, more than one workgroup, 256-column windows and chunks), not workload sizes."""
import numpy as np
import pytest
import torch

import templates_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _on_device(dev, a, misaligned=False):
    """a contiguous tensor; ``misaligned``: a view that starts 4 bytes into a 16-byte aligned buffer (the scalar path)"""
    if not misaligned:
        return torch.from_numpy(a).to(dev)
    buf = torch.empty(a.size + 1, device=dev, dtype=torch.float32)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# ---- pool_templates ----

def _lengths(T, d):
    """template lengths mixing 1, 2, 63, 64, 65 and 1000 (below, at and above the 8-member unroll and its remainder loop)"""
    if T == 1:
        return [{1: 1000, 3: 65, 8: 64, 260: 63, 2048: 2}[d]]
    if T == 5:
        return [65, 1, 1000, 64, 2] if d in (3, 260) else [63, 2, 1, 65, 64]
    return [1000, 1, 2, 63, 64, 65] + [1 + (i % 3) for i in range(T - 6)]


def _pool_case(d, T):
    rng = np.random.default_rng(d * 1000 + T)
    lengths = _lengths(T, d)
    n = int(sum(lengths))
    bounds = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    order = rng.permutation(n).astype(np.int32)
    if n > 1:
        assert not np.array_equal(order, np.arange(n))
    fvs = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2, (n, 1))).astype(F32)
    fvs[rng.random((n, d)) < 0.02] = 0.0
    w = rng.uniform(0.25, 4, n).astype(F32)
    return fvs, order, bounds, w


def _check_pool(dev, fvs, order, bounds, w, misaligned=False):
    from daliid_amd import ops_eval
    fd = _on_device(dev, fvs, misaligned)
    wd = torch.from_numpy(w).to(dev)
    counts = np.diff(bounds)[:, None]
    for mode, weights in (("mean", None), ("mean", w), ("max", None)):
        got = ops_eval.pool_templates(fd, order, bounds, mode, None if weights is None else wd)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(bounds) - 1, fvs.shape[1])
        assert np.array_equal(_bits(got), _bits(R.pool_f32(fvs, order, bounds, weights, mode))), (mode, weights is not None)
        ref, scale, _ = R.pool_f64(fvs, order, bounds, weights, mode)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        assert np.all(err <= (counts + 3) * 2.0 ** -24 * scale), (mode, float((err / np.maximum((counts + 3) * 2.0 ** -24 * scale, 1e-300)).max()))
    return fd


@pytest.mark.parametrize("T", [1, 5, 257])
@pytest.mark.parametrize("d", [1, 3, 8, 260, 2048])
def test_pool_templates_bitwise_and_against_float64(dev, d, T):
    """bit for bit the emulation (mean, weighted mean, max), and within (n_t + 3) 2^-24 sum |w f| / sum w of float64 per element: n_t
    products, n_t additions, the weight sum's roundings and the division, each at most half an ulp of a partial sum that sum |w f|
    bounds (first order; holds for any summation order; exact for max, whose scale is 0)"""
    _check_pool(dev, *_pool_case(d, T))


@pytest.mark.parametrize("d,T", [(8, 5), (260, 5), (2048, 1), (8, 257)])
def test_pool_templates_scalar_path(dev, d, T):
    """a base pointer 4 bytes into a 16-byte aligned buffer: d % 4 == 0 but the rows are read 4 bytes per lane"""
    _check_pool(dev, *_pool_case(d, T), misaligned=True)


def test_pool_templates_derived_weights_and_device_index(dev):
    """"magnitude" / "unit_mean" are the weighted mean with the norms / reciprocal norms of l2norm_rows; order / bounds may live on the
    device; the result does not depend on the number of templates pooled in one call"""
    from daliid_amd import ops_eval
    fvs, order, bounds, _ = _pool_case(260, 257)
    fd = torch.from_numpy(fvs).to(dev)
    _, norms = ops_eval.l2norm_rows(fd, return_norms=True)
    od, bd = torch.from_numpy(order).to(dev), torch.from_numpy(bounds).to(dev)
    mag = ops_eval.pool_templates(fd, od, bd, "magnitude")
    assert torch.equal(mag, ops_eval.pool_templates(fd, order, bounds, "mean", norms))
    assert np.array_equal(_bits(mag), _bits(R.pool_f32(fvs, order, bounds, norms.cpu().numpy())))
    unit = ops_eval.pool_templates(fd, order, bounds, "unit_mean")
    assert torch.equal(unit, ops_eval.pool_templates(fd, order, bounds, "mean", torch.reciprocal(norms)))
    # templates 2 .. 4 first and every other row as one last template: the same rows whatever else the call pools
    sub = np.concatenate([order[bounds[2]:bounds[5]], np.setdiff1d(np.arange(len(order), dtype=np.int32), order[bounds[2]:bounds[5]])]).astype(np.int32)
    sb = np.concatenate([bounds[2:6] - bounds[2], [len(order)]]).astype(np.int32)
    part = ops_eval.pool_templates(fd, sub, sb, "mean")
    assert torch.equal(part[:3], ops_eval.pool_templates(fd, order, bounds, "mean")[2:5])


# ---- segment_reduce2d ----

SEG_LAYOUTS = {
    "mixed": ([300, 1, 64, 2, 65, 1, 2, 65, 64, 1, 64, 65, 2], [65, 300, 1, 2, 64, 1, 300, 64, 65, 2, 1, 30]),
    "window_edges": ([2, 1, 65], [256, 1, 255, 64, 192, 1, 1, 130]),
    "one_entry": ([1], [1]),
    "one_block": ([700], [900]),
}


@pytest.mark.parametrize("layout", sorted(SEG_LAYOUTS))
def test_segment_reduce2d_bitwise(dev, layout):
    """min / max exactly (numpy on the order-preserving integer keys; -0.0 below +0.0) on integer values with -0.0, +inf and duplicates;
    mean bit for bit against the emulation on random values; the matrix read by a pitch ld > cols, the block written into the interior
    of a larger matrix whose other entries stay untouched"""
    from daliid_amd import ops_eval
    rl, cl = SEG_LAYOUTS[layout]
    rb, cb = (np.concatenate([[0], np.cumsum(v)]).astype(np.int32) for v in (rl, cl))
    rows, cols = int(rb[-1]), int(cb[-1])
    rng = np.random.default_rng(rows * 7 + cols)
    xi = rng.integers(-3, 4, (rows, cols)).astype(F32)
    zero = xi == 0
    xi[zero] = np.where(rng.random(int(zero.sum())) < 0.5, F32(-0.0), F32(0.0))
    xi[rng.random((rows, cols)) < 0.01] = np.inf
    xr = rng.standard_normal((rows, cols)).astype(F32)
    for x, modes in ((xi, ("min", "max", "mean")), (xr, ("min", "max", "mean"))):
        wide = torch.full((rows, cols + 3), -5.0, device=dev)
        wide[:, 1:1 + cols] = torch.from_numpy(x).to(dev)
        view = wide[:, 1:1 + cols]                                  # pitch cols + 3, base 4 bytes off
        for mode in modes:
            with np.errstate(invalid="ignore"):
                want = R.segment_mean_f32(x, rb, cb) if mode == "mean" else R.segment_minmax(x, rb, cb, mode)
            got = ops_eval.segment_reduce2d(view, rb, cb, mode)
            assert tuple(got.shape) == (len(rl), len(cl)) and np.array_equal(_bits(got), _bits(want)), mode
            big = torch.full((len(rl) + 5, len(cl) + 4), 7.0, device=dev)
            ops_eval.segment_reduce2d(torch.from_numpy(x).to(dev), torch.from_numpy(rb).to(dev), torch.from_numpy(cb).to(dev), mode,
                                      out=big, out_row0=2, out_col0=3)
            assert np.array_equal(_bits(big[2:2 + len(rl), 3:3 + len(cl)]), _bits(want)), mode
            big[2:2 + len(rl), 3:3 + len(cl)] = 7.0
            assert bool((big == 7.0).all())


# ---- link_templates ----

def _link_case(dev, d=64):
    rng = np.random.default_rng(21)
    ql = [1, 2, 5, 3, 8, 1, 4, 6, 2, 7, 3, 5, 1, 9, 4, 2, 6, 3, 8, 5, 2, 4, 7, 1, 6, 3, 5, 2, 4, 3]
    gl = [4, 1, 7, 3, 12, 2, 5, 9, 1, 6, 3, 8, 2, 10, 4, 7, 1, 5, 11, 3] * 3
    qb, gb = (np.concatenate([[0], np.cumsum(v)]).astype(np.int32) for v in (ql, gl))
    q = (rng.standard_normal((qb[-1], d)) * rng.uniform(0.5, 2, (qb[-1], 1))).astype(F32)
    g = (rng.standard_normal((gb[-1], d)) * rng.uniform(0.5, 2, (gb[-1], 1))).astype(F32)
    return torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), qb, gb


def _round512(nbytes):
    return -(-nbytes // 512) * 512


@pytest.mark.parametrize("linkage", ["min", "mean", "max"])
def test_link_templates_equals_the_reduced_whole_matrix(dev, linkage, monkeypatch):
    """scratch sizes that force 1, 3 and many blocks: the result is bit for bit segment_reduce2d(pairdist(q, g, normalize=True)) on the
    whole (a distance entry does not depend on the block it is computed in), and the call allocates no more than ``scratch_bytes`` on
    top of its result and its (rounded) index tensors"""
    from daliid_amd import ops_eval
    q, g, qb, gb = _link_case(dev)
    nq, ng = q.shape[0], g.shape[0]
    whole = ops_eval.segment_reduce2d(ops_eval.pairdist(q, g, normalize=True), qb, gb, linkage)
    calls = []
    plain = ops_eval.pairdist
    monkeypatch.setattr(ops_eval, "pairdist", lambda *a, **k: (calls.append(tuple(k["out"].shape)), plain(*a, **k))[1])
    three = 4 * ng * (nq // 3 + 9)              # whole gallery width, a third of the query rows plus the longest template
    for scratch_bytes, n_blocks in ((1 << 30, 1), (three, 3), (4 * 9 * 12 * 6, None)):
        del calls[:]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        got = ops_eval.link_templates(q, g, qb, gb, linkage=linkage, scratch_bytes=scratch_bytes)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert torch.equal(got, whole), (scratch_bytes, len(calls))
        assert len(calls) == n_blocks if n_blocks else len(calls) > 20, len(calls)
        assert all(r * c * 4 <= scratch_bytes for r, c in calls)
        assert peak <= min(scratch_bytes, _round512(4 * nq * ng)) + _round512(got.numel() * 4) + 64 * 512, (peak, scratch_bytes)
    with pytest.raises(ValueError, match=str(9 * 12 * 4)):
        ops_eval.link_templates(q, g, qb, gb, linkage=linkage, scratch_bytes=9 * 12 * 4 - 4)
    assert torch.equal(ops_eval.link_templates(q, g, qb, gb, linkage=linkage, scratch_bytes=9 * 12 * 4), whole)


def test_mean_linkage_against_float64(dev):
    """Mean linkage on cosine distances is 1 - (mean of unit q) . (mean of unit g).  Per entry the bound is the project's bf16x3
    ``pairdist``-against-oracle figure at d >= 128 (2e-6, tests/test_gpu_eval.py) plus |a| |b| 2^-23 for the fp32 mean of entries of
    size <= 2.  Largest error observed on an MI355X: 8.2e-7, 0.39 of its entry's bound (docs/experiments.md, template evaluation)."""
    from daliid_amd import ops_eval
    q, g, qb, gb = _link_case(dev, d=256)
    got = ops_eval.link_templates(q, g, qb, gb, linkage="mean").cpu().numpy().astype(np.float64)
    unit = lambda t: (lambda x: x / np.linalg.norm(x, axis=1, keepdims=True))(t.cpu().numpy().astype(np.float64))
    mean = lambda x, b: np.add.reduceat(x, b[:-1], axis=0) / np.diff(b)[:, None]
    ref = 1.0 - mean(unit(q), qb) @ mean(unit(g), gb).T
    err = np.abs(got - ref)
    bound = 2e-6 + np.outer(np.diff(qb), np.diff(gb)) * 2.0 ** -23
    print("mean linkage against float64: largest error %.3g, largest error / bound %.4f" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound), (err / bound).max()


# ---- open_set_search / open_set_metrics ----

def _open_set_case(nq, ng):
    """integer-valued distances (ties are plentiful); subject s has 0, 1 or 3 gallery entries for s % 3 == 0, 1, 2"""
    rng = np.random.default_rng(nq * 10007 + ng)
    g_subj = []
    s = 1
    while len(g_subj) < ng:
        g_subj += [s] * (1 if s % 3 == 1 else 3 if s % 3 == 2 else 0)
        s += 1
    g_subj = rng.permutation(np.array(g_subj[:ng], dtype=np.int32))
    q_subj = rng.integers(0, s + 1, nq).astype(np.int32)
    q_subj[0] = g_subj[0]
    if nq > 1:
        q_subj[1] = 0                                   # subject 0 has no gallery entry
    D = rng.integers(0, 6, (nq, ng)).astype(F32)
    D[D == 0] = np.where(rng.random(int((D == 0).sum())) < 0.5, F32(-0.0), F32(0.0))
    return D, q_subj, g_subj


@pytest.mark.parametrize("ng", [1, 5, 257, 5000])
@pytest.mark.parametrize("nq", [1, 5, 300])
def test_open_set_search_and_metrics_exact(dev, nq, ng):
    from daliid_amd import ops_eval
    D, q_subj, g_subj = _open_set_case(nq, ng)
    want = R.open_set_search(D, q_subj, g_subj)
    if nq > 1:
        assert (want[4] >= 0).any() and (want[4] < 0).any()
    Dd = torch.from_numpy(D).to(dev)
    wide = torch.full((nq, ng + 5), -1.0, device=dev)
    wide[:, 1:1 + ng] = Dd
    for mat in (Dd, wide[:, 1:1 + ng]):                    # 16-byte path with its tail; a pitch > ng with a base 4 bytes off
        got = ops_eval.open_set_search(mat, q_subj, torch.from_numpy(g_subj).to(dev))
        for name, a, b in zip(("mate_dist", "mate_col", "nonmate_dist", "nonmate_col", "rank"), got, want):
            a = a.cpu().numpy()
            assert a.dtype == b.dtype and np.array_equal(a, b), name          # distances compared by value: -0.0 == +0.0
    q_ids, g_ids = np.array(["s%d" % s for s in q_subj]), np.array(["s%d" % s for s in g_subj])
    fpirs, ranks = (1e-1, 1e-2, 1e-3), (1, 20)
    got = ops_eval.open_set_metrics(Dd, q_ids, g_ids, fpirs, ranks)
    assert R.same_summary(got, R.open_set_summary(want[0], want[2], want[4], fpirs, ranks))


# ---- refusals ----

def test_refusals_leave_the_context_usable(dev):
    """every refusal is raised before a launch (or, for index data that lives on the device, skips what is out of range), and a valid
    call right after it gives the right answer"""
    from daliid_amd import _lib, ops_eval
    fvs, order, bounds, w = _pool_case(8, 5)
    fd, wd = torch.from_numpy(fvs).to(dev), torch.from_numpy(w).to(dev)
    good = R.pool_f32(fvs, order, bounds)
    ok = lambda: np.array_equal(_bits(ops_eval.pool_templates(fd, order, bounds)), _bits(good))
    empty = bounds.copy()
    empty[2] = empty[1]
    for args, exc in (((fd, order, empty), ValueError), ((fd, order, bounds[:-1]), ValueError), ((fd, order, bounds + 1), ValueError),
                      ((fd, order[:-1], bounds), ValueError), ((fd, order + 1, bounds), ValueError), ((fd, order, bounds, "median"), ValueError),
                      ((fd, order, bounds, "max", wd), ValueError), ((fd, order, bounds, "magnitude", wd), ValueError),
                      ((fd.double(), order, bounds), _lib.DaliError), ((fd.cpu(), order, bounds), _lib.DaliError)):
        with pytest.raises(exc):
            ops_eval.pool_templates(*args)
        assert ok()
    with pytest.raises(ValueError, match="empty"):
        ops_eval.pool_templates(fd, order, empty)
    # index data on the device is checked by the kernel: nothing outside the rows is read, the call reports it
    bad_order = torch.from_numpy(order).to(dev).clone()
    bad_order[3], bad_order[7] = -1, len(order)
    for o, b, what in ((bad_order, torch.from_numpy(bounds).to(dev), "row number"), (torch.from_numpy(order).to(dev), torch.from_numpy(empty).to(dev), "bounds")):
        with pytest.raises(_lib.DaliError, match=what):
            ops_eval.pool_templates(fd, o, b)
        assert ok()
    # the C entries themselves refuse and name the value
    L, out, status = _lib.lib(), torch.full((5, 8), 7.0, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
    od, bd = torch.from_numpy(order).to(dev), torch.from_numpy(bounds).to(dev)
    n = len(order)
    P = _lib.ptr
    for kw, msg in ((dict(mode=2), "mode=2"), (dict(d=0), "d=0"), (dict(T=n + 1), "n_templates"), (dict(out=_lib.c_void_p(0)), "null"),
                    (dict(mode=1, w=P(wd)), "weights"), (dict(out=P(fd)), "overlaps")):
        rc = L.dali_pool_rows(_lib.ctx(dev), _lib.stream_ptr(), P(fd), n, kw.get("d", 8), P(od), P(bd), kw.get("T", 5), kw.get("w", _lib.c_void_p(0)),
                              kw.get("mode", 0), kw.get("out", P(out)), P(status))
        assert rc != 0 and msg in _lib.last_error(), (kw, _lib.last_error())
    x = torch.from_numpy(np.arange(12, dtype=F32).reshape(3, 4)).to(dev)
    rb, cb = np.array([0, 1, 3], np.int32), np.array([0, 2, 4], np.int32)
    rbd, cbd = torch.from_numpy(rb).to(dev), torch.from_numpy(cb).to(dev)
    seg = lambda **kw: L.dali_segment_reduce2d(_lib.ctx(dev), _lib.stream_ptr(), P(x), 3, 4, kw.get("ld", 4), P(rbd), kw.get("Tr", 2), P(cbd), 2,
                                               kw.get("mode", 0), P(out), 5, 8, kw.get("row0", 0), kw.get("col0", 0), P(status))
    for kw, msg in ((dict(mode=3), "mode=3"), (dict(ld=3), "ld=3"), (dict(Tr=4), "row segments"), (dict(row0=4), "does not lie inside"),
                    (dict(col0=7), "does not lie inside"), (dict(col0=-1), "does not lie inside")):
        assert seg(**kw) != 0 and msg in _lib.last_error(), (kw, _lib.last_error())
    rc = L.dali_open_set_search(_lib.ctx(dev), _lib.stream_ptr(), P(x), 3, 4, 3, P(rbd), P(cbd), P(out), P(od), P(out), P(od), P(od))
    assert rc != 0 and "ld=3" in _lib.last_error()
    rc = L.dali_open_set_search(_lib.ctx(dev), _lib.stream_ptr(), P(x), 0, 4, 4, P(rbd), P(cbd), P(out), P(od), P(out), P(od), P(od))
    assert rc != 0 and "nq=0" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(status.item()) == 0 and torch.equal(od.cpu(), torch.from_numpy(order))
    for args, exc in (((x, rb, cb, "median"), ValueError), ((x, rb[:-1], cb, "min"), ValueError), ((x, rb, np.array([0, 2, 2, 4]), "min"), ValueError),
                      ((x.cpu(), rb, cb, "min"), _lib.DaliError), ((x[0], rb, cb, "min"), ValueError)):
        with pytest.raises(exc):
            ops_eval.segment_reduce2d(*args)
    with pytest.raises(ValueError, match="does not lie inside"):
        ops_eval.segment_reduce2d(x, rb, cb, "min", out=out, out_row0=4)
    with pytest.raises(_lib.DaliError, match="bounds"):
        ops_eval.segment_reduce2d(x, rbd, torch.tensor([0, 5, 4], device=dev, dtype=torch.int32), "min")
    assert ops_eval.segment_reduce2d(x, rb, cb, "max").cpu().tolist() == [[1.0, 3.0], [9.0, 11.0]]
    assert ops_eval.segment_reduce2d(x, rb, cb, "mean").cpu().tolist() == [[0.5, 2.5], [6.5, 8.5]]
    for args in ((x, np.zeros(2, np.int32), np.zeros(4, np.int32)), (x, np.zeros(3, np.float32), np.zeros(4, np.int32)), (x[0], [0], [0, 0, 0, 0])):
        with pytest.raises(ValueError):
            ops_eval.open_set_search(*args)
    got = ops_eval.open_set_search(x, np.array([1, 2, 3], np.int32), np.array([3, 3, 1, 9], np.int32))
    assert [t.cpu().tolist() for t in got] == [[2.0, float("inf"), 8.0], [2, -1, 0], [0.0, 4.0, 10.0], [0, 0, 2], [2, -1, 0]]
    q, g, qb, gb = _link_case(dev)
    for kw, exc in ((dict(linkage="median"), ValueError), (dict(scratch_bytes=16), ValueError), (dict(metric="l1"), ValueError)):
        with pytest.raises(exc):
            ops_eval.link_templates(q, g, qb, gb, **kw)
    with pytest.raises(ValueError):
        ops_eval.link_templates(q, g, qb[:-1], gb)
    assert ok()


# ---- validator: 40 identities x 10 samples in 64 dimensions, 80 queries + 320 gallery rows, 3 cameras ----

class _Model:
    def eval(self):
        return self


def _reid_set(dev, seed=11):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((40, 64))
    x = np.repeat(centres, 10, axis=0) + 0.9 * rng.standard_normal((400, 64))
    x *= rng.uniform(0.5, 2, (400, 1))
    pid = np.repeat(np.arange(40), 10)
    p = rng.permutation(400)
    x, pid = x[p].astype(F32), pid[p]
    pid[:8] = 100 + np.arange(8) // 2                  # four query identities without a gallery entry: non-mated probes
    cam = rng.integers(0, 3, 400)
    rows = np.stack([np.arange(400), pid, cam], axis=1)
    return rows[:80], rows[80:], torch.from_numpy(x[:80]).to(dev), torch.from_numpy(x[80:]).to(dev)


def _validator(name, queries, gallery, qf, gf):
    from daliid_amd import validateModels as V
    v = V.validationManager.getValidator(name)
    v.setParameters(64, 32, False, 0)
    v._features = lambda subset, model: (qf if subset is queries else gf).clone()
    return v


def _gather(fvs, order):
    return fvs.index_select(0, torch.from_numpy(order.astype(np.int64)).to(fvs.device))


def test_validator_templates_are_the_composition_of_the_public_pieces(dev):
    from daliid_amd import ops_eval
    queries, gallery, qf, gf = _reid_set(dev)
    v = _validator("Market", queries, gallery, qf, gf)
    cmc0, map0, d0 = v.validate(queries, gallery, _Model())
    assert torch.equal(d0, v.distance(qf, gf)) and v.template_rows is None
    qo, qb, qfirst = ops_eval.template_index(queries[:, 1])
    go, gb, gfirst = ops_eval.template_index((gallery[:, 1], gallery[:, 2]))
    # pooling: queries by identity (cameras mix), gallery by identity and camera
    for pooling in ("mean", "max", "magnitude", "unit_mean"):
        v.setTemplates(query=1, gallery=(1, 2), pooling=pooling)
        cmc1, map1, d1 = v.validate(queries, gallery, _Model())
        pq, pg = ops_eval.pool_templates(qf, qo, qb, pooling), ops_eval.pool_templates(gf, go, gb, pooling)
        assert tuple(d1.shape) == (len(qfirst), len(gfirst)) and torch.equal(d1, v.distance(pq, pg))
    qr, gr = v.template_rows
    assert np.array_equal(qr[:, :2], queries[qfirst][:, :2]) and np.array_equal(gr, gallery[gfirst])
    # a mixed-camera template is never filtered by camera: its camera id equals no camera, the metrics are those of rank_eval on the template rows
    mixed = np.array([len(set(queries[qo[qb[t]:qb[t + 1]], 2])) > 1 for t in range(len(qfirst))])
    assert mixed.any() and not mixed.all()
    assert not np.isin(qr[mixed, 2], np.concatenate([queries[:, 2], gallery[:, 2]])).any() and np.array_equal(qr[~mixed, 2], queries[qfirst][~mixed, 2])
    want_cmc, want_map = ops_eval.rank_eval(d1, qr[:, 1], gr[:, 1], qr[:, 2], gr[:, 2], max_rank=50)
    assert map1 == want_map and np.array_equal(cmc1, want_cmc)
    idx, dist = v.retrieve(queries, gallery, _Model(), k=7)                  # retrieve searches gallery templates
    tv, ti = ops_eval.topk_rows(d1, 7)
    assert torch.equal(idx, ti) and torch.equal(dist, tv)
    # pooling + query expansion + re-ranking
    v.rerank = True
    v.setQueryExpansion(k=5)
    v.setTemplates(query=1, gallery=(1, 2), pooling="mean")
    _, _, d2 = v.validate(queries, gallery, _Model())
    eq, eg = ops_eval.query_expansion(ops_eval.pool_templates(qf, qo, qb), ops_eval.pool_templates(gf, go, gb), k=5, precision=v.precision)
    assert torch.equal(d2, ops_eval.re_ranking(v.distance(eq, eg), v.distance(eq, eq), v.distance(eg, eg)))
    # linkage; with re-ranking the q-q and g-g blocks use the same linkage; with query expansion it is refused before any feature
    v.setTemplates(query=1, gallery=(1, 2), linkage="min")
    with pytest.raises(ValueError, match="query expansion"):
        v.validate(queries, gallery, _Model())
    v.setQueryExpansion(None)
    sq, sg = _gather(qf, qo), _gather(gf, go)
    link = lambda a, b, ab, bb, how: ops_eval.link_templates(a, b, ab, bb, linkage=how, precision=v.precision)
    _, _, d3 = v.validate(queries, gallery, _Model())
    assert torch.equal(d3, ops_eval.re_ranking(link(sq, sg, qb, gb, "min"), link(sq, sq, qb, qb, "min"), link(sg, sg, gb, gb, "min")))
    v.rerank = False
    for how in ("min", "mean", "max"):
        v.setTemplates(query=1, gallery=(1, 2), linkage=how)
        _, _, d4 = v.validate(queries, gallery, _Model())
        assert torch.equal(d4, link(sq, sg, qb, gb, how))
    v.setTemplates(query=lambda subset: subset[:, 1], linkage="min")         # a callable; the gallery side stays one row per template
    _, _, d5 = v.validate(queries, gallery, _Model())
    assert torch.equal(d5, link(sq, gf, qb, np.arange(321), "min")) and v.template_rows[1] is gallery
    with pytest.raises(NotImplementedError, match="linkage"):
        v.retrieve(queries, gallery, _Model())
    with pytest.raises(NotImplementedError, match="template"):
        v.validate_sharded(queries, gallery, _Model())
    # off again: the plain results exactly
    v.setTemplates()
    cmc6, map6, d6 = v.validate(queries, gallery, _Model())
    assert torch.equal(d6, d0) and map6 == map0 and np.array_equal(cmc6, cmc0) and v.template_rows is None


@pytest.mark.parametrize("name", ["Market", "BRIAR"])
def test_report_open_set_adds_lines_and_leaves_the_rest(dev, name, capsys):
    from daliid_amd import ops_eval
    queries, gallery, qf, gf = _reid_set(dev)
    v = _validator(name, queries, gallery, qf, gf)
    cmc0, map0, d0 = v.validate(queries, gallery, _Model())
    plain = capsys.readouterr().out
    assert "FNIR" not in plain and not hasattr(v, "open_set")
    v.report_open_set = True
    cmc1, map1, d1 = v.validate(queries, gallery, _Model())
    out = capsys.readouterr().out
    assert out.startswith(plain) and torch.equal(d1, d0) and map1 == map0 and np.array_equal(np.asarray(cmc1), np.asarray(cmc0))
    extra = out[len(plain):].splitlines()
    assert len(extra) == 6 and all(ln.startswith("FNIR@FPIR=") for ln in extra) and extra[0].startswith("FNIR@FPIR=0.1 Rank-1  :")
    want = ops_eval.open_set_metrics(d0, queries[:, 1], gallery[:, 1])
    assert R.same_summary(v.open_set, want) and want["n_nonmated"] == 8 and want["n_mated"] == 72
    v.setTemplates(query=1, gallery=1)                                       # on templates: one probe per identity
    _, _, d2 = v.validate(queries, gallery, _Model())
    capsys.readouterr()
    qr, gr = v.template_rows
    assert R.same_summary(v.open_set, ops_eval.open_set_metrics(d2, qr[:, 1], gr[:, 1])) and v.open_set["n_nonmated"] == 4

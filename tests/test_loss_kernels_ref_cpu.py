"""CPU self-tests of tests/loss_kernels_ref.py, the fp64 restatements the GPU kernel tests compare with:
  * the restatements reproduce the reference's own outputs (tests/golden/losses.npz, triplet.npz) at the tolerances tests/test_oracle_losses.py
    uses for the same goldens;
  * every error bound holds, with room, for an fp32 numpy emulation of the same formula (not the kernel: numpy's own exp / log, its own
    summation order) on every input family of the GPU tests, and is not so wide that it would let a wrong formula through: deliberately wrong
    variants of the restatements leave the bounds, or select differently, on those same inputs;
  * the tie inputs really tie at the selection boundary.
"""
import math

import numpy as np
import pytest
import torch

import loss_kernels_ref as R
from conftest import load_golden, loss_case
from oracle import losses as O

KMAX = 16            # any value >= the proxies per identity gives the same rows; the GPU tests ask the library (dali_proxy_kmax)
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------- pinned to the goldens
def _codes(a):
    return np.rint(np.asarray(a, np.float64)).astype(np.int32)


def _sim(a, b):
    return (np.asarray(a, np.float64) @ np.asarray(b, np.float64).T).astype(F32)


@pytest.mark.parametrize("name", [str(c) for c in load_golden("losses.npz")["cases"]])
def test_restatements_match_reference_goldens(name, golden_losses):
    c = loss_case(golden_losses, name)
    epoch, n_epochs, tau = c["hyper"]
    w = O.distortion_weight_table(int(epoch), int(n_epochs)).numpy()[c["distortion"]]
    y = _codes(c["labels"])
    # center head
    cl = _codes(c["centers_labels"])
    S = _sim(c["fv"], c["centers"])
    r = R.center_rows(S, y, cl, w, tau)
    gc = R.center_bwd(S, y, cl, w, tau, r["sums"][1]) @ c["centers"].astype(np.float64)
    assert np.isclose(r["sums"][0] / r["sums"][1], c["center_loss"], rtol=2e-6, atol=1e-6)
    has_one = r["cnt"] == 1
    pred = np.asarray(c["centers_labels"])[r["argmax"]]
    assert np.isclose(O.acc_balanced(pred[has_one], c["labels"][has_one]), c["center_acc"], atol=1e-9)
    assert np.isclose(r["maxp"].mean(), c["center_avg_max_prob"], rtol=1e-5)
    # proxy head
    pl = _codes(c["proxies_labels"])
    Sp = _sim(c["fv"], c["proxies"])
    q = R.proxy_rows(Sp, y, pl, w, tau, KMAX)
    assert q["status"] == 0
    gp = R.proxy_bwd(q["sel_idx"], q["sel_coef"], c["proxies"], q["sums"][1])
    assert np.isclose(q["sums"][0] / q["sums"][1], c["proxy_loss"], rtol=2e-6, atol=1e-6)
    if "center_grad" in c:
        np.testing.assert_allclose(gc, c["center_grad"], rtol=1e-4, atol=2e-6)
        np.testing.assert_allclose(gp, c["proxy_grad"], rtol=1e-4, atol=2e-6)
    else:
        np.testing.assert_allclose(gc[:8], c["center_grad_head"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(gp[:8], c["proxy_grad_head"], rtol=1e-4, atol=1e-6)
        assert np.isclose(np.abs(gc).sum(), c["center_grad_abs_sum"], rtol=1e-5)
        assert np.isclose(np.abs(gp).sum(), c["proxy_grad_abs_sum"], rtol=1e-5)


@pytest.mark.parametrize("name", [str(c) for c in load_golden("triplet.npz")["cases"]])
def test_triplet_restatement_matches_reference_golden(name):
    z = load_golden("triplet.npz")
    epoch, n_epochs, tau = z[name + "/hyper"]
    fv = z[name + "/fv"]
    w = O.triplet_weight_table(int(epoch), int(n_epochs)).numpy()[z[name + "/distortion"]]
    r = R.triplet_rows(_sim(fv, fv), _codes(z[name + "/labels"]), w, tau)
    assert r["status"] == 0
    g = R.triplet_bwd(r["sel_idx"], r["sel_coef"], r["sums"][1]) @ fv.astype(np.float64)
    g_ref = z[name + "/grad"]
    assert np.isclose(r["sums"][0] / r["sums"][1], float(z[name + "/loss"]), rtol=3e-6, atol=1e-6)
    np.testing.assert_allclose(g, g_ref, rtol=1e-4, atol=2e-6 * float(np.abs(g_ref).max()) + 1e-9)


def test_adam_restatement_matches_torch():
    """torch.optim.Adam in double over three steps with a change of learning rate, weight decay folded into the gradient.  torch is given
    the fp32 values of the hyper-parameters, which is what crosses the C ABI (fl32(0.999) moves 1 - beta2 by 1.3e-5 relative)."""
    f = R.f32
    g = torch.Generator().manual_seed(0)
    p = torch.randn(4096, generator=g).double().mul_(0.02).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=f(3.5e-4), betas=(f(0.9), f(0.999)), eps=f(1e-8), weight_decay=f(5e-4))
    rp, rm, rv = p.detach().numpy().copy(), np.zeros(4096), np.zeros(4096)
    for step in (1, 2, 3):
        grad = torch.randn(4096, generator=g).double()
        lr = 3.5e-4 / step
        opt.param_groups[0]["lr"] = f(lr)
        p.grad = grad.clone()
        opt.step()
        rp, rm, rv = R.adam_step(rp, grad.numpy() * 8.0, rm, rv, lr, 0.9, 0.999, 1e-8, 5e-4, step, grad_scale=0.125)
        st = opt.state[p]
        np.testing.assert_allclose(rp, p.detach().numpy(), rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(rm, st["exp_avg"].numpy(), rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(rv, st["exp_avg_sq"].numpy(), rtol=1e-10, atol=1e-18)


# ------------------------------------------------------------------------------------------------------------------------------- fp32 emulations
def _exp32(x):
    return np.exp(x.astype(F32)).astype(F32)


def _lane_sum32(x):
    """row sums in fp32 the way a 64-lane wave would form them: lane l adds columns l, l + 64, .. in order, then a butterfly over the lanes"""
    nb, n = x.shape
    pad = np.zeros((nb, -n % 64), F32)
    lanes = np.concatenate([x.astype(F32), pad], axis=1).reshape(nb, -1, 64)
    acc = np.zeros((nb, 64), F32)
    for t in range(lanes.shape[1]):
        acc = (acc + lanes[:, t]).astype(F32)
    width = 64
    while width > 1:
        width //= 2
        acc = (acc[:, :width] + acc[:, width:2 * width]).astype(F32)
    return acc[:, 0]


def _emu_center(S, y, cl, w, tau, denom, gscale):
    it = F32(1.0) / F32(tau)
    v = (S * it).astype(F32)
    m = v.max(axis=1)
    e = _exp32(v - m[:, None])
    se = _lane_sum32(e)
    mask = cl[None, :] == y[:, None]
    cnt = mask.sum(axis=1).astype(F32)
    pos = _lane_sum32(np.where(mask, v, F32(0)))
    logz = (m + np.log(se).astype(F32)).astype(F32)
    num = (w * ((cnt * logz).astype(F32) - pos).astype(F32)).astype(F32)
    coef = (((F32(gscale) * w).astype(F32) * it).astype(F32) / F32(denom)).astype(F32)
    inv_se = (F32(1.0) / se).astype(F32)
    p = (e * inv_se[:, None]).astype(F32)
    dS = (coef[:, None] * ((cnt[:, None] * p).astype(F32) - mask.astype(F32)).astype(F32)).astype(F32)
    return num, inv_se, dS


@pytest.fixture(scope="module")
def center_inputs():
    return R.center_cases()


def test_case_names_are_the_listed_ones(center_inputs, proxy_refs):
    """the GPU tests parametrise over these lists without building the inputs at import"""
    assert tuple(sorted(center_inputs)) == R.CENTER_CASE_NAMES
    assert tuple(sorted(proxy_refs)) == R.PROXY_CASE_NAMES


def test_center_bounds_hold_for_an_fp32_emulation(center_inputs):
    """Largest error / bound seen over all center inputs: numerator 0.33, max probability 0.30, dS 0.49 (asserted below 0.75: the bounds are
    worst-case sums of moduli, a real evaluation stays well inside; the wrong variants further down show they are not too wide)."""
    worst = np.zeros(3)
    for name, (S, y, cl, w, tau, first) in center_inputs.items():
        NC = S.shape[1]
        r = R.center_rows(S, y, cl, w, tau)
        denom = F32(2.75) * F32(r["sums"][1])
        num, maxp, dS = _emu_center(S, y, cl, w, tau, denom, 0.25)
        ratios = (np.abs(num - r["num"]) / np.maximum(R.center_num_tol(r, w, NC), 1e-300),
                  np.abs(maxp - r["maxp"]) / R.center_maxp_tol(r, NC),
                  np.abs(dS - R.center_bwd(S, y, cl, w, tau, denom, 0.25)) / R.center_bwd_tol(S, y, cl, w, tau, denom, 0.25))
        worst = np.maximum(worst, [float(x.max()) for x in ratios])
        assert np.all(num[r["cnt"] == 0] == 0)
    print("center: largest error / bound", worst)
    assert np.all(worst < 0.75) and np.all(worst > 0.02), worst


def _emu_proxy_row(s, pos, neg, w, it):
    """fp32, terms added in reverse order of the restatement's"""
    vp, vn = (s[pos] * it).astype(F32), (s[neg] * it).astype(F32)
    allv = np.concatenate([vn[::-1], vp[::-1]])
    m = allv.max()
    D = F32(0)
    for x in allv:
        D = F32(D + F32(np.exp(F32(x - m))))
    logD = F32(m + F32(np.log(D)))
    ps = F32(0)
    for x in vp[::-1]:
        ps = F32(ps + x)
    n = F32(len(pos))
    row = F32(-w * F32(F32(ps / n) - logD))
    wt = F32(w * it)
    cp = (wt * (_exp32(vp - logD) - F32(F32(1) / n)).astype(F32)).astype(F32)
    cn = (wt * _exp32(vn - logD)).astype(F32)
    return row, cp, cn


@pytest.fixture(scope="module")
def proxy_refs():
    return {name: (c, R.proxy_rows(*c, KMAX)) for name, c in R.proxy_cases(KMAX).items()}


def test_proxy_bounds_hold_for_an_fp32_emulation(proxy_refs):
    """Largest error / bound over all proxy inputs: row 0.50, coefficients 0.62."""
    worst = np.zeros(2)
    for name, ((S, y, pl, w, tau), r) in proxy_refs.items():
        it = F32(1.0) / F32(tau)
        for i in np.flatnonzero(r["specified"] & (r["den"] > 0)):
            pos, neg = r["sel_idx"][i, :KMAX], r["sel_idx"][i, KMAX:]
            pos, neg = pos[pos >= 0], neg[neg >= 0]
            row, cp, cn = _emu_proxy_row(S[i], pos, neg, w[i], it)
            n, k = len(pos), len(neg)
            worst[0] = max(worst[0], abs(row - r["num"][i]) / r["num_tol"][i])
            err = np.abs(np.concatenate([cp - r["sel_coef"][i, :n], cn - r["sel_coef"][i, KMAX:KMAX + k]]))
            worst[1] = max(worst[1], float((err / np.concatenate([r["coef_tol"][i, :n], r["coef_tol"][i, KMAX:KMAX + k]])).max()))
    print("proxy: largest error / bound", worst)
    assert np.all(worst < 0.75) and np.all(worst > 0.02), worst


def test_triplet_bounds_hold_for_an_fp32_emulation():
    """Largest error / bound: row 0.45, coefficient 0.17."""
    worst = np.zeros(2)
    for nb in (6, 61, 64, 256):
        for family, tau in (("ties", 0.05), ("random", 0.1)):
            S, y, w = R.triplet_inputs(nb, family, 500 + nb)
            r = R.triplet_rows(S, y, w, tau)
            it = F32(1.0) / F32(tau)
            i = np.arange(nb)
            x = ((S[i, r["sel_idx"][:, 1]] - S[i, r["sel_idx"][:, 0]]).astype(F32) * it).astype(F32)
            sp = (np.maximum(x, F32(0)) + np.log1p(_exp32(-np.abs(x))).astype(F32)).astype(F32)
            sg = (F32(1) / (F32(1) + _exp32(-x)).astype(F32)).astype(F32)
            worst[0] = max(worst[0], float((np.abs((w * sp).astype(F32) - r["num"]) / r["num_tol"]).max()))
            worst[1] = max(worst[1], float((np.abs(((w * sg).astype(F32) * it).astype(F32) - r["sel_coef"]) / r["coef_tol"]).max()))
    print("triplet: largest error / bound", worst)
    assert np.all(worst < 0.75) and np.all(worst > 0.02), worst


@pytest.mark.parametrize("D", R.PROXY_BWD_DIMS)
def test_proxy_backward_bound_holds_for_an_fp32_emulation(D):
    """On the GPU test's own random inputs, slots added in reverse order.  Largest error / bound: 0.13 when the result is written (a
    32-term worst-case bound against a random-sign sum), 0.92 when it is added to the buffer: there the last rounding, u |result|, is most of
    the bound wherever the buffer's value dwarfs the gradient and is nearly attained over 10^5 elements, so only < 1 is asserted."""
    sel_idx, sel_coef, P, denom, gscale, base = R.proxy_bwd_random_inputs(D, KMAX)
    acc = np.zeros(base.shape, F32)
    for a in range(2 * KMAX - 1, -1, -1):
        cf = np.where(sel_idx[:, a] >= 0, sel_coef[:, a], F32(0))
        acc = (acc + (cf[:, None] * P[np.maximum(sel_idx[:, a], 0)]).astype(F32)).astype(F32)
    res = (acc * (F32(gscale) / denom)).astype(F32)
    for accumulate, got in ((False, res), (True, (base + res).astype(F32))):
        ref = R.proxy_bwd(sel_idx, sel_coef, P, denom, gscale, accumulate, base)
        ratio = float((np.abs(got - ref) / R.proxy_bwd_tol(sel_idx, sel_coef, P, denom, gscale, accumulate, base)).max())
        print("proxy_bwd D=%d accumulate=%d: largest error / bound %.3f" % (D, accumulate, ratio))
        assert 0.02 < ratio < (1.0 if accumulate else 0.75)


def test_adam_moment_bounds_hold_for_an_fp32_emulation():
    """Largest error / bound: exp_avg 0.86, exp_avg_sq 0.97 (element-wise formulas of three to five operations, each rounding in the bound really occurs:
    over 10^5 elements the bound is nearly attained, so only < 1 is asserted)."""
    rng = np.random.default_rng(6)
    n = 1 << 16
    worst = np.zeros(2)
    for wd, gs in ((0.0, 1.0), (5e-4, 0.125)):
        p = (rng.standard_normal(n) * 0.02).astype(F32)
        g = (rng.standard_normal(n) * 1e-2 / gs).astype(F32)
        m = (rng.standard_normal(n) * 1e-3).astype(F32)
        v = np.square(rng.standard_normal(n) * 1e-2).astype(F32)
        b1, b2 = F32(0.9), F32(0.999)
        gg = ((g * F32(gs)).astype(F32) + (F32(wd) * p).astype(F32)).astype(F32)
        m1 = ((b1 * m).astype(F32) + ((F32(1) - b1) * gg).astype(F32)).astype(F32)
        v1 = ((b2 * v).astype(F32) + (((F32(1) - b2) * gg).astype(F32) * gg).astype(F32)).astype(F32)
        _, rm, rv = R.adam_step(p, g, m, v, 3.5e-4, 0.9, 0.999, 1e-8, wd, 2, gs)
        tm, tv = R.adam_moment_tols(p, g, m, v, 0.9, 0.999, wd, gs)
        worst = np.maximum(worst, [float((np.abs(m1 - rm) / tm).max()), float((np.abs(v1 - rv) / tv).max())])
    print("adam: largest error / bound", worst)
    assert np.all(worst < 1.0) and np.all(worst > 0.02), worst


# ------------------------------------------------------------------------------------------------------------------------------------ sensitivity
def _selection_differs(c, r, wrong):
    q = R.proxy_rows(*c, KMAX, _wrong=wrong)
    return not np.array_equal(q["sel_idx"], r["sel_idx"])


def test_wrong_tie_break_selects_differently(proxy_refs):
    names = [n for n in proxy_refs if n.endswith("_ties") or n.startswith("kmax")]
    assert len(names) >= 12
    for name in names:
        assert _selection_differs(*proxy_refs[name], "tie_desc"), name


def test_tie_inputs_tie_inside_one_thread_of_the_register_path(proxy_refs):
    """The variant above reverses ties over the whole row.  A kernel can also get them wrong only among the entries one thread holds (columns
    equal mod 256): that shows only where a selected negative has an equal one a multiple of 256 columns behind it, which plant_ties puts in
    every row long enough.  Asked for in at least half of the rows of every tie case of more than 1024 proxies that is held in registers."""
    names = [n for n in proxy_refs if (n.endswith("_ties") or n.startswith("kmax")) and 1024 < proxy_refs[n][0][0].shape[1] <= 4096]
    assert {"np3755_ties", "np2253_ties", "np4096_ties", "nb261_ties"} <= set(names)
    for name in names:
        (S, y, pl, w, tau), r = proxy_refs[name]
        rows = R.same_thread_tie_rows(S, y, pl, r["sel_idx"], KMAX)
        print(name, "rows with a tie inside one thread:", rows, "of", S.shape[0])
        assert rows >= (r["den"] > 0).sum() / 2, name


def test_ignoring_the_last_slot_selects_differently(proxy_refs):
    # (NP = 4097 takes the re-reading path, which has no slots, and its 4097th entry is by construction never selected)
    names = [n for n in proxy_refs if n.startswith(("np", "nb261", "kmax", "tau")) and not n.startswith("np4097")]
    assert len(names) >= 18
    for name in names:
        assert _selection_differs(*proxy_refs[name], "ignore_last_slot"), name


def test_k_equal_n_selects_differently(proxy_refs):
    assert _selection_differs(*proxy_refs["tiny_np5"], "k_n")
    assert _selection_differs(*proxy_refs["tiny_all_positive"], "k_n")


def test_cnt_clamped_to_one_leaves_the_bounds(center_inputs):
    names = [n for n in center_inputs if "_c2_" in n or "_c3_" in n]
    assert len(names) >= 12
    for name in names:
        S, y, cl, w, tau, _ = center_inputs[name]
        r = R.center_rows(S, y, cl, w, tau)
        bad = R.center_rows(S, y, cl, w, tau, _wrong="cnt_min1")
        assert np.any(np.abs(bad["num"] - r["num"]) > R.center_num_tol(r, w, S.shape[1])), name
        d = r["sums"][1]
        assert np.any(np.abs(R.center_bwd(S, y, cl, w, tau, d, _wrong="cnt_min1") - R.center_bwd(S, y, cl, w, tau, d))
                      > R.center_bwd_tol(S, y, cl, w, tau, d)), name


def test_last_index_argmax_differs(center_inputs):
    names = [n for n in center_inputs if "_tie_" in n or "_ties_" in n]
    assert len(names) >= 12
    for name in names:
        S, y, cl, w, tau, _ = center_inputs[name]
        assert not np.array_equal(R.center_rows(S, y, cl, w, tau, _wrong="argmax_last")["argmax"], R.center_rows(S, y, cl, w, tau)["argmax"]), name


def test_local_denominator_leaves_the_bound(center_inputs):
    for name, (S, y, cl, w, tau, _) in center_inputs.items():
        r = R.center_rows(S, y, cl, w, tau)
        denom = F32(2.75) * F32(r["sums"][1])
        good = R.center_bwd(S, y, cl, w, tau, denom, 0.25)
        bad = R.center_bwd(S, y, cl, w, tau, denom, 0.25, _wrong="denom_local")
        assert np.any(np.abs(bad - good) > R.center_bwd_tol(S, y, cl, w, tau, denom, 0.25)), name


# -------------------------------------------------------------------------------------------------------------------------- conditions on inputs
def test_tie_inputs_tie_at_the_selection_boundary(proxy_refs):
    names = [n for n in proxy_refs if n.endswith("_ties") or n.startswith("kmax")]
    for name in names:
        (S, y, pl, w, tau), r = proxy_refs[name]
        assert R.boundary_tie_fraction(S, y, pl, r["sel_idx"], KMAX) >= 0.5, name
    # and a positive equal in value to a selected negative occurs
    (S, y, pl, w, tau), r = proxy_refs["np3755_ties"]
    hits = 0
    for i in range(S.shape[0]):
        pos, neg = r["sel_idx"][i, :KMAX], r["sel_idx"][i, KMAX:]
        hits += bool(np.intersect1d(S[i, pos[pos >= 0]], S[i, neg[neg >= 0]]).size)
    assert hits >= 16


def test_center_inputs_allow_an_exact_argmax_comparison(center_inputs):
    """two distinct fp32 values can round to one product with 1/tau; in these inputs no row's two largest entries are that close"""
    for name, (S, y, cl, w, tau, first) in center_inputs.items():
        assert R.top_two_separated(S).all(), name
        if first is not None:
            assert np.array_equal(R.center_rows(S, y, cl, w, tau)["argmax"], first), name


def test_triplet_tie_inputs_tie_both_selections():
    """The tie family must tie the hardest positive and the hardest negative, each between lanes of the wave and, where the batch is longer
    than a wave, inside one lane (columns 64 apart), so that a tie broken the wrong way at either place selects differently."""
    for nb, least in ((6, 2), (61, 16), (64, 16), (256, 64)):
        S, y, w = R.triplet_inputs(nb, "ties", 500 + nb)
        r = R.triplet_rows(S, y, w, 0.05)
        assert r["sel_idx"][0, 0] == 0 and (y == y[0]).sum() == 1          # the lonely row stays
        t = R.triplet_tie_rows(S, y, r["sel_idx"])
        print("nb=%d" % nb, t)
        assert t["pos_lanes"] >= least and t["neg_lanes"] >= least, (nb, t)
        if nb == 256:
            assert t["pos_samelane"] >= 16 and t["neg_samelane"] >= 64, t


def test_proxy_cases_cover_both_paths_and_every_register_slot(proxy_refs):
    """the register path holds entry j in slot j // 256: rows of 3755 and 2253 proxies have 15 and 9 slots live, the last one ragged"""
    shapes = {c[0].shape[1] for c, _ in proxy_refs.values()}
    assert {5120, 4097, 4096, 3755, 2253, 257, 256, 255, 5, 4, 1} <= shapes
    for name in ("np3755_ties", "np2253_random", "np4096_ties"):
        (S, y, pl, w, tau), r = proxy_refs[name]
        neg = r["sel_idx"][:, KMAX:]
        slots = np.unique(neg[neg >= 0] // 256)
        assert len(slots) == math.ceil(S.shape[1] / 256), name

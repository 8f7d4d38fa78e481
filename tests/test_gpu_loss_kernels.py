"""GPU: the kernels that turn Stage-3 activations into the loss and its first gradient, against the float64 restatements of
tests/losses_ref.py at their edges: sw_rpn_loss (the second grid-stride pass where the anchor index wraps, NULL gradient buffers, no
foreground, everything ignored, logits beyond expf's range, non-unit weights, exactly zero residuals), sw_focal_loss (column views of
pitched buffers as the hot path passes them, gamma 0 / 1 / 1.5 / 2, C around the 64 lanes, N around the 4-row workgroup and the
1024-thread reduction, targets outside [0, C)), sw_det_loss_per_image (more than 64 images, the 4096-anchor chunk, 81 logits, counts
at the 64-row column, max_rows 100 and 0), sw_wsddn_scores_bwd (K at the 64 KiB and the 160 KiB LDS edges, three pitches, the
refusals) and sw_threshold_select (the 1024-thread pass, ties, NaN and infinite scores, an empty label set).

Every output buffer the test owns starts as a NaN with a payload no kernel writes (integers: -123456789), with guard rows and guard
columns: what the contract says is written must be finite (or the specified NaN) and within the bar of losses_ref (taken from the
float32 error of the reference formula, never from the kernel) or bit-equal, everything else must still hold the sentinel.  No element
is masked and no case skipped; every kernel is launched twice and the two results compared bit for bit.  The inputs' distance from
the kink of the L1 loss and the ties of the selection cases are asserted by tests/test_losses_ref_cpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import semisup_oracle as SO  # noqa: E402  (checker only)
import losses_ref as L  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


_F32_SENTINEL, _I32_SENTINEL, _KERNEL_NAN = 0x7FA5A5A5, -123456789, 0x7FC00000


def _sent(*shape, dtype=torch.float32):
    if dtype == torch.float32:
        return torch.full(shape, _F32_SENTINEL, device="cuda", dtype=torch.int32).view(torch.float32)
    return torch.full(shape, _I32_SENTINEL, device="cuda", dtype=torch.int32)


def _untouched(t):
    """bool tensor: the element still holds the sentinel bits"""
    if t.dtype == torch.float32:
        return t.view(torch.int32) == _F32_SENTINEL
    return t == _I32_SENTINEL


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _close(kind, regime, got, ref, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: {kind} holds non-finite values"
    e, b = L.rel_err(got, ref), L.bar(kind, regime)
    print(f"{what} {kind}[{regime}]: err {e:.3g} of max|ref|, bar {b:.3g}")
    assert e <= b, f"{what}: {kind} off by {e:.3g} of max|ref| (bar {b:.3g})"


# ------------------------------------------------------------------------------------------------ sw_rpn_loss
_RPN_WS = 2 * 256                    # sw_rpn_loss_workspace_floats(): one partial pair per workgroup of the capped launch


def _run_rpn(ops, dev, n):
    """the C entry on buffers this test owns: -> losses (4,), dlogits (n + 3,), ddeltas (n + 3, 4), workspace (2 * 256 + 64,)"""
    from sos_wsod_amd._lib import check, lib
    assert int(lib.sw_rpn_loss_workspace_floats()) == _RPN_WS
    losses, dl, dd, ws = _sent(4), _sent(n + 3), _sent(n + 3, 4), _sent(_RPN_WS + 64)
    lg, de, lab, an, ma, w, inv = dev
    check(lib.sw_rpn_loss(n, an.shape[0], ops._p(lg), ops._p(de), ops._p(lab), ops._p(an), ops._p(ma), ops._floats(w, 4), float(inv),
                          ops._p(losses), ops._p(dl), ops._p(dd), ops._p(ws), ops._stream()), "sw_rpn_loss")
    torch.cuda.synchronize()
    return losses, dl, dd, ws


@pytest.mark.parametrize("c", L.RPN_CASES, ids=[c["id"] for c in L.RPN_CASES])
def test_rpn_loss_against_float64(ops, c):
    i = L.rpn_inputs(c)
    n, what, reg = c["N"] * c["A"], c["id"], c["w"]
    ref = L.rpn_loss_ref(i["logits"], i["deltas"], i["labels"], i["anchors"], i["matched"], i["weights"], i["inv_norm"])
    dev = (_cu(i["logits"]), _cu(i["deltas"]), _cu(i["labels"]), _cu(i["anchors"]), _cu(i["matched"]), i["weights"], i["inv_norm"])
    losses, dl, dd, ws = _run_rpn(ops, dev, n)
    _close("rpn.loss_cls", reg, losses[0:1], np.array([ref["loss_cls"]]), what)
    _close("rpn.loss_loc", reg, losses[1:2], np.array([ref["loss_loc"]]), what)
    _close("rpn.dlogits", reg, dl[:n], ref["dlogits"], what)
    # ddeltas: sign(residual) * float32(inv_norm) to the bit; +0.0 for an anchor that is no foreground and for the exact-zero group
    sign = np.sign(ref["ddeltas"]).astype(np.float32)
    want_dd = np.where(sign == 0, np.float32(0.0), sign * np.float32(i["inv_norm"])).astype(np.float32)
    got_dd = _bits(dd[:n])
    assert np.array_equal(got_dd, want_dd.view(np.int32)), f"{what}: ddeltas differ at rows {np.unique(np.nonzero(got_dd != want_dd.view(np.int32))[0])[:8]}"
    assert not got_dd[i["labels"] != 1].any() and not got_dd[i["zero"]].any()
    assert not _bits(dl[:n])[i["labels"] < 0].any(), "dlogits of an ignored anchor must be +0.0"
    if c["labels"] == "ignore":
        assert float(losses[0]) == 0.0 and float(losses[1]) == 0.0
    if c["labels"] in ("ignore", "nofg"):
        assert float(losses[1]) == 0.0 and not got_dd.any()
    assert bool(_untouched(losses[2:]).all()), "losses2 beyond its two floats was written"
    assert bool(_untouched(dl[n:]).all() and _untouched(dd[n:]).all()), "gradient rows beyond n were written"
    assert bool(_untouched(ws[_RPN_WS:]).all()), "the workspace beyond 2 * 256 floats was written"
    again = _run_rpn(ops, dev, n)
    assert all(_same_bits(a, b) for a, b in zip((losses, dl, dd), again[:3])), "two launches differ"
    # the optional buffers (ops.rpn_loss): the losses and the buffer that was given keep their bits
    lg, de, lab, an, ma, w, inv = dev
    for with_dl, with_dd in ((False, True), (True, False), (False, False)):
        l2, dl2, dd2 = _sent(4), _sent(n + 3) if with_dl else None, _sent(n + 3, 4) if with_dd else None
        ops.rpn_loss(lg, de, lab, an, ma, w, inv, l2[:2], None if dl2 is None else dl2[:n], None if dd2 is None else dd2[:n])
        torch.cuda.synchronize()
        assert _same_bits(l2, losses), (what, with_dl, with_dd)
        assert dl2 is None or _same_bits(dl2, dl)
        assert dd2 is None or _same_bits(dd2, dd)


# ------------------------------------------------------------------------------------------------ sw_focal_loss
def _run_focal(ops, x, t_d, gamma, with_grad=True):
    """ops.focal_loss on column views of the hot path's rows [cls (C) | box (4 (C - 1)) | pad]: the logits' other columns hold NaN (never
    read), the gradient buffer's hold the sentinel.  -> loss (3,), dlogits (N + 2, ld_d) or None"""
    N, C = x.shape
    ld, ld_d = L.focal_layout(C)
    lg = torch.full((N, ld), float("nan"), device="cuda")
    lg[:, :C] = _cu(x)
    loss, dl = _sent(3), _sent(N + 2, ld_d) if with_grad else None
    ops.focal_loss(lg[:, :C], t_d, gamma, loss[:1], dl[:N, :C] if with_grad else None)
    torch.cuda.synchronize()
    return loss, dl


@pytest.mark.parametrize("c", L.FOCAL_CASES, ids=[c["id"] for c in L.FOCAL_CASES])
def test_focal_loss_against_float64(ops, c):
    """Regime "shift" (logits of N(0, 3^2) + 3e4) is what the exact per-row offset of focal_loss_kernel is for: with the cross-entropy
    formed as m + log(sum exp(x - m)) - x[t] at 3e4 (2e-3 of absolute precision) these seven cases measured, as a share of max|ref|,
    loss 7.6e-5 (N5-C64-g1.5) and 7.2e-5 (N7-C65-g2), dlogits 8.4e-4 (N1025-C81-g1.5), 6.8e-4 (N37-C129-g1), 4.6e-4 / 4.2e-4
    (N9-C1231, g1.5 / g0) and 7.9e-5 (N1-C2-g1.5) against the bar of 2e-5."""
    N, C, what, reg = c["N"], c["C"], c["id"], L.focal_tol_regime(c)
    x, t = L.focal_inputs(c)
    l64, g64 = L.focal_ref(x, t, c["gamma"])
    t_d = _cu(t)
    loss, dl = _run_focal(ops, x, t_d, c["gamma"])
    _close("focal.loss", reg, loss[:1], np.array([l64]), what)
    _close("focal.dlogits", reg, dl[:N, :C], g64, what)
    assert bool(_untouched(dl[:N, C:]).all()), "gradient columns beyond C were written"
    assert bool(_untouched(dl[N:]).all() and _untouched(loss[1:]).all()), "gradient rows beyond N / the loss's neighbours were written"
    loss2, dl2 = _run_focal(ops, x, t_d, c["gamma"])
    assert _same_bits(loss2, loss) and _same_bits(dl2, dl), "two launches differ"
    loss3, _ = _run_focal(ops, x, t_d, c["gamma"], with_grad=False)
    assert _same_bits(loss3, loss), "the loss without a gradient buffer differs"


@pytest.mark.parametrize("cid", ["N7-C65-g0-sd3", "N1025-C81-g0-sd40", "N37-C129-g1.5-sd3"])
def test_focal_loss_target_outside_the_classes_gives_nan_and_touches_nothing_else(ops, cid):
    """targets -1, C and 2^31 - 1 (heads.hip: neither a read out of bounds nor a plausible number): the loss is NaN, those rows'
    dlogits[:C] are the kernel's NaN, every other row's gradient is still within the bar"""
    c = next(c for c in L.FOCAL_CASES if c["id"] == cid)
    N, C, reg = c["N"], c["C"], L.focal_tol_regime(c)
    x, t = L.focal_inputs(c)
    bad_rows = [0, N // 2, N - 1]
    t_bad = t.copy()
    t_bad[bad_rows] = [C if v is None else v for v in L.FOCAL_BAD_TARGETS]
    ok = np.ones(N, bool); ok[bad_rows] = False
    _, g64 = L.focal_ref(x, np.where(ok, t, 0), c["gamma"])                   # rows are independent: 1 / N of each row's own gradient
    t_d = _cu(t_bad)
    loss, dl = _run_focal(ops, x, t_d, c["gamma"])
    assert bool(torch.isnan(loss[0])) and not bool(_untouched(loss[:1]).any()), "the loss must be a NaN the kernel wrote"
    got = _bits(dl[:N, :C])
    assert (got[~ok] == _KERNEL_NAN).all(), "rows with a target outside [0, C) must hold NaN in dlogits[:C]"
    _close("focal.dlogits", reg, dl[:N, :C][torch.from_numpy(ok).cuda()], g64[ok], cid)
    assert bool(_untouched(dl[:N, C:]).all() and _untouched(dl[N:]).all() and _untouched(loss[1:]).all())
    loss2, dl2 = _run_focal(ops, x, t_d, c["gamma"])
    assert _same_bits(dl2, dl) and bool(torch.isnan(loss2[0]))
    loss3, _ = _run_focal(ops, x, t_d, c["gamma"], with_grad=False)
    assert bool(torch.isnan(loss3[0])) and not bool(_untouched(loss3[:1]).any()) and bool(_untouched(loss3[1:]).all())


# ------------------------------------------------------------------------------------------------ sw_det_loss_per_image
@pytest.mark.parametrize("c", L.DETLOSS_CASES, ids=[c["id"] for c in L.DETLOSS_CASES])
def test_det_loss_per_image_against_float64(ops, c):
    inp = L.detloss_inputs(c)
    lo, de, lab, an, ma, lg, cls, bx, gt, cnt = [t.cuda() for t in inp]
    K = c["K"]
    assert lg.shape[1] == 5 * K + 1 + c["pad"]
    for box_type, gamma in L.DETLOSS_TYPES:
        def run():
            return ops.det_loss_per_image(lo, de, lab, an, ma, L.UNIT_WEIGHTS, c["rpn_bs"], box_type, lg, K, cls, bx, gt, cnt,
                                          c["max_rows"], L.REG_WEIGHTS, gamma, box_type)
        a = run(); b = run()
        torch.cuda.synchronize()
        what = f"{c['id']}-{box_type}-g{gamma:g}"
        assert a.shape == (c["N"], 5) and _same_bits(a, b), f"{what}: two launches differ"
        got = a.cpu().double().numpy()
        want = L.det_loss_ref(inp, c["rpn_bs"], box_type, K, gamma, box_type)
        nan_w = np.isnan(want)
        assert (np.isnan(got) == nan_w).all(), (what, np.argwhere(np.isnan(got) != nan_w))
        err = np.abs(got - want)[~nan_w] / (L.DETLOSS_ATOL + L.DETLOSS_RTOL * np.abs(want[~nan_w]))
        print(f"{what}: largest |got - ref| / (atol + rtol |ref|) = {err.max():.3g} (bar 1), {int(nan_w.sum())} NaN")
        np.testing.assert_allclose(got[~nan_w], want[~nan_w], rtol=L.DETLOSS_RTOL, atol=L.DETLOSS_ATOL, err_msg=what)
        s = a.cpu()
        tot = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]                      # f32, left to right (split_single.py:74)
        assert torch.equal(tot[~torch.isnan(tot)], s[:, 4][~torch.isnan(s[:, 4])]) and torch.equal(torch.isnan(tot), torch.isnan(s[:, 4]))
        zero_rows = np.asarray(c["counts"]) == 0
        assert (got[zero_rows, 0] == 0.0).all()                              # CE over no rows: 0 (layers/wrappers.py:26-33)
        if box_type == "smooth_l1":
            assert (got[zero_rows, 1] == 0.0).all()
            if c["bad_image"] is None:
                assert not nan_w.any()
        else:
            assert nan_w[zero_rows, 1].all()                                  # torch's mean over an empty foreground set
            if c["N"] > 2:
                assert nan_w[0, 3] and (c["counts"][1] == 0 or nan_w[1, 1])    # no RPN foreground / no ROI foreground
        if c["bad_image"] is not None:                                       # a class id K + 1: that image's loss_cls and sum, no other image
            bi = c["bad_image"]
            assert nan_w[bi, 0] and nan_w[bi, 4] and not nan_w[np.arange(c["N"]) != bi][:, [0, 2]].any()


# ------------------------------------------------------------------------------------------------ sw_wsddn_scores_bwd
def _scores_bwd_close(got, ref, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"{what} holds non-finite values"
    d, m = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{what}: |err| {d:.3g}, bar {L.SCORES_BWD_REL * m + L.SCORES_BWD_ABS:.3g} (max|ref| {m:.3g})")
    assert d <= L.SCORES_BWD_REL * m + L.SCORES_BWD_ABS, f"{what} off by {d:.3g} (max|ref| {m:.3g})"


def _run_scores_bwd(ops, x, g, R, K):
    ld, ld_g, ld_d = L.scores_bwd_layout(K)
    lg = torch.full((R, ld), float("nan"), device="cuda"); lg[:, :2 * K] = _cu(x)
    gs = torch.full((R, ld_g), float("nan"), device="cuda"); gs[:, :K] = _cu(g)
    d = _sent(R + 2, ld_d)
    ops.wsddn_scores_bwd(lg[:, :2 * K], K, gs[:, :K], d[:R, :2 * K])
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("c", L.SCORES_BWD_CASES, ids=[c["id"] for c in L.SCORES_BWD_CASES])
def test_wsddn_scores_bwd_against_float64(ops, c):
    R, K = c["R"], c["K"]
    x, g = L.scores_bwd_inputs(c)
    dC, dD = L.wsddn_scores_bwd_ref(x, K, g)
    d = _run_scores_bwd(ops, x, g, R, K)
    _scores_bwd_close(d[:R, :K], dC, c["id"] + " dC")
    _scores_bwd_close(d[:R, K:2 * K], dD, c["id"] + " dD")
    assert bool(_untouched(d[:R, 2 * K:]).all()), "gradient columns beyond 2K were written"
    assert bool(_untouched(d[R:]).all()), "gradient rows beyond R were written"
    assert _same_bits(_run_scores_bwd(ops, x, g, R, K), d), "two launches differ"


@pytest.mark.parametrize("K", L.SCORES_BWD_REFUSED)
def test_wsddn_scores_bwd_refuses_what_exceeds_lds_and_writes_nothing(ops, K):
    R = 5
    d = _sent(R, 2 * K)
    with pytest.raises(Exception, match="sw_wsddn_scores_bwd"):
        ops.wsddn_scores_bwd(torch.zeros(R, 2 * K, device="cuda"), K, torch.ones(R, K, device="cuda"), d)
    torch.cuda.synchronize()
    assert bool(_untouched(d).all())


# ------------------------------------------------------------------------------------------------ sw_threshold_select
def _select_entry(ops, scores_d, classes_d, boxes_d, thres, allowed_d, n_allowed):
    """the C entry on buffers this test owns (n + 2 rows each) -> count (2,), boxes, classes or None, scores, index"""
    from sos_wsod_amd._lib import check, lib
    n = scores_d.shape[0]
    cnt, ob, osc, oi = _sent(2, dtype=torch.int32), _sent(n + 2, 4), _sent(n + 2), _sent(n + 2, dtype=torch.int32)
    oc = _sent(n + 2, dtype=torch.int32) if classes_d is not None else None
    check(lib.sw_threshold_select(n, ops._p(scores_d), ops._p(classes_d), ops._p(boxes_d), float(thres), ops._p(allowed_d), n_allowed,
                                  ops._p(cnt), ops._p(ob), ops._p(oc), ops._p(osc), ops._p(oi), ops._stream()), "sw_threshold_select")
    torch.cuda.synchronize()
    return cnt, ob, oc, osc, oi


def _select_check(what, out, want, has_classes):
    cnt, ob, oc, osc, oi = out
    wb, wc, ws, wi = want
    k = int(cnt[0].item())
    assert k == len(wi), f"{what}: kept {k}, the oracle keeps {len(wi)}"
    assert np.array_equal(oi[:k].cpu().numpy(), wi.astype(np.int32))
    assert np.array_equal(_bits(ob[:k]), wb.view(np.int32).reshape(-1, 4)) and np.array_equal(_bits(osc[:k]), ws.view(np.int32))
    if has_classes:
        assert np.array_equal(oc[:k].cpu().numpy(), wc)
    return k


@pytest.mark.parametrize("c", L.SELECT_CASES, ids=[c["id"] for c in L.SELECT_CASES])
def test_threshold_select_bit_exact_against_the_oracle(ops, c):
    scores, classes, boxes, thres = L.select_inputs(c)
    n = c["n"]
    s_d, c_d, b_d = _cu(scores), _cu(classes), _cu(boxes)
    some = torch.zeros(1, dtype=torch.int32, device="cuda")                   # a valid address for "non-NULL with n_allowed == 0"
    for name, (cls_kind, allowed) in L.SELECT_FILTERS.items():
        what = f"{c['id']}-{name}"
        has_classes = cls_kind == "classes"
        with np.errstate(invalid="ignore"):
            want = SO.threshold_bbox(scores, classes if has_classes else None, boxes, thres, allowed)
        a_d = None if allowed is None else torch.tensor(allowed, dtype=torch.int32).cuda()
        # through ops.threshold_select (what semisup.threshold_bbox calls)
        got = ops.threshold_select(s_d, c_d if has_classes else None, b_d, thres, a_d)
        torch.cuda.synchronize()
        k = _select_check(what, got, want, has_classes)
        print(f"{what}: kept {k} of {n}")
        if name == "empty":
            assert k == 0
        # through the C entry on sentinel buffers: NULL = no filter, non-NULL with n_allowed == 0 = keep nothing
        if allowed is None:
            ptr, n_allowed = None, 0
        else:
            ptr, n_allowed = (a_d if len(allowed) else some), len(allowed)
        out = _select_entry(ops, s_d, c_d if has_classes else None, b_d, thres, ptr, n_allowed)
        assert _select_check(what, out, want, has_classes) == k
        cnt, ob, oc, osc, oi = out
        assert bool(_untouched(cnt[1:]).all() and _untouched(ob[k:]).all() and _untouched(osc[k:]).all() and _untouched(oi[k:]).all())
        assert oc is None or bool(_untouched(oc[k:]).all())
        again = _select_entry(ops, s_d, c_d if has_classes else None, b_d, thres, ptr, n_allowed)
        assert all(x is None or _same_bits(x, y) for x, y in zip(out, again)), f"{what}: two launches differ"


def test_threshold_bbox_with_an_empty_label_set_keeps_nothing():
    """semisup.threshold_bbox(..., has_multi_label=True) on an image whose multi_label is empty: no class is in an empty set
    (trainer.py:381-386), so the result is an empty Instances"""
    from sos_wsod_amd import semisup
    from sos_wsod_amd.structures import Boxes, Instances
    scores, classes, boxes, _ = L.select_inputs(dict(n=1025, kind="all"))
    p = Instances((480, 640))
    p.pred_boxes = Boxes(_cu(boxes)); p.scores = _cu(scores); p.pred_classes = _cu(classes).long()
    out = semisup.threshold_bbox({"multi_label": []}, p, thres=-0.5, proposal_type="roih", has_multi_label=True)
    assert len(out) == 0 and out.gt_boxes.tensor.shape == (0, 4) and out.gt_classes.numel() == 0 and out.scores.numel() == 0
    out = semisup.threshold_bbox({"multi_label": [int(classes[0])]}, p, thres=-0.5, proposal_type="roih", has_multi_label=True)
    assert len(out) == int((classes == classes[0]).sum())

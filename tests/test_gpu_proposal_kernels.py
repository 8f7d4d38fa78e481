"""GPU: the index-side kernels of the Stage-3 detector (csrc/proposals.hip) at their radix, chunk, capacity and tie edges, through
their entry points: ops.rpn_select_pack (selection bit for bit against torch.sort(descending, stable); decode against float64),
ops.rpn_label_anchors and ops.roi_label_sample (every label / sampled row against oracle.frcnn_oracle with its closed-form
permutation), ops.roi_assign_levels (against the oracle; exact at the power-of-two edges).  The case tables and references live in
tests/proposals_ref.py; tests/test_proposals_ref_cpu.py proves that each table reaches the edge it is named for.  Every refused size is
one the entry point turns down before it launches anything; no case hands a kernel a size its entry point accepts but cannot hold."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import proposals_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. selection
def _select(ops, levels, pre_topk, single_tensor=False, hw=R.SEL_IMG_HW):
    """levels: per level (N, n_l) logits; index anchors, zero deltas -> (scores, boxes, finite) on the host"""
    N = levels[0].shape[0]
    anchors = [_t(R.index_anchors(l.shape[1])) for l in levels]
    img_hw = torch.tensor([list(hw)] * N, dtype=torch.int32).cuda()
    if single_tensor:
        lg = _t(np.concatenate(levels, 1))
        sc, bx, fin = ops.rpn_select_pack(lg, torch.zeros(*lg.shape, 4, device="cuda"), anchors, pre_topk, R.W1, R.SCALE_CLAMP, img_hw)
    else:
        sc, bx, fin = ops.rpn_select_pack([_t(l) for l in levels], [torch.zeros(*l.shape, 4, device="cuda") for l in levels], anchors, pre_topk,
                                          R.W1, R.SCALE_CLAMP, img_hw)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), bx.cpu().numpy(), fin.cpu().numpy()


def _check_selection(ops, levels, pre_topk, what, single_tensor=False):
    sc, bx, fin = _select(ops, levels, pre_topk, single_tensor)
    want_sc, want_bx, want_fin = R.select_expected(levels, pre_topk)
    L = len(levels)
    # the row order: every box is its anchor, and the anchor spells its index
    bad = np.nonzero((bx != want_bx).any(2))
    assert bad[0].size == 0, f"{what}: {bad[0].size} rows hold another anchor than torch.sort(stable)[:k], first (image, row) {(int(bad[0][0]), int(bad[1][0]))}: " \
                             f"got {bx[bad[0][0], bad[1][0], :4].tolist()}, want {want_bx[bad[0][0], bad[1][0], :4].tolist()}"
    assert R.same_bits(bx, want_bx), f"{what}: boxes differ in bits (a signed zero)"
    assert R.same_bits(sc, want_sc), f"{what}: the score column does not hold the logit / unused entries are not -inf"
    assert np.array_equal(fin != 0, want_fin != 0), f"{what}: finite {fin.tolist()} != {want_fin.tolist()}"
    assert bx.shape[2] == 4 * L and sc.shape[2] == L + 1


@pytest.mark.parametrize("n", R.SEG_N)
def test_selection_at_segment_lengths_and_k_edges(ops, n):
    lg = R.quantised_logits(2, n, 0)
    for pre in R.seg_pre_topks(n):
        _check_selection(ops, [lg], pre, f"n={n} pre_topk={pre}")


@pytest.mark.parametrize("n,pre,cap", R.CAP_CASES, ids=[f"pre{p}-cap{c}" for _, p, c in R.CAP_CASES])
def test_selection_at_sort_capacity_edges(ops, n, pre, cap):
    _check_selection(ops, [R.quantised_logits(1, n, pre)], pre, f"n={n} pre_topk={pre} (capacity {cap})")


@pytest.mark.parametrize("which", R.RADIX_SETS)
def test_selection_radix_digit_edges(ops, which):
    v = R.radix_logits(which)
    for k in R.radix_ks(which):
        _check_selection(ops, [v[None]], k, f"radix set {which} pre_topk={k}")


@pytest.mark.parametrize("name", sorted(R.tie_cases()))
def test_selection_tie_edges(ops, name):
    v, k = R.tie_cases()[name]
    _check_selection(ops, [v[None]], k, f"ties {name}")


def test_selection_special_values(ops):
    """+0 / -0 tie (index order decides), denormals keep their order, NaN first in index order, +-inf and -FLT_MAX in place; a selected
    NaN or inf logit clears `finite` of ITS image only and scores -inf"""
    lg = R.special_logits()
    _check_selection(ops, [lg], R.SPECIAL_PRE, "special values")
    _check_selection(ops, [lg[:1]], R.SPECIAL_PRE, "signed zeros alone")


@pytest.mark.parametrize("name", sorted(R.SHAPE_CASES))
def test_selection_call_shapes(ops, name):
    N, n_l, pre, single = R.SHAPE_CASES[name]
    _check_selection(ops, R.shape_logits(name), pre, f"shape {name}", single_tensor=single)


def test_selection_refusals_return_before_any_launch(ops):
    """pre_topk above 16384 and more than 8 levels are turned down by the entry point's first check"""
    from sos_wsod_amd._lib import HipKernelError
    lg = R.quantised_logits(1, 300, 1)
    with pytest.raises(HipKernelError, match="-5"):
        _select(ops, [lg], R.PRE_TOPK_MAX + 1)
    with pytest.raises(HipKernelError, match="-5"):
        _select(ops, [lg] * 9, 100)
    _check_selection(ops, [lg] * 8, 100, "8 levels after the refusals")


# ------------------------------------------------------------------------------------------------ 2. decode
@pytest.mark.parametrize("weights", R.DEC_WEIGHTS, ids=["w1", "w10-10-5-5"])
def test_decode_against_float64(ops, weights):
    """boxes within 4 x the float32 CPU reference's own max error against float64 (measured on these inputs); 'kept or emptied' where
    float64 leaves no doubt; the exactly-empty boxes (x2 == 0, x1 == W, wholly outside) emptied; one inf delta clears finite[1] only"""
    c, e = R.decode_case(weights), R.decode_expected(weights)
    N, L = R.DEC_N, len(R.DEC_LEVELS)
    pre = max(R.DEC_LEVELS)
    img_hw = torch.tensor([list(R.DEC_HW)] * N, dtype=torch.int32).cuda()
    sc, bx, fin = ops.rpn_select_pack([_t(x) for x in c["logits"]], [_t(x) for x in c["deltas"]], [_t(x) for x in c["anchors"]], pre, weights,
                                      R.SCALE_CLAMP, img_hw)
    torch.cuda.synchronize()
    sc, bx, fin = sc.cpu().numpy(), bx.cpu().numpy(), fin.cpu().numpy()
    assert np.array_equal(fin != 0, e["finite"] != 0)
    worst = 0.0
    for l, n in enumerate(R.DEC_LEVELS):
        for img in range(N):
            rows = slice(l * pre, l * pre + n)
            got = bx[img, rows, 4 * l:4 * l + 4].astype(np.float64)
            assert np.array_equal(bx[img, rows], np.tile(bx[img, rows, :4], (1, L)))
            ref = e["box64"][l][img]
            ok = np.isfinite(ref)
            assert np.array_equal(got[~ok], ref[~ok])                                     # the inf row: the same infinities
            worst = max(worst, float(np.abs(got[ok] - ref[ok]).max()))
            lg = c["logits"][l][img][e["order"][l][img]]
            want_s = np.where(e["keep"][l][img], lg, -np.inf).astype(np.float32)
            sure = e["sure"][l][img]
            assert R.same_bits(sc[img, rows, l][sure], want_s[sure]), (l, img)
            assert np.isin(sc[img, rows, l][~sure], np.concatenate([lg[~sure], [-np.inf]])).all()
            assert np.isneginf(np.delete(sc[img, rows], l, axis=1)).all() and np.isneginf(sc[img, l * pre + n:(l + 1) * pre]).all()
            assert not bx[img, l * pre + n:(l + 1) * pre].any()
            if l == 0:                                                                    # exact arithmetic (zero deltas): no allowance
                at = {int(a): r for r, a in enumerate(e["order"][0][img])}
                for nm in ("zero_w_left", "zero_w_right", "outside"):
                    assert np.isneginf(sc[img, at[R.DEC_NAMED[nm]], 0]), nm
                assert bx[img, at[R.DEC_NAMED["zero_w_left"]], 2] == 0 and bx[img, at[R.DEC_NAMED["zero_w_right"]], 0] == R.DEC_HW[1]
                w_of = lambda nm: float(bx[img, at[R.DEC_NAMED[nm]], 2]) - float(bx[img, at[R.DEC_NAMED[nm]], 0])
                assert w_of("dw_eq") == w_of("dw_above") > w_of("dw_below")               # the clamp holds at and above scale_clamp
    print(f"decode {weights}: max |box - float64| {worst:.3g}, bar {e['bar']:.3g} (float32 reference: {e['e32']:.3g})")
    assert worst <= e["bar"]


def test_decode_keeps_nan_size_deltas(ops):
    """the RPN's clamps of dw and of dh keep a NaN as torch.clamp(max=) does (the heads' fminf drops it): a NaN dw makes x0 and x2 of
    that box NaN, a NaN dh y0 and y2, the score is -inf and finite[img] is cleared; the other image is untouched by it"""
    an = _t(np.array([[10, 10, 30, 50], [100, 100, 120, 140]], np.float32))
    dl = np.zeros((2, 2, 4), np.float32)
    dl[0, 0, 2] = np.nan                                                                # dw of anchor 0, dh of anchor 1: one clamp each
    dl[0, 1, 3] = np.nan
    img_hw = torch.tensor([[300, 400]] * 2, dtype=torch.int32).cuda()
    sc, bx, fin = ops.rpn_select_pack([_t(np.array([[2.0, 1.0]] * 2, np.float32))], [_t(dl)], [an], 2, R.W1, R.SCALE_CLAMP, img_hw)
    torch.cuda.synchronize()
    sc, bx, fin = sc.cpu().numpy(), bx.cpu().numpy(), fin.cpu().numpy()
    assert (fin != 0).tolist() == [False, True]
    assert np.isnan(bx[0, 0, [0, 2]]).all() and bx[0, 0, [1, 3]].tolist() == [10.0, 50.0] and np.isneginf(sc[0, 0]).all()
    assert np.isnan(bx[0, 1, [1, 3]]).all() and bx[0, 1, [0, 2]].tolist() == [100.0, 120.0] and np.isneginf(sc[0, 1]).all()
    assert bx[1].tolist() == [[10.0, 10.0, 30.0, 50.0], [100.0, 100.0, 120.0, 140.0]] and sc[1, :, 0].tolist() == [2.0, 1.0]


# ------------------------------------------------------------------------------------------------ 3. anchor labels
@pytest.mark.parametrize("case", R.LABEL_CASES, ids=[c[0] for c in R.LABEL_CASES])
def test_rpn_label_anchors_against_the_oracle(ops, case):
    name, A, kinds, batch, max_pos = case
    an, gts, seeds, want_labels, want_matched = R.label_expected(case)
    n_gt = [len(g) for g in gts]
    cat = _t(np.concatenate(gts, 0)) if sum(n_gt) else torch.zeros(0, 4, device="cuda")
    labels, matched = ops.rpn_label_anchors(_t(an), cat, n_gt, seeds, batch, max_pos)
    torch.cuda.synchronize()
    labels, matched = labels.cpu().numpy().astype(np.int64), matched.cpu().numpy()
    for i in range(len(gts)):
        diff = np.nonzero(labels[i] != want_labels[i])[0]
        assert diff.size == 0, f"{name} image {i} ({kinds[i]}): {diff.size} labels differ, first anchor {int(diff[0])}: got {int(labels[i][diff[0]])}, " \
                               f"want {int(want_labels[i][diff[0]])}"
        assert R.same_bits(matched[i], want_matched[i]), f"{name} image {i} ({kinds[i]}): matched boxes differ"
    if batch >= A and max_pos == batch and kinds[0] == "thr" and A >= 9:                # nothing is sampled away: the matcher's own labels
        pos = R.special_positions(A)
        by_m = {m: int(labels[0][pos[j]]) for j, m in enumerate(R.SPECIAL_M)}
        assert by_m == {70: 1, 30: -1, 100: 1, 71: 1, 69: -1, 31: -1, 29: 0, 1: 0}, by_m   # IoU == 0.7 -> 1, == 0.3 -> -1 and not 0
        assert np.array_equal(matched[0][pos[len(R.SPECIAL_M)]], R.SPLIT_GT[0])            # two equally good boxes: the first wins


def test_rpn_label_anchors_pairwise_iou_edge_pairs(ops):
    """pairwise_iou at its edges, nothing sampled away, against the oracle's matcher: a box that shares only an edge with the
    ground-truth box (inter == 0: IoU exactly 0), a zero-area box against itself (0, not 0 / 0 = NaN: as the image's only
    ground-truth box its best IoU is 0, so every anchor with IoU 0 is a low-quality positive, the twin included), and an anchor with
    a NaN coordinate.  There the oracle's intersection is NaN and its where(inter > 0, ., 0) gives 0; the kernel's fminf / fmaxf drop
    the NaN, its intersection is positive and pairwise_iou returns inter / NaN = NaN, not 0: the labels agree because a NaN never
    wins `v > best` and never equals a ground-truth box's best IoU"""
    gt = np.array([10, 10, 20, 20], np.float32)
    flat = np.array([30, 30, 30, 40], np.float32)                                       # zero width
    an = np.array([[10, 10, 20, 20], [20, 10, 30, 20], [10, 20, 20, 30], [12, 10, 22, 20], flat, [40, 40, 50, 50],
                   [np.nan, 10, 20, 20], [10, 10, 20, np.nan]], np.float32)
    for name, gtb in (("edge", gt[None]), ("flat_twin", flat[None]), ("both", np.stack([gt, flat]))):
        want = R.matcher_labels(an, gtb)
        labels, matched = ops.rpn_label_anchors(_t(an), _t(gtb), [len(gtb)], [1, 2], 64, 64)
        torch.cuda.synchronize()
        got = labels.cpu().numpy().astype(np.int64)[0]
        assert np.array_equal(got, want), f"{name}: labels {got.tolist()}, the oracle's matcher {want.tolist()}"
    assert R.matcher_labels(an, gt[None]).tolist()[:3] == [1, 0, 0]                    # the edge neighbours are background, not ignored
    assert R.matcher_labels(an, flat[None])[4] == 1                                     # the twin of the zero-area box: IoU 0 == its best


# ------------------------------------------------------------------------------------------------ 4. ROI sampling
def _roi_call(ops, case):
    name, imgs, p_stride, append, batch, max_pos = case
    props, gts, seeds, want = R.roi_expected(case)
    N = len(imgs)
    buf = np.full((N, p_stride, 4), 7.0, np.float32)                                      # rows beyond p_cnt: never read
    for i, p in enumerate(props):
        buf[i, :len(p)] = p
    n_gt = [len(g[0]) for g in gts]
    tot = sum(n_gt)
    cat_b = _t(np.concatenate([g[0] for g in gts], 0)) if tot else torch.zeros(0, 4, device="cuda")
    cat_c = _t(np.concatenate([g[1] for g in gts], 0).astype(np.int32)) if tot else torch.zeros(0, dtype=torch.int32, device="cuda")
    out = ops.roi_label_sample(_t(np.array([len(p) for p in props], np.int32)), _t(buf), cat_b, cat_c, n_gt, seeds, append, 0.5, R.ROI_K, batch, max_pos)
    torch.cuda.synchronize()
    return want, [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("case", R.ROI_CASES, ids=[c[0] for c in R.ROI_CASES])
def test_roi_label_sample_against_the_oracle(ops, case):
    name, imgs, p_stride, append, batch, max_pos = case
    want, (cnt, idx, cls, both) = _roi_call(ops, case)
    for i, w in enumerate(want):
        n = int(cnt[i])
        assert n == len(w["sampled_idx"]), f"{name} image {i}: count {n}, oracle {len(w['sampled_idx'])}"
        assert np.array_equal(idx[i, :n], w["sampled_idx"]), f"{name} image {i}: sampled rows / their order differ"
        assert np.array_equal(cls[i, :n], w["gt_classes"]), f"{name} image {i}: classes differ"
        assert R.same_bits(both[0, i, :n], w["boxes"]) and R.same_bits(both[1, i, :n], w["gt_boxes"]), f"{name} image {i}: boxes differ"
        assert (idx[i, n:] == -1).all() and (cls[i, n:] == -1).all() and not both[:, i, n:].any(), f"{name} image {i}: rows beyond the count"


def test_roi_label_sample_refuses_more_than_4096_rows_before_launch(ops):
    from sos_wsod_amd._lib import HipKernelError
    with pytest.raises(HipKernelError, match="-6"):
        _roi_call(ops, R.ROI_REFUSED)


# ------------------------------------------------------------------------------------------------ 5. FPN levels
def _levels_call(ops, boxes, row_cnt):
    """the images' blocks lie apart in one buffer (a gap of 3 boxes between them)"""
    R_ = len(boxes)
    base = np.full((R_ + 3 * len(row_cnt), 4), np.nan, np.float32)
    offs, at, r0 = [], 0, 0
    for c in row_cnt:
        offs.append(at * 4)
        base[at:at + c] = boxes[r0:r0 + c]
        at += c + 3; r0 += c
    rois, lv, sel, cnt = ops.roi_assign_levels(_t(base), row_cnt, offs)
    torch.cuda.synchronize()
    return rois.cpu().numpy(), lv.cpu().numpy().astype(np.int64), sel.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)


def _check_level_lists(lv, sel, cnt, R_):
    assert int(cnt.sum()) == R_ and ((lv >= 0) & (lv <= 3)).all()
    for l in range(4):
        assert np.array_equal(sel[l, :cnt[l]], np.nonzero(lv == l)[0]), f"level {l}: the row list is not ascending and complete"


@pytest.mark.parametrize("R_", R.LEVEL_R)
def test_roi_assign_levels_at_level_and_slab_edges(ops, R_):
    boxes, kind, row_cnt = R.level_case(R_)
    rois, lv, sel, cnt = _levels_call(ops, boxes, row_cnt)
    img = np.repeat(np.arange(3), row_cnt).astype(np.float32)
    assert np.array_equal(rois[:, 0], img) and np.array_equal(rois[:, 1:], boxes)
    want = R.level_expected(boxes, kind)
    diff = lv != want
    assert not (diff & (kind != 2)).any(), f"R={R_}: rows {np.nonzero(diff & (kind != 2))[0][:8].tolist()} differ (kinds " \
                                           f"{kind[diff & (kind != 2)][:8].tolist()}: 1 = exact edge, 3 = odd size, 4 = negative side -> level 0)"
    assert not (diff & ~R.near_level_edge(boxes)).any()                                   # a one-ulp neighbour may move, nothing else
    assert (np.abs(lv - want)[diff] == 1).all()
    _check_level_lists(lv, sel, cnt, R_)


def test_roi_assign_levels_with_levels_that_receive_no_rows(ops):
    boxes = R.small_boxes(1500)
    rois, lv, sel, cnt = _levels_call(ops, boxes, [700, 0, 800])
    assert cnt.tolist() == [1500, 0, 0, 0] and not lv.any()
    _check_level_lists(lv, sel, cnt, 1500)

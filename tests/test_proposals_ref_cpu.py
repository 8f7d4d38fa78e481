"""CPU: the references and case tables of tests/proposals_ref.py.  The references are pinned to torch and to the oracle on random
inputs; each case table is shown, with the model of the kernel's selection key, to reach the edge it is named for (which radix pass
decides, which digit, the size of the tied group, the chunks it spans, the sort capacity, the segment and image counts); and every cap
the GPU tests rely on (decode bar and the share of rows it excuses, the excusable level rows) is asserted for the reference alone.
`python tests/test_proposals_ref_cpu.py` prints the measured decode bars."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import frcnn_oracle as FO  # noqa: E402
import proposals_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------ key model and selection reference
def test_key_model_orders_like_torch_sort_on_random_and_special_floats():
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 1 << 32, 6000, dtype=np.uint64).astype(np.uint32)              # every float class, NaN included
    v = np.concatenate([bits.view(np.float32), np.array([0.0, -0.0, np.inf, -np.inf, np.nan, R.DEN_MIN, -R.DEN_MIN, R.FLT_MAX, -R.FLT_MAX] * 3, np.float32)])
    v = v[rng.permutation(len(v))]
    assert np.isnan(v).sum() > 10 and (v == 0).sum() >= 6
    assert np.array_equal(R.model_order(v), R.sort_ref(v, len(v)))
    k = R.desc_key(v)
    assert (k[np.isnan(v)] == 0).all() and (k != R.KEY_NONE).all()
    z = R.desc_key(np.array([0.0, -0.0], np.float32))
    assert z[0] == z[1]
    fin = v[~np.isnan(v) & (v != 0)]
    assert R.same_bits(R.float_of_key(R.desc_key(fin)), fin)                              # the inverse used to build logits from keys


def test_sort_ref_disagrees_with_the_numpy_argsort_on_nan():
    """why the selection reference is torch.sort and not the oracle's numpy argsort: NaN goes first here, last there"""
    v = np.array([1.0, np.nan, 3.0, np.nan, 2.0], np.float32)
    assert R.sort_ref(v, 5).tolist() == [1, 3, 2, 4, 0]
    assert FO._sort_desc_stable(v).tolist()[-2:] == [1, 3]
    q = R.quantised_logits(1, 3000, 9)[0]
    assert np.array_equal(R.sort_ref(q, 3000), FO._sort_desc_stable(q))                   # and agree everywhere else


def test_index_anchors_decode_exactly_to_themselves():
    an = R.index_anchors(16500)
    assert len(np.unique(an[:, :2], axis=0)) == 16500 and an.max() < min(R.SEL_IMG_HW)
    assert R.same_bits(R.apply_deltas32(np.zeros((16500, 4), np.float32), an, R.W1), an)
    assert np.array_equal(R.apply_deltas64(np.zeros((16500, 4), np.float32), an, R.W1), an.astype(np.float64))


def test_unreachable_top_digits_are_nan_bit_patterns():
    """the top radix digit of a non-NaN float is 3 (+inf only), 4 .. 2043, or 2044 (-inf only): digits 0..2 and 2045..2047 are NaN bit
    patterns, which the key folds onto 0 — so 'digit 0' of pass 0 is reached by NaN and 'the last digit' by -inf"""
    for d in (0, 1, 2, 2045, 2046, 2047):
        for low in (0, 1, 0x1FFFFF):
            assert np.isnan(R.float_of_key(np.array([(d << 21) | low], np.uint64)))[0]
    assert R.digits(R.desc_key(np.array([np.inf, R.FLT_MAX, -R.FLT_MAX, -np.inf, np.nan], np.float32)))[0].tolist() == [3, 4, 2043, 2044, 0]


@pytest.mark.parametrize("n", R.SEG_N)
def test_segment_cases_reach_take_all_threshold_and_chunk_edges(n):
    lg = R.quantised_logits(2, n, 0)
    modes = set()
    for pre in R.seg_pre_topks(n):
        for img in range(2):
            w = R.radix_walk(lg[img], min(n, pre))
            modes.add(w["mode"])
            if w["mode"] == 0:
                assert np.array_equal(R.model_order(lg[img])[:pre], R.sort_ref(lg[img], pre))
    assert 1 in modes and (n == 1 or 0 in modes)
    assert R.seg_pre_topks(n)[-1] == n + 1 and (n == 1 or {1, n - 1, n} <= set(R.seg_pre_topks(n)))
    assert {1023, 1024, 1025} <= set(R.SEG_N) and {(n + R.CHUNK - 1) // R.CHUNK for n in R.SEG_N} >= {1, 2, 3, 5}


def test_capacity_cases_reach_1024_2048_and_the_large_lds_branch():
    assert [(R.sort_capacity(p), p <= n) for n, p, _ in R.CAP_CASES] == [(c, True) for _, _, c in R.CAP_CASES]
    assert any(c * 8 > 64 * 1024 for _, _, c in R.CAP_CASES) and any(p == R.PRE_TOPK_MAX for _, p, _ in R.CAP_CASES)
    assert {1024, 1025} <= {p for _, p, _ in R.CAP_CASES}


@pytest.mark.parametrize("which", R.RADIX_ONE_DIGIT)
def test_radix_sets_differ_in_one_digit_and_the_threshold_lands_on_its_first_and_last_value(which):
    v = R.radix_logits(which)
    d = R.digits(R.desc_key(v))
    p = {"top": 0, "mid": 1, "low": 2, "top_special": 0}[which]
    for q in range(3):
        assert (len(np.unique(d[q])) == 1) == (q != p), (which, q)                        # only digit p varies
    lo, hi = int(d[p].min()), int(d[p].max())
    want_lo, want_hi = {"top": (4, 2043), "mid": (0, 2047), "low": (0, 1023), "top_special": (0, 2044)}[which]
    assert (lo, hi) == (want_lo, want_hi)
    seen = []
    for k in R.radix_ks(which):
        w = R.radix_walk(v, k)
        assert w["mode"] == 0 and w["deciding"] == p
        assert all(pure is False for _, _, pure in w["passes"][:p])                       # the earlier passes see one mixed bucket
        seen.append((w["passes"][p][0], w["k_rem"], w["group"]))
        assert np.array_equal(R.model_order(v)[:k], R.sort_ref(v, k))
    assert seen[0][0] == lo and seen[0][1] == 1 and seen[1][0] == lo and seen[1][1] == seen[1][2]      # one of / all of the first group
    assert seen[-1][0] == hi and seen[-2][0] == hi and seen[-2][1] == 1 and lo < seen[2][0] < hi
    assert all(seen[j][2] >= 3 for j in (0, 1, 3, 4))                                     # the first and the last group are ties of several
    if which == "top_special":
        assert np.isnan(v).sum() == 4 and np.isneginf(v).sum() == 5


def test_radix_pair_set_puts_the_threshold_in_either_of_two_buckets_that_share_21_bits():
    v = R.radix_logits("pair")
    d = R.digits(R.desc_key(v))
    assert len(np.unique(d[0])) == 1 and sorted(np.unique(d[1]).tolist()) == [0x2AA, 0x2AB] and len(np.unique(d[2])) > 900
    assert len(np.unique(R.desc_key(v) >> 11)) == 1                                       # equal in the top 21 bits: bit 10 alone tells them apart
    picked = []
    for k in R.radix_ks("pair"):
        w = R.radix_walk(v, k)
        assert w["mode"] == 0 and w["deciding"] == 2 and w["passes"][1][1] < len(v)
        picked.append(w["passes"][1][0])
        sibling = (d[1] != w["passes"][1][0]) & (d[2] < w["passes"][2][0])
        assert sibling.sum() > 100                                                        # the other bucket holds smaller low digits too
        assert np.array_equal(R.model_order(v)[:k], R.sort_ref(v, k))
    assert picked == [0x2AA, 0x2AB, 0x2AB]


def test_tie_cases_span_the_chunks_they_claim():
    t = R.tie_cases()
    w = R.radix_walk(*t["all_equal"])
    assert w["group"] == 5000 and w["chunks"] == [0, 1, 2, 3, 4] and w["k_rem"] == 2500 and w["cut_chunk"] == 2 and w["cut_index"] % R.CHUNK not in (0, 1023)
    w = R.radix_walk(*t["interleaved_mid"])
    assert w["group"] == 1000 and w["chunks"] == [0, 1, 2] and w["k_rem"] == 500 and w["cut_chunk"] == 1 and 100 < w["cut_index"] % R.CHUNK < 900
    lg = t["interleaved_mid"][0]
    k = R.desc_key(lg)
    assert (k < w["T"]).sum() == 1000 and (k > w["T"]).sum() == 1000
    after = np.arange(3000) > w["cut_index"]
    assert (after & (k < w["T"]) & (np.arange(3000) // R.CHUNK == 1)).any()               # smaller keys follow the cut inside its chunk
    w = R.radix_walk(*t["interleaved_end"])
    assert w["k_rem"] == w["group"] == 1000
    w = R.radix_walk(*t["interleaved_one"])
    assert w["k_rem"] == 1 and w["group"] == 1000
    for lg, k in t.values():
        assert np.array_equal(R.model_order(lg)[:k], R.sort_ref(lg, k))


def test_special_value_cases_cut_their_tied_groups():
    lg = R.special_logits()
    w = [R.radix_walk(lg[i], R.SPECIAL_PRE) for i in range(3)]
    assert all(x["mode"] == 0 and x["group"] == 600 and x["k_rem"] == 300 for x in w)
    assert w[0]["T"] == int(R.desc_key(np.zeros(1, np.float32))[0])
    z = lg[0][lg[0] == 0]
    assert np.signbit(z).any() and not np.signbit(z).all()                                # +0 and -0 mixed inside the tied group
    sel1 = R.sort_ref(lg[1], R.SPECIAL_PRE)
    assert np.isnan(lg[1][sel1[:7]]).all() and np.array_equal(sel1[:7], np.nonzero(np.isnan(lg[1]))[0])       # NaN first, index order
    assert w[2]["T"] == int(R.desc_key(np.array([-R.FLT_MAX]))[0]) and np.isposinf(lg[2]).sum() == 3 and np.isneginf(lg[2]).sum() == 500
    den = np.abs(lg[[0, 2]]) < np.finfo(np.float32).tiny
    assert (den & (lg[[0, 2]] != 0)).sum() > 700
    sc, bx, fin = R.select_expected([lg], R.SPECIAL_PRE)
    assert fin.tolist() == [1, 0, 0]
    for i in range(3):
        assert np.array_equal(R.model_order(lg[i])[:R.SPECIAL_PRE], R.sort_ref(lg[i], R.SPECIAL_PRE))


def test_shape_cases_reach_the_segment_limits():
    seg = {k: v[0] * len(v[1]) for k, v in R.SHAPE_CASES.items()}
    assert seg["seg40"] == R.MAX_SEG and seg["seg45"] == 45 and seg["single_tensor_ranges"] > R.MAX_SEG
    assert len(R.SHAPE_CASES["L1"][1]) == 1 and len(R.SHAPE_CASES["L8_mixed"][1]) == 8 == len(R.SHAPE_CASES["seg40"][1])
    N, n_l, pre, _ = R.SHAPE_CASES["L8_mixed"]
    assert any(n < pre for n in n_l) and any(n > pre for n in n_l) and any(n == pre for n in n_l)
    lg = R.shape_logits("L8_mixed")
    assert {R.radix_walk(l[0], min(pre, l.shape[1]))["mode"] for l in lg} == {0, 1}
    assert R.SHAPE_CASES["single_tensor"][3] and not R.SHAPE_CASES["seg45"][3]
    sc, bx, fin = R.select_expected(lg, pre)
    assert sc.shape == (N, 8 * pre, 9) and bx.shape == (N, 8 * pre, 32) and fin.all()
    assert np.isneginf(sc[:, 7 * pre + 1:]).all() and not bx[:, 7 * pre + 1:].any()       # the 1-anchor level: 699 unused rows


# ------------------------------------------------------------------------------------------------ decode
def test_apply_deltas64_against_the_float32_oracle_on_random_inputs():
    rng = np.random.default_rng(2)
    an = np.concatenate([rng.random((500, 2)) * 100, 120 + rng.random((500, 2)) * 100], 1).astype(np.float32)
    dl = (rng.standard_normal((500, 4)) * 0.5).astype(np.float32)
    for w in R.DEC_WEIGHTS:
        a, b = R.apply_deltas64(dl * np.asarray(w, np.float32), an, w), R.apply_deltas32(dl * np.asarray(w, np.float32), an, w)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max()


@pytest.mark.parametrize("weights", R.DEC_WEIGHTS)
def test_decode_case_reaches_its_edges_and_the_bar_excuses_few_rows(weights):
    c, e = R.decode_case(weights), R.decode_expected(weights)
    print(f"decode weights {weights}: float32 reference max error {e['e32']:.3g}, bar {e['bar']:.3g}")
    assert 0 < e["e32"] < 1e-2                                                            # a sane bar: boxes are up to a few thousand wide
    wv = np.asarray(weights, np.float32)
    d0 = c["deltas"][0][0]
    c32 = np.float32(R.SCALE_CLAMP)
    q = lambda row, col: np.float32(d0[row, col] / wv[col])
    n = R.DEC_NAMED
    assert q(n["dw_eq"], 2) == c32 and q(n["dw_above"], 2) > c32 and q(n["dw_below"], 2) < c32 and q(n["dh_eq"], 3) == c32 and q(n["dh_above"], 3) > c32
    b32 = R.apply_deltas32(d0, c["anchors"][0], weights)
    H, W = R.DEC_HW
    assert b32[n["zero_w_left"], 2] == 0 and b32[n["zero_w_right"], 0] == W and (b32[n["outside"], :2] > [W, H]).all()
    assert b32[n["dw_eq"], 2] - b32[n["dw_eq"], 0] == b32[n["dw_above"], 2] - b32[n["dw_above"], 0] > b32[n["dw_below"], 2] - b32[n["dw_below"], 0]
    assert e["finite"].tolist() == [1, 0]
    img, l, row = R.DEC_INF_ROW
    assert np.isinf(c["deltas"][l][img, row, 0]) and sum(int(np.isinf(d).sum()) for d in c["deltas"]) == 1
    over = np.concatenate([(d[..., 2:] / wv[2:] > c32).ravel() for d in c["deltas"]])
    assert 0.02 < over.mean() < 0.5
    sure = np.concatenate([s for lv in e["sure"] for s in lv]); keep = np.concatenate([k for lv in e["keep"] for k in lv])
    assert (~sure).mean() <= 0.02                                                         # the cap of the issue, for the chosen seed
    assert 0.02 < (~keep).mean() < 0.5 and len({len(np.unique(lg)) == lg.size for lg in c["logits"]}) == 1


# ------------------------------------------------------------------------------------------------ anchor labels
def test_exact_iou_ladder_and_the_matcher_rules_the_label_cases_name():
    an = R.label_anchors(3073)
    pos = R.special_positions(3073)
    assert {0, 1023, 1024, 3072} <= set(pos) and len(pos) == 9
    iou = FO.O.pairwise_iou(R.G0[None], an)[0]
    for j, m in enumerate(R.SPECIAL_M):
        assert iou[pos[j]] == np.float32(m / 100.0) == np.float32(m) / np.float32(100)
    assert iou[pos[0]] == np.float32(0.7) and iou[pos[1]] == np.float32(0.3)
    gt = R.label_gt("thr", 3073)
    lab = R.matcher_labels(an, gt)
    by_m = {m: int(lab[pos[j]]) for j, m in enumerate(R.SPECIAL_M)}
    assert by_m == {70: 1, 30: -1, 100: 1, 71: 1, 69: -1, 31: -1, 29: 0, 1: 0}            # == 0.7 -> 1, == 0.3 -> -1 (not 0)
    m, _ = FO.matcher(FO.O.pairwise_iou(gt, an), (0.3, 0.7), (0, -1, 1), True)
    split = pos[len(R.SPECIAL_M)]
    assert np.array_equal(gt[m[split]], R.SPLIT_GT[0]) and FO.O.pairwise_iou(R.SPLIT_GT, an[split:split + 1])[:, 0].tolist() == [0.5, 0.5]
    far = R.matcher_labels(an, R.label_gt("far_only", 3073))
    assert (far == 1).all()                                                               # best IoU 0: every zero-IoU anchor is positive
    assert (R.matcher_labels(an, R.label_gt("far", 3073)) == 1).all()                     # ... the ladder's anchors too: none overlaps it
    assert (R.matcher_labels(R.label_anchors(1025), R.label_gt("exact5", 1025)) == 1).sum() == 5


def test_label_cases_reach_every_sampling_count_edge():
    seen = set()
    assert {c[1] for c in R.LABEL_CASES} >= {1, 1023, 1024, 1025, 3 * 1024 + 1}
    for case in R.LABEL_CASES:
        name, A, kinds, batch, max_pos = case
        an, gts, seeds, labels, matched = R.label_expected(case)
        assert len(seeds) == 2 * len(kinds) and np.array_equal(an, np.round(an))
        for i, g in enumerate(gts):
            pre = R.matcher_labels(an, g)
            npos, nneg = int((pre == 1).sum()), int((pre == 0).sum())
            got_pos, got_neg = int((labels[i] == 1).sum()), int((labels[i] == 0).sum())
            assert got_pos == min(npos, max_pos) and got_neg == min(nneg, batch - got_pos)
            seen |= {("pos>cap", npos > max_pos > 0), ("pos==cap", npos == max_pos > 0), ("pos0", npos == 0), ("neg_short", nneg < batch - got_pos),
                     ("all_taken", A < batch and max_pos >= npos), ("cap0", max_pos == 0 and npos > 0), ("G0", len(g) == 0),
                     ("neg_sampled", nneg > batch - got_pos)}
            if len(g) == 0:
                assert not matched[i].any()
    assert all((k, True) in seen for k in ("pos>cap", "pos==cap", "pos0", "neg_short", "all_taken", "cap0", "G0", "neg_sampled"))
    assert any(len(c[2]) > R.LABEL_MAX_IMG for c in R.LABEL_CASES) and any(all(k == "none" for k in c[2]) for c in R.LABEL_CASES)


# ------------------------------------------------------------------------------------------------ ROI sampling
def test_roi_cases_reach_the_count_matching_and_image_edges():
    ns = set()
    for case in R.ROI_CASES + [R.ROI_REFUSED]:
        name, imgs, p_stride, append, batch, max_pos = case
        props, gts, seeds, want = R.roi_expected(case)
        for (p, G, mode), pb, (gb, gc), w in zip(imgs, props, gts, want):
            assert len(pb) == p <= p_stride and np.array_equal(pb, np.round(pb))           # no p_cnt above p_stride, integer boxes
            n = p + (len(gb) if append else 0)
            ns.add(n)
            assert n <= R.ROI_CAP and len(w["sampled_idx"]) <= batch
            fg = w["gt_classes"] != R.ROI_K
            assert fg.sum() <= max_pos and (w["gt_classes"] >= 0).all()
    assert {0, 1023, 1024, 1025, 2048, 2049, 4096} <= ns
    by = {c[0]: c for c in R.ROI_CASES}
    assert max(c[2] + max(g for _, g, _ in c[1]) for c in R.ROI_CASES if c[3]) == R.ROI_CAP
    assert R.ROI_REFUSED[2] + R.ROI_REFUSED[1][0][1] == R.ROI_CAP + 1
    w = R.roi_expected(by["empty_everything"])[3]
    assert len(w[0]["sampled_idx"]) == 0 and len(w[1]["sampled_idx"]) == 5
    w = R.roi_expected(by["empty_props_gt_appended"])[3]
    assert [len(x["sampled_idx"]) for x in w] == [3, 1] and all((x["gt_classes"] != R.ROI_K).all() for x in w)
    w = R.roi_expected(by["all_foreground"])[3][0]
    assert len(w["sampled_idx"]) == 128 and (w["gt_classes"] != R.ROI_K).all()             # a short batch: no background to fill with
    for nm in ("no_foreground", "no_gt_append_on"):
        w = R.roi_expected(by[nm])[3][0]
        assert (w["gt_classes"] == R.ROI_K).all() and len(w["sampled_idx"]) == 300
    assert len(by["images65"][1]) == R.ROI_MAX_IMG + 1 and {g for _, g, _ in by["images65"][1]} == {0, 1, 2}
    # IoU == 0.5 exactly is foreground, 0.49 background (matcher.py: thresholds are inclusive below)
    props, gts, _, want = R.roi_expected(by["n1025"])
    pb, (gb, gc) = props[0], gts[0]
    iou = FO.O.pairwise_iou(gb, pb).max(0)
    assert (iou == np.float32(0.5)).sum() > 50 and (iou == np.float32(0.49)).sum() > 50
    m, lab = FO.matcher(FO.O.pairwise_iou(gb, pb), (0.5,), (0, 1), False)
    assert (lab[iou == np.float32(0.5)] == 1).all() and (lab[iou == np.float32(0.49)] == 0).all()
    # the split proposal takes the FIRST of its two equally good boxes
    props, gts, _, want = R.roi_expected(by["split_pair"])
    row = by["split_pair"][1][0][0] // 2
    at = int(np.nonzero(want[0]["sampled_idx"] == row)[0][0])
    assert want[0]["gt_classes"][at] == gts[0][1][0] and np.array_equal(want[0]["gt_boxes"][at], R.SPLIT_GT[0])


# ------------------------------------------------------------------------------------------------ FPN levels
def test_level_reference_against_torch_on_random_boxes():
    b = R.level_case(2049)[0]
    ok = R.level_case(2049)[1] != 4
    t = torch.from_numpy(b[ok])
    want = torch.clamp(torch.floor(4 + torch.log2(torch.sqrt((t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])) / 224 + 1e-8)), 2, 5).long() - 2
    got = FO.assign_levels(b[ok])
    diff = got != want.numpy()
    assert not (diff & ~R.near_level_edge(b[ok])).any()
    v = R.level_value64(b[ok])
    far = ~R.near_level_edge(b[ok])
    assert np.array_equal(np.clip(np.floor(v[far]), 2, 5).astype(np.int64) - 2, got[far])


def test_level_edges_are_exact_and_the_excusable_rows_are_exactly_the_named_neighbours():
    assert np.array_equal(FO.assign_levels(R.LEVEL_EDGES), R.LEVEL_EDGE_WANT)              # exact powers of two: no allowance
    assert np.array_equal(FO.assign_levels(R.LEVEL_ODD), R.LEVEL_ODD_WANT)
    e = R.LEVEL_EDGES
    size = np.sqrt(((e[:, 2] - e[:, 0]) * (e[:, 3] - e[:, 1])).astype(np.float32))
    assert set(size.tolist()) == {112.0, 224.0, 448.0} and (e[:, 2] - e[:, 0] != e[:, 3] - e[:, 1]).sum() == 7
    assert np.isnan(R.level_value64(R.LEVEL_NEGATIVE)).all()
    assert (np.abs(R.LEVEL_NEIGHBOURS[:, 2] - R.LEVEL_NEIGHBOURS[:, 3]) > 0).all()
    assert {R.LEVEL_ODD[2, 2], R.LEVEL_ODD[3, 2]} == {np.float32(1e-3), np.float32(1e4)}
    for Rn in R.LEVEL_R:
        boxes, kind, row_cnt = R.level_case(Rn)
        assert len(boxes) == Rn == sum(row_cnt) and row_cnt[1] == 0
        near = R.near_level_edge(boxes)
        assert np.array_equal(near, (kind == 1) | (kind == 2))                            # within 1e-6 of an integer: edges + neighbours only
        excusable = near & (kind != 1)                                                    # ... and the edges themselves must match exactly
        assert np.array_equal(excusable, kind == 2)
        if Rn > 1:
            assert {1, 2, 3, 4} <= set(kind.tolist()) and kind[[0, Rn - 1]].all() and set(R.level_expected(boxes, kind).tolist()) == {0, 1, 2, 3}
        if Rn > 1024:
            assert kind[[1022, 1023, 1024]].all()
    assert set(R.LEVEL_R) == {1, 1023, 1024, 1025, 2049}
    assert set(FO.assign_levels(R.small_boxes(1500)).tolist()) == {0}


if __name__ == "__main__":
    for w in R.DEC_WEIGHTS:
        e = R.decode_expected(w)
        print(f"decode weights {w}: e32 {e['e32']:.4g} bar {e['bar']:.4g} excused {np.mean(~np.concatenate([s for lv in e['sure'] for s in lv])):.4f}")

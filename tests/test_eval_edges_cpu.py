"""CPU: the cases of eval_edge_cases.py reach the edges of the evaluation kernels they are named for (asserted from the
restatements and the host-side layout, nothing from the kernels), and each is sensitive: a restatement that is wrong on purpose
in one rule changes at least one output bit on the case meant to catch that rule.  test_gpu_eval_edges.py runs the kernels on
the same cases."""
import numpy as np
import pytest

import coco_eval_fixture as CF
import eval_edge_cases as C
import voc_eval_fixture as VF
from test_coco_eval_cpu import _same

THR = [t / 100.0 for t in range(50, 100, 5)]


def _bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


# ---- VOC ----------------------------------------------------------------------------------------------------------------------

def test_voc_tile_split_sits_on_the_tile_and_grid_edges():
    objs, dets, K = C.voc_tile_split()
    detail = C.voc_restated("tile")[3]
    assert K == 13 and [len(d["order"]) for d in detail] == list(C.TILE_ND)
    assert [n for n in C.TILE_ND if n] == [1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]
    assert [c for c, n in enumerate(C.TILE_ND) if n == 0] == [0, 6, 12]          # empty at the front, in the middle, at the end
    # the match kernel's grid: the split ends inside a workgroup; classes start on a workgroup's first lane (1 + 255 = 256) and
    # inside one, and the empty classes share their neighbour's offset
    off = np.cumsum((0,) + C.TILE_ND)
    assert off[-1] == 9985 and off[-1] % C.VOC_LANES != 0 and off[3] == 256 and off[4] == 512 and off[5] % C.VOC_LANES == 1
    assert off[0] == off[1] and off[6] == off[7] and off[12] == off[13]
    for c, nd in enumerate(C.TILE_ND):
        d = detail[c]
        if nd == 0:
            continue
        rank = np.arange(nd)
        kinds = {"difficult": 0, "duplicate": 0, "miss": 0, "no_object": int(np.isinf(d["ovmax"]).sum())}
        for t in range(10):
            tp, fp = d["tp"][t] > 0, d["fp"][t] > 0
            kinds["difficult"] += int((~tp & ~fp).sum())
            kinds["duplicate"] += int((fp & (d["ovmax"] > THR[t])).sum())
            kinds["miss"] += int((fp & ~(d["ovmax"] > THR[t]) & np.isfinite(d["ovmax"])).sum())
            # pass 1 tiles the ranks forward, pass 2 the sentinel-extended arrays backward (rank d is item nd - d); a tile of one
            # detection cannot hold both kinds, every larger one holds a true and a false positive
            for tile in (rank // C.VOC_TILE, (nd - rank) // C.VOC_TILE):
                for k in np.unique(tile):
                    sel = tile == k
                    if sel.sum() >= 2:
                        assert tp[sel].any() and fp[sel].any(), (c, t, int(k))
            if nd >= 255:                             # the precision curve goes down and up again: the envelope has work to do
                ctp, cfp = np.cumsum(tp), np.cumsum(fp)
                prec = ctp / np.maximum(ctp + cfp, 1)
                assert (np.diff(prec) > 0).any() and (np.diff(prec) < 0).any(), (c, t)
        if nd >= 255:
            assert all(v > 0 for v in kinds.values()), (c, kinds)
    assert len(detail[6]["order"]) == 0 and any(o[0] == 6 for im in objs for o in im)


@pytest.mark.parametrize("call", range(len(C.SUM_TERMS)))
def test_voc_sum_split_term_counts_and_summation_order(call):
    detail = C.voc_restated("sum", call)[3]
    ap_area = C.voc_restated("sum", call)[1]
    for c, n in enumerate(C.SUM_TERMS[call]):
        terms = detail[c]["terms"]
        assert all(len(t) == n for t in terms), (n, [len(t) for t in terms])                      # (a)
        t0 = terms[0]
        assert _bits(np.sum(t0) * 100) == _bits(ap_area[c, 0])
        # the spelled-out order (chunks of 8192, pairwise blocks, leaves of 128, eight accumulators) is np.sum's
        assert _bits(VF.pairwise_sum(t0)) == _bits(np.sum(t0)), n
        if n >= 129:                                                                              # (b)
            assert _bits(VF.sequential_sum(t0)) != _bits(np.sum(t0)), n
        if n > 8192:                                                                              # (c)
            assert _bits(VF.pairwise_sum(t0, chunk=None)) != _bits(np.sum(t0)), n
        # the closing sentinel adds the last term exactly when recall ends below 1
        tp = detail[c]["tp"][0].sum()
        assert n == tp + (c % 2), (n, tp)
    assert sorted(n for ns in C.SUM_TERMS for n in ns) == [7, 8, 9, 127, 128, 129, 136, 8191, 8192, 8193, 16389]


def test_voc_tie_split_arithmetic_is_exact():
    a07, area, cl, d = C.voc_restated("ties", "ties")
    # class 0: IoU exactly on the thresholds 0.5 and 0.75 is no match
    assert d[0]["ovmax"].tolist() == [0.5, 0.75, 1.0, 1.0] and THR[0] == 0.5 and THR[5] == 0.75
    assert d[0]["tp"][0].tolist() == [0, 1, 1, 0] and d[0]["fp"][0].tolist() == [1, 0, 0, 1]
    assert d[0]["tp"][5].tolist() == [0, 0, 1, 0] and d[0]["tp"][4].tolist() == [0, 1, 1, 0]
    # class 1: two objects at the same IoU, the first wins: difficult in image 3 (neither TP nor FP), plain in image 4
    assert d[1]["order"].tolist() == [0, 2, 1] and d[1]["ovmax"][0] == d[1]["ovmax"][2] == 90.0 / 110.0
    assert d[1]["jmax"].tolist() == [0, 0, 0] and d[1]["img"].tolist() == [3, 3, 4]
    assert (d[1]["tp"][0] + d[1]["fp"][0]).tolist() == [0, 1, 1] and d[1]["tp"][0].tolist() == [0, 0, 1]
    # class 2: equal scores rank in line order; the earlier line is the TP at every threshold, the later one a duplicate up to 0.85
    assert d[2]["order"].tolist() == [0, 1, 2] and d[2]["ovmax"].tolist()[:2] == [1.0, 0.9] and THR[8] == 0.9
    assert all(d[2]["tp"][t].tolist() == [1, 0, 0] for t in range(10))
    # class 3: the best match is difficult: the detection counts as nothing although a plain object overlaps it by 0.6
    assert d[3]["jmax"][0] == 0 and d[3]["ovmax"][0] == 1.0 and d[3]["tp"][0][0] == 0 and d[3]["fp"][0][0] == 0
    # class 4: image 7 holds only a difficult object and gets no CorLoc slot
    assert sorted(d[4]["holder"]) == [8] and cl[4].tolist() == [100.0] * 6 + [0.0] * 4
    # class 5: the NaN detection ranks first, is a false positive and holds the image's CorLoc slot
    assert np.isnan(d[5]["ovmax"][0]) and d[5]["fp"][0].tolist() == [1, 0] and (cl[5] == 0).all() and (area[5] == 50).all()
    # class 6: x2 < x1 with area -100 against an object of area 100: 0 / 0
    assert np.isnan(d[6]["ovmax"][0]) and d[6]["ovmax"][2] == 0.0 and d[6]["tp"][9].tolist() == [0, 1, 0]
    a07, area, cl, d = C.voc_restated("ties", "npos0")
    assert cl is None and np.isnan(area[1]).all() and (a07[1] == 0).all() and len(d[1]["order"]) == 3 and (area[0] == 100).all()
    objs, dets, K = C.voc_case("ties", "one_image")
    assert len(objs) == 1
    a07, area, cl, d = C.voc_restated("ties", "one_image")
    assert cl[0].tolist() == [100.0] * 6 + [0.0] * 4 and d[1]["order"].tolist() == [0, 1]


def test_voc_contention_split_has_one_winner_per_threshold():
    a07, area, cl, d = C.voc_restated("contention")
    d = d[0]
    n = C.CONTENTION_DETS
    assert len(d["order"]) == n and -(-n // C.VOC_LANES) == 12
    assert not np.array_equal(d["order"], np.arange(n))                           # line order is not rank order
    winners = []
    for t in range(10):
        passing = np.flatnonzero(d["ovmax"] > THR[t])
        groups = np.unique(passing // C.VOC_LANES)    # the workgroups whose lanes take part in the claim
        assert len(passing) > 12 and len(groups) == (12 if t < 4 else 10), (t, groups)
        assert np.flatnonzero(d["tp"][t]).tolist() == [passing[0]]                # the best-ranked one holds it, alone
        assert d["fp"][t].sum() == n - 1
        winners.append(int(passing[0]))
    assert len({w // C.VOC_LANES for w in winners}) >= 2 and winners[0] < C.VOC_LANES <= 600 <= winners[-1]
    # CorLoc reads rank 0, which is below 0.7, not the winners
    assert d["holder"] == {0: 0} and cl[0].tolist() == [100.0 * bool(d["ovmax"][0] > th) for th in THR] and cl[0, 0] != cl[0, 9]


@pytest.mark.parametrize("variant,case", [("ge", ("ties", "ties")), ("last_max", ("ties", "ties")),
                                          ("reversed_ties", ("ties", "ties")), ("sequential_sum", ("sum", 0))])
def test_voc_cases_notice_a_wrong_rule(variant, case):
    objs, dets, K = C.voc_case(*case)
    right = C.voc_restated(*case)
    wrong = VF.restated(objs, len(objs), dets, K, variant=variant)
    changed = [k for k in range(3) if not _same(right[k], wrong[k])]
    assert changed, variant
    cls = {"ge": 0, "last_max": 1, "reversed_ties": 2}.get(variant)
    if cls is not None:                               # the class built for the rule is among those that move
        assert not _same(right[1][cls], wrong[1][cls]) or not _same(right[2][cls], wrong[2][cls])
    else:
        moved = [c for c in range(K) if not _same(right[1][c], wrong[1][c])]
        assert set(moved) >= {c for c, n in enumerate(C.SUM_TERMS[0]) if n >= 129} and 0 not in moved, moved   # 7 terms: one order


# ---- COCO ---------------------------------------------------------------------------------------------------------------------

def _layout(ds, res, cap=1600):
    from sos_wsod_amd import evaluation as E
    gt = E.COCOGroundTruth(ds)
    return gt, E.coco_eval_layout(gt, E.COCODetections.from_results(res, gt), lds_doubles=cap)


def _pair_shapes(gt, L):
    K = len(gt.cat_ids)
    key = [(gt.img_ids[int(g) // K], gt.cat_ids[int(g) % K]) for g in L["pair_gt"]]
    D = np.diff(L["pair_off"])
    G = L["gt_off"][L["pair_gt"] + 1] - L["gt_off"][L["pair_gt"]]
    return key, D.tolist(), G.tolist()


# (D, G) -> (path, words of a walk's bitmask) at lds_doubles = 1600
SHAPE_PATHS = {(1, 1): ("lds", 1), (100, 16): ("lds", 1), (100, 17): ("ws", 1), (25, 64): ("lds", 1), (25, 65): ("ws", 2),
               (1, 64): ("lds", 1), (1, 65): ("ws", 2), (3, 128): ("ws", 2), (3, 129): ("ws", 3), (100, 200): ("ws", 4),
               (5, 0): ("lds", 0)}


def test_coco_shape_split_path_of_every_pair():
    from sos_wsod_amd import evaluation as E
    ds, res, shape_of = C.coco_shape_split()
    assert sorted(shape_of.values()) == sorted(SHAPE_PATHS) == sorted((D, G) for D, G, _ in C.COCO_SHAPES)
    for cap in (1600, 64, 0):
        gt, L = _layout(ds, res, cap)
        key, D, G = _pair_shapes(gt, L)
        assert len(key) == len(C.COCO_SHAPES) and 90 in gt.cat_ids and all(c != 90 for _, c in key)
        used = 0
        for p, k in enumerate(key):
            assert (D[p], G[p]) == shape_of[k]
            words = int(E.coco_pair_workspace_words(D[p], G[p], cap))
            fits = G[p] <= 64 and D[p] * G[p] <= cap
            if cap == 1600:
                path, W = SHAPE_PATHS[D[p], G[p]]
                assert fits == (path == "lds") and (G[p] + 63) // 64 == W, k
            assert (words == 0) == fits and (L["pair_ws"][p] == -1) == fits, (k, cap)
            if not fits:
                assert L["pair_ws"][p] == used and words == D[p] * G[p] + 40 * ((G[p] + 63) // 64) + 2 * G[p]
                used += words
        assert L["ws_words"] == used
    assert 100 * 16 == 1600 and shape_of[100 - 3 * 2, 2 + 2 * 2] == (100, 17)     # G <= 64, in the workspace only for D * G


def test_coco_shape_split_contents():
    ds, res, shape_of = C.coco_shape_split()
    ev, pairs = C.coco_restated("shapes")
    gts, dts = CF.prepare(ds, res)[2:]
    assert set(pairs) == set(shape_of)
    n_half = n_dup = n_crowd_only = 0
    for s, (D, G, crowd) in enumerate(C.COCO_SHAPES):
        key = (100 - 3 * s, 2 + 2 * s)
        gt, dt, rec = gts[key], dts[key], pairs[key]
        flags = [g["iscrowd"] for g in gt]
        assert {"none": not any(flags), "some": 0 < sum(flags) < max(G, 1), "all": all(flags) and G > 0}[crowd], key
        if crowd == "all":                            # nvalid == 0 in every area range
            assert all(all(ig) for ig in rec["gt_ignored"]) and rec["ignored"].all()
        ious = np.asarray(CF.compute_iou(gt, dt)).reshape(len(dt), len(gt))
        n_half += int((ious == 0.5).sum())
        if G:
            plain = np.asarray(flags) == 0
            n_dup += int(((ious[:, plain] == 1.0).sum(0) >= 2).sum())
            n_crowd_only += int(((ious[:, ~plain] > 0).any(1) & ~(ious[:, plain] > 0).any(1)).sum())
        assert len(dt) == D and len(gt) == G
        if G >= 17:                                   # objects of all four ranges and on both range edges
            areas = {g["area"] for g in gt if not g["iscrowd"]} if crowd != "all" else {g["area"] for g in gt}
            assert 32.0 ** 2 in areas and 96.0 ** 2 in areas and min(areas) < 1024 and max(areas) > 9216, key
            per_range = [[not ig for ig in rec["gt_ignored"][a]] for a in range(4)]
            if crowd != "all":
                assert all(any(v) for v in per_range) and not all(per_range[1]) and not all(per_range[3])
        if G >= 2 and crowd != "all":
            # the area cluster: in the medium range the cluster's detection holds the plain medium object and stops at the
            # ignored small one of IoU 1; without the stop it would take that one and be ignored
            wrong = CF.pair_matches({**ds, "annotations": [a for a in ds["annotations"] if a["image_id"] == key[0]]},
                                    [r for r in res if r["image_id"] == key[0]], variant="no_break")[key]
            assert (wrong["ignored"][2] & ~rec["ignored"][2]).any(), key
    assert n_half >= 6 and n_dup >= 4 and n_crowd_only >= 4
    assert any(a["id"] == 0 for a in ds["annotations"])
    # bits the accumulated arrays cannot see: ignored detections, and whole area ranges without a non-ignored object
    npig0 = [(key, a) for key, rec in pairs.items() for a in range(4) if all(rec["gt_ignored"][a])]
    assert len(npig0) >= 6 and any(pairs[key]["matched"][a].any() for key, a in npig0)
    assert any((rec["ignored"] & rec["matched"]).any() for rec in pairs.values())


@pytest.mark.parametrize("name,arg", [("shapes", None), ("accum", None), ("count", 1), ("count", 2), ("count", 3), ("count", 4),
                                      ("count", 5), ("trivial", 41)])
def test_coco_expected_match_words_follow_the_layout_order(name, arg):
    ds, res = C.coco_case(name, arg)
    ev, pairs = C.coco_restated(name, arg)
    gt, L = _layout(ds, res)
    words = C.coco_expected_words(L, gt.img_ids, gt.cat_ids, pairs)
    assert words.shape == (len(L["det_score"]), 2) and (words >= 0).all() and (words < (1 << 40)).all()
    assert (words[:, 0] != 0).any() and (words[:, 1] != 0).any()
    if name == "count":
        key, D, G = _pair_shapes(gt, L)
        assert len(key) == arg and list(zip(D, G)) == [s[:2] for s in C.COUNT_SHAPES[:arg]]
    if name == "trivial":
        key, D, G = _pair_shapes(gt, L)
        assert len(key) == arg and set(D) == {1} and set(G) == {1}
        assert len(np.unique(ev["precision"][:, :, 0, 0, 2])) > 2


def test_coco_accum_split_sits_on_the_tile_edges():
    ds, res = C.coco_accum_split()
    ev, pairs = C.coco_restated("accum")
    gt, L = _layout(ds, res)
    assert np.diff(L["cat_off"]).tolist() == [n for n, _, _ in C.ACCUM_CATS] == [1023, 1024, 1025, 2048, 2049, 1030]
    assert L["npig"][:, 0].tolist() == [g for _, g, _ in C.ACCUM_CATS] == [1, 3, 100, 101, 100, 3]
    assert len(res) > len(L["det_score"])                                          # the cut at 100 per pair took some away
    words = C.coco_expected_words(L, gt.img_ids, gt.cat_ids, pairs)
    for k, (n, npig, all_fp) in enumerate(C.ACCUM_CATS):
        lo, hi = L["cat_off"][k], L["cat_off"][k + 1]
        rank, score = L["det_rank"][lo:hi], L["det_score"][lo:hi]
        assert (rank == 0).any() and ((rank >= 1) & (rank <= 9)).any() and (rank >= 10).any() and rank.max() == 99
        # equal scores in different images: the category's list keeps them in layout order
        listed = L["order"][lo:hi]
        s = L["det_score"][listed]
        img = np.searchsorted(L["pair_off"], listed, side="right")
        tie = s[1:] == s[:-1]
        assert (np.diff(s) <= 0).all() and (tie & (img[1:] != img[:-1])).sum() > 50 and (np.diff(listed)[tie] > 0).all()
        matched, ignored = words[lo:hi, 0] & 1, words[lo:hi, 1] & 1              # area "all", IoU 0.5
        assert ignored.any() and (words[lo:hi, 1] & (1 << 10)).any()
        if all_fp:
            assert not (words[lo:hi, 0] & ~words[lo:hi, 1]).any() and (ev["recall"][:, k, 0] == 0).all()
            assert (ev["precision"][:, :, k, 0] == 0).all()
        else:
            assert (matched & ~ignored).any()
            p = ev["precision"][:, :, k, 0]
            # the three maxDets give three curves; a single true positive of high score sees the same false positives before it
            # at 10 and at 100 per image, so there only the first and the last are told apart
            assert not np.array_equal(p[..., 0], p[..., 2]), k
            if npig > 1:
                assert not np.array_equal(p[..., 0], p[..., 1]) and not np.array_equal(p[..., 1], p[..., 2]), k
    # tp / npig on the recall levels and between them
    # tp / npig lands on recall levels (k / 100 is the level for most k), one bit beside them (np.linspace's 0.35 and nine more
    # are not k / 100), and between them (thirds, k / 101)
    off = [k for k in range(101) if CF.REC_THRS[k] != k / 100]
    assert off == [35, 41, 47, 57, 69, 70, 82, 83, 94, 95] and 1 / 3 not in CF.REC_THRS and 50 / 101 not in CF.REC_THRS
    for k, (n, npig, all_fp) in enumerate(C.ACCUM_CATS[:5]):                     # the true positives reach past those levels
        r1, r100 = ev["recall"][0, k, 0, 0], ev["recall"][0, k, 0, 2]
        assert r100 * npig >= min(npig, 96) and (npig == 1 or 0 < r1 < r100), k


@pytest.mark.parametrize("variant", CF.VARIANTS)
def test_coco_shape_split_notices_a_wrong_rule(variant):
    ds, res, _ = C.coco_shape_split()
    right, pairs = C.coco_restated("shapes")
    wrong_pairs = {}
    wrong = CF.restated(ds, res, variant=variant, pairs=wrong_pairs)
    assert any(not _same(right[k], wrong[k]) for k in ("precision", "recall", "scores")), variant
    gt, L = _layout(ds, res)
    a, b = (C.coco_expected_words(L, gt.img_ids, gt.cat_ids, p) for p in (pairs, wrong_pairs))
    assert not np.array_equal(a, b), variant


def test_coco_refusal_layout_is_one_detection_past_the_limit():
    from sos_wsod_amd._lib import lib
    for D, ok in ((256, False), (255, True)):
        L = C.coco_refusal_layout(D)
        assert np.diff(L["pair_off"]).tolist() == [D] and len(L["det_score"]) == D and L["det_rank"].tolist() == list(range(D))
        assert lib.sw_coco_eval_workspace_bytes(D, 1, 1600) == (0 if ok else -1)
        assert (np.diff(L["det_score"]) < 0).all() and CF.bb_iou(L["det_box"][0], L["gt_box"][0], False) == 1.0

"""GPU: the VOC and COCO evaluation kernels (csrc/evaluation.hip: voc_match_kernel, voc_ap_kernel, coco_match_kernel,
coco_accum_kernel) on the cases of eval_edge_cases.py, which sit on the kernels' tile, chunk, path and tie edges
(test_eval_edges_cpu.py asserts that they do, and that each notices a wrong rule).  Everything is compared bit for bit with the
float64 restatements (voc_eval_fixture.restated_detail, coco_eval_fixture.restated); COCO also compares the per-detection match
words, all 40 bits of both, with what evaluate_pair decides."""
import numpy as np
import pytest
import torch

import eval_edge_cases as C
from test_coco_eval_cpu import _same
from test_gpu_coco_eval import _call_ops

pytestmark = pytest.mark.gpu


# ---- VOC ----------------------------------------------------------------------------------------------------------------------

def _check_voc(name, call=None):
    from sos_wsod_amd import evaluation as E
    import voc_eval_fixture as F
    objs, dets, K = C.voc_case(name, call)
    a07, area, cl, _ = C.voc_restated(name, call)
    names = [f"{i:06d}" for i in range(len(objs))]
    recs = {n: [{"name": F.CLASS_NAMES[c], "pose": "Unspecified", "truncated": 0, "difficult": d, "bbox": b} for c, b, d in o]
            for n, o in zip(names, objs)}
    gt = E.GroundTruth(names, recs, F.CLASS_NAMES[:K])
    res = E.voc_eval_arrays(gt, E.Detections(dets), corloc=cl is not None)
    print(name, call, "ap_area", res["ap_area"][:, 0].tolist(), "restated", area[:, 0].tolist())
    assert _same(res["ap_07"], a07), np.argwhere(res["ap_07"] != a07)
    assert _same(res["ap_area"], area), np.argwhere((res["ap_area"] != area) & ~(np.isnan(area) & np.isnan(res["ap_area"])))
    if cl is not None:
        assert _same(res["corloc"], cl), np.argwhere(res["corloc"] != cl)
    else:
        assert res["corloc"] is None
    return res


def test_voc_tile_and_grid_edges_with_empty_classes():
    """nd = 1, 255 .. 257, 1023 .. 1025, 2047 .. 2049 in one split whose classes 0, 6 and 12 are empty"""
    res = _check_voc("tile")
    assert (res["ap_area"][[0, 6, 12]] == 0).all() and (res["ap_area"][[2, 5, 7, 8, 11], 0] > 0).all()


@pytest.mark.parametrize("call", range(len(C.SUM_TERMS)))
def test_voc_area_sum_in_numpy_order(call):
    """7, 8, 9, 127, 128, 129, 136 / 8191, 8192 / 8193, 16389 summed terms: any other order changes a bit (asserted on the CPU)"""
    _check_voc("sum", call)


@pytest.mark.parametrize("split", ["ties", "npos0", "one_image"])
def test_voc_ties_and_special_values(split):
    _check_voc("ties", split)


def test_voc_claim_contention_across_workgroups():
    """3000 detections in 12 workgroups claim one object: the best-ranked one above each threshold holds it"""
    _check_voc("contention")


# ---- COCO ---------------------------------------------------------------------------------------------------------------------

def _check_coco(name, arg=None, cap=1600):
    """the product path and a direct ops.coco_eval call with the match words kept, both against the restatement"""
    from sos_wsod_amd import evaluation as E
    ds, res = C.coco_case(name, arg)
    want, pairs = C.coco_restated(name, arg)
    gt = E.COCOGroundTruth(ds)
    dets = E.COCODetections.from_results(res, gt)
    got = E.coco_eval_arrays(gt, dets, lds_doubles=cap)
    for k in ("precision", "recall", "scores"):
        assert _same(got[k], want[k]), (name, arg, cap, k, np.argwhere(got[k] != want[k])[:5])
    L = E.coco_eval_layout(gt, dets, lds_doubles=cap)
    N, pad = len(L["det_score"]), 64
    match_buf = torch.full((N + 2 * pad, 2), -1, device="cuda", dtype=torch.int64)
    out, _ = _call_ops(L, cap, match=match_buf[pad:pad + N])
    host = out.cpu().numpy()
    n = int(np.prod(want["counts"]))
    assert _same(host[:n].reshape(want["counts"]), want["precision"]) and _same(host[n:2 * n].reshape(want["counts"]), want["scores"])
    assert _same(host[2 * n:].reshape(want["recall"].shape), want["recall"])
    words = match_buf.cpu().numpy()
    assert (words[:pad] == -1).all() and (words[pad + N:] == -1).all()
    expect = C.coco_expected_words(L, gt.img_ids, gt.cat_ids, pairs)
    bad = np.argwhere(words[pad:pad + N] != expect)
    assert len(bad) == 0, (name, arg, cap, bad[:5], [(hex(words[pad + d, w]), hex(expect[d, w])) for d, w in bad[:5]])
    return L


@pytest.mark.parametrize("cap", [1600, 64, 0])
def test_coco_pair_shapes_on_every_path(cap):
    """(D, G) on both sides of D * G == 1600, G == 64, 128: LDS and workspace with one to four bitmask words; lds_doubles 64 and 0
    move pairs to the workspace and change nothing"""
    from sos_wsod_amd import evaluation as E
    L = _check_coco("shapes", cap=cap)
    D, G = np.diff(L["pair_off"]), L["gt_off"][L["pair_gt"] + 1] - L["gt_off"][L["pair_gt"]]
    assert np.array_equal(L["pair_ws"] >= 0, E.coco_pair_workspace_words(D, G, cap) > 0)
    assert int((L["pair_ws"] >= 0).sum()) == {1600: 6, 64: 8, 0: 10}[cap]


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_coco_waves_without_a_pair(P):
    L = _check_coco("count", P)
    assert len(L["pair_gt"]) == P


def test_coco_more_pairs_than_one_grid_pass():
    """the match kernel's grid is capped at 8 workgroups of 4 waves per compute unit: more pairs than that stride the grid"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P = 32 * cus + 8
    L = _check_coco("trivial", P)
    assert len(L["pair_gt"]) == P and P > 32 * cus and (np.diff(L["pair_off"]) == 1).all()


def test_coco_accumulation_tile_edges():
    """category lists of 1023, 1024, 1025, 2048, 2049 detections, tied scores, ignored detections, one category without a TP"""
    L = _check_coco("accum")
    assert np.diff(L["cat_off"]).tolist() == [n for n, _, _ in C.ACCUM_CATS]


def test_coco_refuses_a_pair_of_256_detections():
    """a pair beyond SW_COCO_MAX_PAIR_DETS is not touched and the whole output is NaN; at 255 the same arrays evaluate"""
    pad = 64
    for D, refused in ((256, True), (255, False)):
        L = C.coco_refusal_layout(D)
        n_out = 2 * 10 * 101 * 12 + 10 * 12
        out_buf = torch.full((n_out + 2 * pad,), 7.0, device="cuda", dtype=torch.float64)
        match_buf = torch.full((D + 2 * pad, 2), -1, device="cuda", dtype=torch.int64)
        _call_ops(L, 1600, out=out_buf[pad:pad + n_out], match=match_buf[pad:pad + D])
        host, words = out_buf.cpu().numpy(), match_buf.cpu().numpy()
        assert (host[:pad] == 7.0).all() and (host[pad + n_out:] == 7.0).all()
        assert (words[:pad] == -1).all() and (words[pad + D:] == -1).all()
        inner = host[pad:pad + n_out]
        if refused:
            assert np.isnan(inner).all()
            assert (words[pad:pad + D] == -1).all()               # nothing of the pair was touched
        else:
            assert not np.isnan(inner).any() and (inner != 7.0).all()
            assert ((words[pad:pad + D] >= 0) & (words[pad:pad + D] < (1 << 40))).all()

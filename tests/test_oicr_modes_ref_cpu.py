"""CPU: the restatements of OICRPlusHeads' other mining rules (tests/oicr_modes_ref.py) reproduce the fixtures the reference wrote
(tests/golden/make_oicr_modes_golden.py), the reference's own float32 candidate boxes sit inside the decode bar, and the head builds
with either switch set."""
import numpy as np
import pytest

import oicr_modes_ref as M


@pytest.mark.parametrize("name", list(M.CASES))
def test_restatements_reproduce_the_reference_fixtures(name):
    g = M.load_case(name)
    _, refine_mist, bbox_update = M.CASES[name]
    assert bool(g["refine_mist"]) == refine_mist and bool(g["bbox_update"]) == bbox_update
    _, views, gt, _ = M.case_inputs(g)
    boxes, gt_int, K = views[0]["boxes"], np.unique(np.asarray(gt, np.int64)), int(g["K"])
    assert np.array_equal(gt_int, g["gt_int"])
    for k in range(4):
        cand = g[f"r{k}/cand_boxes"] if f"r{k}/cand_boxes" in g.files else None
        assert (cand is not None) == (bbox_update and k >= 1)
        p, l = M.mine_and_label(g[f"r{k}/scores"], boxes, gt_int, K, cand, 0 if refine_mist else 1)
        assert np.array_equal(p["index"], g[f"r{k}/pgt_index"]) and np.array_equal(p["classes"], g[f"r{k}/pgt_classes"])
        assert np.array_equal(p["scores"].view(np.int32), g[f"r{k}/pgt_scores"].view(np.int32))
        assert np.array_equal(p["boxes"].view(np.int32), g[f"r{k}/pgt_boxes"].view(np.int32))
        assert np.array_equal(l["gt_classes"], g[f"r{k}/gt_classes"]) and np.array_equal(l["gt_index"], g[f"r{k}/gt_index"])
        assert np.array_equal(l["gt_weights"].view(np.int32), g[f"r{k}/gt_weights"].view(np.int32))
        assert np.array_equal(l["gt_boxes"].view(np.int32), g[f"r{k}/gt_boxes"].view(np.int32))
        if not refine_mist:                                 # exactly one entry per image-level class, in class order
            assert np.array_equal(p["classes"], gt_int)
        if cand is not None:                                # the pseudo boxes are no longer proposal boxes
            assert not np.array_equal(p["boxes"], boxes[p["index"]])


@pytest.mark.parametrize("name", [n for n, c in M.CASES.items() if c[2]])
def test_reference_float32_decode_sits_inside_the_bar(name):
    """the candidate boxes the reference computed in float32 (from its own float32 deltas, which the fixture keeps) against the
    float64 decode of the same deltas: the bar the GPU decode is held to must hold the reference too, or the bar is wrong"""
    g = M.load_case(name)
    _, views, _, _ = M.case_inputs(g)
    boxes = views[0]["boxes"]
    worst = 0.0
    for k in range(1, 4):
        d = g[f"r{k}/deltas"]
        err = np.abs(g[f"r{k}/cand_boxes"].astype(np.float64) - M.decode(d, boxes))
        bar = M.decode_bar(d, boxes)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (k, float((err / bar).max()))
        assert float(bar.max()) <= float(g["bar_max"]) * (1 + 1e-12)      # the generator's margins were taken against this bar
        # and the float32 restatement of the decode is the reference's arithmetic: the same bits up to exp
        f32 = M.decode(d, boxes, dtype=np.float32)
        assert (np.abs(f32.astype(np.float64) - g[f"r{k}/cand_boxes"]) <= bar).all()
    print(f"{name}: the reference's float32 boxes use {worst:.3f} of the decode bar")
    assert M.iou_sensitivity(1.0) * float(g["bar_max"]) < 1.0


def test_decode_bar_scales_with_centre_and_size_not_with_the_cancelled_mean():
    """deltas that cancel exactly to +-0 still carry a bar from the terms that were added; a clamped dw stops growing the size"""
    boxes = np.array([[10.0, 20.0, 50.0, 100.0]], np.float32)
    d = np.zeros((4, 1, 1, 4), np.float32)
    d[0, ..., 0], d[1, ..., 0] = 3.0, 3.0                       # dx: 3 - 3 + 0 - 0
    d[:, ..., 2] = 100.0                                        # dw far beyond the clamp
    out = M.decode(d, boxes)
    assert out[0, 0, 2] - out[0, 0, 0] == pytest.approx(62.5 * 40.0)
    assert 0.5 * (out[0, 0, 0] + out[0, 0, 2]) == 30.0
    bar = M.decode_bar(d, boxes)
    assert (bar > 0).all() and bar[0, 0, 0] < 0.1 and bar[0, 0, 1] < 1e-3


def _cfg(extra):
    from sos_wsod_amd.config import add_wsl_config, get_cfg
    cfg = add_wsl_config(get_cfg())
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "MultiInputRCNN", "MODEL.BACKBONE.NAME",
                         "build_vgg_backbone", "MODEL.VGG.CONV5_DILATION", 2, "MODEL.ROI_HEADS.NAME", "OICRPlusHeads",
                         "MODEL.ROI_HEADS.IN_FEATURES", ["plain5"], "MODEL.ROI_HEADS.NUM_CLASSES", 20,
                         "MODEL.ROI_HEADS.IOU_THRESHOLDS", [0.5, 0.6], "MODEL.ROI_HEADS.IOU_LABELS", [0, -1, 1],
                         "MODEL.ROI_BOX_HEAD.NAME", "DiscriminativeAdaptionNeck", "MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIPool",
                         "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7, "MODEL.ROI_BOX_HEAD.DAN_DIM", [64, 64],
                         "MODEL.PROPOSAL_GENERATOR.NAME", "PrecomputedProposals", "WSL.REFINE_NUM", 4,
                         "WSL.REFINE_REG", [True] * 4] + extra)
    return cfg


@pytest.mark.parametrize("extra,mist,update", [(["OICRPLUS.BBOX_UPDATE", True, "WSL.REFINE_MIST", True], True, True),
                                               (["WSL.REFINE_MIST", False], False, False),
                                               ([], False, False),                       # a YAML that omits the key: the default
                                               (["OICRPLUS.BBOX_UPDATE", True], False, True)])
def test_from_config_builds_the_head_with_either_switch(extra, mist, update):
    from sos_wsod_amd.rcnn_multi import build_model
    heads = build_model(_cfg(extra)).roi_heads
    assert heads.refine_mist is mist and heads.bbox_update is update


def test_mist_type_wetectron_is_still_refused():
    from sos_wsod_amd.rcnn_multi import build_model
    with pytest.raises(AssertionError, match="get_pgt_mist_mist"):
        build_model(_cfg(["WSL.REFINE_MIST", True, "WSL.MIST_TYPE", "wetectron"]))


@pytest.mark.parametrize("name", list(M.EDGE_CASES))
def test_edge_cases_hold_what_they_are_built_for(name):
    c = M.edge_case(name)
    p, l = M.mine_and_label(c["scores"], c["boxes"], c["gt"], c["K"], c["cand"], c["seed_rule"])
    K = c["K"]
    if name.startswith("same_seed"):                       # every class seeds proposal 5; the lowest class id labels its neighbours
        assert set(p["index"].tolist()) == {5} and np.array_equal(p["classes"], c["gt"])
        fg = l["gt_classes"][(l["gt_classes"] >= 0) & (l["gt_classes"] < K)]
        assert len(fg) and set(fg.tolist()) == {int(c["gt"][0])}
    if name == "nms_sides":                                # the refined boxes keep both seeds apart; the proposal box would merge them
        assert len(p["index"]) == 2
        q, _ = M.mine_and_label(c["scores"], c["boxes"], c["gt"], K, None, c["seed_rule"])
        assert len(q["index"]) == 1
    if name == "iou_exact":
        v = l["iou"].max(0)
        assert (v == np.float32(0.5)).any() and (v == np.float32(0.6)).any()
        assert (l["gt_classes"][v == np.float32(0.5)] == -1).all() and (l["gt_classes"][v == np.float32(0.6)] < K).all()
    if name == "nan_inf":
        assert np.isnan(p["boxes"]).any() and np.isinf(p["boxes"]).any() and not np.isnan(l["iou"]).any()

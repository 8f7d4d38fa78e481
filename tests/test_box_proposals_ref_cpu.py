"""CPU: the box-proposal AR fixtures (the reference's `_evaluate_box_proposals`, run by tests/golden/make_box_proposal_golden.py)
against the NumPy restatement (box_proposal_ref), restatements made wrong in one rule each, and the host side of
sos_wsod_amd.box_proposals, the evaluator, the postprocess branch and frcnn.ProposalNetwork: layouts, files, what is refused."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import box_proposal_fixture as F
import box_proposal_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def same_bits(a, b):
    """float32 arrays equal bit for bit; a NaN equals a NaN"""
    a, b = np.asarray(a, dtype=np.float32).reshape(-1), np.asarray(b, dtype=np.float32).reshape(-1)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)))


def matches_reference(z, k, r):
    return (same_bits(r["gt_overlaps"], z[k + "/gt_overlaps"]) and same_bits(r["recalls"], z[k + "/recalls"])
            and same_bits(r["ar"], z[k + "/ar"]) and int(r["num_pos"]) == int(z[k + "/num_pos"]))


@pytest.mark.parametrize("name", F.CASES)
def test_restatement_equals_the_reference_bit_for_bit(golden_dir, name):
    z = F.load(golden_dir, name)
    _, _, settings = F.case(name)
    for area, limit in settings:
        r = R.evaluate_case(name, area, limit)
        assert matches_reference(z, F.key(area, limit), r), (name, area, limit)
        assert len(r["gt_overlaps"]) == sum(len(im[1]) for im in r["images"])


def test_hand_case_holds_its_rule_cases(golden_dir):
    z = F.load(golden_dir, "hand")
    _, preds, _ = F.case("hand")
    pos = {p["image_id"]: n for n, p in enumerate(preds)}
    by = {im[0]: im for im in R.evaluate_case("hand", "all", None)["images"]}
    assert by[pos[1]][2].tolist() == [0, 1] and by[pos[1]][3].tolist() == [0, 1] and by[pos[1]][1][0] == 1.0      # the runner-up
    assert by[pos[2]][3].tolist() == [0, 1]                                                    # identical proposals: the first wins
    assert by[pos[3]][1].tolist() == [0, 0, 0] and by[pos[3]][2].tolist() == [0, 1, 2] and by[pos[3]][3].tolist() == [0, 1, 2]
    assert by[pos[4]][1].tolist() == [0.5]                                                     # counted at threshold 0.5
    assert by[pos[8]][1][2:].tolist() == [0, 0, 0] and by[pos[8]][2][2:].tolist() == [-1, -1, -1]
    assert pos[12] not in by and pos[13] not in by and pos[999] not in by
    assert sum(1 for n, p in enumerate(preds) if p["image_id"] == 9 and n in by) == 2         # listed twice, evaluated twice
    # areas 1023.9999 / 1024 / 1024.00001 / 9216 of image 5: small takes three of them, medium three
    small = {im[0]: im for im in R.evaluate_case("hand", "small", None)["images"]}
    medium = {im[0]: im for im in R.evaluate_case("hand", "medium", None)["images"]}
    assert len(small[pos[5]][1]) == 3 and len(medium[pos[5]][1]) == 3
    assert int(z["512-inf/none/num_pos"]) == 0 and np.isnan(z["512-inf/none/ar"]) and np.isnan(z["512-inf/none/recalls"]).all()
    # limit 2 against 2 and 3 proposals: the third in rank is the best one
    assert R.evaluate_case("hand", "all", 2)["images"] != [] and by[pos[11]][1][0] == 1.0
    assert {im[0]: im for im in R.evaluate_case("hand", "all", 2)["images"]}[pos[11]][1][0] == 0.75


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_a_restatement_wrong_in_one_rule_changes_a_bit_on_the_hand_case(golden_dir, variant):
    z = F.load(golden_dir, "hand")
    ds, preds, settings = F.case("hand")
    changed = []
    for area, limit in settings:
        if int(z[F.key(area, limit) + "/num_pos"]) == 0 and variant != "count_no_proposals":
            continue
        r = R.evaluate(ds, preds, area=area, limit=limit, variant=variant)
        if not matches_reference(z, F.key(area, limit), r):
            changed.append((area, limit))
    assert changed, variant


def test_python_mirrors_of_the_header_constants():
    import sos_wsod_amd.box_proposals as BP
    import sos_wsod_amd.ops as ops
    src = open(os.path.join(ROOT, "include", "soswsod_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+SW_BOXAR_(\w+)\s+(\d+)", src, flags=re.M)}
    assert (ops.BOXAR_MAX_AREAS, ops.BOXAR_MAX_LIMITS, ops.BOXAR_MAX_THRESHOLDS, ops.BOXAR_LDS_BOXES, ops.BOXAR_LDS_GT) == \
        (d["MAX_AREAS"], d["MAX_LIMITS"], d["MAX_THRESHOLDS"], d["LDS_BOXES"], d["LDS_GT"])
    assert (BP.MAX_AREAS, BP.MAX_LIMITS, BP.MAX_THRESHOLDS) == (d["MAX_AREAS"], d["MAX_LIMITS"], d["MAX_THRESHOLDS"])
    assert set(ops.BOXAR_STATUS) == {d["BAD_OFFSETS"], d["BAD_LAYOUT"], d["WORKSPACE"]}
    assert BP.AREAS == R.AREAS and BP.AREA_RANGES == R.AREA_RANGES
    assert same_bits(BP.default_thresholds().numpy(), R.default_thresholds())


def test_op_refuses_host_tensors():
    import sos_wsod_amd.ops as ops
    off = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ops.box_proposal_ar(off, torch.zeros(0, 4), off, torch.zeros(0, 4), torch.zeros(0), [[0, 1e10]], [0], [0.5], torch.zeros(2, dtype=torch.int64))


@pytest.mark.parametrize("name", ("hand", "random"))
def test_host_layout_counts_what_the_reference_counts(golden_dir, name):
    """box_proposal_layout needs no GPU: num_pos, the item regions and the ranking against the fixture and the restatement"""
    from sos_wsod_amd.box_proposals import box_proposal_layout
    from sos_wsod_amd.evaluation import COCOGroundTruth
    z = F.load(golden_dir, name)
    ds, preds, settings = F.case(name)
    areas, limits = list(F.AREA_NAMES), [None, 1, 2, 100]
    L = box_proposal_layout(F.records(preds), COCOGroundTruth(ds), areas, limits)
    n = len(preds)
    assert L["item_off"].shape == (len(limits) * len(areas) * n + 1,) and L["item_off"][0] == 0 and (np.diff(L["item_off"]) >= 0).all()
    for a, area in enumerate(areas):
        assert int(L["num_pos"][a]) == int(z[F.key(area, None) + "/num_pos"]), area
        for l, limit in enumerate(limits):
            r = R.evaluate_case(name, area, limit)
            base = (l * len(areas) + a) * n
            lens = np.diff(L["item_off"][base:base + n + 1])
            assert np.nonzero(lens)[0].tolist() == [im[0] for im in r["images"]]
            assert lens[lens > 0].tolist() == [len(im[1]) for im in r["images"]]
    assert L["limits"].tolist() == [0, 1, 2, 100] and L["prop_box"].dtype == np.float32 and L["gt_area"].dtype == np.float32
    gt = R.ground_truth(ds)
    for k, p in enumerate(preds):
        inds = torch.from_numpy(p["logits"].copy()).sort(descending=True)[1].numpy()
        assert np.array_equal(L["prop_box"][L["prop_off"][k]:L["prop_off"][k + 1]], p["boxes"][inds])
        want = gt.get(p["image_id"], (np.zeros((0, 4), np.float32),))[0]
        assert np.array_equal(L["gt_box"][L["gt_off"][k]:L["gt_off"][k + 1]].view(np.uint32), want.view(np.uint32))
    # limits that are all finite cut the upload at the largest
    L2 = box_proposal_layout(F.records(preds), COCOGroundTruth(ds), ["all"], [1, 2])
    assert (np.diff(L2["prop_off"]) <= 2).all()


def test_module_refuses_misuse():
    from sos_wsod_amd.box_proposals import box_proposal_layout, evaluate_box_proposals
    from sos_wsod_amd.evaluation import COCOGroundTruth
    ds, preds, _ = F.case("hand")
    gt, recs = COCOGroundTruth(ds), F.records(preds)
    with pytest.raises(ValueError, match="Unknown area range"):
        box_proposal_layout(recs, gt, ["tiny"], [None])
    with pytest.raises(ValueError, match="limit"):
        box_proposal_layout(recs, gt, ["all"], [0])
    with pytest.raises(ValueError, match="per call"):
        box_proposal_layout(recs, gt, ["all"], list(range(1, 10)))
    bad = [dict(preds[0], logits=np.array([np.nan, 1.0, 2.0], dtype=np.float32))]
    with pytest.raises(ValueError, match="finite"):
        box_proposal_layout(bad, gt, ["all"], [None])
    bad = [dict(preds[0], boxes=np.full((3, 4), np.inf, dtype=np.float32))]
    with pytest.raises(ValueError, match="finite"):
        box_proposal_layout(bad, gt, ["all"], [None])
    with pytest.raises(ValueError, match="thresholds"):
        evaluate_box_proposals(recs, gt, thresholds=torch.zeros(17))
    with pytest.raises(ValueError, match="float32"):
        evaluate_box_proposals(recs, gt, thresholds=torch.zeros(3, dtype=torch.float64))


def test_evaluator_keeps_proposals_only_when_asked(tmp_path):
    from sos_wsod_amd.evaluation import COCOEvaluator
    _, preds, _ = F.case("hand")
    recs = F.records(preds[:3])
    inputs = [{"image_id": r["image_id"]} for r in recs]
    outputs = [{"proposals": r["proposals"]} for r in recs]
    with pytest.raises(ValueError, match="box-proposal AR is out of scope"):                   # the default stays the refusal
        COCOEvaluator(str(tmp_path / "none.json")).process(inputs, outputs)
    ev = COCOEvaluator(str(tmp_path / "none.json"), box_proposals=True)
    ev.process(inputs, outputs)
    assert [p["image_id"] for p in ev._predictions] == [1, 2, 3] and all(set(p) == {"image_id", "proposals"} for p in ev._predictions)
    kept = ev._predictions[0]["proposals"]
    assert kept.proposal_boxes.tensor.device.type == "cpu" and torch.equal(kept.objectness_logits, recs[0]["proposals"].objectness_logits)


def test_box_proposals_pkl_round_trip(tmp_path):
    """the reference's keys (coco_evaluation.py:270-275); read_proposal_file, the scoring path and the Stage-1 loader accept it"""
    from sos_wsod_amd.box_proposals import predictions_from_file, write_box_proposals
    from sos_wsod_amd.proposals import load_proposals_into_dataset, read_proposal_file
    _, preds, _ = F.case("hand")
    path = str(tmp_path / "box_proposals.pkl")
    write_box_proposals(F.records(preds), path)
    with open(path, "rb") as f:
        raw = pickle.load(f)
    assert set(raw) == {"boxes", "objectness_logits", "ids", "bbox_mode"} and raw["bbox_mode"] == 0
    assert raw["ids"] == [p["image_id"] for p in preds]
    assert all(isinstance(b, np.ndarray) and b.dtype == np.float32 for b in raw["boxes"])
    back = read_proposal_file(path)
    for p, b, s in zip(preds, back["boxes"], back["objectness_logits"]):
        assert np.array_equal(b, p["boxes"]) and np.array_equal(s, p["logits"])                # as produced, not ranked
    again = predictions_from_file(path)
    assert [a["image_id"] for a in again] == raw["ids"] and all(np.array_equal(a["boxes"], p["boxes"]) for a, p in zip(again, preds))
    recs = load_proposals_into_dataset([{"image_id": 15}, {"image_id": 1}], path)
    assert recs[0]["proposal_objectness_logits"].tolist() == [4.0, 3.0, 2.0, 1.0, 0.5] and recs[0]["proposal_bbox_mode"] == 0
    # a Detectron-style pickle with XYWH boxes and int16 coordinates is read the same way
    mcg = str(tmp_path / "mcg.pkl")
    with open(mcg, "wb") as f:
        pickle.dump({"boxes": [np.array([[1, 2, 10, 20]], dtype=np.int16)], "scores": [np.array([0.5], dtype=np.float32)],
                     "indexes": ["000005"], "bbox_mode": 1}, f)
    got = predictions_from_file(mcg)
    assert got[0]["image_id"] == "000005" and got[0]["boxes"].tolist() == [[1.0, 2.0, 11.0, 22.0]] and got[0]["boxes"].dtype == np.float32


def test_cli_takes_a_proposals_path(tmp_path):
    from sos_wsod_amd import evaluation as E
    pkl, js = tmp_path / "p.pkl", tmp_path / "gt.json"
    pkl.write_bytes(b"")
    js.write_text("{}")
    args = E.parse_args(["--proposals", str(pkl), "--coco-json", str(js)])
    assert args.proposals == str(pkl) and args.detections is None
    for argv in (["--proposals", str(pkl)], ["--proposals", str(pkl), "--coco-json", str(js), "--detections", str(js)],
                 ["--proposals", str(tmp_path / "missing.pkl"), "--coco-json", str(js)],
                 ["--proposals", str(pkl), "--coco-json", str(js), "--voc-root", str(tmp_path)]):
        with pytest.raises(SystemExit):
            E.parse_args(argv)


def test_voc_adapter_gives_what_convert_to_coco_json_gives(tmp_path):
    from sos_wsod_amd.box_proposals import voc_coco_dataset, voc_ground_truth
    (tmp_path / "ImageSets" / "Main").mkdir(parents=True)
    (tmp_path / "Annotations").mkdir()
    (tmp_path / "ImageSets" / "Main" / "test.txt").write_text("000001\n000002\n")
    obj = "<object><name>{}</name><difficult>{}</difficult><bndbox><xmin>{}</xmin><ymin>{}</ymin><xmax>{}</xmax><ymax>{}</ymax></bndbox></object>"
    xml = "<annotation><size><width>500</width><height>375</height></size>{}</annotation>"
    (tmp_path / "Annotations" / "000001.xml").write_text(xml.format(obj.format("dog", 0, 48, 240, 195, 371) + obj.format("person", 1, 8, 12, 352, 498)))
    (tmp_path / "Annotations" / "000002.xml").write_text(xml.format(""))
    ds = voc_coco_dataset(str(tmp_path), "test")
    assert [im["id"] for im in ds["images"]] == ["000001", "000002"] and ds["images"][0]["height"] == 375
    assert [a["bbox"] for a in ds["annotations"]] == [[47.0, 239.0, 148.0, 132.0], [7.0, 11.0, 345.0, 487.0]]      # difficult kept
    assert [a["area"] for a in ds["annotations"]] == [148.0 * 132.0, 345.0 * 487.0] and all(a["iscrowd"] == 0 for a in ds["annotations"])
    gt = voc_ground_truth(str(tmp_path), "test")
    assert gt.img_ids == ["000001", "000002"] and gt.ann_box.tolist() == [[47.0, 239.0, 148.0, 132.0], [7.0, 11.0, 345.0, 487.0]]


def test_postprocess_branch_for_proposals_agrees_with_the_restatement():
    from sos_wsod_amd.inference import detector_postprocess
    from sos_wsod_amd.structures import Boxes, Instances
    rng = np.random.default_rng(5)
    xy = rng.uniform(-20, 620, (60, 2)).astype(np.float32)
    boxes = np.concatenate([xy, xy + rng.uniform(-5, 200, (60, 2)).astype(np.float32)], 1)
    boxes[:3] = [[700, 10, 800, 50], [10, 500, 50, 600], [5, 5, 5, 80]]                       # outside, outside, zero width
    logits = rng.normal(size=60).astype(np.float32)
    inst = Instances((480, 640))
    inst.proposal_boxes = Boxes(torch.from_numpy(boxes.copy()))
    inst.objectness_logits = torch.from_numpy(logits.copy())
    for oh, ow in ((375, 500), (480, 640), (961, 1283)):
        out = detector_postprocess(inst, oh, ow)
        wb, wl = R.postprocess_proposals(boxes, logits, (480, 640), oh, ow)
        assert out.image_size == (oh, ow) and len(out) == len(wb) < 60
        assert np.array_equal(out.proposal_boxes.tensor.numpy().view(np.uint32), wb.view(np.uint32))
        assert np.array_equal(out.objectness_logits.numpy(), wl)
    assert np.array_equal(inst.proposal_boxes.tensor.numpy(), boxes)                           # the input is left alone
    # pred_boxes: as before
    det = Instances((480, 640))
    det.pred_boxes = Boxes(torch.from_numpy(boxes.copy()))
    det.scores = torch.from_numpy(logits.copy())
    out = detector_postprocess(det, 375, 500)
    wb, wl = R.postprocess_proposals(boxes, logits, (480, 640), 375, 500)
    assert np.array_equal(out.pred_boxes.tensor.numpy().view(np.uint32), wb.view(np.uint32)) and np.array_equal(out.scores.numpy(), wl)


def test_proposal_network_builds_from_a_config_with_the_reference_names():
    import sosplus_ref as SP
    from sos_wsod_amd import frcnn
    from sos_wsod_amd.config import add_wsl_config, get_cfg
    from sos_wsod_amd.rcnn_multi import build_model
    from sos_wsod_amd.registry import META_ARCH_REGISTRY
    assert META_ARCH_REGISTRY.get("ProposalNetwork") is frcnn.ProposalNetwork
    cfg = add_wsl_config(get_cfg())
    cfg.merge_from_list(SP.cfg_list("woi", device="cpu") + ["MODEL.META_ARCHITECTURE", "ProposalNetwork", "MODEL.RPN.POST_NMS_TOPK_TEST", 300])
    m = build_model(cfg)
    assert type(m) is frcnn.ProposalNetwork and not hasattr(m, "roi_heads")
    assert m.proposal_generator.post_nms_topk[1] == 300
    cfg.merge_from_list(["MODEL.META_ARCHITECTURE", "GeneralizedRCNN"])
    det = build_model(cfg)
    dsd, sd = det.state_dict(), m.state_dict()
    assert set(sd) == {k for k in dsd if not k.startswith("roi_heads.")} and any(k.startswith("roi_heads.") for k in dsd)
    assert all(k.startswith(("backbone.", "proposal_generator.")) for k in sd) and all(sd[k].shape == dsd[k].shape for k in sd)
    assert tuple(m.pixel_mean.shape) == (3, 1, 1) and tuple(m.pixel_std.shape) == (3, 1, 1)
    assert {n for n, p in m.named_parameters() if not p.requires_grad} == \
        {n for n, p in det.named_parameters() if not p.requires_grad and not n.startswith("roi_heads.")}
    # a detector checkpoint loads by name, the ROI-head keys ignored; anything else that does not fit is an error
    with torch.no_grad():
        for v in dsd.values():
            v.fill_(0.25)
    m.load_detector_state_dict(dsd)
    assert all(bool((v == 0.25).all()) for v in m.state_dict().values())
    with pytest.raises(RuntimeError):
        m.load_detector_state_dict({k: v for k, v in dsd.items() if k != "proposal_generator.rpn_head.conv.weight"})

"""CPU: the two NumPy forms of the PGF threshold sweep (tests/pgf_sweep_ref.py) agree on every case table, and the host side of
sos_wsod_amd.pgf_sweep — packing, metrics, the best cell, grid parsing, the pseudo-label records — does what it says."""
import copy
import json
import math
import os
import re

import numpy as np
import pytest

import pgf_sweep_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("name", list(R.CASES))
def test_literal_and_decomposed_forms_agree(name):
    case = R.make_case(name)
    lit = R.literal_tables(case)
    for key in ("kept", "tp", "ign", "npos"):
        assert np.array_equal(lit[key], case["expected"][key]), (name, key)


def test_case_tables_cover_what_they_claim():
    sizes = np.diff(R.make_case("sizes_voc")["off"]).tolist()
    assert sizes[:10] == [0, 1, 2, 63, 64, 65, 255, 256, 257, 600] and len(sizes) % 2 == 1 and len(sizes) % 4 != 0
    e = R.make_case("sizes_voc")["expected"]
    assert e["kept"].max() > e["kept"].min() and e["tp"].sum() > 0 and e["ign"].sum() > 0      # the grid changes the result
    big = R.make_case("grid_32x32")
    assert (len(big["t_keep"]), len(big["t_con"]), len(big["iou"])) == (32, 32, 10)
    assert len(set(big["t_keep"])) < 32 and big["t_keep"] != sorted(big["t_keep"])              # repeats, unsorted
    assert {-0.5, 0.0, 1.5} <= set(big["t_keep"]) and {0.0, 1.25} <= set(big["t_con"])
    q = R.make_case("sizes_voc")["t_con"][0]
    assert R.make_case("sizes_voc")["t_con"][1:3] == [np.nextafter(q, -np.inf), np.nextafter(q, np.inf)]
    mem = R.make_case("members")
    assert np.diff(mem["off"]).tolist() == [63, 64, 65, 130, 300] and mem["expected"]["tp"].sum() > 0
    assert all(len(set(mem["classes"][a:b].tolist())) == 1 for a, b in zip(mem["off"][:-1], mem["off"][1:]))
    obj = R.make_case("objects")
    per = {}
    for k in range(len(obj["gt_off"]) - 1):
        for c in obj["gt_cls"][obj["gt_off"][k]:obj["gt_off"][k + 1]]:
            per[(k, int(c))] = per.get((k, int(c)), 0) + 1
    assert {1, 64, 65} <= set(per.values())
    ign = R.make_case("all_ignored")
    assert ign["gt_ign"].all() and ign["expected"]["npos"].sum() == 0 and ign["expected"]["tp"].sum() == 0
    assert ign["expected"]["ign"].sum() > 0


def test_edge_case_counts():
    """the hand-made images, from the rule alone: thresholds 0.5, 0.45, 0.75"""
    e = R.make_case("edges")["expected"]
    kept, tp, ign = e["kept"][0, 0], e["tp"][:, 0, 0], e["ign"][:, 0, 0]
    assert kept[[0, 1, 2, 3, 4, 7]].tolist() == [1, 1, 1, 1, 2, 0]
    assert tp[:, 0].tolist() == [0, 1, 0]                      # IoU exactly 0.5: no match at 0.5, one at 0.45
    assert tp[:, 1].tolist() == [1, 1, 0]                      # two objects at 2 / 3: one claimed
    assert tp[:, 4].tolist() == [1, 1, 1]                      # two identical detections, one object
    assert tp[:, 2].tolist() == [0, 0, 0] and ign[:, 2].tolist() == [1, 1, 1]
    assert tp[:, 3].tolist() == [0, 0, 0] and ign.sum() == 3   # no object row: kept, nothing to match
    assert e["npos"][[0, 1, 2, 3, 4]].tolist() == [1, 2, 1, 0, 1]


def test_header_limits_mirrored():
    import sos_wsod_amd.ops as ops
    import sos_wsod_amd.pgf_sweep as S
    src = open(os.path.join(ROOT, "include", "soswsod_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+(SW_PGF\w+)\s+(\d+)\s*$", src, flags=re.M)}
    assert (ops.PGF_SWEEP_MAX_KEEP, ops.PGF_SWEEP_MAX_CON, ops.PGF_SWEEP_MAX_IOU, ops.PGF_SWEEP_WS_WORDS) == \
        (d["SW_PGF_SWEEP_MAX_KEEP"], d["SW_PGF_SWEEP_MAX_CON"], d["SW_PGF_SWEEP_MAX_IOU"], d["SW_PGF_SWEEP_WS_WORDS"])
    assert (S.MAX_KEEP, S.MAX_CON, S.MAX_IOU) == (ops.PGF_SWEEP_MAX_KEEP, ops.PGF_SWEEP_MAX_CON, ops.PGF_SWEEP_MAX_IOU)
    assert (ops.PGF_LDS_CAP, ops.PGF_MAX_CLASSES) == (d["SW_PGF_LDS_CAP"], d["SW_PGF_MAX_CLASSES"])
    assert len(S.IOU_THRESHOLDS) == S.MAX_IOU


def test_packed_layout():
    import sos_wsod_amd.ops as ops
    layout, total = ops.pgf_sweep_layout(3, 2, 4, 5, guard=7)
    assert layout["kept"] == (7, (3, 2, 5)) and layout["tp"] == (7 + 30 + 7, (4, 3, 2, 5))
    assert layout["ign"][0] == 44 + 120 + 7 and layout["npos"] == (171 + 120 + 7, (5,)) and total == 298 + 5 + 7
    host = np.arange(total, dtype=np.int64)
    t = ops.pgf_sweep_unpack(host, 3, 2, 4, 5, guard=7)
    assert t["kept"][0, 0, 0] == 7 and t["npos"].tolist() == list(range(298, 303)) and t["tp"].shape == (4, 3, 2, 5)


VOC_DICTS = [
    {"image_id": "000005", "annotations": [
        {"category_id": 8, "bbox": [262.0, 210.0, 324.0, 339.0], "bbox_mode": 0, "difficult": 0},
        {"category_id": 8, "bbox": [4.0, 243.0, 67.0, 374.0], "bbox_mode": 0, "difficult": 1},
        {"category_id": 3, "bbox": [10.0, 20.0, 30.0, 40.0], "bbox_mode": 1}]},
    {"image_id": "000007", "annotations": [{"category_id": 6, "bbox": [140.0, 49.0, 500.0, 330.0], "bbox_mode": 0, "difficult": 0}]},
    {"image_id": "000009", "annotations": [{"category_id": 12, "bbox": [1.0, 2.0, 3.0, 4.0], "bbox_mode": 0, "difficult": 0}]},
]
VOC_RECORDS = [
    {"image_id": 7, "category_id": 7, "score": 0.9, "bbox": [141.0, 50.0, 500.0, 330.0]},
    {"image_id": 5, "category_id": 9, "score": 0.8, "bbox": [263.0, 211.0, 324.0, 339.0]},
    {"image_id": 5, "category_id": 2, "score": 0.3, "bbox": [1.0, 1.0, 9.0, 9.0]},        # class 1: not in the image's ground truth
    {"image_id": 11, "category_id": 9, "score": 0.7, "bbox": [1.0, 1.0, 9.0, 9.0]},       # no such image: skipped
    {"image_id": 7, "category_id": 7, "score": 0.1, "bbox": [141.0, 50.0, 400.0, 300.0]},
]


def test_voc_packing_and_inputs_not_mutated():
    import sos_wsod_amd.pgf_sweep as S
    from sos_wsod_amd import pseudo_labels as P
    records, dicts = copy.deepcopy(VOC_RECORDS), copy.deepcopy(VOC_DICTS)
    groups, anns = S.voc_groups(records, dicts)
    assert records == VOC_RECORDS and dicts == VOC_DICTS
    assert list(groups) == [7, 5, 9] and [len(groups[i]) for i in groups] == [2, 2, 0]      # first appearance, then the rest
    assert [r["category_id"] for r in groups[7]] == [6, 6] and groups[7][0] is not records[0]
    class_dict = {i: P._unique(a["category_id"] for a in anns[i]) for i in groups}
    g = P.pack_groups(groups, class_dict, P.VOC_DIFF_CLASSES)
    assert g["universe"].tolist() == [1, 3, 6, 8, 12] and g["K"] == 5 and g["off"].tolist() == [0, 2, 4, 4]
    assert g["classes"].tolist() == [2, 2, 3, 0]
    assert g["gt_mask"][:, 0].tolist() == [0b00100, 0b01010, 0b10000] and g["diff_mask"].tolist() == [0b01100]
    off, box, cls, ign = S.pack_ground_truth(g["ids"], anns, g["universe"], "difficult", (1.0, 1.0, 0.0, 0.0))
    assert off.tolist() == [0, 1, 4, 5] and cls.tolist() == [2, 3, 3, 1, 4] and ign.tolist() == [0, 0, 1, 0, 0]
    assert off.dtype == np.int64 and box.dtype == np.float64 and cls.dtype == np.int32 and ign.dtype == np.uint8
    assert box[0].tolist() == [141.0, 50.0, 500.0, 330.0]                                  # the loader's - 1 undone
    assert box[3].tolist() == [11.0, 21.0, 40.0, 60.0]                                     # XYWH -> corners, then the shift
    assert records == VOC_RECORDS and dicts == VOC_DICTS


def test_coco_packing_image_without_ground_truth_of_a_detected_class():
    import sos_wsod_amd.pgf_sweep as S
    from sos_wsod_amd import pseudo_labels as P
    dicts = [{"image_id": 42, "annotations": [{"category_id": 5, "bbox": [1.5, 2.5, 10.0, 20.0], "bbox_mode": 1, "iscrowd": 1}]},
             {"image_id": 43, "annotations": []}]
    dets = [{"image_id": 43, "instances": [{"category_id": 9, "bbox": [0.0, 0.0, 5.0, 5.0], "score": 0.5}]},
            {"image_id": 42, "instances": [{"category_id": 9, "bbox": [0.0, 0.0, 5.0, 5.0], "score": 0.5}]},
            {"image_id": 42, "instances": [{"category_id": 7, "bbox": [1.0, 1.0, 5.0, 5.0], "score": 0.25}]}]   # the last entry wins
    before = copy.deepcopy((dets, dicts))
    groups, anns = S.coco_groups(dets, dicts)
    assert (dets, dicts) == before
    assert list(groups) == [43, 42] and groups[42][0]["category_id"] == 7
    class_dict = {i: P._unique(a["category_id"] for a in anns[i]) for i in groups}
    g = P.pack_groups(groups, class_dict, ())
    assert g["universe"].tolist() == [5, 7, 9] and g["gt_mask"][:, 0].tolist() == [0, 1]     # no detected class is in any mask
    off, box, cls, ign = S.pack_ground_truth(g["ids"], anns, g["universe"], "iscrowd", (0.0, 0.0, 0.0, 0.0))
    assert off.tolist() == [0, 0, 1] and box.tolist() == [[1.5, 2.5, 11.5, 22.5]] and cls.tolist() == [0] and ign.tolist() == [1]
    with pytest.raises(ValueError):
        S.corners([0, 0, 1, 1], 2)
    with pytest.raises(ValueError):
        S.sweep_coco(dets, dicts, [0.2], [0.85], use_diff=False)


def _result():
    import sos_wsod_amd.pgf_sweep as S
    kept = np.array([[[4, 0, 3], [2, 0, 0]]])                           # [1, 2, 3]
    tp = np.array([[[[2, 0, 1], [1, 0, 0]]], [[[1, 0, 0], [0, 0, 0]]]])  # [2, 1, 2, 3]
    ign = np.array([[[[1, 0, 1], [2, 0, 0]]], [[[0, 0, 0], [0, 0, 0]]]])
    return S.SweepResult(kept, tp, ign, [4, 0, 2], [0.2], [0.5, 0.85], [0.5, 0.75], [3, 8, 11])


def test_metric_formulas_and_zero_denominators():
    r = _result()
    p, rec, f = r.precision(True), r.recall(True), r.f1(True)
    assert p.shape == (2, 1, 2, 3) and rec.shape == (2, 1, 2, 3)
    assert p[0, 0, 0].tolist()[0] == 2 / 3 and math.isnan(p[0, 0, 0, 1]) and p[0, 0, 0, 2] == 0.5
    assert math.isnan(p[0, 0, 1, 0])                                    # kept - ign == 0
    assert rec[0, 0, 0, 0] == 0.5 and math.isnan(rec[0, 0, 0, 1]) and rec[0, 0, 0, 2] == 0.5
    assert f[0, 0, 0, 0] == 2 * 2 / (3 + 4) and math.isnan(f[0, 0, 0, 1]) and math.isnan(f[0, 0, 1, 0])
    assert f[1, 0, 1, 2] != f[1, 0, 1, 2]                               # class 11 keeps nothing in cell (0, 1)
    pm, rm, fm = r.precision(), r.recall(), r.f1()
    assert pm.shape == (2, 1, 2) and math.isnan(pm[0, 0, 1]) and math.isnan(fm[0, 0, 1])
    assert pm[0, 0, 0] == 3 / 5 and rm[0, 0].tolist() == [3 / 6, 1 / 6] and fm[0, 0, 0] == 6 / (5 + 6)
    assert pm[1, 0, 0] == 1 / 7 and pm[1, 0, 1] == 0.0 and fm[1, 0, 1] == 0.0
    back = type(r).from_json(json.loads(json.dumps(r.to_json())))
    assert np.array_equal(back.tp, r.tp) and back.t_con == r.t_con and back.classes == [3, 8, 11]


def test_best_prefers_lowest_t_keep_then_lowest_t_con():
    import sos_wsod_amd.pgf_sweep as S
    t_keep, t_con = [0.3, 0.1, 0.1], [0.9, 0.7]                         # unsorted, repeated
    kept = np.full((3, 2, 1), 4)
    tp = np.full((1, 3, 2, 1), 2)
    tp[0, 0, 0, 0] = 1                                                  # one worse cell
    r = S.SweepResult(kept, tp, np.zeros_like(tp), [4], t_keep, t_con, [0.5], [0])
    b = r.best()
    assert (b["t_keep"], b["t_con"], b["a"], b["b"], b["f1"]) == (0.1, 0.7, 1, 1, 0.5)
    assert r.best("recall", 0.5)["recall"] == 0.5
    with pytest.raises(ValueError):
        r.best("f1", 0.6)
    with pytest.raises(ValueError):
        r.best("map")
    empty = S.SweepResult(np.zeros((1, 1, 1)), np.zeros((1, 1, 1, 1)), np.zeros((1, 1, 1, 1)), [0], [0.2], [0.85], [0.5], [0])
    assert empty.best() is None


def test_grid_parsing():
    import sos_wsod_amd.pgf_sweep as S
    assert S.parse_grid("0:1:0.05") == [round(0.05 * i, 10) for i in range(21)]
    assert S.parse_grid("0.5:1:0.05")[-1] == 1.0 and len(S.parse_grid("0.5:1:0.05")) == 11
    assert S.parse_grid("0.2:0.9:0.25") == [0.2, 0.45, 0.7]
    assert S.parse_grid("0.85,0.2, 0.85") == [0.85, 0.2, 0.85]
    assert S.parse_grid("0.3") == [0.3]
    for bad in ("0:1", "0:1:0", "1:0:0.1"):
        with pytest.raises(ValueError):
            S.parse_grid(bad)
    with pytest.raises(ValueError):
        S.check_grid([0.1] * 33, [0.5], [0.5])
    with pytest.raises(ValueError):
        S.check_grid([0.1], [], [0.5])
    with pytest.raises(ValueError):
        S.check_grid([0.1], [float("nan")], [0.5])
    with pytest.raises(ValueError):
        S.check_grid([0.1], [0.5], [0.5] * 11)
    args = S.parse_args(["--gt-dicts", "x.json", "--t-keep", "0:0.2:0.1", "--t-con", "0.85"])
    assert args.t_keep == [0.0, 0.1, 0.2] and args.t_con == [0.85] and args.iou == list(S.IOU_THRESHOLDS)
    with pytest.raises(SystemExit):
        S.parse_args(["--gt-dicts", "x.json", "--dataset", "coco"])
    with pytest.raises(SystemExit):
        S.parse_args(["--gt-dicts", "x.json", "--t-keep", "0:1:0.01"])


def test_pseudo_label_records_round_trip(tmp_path):
    """records -> the pseudo-label file pgf_voc writes (0-based classes, grouped by image) -> the records the evaluator reads"""
    import sos_wsod_amd.pgf_sweep as S
    from sos_wsod_amd import pseudo_labels as P
    kept = [r for r in VOC_RECORDS if r["image_id"] != 11]
    pgt = {}
    for r in kept:
        pgt.setdefault(r["image_id"], []).append(dict(r, category_id=r["category_id"] - 1))
    P.add_multi_label(pgt, VOC_DICTS)
    before = copy.deepcopy(pgt)
    path = tmp_path / "pgt.json"
    P.write_json(pgt, str(path))
    for source in (pgt, str(path)):
        out = S.pseudo_label_records(source)
        assert sorted(out, key=json.dumps) == sorted(kept, key=json.dumps)
        assert [r["image_id"] for r in out] == [7, 7, 5, 5]             # file order: grouped by image
    assert pgt == before

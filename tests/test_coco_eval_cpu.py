"""CPU: the COCO evaluation's host side (sos_wsod_amd.evaluation) and the NumPy restatement the GPU fuzz is measured against
(coco_eval_fixture.restated), which must equal the reference's own arrays (tests/golden/coco_eval_*.npz) bit for bit."""
import json
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import coco_eval_fixture as F


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.where(np.isnan(a), 0.0, a).tobytes() == np.where(np.isnan(b), 0.0, b).tobytes()


def check_against_fixture(z, ev, stats, result):
    """precision, scores, recall, stats and the result dict against what the fixture stores, all bitwise"""
    assert ev["counts"] == [10, 101, len(z["cat_ids"]), 4, 3]
    assert _same(ev["recall"], z["recall"]), np.argwhere(ev["recall"] != z["recall"])[:5]
    for k in ("precision", "scores"):
        if k in z:
            assert _same(ev[k], z[k]), (k, np.argwhere(ev[k] != z[k])[:5])
        else:
            sha, crc = F.digest(ev[k])
            assert np.array_equal(crc, z[k + "_crc"]), (k, "categories", np.nonzero(crc != z[k + "_crc"])[0])
            assert np.array_equal(sha, z[k + "_sha256"]), k
    assert _same(stats, z["stats"]), (stats, z["stats"])
    want = F.expected_results(z)
    assert list(result) == list(want)
    for k in want:
        assert _same(result[k], want[k]), (k, result[k], want[k])


@pytest.mark.parametrize("case", F.CASES)
def test_restatement_equals_reference(golden_dir, case):
    z = F.load(golden_dir, case)
    ds, res = F.dataset(z), F.results(z)
    ev = F.restated(ds, res)
    stats = F.summarize(ev)
    names = [c["name"] for c in sorted(ds["categories"], key=lambda c: c["id"])]
    check_against_fixture(z, ev, stats, F.derive(ev, stats, names))


def test_hand_case_covers_its_edges(golden_dir):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "hand")
    ds, res = F.dataset(z), F.results(z)
    # IoU exactly at the thresholds, where >= matches
    assert F.bb_iou([0, 0, 10, 5], [0, 0, 10, 10], False) == 0.5 == F.IOU_THRS[0]
    assert F.bb_iou([100, 100, 10, 7.5], [100, 100, 10, 10], False) == 0.75 >= F.IOU_THRS[5]
    assert F.bb_iou([0, 0, 10, 4.9], [0, 0, 10, 10], False) < 0.5
    assert F.bb_iou([300, 300, 20, 20], [290, 290, 80, 80], True) == 1.0          # the crowd box behind the held match
    assert 0.5 < F.bb_iou([300, 300, 20, 20], [300, 300, 25, 25], False) < 1.0
    assert F.bb_iou([10, 10, 0, 40], [10, 10, 40, 40], False) == 0.0              # zero width
    cat = {c["name"]: k for k, c in enumerate(sorted(ds["categories"], key=lambda c: c["id"]))}
    assert (z["precision"][:, :, :, 3, :] == -1).all() and z["stats"][5] == -1     # no ground truth in the large range
    assert np.isnan(F.expected_results(z)["APl"])
    assert (z["precision"][:, :, cat["nogt"]] == -1).all()
    assert (z["precision"][:, :, cat["nodet"], 0] == 0).all() and (z["recall"][:, cat["nodet"], 0] == 0).all()
    assert z["precision"][0, 0, cat["edge"], 0, 2] == 1.0 and z["recall"][0, cat["edge"], 0, 2] > z["recall"][1, cat["edge"], 0, 2]
    # the id-0 annotation: its perfect detection is no true positive, so recall at 0.5 stays below 1
    assert 0 in z["ann_id"] and z["recall"][0, cat["area"], 0, 2] < 1.0
    # a pair beyond the LDS slice (100 x 20 IoUs), one beyond 64 objects, a category beyond one accumulate tile
    L = E.coco_eval_layout(E.COCOGroundTruth(ds), E.COCODetections.from_results(res, E.COCOGroundTruth(ds)))
    D, G = np.diff(L["pair_off"]), L["gt_off"][L["pair_gt"] + 1] - L["gt_off"][L["pair_gt"]]
    assert ((D == 100) & (G == 20)).any() and (G == 70).any() and D.max() == 100
    assert (L["pair_ws"] >= 0).sum() == 2 and L["ws_words"] == (100 * 20 + 40 + 40) + (25 * 70 + 80 + 140)
    assert np.diff(L["cat_off"]).max() > 1024
    assert sum(1 for r in res if r["category_id"] == 99) == 1 and len(L["det_score"]) == len(res) - 1 - 30


def test_ground_truth_loading_and_id_mapping(tmp_path):
    from sos_wsod_amd import evaluation as E
    ds = {"images": [{"id": 9}, {"id": 2}, {"id": 5}],
          "categories": [{"id": 7, "name": "g"}, {"id": 3, "name": "c"}, {"id": 90, "name": "z"}],
          "annotations": [
              {"id": 4, "image_id": 5, "category_id": 7, "bbox": [1, 2, 3, 4], "area": 5.5, "iscrowd": 0, "ignore": 1},
              {"id": 0, "image_id": 2, "category_id": 3, "bbox": [0, 0, 10, 10], "area": 100, "iscrowd": 1},
              {"id": 6, "image_id": 77, "category_id": 3, "bbox": [0, 0, 1, 1], "area": 1, "iscrowd": 0},       # unlisted image
              {"id": 8, "image_id": 5, "category_id": 8, "bbox": [0, 0, 1, 1], "area": 1, "iscrowd": 0},        # unlisted category
              {"id": 9, "image_id": 5, "category_id": 7, "bbox": [5, 5, 5, 5], "area": 25}]}
    path = tmp_path / "ann.json"
    path.write_text(json.dumps(ds))
    gt = E.COCOGroundTruth.load(str(path))
    assert gt.img_ids == [2, 5, 9] and gt.cat_ids == [3, 7, 90] and gt.thing_classes == ["c", "g", "z"]
    assert gt.thing_dataset_id_to_contiguous_id == {3: 0, 7: 1, 90: 2}
    assert gt.ann_img.tolist() == [1, 0, 1] and gt.ann_cat.tolist() == [1, 0, 1]
    assert gt.ann_crowd.tolist() == [False, True, False]            # "ignore" in the file is overwritten by iscrowd
    assert gt.ann_idpos.tolist() == [True, False, True] and gt.ann_area.tolist() == [5.5, 100.0, 25.0]
    L = E.coco_eval_layout(gt, E.COCODetections([], [], [], []))
    assert L["gt_off"].tolist() == [0, 1, 1, 1, 1, 3, 3, 3, 3, 3] and L["gt_flags"].tolist() == [1, 2, 2]
    assert L["npig"].tolist() == [[0, 0, 0, 0], [2, 2, 0, 0], [0, 0, 0, 0]] and L["ws_words"] == 0
    ids, pos = gt.select([9, 2, 9])
    assert ids == [2, 9] and pos.tolist() == [0, -1, 1]
    with pytest.raises(ValueError, match="not in the annotation file"):
        gt.select([2, 3])
    with pytest.raises(ValueError, match="no annotations"):
        E.COCOGroundTruth({"images": [], "categories": [{"id": 1}]})
    bad = dict(ds, annotations=[dict(ds["annotations"][0], bbox=[0, 0, float("inf"), 1])])
    with pytest.raises(ValueError, match="finite"):
        E.COCOGroundTruth(bad)


def test_load_res_rules():
    from sos_wsod_amd import evaluation as E
    gt = E.COCOGroundTruth({"images": [{"id": 1}, {"id": 2}], "categories": [{"id": 5}, {"id": 6}], "annotations": []})
    res = [{"image_id": 2, "category_id": 6, "bbox": [1, 2, 3, 4], "score": 0.5},
           {"image_id": 1, "category_id": 4, "bbox": [1, 2, 3, 4], "score": 0.9},         # unknown category: dropped
           {"image_id": 1, "category_id": 5, "bbox": [0, 0, 2, 2], "score": 0.5}]
    d = E.COCODetections.from_results(res, gt)
    assert d.img.tolist() == [1, 0] and d.cat.tolist() == [1, 0] and d.box.tolist() == [[1, 2, 3, 4], [0, 0, 2, 2]]
    with pytest.raises(ValueError, match="not in the annotation file"):
        E.COCODetections.from_results([dict(res[0], image_id=3)], gt)
    for k, v in (("score", float("nan")), ("bbox", [0, 0, float("inf"), 1])):
        with pytest.raises(ValueError, match="finite"):
            E.COCODetections.from_results([dict(res[0], **{k: v})], gt)
    for extra in ({"segmentation": {}}, {"keypoints": []}):
        with pytest.raises(ValueError, match="out of scope"):
            E.COCODetections.from_results([dict(res[0], **extra)], gt)
    # ties keep list order; a pair is cut at 100; ranks restart per pair
    many = [{"image_id": 1, "category_id": 5, "bbox": [0, 0, 1 + k, 1], "score": 0.5 if k % 2 else 0.25} for k in range(120)]
    L = E.coco_eval_layout(gt, E.COCODetections.from_results(many + res, gt))
    assert L["pair_off"].tolist() == [0, 100, 101] and L["cat_off"].tolist() == [0, 100, 101]
    assert L["det_rank"].tolist() == list(range(100)) + [0]
    # the 60 of score 0.5 in list order, then the later entry of the same score, then the first of score 0.25
    assert L["det_box"][:62, 2].tolist() == [2 + 2 * k for k in range(60)] + [2, 1]
    assert L["pair_gt"].tolist() == [0, 3]


def test_workspace_words_equal_the_library():
    from sos_wsod_amd import evaluation as E
    from sos_wsod_amd._lib import lib
    for cap in (0, 1, 640, 1600):
        for D in (0, 1, 16, 25, 26, 100):
            for G in (0, 1, 16, 17, 64, 65, 128, 129, 700):
                assert lib.sw_coco_eval_workspace_bytes(D, G, cap) == 8 * int(E.coco_pair_workspace_words(D, G, cap)), (D, G, cap)
    assert lib.sw_coco_eval_workspace_bytes(100, 16, 1600) == 0 and lib.sw_coco_eval_workspace_bytes(100, 17, 1600) > 0
    assert lib.sw_coco_eval_workspace_bytes(256, 1, 1600) == -1 and lib.sw_coco_eval_workspace_bytes(1, 1, 1601) == -1
    # the largest pair the kernel takes: 255 x (2^23 - 1) IoUs still index with an int
    g_max = (1 << 23) - 1
    assert 255 * g_max < 2 ** 31 and lib.sw_coco_eval_workspace_bytes(255, g_max, 1600) == 8 * int(E.coco_pair_workspace_words(255, g_max))
    assert lib.sw_coco_eval_workspace_bytes(1, g_max + 1, 1600) == -1


def test_summarize_and_results_of_stored_arrays(golden_dir):
    from sos_wsod_amd import evaluation as E
    for case in ("hand", "random"):
        z = F.load(golden_dir, case)
        ev = {"precision": z["precision"], "recall": z["recall"], "scores": z["scores"]}
        stats = E.coco_summarize(ev)
        assert _same(stats, z["stats"])
        names = [str(z["cat_names"][k]) for k in np.argsort(z["cat_ids"], kind="stable")]
        got, want = E.derive_coco_results(ev, stats, names), F.expected_results(z)
        assert list(got) == list(want) and all(_same(got[k], want[k]) for k in want)
    assert np.array_equal(E.COCO_IOU_THRS, F.IOU_THRS) and np.array_equal(E.COCO_REC_THRS, F.REC_THRS)
    nan = E.derive_coco_results(None, None, ["a", "b"])
    assert list(nan) == list(E.COCO_METRICS) and all(np.isnan(v) for v in nan.values())


def test_ops_refuse_host_tensors():
    import torch
    from sos_wsod_amd import ops
    z64, zf = torch.zeros(1, dtype=torch.int64), torch.zeros(0, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ops.coco_eval(z64, z64[:0], z64[:0], 0, zf, z64, zf, zf[:, 0], torch.zeros(0, dtype=torch.uint8), torch.zeros(4, 2).double(),
                      torch.zeros(10).double(), torch.zeros(101).double(), torch.zeros(3, dtype=torch.int32),
                      torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.uint8),
                      zf[:, 0], torch.zeros(1, 4, dtype=torch.int64))


def _instances(boxes, scores, classes):
    import torch
    from sos_wsod_amd.structures import Boxes, Instances
    inst = Instances((480, 640))
    inst.pred_boxes = Boxes(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4))
    inst.scores = torch.tensor(scores, dtype=torch.float32)
    inst.pred_classes = torch.tensor(classes, dtype=torch.int64)
    return inst


def test_evaluator_records_files_and_pseudo_label_round_trip(tmp_path, monkeypatch):
    from sos_wsod_amd import evaluation as E
    from sos_wsod_amd import pseudo_labels as PL
    ds = {"images": [{"id": 3}, {"id": 8}], "categories": [{"id": 2, "name": "a"}, {"id": 5, "name": "b"}],
          "annotations": [{"id": 1, "image_id": 3, "category_id": 5, "bbox": [10, 10, 20, 20], "area": 400, "iscrowd": 0}]}
    ann = tmp_path / "ann.json"
    ann.write_text(json.dumps(ds))
    with pytest.raises(ValueError, match="save_path"):
        E.COCOEvaluator(str(ann), save_detection_result=True)
    ev = E.COCOEvaluator(str(ann), output_dir=str(tmp_path / "out"), save_detection_result=True,
                         save_path=str(tmp_path / "oicr_plus_{}.json"), name="coco_2014_train")
    ev.reset()
    assert ev.evaluate() == {}                                     # no predictions
    ev.process([{"image_id": 3}, {"image_id": 8}],
               [{"instances": _instances([[10, 10, 30, 30], [0, 0, 5.5, 4]], [0.75, 0.5], [1, 0])}, {"instances": _instances([], [], [])}])
    assert ev._predictions == [
        {"image_id": 3, "instances": [{"image_id": 3, "category_id": 1, "bbox": [10.0, 10.0, 20.0, 20.0], "score": 0.75},
                                      {"image_id": 3, "category_id": 0, "bbox": [0.0, 0.0, 5.5, 4.0], "score": 0.5}]},
        {"image_id": 8, "instances": []}]
    with pytest.raises(ValueError, match="out of scope"):
        ev.process([{"image_id": 3}], [{"proposals": None}])
    for field in ("pred_masks", "pred_keypoints"):                 # segm and keypoint outputs are refused, not dropped
        inst = _instances([[0, 0, 1, 1]], [0.5], [0])
        setattr(inst, field, inst.scores.clone())
        with pytest.raises(ValueError, match="out of scope"):
            ev.process([{"image_id": 3}], [{"instances": inst}])
    assert len(ev._predictions) == 2
    seen = {}

    def fake_arrays(gt, dets, img_ids=None, **kw):
        seen.update(cat=dets.cat.tolist(), box=dets.box.tolist(), img_ids=img_ids)
        return F.restated(ds, json.loads((tmp_path / "out" / "coco_instances_results.json").read_text()), img_ids)

    monkeypatch.setattr(E, "coco_eval_arrays", fake_arrays)
    got = ev.evaluate(img_ids=[3])
    assert seen == {"cat": [1, 0], "box": [[10.0, 10.0, 20.0, 20.0], [0.0, 0.0, 5.5, 4.0]], "img_ids": [3]}
    assert list(got) == ["bbox"] and got["bbox"]["AP"] == 100.0 and got["bbox"]["AP-b"] == 100.0 and np.isnan(got["bbox"]["AP-a"])
    assert ev.stats[0] == 1.0 and ev.eval["precision"].shape == (10, 101, 2, 4, 3)
    written = json.loads((tmp_path / "out" / "coco_instances_results.json").read_text())
    assert [r["category_id"] for r in written] == [5, 2]           # dataset ids in the result file
    saved = json.loads((tmp_path / "oicr_plus_coco_2014_train.json").read_text())
    assert saved == ev._predictions                                # contiguous ids in the Stage-2 file
    # Stage 2 reads the saved file: pgf_coco groups it by image against the dataset dicts
    groups = {}
    monkeypatch.setattr(PL, "filter_groups", lambda g, class_dict, *a: (groups.update(g) or g, {"n": len(class_dict)}))
    dicts = [{"image_id": 3, "annotations": [{"category_id": 1}]}, {"image_id": 8, "annotations": []}]
    result, _ = PL.pgf_coco(saved, dicts)
    assert list(result) == [3, 8] and result[3] == saved[0]["instances"] and result[8] == []
    anns = PL.gen_annotations(result, id2cat={0: 2, 1: 5})
    assert [(a["image_id"], a["category_id"], a["bbox"]) for a in anns] == [(3, 5, [10.0, 10.0, 20.0, 20.0]), (3, 2, [0.0, 0.0, 5.5, 4.0])]
    # predictions without any instance: the all-NaN dict
    ev.reset()
    ev.process([{"image_id": 8}], [{"instances": _instances([], [], [])}])
    got = ev.evaluate()
    assert list(got["bbox"]) == list(E.COCO_METRICS) and all(np.isnan(v) for v in got["bbox"].values())
    # a class outside the dataset's contiguous range is refused as the reference asserts
    ev.reset()
    ev.process([{"image_id": 8}], [{"instances": _instances([[0, 0, 1, 1]], [0.5], [2])}])
    with pytest.raises(ValueError, match="not available in the dataset"):
        ev.evaluate()


def test_cli_argument_parsing(tmp_path):
    from sos_wsod_amd import evaluation as E
    ann, det = tmp_path / "ann.json", tmp_path / "coco_instances_results.json"
    ann.write_text("{}")
    det.write_text("[]")
    args = E.parse_args(["--coco-json", str(ann), "--detections", str(det)])
    assert args.coco_json == str(ann) and args.detections == str(det) and args.out is None and args.voc_root is None
    args = E.parse_args(["--coco-json", str(ann), "--detections", str(det), "--out", str(tmp_path / "m.json")])
    assert args.out == str(tmp_path / "m.json")
    bad = [["--coco-json", str(ann)],
           ["--coco-json", str(tmp_path / "none.json"), "--detections", str(det)],
           ["--coco-json", str(ann), "--detections", str(tmp_path / "none.json")],
           ["--coco-json", str(ann), "--voc-root", str(tmp_path), "--detections", str(det)],
           ["--detections", str(det)]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            E.parse_args(argv)
        assert e.value.code == 2, argv


def test_cli_missing_argument_messages(capsys):
    """argparse's own wording for the arguments a VOC call needs, whichever are missing"""
    from sos_wsod_amd import evaluation as E
    for argv, flags in (([], "--voc-root, --detections"), (["--detections", "d.json"], "--voc-root"),
                        (["--voc-root", "r"], "--detections"), (["--coco-json", "a.json"], "--detections")):
        with pytest.raises(SystemExit):
            E.parse_args(argv)
        assert capsys.readouterr().err.strip().endswith("error: the following arguments are required: " + flags), argv


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_GATHER_DS = {"images": [{"id": 3}, {"id": 8}], "categories": [{"id": 2, "name": "a"}, {"id": 5, "name": "b"}],
              "annotations": [{"id": 1, "image_id": 3, "category_id": 5, "bbox": [10, 10, 20, 20], "area": 400, "iscrowd": 0},
                              {"id": 2, "image_id": 8, "category_id": 2, "bbox": [0, 0, 8, 8], "area": 64, "iscrowd": 0}]}


def _gather_records(rank):
    """rank 1 holds image 3 (the list's first image), rank 0 image 8: rank order, not image order, decides the gathered list"""
    if rank == 0:
        return [{"image_id": 8, "instances": [{"image_id": 8, "category_id": 0, "bbox": [0.0, 0.0, 8.0, 8.0], "score": 0.5},
                                              {"image_id": 8, "category_id": 1, "bbox": [1.0, 1.0, 2.0, 2.0], "score": 0.5}]}]
    return [{"image_id": 3, "instances": [{"image_id": 3, "category_id": 1, "bbox": [10.0, 10.0, 20.0, 20.0], "score": 0.5}]}]


def _gather_worker(rank, world, port, tmp):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import evaluation as E
    seen = []

    def fake_arrays(gt, dets, img_ids=None, **kw):                 # the kernels' stand-in: the restatement of what rank 0 wrote
        seen.append({"img": dets.img.tolist(), "cat": dets.cat.tolist()})
        with open(os.path.join(tmp, f"out{rank}", "coco_instances_results.json")) as f:
            return F.restated(_GATHER_DS, json.load(f), img_ids)

    E.coco_eval_arrays = fake_arrays
    ev = E.COCOEvaluator(os.path.join(tmp, "ann.json"), output_dir=os.path.join(tmp, f"out{rank}"), save_detection_result=True,
                         save_path=os.path.join(tmp, "saved_rank%d_{}.json" % rank), name="split")
    ev.reset()
    ev.set_predictions(_gather_records(rank))
    got = ev.evaluate()
    with open(os.path.join(tmp, f"result.{rank}"), "w") as f:
        json.dump({"result": got, "seen": seen, "gathered": E.gather_predictions(_gather_records(rank))}, f)
    dist.barrier()
    dist.destroy_process_group()


def test_predictions_gathered_in_rank_order_gloo_world2(tmp_path):
    (tmp_path / "ann.json").write_text(json.dumps(_GATHER_DS))
    mp.spawn(_gather_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (json.loads((tmp_path / f"result.{k}").read_text()) for k in (0, 1))
    want = _gather_records(0) + _gather_records(1)                 # rank 0's records first, then rank 1's
    assert r0["gathered"] == want and r1["gathered"] is None
    # rank 0 evaluates the gathered list and writes both files; the other rank returns {} and writes nothing
    assert r1["result"] == {} and r1["seen"] == [] and not (tmp_path / "out1").exists()
    assert not (tmp_path / "saved_rank1_split.json").exists()
    assert json.loads((tmp_path / "saved_rank0_split.json").read_text()) == want
    written = json.loads((tmp_path / "out0" / "coco_instances_results.json").read_text())
    assert [(r["image_id"], r["category_id"]) for r in written] == [(8, 2), (8, 5), (3, 5)]
    assert r0["seen"] == [{"img": [1, 1, 0], "cat": [0, 1, 1]}]
    assert list(r0["result"]) == ["bbox"] and r0["result"]["bbox"]["AP"] == 100.0
    assert r0["result"]["bbox"]["AP-a"] == 100.0 and r0["result"]["bbox"]["AP-b"] == 100.0

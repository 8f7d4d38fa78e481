"""GPU: COCO bbox evaluation (sos_wsod_amd.evaluation over ops.coco_eval) against the arrays the reference's cocoeval.cpp returned
(tests/golden/coco_eval_*.npz, tests/golden/make_coco_eval_golden.py) and against the float64 NumPy restatement
(coco_eval_fixture.restated, pinned to the same fixtures by test_coco_eval_cpu.py) on random splits.  Everything is compared
bitwise: every division's operands are exact integers or the same f64 values on both sides."""
import json

import numpy as np
import pytest
import torch

import coco_eval_fixture as F
from test_coco_eval_cpu import _same, check_against_fixture

pytestmark = pytest.mark.gpu


def _inputs(ds, res):
    from sos_wsod_amd import evaluation as E
    gt = E.COCOGroundTruth(ds)
    return gt, E.COCODetections.from_results(res, gt)


def _equal(a, b):
    return all(_same(a[k], b[k]) for k in ("precision", "recall", "scores")) and a["counts"] == b["counts"]


@pytest.mark.parametrize("case", F.CASES)
def test_arrays_stats_and_results_equal_reference(golden_dir, case):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, case)
    gt, dets = _inputs(F.dataset(z), F.results(z))
    ev = E.coco_eval_arrays(gt, dets)
    stats = E.coco_summarize(ev)
    check_against_fixture(z, ev, stats, E.derive_coco_results(ev, stats, gt.thing_classes))


def _check_fuzz(ds, res, img_ids=None, **kw):
    from sos_wsod_amd import evaluation as E
    gt, dets = _inputs(ds, res)
    got, want = E.coco_eval_arrays(gt, dets, img_ids=img_ids, **kw), F.restated(ds, res, img_ids)
    for k in ("precision", "recall", "scores"):
        assert _same(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5])
    return got


def test_fuzz_against_restatement():
    rng = np.random.default_rng(21)
    for it in range(60):
        K = int(rng.choice([1, 1, 2, 3, 5, 12, 80]))
        n_img = int(rng.choice([1, 1, 2, 5, 20, 60]))
        ds, res = F.random_split(rng, n_img, K, int(rng.choice([0, 3, 30, 130])), crowd_p=float(rng.choice([0.0, 0.1, 0.5])),
                                 max_obj=int(rng.choice([0, 2, 6, 30])), one_class=bool(it % 3 == 0), no_gt=bool(it % 7 == 3),
                                 score_steps=int(rng.choice([5, 30, 1000])))
        _check_fuzz(ds, res, lds_doubles=int(rng.choice([1600, 1600, 64, 0])))
    ds, res = F.random_split(np.random.default_rng(22), 300, 4, 60, max_obj=10, score_steps=200)
    _check_fuzz(ds, res)


def test_two_runs_identical_bits(golden_dir):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "random")
    gt, dets = _inputs(F.dataset(z), F.results(z))
    a, b = E.coco_eval_arrays(gt, dets), E.coco_eval_arrays(gt, dets)
    for k in ("precision", "recall", "scores"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("case", ["hand", "random"])
def test_lds_and_workspace_paths_agree(golden_dir, case):
    """lds_doubles shrinks the slice the kernel may use: 0 sends every pair with ground truth through the global workspace"""
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, case)
    gt, dets = _inputs(F.dataset(z), F.results(z))
    full = E.coco_eval_arrays(gt, dets)
    n_ws = [int((E.coco_eval_layout(gt, dets, lds_doubles=cap)["pair_ws"] >= 0).sum()) for cap in (1600, 40, 0)]
    assert n_ws[0] < n_ws[1] < n_ws[2]
    for cap in (40, 0):
        assert _equal(full, E.coco_eval_arrays(gt, dets, lds_doubles=cap)), cap


def _call_ops(L, lds_doubles, out=None, match=None):
    from sos_wsod_amd import evaluation as E
    from sos_wsod_amd import ops

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)

    i64, f64 = torch.int64, torch.float64
    return ops.coco_eval(dev(L["pair_off"], i64), dev(L["pair_gt"], i64), dev(L["pair_ws"], i64), L["ws_words"], dev(L["det_box"], f64),
                         dev(L["gt_off"], i64), dev(L["gt_box"], f64), dev(L["gt_area"], f64), dev(L["gt_flags"], torch.uint8),
                         dev(np.asarray(E.COCO_AREA_RNG, dtype=np.float64), f64), dev(E.COCO_IOU_THRS, f64), dev(E.COCO_REC_THRS, f64),
                         dev(np.asarray(E.COCO_MAX_DETS), torch.int32), dev(L["cat_off"], i64), dev(L["order"], torch.int32),
                         dev(L["det_rank"], torch.uint8), dev(L["det_score"], f64), dev(L["npig"], i64), lds_doubles=lds_doubles,
                         out=out, match=match)


def test_every_output_slot_written_and_nothing_beyond(golden_dir):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "hand")
    gt, dets = _inputs(F.dataset(z), F.results(z))
    for cap in (1600, 0):
        L = E.coco_eval_layout(gt, dets, lds_doubles=cap)
        N, n_out = len(L["det_score"]), 2 * 10 * 101 * L["K"] * 12 + 10 * L["K"] * 12
        pad = 64
        out_buf = torch.full((n_out + 2 * pad,), float("nan"), device="cuda", dtype=torch.float64)
        match_buf = torch.full((N + 2 * pad, 2), -1, device="cuda", dtype=torch.int64)
        out, match = _call_ops(L, cap, out=out_buf[pad:pad + n_out], match=match_buf[pad:pad + N])
        host, mhost = out_buf.cpu().numpy(), match_buf.cpu().numpy()
        assert np.isnan(host[:pad]).all() and np.isnan(host[pad + n_out:]).all() and not np.isnan(host[pad:pad + n_out]).any()
        assert (mhost[:pad] == -1).all() and (mhost[pad + N:] == -1).all()
        inner = mhost[pad:pad + N]
        assert (inner >= 0).all() and (inner < (1 << 40)).all()        # 40 walks: the sentinel's high bits are gone everywhere
        n = 10 * 101 * L["K"] * 12
        assert _same(host[pad:pad + n].reshape(10, 101, L["K"], 4, 3), z["precision"])


def test_workspace_offset_outside_the_workspace_is_refused(golden_dir):
    """the kernel checks every region against the workspace's size before it touches it"""
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "hand")
    gt, dets = _inputs(F.dataset(z), F.results(z))
    L = E.coco_eval_layout(gt, dets)
    L["pair_ws"] = np.where(L["pair_ws"] >= 0, L["pair_ws"] + 1, -1)   # the last region now ends one word behind the workspace
    out, _ = _call_ops(L, 1600)
    assert np.isnan(out.cpu().numpy()).all()


def test_one_device_to_host_copy(golden_dir, monkeypatch):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "hand")
    gt, dets = _inputs(F.dataset(z), F.results(z))
    calls = []
    real = torch.Tensor.cpu

    def counting(self, *a, **k):
        calls.append(tuple(self.shape))
        return real(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", counting)
    E.coco_eval_arrays(gt, dets)
    K = len(gt.cat_ids)
    assert calls == [(2 * 10 * 101 * K * 12 + 10 * K * 12,)]


def test_img_ids_subset(golden_dir):
    z = F.load(golden_dir, "random")
    ds, res = F.dataset(z), F.results(z)
    ids = sorted(int(i) for i in z["img_ids"])
    sub = _check_fuzz(ds, res, img_ids=ids[::3] + ids[:2])
    assert not _same(sub["recall"], z["recall"])
    one = _check_fuzz(ds, res, img_ids=[ids[0]])
    assert one["counts"] == [10, 101, len(z["cat_ids"]), 4, 3]


def _model_outputs(ds, res, gt):
    """per image the Instances a model would return for the fixture's result list (XYXY boxes, contiguous classes)"""
    from sos_wsod_amd.structures import Boxes, Instances
    per = {im["id"]: [] for im in ds["images"]}
    for r in res:
        if r["category_id"] in gt.thing_dataset_id_to_contiguous_id:
            per[r["image_id"]].append(r)
    outs = {}
    for i, rs in per.items():
        b = np.asarray([r["bbox"] for r in rs], dtype=np.float64).reshape(-1, 4)
        inst = Instances((480, 640))
        inst.pred_boxes = Boxes(torch.tensor(np.concatenate([b[:, :2], b[:, :2] + b[:, 2:]], 1), dtype=torch.float64))
        inst.scores = torch.tensor([r["score"] for r in rs], dtype=torch.float64)
        inst.pred_classes = torch.tensor([gt.thing_dataset_id_to_contiguous_id[r["category_id"]] for r in rs], dtype=torch.int64)
        outs[i] = inst
    return outs


def test_evaluator_end_to_end_cli_and_pseudo_labels(golden_dir, tmp_path):
    from sos_wsod_amd import evaluation as E
    from sos_wsod_amd import pseudo_labels as PL
    z = F.load(golden_dir, "random")
    ds, res = F.dataset(z), F.results(z)
    ann = tmp_path / "instances.json"
    ann.write_text(json.dumps(ds))
    ev = E.COCOEvaluator(str(ann), output_dir=str(tmp_path / "out"), save_detection_result=True,
                         save_path=str(tmp_path / "{}.json"), name="coco_2014_minival")
    ev.reset()
    outs = _model_outputs(ds, res, ev.ground_truth())
    order = [im["id"] for im in ds["images"]]
    for k in range(0, len(order), 8):
        ev.process([{"image_id": i} for i in order[k:k + 8]], [{"instances": outs[i]} for i in order[k:k + 8]])
    got = ev.evaluate()
    # boxes went XYWH -> XYXY -> XYWH in f64: x + w - x is not always w, so the yardstick is the written result file
    written = json.loads((tmp_path / "out" / "coco_instances_results.json").read_text())
    want_ev = F.restated(ds, written)
    want_stats = F.summarize(want_ev)
    want = F.derive(want_ev, want_stats, ev.ground_truth().thing_classes)
    assert list(got) == ["bbox"] and list(got["bbox"]) == list(want)
    assert all(_same(got["bbox"][k], want[k]) for k in want) and _same(ev.stats, want_stats) and _equal(ev.eval, want_ev)
    cli = E.main(["--coco-json", str(ann), "--detections", str(tmp_path / "out" / "coco_instances_results.json"),
                  "--out", str(tmp_path / "m.json")])
    assert all(_same(cli["bbox"][k], want[k]) for k in want)
    assert _same(json.loads((tmp_path / "m.json").read_text())["stats"], want_stats)
    # Stage 2 takes the saved detection file as it is
    saved = json.loads((tmp_path / "coco_2014_minival.json").read_text())
    cont = ev.ground_truth().thing_dataset_id_to_contiguous_id
    dicts = [{"image_id": im["id"], "annotations": [{"category_id": cont[a["category_id"]]} for a in ds["annotations"]
                                                    if a["image_id"] == im["id"]]} for im in ds["images"]]
    result, stats = PL.pgf_coco(saved, dicts)
    assert stats["before_class_filter"] == len(written) and 0 < stats["after_containment"] <= stats["after_class_filter"]
    assert set(result) == {im["id"] for im in ds["images"]}


def test_inference_on_dataset_with_stub_model(golden_dir, tmp_path):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "hand")
    ds, res = F.dataset(z), F.results(z)
    ann = tmp_path / "instances.json"
    ann.write_text(json.dumps(ds))
    ev = E.COCOEvaluator(str(ann))
    outs = _model_outputs(ds, res, ev.ground_truth())

    class Stub(torch.nn.Module):
        def forward(self, inputs):
            assert not self.training and not torch.is_grad_enabled()
            return [{"instances": outs[inp["image_id"]]} for inp in inputs]

    model = Stub().train()
    got = E.inference_on_dataset(model, [[{"image_id": im["id"]}] for im in ds["images"]], ev)
    assert model.training and list(got) == ["bbox"]
    flat = [r for p in ev._predictions for r in p["instances"]]
    rev = {v: k for k, v in ev.ground_truth().thing_dataset_id_to_contiguous_id.items()}
    want_ev = F.restated(ds, [dict(r, category_id=rev[r["category_id"]]) for r in flat])
    assert _equal(ev.eval, want_ev) and np.isnan(got["bbox"]["APl"]) and got["bbox"]["AP"] > 0
    # not compared with the fixture's stats: the records come in image order, not the fixture's list order (ties rank by it), and
    # y + h - y in float64 does not give h back for every box of the hand case (100 + 7.4 - 100)

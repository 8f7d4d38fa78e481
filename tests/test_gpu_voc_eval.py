"""GPU: VOC mAP and CorLoc (sos_wsod_amd.evaluation over ops.voc_eval) against the reference's own numbers
(tests/golden/voc_eval_*.npz, tests/golden/make_voc_eval_golden.py) and against a float64 NumPy restatement of the reference
(voc_eval_fixture.restated) on random splits."""
import json

import numpy as np
import pytest
import torch

import voc_eval_fixture as F

pytestmark = pytest.mark.gpu


def _same(a, b):
    """equal bits; a NaN matches a NaN (x86 numpy makes 0 / 0 a NaN with the sign bit set, the GPU one without)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.where(np.isnan(a), 0.0, a).tobytes() == np.where(np.isnan(b), 0.0, b).tobytes()


def _arrays(z, root):
    from sos_wsod_amd import evaluation as E
    gt = E.GroundTruth.load(F.write_devkit(z, root), F.SPLIT, F.CLASS_NAMES)
    return gt, E.Detections.from_lines(F.lines(z), gt)


@pytest.mark.parametrize("case", F.CASES)
def test_per_class_ap_and_corloc_equal_reference(golden_dir, tmp_path, case):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, case)
    gt, dets = _arrays(z, tmp_path / "VOC2007")
    full = case != "npos0"
    res = E.voc_eval_arrays(gt, dets, corloc=full)
    for k in ("ap_07", "ap_area"):
        for c in range(len(F.CLASS_NAMES)):
            assert _same(res[k][c], z[k][c]), (case, k, F.CLASS_NAMES[c], res[k][c], z[k][c])
    if full:
        assert _same(res["corloc"], z["corloc"]), (case, np.argwhere(res["corloc"] != z["corloc"]))
    else:
        assert np.isnan(z["ap_area"][0]).all() and (z["ap_07"][0] == 0).all()      # npos == 0 with detections


@pytest.mark.parametrize("case", ["hand", "random", "noties"])
def test_evaluate_dict_equals_reference(golden_dir, tmp_path, case):
    from sos_wsod_amd import evaluation as E
    from sos_wsod_amd.inference import VOCDetectionWriter
    z = F.load(golden_dir, case)
    root = F.write_devkit(z, tmp_path / "VOC2007")
    for year in (2007, 2012):
        ev = E.PascalVOCDetectionEvaluator(root, F.SPLIT, year, class_names=F.CLASS_NAMES)
        ev.reset()
        ev._writer = VOCDetectionWriter.from_lines(F.lines(z))
        got = ev.evaluate()
        want = F.result_dict(z, year)
        for a, b in F.DICT_KEYS:
            assert _same(got[a][b], want[a][b]), (case, year, a, b, got[a][b], want[a][b])
        metric = "ap_07" if year == 2007 else "ap_area"
        assert _same(ev.per_class_ap, z[metric]) and _same(ev.per_class_corloc, z["corloc"])


def _instances(rng, n, names, K):
    from sos_wsod_amd.structures import Boxes, Instances
    inputs, outputs = [], []
    for name in names:
        m = int(rng.integers(0, n + 1))
        xy = rng.uniform(0, 300, (m, 2))
        wh = rng.uniform(1, 150, (m, 2))
        inst = Instances((375, 500))
        inst.pred_boxes = Boxes(torch.tensor(np.concatenate([xy, xy + wh], 1), dtype=torch.float32))
        inst.scores = torch.tensor(rng.random(m).round(3), dtype=torch.float32)
        inst.pred_classes = torch.tensor(rng.integers(0, K, m), dtype=torch.int64)
        inputs.append({"image_id": name})
        outputs.append({"instances": inst})
    return inputs, outputs


def _random_tree(rng, root, n_img, K, name_of=lambda i: f"{i + 1:06d}"):
    import os
    os.makedirs(root / "Annotations")
    os.makedirs(root / "ImageSets" / "Main")
    names = [name_of(i) for i in range(n_img)]
    objs = []
    for n in names:
        o = []
        for _ in range(int(rng.integers(0, 5))):
            x1, y1 = int(rng.integers(1, 300)), int(rng.integers(1, 300))
            o.append((int(rng.integers(0, K)), [x1, y1, x1 + int(rng.integers(0, 150)), y1 + int(rng.integers(0, 150))],
                      int(rng.random() < 0.15)))
        objs.append(o)
        (root / "Annotations" / f"{n}.xml").write_text(F._xml(
            [{"name": F.CLASS_NAMES[c], "pose": "Unspecified", "truncated": 0, "difficult": d, "bbox": b} for c, b, d in o]))
    (root / "ImageSets" / "Main" / "test.txt").write_text("".join(n + "\n" for n in names))
    return names, objs


def test_process_instances_equals_cli_on_dumped_json(tmp_path):
    from sos_wsod_amd import evaluation as E
    rng = np.random.default_rng(3)
    names, _ = _random_tree(rng, tmp_path / "VOC2007", 40, 20)
    ev = E.PascalVOCDetectionEvaluator(str(tmp_path / "VOC2007"), "test", 2007, save_detection_result=True,
                                       save_path=str(tmp_path / "{}.json"))
    ev.reset()
    inputs, outputs = _instances(rng, 30, names, 20)
    gt = ev.ground_truth()
    keep = [k for k in range(20) if gt.npos_im[k] > 0]
    for o in outputs:                                 # classes without a non-difficult object have undefined CorLoc
        inst = o["instances"]
        sel = torch.tensor([int(c) in keep for c in inst.pred_classes.tolist()], dtype=torch.bool)
        inst.pred_boxes.tensor = inst.pred_boxes.tensor[sel]
        inst.scores = inst.scores[sel]
        inst.pred_classes = inst.pred_classes[sel]
    for k in range(0, len(inputs), 8):
        ev.process(inputs[k:k + 8], outputs[k:k + 8])
    got = ev.evaluate()
    dumped = tmp_path / "voc_2007_test.json"
    assert dumped.exists()
    cli = E.main(["--voc-root", str(tmp_path / "VOC2007"), "--split", "test", "--year", "2007", "--detections", str(dumped),
                  "--out", str(tmp_path / "m.json")])
    for a, b in F.DICT_KEYS:
        assert _same(got[a][b], cli[a][b]), (a, b)
    saved = json.loads((tmp_path / "m.json").read_text())
    assert np.array_equal(np.array(saved["per_class"]["AP"]), ev.per_class_ap, equal_nan=True)


def _fuzz_split(rng, n_img, K, n_det, n_obj=(0, 5), tie_scores=True):
    objs = []
    for i in range(n_img):
        o = []
        for _ in range(int(rng.integers(n_obj[0], n_obj[1] + 1))):
            x1, y1 = int(rng.integers(1, 200)), int(rng.integers(1, 200))
            o.append((int(rng.integers(0, K)), [x1, y1, x1 + int(rng.integers(-1, 80)), y1 + int(rng.integers(-1, 80))],
                      int(rng.random() < 0.2)))
        objs.append(o)
    dets = []
    for c in range(K):
        n = int(rng.integers(0, n_det + 1))
        img = rng.integers(0, n_img, n)
        score = (rng.integers(0, 30 if tie_scores else 1000, n) / (30 if tie_scores else 1000)).round(3)
        box = np.empty((n, 4))
        for d in range(n):
            g = [o for o in objs[img[d]] if o[0] == c]
            if g and rng.random() < 0.7:
                b = np.array(g[int(rng.integers(0, len(g)))][1], dtype=np.float64) + rng.integers(-60, 61, 4) / 10
            else:
                x, y = rng.integers(0, 2000, 2) / 10
                b = np.array([x, y, x + rng.integers(0, 800) / 10, y + rng.integers(0, 800) / 10])
            box[d] = b.round(1)
        if n and rng.random() < 0.1:
            box[int(rng.integers(0, n)), int(rng.integers(0, 4))] = np.nan
        dets.append((img, score, box))
    return objs, dets


def _check_fuzz(objs, dets, K, detail=None):
    """detail: a list that receives the restatement's per-class intermediates (voc_eval_fixture.restated_detail)"""
    from sos_wsod_amd import evaluation as E
    names = [f"{i:06d}" for i in range(len(objs))]
    recs = {n: [{"name": F.CLASS_NAMES[c], "pose": "Unspecified", "truncated": 0, "difficult": d, "bbox": b} for c, b, d in o]
            for n, o in zip(names, objs)}
    gt = E.GroundTruth(names, recs, F.CLASS_NAMES[:K])
    corloc = all(gt.npos_im[c] > 0 or len(dets[c][0]) == 0 for c in range(K))
    res = E.voc_eval_arrays(gt, E.Detections(dets), corloc=corloc)
    a07, aar, cl, per_class = F.restated_detail(objs, len(objs), dets, K, corloc=corloc)
    if detail is not None:
        detail.extend(per_class)
    assert _same(res["ap_07"], a07), np.argwhere(res["ap_07"] != a07)
    assert _same(res["ap_area"], aar), np.argwhere((res["ap_area"] != aar) & ~(np.isnan(aar) & np.isnan(res["ap_area"])))
    if corloc:
        assert _same(res["corloc"], cl), np.argwhere(res["corloc"] != cl)
    return res


def test_fuzz_small_splits_against_restatement():
    rng = np.random.default_rng(11)
    for it in range(300):
        K = int(rng.integers(1, 6))
        objs, dets = _fuzz_split(rng, int(rng.integers(1, 25)), K, int(rng.integers(0, 60)), tie_scores=bool(it % 2))
        _check_fuzz(objs, dets, K)


def test_fuzz_large_class_against_restatement():
    """tens of thousands of detections in a class, more than 8192 recall change points (np.sum's buffer chunks)"""
    rng = np.random.default_rng(12)
    n_img, K = 2500, 2
    objs = [[(0, [10 + k * 30, 10, 30 + k * 30, 40], 0) for k in range(4)] + [(1, [5, 5, 60, 60], int(i % 3 == 0))]
            for i in range(n_img)]
    dets = []
    for c, n in ((0, 30000), (1, 5000)):
        img = rng.integers(0, n_img, n)
        score = (rng.integers(0, 1000, n) / 1000).round(3)
        slot = rng.integers(0, 4, n)
        hit = rng.random(n) < 0.8
        box = np.where(hit[:, None], np.stack([10 + slot * 30, np.full(n, 10), 30 + slot * 30, np.full(n, 40)], 1).astype(float),
                       np.array([200.0, 200.0, 260.0, 260.0]))
        if c == 1:
            box = np.where(hit[:, None], np.array([5.0, 5.0, 60.0, 60.0]), box)
        dets.append((img, score, box + rng.integers(-10, 11, (n, 4)) / 10))
    detail = []
    res = _check_fuzz(objs, dets, K, detail)
    assert res["ap_area"][0, 0] > 0
    assert len(detail[0]["terms"][0]) > 8192, len(detail[0]["terms"][0])       # the change points of class 0 at IoU 0.5


def test_two_runs_identical_bits(golden_dir, tmp_path):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "random")
    gt, dets = _arrays(z, tmp_path / "VOC2007")
    a = E.voc_eval_arrays(gt, dets)
    b = E.voc_eval_arrays(gt, dets)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_one_device_to_host_copy(golden_dir, tmp_path, monkeypatch):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "hand")
    gt, dets = _arrays(z, tmp_path / "VOC2007")
    calls = []
    real = torch.Tensor.cpu

    def counting(self, *a, **k):
        calls.append(tuple(self.shape))
        return real(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", counting)
    E.voc_eval_arrays(gt, dets)
    assert calls == [(3, len(F.CLASS_NAMES), 10)]


def test_inference_on_dataset_with_stub_model(golden_dir, tmp_path):
    from sos_wsod_amd import evaluation as E
    from sos_wsod_amd.structures import Boxes, Instances
    z = F.load(golden_dir, "hand")
    root = F.write_devkit(z, tmp_path / "VOC2007")
    cls, img, score, box = F.detections(z)
    nm = list(dict.fromkeys(F.names(z)))

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.seen = []

        def forward(self, inputs):
            assert not self.training and not torch.is_grad_enabled()
            outs = []
            for inp in inputs:
                i = nm.index(inp["image_id"])
                sel = img == i
                b = box[sel].copy()
                b[:, :2] -= 1                         # the evaluator adds the +1 back
                inst = Instances((500, 500))
                inst.pred_boxes = Boxes(torch.tensor(b, dtype=torch.float64))
                inst.scores = torch.tensor(score[sel], dtype=torch.float64)
                inst.pred_classes = torch.tensor(cls[sel])
                outs.append({"instances": inst})
                self.seen.append(i)
            return outs

    model = Stub().train()
    loader = [[{"image_id": nm[i]}] for i in range(len(nm))]
    ev = E.PascalVOCDetectionEvaluator(root, F.SPLIT, 2012, class_names=F.CLASS_NAMES)
    got = E.inference_on_dataset(model, loader, ev)
    assert model.training and model.seen == list(range(len(nm)))
    # the same lines as the fixture's, in image order rather than the fixture's line order (so ties may rank differently)
    fixture_lines = F.lines(z)
    assert all(sorted(ev._writer.lines()[k]) == sorted(fixture_lines[k]) for k in range(len(F.CLASS_NAMES)))
    assert set(got) == {"bbox", "bbox CorLoc"}
    want = E.voc_eval_arrays(ev.ground_truth(), E.Detections.from_lines(ev._writer.lines(), ev.ground_truth()))
    assert _same(ev.per_class_ap, want["ap_area"]) and _same(ev.per_class_corloc, want["corloc"])
    assert _same(got["bbox"]["AP50"], np.mean(want["ap_area"][:, 0].tolist()))

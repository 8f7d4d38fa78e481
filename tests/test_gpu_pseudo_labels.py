"""GPU: Stage-2 pseudo-ground-truth filtering (sos_wsod_amd.pseudo_labels over ops.pgf_keep) against the reference's own outputs
(tests/golden/pgf_{voc,coco}.npz, tests/golden/make_pgf_golden.py) and against a float64 NumPy restatement of the reference loops."""
import json

import numpy as np
import pytest

import pgf_fixture as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(F.CASES))
def test_outputs_equal_reference_bytes(golden_dir, case):
    from sos_wsod_amd import pseudo_labels as P
    voc = F.CASES[case] == "voc"
    z = F.load(golden_dir, F.CASES[case])
    t_con, t_keep, use_diff = F.params(z, case)
    for s in F.SPLITS:
        gt = F.gt_dicts(z, s, voc)
        if voc:
            det = F.voc_records(z, s)
            result, stats = P.pgf_voc(det, gt, t_con, t_keep, use_diff)
            text = json.dumps(result)
            assert [r["category_id"] for r in det] == (z[f"{s}_det_cat"] - 1).tolist()                # mutated in place
        else:
            result, stats = P.pgf_coco(F.coco_records(z, s), gt, t_con, t_keep, use_diff)
            text = json.dumps(P.coco_pseudo_labels(F.coco_base(z, s), result))
        assert [stats[k] for k in P.STAT_KEYS] == z[f"{case}_{s}_counts"].tolist(), (case, s, stats)
        assert F.sha256(text) == str(z[f"{case}_{s}_sha256"]), (case, s)


def test_multi_label_and_loader_on_gpu_output(golden_dir):
    from sos_wsod_amd import pseudo_labels as P
    z = F.load(golden_dir, "voc")
    for s in F.SPLITS:
        gt = F.gt_dicts(z, s, voc=True)
        result, _ = P.pgf_voc(F.voc_records(z, s), gt, *F.params(z, "voc_a"))
        pgt = P.add_multi_label(result, gt)
        assert F.sha256(json.dumps(pgt)) == str(z[f"voc_a_{s}_multi_label_sha256"])
        dicts = P.load_voc_pseudo_labels(json.loads(json.dumps(pgt)), F.voc_images(z, s))
        assert F.sha256(json.dumps(dicts)) == str(z[f"voc_a_{s}_dicts_sha256"])


def test_cli_writes_reference_files(golden_dir, tmp_path):
    from sos_wsod_amd import pseudo_labels as P
    z = F.load(golden_dir, "voc")
    (tmp_path / "det").mkdir()
    for s in F.SPLITS:
        (tmp_path / "det" / f"oicr_plus_voc_2007_{s}.json").write_text(json.dumps(F.voc_records(z, s)))
    (tmp_path / "gt.json").write_text(json.dumps({f"voc_2007_{s}": F.gt_dicts(z, s, voc=True) for s in F.SPLITS}))
    P.main(["--det-path", str(tmp_path / "det"), "--save-path", str(tmp_path / "out"), "--gt-dicts", str(tmp_path / "gt.json"),
            "--t-con", "0.85", "--t-keep", "0.2"])
    for s in F.SPLITS:
        assert F.sha256((tmp_path / "out" / f"oicr_plus_voc_2007_{s}.json").read_text()) == str(z[f"voc_a_{s}_sha256"])


def test_one_device_to_host_copy_per_split(golden_dir, monkeypatch):
    import torch
    from sos_wsod_amd import pseudo_labels as P
    z = F.load(golden_dir, "coco")
    copies = []
    orig = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        if self.is_cuda:
            copies.append(self.numel())
        return orig(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    P.pgf_coco(F.coco_records(z, "train"), F.gt_dicts(z, "train", voc=False), use_diff=True)
    assert len(copies) == 1


def test_non_finite_input_rejected(golden_dir):
    from sos_wsod_amd import pseudo_labels as P
    z = F.load(golden_dir, "voc")
    for field, bad in (("score", float("nan")), ("bbox", [1.0, 2.0, float("inf"), 4.0])):
        det = F.voc_records(z, "train")
        det[-1][field] = bad
        with pytest.raises(ValueError):
            P.pgf_voc(det, F.gt_dicts(z, "train", voc=True))


def test_coco_without_use_diff_rejected():
    from sos_wsod_amd import pseudo_labels as P
    with pytest.raises(ValueError):
        P.pgf_coco([], [], use_diff=False)


# ---- float64 NumPy restatement of class_filter + pgf (tools/pgf.py:221-292), kept with the test -------------------------------
def reference_keep(off, boxes, scores, classes, gt_sets, diff_set, t_keep, t_con, use_diff):
    keep = np.zeros(len(scores), dtype=bool)
    counts = [len(scores), 0, 0, 0]
    for k in range(len(off) - 1):
        a, b = off[k], off[k + 1]
        cls = classes[a:b]
        s1 = np.array([c in gt_sets[k] for c in cls], dtype=bool)
        idx = np.nonzero(s1)[0]
        seen, s4 = set(), np.zeros(b - a, dtype=bool)
        for i in idx:
            if cls[i] not in seen:
                seen.add(cls[i]); s4[i] = True
            else:
                s4[i] = not (scores[a + i] < t_keep)
        bx = boxes[a:b].copy()
        x2, y2 = bx[:, 0] + bx[:, 2], bx[:, 1] + bx[:, 3]
        cx1 = np.where(bx[None, :, 0] > bx[:, None, 0], bx[None, :, 0], bx[:, None, 0])      # Python max(a_i, b_j)
        cy1 = np.where(bx[None, :, 1] > bx[:, None, 1], bx[None, :, 1], bx[:, None, 1])
        cx2 = np.where(x2[None, :] < x2[:, None], x2[None, :], x2[:, None])                   # Python min(a_i, b_j)
        cy2 = np.where(y2[None, :] < y2[:, None], y2[None, :], y2[:, None])
        w, h = cx2 - cx1, cy2 - cy1
        area_c = np.where(w > 0, w, 0.0) * np.where(h > 0, h, 0.0)
        aw, ah = x2 - bx[:, 0], y2 - bx[:, 1]
        area_a = np.where(aw > 0, aw, 0.0) * np.where(ah > 0, ah, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = area_c / (area_a + 1e-6)[:, None]
        pair = (cls[:, None] == cls[None, :]) & s4[None, :] & ~np.eye(b - a, dtype=bool) & (ratio >= t_con)
        exempt = np.array([(not use_diff) and c in diff_set for c in cls], dtype=bool)
        out = s4 & ~(pair.any(axis=1) & ~exempt)
        keep[a:b] = out
        counts[1] += int(s1.sum()); counts[2] += int(s4.sum()); counts[3] += int(out.sum())
    return keep, counts


def _random_split(rng, n_img, K):
    sizes = rng.integers(0, 60, n_img)
    sizes[rng.random(n_img) < 0.05] = 0                                           # empty images
    big = rng.choice(n_img, 6, replace=False)
    sizes[big] = rng.integers(257, 700, 6)                                        # over the LDS stage
    sizes[big[0]] = 256                                                           # exactly at it
    off = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    n = int(off[-1])
    g = rng.integers(0, 4, (n, 4)) * 16.0                                          # coarse grid: duplicates, nesting, ratio 1
    fine = rng.uniform(-5, 300, (n, 4)).round(1)
    boxes = np.where((rng.random(n) < 0.5)[:, None], g, fine)
    boxes[:, 2:] = np.where(rng.random((n, 2)) < 0.03, 0.0, boxes[:, 2:])          # zero extent
    scores = rng.random(n).round(3)
    gt_sets = [set(rng.choice(K, rng.integers(1, 4), replace=False).tolist()) for _ in range(n_img)]
    classes = np.empty(n, dtype=np.int32)
    for k in range(n_img):
        a, b = off[k], off[k + 1]
        own = np.array(sorted(gt_sets[k]))
        classes[a:b] = np.where(rng.random(b - a) < 0.75, rng.choice(own, b - a), rng.integers(0, K, b - a))
    return off, boxes, scores, classes, gt_sets


@pytest.mark.parametrize("K,use_diff,t_keep,t_con", [(80, True, 0.2, 0.85), (20, False, 0.3, 0.7), (256, True, 0.0, 0.999999)])
def test_keep_flags_equal_float64_restatement(K, use_diff, t_keep, t_con):
    import torch
    from sos_wsod_amd import ops
    rng = np.random.default_rng(K)
    n_img = 10000
    off, boxes, scores, classes, gt_sets = _random_split(rng, n_img, K)
    diff_set = {4, 5, 6, 8, 9, 15, 16}
    words = (K + 31) // 32
    gt_mask = np.zeros((n_img, words), dtype=np.uint32)
    for k, s in enumerate(gt_sets):
        for c in s:
            gt_mask[k, c >> 5] |= np.uint32(1 << (c & 31))
    diff_mask = np.zeros(words, dtype=np.uint32)
    for c in diff_set:
        diff_mask[c >> 5] |= np.uint32(1 << (c & 31))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    packed = ops.pgf_keep(up(off), up(boxes), up(scores), up(classes), K, up(gt_mask.view(np.int32)), up(diff_mask.view(np.int32)),
                          t_keep, t_con, use_diff)
    host = packed.cpu().numpy()
    keep_ref, counts_ref = reference_keep(off, boxes, scores, classes, gt_sets, diff_set, t_keep, t_con, use_diff)
    assert host[:32].view(np.int64).tolist() == counts_ref
    keep = host[32:].astype(bool)
    bad = np.nonzero(keep != keep_ref)[0]
    assert bad.size == 0, f"{bad.size} flags differ, first at {bad[:5]}"
    assert counts_ref[3] > 0 and counts_ref[2] > counts_ref[3]                     # both stages drop something

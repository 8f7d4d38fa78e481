"""GPU: proposal recall (sos_wsod_amd.proposal_recall over ops.proposal_recall) against the numbers the reference's own script
printed (tests/golden/proposal_*.npz, tests/golden/make_proposal_golden.py) and against a float64 NumPy restatement
(proposal_fixture.restated) on random splits.  Everything is compared bit for bit."""
import json

import numpy as np
import pytest
import torch

import proposal_fixture as F

pytestmark = pytest.mark.gpu


def _read(PR, z, path):
    mode = str(z["mode"])
    if mode == "mcg":
        return PR.read_mcg_dir(F.records(z), path, F.name_of(z))
    return PR.read_eb_mat(path) if mode == "eb" else PR.read_ss_mat(path)


@pytest.mark.parametrize("case", F.CASES)
def test_recall_and_matches_equal_reference(golden_dir, tmp_path, case):
    from sos_wsod_amd import proposal_recall as PR
    z = F.load(golden_dir, case)
    mode = str(z["mode"])
    p = _read(PR, z, F.write_mats(z, str(tmp_path / "mat")))
    rng = np.random.RandomState(int(z["seed"])) if mode == "ss" else None
    res = PR.proposal_recall(F.records(z), p, F.name_of(z), mode=mode, rng=rng, return_matches=True)
    G = int(z["gt_off"][-1])
    assert res["cnt_gt"] == G and res["ovmax"].shape == (G, 10) and res["jmax"].dtype == np.int32
    assert F.same(res["ovmax"].T, z["ovmax"]), (case, np.argwhere(res["ovmax"].T != z["ovmax"])[:5])
    assert np.array_equal(res["jmax"].T, z["jmax"]), (case, np.argwhere(res["jmax"].T != z["jmax"])[:5])
    assert F.same(res["recall"], z["recall"]) and res["recall"].shape == (10, 11)
    assert np.array_equal(res["cnt_yes"], np.rint(z["recall"] * G).astype(np.int64)) and res["cnt_yes"].dtype == np.int64
    if case == "handcoco":
        assert np.isnan(res["ovmax"][0, 1:]).all() and res["ovmax"][0, 0] == z["ovmax"][0, 0]      # NaN from the cut that holds it


@pytest.mark.parametrize("case", ["hand", "random"])
def test_converted_pickle_equals_restatement(golden_dir, tmp_path, case):
    """mode "pkl": the int16 boxes of the converted file, matched to the records by image id (given here in reverse order)"""
    from sos_wsod_amd import proposal_recall as PR
    z = F.load(golden_dir, case)
    recs = F.records(z)
    out = str(tmp_path / "p.pkl")
    PR.convert_mcg_box(recs[::-1], F.write_mats(z, str(tmp_path / "mat")), out, F.name_of(z))
    p = PR.read_proposal_pkl(out)
    assert p["ids"] == [d["image_id"] for d in recs[::-1]]
    p["scores"] = [np.atleast_1d(s) for s in p["scores"]]
    res = PR.proposal_recall(recs, p, F.name_of(z), mode="pkl", return_matches=True)
    ov, jm, cnt, recall = F.restated(recs, F.ranked(p["boxes"][::-1], p["scores"][::-1]), F.name_of(z))
    assert F.same(res["ovmax"], ov) and np.array_equal(res["jmax"], jm) and np.array_equal(res["cnt_yes"], cnt)
    assert F.same(res["recall"], recall)


def _split(seed, n_img, max_props, dtype, grid, size=300):
    """a random split: coordinates on a coarse grid (many equal overlaps, duplicates) or fine; some images without objects; for an
    unsigned dtype some xmin at the dtype's maximum, as a file's 0 becomes after `- 1` (the width then wraps)"""
    rng = np.random.default_rng(seed)
    recs, boxes, scores = [], [], []
    for k in range(n_img):
        n_gt = 0 if k % 7 == 3 else int(rng.integers(1, 6))
        xy = rng.integers(0, size // grid, (n_gt, 2)) * grid
        gt = np.concatenate([xy, xy + rng.integers(1, 2 * size // (3 * grid), (n_gt, 2)) * grid], 1).astype(np.float64)
        n = max_props if k == 1 else int(rng.integers(1, min(max_props, 150)))
        pxy = rng.integers(0, size // grid, (n, 2)) * grid
        b = np.concatenate([pxy, pxy + rng.integers(1, 2 * size // (3 * grid), (n, 2)) * grid], 1)
        if n_gt and n > 3:
            b[rng.integers(0, n, 3)] = gt[0]                                  # IoU exactly 1.0, three times
        if np.dtype(dtype).kind == "u":
            b[rng.integers(0, n, 2), 0] = np.iinfo(dtype).max
        recs.append({"file_name": f"{k}.jpg", "image_id": k, "annotations": [{"bbox": [float(v) for v in g]} for g in gt]})
        boxes.append(b.astype(dtype) + (0.125 if dtype == np.float64 and not k % 2 else 0))
        scores.append(rng.permutation(n).astype(np.float64))
    return recs, boxes, scores


@pytest.mark.parametrize("seed,n_img,max_props,dtype,grid,size,budgets", [
    (1, 33, 3100, np.float64, 20, 300, (1, 3, 63, 64, 65, 1000, 1024, 1025, 2047, 3000)),      # three LDS passes, cuts at their edges
    (2, 64, 1300, np.int16, 25, 300, F.BUDGETS),
    (3, 17, 2049, np.int32, 1, 300, (2048, 2049)),
    (4, 9, 60, np.uint8, 10, 150, (2, 7, 60)),
])
def test_random_splits_equal_restatement(seed, n_img, max_props, dtype, grid, size, budgets):
    from sos_wsod_amd import proposal_recall as PR
    recs, boxes, scores = _split(seed, n_img, max_props, dtype, grid, size)
    thr = (0.0, 0.3, 0.5, 1.0)
    res = PR.proposal_recall(recs, {"boxes": boxes, "scores": scores}, "synthetic", budgets=budgets, thresholds=thr, mode="eb",
                             return_matches=True)
    ov, jm, cnt, recall = F.restated(recs, F.ranked(boxes, scores, budgets[-1]), "synthetic", budgets, thr)
    assert F.same(res["ovmax"], ov), np.argwhere(res["ovmax"] != ov)[:5]
    assert np.array_equal(res["jmax"], jm), np.argwhere(res["jmax"] != jm)[:5]
    assert np.array_equal(res["cnt_yes"], cnt) and F.same(res["recall"], recall)
    assert (ov == 1.0).any() and 0 < cnt[0, 2] and cnt[0, 3] < len(ov)


def _device_arrays(recs, lists, name="synthetic"):
    gts = F.gt_xyxy(recs, name)
    gt_off = np.cumsum([0] + [len(g) for g in gts]).astype(np.int64)
    gt_box = np.array([b for g in gts for b in g], dtype=np.float64).reshape(-1, 4)
    prop_off = np.cumsum([0] + [len(b) for b in lists]).astype(np.int64)
    prop_box = np.concatenate(lists).astype(np.float64)
    return [torch.from_numpy(a).cuda() for a in (prop_off, prop_box, gt_off, gt_box)]


def _t(values, dtype):
    return torch.tensor(values, dtype=dtype, device="cuda")


def test_one_launch_equals_single_cut_launches_and_repeats_itself():
    from sos_wsod_amd import ops
    recs, boxes, scores = _split(5, 40, 2500, np.float64, 20)
    dev = _device_arrays(recs, F.ranked(boxes, scores, 4096))
    thr = _t(F.THRESHOLDS, torch.float64)
    ov, jm, cnt = ops.proposal_recall(*dev, _t(F.BUDGETS, torch.int32), thr)
    for k, m in enumerate(F.BUDGETS):
        o1, j1, c1 = ops.proposal_recall(*dev, _t([m], torch.int32), thr)
        assert torch.equal(o1[:, 0].view(torch.int64), ov[:, k].view(torch.int64)) and torch.equal(j1[:, 0], jm[:, k]), m
        assert torch.equal(c1[0], cnt[k]), m
    ov2, jm2, cnt2 = ops.proposal_recall(*dev, _t(F.BUDGETS, torch.int32), thr)
    assert torch.equal(ov2.view(torch.int64), ov.view(torch.int64)) and torch.equal(jm2, jm) and torch.equal(cnt2, cnt)
    assert 0 < int(cnt[0, 0]) < int(cnt[-1, 0])


@pytest.mark.parametrize("cuts", [(5,), tuple(range(1, 32, 2)), (1, 2, 3, 4, 5, 6, 7, 8, 100, 200, 1023, 1024, 1025, 1500, 2000, 2600)])
def test_cut_counts_and_untouched_padding(cuts):
    """n_cut = 1 and 16, 16 thresholds; the rows past the ground truth keep their sentinels"""
    from sos_wsod_amd import ops
    recs, boxes, scores = _split(6, 21, 2600, np.float64, 20)
    lists = F.ranked(boxes, scores, cuts[-1])
    dev = _device_arrays(recs, lists)
    thr = tuple(np.linspace(0.05, 1.0, 16).tolist())
    G, pad = dev[3].shape[0], 5
    ov = torch.full((G + pad, len(cuts)), -7.5, dtype=torch.float64, device="cuda")
    jm = torch.full((G + pad, len(cuts)), -77, dtype=torch.int32, device="cuda")
    o, j, cnt = ops.proposal_recall(*dev, _t(cuts, torch.int32), _t(thr, torch.float64), ovmax=ov, jmax=jm)
    assert o is ov and j is jm and cnt.shape == (len(cuts), 16)
    want_ov, want_jm, want_cnt, _ = F.restated(recs, lists, "synthetic", cuts, thr)
    assert F.same(ov[:G].cpu().numpy(), want_ov) and np.array_equal(jm[:G].cpu().numpy(), want_jm)
    assert np.array_equal(cnt.cpu().numpy(), want_cnt)
    assert (ov[G:] == -7.5).all() and (jm[G:] == -77).all()


def test_cli_prints_the_same_table_for_the_mat_directory_and_its_pickle(golden_dir, tmp_path, capsys):
    import scipy.io as sio
    import voc_eval_fixture as V
    from sos_wsod_amd import proposal_recall as PR
    z = V.load(golden_dir, "hand")
    root = V.write_devkit(z, tmp_path / "VOC2007")
    recs = PR.voc_records(root, V.SPLIT)
    rng = np.random.default_rng(9)
    (tmp_path / "mcg").mkdir()
    for d in recs:
        n = int(rng.integers(3, 90))
        xy = rng.integers(1, 300, (n, 2))
        b = np.concatenate([xy, xy + rng.integers(5, 150, (n, 2))], 1)
        for k, a in enumerate(d["annotations"][:2]):
            b[k] = np.asarray(a["bbox"]) + [2, 2, 1, 1] + rng.integers(-4, 5, 4)          # file coordinates are 1-based
        sio.savemat(str(tmp_path / "mcg" / f"{d['image_id']}.mat"),
                    {"boxes": np.maximum(b, 1)[:, (1, 0, 3, 2)].astype(np.uint16), "scores": rng.permutation(n).reshape(-1, 1) / n})
    gt = ["--voc-root", root, "--split", V.SPLIT]
    PR.main(["convert", "--mode", "mcg", "--proposals", str(tmp_path / "mcg"), "--out", str(tmp_path / "p.pkl")] + gt)
    capsys.readouterr()
    a = PR.main(["recall", "--mode", "mcg", "--proposals", str(tmp_path / "mcg"), "--out", str(tmp_path / "a.json")] + gt)
    table_mat = capsys.readouterr().out
    b = PR.main(["recall", "--mode", "pkl", "--proposals", str(tmp_path / "p.pkl")] + gt)
    table_pkl = capsys.readouterr().out
    assert table_mat == table_pkl and F.same(a["recall"], b["recall"])
    lines = table_mat.splitlines()
    assert len(lines) == 11 and all(len(x.split()) == 12 for x in lines)                  # the budget and eleven thresholds
    saved = json.loads((tmp_path / "a.json").read_text())
    assert saved["recall"] == a["recall"].tolist() and saved["dataset"] == "voc_2007_val" and saved["budgets"] == list(F.BUDGETS)
    assert 0 < a["recall"][0, 0] < a["recall"][-1, 0] <= 1


@pytest.mark.parametrize("cuts", [(8, 4), (4, 4), (0, 4)])
def test_cuts_out_of_order_are_refused_before_the_launch(cuts):
    from sos_wsod_amd import ops
    recs, boxes, scores = _split(7, 3, 20, np.float64, 20)
    dev = _device_arrays(recs, F.ranked(boxes, scores, 8))
    with pytest.raises(AssertionError, match="strictly ascending"):
        ops.proposal_recall(*dev, _t(cuts, torch.int32), _t((0.5,), torch.float64))

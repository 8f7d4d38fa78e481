"""CPU: the proposal fixtures written by the reference's tools (tests/golden/proposal_*.npz) against the float64 NumPy restatement
(proposal_fixture.restated) and against the host side of sos_wsod_amd.proposal_recall: the readers, the converters, what is refused."""
import pickle
import re

import numpy as np
import pytest

import proposal_fixture as F


def _lists(z, tmp_path):
    """the per-image box lists each budget reads, through the module's own readers"""
    from sos_wsod_amd import proposal_recall as PR
    path = F.write_mats(z, str(tmp_path / "mat"))
    mode = str(z["mode"])
    if mode == "mcg":
        p = PR.read_mcg_dir(F.records(z), path, F.name_of(z))
    else:
        p = PR.read_eb_mat(path) if mode == "eb" else PR.read_ss_mat(path)
    return p, path


@pytest.mark.parametrize("case", [c for c in F.CASES if c != "ss"])
def test_restatement_equals_reference(golden_dir, tmp_path, case):
    z = F.load(golden_dir, case)
    p, _ = _lists(z, tmp_path)
    assert p["boxes"][0].dtype == z["prop_box"].dtype                      # the readers keep the file's dtype
    ov, jm, cnt, recall = F.restated(F.records(z), F.ranked(p["boxes"], p["scores"]), F.name_of(z))
    assert F.same(ov.T, z["ovmax"]) and np.array_equal(jm.T, z["jmax"])
    assert F.same(recall, z["recall"])
    assert np.array_equal(cnt, np.rint(z["recall"] * len(ov)).astype(np.int64))
    if case == "handcoco":
        assert np.isnan(z["ovmax"][1:, 0]).all() and not np.isnan(z["ovmax"][0]).any() and (z["jmax"][1:, 0] == 5).all()
    if case == "hand":
        assert (z["ovmax"] == 1.0).any() and z["recall"][-1, -1] > 0      # IoU exactly 1.0 counts at threshold 1.0
        assert (z["prop_box"] == 0).sum() == 3                             # the coordinates that wrap


def test_restatement_equals_reference_random_draws(golden_dir, tmp_path):
    z = F.load(golden_dir, "ss")
    p, _ = _lists(z, tmp_path)
    rng = np.random.RandomState(int(z["seed"]))
    for k, m in enumerate(F.BUDGETS):
        drawn = [b[rng.choice(b.shape[0], size=min(b.shape[0], m), replace=False), ...] for b in p["boxes"]]
        ov, jm, _, recall = F.restated(F.records(z), drawn, F.name_of(z), budgets=(m,))
        assert F.same(ov[:, 0], z["ovmax"][k]) and np.array_equal(jm[:, 0], z["jmax"][k]) and F.same(recall[0], z["recall"][k]), m


def test_constants_are_the_reference_s_and_the_header_s():
    import os
    from sos_wsod_amd import ops
    from sos_wsod_amd import proposal_recall as PR
    assert PR.IOU_THRESHOLDS == F.THRESHOLDS and PR.BUDGETS == F.BUDGETS and len(PR.IOU_THRESHOLDS) == 11
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "soswsod_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+SW_PROPOSAL_RECALL_(\w+)\s+(\d+)", src, flags=re.M)}
    assert (PR.MAX_CUTS, PR.MAX_THRESHOLDS) == (d["MAX_CUTS"], d["MAX_THRESHOLDS"])
    assert (ops.PROPOSAL_RECALL_MAX_CUTS, ops.PROPOSAL_RECALL_MAX_THRESHOLDS, ops.PROPOSAL_RECALL_LDS_BOXES) == \
        (d["MAX_CUTS"], d["MAX_THRESHOLDS"], d["LDS_BOXES"])
    assert len(PR.BUDGETS) <= PR.MAX_CUTS and PR.BUDGETS[-1] > d["LDS_BOXES"]          # the default run takes more than one pass


@pytest.mark.parametrize("case", ["hand", "handcoco", "random", "ss"])
def test_converters_write_the_reference_s_pickle(golden_dir, tmp_path, case):
    from sos_wsod_amd import proposal_recall as PR
    from sos_wsod_amd.proposals import load_proposals_into_dataset
    z = F.load(golden_dir, case)
    recs = F.records(z)
    path = F.write_mats(z, str(tmp_path / "mat"))
    out = str(tmp_path / "out.pkl")
    (PR.convert_ss_box if case == "ss" else PR.convert_mcg_box)(recs, path, out, F.name_of(z))
    with open(out, "rb") as f:
        p = pickle.load(f)
    assert sorted(p) == ["boxes", "indexes", "scores"]
    assert all(b.dtype == np.int16 and b.ndim == 2 for b in p["boxes"]) and all(s.dtype == np.float32 for s in p["scores"])
    assert np.concatenate(p["boxes"]).tobytes() == z["conv_box"].tobytes()
    assert np.concatenate([s.reshape(-1) for s in p["scores"]]).tobytes() == z["conv_score"].tobytes()
    assert [len(b) for b in p["boxes"]] == np.diff(z["prop_off"]).tolist()
    assert p["indexes"] == z["conv_id"].tolist() == [d["image_id"] for d in recs]
    if case == "hand":
        assert (z["conv_box"] == -1).sum() == 3                            # uint16 65535 -> int16 -1, as the reference writes it

    # the pickle loads through the Stage-1 loader: every record gets its boxes by descending score
    # (np.squeeze leaves the score of an image with one proposal 0-d, there as here; the loader cannot index it)
    loaded = load_proposals_into_dataset([dict(d) for d, s in zip(recs, p["scores"]) if s.ndim == 1], out)
    assert len(loaded) >= len(recs) - 1
    at = {str(i): k for k, i in enumerate(p["indexes"])}
    for d in loaded:
        k = at[str(d["image_id"])]
        assert d["proposal_boxes"].shape == p["boxes"][k].shape and d["proposal_bbox_mode"] == 0
        assert np.array_equal(np.sort(d["proposal_objectness_logits"])[::-1], d["proposal_objectness_logits"])
        assert sorted(map(tuple, d["proposal_boxes"].tolist())) == sorted(map(tuple, p["boxes"][k].tolist()))
    rd = PR.read_proposal_pkl(out)
    assert rd["ids"] == p["indexes"] and rd["boxes"][0].dtype == np.int16 and len(rd["scores"]) == len(recs)


def _tiny(dtype, n=3):
    recs = [{"file_name": "a.jpg", "image_id": "000001", "annotations": [{"bbox": [1.0, 2.0, 30.0, 40.0]}]}]
    return recs, {"boxes": [np.array([[1, 2, 30, 40], [5, 5, 20, 20], [0, 0, 9, 9]], dtype=dtype)[:n]],
                  "scores": [np.array([0.3, 0.2, 0.1])[:n]]}


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_narrow_float_boxes_are_refused(dtype):
    from sos_wsod_amd import proposal_recall as PR
    recs, p = _tiny(dtype)
    with pytest.raises(ValueError, match=np.dtype(dtype).name):
        PR.proposal_recall(recs, p, "voc_2007_test")
    with pytest.raises(ValueError, match=np.dtype(dtype).name):
        PR.proposal_recall(recs, {"boxes": p["boxes"]}, "voc_2007_test", mode="ss", rng=np.random.RandomState(0))


def test_ground_truth_without_proposals_is_refused():
    from sos_wsod_amd import proposal_recall as PR
    recs, p = _tiny(np.float64, n=0)
    with pytest.raises(ValueError, match="no proposals"):
        PR.proposal_recall(recs, p, "voc_2007_test")


def test_other_refusals():
    from sos_wsod_amd import proposal_recall as PR
    recs, p = _tiny(np.float64)
    with pytest.raises(ValueError, match="ascending"):
        PR.proposal_recall(recs, p, "voc_2007_test", budgets=(8, 4))
    with pytest.raises(ValueError, match="rng"):
        PR.proposal_recall(recs, p, "voc_2007_test", mode="ss")
    with pytest.raises(ValueError, match="carry none"):
        PR.proposal_recall(recs, {"boxes": p["boxes"]}, "voc_2007_test", mode="eb")
    with pytest.raises(ValueError, match="no ground-truth"):
        PR.proposal_recall([dict(recs[0], annotations=[])], p, "voc_2007_test")
    with pytest.raises(ValueError, match="1 proposal entries for 2 images"):
        PR.proposal_recall(recs + recs, p, "voc_2007_test")
    with pytest.raises(ValueError, match="overflows int16"):
        PR.proposal_recall(recs, {"boxes": [np.array([[-20000, 0, 20000, 5]], dtype=np.int16)], "scores": [np.ones(1)]}, "voc_2007_test")


def test_integer_extent_that_wraps_is_moved_out_of_the_image_with_its_wrapped_size():
    from sos_wsod_amd import proposal_recall as PR
    b = np.array([[65535, 3, 50, 40], [7, 65535, 60, 9], [4, 5, 65535, 50]], dtype=np.uint16)
    f = PR._boxes_f64(b)
    ref_w = (b[:, 2] - b[:, 0] + 1.0).tolist()
    ref_h = (b[:, 3] - b[:, 1] + 1.0).tolist()
    assert (f[:, 2] - f[:, 0] + 1.0).tolist() == ref_w == [52.0, 54.0, 65532.0]
    assert (f[:, 3] - f[:, 1] + 1.0).tolist() == ref_h == [38.0, 11.0, 46.0]
    assert f[2].tolist() == [4.0, 5.0, 65535.0, 50.0] and f[0, 0] > 1e9 and f[1, 1] > 1e9          # only a wrapped extent moves


def test_voc_records_follow_the_reference_loader(golden_dir, tmp_path):
    import voc_eval_fixture as V
    from sos_wsod_amd import proposal_recall as PR
    z = V.load(golden_dir, "hand")
    root = V.write_devkit(z, tmp_path / "VOC2007")
    recs = PR.voc_records(root, V.SPLIT)
    kept = PR.voc_records(root, V.SPLIT, keep_difficult=True)
    objs = V.recs(z)
    assert [d["image_id"] for d in recs] == V.names(z)
    for d, k in zip(recs, kept):
        o = objs[d["image_id"]]
        assert [a["bbox"] for a in k["annotations"]] == [[b[0] - 1.0, b[1] - 1.0, float(b[2]), float(b[3])] for b in (x["bbox"] for x in o)]
        assert [a["bbox"] for a in d["annotations"]] == [a["bbox"] for a, x in zip(k["annotations"], o) if x["difficult"] != 1]
    assert sum(len(d["annotations"]) for d in recs) < sum(len(d["annotations"]) for d in kept)


def test_ground_truth_that_could_reach_a_relocated_wrapped_box_is_refused():
    from sos_wsod_amd import proposal_recall as PR
    recs, p = _tiny(np.float64)
    recs[0]["annotations"].append({"bbox": [0.0, 0.0, 2.0 ** 39, 5.0]})
    with pytest.raises(ValueError, match="magnitude"):
        PR.proposal_recall(recs, p, "voc_2007_test")
    assert PR._FAR / 2 == 2.0 ** 39


def test_coco_records_are_sorted_by_image_id_as_load_coco_json_returns_them(tmp_path):
    import json
    from sos_wsod_amd import proposal_recall as PR
    ann = lambda i, img, box: {"id": i, "image_id": img, "category_id": 7, "bbox": box, "area": box[2] * box[3], "iscrowd": 0}  # noqa: E731
    data = {"images": [{"id": 30, "file_name": "c.jpg"}, {"id": 4, "file_name": "a.jpg"}, {"id": 11}],
            "categories": [{"id": 7, "name": "thing"}],
            "annotations": [ann(1, 30, [1, 2, 3, 4]), ann(2, 4, [5.5, 6, 7, 8]), ann(3, 30, [9, 10, 11, 12])]}
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(data))
    recs = PR.coco_records(str(path))
    assert [d["image_id"] for d in recs] == [4, 11, 30] and [d["file_name"] for d in recs] == ["a.jpg", "11.jpg", "c.jpg"]
    assert [[a["bbox"] for a in d["annotations"]] for d in recs] == [[[5.5, 6.0, 7.0, 8.0]], [], [[1.0, 2.0, 3.0, 4.0], [9.0, 10.0, 11.0, 12.0]]]
    del data["annotations"]
    path.write_text(json.dumps(data))
    with pytest.raises(ValueError, match="no annotations"):
        PR.coco_records(str(path))

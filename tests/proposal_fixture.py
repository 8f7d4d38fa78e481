"""The proposal fixtures tests/golden/proposal_*.npz (written by tests/golden/make_proposal_golden.py, which runs the reference's
proposal_recall.py and proposal_convert.py): the arrays they hold, the records and `.mat` files those arrays stand for, and a
float64 NumPy restatement of the recall computation for fuzzing.

A fixture holds, per case: `dataset_name`, `mode` (mcg / eb / ss), `seed` (ss), `image_id` (str or int) and `file_name` per image,
the ground truth (`gt_off` [n_img + 1], `gt_box` [G, 4] f64 as the annotations spell it: XYXY, or XYWH for a coco name), the
proposals as the `.mat` files hold them (`prop_off` [n_img + 1], `prop_box` [P, 4] in the file's dtype, 1-based (y1, x1, y2, x2);
`prop_score` [P] f64, absent for ss), and what the reference returned: `recall` [10, 11] (one row per budget), `ovmax` [10, G] f64
and `jmax` [10, G] i64 parsed from its printed `ovmax jmax` lines, and the pickle its converter wrote from the same files
(`conv_box` [P, 4] i16, `conv_score` [P] f32, `conv_id` per image; absent for eb, which the reference does not convert)."""
import os

import numpy as np

CASES = ("hand", "handcoco", "random", "eb", "ss")
BUDGETS = (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)
THRESHOLDS = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95, 1.0)


def load(golden_dir, case):
    with np.load(os.path.join(golden_dir, f"proposal_{case}.npz")) as z:
        return dict(z)


def name_of(z):
    return str(z["dataset_name"])


def records(z):
    """the dataset records the reference's DatasetCatalog returned"""
    ids = z["image_id"].tolist()
    off = z["gt_off"].tolist()
    return [{"file_name": str(f), "image_id": i,
             "annotations": [{"bbox": [float(v) for v in z["gt_box"][g]]} for g in range(off[k], off[k + 1])]}
            for k, (i, f) in enumerate(zip(ids, z["file_name"].tolist()))]


def per_image(z, key):
    off = z["prop_off"].tolist()
    return [z[key][off[k]:off[k + 1]] for k in range(len(off) - 1)]


def cells(arrays):
    c = np.empty((1, len(arrays)), dtype=object)
    for k, a in enumerate(arrays):
        c[0, k] = a
    return c


def write_mats(z, root):
    """the proposal files of the case under root -> the path the tools take (a directory for mcg, a file for eb / ss)"""
    import scipy.io as sio
    os.makedirs(root, exist_ok=True)
    mode, name = str(z["mode"]), name_of(z)
    boxes = per_image(z, "prop_box")
    if mode == "ss":
        path = os.path.join(root, "ss.mat")
        sio.savemat(path, {"boxes": cells(boxes)})
        return path
    scores = [s.reshape(-1, 1) for s in per_image(z, "prop_score")]
    if mode == "eb":
        path = os.path.join(root, "eb.mat")
        sio.savemat(path, {"boxes": cells(boxes), "boxScores": cells(scores)})
        return path
    for d, b, s in zip(records(z), boxes, scores):
        stem = os.path.basename(d["file_name"])[:-4] if ("coco" in name or "flickr" in name) else d["image_id"]
        keys = ("bboxes", "bboxes_scores") if "flickr" in name else ("boxes", "scores")
        sio.savemat(os.path.join(root, f"{stem}.mat"), {keys[0]: b, keys[1]: s})
    return str(root)


# ---- the restatement: what recall means, written against the arrays as NumPy holds them ------------------------------------------
def overlaps(boxes, gt):
    """IoU of one ground-truth box (xyxy floats) with each row of `boxes` (any dtype), pixel-inclusive extents"""
    left, top = np.maximum(boxes[:, 0], gt[0]), np.maximum(boxes[:, 1], gt[1])
    right, bottom = np.minimum(boxes[:, 2], gt[2]), np.minimum(boxes[:, 3], gt[3])
    w = np.maximum(right - left + 1.0, 0.0)
    h = np.maximum(bottom - top + 1.0, 0.0)
    shared = w * h
    total = (gt[2] - gt[0] + 1.0) * (gt[3] - gt[1] + 1.0) + (boxes[:, 2] - boxes[:, 0] + 1.0) * (boxes[:, 3] - boxes[:, 1] + 1.0) - shared
    return shared / total


def gt_xyxy(recs, dataset_name):
    out = []
    for d in recs:
        rows = []
        for a in d["annotations"]:
            b = a["bbox"]
            rows.append([b[0], b[1], b[0] + b[2], b[1] + b[3]] if "coco" in dataset_name else list(b))
        out.append(rows)
    return out


def restated(recs, lists, dataset_name, budgets=BUDGETS, thresholds=THRESHOLDS):
    """lists: per image the boxes in the order they count (ranked, or drawn), in their own dtype; every budget reads a prefix.
    -> ovmax [G, n_budget] f64, jmax [G, n_budget] i64, cnt_yes [n_budget, n_thr] i64, recall [n_budget, n_thr] f64

    ovmax is the overlap at jmax, not `np.max`: the two are the same number, but where a prefix holds both +0.0 and -0.0 (a box with
    xmax < xmin has a negative area, and 0 / negative is -0.0) the sign `np.max` returns depends on the order in which the host's
    vector unit folds the array, while `np.argmax` is documented to give the first of equal values."""
    ov, jm = [], []
    with np.errstate(all="ignore"):
        for boxes, gts in zip(lists, gt_xyxy(recs, dataset_name)):
            for gt in gts:
                o = overlaps(boxes[:budgets[-1]], gt)
                at = [int(np.argmax(o[:m])) for m in budgets]
                assert all(o[j] == np.max(o[:m]) or np.isnan(o[j]) and np.isnan(np.max(o[:m])) for j, m in zip(at, budgets))
                ov.append([o[j] for j in at])
                jm.append(at)
    ov = np.asarray(ov, dtype=np.float64).reshape(-1, len(budgets))
    jm = np.asarray(jm, dtype=np.int64).reshape(-1, len(budgets))
    cnt = np.array([[int(np.sum(ov[:, b] >= t)) for t in thresholds] for b in range(len(budgets))], dtype=np.int64)
    recall = np.array([[1.0 * int(c) / len(ov) for c in row] for row in cnt], dtype=np.float64)
    return ov, jm, cnt, recall


def ranked(boxes, scores, budget=BUDGETS[-1]):
    """each image's boxes by descending score (the reference's own call), cut to the largest budget"""
    return [b[np.argsort(-(np.asarray(s).flatten())), :][:budget] for b, s in zip(boxes, scores)]


def same(a, b):
    """equal bits; a NaN matches a NaN (x86 numpy makes 0 / 0 a NaN with the sign bit set, the GPU one without)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.where(np.isnan(a), 0.0, a).tobytes() == np.where(np.isnan(b), 0.0, b).tobytes()

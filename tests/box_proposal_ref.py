"""A NumPy restatement of the reference's `_evaluate_box_proposals` (detectron2/detectron2/evaluation/coco_evaluation.py:427-535,
with BoxMode.convert and pairwise_iou of structures/boxes.py) over the inputs of tests/box_proposal_fixture.py.  Besides the
reference's values it returns, per evaluated image, what every round took: the box's index among the valid boxes and the
proposal's rank — which the GPU tests compare element for element.

The rules, for one `area` and one `limit`, walking the predictions in list order:
  * ranking: `torch.sort(descending=True)` of the logits (torch's own call: its order among equal logits);
  * ground truth: the image's annotations with iscrowd == 0 in file order; BoxMode.convert makes a float32 tensor of a float
    list, so x2 = f32(f32(x) + f32(w)) (an all-integer list is added exactly and rounded once, the same value below 2^24);
    the annotation's area is compared in float32 with both bounds closed;
  * an image without non-crowd ground truth, without proposals, or unknown to the annotations is skipped before num_pos is
    counted; otherwise num_pos += G' and the ranked proposals are cut to `limit`;
  * IoU in float32: a = (x2 - x1) * (y2 - y1); w = max(min(x2) - max(x1), 0); inter = w * h; inter > 0 ? inter / (a1 + a2 -
    inter) : 0;
  * min(P', G') rounds, each taking the best unused pair under (largest IoU, smallest box index, smallest proposal index);
  * gt_overlaps: the sorted concatenation; recalls[t] = f32(count(gt_overlaps >= thr[t])) / num_pos; ar = recalls.mean().

`variant` makes the restatement wrong in one rule (VARIANTS), for the sensitivity tests."""
import warnings

import numpy as np
import torch

AREAS = {"all": 0, "small": 1, "medium": 2, "large": 3, "96-128": 4, "128-256": 5, "256-512": 6, "512-inf": 7}
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2], [96 ** 2, 128 ** 2],
               [128 ** 2, 256 ** 2], [256 ** 2, 512 ** 2], [512 ** 2, 1e5 ** 2]]
VARIANTS = ("last_box", "last_prop", "strict_threshold", "count_no_proposals", "area_f64", "cut_before_rank")
f32 = np.float32


def default_thresholds():
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32).numpy()


def ground_truth(ds):
    """{image id: (boxes f32 [G, 4] xyxy, areas f64 [G])} of the non-crowd annotations, in file order"""
    out = {}
    for a in ds["annotations"]:
        if a["iscrowd"] == 0:
            out.setdefault(a["image_id"], []).append(a)
    gt = {}
    for i, anns in out.items():
        b = np.asarray([[f32(v) for v in a["bbox"]] for a in anns], dtype=f32).reshape(-1, 4)
        box = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(f32)
        gt[i] = (box, np.asarray([float(a["area"]) for a in anns], dtype=np.float64))
    return gt


def iou_matrix(gt, prop):
    """[G, P] float32, pairwise_iou(prop, gt) transposed"""
    ga = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    pa = (prop[:, 2] - prop[:, 0]) * (prop[:, 3] - prop[:, 1])
    w = np.minimum(prop[None, :, 2], gt[:, None, 2]) - np.maximum(prop[None, :, 0], gt[:, None, 0])
    h = np.minimum(prop[None, :, 3], gt[:, None, 3]) - np.maximum(prop[None, :, 1], gt[:, None, 1])
    inter = np.maximum(w, f32(0)) * np.maximum(h, f32(0))
    assert inter.dtype == f32
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (pa[None, :] + ga[:, None] - inter)
    return np.where(inter > 0, iou, f32(0)).astype(f32)


def greedy(m, variant=None):
    """m [G, P] -> (overlaps f32 [G], box index i32 [G], proposal index i32 [G]); -1 where no round ran"""
    m = m.copy()
    G, P = m.shape
    ov, gi, pi = np.zeros(G, dtype=f32), np.full(G, -1, dtype=np.int32), np.full(G, -1, dtype=np.int32)
    for r in range(min(P, G)):
        if variant == "last_box":                                  # per box the first proposal, then the last box of equals
            v = m.max()
            g = int(np.nonzero((m == v).any(axis=1))[0][-1])
            p = int(np.argmax(m[g]))
        elif variant == "last_prop":
            g, p = divmod(int(np.argmax(m)), P)
            p = int(np.nonzero(m[g] == m[g, p])[0][-1])
        else:
            g, p = divmod(int(np.argmax(m)), P)                    # row-major: the first box, then the first proposal, of equals
        ov[r], gi[r], pi[r] = m[g, p], g, p
        m[g, :] = -1
        m[:, p] = -1
    return ov, gi, pi


def evaluate(ds, preds, thresholds=None, area="all", limit=None, variant=None, gt=None):
    """-> {"ar", "recalls", "thresholds", "gt_overlaps" (sorted), "num_pos", "counts" i64 [T], "images": [(position in preds,
    overlaps, match_gt, match_box) of every image that reached the matching, before sorting]}"""
    assert variant is None or variant in VARIANTS, variant
    lo, hi = AREA_RANGES[AREAS[area]]
    gt = ground_truth(ds) if gt is None else gt
    images, num_pos = [], 0
    for n, p in enumerate(preds):
        boxes, logits = p["boxes"], p["logits"]
        if variant == "cut_before_rank" and limit is not None:
            boxes, logits = boxes[:limit], logits[:limit]
        inds = torch.from_numpy(logits.copy()).sort(descending=True)[1].numpy()
        boxes = boxes[inds]
        g = gt.get(p["image_id"])
        if g is None or (len(boxes) == 0 and variant != "count_no_proposals"):
            continue
        if variant == "area_f64":
            valid = (g[1] >= lo) & (g[1] <= hi)
        else:
            valid = (g[1].astype(f32) >= f32(lo)) & (g[1].astype(f32) <= f32(hi))
        gb = g[0][valid]
        num_pos += len(gb)
        if len(gb) == 0 or len(boxes) == 0:
            continue
        if limit is not None and len(boxes) > limit:
            boxes = boxes[:limit]
        images.append((n,) + greedy(iou_matrix(gb, boxes), variant))
    gt_overlaps = np.sort(np.concatenate([im[1] for im in images])) if images else np.zeros(0, dtype=f32)
    thr = default_thresholds() if thresholds is None else np.asarray(thresholds, dtype=f32)
    if variant == "strict_threshold":
        counts = np.asarray([(gt_overlaps > t).sum() for t in thr], dtype=np.int64)
    else:
        counts = np.asarray([(gt_overlaps >= t).sum() for t in thr], dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        recalls = (torch.from_numpy(counts).float() / np.float64(num_pos)).numpy()          # num_pos 0: NaN, as the reference's
    ar = torch.from_numpy(recalls).mean().numpy()
    return {"ar": ar, "recalls": recalls, "thresholds": thr, "gt_overlaps": gt_overlaps, "num_pos": num_pos, "counts": counts,
            "images": images}


_shared = {}


def evaluate_case(name, area, limit):
    """the restatement of a fixture case, computed once per process and shared by the tests (read-only)"""
    import box_proposal_fixture as F
    k = (name, area, limit)
    if k not in _shared:
        ds, preds, _ = F.case(name)
        if ("gt", name) not in _shared:
            _shared["gt", name] = ground_truth(ds)
        _shared[k] = evaluate(ds, preds, area=area, limit=limit, gt=_shared["gt", name])
    return _shared[k]


def postprocess_proposals(boxes, logits, image_size, output_height, output_width):
    """modeling/postprocessing.py:9-44 for `proposal_boxes` in float32: scale, clip, drop empty -> (boxes, logits)"""
    sx, sy = f32(output_width / image_size[1]), f32(output_height / image_size[0])
    b = np.asarray(boxes, dtype=f32).copy()
    b[:, 0::2] *= sx
    b[:, 1::2] *= sy
    b[:, 0::2] = np.clip(b[:, 0::2], f32(0), f32(output_width))
    b[:, 1::2] = np.clip(b[:, 1::2], f32(0), f32(output_height))
    keep = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
    return b[keep], np.asarray(logits)[keep]

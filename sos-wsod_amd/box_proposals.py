"""Box-proposal AR: how good a proposal set is, measured the detectron2 way, and the file that carries it back to Stage 1.

Port of the reference's `COCOEvaluator._eval_box_proposals` and `_evaluate_box_proposals`
(detectron2/detectron2/evaluation/coco_evaluation.py:255-292, 427-535; the copy under uwsod/ is identical): per image the
proposals are ranked by objectness, cut to `limit`, and matched one to one with the non-crowd ground-truth boxes of an area range
by greedy coverage — min(P', G') rounds, each taking the best remaining (proposal, box) pair; AR is the mean over the IoU
thresholds 0.50:0.05:0.95 of the share of boxes covered.  `proposal_recall` measures the WSL way (best overlap per box, one
proposal may serve many boxes); this is the one-to-one measure behind AR@100 / AR@1000 and ARs / ARm / ARl.

The reference walks the split once per (area, limit) with `torch.max` over each image's whole IoU matrix per round.  Here the
host ranks (the reference's own `objectness_logits.sort(descending=True)` on CPU tensors, so the order among equal logits is
torch's), builds the CSR arrays with vectorised NumPy and makes ONE launch (`ops.box_proposal_ar`) for all areas and limits; the
IoUs, the rounds and the counts run on the GPU in the reference's float32 operations, so `gt_overlaps`, `recalls`, `ar` and
`num_pos` are bit-identical to the reference's.  Recalls and their mean are formed on the host with the torch expressions of
:523-528 from the integer counts.

Kept from the reference: an image without non-crowd ground truth, WITHOUT PROPOSALS, or unknown to the annotation file is skipped
before num_pos is counted (its boxes do not count as missed); a prediction listed twice is evaluated twice; an annotation's own
"area" decides its range, compared in float32 with both bounds closed (1024 is small and medium, and so is 1024.00001);
ground-truth corners are x + w in float32 (BoxMode.convert makes a float32 tensor of the list); num_pos == 0 gives NaN.
What differs: non-finite logits or boxes, and a limit below 1, are a ValueError; annotations of a category the file does not
declare are not read (`COCOGroundTruth` drops them, pycocotools keeps them).

    python -m sos_wsod_amd.evaluation --proposals FILE.pkl (--coco-json FILE | --voc-root DIR [--split S] [--year Y])
"""
import pickle
from collections import OrderedDict

import numpy as np
import torch

from .proposals import XYWH_ABS, XYXY_ABS, read_proposal_file

AREAS = {"all": 0, "small": 1, "medium": 2, "large": 3, "96-128": 4, "128-256": 5, "256-512": 6, "512-inf": 7}      # :435-444
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2], [96 ** 2, 128 ** 2],
               [128 ** 2, 256 ** 2], [256 ** 2, 512 ** 2], [512 ** 2, 1e5 ** 2]]                                      # :445-454
AREA_SUFFIX = OrderedDict([("all", ""), ("small", "s"), ("medium", "m"), ("large", "l")])                              # :285
MAX_AREAS, MAX_LIMITS, MAX_THRESHOLDS = 8, 8, 16          # SW_BOXAR_MAX_AREAS / _MAX_LIMITS / _MAX_THRESHOLDS


def default_thresholds():
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)                                                   # :520-522


# ---------------------------------------------------------------------------------------------------------------------- records
def _arrays(prediction):
    """one prediction -> (image id, boxes f32 [n, 4], logits f32 [n]), from an evaluator record ({"image_id", "proposals":
    Instances}) or from arrays ({"image_id", "boxes", "logits" | "objectness_logits"})"""
    if "proposals" in prediction:
        inst = prediction["proposals"]
        boxes = inst.proposal_boxes.tensor.detach().cpu().numpy()
        logits = inst.objectness_logits.detach().cpu().numpy()
    else:
        boxes = prediction["boxes"]
        logits = prediction["logits"] if "logits" in prediction else prediction["objectness_logits"]
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    logits = np.asarray(logits, dtype=np.float32).reshape(-1)
    if len(boxes) != len(logits):
        raise ValueError(f"image {prediction['image_id']!r}: {len(boxes)} boxes and {len(logits)} logits")
    return prediction["image_id"], boxes, logits


def predictions_from_file(path):
    """A proposal pickle (this module's box_proposals.pkl, or a converted MCG / Selective Search pickle), through
    `proposals.read_proposal_file` -> [{"image_id", "boxes" f32 xyxy, "logits"}] in the file's order"""
    p = read_proposal_file(path)
    mode = int(p["bbox_mode"]) if "bbox_mode" in p else XYXY_ABS
    if mode not in (XYXY_ABS, XYWH_ABS):
        raise ValueError(f"unsupported proposal bbox_mode {mode}")
    out = []
    for i, b, s in zip(p["ids"], p["boxes"], p["objectness_logits"]):
        b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
        if mode == XYWH_ABS:
            b = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1)
        out.append({"image_id": i, "boxes": b, "logits": np.asarray(s, dtype=np.float32).reshape(-1)})
    return out


def write_box_proposals(predictions, path):
    """The reference's box_proposals.pkl (:260-277): {"boxes", "objectness_logits", "ids", "bbox_mode": XYXY_ABS}, one entry per
    prediction in list order, as produced (not ranked).  `proposals.read_proposal_file` and the Stage-1 loader read it."""
    ids, boxes, logits = [], [], []
    for p in predictions:
        i, b, s = _arrays(p)
        ids.append(i)
        boxes.append(b)
        logits.append(s)
    with open(path, "wb") as f:
        pickle.dump({"boxes": boxes, "objectness_logits": logits, "ids": ids, "bbox_mode": XYXY_ABS}, f)


def _image_index(gt):
    """COCOGroundTruth.img_index, with ids that differ only in int / str spelling (a VOC split's) matched too"""
    index = dict(gt.img_index)
    for k, v in gt.img_index.items():
        index.setdefault(str(k), v)
    return index


# ---------------------------------------------------------------------------------------------------------------------- layout
def box_proposal_layout(predictions, gt, areas, limits):
    """The kernel's arrays (include/soswsod_hip.h, sw_box_proposal_ar) of one evaluation, on the host.  An "image" is an entry of
    `predictions`.  -> dict(prop_off, prop_box, gt_off, gt_box, gt_area, area_rng [A, 2] f32, limits [L] (0: none), item_off,
    num_pos [A] (the same for every limit), counts [A, n_img] valid boxes per item)"""
    for a in areas:
        if a not in AREAS:
            raise ValueError("Unknown area range: {}".format(a))
    for lim in limits:
        if lim is not None and int(lim) < 1:
            raise ValueError(f"limit {lim!r}: None or at least 1")
    if not 1 <= len(areas) <= MAX_AREAS or not 1 <= len(limits) <= MAX_LIMITS:
        raise ValueError(f"1..{MAX_AREAS} area ranges and 1..{MAX_LIMITS} limits per call")
    lims = np.asarray([0 if lim is None else int(lim) for lim in limits], dtype=np.int32)
    keep = None if (lims == 0).any() else int(lims.max())               # ranks beyond the largest limit are never read
    n_img = len(predictions)
    index = _image_index(gt)
    ranked, img = [], np.full(n_img, -1, dtype=np.int64)
    for n, p in enumerate(predictions):
        i, boxes, logits = _arrays(p)
        if not (np.isfinite(boxes).all() and np.isfinite(logits).all()):
            raise ValueError(f"image {i!r}: proposal boxes and objectness logits must be finite")
        inds = torch.from_numpy(logits).sort(descending=True)[1].numpy()                     # :465, torch's own order among equals
        ranked.append(boxes[inds[:keep]])
        k = index.get(i, index.get(str(i)))
        img[n] = -1 if k is None else k
    n_prop = np.asarray([len(b) for b in ranked], dtype=np.int64)
    prop_off = np.concatenate([[0], np.cumsum(n_prop)]).astype(np.int64)
    prop_box = np.concatenate(ranked).astype(np.float32) if ranked else np.zeros((0, 4), dtype=np.float32)
    # the non-crowd annotations of every image of the file, in file order, then gathered per prediction
    plain = np.nonzero(~gt.ann_crowd)[0]
    order = plain[np.argsort(gt.ann_img[plain], kind="stable")]
    per_img = np.bincount(gt.ann_img[plain], minlength=len(gt.img_ids)).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(per_img)])
    n_gt = np.where(img >= 0, per_img[np.maximum(img, 0)], 0) if n_img else np.zeros(0, dtype=np.int64)
    gt_off = np.concatenate([[0], np.cumsum(n_gt)]).astype(np.int64)
    rows = np.repeat(start[np.maximum(img, 0)] - gt_off[:-1], n_gt) + np.arange(gt_off[-1])
    rows = order[rows]
    b = gt.ann_box[rows].astype(np.float32)
    gt_box = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32) if len(b) else \
        np.zeros((0, 4), dtype=np.float32)
    gt_area = gt.ann_area[rows].astype(np.float32)
    area_rng = np.asarray([AREA_RANGES[AREAS[a]] for a in areas], dtype=np.float32)
    # valid boxes per (area, image); an image without proposals or ground truth has no items (:479)
    row_img = np.repeat(np.arange(n_img), n_gt)
    live = (n_prop > 0) & (n_gt > 0)
    counts = np.zeros((len(areas), n_img), dtype=np.int64)
    for a, (lo, hi) in enumerate(area_rng):
        valid = (gt_area >= lo) & (gt_area <= hi)                                             # :482, in float32
        counts[a] = np.bincount(row_img[valid], minlength=n_img) * live
    item_len = np.broadcast_to(counts[None], (len(lims),) + counts.shape).reshape(-1)
    item_off = np.concatenate([[0], np.cumsum(item_len)]).astype(np.int64)
    return dict(n_img=n_img, prop_off=prop_off, prop_box=prop_box, gt_off=gt_off, gt_box=gt_box, gt_area=gt_area,
                area_rng=area_rng, limits=lims, item_off=item_off, num_pos=counts.sum(1), counts=counts,
                max_boxes=int(n_gt.max()) if n_img else 0, max_props=int(n_prop.max()) if n_img else 0)


def _launch(L, thresholds, device, return_matches):
    from . import ops

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    n_out = int(L["item_off"][-1])                                 # known here: the wrapper need not read it back
    overlap, match_gt, match_box, cnt, status = ops.box_proposal_ar(
        dev(L["prop_off"]), dev(L["prop_box"]), dev(L["gt_off"]), dev(L["gt_box"]), dev(L["gt_area"]), L["area_rng"].tolist(),
        L["limits"].tolist(), thresholds.tolist(), dev(L["item_off"]), overlap=torch.empty(n_out, device=device, dtype=torch.float32),
        match_gt=torch.empty(n_out, device=device, dtype=torch.int32), match_box=torch.empty(n_out, device=device, dtype=torch.int32),
        max_boxes=L["max_boxes"], max_props=L["max_props"], check_offsets=False)
    code = int(status.item())
    if code:
        raise RuntimeError(f"sw_box_proposal_ar refused part of the split: {ops.BOXAR_STATUS.get(code, code)}")
    out = [overlap.cpu(), cnt.cpu()]
    if return_matches:
        out += [match_gt.cpu().numpy(), match_box.cpu().numpy()]
    return out


def _stats(L, la, n_areas, overlap, cnt, thresholds, matches):
    """the reference's result dict (:515-535) of one (limit, area) from its region of the launch's outputs"""
    l, a = la
    n_img = L["n_img"]
    base = (l * n_areas + a) * n_img
    lo, hi = int(L["item_off"][base]), int(L["item_off"][base + n_img])
    gt_overlaps, _ = torch.sort(overlap[lo:hi].clone())
    num_pos = int(L["num_pos"][a])
    recalls = torch.zeros_like(thresholds)
    for i in range(len(thresholds)):
        recalls[i] = torch.tensor(int(cnt[l, a, i])).float() / float(num_pos)                 # :526 from the integer count
    out = {"ar": recalls.mean(), "recalls": recalls, "thresholds": thresholds, "gt_overlaps": gt_overlaps, "num_pos": num_pos}
    if matches is not None:
        off = L["item_off"][base:base + n_img + 1]
        ov = overlap.numpy()
        out["images"] = [(n, ov[off[n]:off[n + 1]].copy(), matches[0][off[n]:off[n + 1]].copy(), matches[1][off[n]:off[n + 1]].copy())
                         for n in np.nonzero(np.diff(off))[0]]
    return out


def _thresholds(thresholds):
    thr = default_thresholds() if thresholds is None else torch.as_tensor(thresholds).detach().cpu()
    if thr.dim() != 1 or not 1 <= thr.numel() <= MAX_THRESHOLDS or not thr.is_floating_point():
        raise ValueError(f"thresholds: a 1-d float tensor of 1..{MAX_THRESHOLDS} values")
    if thr.dtype != torch.float32:
        raise ValueError("thresholds must be float32 (the reference compares float32 overlaps with them)")
    return thr


def evaluate_box_proposals(predictions, gt, thresholds=None, area="all", limit=None, return_matches=False, device="cuda"):
    """`_evaluate_box_proposals(dataset_predictions, coco_api, thresholds, area, limit)` (:427-535) with `gt` a
    `evaluation.COCOGroundTruth` -> the reference's dict: "ar" (0-d f32 tensor), "recalls" f32 [T], "thresholds", "gt_overlaps"
    f32 sorted, "num_pos" int; with return_matches also "images": [(position in predictions, overlaps f32 [G'], match_gt i32,
    match_box i32)] — per image that was matched, what each round took: the IoU, the box's index among the valid boxes and the
    proposal's rank (-1 where no round ran)."""
    thr = _thresholds(thresholds)
    L = box_proposal_layout(predictions, gt, [area], [limit])
    res = _launch(L, thr, device, return_matches)
    return _stats(L, (0, 0), 1, res[0], res[1], thr, res[2:] if return_matches else None)


def box_proposal_metrics(predictions, gt, areas=("all", "small", "medium", "large"), limits=(100, 1000), return_matches=False,
                         device="cuda"):
    """`COCOEvaluator._eval_box_proposals` (:284-292): every (limit, area) in one launch -> OrderedDict {"AR@100", "ARs@100",
    "ARm@100", "ARl@100", "AR@1000", ...: float(ar * 100)} in the reference's order and spelling (an area outside the four named
    ones is spelt "AR[name]@limit").  With return_matches -> (that dict, {(area, limit): evaluate_box_proposals' dict with
    "images"})."""
    thr = default_thresholds()
    areas, limits = list(areas), list(limits)
    L = box_proposal_layout(predictions, gt, areas, limits)
    res = _launch(L, thr, device, return_matches)
    out, stats = OrderedDict(), {}
    for l, limit in enumerate(limits):
        for a, area in enumerate(areas):
            s = _stats(L, (l, a), len(areas), res[0], res[1], thr, res[2:] if return_matches else None)
            suffix = AREA_SUFFIX.get(area, f"[{area}]")
            out["AR{}@{}".format(suffix, "all" if limit is None else "{:d}".format(limit))] = float(s["ar"].item() * 100)     # :289-290
            stats[area, limit] = s
    return (out, stats) if return_matches else out


# ---------------------------------------------------------------------------------------------------------------------- VOC
def voc_coco_dataset(dirname, split, class_names=None):
    """The COCO-format dict `convert_to_coco_json` (detectron2/detectron2/data/datasets/coco.py:476-528) makes of a VOC split
    loaded by `load_voc_instances` (data/datasets/pascal_voc.py:60-85), as far as this evaluation reads it: every object,
    difficult ones included; bbox XYWH of (xmin - 1, ymin - 1, xmax, ymax); area = that box's float32 area; iscrowd 0."""
    import os
    import xml.etree.ElementTree as ET
    from .evaluation import VOC_CLASS_NAMES
    names = list(VOC_CLASS_NAMES if class_names is None else class_names)
    with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
        fileids = [x.strip() for x in f if x.strip()]
    ds = {"images": [], "categories": [{"id": k, "name": n} for k, n in enumerate(names)], "annotations": []}
    for fileid in fileids:
        tree = ET.parse(os.path.join(dirname, "Annotations", fileid + ".xml"))
        size = tree.find("size")
        ds["images"].append({"id": fileid, "file_name": os.path.join(dirname, "JPEGImages", fileid + ".jpg"),
                             "height": int(size.find("height").text), "width": int(size.find("width").text)})
        for obj in tree.findall("object"):
            bb = obj.find("bndbox")
            x1, y1, x2, y2 = (np.float32(float(bb.find(k).text)) for k in ("xmin", "ymin", "xmax", "ymax"))
            x1, y1 = x1 - np.float32(1.0), y1 - np.float32(1.0)
            w, h = x2 - x1, y2 - y1                                                            # BoxMode.convert: a float32 tensor
            ds["annotations"].append({"id": len(ds["annotations"]) + 1, "image_id": fileid,
                                      "category_id": names.index(obj.find("name").text),
                                      "bbox": [round(float(v), 3) for v in (x1, y1, w, h)], "area": float(w * h), "iscrowd": 0})
    return ds


def voc_ground_truth(dirname, split, class_names=None):
    from .evaluation import COCOGroundTruth
    return COCOGroundTruth(voc_coco_dataset(dirname, split, class_names))

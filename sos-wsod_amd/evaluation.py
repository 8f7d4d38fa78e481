"""Detection evaluation: VOC mAP and CorLoc at the IoU thresholds 0.50:0.05:0.95 and COCO bbox AP, the numbers SoS-WSOD reports.

Port of the reference's `PascalVOCDetectionEvaluator` (`evaluation/pascal_voc_evaluation.py`, with `voc_eval`, `voc_ap`,
`voc_eval_corloc` and `parse_rec`) and of the core of its `inference_on_dataset` (`evaluation/evaluator.py:101`).  The matching,
the TP / FP decisions, the cumulative sums, precision / recall, both AP metrics and CorLoc of every class at every threshold run
on the GPU (`ops.voc_eval`: two launches and one device-to-host copy per evaluation).  The host parses the annotations and the
detection lines, orders each class's detections and builds the CSR arrays; the final means are numpy's, as in the reference.

Per class and threshold the results are bit-identical to the reference's functions run with a stable sort.  What differs:
  * Tie order.  The reference ranks a class's detections with `np.argsort(-confidence)`, which is not stable, so among equal
    scores (frequent: the lines carry three decimals) its order depends on numpy's sort and the host CPU.  Here the rank is
    descending score, ties in line order; after a multi-rank gather, line order is rank order.
  * A detection whose image is not in the split is a ValueError (the reference raised KeyError).
  * CorLoc of a class that has detections but no image with a non-difficult object is a ValueError (the reference divided by
    zero).  `voc_eval_arrays(..., corloc=False)` evaluates AP alone for such a class: its area AP is NaN, its 11-point AP 0.
  * The `comp4_*` result files the reference writes into the dataset tree are not written.
  * `voc_2012_test` has no public annotations and is refused.

COCO: port of the reference's `COCOEvaluator` with `use_fast_impl=True` for the "bbox" task (`evaluation/coco_evaluation.py`;
`COCOeval_opt` in `evaluation/fast_eval_api.py` over `layers/csrc/cocoeval/cocoeval.cpp`, with pycocotools' `_prepare`,
`computeIoU`, `loadRes` and `summarize`).  pycocotools is not used.  The IoU matrices, the greedy matching of every (image,
category, area range, threshold) and the accumulation of every precision / recall curve run on the GPU (`ops.coco_eval`: two
launches and one device-to-host copy); the host reads the JSON, does the two stable sorts, counts the non-ignored ground truth and
takes `summarize`'s means with numpy.  `precision`, `recall` and `scores` are bit-identical to `COCOeval_opt`'s.  What differs:
  * A detection of an image outside the annotation file is a ValueError (loadRes asserts); non-finite boxes or scores are a
    ValueError; an annotation file without "annotations" is refused (the reference returns no results).
  * Only "bbox": segm, keypoints and box-proposal AR are refused; LVIS evaluation is not provided.  `instances_predictions.pth`
    is not written.
  * Kept quirk: `cocoeval.cpp` calls a detection matched when the matched annotation's id is > 0, so an annotation with id 0 takes
    its detection (no other detection can have it) but never counts as a true positive.
"""
import argparse
import json
import os
import xml.etree.ElementTree as ET
from collections import OrderedDict

import numpy as np

from .inference import VOCDetectionWriter
from .ops import COCO_LDS_DOUBLES, COCO_MAX_CLASSES

VOC_CLASS_NAMES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
                   "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
IOU_THRESHOLDS = tuple(range(50, 100, 5))                 # percent, as the reference loops over them
RECALL_LEVELS = np.arange(0.0, 1.1, 0.1)                  # voc_ap's 11 points: 0.30000000000000004, not 0.3
MAX_CLASSES = 256                                         # SW_VOC_MAX_CLASSES


def parse_rec(filename):
    """The objects of one VOC annotation file, as the reference's parse_rec reads them (difficult objects included)."""
    tree = ET.parse(filename)
    objects = []
    for obj in tree.findall("object"):
        bbox = obj.find("bndbox")
        objects.append({
            "name": obj.find("name").text,
            "pose": obj.find("pose").text,
            "truncated": int(obj.find("truncated").text),
            "difficult": int(obj.find("difficult").text),
            "bbox": [int(bbox.find("xmin").text), int(bbox.find("ymin").text), int(bbox.find("xmax").text),
                     int(bbox.find("ymax").text)],
        })
    return objects


class GroundTruth:
    """The ground truth of one split in the kernel's layout.

    names: the image-set lines (stripped; a repeated line counts again in npos, as in the reference); images: the distinct names
    in first-appearance order; gt_off [n_img * K + 1]: objects of (image i, class c) are rows [gt_off[i * K + c], ...) of
    gt_box [G, 4] f64 and gt_diff [G] u8, in annotation order; npos / npos_im [K]: non-difficult objects / images with one."""

    def __init__(self, names, recs, class_names):
        self.names = list(names)
        self.class_names = tuple(class_names)
        self.images = list(dict.fromkeys(self.names))
        self.index = {n: i for i, n in enumerate(self.images)}
        K, n_img = len(self.class_names), len(self.images)
        cls_of = {c: k for k, c in enumerate(self.class_names)}
        obj_img, obj_cls, box, diff = [], [], [], []
        for i, name in enumerate(self.images):
            for o in recs[name]:
                k = cls_of.get(o["name"])
                if k is not None:                              # objects of other classes are never read
                    obj_img.append(i)
                    obj_cls.append(k)
                    box.append(o["bbox"])
                    diff.append(o["difficult"])
        key = np.asarray(obj_img, dtype=np.int64) * K + np.asarray(obj_cls, dtype=np.int64)
        order = np.argsort(key, kind="stable")
        self.gt_box = np.asarray(box, dtype=np.float64).reshape(-1, 4)[order]
        self.gt_diff = np.asarray(diff, dtype=bool)[order].astype(np.uint8)
        self.gt_off = np.zeros(n_img * K + 1, dtype=np.int64)
        np.cumsum(np.bincount(key, minlength=n_img * K), out=self.gt_off[1:])
        plain = np.zeros((n_img, K), dtype=np.int64)
        np.add.at(plain, (np.asarray(obj_img, dtype=np.int64), np.asarray(obj_cls, dtype=np.int64)),
                  1 - np.asarray(diff, dtype=bool).astype(np.int64))
        per_line = plain[[self.index[n] for n in self.names]] if self.names else np.zeros((0, K), np.int64)
        self.npos = per_line.sum(0).astype(np.int64)
        self.npos_im = (per_line > 0).sum(0).astype(np.int64)
        self._int_index = None

    @classmethod
    def load(cls, dirname, split, class_names=VOC_CLASS_NAMES):
        """ImageSets/Main/{split}.txt and Annotations/{id}.xml under the dataset directory (e.g. datasets/VOC2007)"""
        with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
            names = [x.strip() for x in f.readlines()]
        recs = {n: parse_rec(os.path.join(dirname, "Annotations", n + ".xml")) for n in dict.fromkeys(names)}
        return cls(names, recs, class_names)

    def image_of_record_id(self, image_id):
        """the image index of a JSON record's integer image_id (int() of the file id, as VOCDetectionWriter.records writes it)"""
        if self._int_index is None:
            self._int_index = {}
            for i, n in enumerate(self.images):
                try:
                    k = int(n)
                except ValueError:
                    continue
                if k in self._int_index:
                    raise ValueError(f"image ids {self.images[self._int_index[k]]!r} and {n!r} are the same integer")
                self._int_index[k] = i
        try:
            return self._int_index[int(image_id)]
        except KeyError:
            raise ValueError(f"detection for image {image_id!r}, which is not in the split") from None


class Detections:
    """The detections of each class in line order: image index [n] i64, score [n] f64, box [n, 4] f64 (xmin + 1, ymin + 1,
    xmax, ymax, as the lines carry them)."""

    def __init__(self, per_class):
        self.per_class = [(np.asarray(i, dtype=np.int64), np.asarray(s, dtype=np.float64),
                           np.asarray(b, dtype=np.float64).reshape(-1, 4)) for i, s, b in per_class]

    @classmethod
    def from_lines(cls, lines, gt):
        """{class index: ["image_id score xmin ymin xmax ymax", ...]} (the evaluator's lines) -> Detections"""
        per_class = []
        for k in range(len(gt.class_names)):
            ls = [x for x in lines.get(k, []) if x.strip()]
            toks = " ".join(x.strip() for x in ls).split(" ") if ls else []
            if len(toks) != 6 * len(ls):
                raise ValueError(f"class {gt.class_names[k]}: a detection line does not have 6 fields")
            try:
                img = [gt.index[t] for t in toks[0::6]]
            except KeyError as e:
                raise ValueError(f"detection for image {e.args[0]!r}, which is not in the split") from None
            score = np.fromiter(map(float, toks[1::6]), dtype=np.float64, count=len(ls))
            box = np.stack([np.fromiter(map(float, toks[2 + q::6]), dtype=np.float64, count=len(ls)) for q in range(4)], 1)
            per_class.append((img, score, box))
        return cls(per_class)

    @classmethod
    def from_records(cls, records, gt):
        """VOCDetectionWriter.records() / the JSON of its dump (1-based category_id) -> Detections, in record order per class"""
        K = len(gt.class_names)
        img, score, box = ([[] for _ in range(K)] for _ in range(3))
        for r in records:
            k = int(r["category_id"]) - 1
            if not 0 <= k < K:
                raise ValueError(f"category_id {r['category_id']} is outside 1..{K}")
            img[k].append(gt.image_of_record_id(r["image_id"]))
            score[k].append(float(r["score"]))
            box[k].append([float(v) for v in r["bbox"]])
        return cls(zip(img, score, box))


def voc_eval_arrays(gt, dets, corloc=True, device="cuda"):
    """Every class at every IoU threshold on the GPU.  -> {"ap_area", "ap_07", "corloc"}: f64 [K, 10] in percent (value * 100, as
    the reference collects them), thresholds in IOU_THRESHOLDS order; "corloc" is None when corloc=False.
    Raises ValueError before any GPU work for a class with detections and no non-difficult object when corloc=True."""
    K = len(gt.class_names)
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"{K} classes: the evaluation kernel takes 1..{MAX_CLASSES}")
    if len(dets.per_class) != K:
        raise ValueError(f"detections for {len(dets.per_class)} classes, ground truth for {K}")
    nd = np.array([len(s) for _, s, _ in dets.per_class], dtype=np.int64)
    if corloc:
        bad = [gt.class_names[k] for k in range(K) if nd[k] > 0 and gt.npos_im[k] == 0]
        if bad:
            raise ValueError(f"CorLoc is undefined for {bad}: detections but no image with a non-difficult object of the class")
    # rank: descending score, ties in line order
    orders = [np.argsort(-s, kind="stable") for _, s, _ in dets.per_class]
    det_off = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(nd, out=det_off[1:])
    det_img = np.concatenate([i[o] for (i, _, _), o in zip(dets.per_class, orders)]).astype(np.int32)
    det_box = np.concatenate([b[o] for (_, _, b), o in zip(dets.per_class, orders)]).reshape(-1, 4)
    thr = np.array([t / 100.0 for t in IOU_THRESHOLDS], dtype=np.float64)
    import torch
    from . import ops

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)

    out = ops.voc_eval(dev(det_off, torch.int64), dev(det_img, torch.int32), dev(det_box, torch.float64),
                       dev(gt.gt_off, torch.int64), dev(gt.gt_box, torch.float64), dev(gt.gt_diff, torch.uint8),
                       dev(gt.npos, torch.int64), dev(gt.npos_im, torch.int64), dev(thr, torch.float64),
                       dev(RECALL_LEVELS, torch.float64)).cpu().numpy()          # the one device-to-host copy
    return {"ap_area": out[0] * 100, "ap_07": out[1] * 100, "corloc": out[2] * 100 if corloc else None}


def summarize(ap, corloc):
    """PVE's final means over per-class [K, 10] arrays (percent) -> {"bbox": {AP, AP50, AP75}, "bbox CorLoc": {CL, CL50, CL75}}"""
    ret = OrderedDict()
    mAP = {iou: np.mean(ap[:, t].tolist()) for t, iou in enumerate(IOU_THRESHOLDS)}
    ret["bbox"] = {"AP": np.mean(list(mAP.values())), "AP50": mAP[50], "AP75": mAP[75]}
    mCL = {iou: np.mean(corloc[:, t].tolist()) for t, iou in enumerate(IOU_THRESHOLDS)}
    ret["bbox CorLoc"] = {"CL": np.mean(list(mCL.values())), "CL50": mCL[50], "CL75": mCL[75]}
    return ret


def _dist_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def gather_lines(lines, num_classes):
    """{class: [line]} of every rank, concatenated per class in rank order, on rank 0; None on the other ranks"""
    import torch.distributed as dist
    rank, world = _dist_world()
    if world == 1:
        return {k: list(lines.get(k, [])) for k in range(num_classes)}
    gathered = [None] * world if rank == 0 else None
    dist.gather_object(lines, gathered, dst=0)
    if rank != 0:
        return None
    return {k: [x for part in gathered for x in part.get(k, [])] for k in range(num_classes)}


class PascalVOCDetectionEvaluator:
    """VOC mAP and CorLoc of a split, the reference's `PascalVOCDetectionEvaluator` (evaluation/pascal_voc_evaluation.py).

    dirname: the dataset directory holding Annotations/ and ImageSets/Main/ (e.g. datasets/VOC2007); year 2007 selects the
    11-point AP, 2012 the area AP.  `process` makes the reference's text lines (`inference.VOCDetectionWriter`).  `evaluate`
    gathers them to rank 0 when a process group of more than one rank is initialised (other ranks return None) and returns
    {"bbox": {"AP", "AP50", "AP75"}, "bbox CorLoc": {"CL", "CL50", "CL75"}}; the per-class values behind the means are kept in
    `per_class_ap` and `per_class_corloc` (f64 [K, 10], percent, thresholds 50, 55, ..., 95).  With save_detection_result the
    JSON records are written to save_path.format("voc_{year}_{split}") first.  The reference's comp4_* files under the dataset's
    results/ directory are not written.  See the module docstring for the tie rule and the two ValueErrors."""

    def __init__(self, dirname, split, year, class_names=VOC_CLASS_NAMES, save_detection_result=False, save_path=None):
        year = int(year)
        if year not in (2007, 2012):
            raise ValueError(f"year {year}: VOC evaluation knows 2007 and 2012")
        if year == 2012 and split == "test":
            raise ValueError("voc_2012_test has no public annotations")
        if save_detection_result and not save_path:
            raise ValueError("save_detection_result needs a save_path")
        self.dirname, self.split, self.year = dirname, split, year
        self.dataset_name = f"voc_{year}_{split}"
        self.class_names = tuple(class_names)
        self.save_detection_result = save_detection_result
        self.save_path = save_path
        self._writer = VOCDetectionWriter(len(self.class_names))
        self._gt = None
        self.per_class_ap = self.per_class_corloc = None

    def reset(self):
        self._writer.reset()

    def process(self, inputs, outputs):
        self._writer.process(inputs, outputs)

    def ground_truth(self):
        if self._gt is None:
            self._gt = GroundTruth.load(self.dirname, self.split, self.class_names)
        return self._gt

    def evaluate(self):
        lines = gather_lines(self._writer.lines(), len(self.class_names))
        if lines is None:
            return None
        if self.save_detection_result:
            VOCDetectionWriter.from_lines(lines).dump(self.save_path.format(self.dataset_name))
        gt = self.ground_truth()
        res = voc_eval_arrays(gt, Detections.from_lines(lines, gt))
        self.per_class_ap = res["ap_07"] if self.year == 2007 else res["ap_area"]
        self.per_class_corloc = res["corloc"]
        return summarize(self.per_class_ap, self.per_class_corloc)


# ---- COCO bbox evaluation ----------------------------------------------------------------------------------------------------
# pycocotools' Params.setDetParams, in its own expressions (the f64 values of these arrays are the thresholds)
COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_MAX_DETS = (1, 10, 100)
COCO_AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
COCO_AREA_LBL = ("all", "small", "medium", "large")
COCO_METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
_COCO_WALKS = len(COCO_AREA_RNG) * len(COCO_IOU_THRS)


class COCOGroundTruth:
    """The ground truth of a COCO annotation file as the reference's `COCO` + `COCOeval._prepare` read it.

    img_ids / cat_ids: the sorted unique ids of "images" / "categories" (COCOeval's params.imgIds / catIds);
    thing_dataset_id_to_contiguous_id: sorted category ids -> 0..K-1 and thing_classes: their names, as load_coco_json builds
    them.  Per annotation, in file order (annotations of an image or category outside the lists are never read): ann_img (index
    into img_ids), ann_cat (contiguous), ann_box [x, y, w, h] f64, ann_area (the annotation's own "area"), ann_crowd (its
    "iscrowd", which _prepare also makes its ignore flag, overwriting any "ignore" key), ann_idpos (id > 0)."""

    def __init__(self, dataset):
        if "annotations" not in dataset:
            raise ValueError("the COCO file has no annotations (a test split): nothing to evaluate against")
        self.img_ids = sorted({im["id"] for im in dataset.get("images", [])})
        cats = {c["id"]: c.get("name", str(c["id"])) for c in dataset.get("categories", [])}
        self.cat_ids = sorted(cats)
        if not 1 <= len(self.cat_ids) <= COCO_MAX_CLASSES:
            raise ValueError(f"{len(self.cat_ids)} categories: the evaluation kernel takes 1..{COCO_MAX_CLASSES}")
        self.thing_classes = [cats[c] for c in self.cat_ids]
        self.thing_dataset_id_to_contiguous_id = {c: k for k, c in enumerate(self.cat_ids)}
        self.img_index = {i: k for k, i in enumerate(self.img_ids)}
        img, cat, box, area, crowd, idpos = [], [], [], [], [], []
        for a in dataset["annotations"]:
            i, c = self.img_index.get(a["image_id"]), self.thing_dataset_id_to_contiguous_id.get(a["category_id"])
            if i is None or c is None:
                continue
            img.append(i)
            cat.append(c)
            box.append([float(v) for v in a["bbox"]])
            area.append(float(a["area"]))
            crowd.append(bool(a.get("iscrowd", 0)))
            idpos.append(int(a["id"]) > 0)
        self.ann_img = np.asarray(img, dtype=np.int64)
        self.ann_cat = np.asarray(cat, dtype=np.int64)
        self.ann_box = np.asarray(box, dtype=np.float64).reshape(-1, 4)
        self.ann_area = np.asarray(area, dtype=np.float64)
        self.ann_crowd = np.asarray(crowd, dtype=bool)
        self.ann_idpos = np.asarray(idpos, dtype=bool)
        if not (np.isfinite(self.ann_box).all() and np.isfinite(self.ann_area).all()):
            raise ValueError("COCO evaluation needs finite ground-truth boxes and areas")

    @classmethod
    def load(cls, json_file):
        with open(json_file) as f:
            return cls(json.load(f))

    def select(self, img_ids=None):
        """positions of the evaluated images: (sorted unique ids, pos [len(self.img_ids)] i64 with -1 for an image left out)"""
        if img_ids is None:
            return list(self.img_ids), np.arange(len(self.img_ids), dtype=np.int64)
        ids = sorted(set(img_ids))
        unknown = [i for i in ids if i not in self.img_index]
        if unknown:
            raise ValueError(f"img_ids {unknown[:5]} are not in the annotation file")
        pos = np.full(len(self.img_ids), -1, dtype=np.int64)
        pos[[self.img_index[i] for i in ids]] = np.arange(len(ids))
        return ids, pos


class COCODetections:
    """A COCO result list as `COCO.loadRes` reads it for boxes, in list order (the 1-based position is the detection's id):
    img (index into gt.img_ids), cat (contiguous class), score f64, box [x, y, w, h] f64; area = w * h is taken on the GPU."""

    def __init__(self, img, cat, score, box):
        self.img = np.asarray(img, dtype=np.int64)
        self.cat = np.asarray(cat, dtype=np.int64)
        self.score = np.asarray(score, dtype=np.float64)
        self.box = np.asarray(box, dtype=np.float64).reshape(-1, 4)
        if not (np.isfinite(self.score).all() and np.isfinite(self.box).all()):
            raise ValueError("COCO evaluation needs finite boxes and scores")

    @classmethod
    def from_results(cls, results, gt):
        """[{"image_id", "category_id" (dataset id), "bbox" XYWH, "score"}].  An image outside the annotation file is a ValueError
        (loadRes asserts); a category outside it is dropped silently (getAnnIds(catIds=...) never returns it)."""
        img, cat, score, box = [], [], [], []
        for r in results:
            if "bbox" not in r or "segmentation" in r or "keypoints" in r:
                raise ValueError("only bbox results are evaluated (segm and keypoints are out of scope)")
            i = gt.img_index.get(r["image_id"])
            if i is None:
                raise ValueError(f"detection for image {r['image_id']!r}, which is not in the annotation file")
            c = gt.thing_dataset_id_to_contiguous_id.get(r["category_id"])
            if c is None:
                continue
            img.append(i)
            cat.append(c)
            score.append(float(r["score"]))
            box.append([float(v) for v in r["bbox"]])
        return cls(img, cat, score, box)


def coco_pair_workspace_words(D, G, lds_doubles=COCO_LDS_DOUBLES):
    """numpy form of sw_coco_eval_workspace_bytes / 8: the 8-byte words an (image, category) pair of D detections and G ground
    truths needs in the global workspace, 0 when its IoU matrix fits the wave's LDS slice"""
    D, G = np.asarray(D, dtype=np.int64), np.asarray(G, dtype=np.int64)
    fits = (G <= 64) & (D * G <= lds_doubles)
    return np.where(fits, 0, D * G + _COCO_WALKS * ((G + 63) // 64) + 2 * G)


def coco_eval_layout(gt, dets, img_ids=None, lds_doubles=COCO_LDS_DOUBLES):
    """The kernel's arrays (include/soswsod_hip.h, sw_coco_eval) of one evaluation, on the host: the detections grouped by
    (category, image) in stable descending score order and cut at 100 per pair, each category's stable score order, the ground
    truth CSR over (image, category), npig."""
    ids, pos = gt.select(img_ids)
    n_img, K, A = len(ids), len(gt.cat_ids), len(COCO_AREA_RNG)
    # ground truth
    gi = pos[gt.ann_img]
    keep = gi >= 0
    gkey = gi[keep] * K + gt.ann_cat[keep]
    gorder = np.argsort(gkey, kind="stable")
    gt_off = np.zeros(n_img * K + 1, dtype=np.int64)
    np.cumsum(np.bincount(gkey, minlength=n_img * K), out=gt_off[1:])
    area, crowd = gt.ann_area[keep][gorder], gt.ann_crowd[keep][gorder]
    gcat = gt.ann_cat[keep][gorder]
    npig = np.zeros((K, A), dtype=np.int64)
    for a, (lo, hi) in enumerate(COCO_AREA_RNG):
        valid = ~(crowd | (area < lo) | (area > hi))
        npig[:, a] = np.bincount(gcat[valid], minlength=K)
    # detections: category-major, images in imgIds order, stable descending score inside a pair, the first 100 of a pair
    di = pos[dets.img] if len(dets.img) else np.zeros(0, dtype=np.int64)
    dsel = np.nonzero(di >= 0)[0]
    dkey = dets.cat[dsel] * n_img + di[dsel]
    o = dsel[np.lexsort((-dets.score[dsel], dkey))]                # lexsort is stable: ties stay in list (id) order
    key = dets.cat[o] * n_img + di[o]
    start = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0] if len(o) else np.zeros(0, dtype=np.int64)
    rank = np.arange(len(o)) - np.repeat(start, np.diff(np.r_[start, len(o)]))
    cut = rank < COCO_MAX_DETS[-1]
    o, key, rank = o[cut], key[cut], rank[cut]
    start = np.nonzero(rank == 0)[0]
    pair_off = np.r_[start, len(o)].astype(np.int64)
    pkey = key[start]
    pair_gt = (pkey % n_img) * K + pkey // n_img if len(start) else np.zeros(0, dtype=np.int64)
    cat = dets.cat[o]
    cat_off = np.searchsorted(cat, np.arange(K + 1)).astype(np.int64)
    score = dets.score[o]
    order = np.lexsort((-score, cat)).astype(np.int32)
    D, G = np.diff(pair_off), (gt_off[pair_gt + 1] - gt_off[pair_gt]) if len(start) else np.zeros(0, dtype=np.int64)
    words = coco_pair_workspace_words(D, G, lds_doubles)
    pair_ws = np.where(words > 0, np.cumsum(words) - words, -1).astype(np.int64)
    return dict(n_img=n_img, K=K, pair_off=pair_off, pair_gt=pair_gt.astype(np.int64), pair_ws=pair_ws, ws_words=int(words.sum()),
                det_box=dets.box[o], det_rank=rank.astype(np.uint8), det_score=score, det_index=o, gt_off=gt_off,
                gt_box=gt.ann_box[keep][gorder], gt_area=area,
                gt_flags=(crowd.astype(np.uint8) | (gt.ann_idpos[keep][gorder].astype(np.uint8) << 1)), cat_off=cat_off,
                order=order, npig=npig)


def coco_eval_arrays(gt, dets, img_ids=None, device="cuda", lds_doubles=COCO_LDS_DOUBLES):
    """COCOeval_opt's evaluate() + accumulate() on the GPU (`ops.coco_eval`: two launches, one device-to-host copy).
    -> {"precision" [T, R, K, A, M], "recall" [T, K, A, M], "scores" [T, R, K, A, M], "counts" [T, R, K, A, M]} with T = 10 IoU
    thresholds, R = 101 recall levels, K categories, A = 4 area ranges, M = 3 maxDets, -1 where there is no ground truth."""
    import torch
    from . import ops
    L = coco_eval_layout(gt, dets, img_ids, lds_doubles)

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)

    i64, f64 = torch.int64, torch.float64
    out, _ = ops.coco_eval(dev(L["pair_off"], i64), dev(L["pair_gt"], i64), dev(L["pair_ws"], i64), L["ws_words"],
                           dev(L["det_box"], f64), dev(L["gt_off"], i64), dev(L["gt_box"], f64), dev(L["gt_area"], f64),
                           dev(L["gt_flags"], torch.uint8), dev(np.asarray(COCO_AREA_RNG, dtype=np.float64), f64),
                           dev(COCO_IOU_THRS, f64), dev(COCO_REC_THRS, f64), dev(np.asarray(COCO_MAX_DETS), torch.int32),
                           dev(L["cat_off"], i64), dev(L["order"], torch.int32), dev(L["det_rank"], torch.uint8),
                           dev(L["det_score"], f64), dev(L["npig"], i64), lds_doubles=lds_doubles)
    host = out.cpu().numpy()                                       # the one device-to-host copy
    if np.isnan(host).any():
        raise RuntimeError("sw_coco_eval: a pair's workspace region lies outside the workspace")
    counts = [len(COCO_IOU_THRS), len(COCO_REC_THRS), L["K"], len(COCO_AREA_RNG), len(COCO_MAX_DETS)]
    n = int(np.prod(counts))
    return {"precision": host[:n].reshape(counts), "scores": host[n:2 * n].reshape(counts),
            "recall": host[2 * n:].reshape(counts[:1] + counts[2:]), "counts": counts}


def coco_summarize(ev):
    """COCOeval.summarize's twelve stats of an accumulated evaluation, in pycocotools' expressions"""
    def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
        aind = [i for i, lbl in enumerate(COCO_AREA_LBL) if lbl == areaRng]
        mind = [i for i, m in enumerate(COCO_MAX_DETS) if m == maxDets]
        s = ev["precision"] if ap == 1 else ev["recall"]
        if iouThr is not None:
            s = s[np.where(iouThr == COCO_IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    stats = np.zeros((12,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5, maxDets=COCO_MAX_DETS[2])
    stats[2] = _summarize(1, iouThr=.75, maxDets=COCO_MAX_DETS[2])
    stats[3] = _summarize(1, areaRng="small", maxDets=COCO_MAX_DETS[2])
    stats[4] = _summarize(1, areaRng="medium", maxDets=COCO_MAX_DETS[2])
    stats[5] = _summarize(1, areaRng="large", maxDets=COCO_MAX_DETS[2])
    stats[6] = _summarize(0, maxDets=COCO_MAX_DETS[0])
    stats[7] = _summarize(0, maxDets=COCO_MAX_DETS[1])
    stats[8] = _summarize(0, maxDets=COCO_MAX_DETS[2])
    stats[9] = _summarize(0, areaRng="small", maxDets=COCO_MAX_DETS[2])
    stats[10] = _summarize(0, areaRng="medium", maxDets=COCO_MAX_DETS[2])
    stats[11] = _summarize(0, areaRng="large", maxDets=COCO_MAX_DETS[2])
    return stats


def derive_coco_results(ev, stats, class_names=None):
    """COCOEvaluator._derive_coco_results for "bbox" (coco_evaluation.py:294-360); ev None: no predictions, every metric NaN"""
    if ev is None:
        return {metric: float("nan") for metric in COCO_METRICS}
    results = {metric: float(stats[idx] * 100 if stats[idx] >= 0 else "nan") for idx, metric in enumerate(COCO_METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    precisions = ev["precision"]
    if len(class_names) != precisions.shape[2]:
        raise ValueError(f"{len(class_names)} class names for {precisions.shape[2]} categories")
    for idx, name in enumerate(class_names):
        precision = precisions[:, :, idx, 0, -1]
        precision = precision[precision > -1]
        ap = np.mean(precision) if precision.size else float("nan")
        results["AP-" + "{}".format(name)] = float(ap * 100)
    return results


def instances_to_coco_json(instances, img_id):
    """an image's Instances -> COCO result dicts with XYWH boxes (coco_evaluation.py: instances_to_coco_json); masks and
    keypoints are refused"""
    if instances.has("pred_masks") or instances.has("pred_keypoints"):
        raise ValueError("only bbox results are evaluated (segm and keypoints are out of scope)")
    if len(instances) == 0:
        return []
    boxes = instances.pred_boxes.tensor.cpu().numpy().copy()
    boxes[:, 2] -= boxes[:, 0]                                     # BoxMode.convert XYXY_ABS -> XYWH_ABS, in the boxes' dtype
    boxes[:, 3] -= boxes[:, 1]
    boxes = boxes.tolist()
    scores = instances.scores.tolist()
    classes = instances.pred_classes.tolist()
    return [{"image_id": img_id, "category_id": classes[k], "bbox": boxes[k], "score": scores[k]} for k in range(len(scores))]


def gather_predictions(predictions):
    """the prediction lists of every rank, concatenated in rank order, on rank 0; None on the other ranks"""
    import torch.distributed as dist
    rank, world = _dist_world()
    if world == 1:
        return list(predictions)
    gathered = [None] * world if rank == 0 else None
    dist.gather_object(predictions, gathered, dst=0)
    if rank != 0:
        return None
    return [x for part in gathered for x in part]


class COCOEvaluator:
    """COCO bbox AP of a split, the reference's `COCOEvaluator` with use_fast_impl (evaluation/coco_evaluation.py) for the
    "bbox" task.

    json_file: the COCO annotation file; thing_classes: names for the per-class "AP-<name>" entries (default: the file's
    category names in id order).  `process` keeps `{"image_id", "instances": [COCO result dicts, contiguous classes]}` per
    image; `evaluate(img_ids=None)` gathers them to rank 0 in rank order when a process group of more than one rank is
    initialised (other ranks return {}), maps the classes to dataset ids and returns {"bbox": {AP, AP50, AP75, APs, APm, APl,
    AP-<name>...}} in percent, NaN where COCOeval has -1.  No predictions returns {}; predictions without any instance give the
    all-NaN dict.  `eval` holds the accumulated arrays, `stats` COCOeval's twelve numbers.  With save_detection_result the
    gathered predictions are written to save_path.format(name) first (Stage 2's `pgf_coco` reads that file); output_dir
    receives coco_instances_results.json.  Outputs with masks or keypoints are refused: segm and keypoints are out of scope (so
    is LVIS, for which there is no evaluator here).  Outputs with "proposals" are refused too unless box_proposals=True: then
    `process` keeps them (moved to the CPU, coco_evaluation.py:141-142) and `evaluate` writes the reference's box_proposals.pkl
    into output_dir and adds {"box_proposals": {AR@100, ARs@100, ARm@100, ARl@100, AR@1000, ...}} (box_proposals.py; one launch),
    beside "bbox" when instances were given too.  `set_predictions` takes the records of an
    earlier run (the save_detection_result file) in place of `process`.  Kept from the reference: an annotation whose id is 0 can never be a true positive
    (cocoeval.cpp tests the matched id > 0), though it does take its detection."""

    def __init__(self, json_file, thing_classes=None, output_dir=None, save_detection_result=False, save_path=None,
                 name="coco", box_proposals=False):
        if save_detection_result and not save_path:
            raise ValueError("save_detection_result needs a save_path")
        self.json_file = json_file
        self.dataset_name = name
        self.output_dir = output_dir
        self.save_detection_result = save_detection_result
        self.save_path = save_path
        self._thing_classes = thing_classes
        self.box_proposals = bool(box_proposals)
        self._gt = None
        self._predictions = []
        self.eval = self.stats = None

    def reset(self):
        self._predictions = []

    def set_predictions(self, predictions):
        """replace what `process` collected by the per-image records of an earlier run: [{"image_id", "instances": [...]}]"""
        self._predictions = list(predictions)

    def ground_truth(self):
        if self._gt is None:
            self._gt = COCOGroundTruth.load(self.json_file)
        return self._gt

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            if "proposals" in out and not self.box_proposals:
                raise ValueError("box-proposal AR is out of scope: COCOEvaluator takes outputs with 'instances' only "
                                 "(COCOEvaluator(..., box_proposals=True) evaluates proposals)")
            prediction = {"image_id": inp["image_id"]}
            if "instances" in out:
                prediction["instances"] = instances_to_coco_json(out["instances"], inp["image_id"])
            if "proposals" in out:
                prediction["proposals"] = out["proposals"].to("cpu")
            self._predictions.append(prediction)

    def evaluate(self, img_ids=None):
        predictions = gather_predictions(self._predictions)
        if predictions is None:
            return {}
        if self.save_detection_result:
            with open(self.save_path.format(self.dataset_name), "w") as f:
                json.dump([{k: v for k, v in x.items() if k != "proposals"} for x in predictions], f)
        if len(predictions) == 0:
            return {}
        results = OrderedDict()
        if "proposals" in predictions[0]:                          # coco_evaluation.py:175-176, before the instances
            results["box_proposals"] = self._eval_box_proposals(predictions)
        if "instances" not in predictions[0]:
            return results
        results["bbox"] = self._eval_instances(predictions, img_ids)
        return results

    def _eval_box_proposals(self, predictions):
        """coco_evaluation.py:255-292: box_proposals.pkl into output_dir, then the eight ARs"""
        from .box_proposals import box_proposal_metrics, write_box_proposals
        if self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            write_box_proposals(predictions, os.path.join(self.output_dir, "box_proposals.pkl"))
        return box_proposal_metrics(predictions, self.ground_truth())

    def _eval_instances(self, predictions, img_ids):
        gt = self.ground_truth()
        reverse = {v: k for k, v in gt.thing_dataset_id_to_contiguous_id.items()}
        coco_results = []
        for x in predictions:
            for r in x["instances"]:
                if r["category_id"] not in reverse:
                    raise ValueError(f"A prediction has category_id={r['category_id']}, which is not available in the dataset.")
                coco_results.append(dict(r, category_id=reverse[r["category_id"]]))
        if self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            with open(os.path.join(self.output_dir, "coco_instances_results.json"), "w") as f:
                f.write(json.dumps(coco_results))
        names = gt.thing_classes if self._thing_classes is None else list(self._thing_classes)
        if len(coco_results) == 0:                                 # "cocoapi does not handle empty results very well"
            self.eval = self.stats = None
        else:
            self.eval = coco_eval_arrays(gt, COCODetections.from_results(coco_results, gt), img_ids=img_ids)
            self.stats = coco_summarize(self.eval)
        return derive_coco_results(self.eval, self.stats, names)


def evaluate_coco_results(results, json_file, img_ids=None):
    """the evaluator's numbers for a COCO result list (coco_instances_results.json) -> (result dict, eval arrays, stats)"""
    gt = COCOGroundTruth.load(json_file)
    if len(results) == 0:
        return OrderedDict(bbox=derive_coco_results(None, None)), None, None
    ev = coco_eval_arrays(gt, COCODetections.from_results(results, gt), img_ids=img_ids)
    stats = coco_summarize(ev)
    return OrderedDict(bbox=derive_coco_results(ev, stats, gt.thing_classes)), ev, stats


def inference_on_dataset(model, data_loader, evaluator):
    """Run the model over the loader in eval mode without gradients and evaluate (evaluation/evaluator.py:101, timing logs left
    out); the model's training mode is restored afterwards."""
    import torch
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            evaluator.reset()
            for inputs in data_loader:
                evaluator.process(inputs, model(inputs))
    finally:
        model.train(was_training)
    results = evaluator.evaluate()
    return {} if results is None else results


def parse_args(argv=None):
    p = argparse.ArgumentParser("python -m sos_wsod_amd.evaluation",
                                description="VOC mAP and CorLoc of a detection file (VOCDetectionWriter.dump JSON), or with "
                                            "--coco-json the COCO bbox AP of a coco_instances_results.json; with --proposals "
                                            "the box-proposal AR of a proposal pickle against either ground truth.")
    p.add_argument("--voc-root", default=None, help="dataset directory holding Annotations/ and ImageSets/Main/")
    p.add_argument("--split", default="test")
    p.add_argument("--year", type=int, default=2007, choices=(2007, 2012))
    p.add_argument("--coco-json", default=None, help="COCO annotation file: evaluate --detections as a COCO result list instead")
    p.add_argument("--detections", default=None, help="JSON list of {image_id, category_id (1-based), score, bbox}; with "
                                                      "--coco-json: {image_id, category_id (dataset id), bbox XYWH, score}")
    p.add_argument("--proposals", default=None, help="a proposal pickle (box_proposals.pkl, or a converted MCG / Selective Search "
                                                     "file): print AR@100 ... ARl@1000 instead; takes no --detections")
    p.add_argument("--out", default=None, help="also write the metrics and per-class arrays here as JSON")
    args = p.parse_args(argv)
    if args.proposals is not None:
        if args.detections is not None:
            p.error("--proposals and --detections exclude each other")
        if (args.voc_root is None) == (args.coco_json is None):
            p.error("--proposals needs one of --coco-json and --voc-root")
        paths = [(args.proposals, "--proposals")]
        paths.append((args.coco_json, "--coco-json") if args.coco_json is not None else
                     (os.path.join(args.voc_root, "ImageSets", "Main", args.split + ".txt"), "--voc-root/--split image set"))
        for path, what in paths:
            if not os.path.isfile(path):
                p.error(f"{what}: no file {path}")
        return args
    # --voc-root is required unless --coco-json is given, --detections always: argparse's own message for what is missing
    missing = [flag for flag, v in (("--voc-root", args.voc_root if args.coco_json is None else ""), ("--detections", args.detections))
               if v is None]
    if missing:
        p.error("the following arguments are required: " + ", ".join(missing))
    if args.coco_json is not None:
        if args.voc_root is not None:
            p.error("--coco-json and --voc-root exclude each other")
        for path, what in ((args.detections, "--detections"), (args.coco_json, "--coco-json")):
            if not os.path.isfile(path):
                p.error(f"{what}: no file {path}")
        return args
    if args.year == 2012 and args.split == "test":
        p.error("voc_2012_test has no public annotations")
    for path, what in ((args.detections, "--detections"), (os.path.join(args.voc_root, "ImageSets", "Main", args.split + ".txt"),
                                                            "--voc-root/--split image set")):
        if not os.path.isfile(path):
            p.error(f"{what}: no file {path}")
    return args


def evaluate_records(records, dirname, split, year, class_names=VOC_CLASS_NAMES):
    """the evaluator's numbers for a list of JSON records -> (result dict, per-class AP [K, 10], per-class CorLoc [K, 10])"""
    gt = GroundTruth.load(dirname, split, class_names)
    res = voc_eval_arrays(gt, Detections.from_records(records, gt))
    ap = res["ap_07"] if int(year) == 2007 else res["ap_area"]
    return summarize(ap, res["corloc"]), ap, res["corloc"]


def evaluate_proposal_file(path, json_file=None, voc_root=None, split="test"):
    """AR@100 ... ARl@1000 of a proposal pickle against a COCO annotation file, or against a VOC split as convert_to_coco_json
    would describe it"""
    from .box_proposals import box_proposal_metrics, predictions_from_file, voc_ground_truth
    gt = COCOGroundTruth.load(json_file) if json_file is not None else voc_ground_truth(voc_root, split)
    return box_proposal_metrics(predictions_from_file(path), gt)


def main(argv=None):
    args = parse_args(argv)
    if args.proposals is not None:
        result = OrderedDict(box_proposals=evaluate_proposal_file(args.proposals, args.coco_json, args.voc_root, args.split))
        print(json.dumps(result))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f)
        return result
    with open(args.detections) as f:
        records = json.load(f)
    if args.coco_json is not None:
        result, ev, stats = evaluate_coco_results(records, args.coco_json)
        print(json.dumps(result))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(dict(result, stats=None if stats is None else stats.tolist(),
                               recall=None if ev is None else ev["recall"].tolist()), f)
        return result
    result, ap, cl = evaluate_records(records, args.voc_root, args.split, args.year)
    out = {k: {m: float(v) for m, v in d.items()} for k, d in result.items()}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(out, per_class={"thresholds": list(IOU_THRESHOLDS), "AP": ap.tolist(), "CorLoc": cl.tolist()}), f)
    return result


if __name__ == "__main__":
    main()

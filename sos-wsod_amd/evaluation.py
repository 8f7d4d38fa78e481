"""VOC detection evaluation: mAP and CorLoc at the IoU thresholds 0.50:0.05:0.95, the numbers SoS-WSOD reports.

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
"""
import argparse
import json
import os
import xml.etree.ElementTree as ET
from collections import OrderedDict

import numpy as np

from .inference import VOCDetectionWriter

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
                                description="VOC mAP and CorLoc of a detection file (VOCDetectionWriter.dump JSON).")
    p.add_argument("--voc-root", required=True, help="dataset directory holding Annotations/ and ImageSets/Main/")
    p.add_argument("--split", default="test")
    p.add_argument("--year", type=int, default=2007, choices=(2007, 2012))
    p.add_argument("--detections", required=True, help="JSON list of {image_id, category_id (1-based), score, bbox}")
    p.add_argument("--out", default=None, help="also write the metrics and per-class arrays here as JSON")
    args = p.parse_args(argv)
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


def main(argv=None):
    args = parse_args(argv)
    with open(args.detections) as f:
        records = json.load(f)
    result, ap, cl = evaluate_records(records, args.voc_root, args.split, args.year)
    out = {k: {m: float(v) for m, v in d.items()} for k, d in result.items()}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(out, per_class={"thresholds": list(IOU_THRESHOLDS), "AP": ap.tolist(), "CorLoc": cl.tolist()}), f)
    return result


if __name__ == "__main__":
    main()

"""How good are the Stage-2 pseudo labels?  The pseudo-ground-truth filter (`pseudo_labels`, the reference's tools/pgf.py) at every
cell of a grid t_keep x t_con, each cell's kept boxes matched against the ground truth that VOC and COCO trainval do have.

One launch (`ops.pgf_sweep`) and one device-to-host copy per split give integer count tables per cell and class:
    kept  [nk, nc, K]       detections the filter keeps at (t_keep[a], t_con[b]) — exactly what `filter_groups` keeps there
    tp    [nt, nk, nc, K]   ground-truth objects a kept detection claims at IoU threshold iou[t]
    ign   [nt, nk, nc, K]   kept detections whose best object is ignored (VOC difficult, COCO iscrowd)
    npos  [K]               non-ignored ground-truth objects
Matching is voc_eval's rule (evaluation/pascal_voc_evaluation.py:357-397): a detection's candidates are its image's objects of
its class, the best one by numpy's max / argmax (the first maximum wins), a match needs IoU > threshold.  Which object a
detection claims does not depend on the other detections, so the claimed objects are what the reference's sequential
"first unclaimed match is the true positive" loop counts.  precision = tp / (kept - ign), recall = tp / npos.

VOC: detections are VOCDetectionWriter records `[x1 + 1, y1 + 1, x2, y2]`, matched as they stand with `+ 1` extents against the
annotation's 1-based corners; the dataset dicts hold 0-based x1 / y1 (the loader's `- 1`), which is undone here.  COCO: XYWH
detections become (x, y, x + w, y + h), extents without `+ 1`.

`pseudo_label_records` turns a written VOC pseudo-label file into the records `python -m sos_wsod_amd.evaluation --detections`
reads, for the mAP and CorLoc of the pseudo labels at one threshold pair.
"""
import argparse
import json
import os

import numpy as np

from . import pseudo_labels as P

IOU_THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))
MAX_KEEP, MAX_CON, MAX_IOU = 32, 32, 10           # SW_PGF_SWEEP_MAX_KEEP / _MAX_CON / _MAX_IOU
XYXY_ABS, XYWH_ABS = 0, 1                         # detectron2 BoxMode
METRICS = ("precision", "recall", "f1")


def _div(num, den):
    """num / den in float64, NaN where den is 0"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


class SweepResult:
    """The four count tables of one split with their grids; `classes[k]` is the class id of table column k."""

    def __init__(self, kept, tp, ign, npos, t_keep, t_con, iou, classes):
        self.kept, self.tp, self.ign, self.npos = (np.asarray(a, dtype=np.int64) for a in (kept, tp, ign, npos))
        self.t_keep, self.t_con, self.iou = ([float(v) for v in g] for g in (t_keep, t_con, iou))
        self.classes = [int(c) for c in classes]
        nk, nc, nt, K = len(self.t_keep), len(self.t_con), len(self.iou), len(self.classes)
        assert self.kept.shape == (nk, nc, K) and self.tp.shape == (nt, nk, nc, K) and self.ign.shape == (nt, nk, nc, K)
        assert self.npos.shape == (K,)

    def _sums(self, per_class):
        if per_class:
            return self.kept[None], self.tp, self.ign, self.npos
        return self.kept.sum(-1)[None], self.tp.sum(-1), self.ign.sum(-1), self.npos.sum()

    def precision(self, per_class=False):
        """tp / (kept - ign): [nt, nk, nc] micro-averaged over the classes, [nt, nk, nc, K] per class; NaN where nothing counts"""
        kept, tp, ign, _ = self._sums(per_class)
        return _div(tp, kept - ign)

    def recall(self, per_class=False):
        """tp / npos, NaN for a class (or a split) without a non-ignored object"""
        _, tp, _, npos = self._sums(per_class)
        return _div(tp, npos)

    def f1(self, per_class=False):
        """2 tp / (kept - ign + npos), the harmonic mean of precision and recall; NaN where either is undefined"""
        kept, tp, ign, npos = self._sums(per_class)
        out = _div(2 * tp, kept - ign + npos)
        out[np.isnan(self.precision(per_class)) | np.isnan(self.recall(per_class))] = np.nan
        return out

    def iou_index(self, iou):
        for t, v in enumerate(self.iou):
            if v == float(iou):
                return t
        raise ValueError(f"IoU {iou} is not one of {self.iou}")

    def best(self, metric="f1", iou=0.5):
        """The cell with the largest micro-averaged metric at that IoU; among equal cells the lowest t_keep, then the lowest
        t_con.  -> {"t_keep", "t_con", "a", "b", metric} or None when the metric is NaN everywhere"""
        if metric not in METRICS:
            raise ValueError(f"metric {metric!r} is not one of {METRICS}")
        table = getattr(self, metric)()[self.iou_index(iou)]
        best = None
        for a in range(len(self.t_keep)):
            for b in range(len(self.t_con)):
                v = table[a, b]
                if np.isnan(v):
                    continue
                key = (-v, self.t_keep[a], self.t_con[b])
                if best is None or key < best[0]:
                    best = (key, a, b)
        if best is None:
            return None
        _, a, b = best
        return {"t_keep": self.t_keep[a], "t_con": self.t_con[b], "a": a, "b": b, metric: float(table[a, b])}

    def to_json(self):
        """a dict json.dump takes: the grids, the class ids and the four tables as nested lists"""
        return {"t_keep": self.t_keep, "t_con": self.t_con, "iou": self.iou, "classes": self.classes, "kept": self.kept.tolist(),
                "tp": self.tp.tolist(), "ign": self.ign.tolist(), "npos": self.npos.tolist()}

    @classmethod
    def from_json(cls, d):
        return cls(d["kept"], d["tp"], d["ign"], d["npos"], d["t_keep"], d["t_con"], d["iou"], d["classes"])


def corners(bbox, mode):
    """an annotation's box as float64 corners (x1, y1, x2, y2)"""
    x, y, w, h = (float(v) for v in bbox)
    if int(mode) == XYXY_ABS:
        return [x, y, w, h]
    if int(mode) == XYWH_ABS:
        return [x, y, x + w, y + h]
    raise ValueError(f"bbox_mode {mode} is not supported (XYXY_ABS, XYWH_ABS)")


def pack_ground_truth(ids, annotations, universe, ignore_key, shift):
    """The objects of the images `ids`, in annotation order, as CSR arrays: annotations {image id: [annotation dict]};
    universe: the sorted class ids behind the dense indices; ignore_key: "difficult" or "iscrowd"; shift is added to the corners.
    -> (gt_off [n + 1] i64, gt_box [G, 4] f64, gt_cls [G] i32 dense, gt_ign [G] u8)"""
    off = np.zeros(len(ids) + 1, dtype=np.int64)
    box, cls, ign = [], [], []
    for k, i in enumerate(ids):
        for a in annotations[i]:
            box.append(corners(a["bbox"], a.get("bbox_mode", XYXY_ABS)))
            cls.append(a["category_id"])
            ign.append(1 if a.get(ignore_key, 0) else 0)
        off[k + 1] = len(cls)
    gt_box = np.array(box, dtype=np.float64).reshape(len(cls), 4) + np.asarray(shift, dtype=np.float64)
    if not np.isfinite(gt_box).all():
        raise ValueError("the sweep needs finite ground-truth boxes")
    gt_cls = np.searchsorted(universe, np.array(cls, dtype=np.int64)).astype(np.int32)
    return off, gt_box, gt_cls, np.array(ign, dtype=np.uint8)


def check_grid(t_keep, t_con, iou):
    t_keep, t_con, iou = ([float(v) for v in np.atleast_1d(np.asarray(g, dtype=np.float64))] for g in (t_keep, t_con, iou))
    for name, g, cap in (("t_keep", t_keep, MAX_KEEP), ("t_con", t_con, MAX_CON), ("iou", iou, MAX_IOU)):
        if not 1 <= len(g) <= cap:
            raise ValueError(f"{name}: {len(g)} values, the sweep takes 1..{cap}")
        if not np.isfinite(g).all():
            raise ValueError(f"{name}: the values must be finite")
    return t_keep, t_con, iou


def sweep_groups(groups, annotations, t_keep, t_con, iou, use_diff, diff_classes, ignore_key, xywh, plus_one, shift):
    """The sweep over {image id: [detection dict]} (0-based classes) and {image id: [annotation dict]} for the same ids, on the GPU"""
    import torch
    from . import ops

    t_keep, t_con, iou = check_grid(t_keep, t_con, iou)
    class_dict = {i: P._unique(a["category_id"] for a in annotations[i]) for i in groups}
    g = P.pack_groups(groups, class_dict, diff_classes)
    gt_off, gt_box, gt_cls, gt_ign = pack_ground_truth(g["ids"], annotations, g["universe"], ignore_key, shift)
    dev = torch.device("cuda", torch.cuda.current_device())

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    K = g["K"]
    packed = ops.pgf_sweep(up(g["off"]), up(g["boxes"]), up(g["scores"]), up(g["classes"]), K, up(g["gt_mask"].view(np.int32)),
                           up(g["diff_mask"].view(np.int32)), use_diff, t_keep, t_con, iou, up(gt_off), up(gt_box), up(gt_cls),
                           up(gt_ign), xywh, plus_one)
    host = packed.cpu().numpy()                   # the split's one device-to-host copy
    t = ops.pgf_sweep_unpack(host, len(t_keep), len(t_con), len(iou), K)
    classes = g["universe"].tolist() if len(g["universe"]) else [0]
    return SweepResult(t["kept"], t["tp"], t["ign"], t["npos"], t_keep, t_con, iou, classes)


def _annotations(dataset_dicts, key):
    """{key(image_id): annotations}; a repeated image id keeps its position and takes the last dict's, as gt_classes does"""
    anns = {}
    for d in dataset_dicts:
        anns[key(d["image_id"])] = d["annotations"]
    return anns


def voc_groups(detections, dataset_dicts):
    """pgf_voc's grouping on copies: records with 0-based classes per image in first-appearance order, then the ground-truth images
    without a record (their objects count in npos).  -> (groups, annotations)"""
    anns = _annotations(dataset_dicts, int)
    groups = {}
    for rec in detections:
        if rec["image_id"] in anns:
            groups.setdefault(rec["image_id"], []).append(dict(rec, category_id=rec["category_id"] - 1))
    for i in anns:
        groups.setdefault(i, [])
    return groups, anns


def coco_groups(detections, dataset_dicts):
    """pgf_coco's grouping (the last entry of a repeated image id wins), then the ground-truth images without an entry"""
    anns = _annotations(dataset_dicts, lambda i: i)
    groups = {}
    for rec in detections:
        if rec["image_id"] in anns:
            groups[rec["image_id"]] = list(rec["instances"])
    for i in anns:
        groups.setdefault(i, [])
    return groups, anns


def sweep_voc(detections, dataset_dicts, t_keep, t_con, iou=IOU_THRESHOLDS, use_diff=False, diff_classes=P.VOC_DIFF_CLASSES):
    """The sweep of one VOC split.  detections: VOCDetectionWriter records (1-based category_id; left as they are);
    dataset_dicts: the split's dicts with "bbox" (x1 and y1 0-based, as the loader leaves them), "bbox_mode", "category_id"
    (0-based) and "difficult" in the annotations.  -> SweepResult"""
    groups, anns = voc_groups(detections, dataset_dicts)
    return sweep_groups(groups, anns, t_keep, t_con, iou, use_diff, diff_classes, "difficult", False, True, (1.0, 1.0, 0.0, 0.0))


def sweep_coco(detections, dataset_dicts, t_keep, t_con, iou=IOU_THRESHOLDS, use_diff=True):
    """The sweep of one COCO split.  detections: [{"image_id", "instances": [{"bbox" XYWH, "category_id" contiguous 0-based,
    "score"}]}]; dataset_dicts with "bbox", "bbox_mode", "category_id" (contiguous) and "iscrowd".  -> SweepResult"""
    if not use_diff:
        raise ValueError("COCO has no difficult-class list: the reference fails without use_diff (pass --use-diff)")
    groups, anns = coco_groups(detections, dataset_dicts)
    return sweep_groups(groups, anns, t_keep, t_con, iou, True, (), "iscrowd", True, False, (0.0, 0.0, 0.0, 0.0))


def score(detections, dataset_dicts, dataset="voc", t_con=P.T_CON, t_keep=P.T_KEEP, iou=IOU_THRESHOLDS, use_diff=None):
    """the 1 x 1 grid at one threshold pair"""
    if dataset == "coco":
        return sweep_coco(detections, dataset_dicts, [t_keep], [t_con], iou, True if use_diff is None else use_diff)
    return sweep_voc(detections, dataset_dicts, [t_keep], [t_con], iou, bool(use_diff))


def pseudo_label_records(pgt):
    """A VOC pseudo-label file ({image id: [records with 0-based category_id]}, its "multi_label" entry skipped) or its path
    -> the 1-based records `python -m sos_wsod_amd.evaluation --detections` reads, in file order"""
    if isinstance(pgt, str):
        with open(pgt) as f:
            pgt = json.load(f)
    out = []
    for key, records in pgt.items():
        if key == "multi_label":
            continue
        for r in records:
            out.append({"image_id": r["image_id"], "category_id": r["category_id"] + 1, "score": r["score"], "bbox": list(r["bbox"])})
    return out


def parse_grid(text):
    """"lo:hi:step" (hi included when a whole number of steps reaches it, each value lo + i * step rounded to 10 decimals) or a
    comma list -> [float]"""
    if ":" in text:
        parts = text.split(":")
        if len(parts) != 3:
            raise ValueError(f"range {text!r} is not lo:hi:step")
        lo, hi, step = (float(p) for p in parts)
        if not step > 0 or hi < lo:
            raise ValueError(f"range {text!r} needs step > 0 and hi >= lo")
        n = int(np.floor((hi - lo) / step + 1e-9)) + 1
        return [round(lo + i * step, 10) for i in range(n)]
    return [float(p) for p in text.split(",") if p.strip()]


def format_table(result, metric="f1", iou=0.5):
    """the micro-averaged metric at one IoU as text: a row per t_keep, a column per t_con"""
    table = getattr(result, metric)()[result.iou_index(iou)]
    lines = ["t_keep \\ t_con " + " ".join(f"{v:>7.4g}" for v in result.t_con)]
    for a, tk in enumerate(result.t_keep):
        lines.append(f"{tk:>14.4g} " + " ".join(f"{v:7.4f}" for v in table[a]))
    return "\n".join(lines)


def parse_args(argv=None):
    p = argparse.ArgumentParser("python -m sos_wsod_amd.pgf_sweep",
                                description="Score the Stage-2 pseudo labels against the ground truth over a grid of PGF thresholds.")
    p.add_argument("--det-path", default="datasets/VOC2007/detection_results/")
    p.add_argument("--prefix", default="oicr_plus_")
    p.add_argument("--dataset", default="voc2007", choices=("voc2007", "voc2012", "coco"))
    p.add_argument("--gt-dicts", required=True,
                   help="JSON {dataset name: [dataset dicts]} with the ground truth of both splits (boxes and difficult / iscrowd "
                        "flags included), e.g. voc_2007_train and voc_2007_val")
    p.add_argument("--t-keep", default="0:1:0.05", help="lo:hi:step or a comma list, at most 32 values")
    p.add_argument("--t-con", default="0.5:1:0.05", help="lo:hi:step or a comma list, at most 32 values")
    p.add_argument("--iou", default=",".join(str(v) for v in IOU_THRESHOLDS), help="comma list, at most 10 values; holds 0.5")
    p.add_argument("--use-diff", action="store_true")
    p.add_argument("--out", default=None, help="write the tables of every split here as JSON")
    args = p.parse_args(argv)
    if args.dataset == "coco" and not args.use_diff:
        p.error("--dataset coco needs --use-diff: COCO has no difficult-class list")
    try:
        args.t_keep, args.t_con, args.iou = check_grid(parse_grid(args.t_keep), parse_grid(args.t_con), parse_grid(args.iou))
    except ValueError as e:
        p.error(str(e))
    if 0.5 not in args.iou:
        p.error("--iou must hold 0.5: the printed table is at IoU 0.5")
    return args


def main(argv=None):
    args = parse_args(argv)
    with open(args.gt_dicts) as f:
        gt = json.load(f)
    if args.dataset == "coco":
        names = ["coco_2014_train", "coco_2014_valminusminival"]
    else:
        names = [f"voc_{args.dataset[3:]}_{split}" for split in ("train", "val")]
    print("t_keep", json.dumps([repr(v) for v in args.t_keep]))
    print("t_con", json.dumps([repr(v) for v in args.t_con]))
    out = {}
    for name in names:
        with open(os.path.join(args.det_path, f"{args.prefix}{name}.json")) as f:
            dets = json.load(f)
        if args.dataset == "coco":
            result = sweep_coco(dets, gt[name], args.t_keep, args.t_con, args.iou, args.use_diff)
        else:
            result = sweep_voc(dets, gt[name], args.t_keep, args.t_con, args.iou, args.use_diff)
        best = result.best("f1", 0.5)
        print(f"{name}: F1 at IoU 0.5")
        print(format_table(result))
        print(name, "best", json.dumps(best))
        out[name] = dict(result.to_json(), best=best)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)
    return out


if __name__ == "__main__":
    main()

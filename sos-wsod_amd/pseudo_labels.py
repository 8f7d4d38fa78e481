"""Stage 2 of SoS-WSOD: pseudo-ground-truth filtering (PGF) of the Stage-1 detections into the Stage-3 pseudo labels.

Port of the reference's `tools/pgf.py` and `tools/add_multi_label.py`, plus the dataset dicts its Stage-3 tree builds from a
pseudo-label file (`detectron2/data/datasets/pascal_voc.py:89-156`, `load_voc_instances_wsl`).  The per-image filtering runs on
the GPU (`ops.pgf_keep`, one launch and one device-to-host copy per split); grouping, JSON and bookkeeping stay on the host.

The reference's semantics are kept, quirks included:
  * VOC records are `{"image_id", "category_id" (1-based), "score", "bbox": [x1 + 1, y1 + 1, x2, y2]}` (what
    `inference.VOCDetectionWriter` writes).  `category_id -= 1` mutates the caller's records in place, before a record of an
    image absent from the ground truth is skipped.
  * `contain_cal` reads every box as [x, y, w, h] — on VOC records, which hold corners, that is a reinterpretation the reference
    makes and this port keeps: x2' = x2 + x1 + 1, and so on.
  * The containment test is pairwise over the keep-stage survivors: a box that is itself dropped still drops the boxes it
    contains, and two identical boxes drop each other.
  * COCO passes no difficult classes, so the reference fails on COCO without `--use-diff`; here that combination is a ValueError.
"""
import argparse
import json
import os

import numpy as np

T_CON = 0.85
T_KEEP = 0.2
VOC_DIFF_CLASSES = (4, 5, 6, 8, 9, 15, 16)        # 0-based: boat, bottle, bus, chair, cow, pottedplant, sheep (pgf.py:99)
COCO_ID2CAT = {
    0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 8, 8: 9, 9: 10, 10: 11, 11: 13, 12: 14, 13: 15, 14: 16, 15: 17, 16: 18, 17: 19,
    18: 20, 19: 21, 20: 22, 21: 23, 22: 24, 23: 25, 24: 27, 25: 28, 26: 31, 27: 32, 28: 33, 29: 34, 30: 35, 31: 36, 32: 37, 33: 38,
    34: 39, 35: 40, 36: 41, 37: 42, 38: 43, 39: 44, 40: 46, 41: 47, 42: 48, 43: 49, 44: 50, 45: 51, 46: 52, 47: 53, 48: 54, 49: 55,
    50: 56, 51: 57, 52: 58, 53: 59, 54: 60, 55: 61, 56: 62, 57: 63, 58: 64, 59: 65, 60: 67, 61: 70, 62: 72, 63: 73, 64: 74, 65: 75,
    66: 76, 67: 77, 68: 78, 69: 79, 70: 80, 71: 81, 72: 82, 73: 84, 74: 85, 75: 86, 76: 87, 77: 88, 78: 89, 79: 90}
STAT_KEYS = ("before_class_filter", "after_class_filter", "after_keep", "after_containment")
XYXY_ABS = 0                                      # detectron2 BoxMode.XYXY_ABS


def _unique(values):
    out = []
    for v in values:
        if v not in out:
            out.append(v)
    return out


def gt_classes(dataset_dicts, key=lambda image_id: image_id):
    """{key(image_id): the image's ground-truth classes, unique, in first-appearance order}; a repeated image id keeps its
    position and takes the last dict's annotations (pgf.py:36-45,71-89)"""
    anns = {}
    for d in dataset_dicts:
        anns[key(d["image_id"])] = d["annotations"]
    return {i: _unique(a["category_id"] for a in ann) for i, ann in anns.items()}


def pack_groups(groups, class_dict, diff_classes=()):
    """{image_id: [detection dict]} and {image_id: ground-truth classes} as the arrays the filter kernels read: detections back to
    back in group order (CSR), the classes that occur renamed to dense indices 0..K-1, class bitmasks per image.
    -> dict: ids, dets, off, boxes, scores, classes (dense i32), universe (the class id of each dense index), K, gt_mask, diff_mask"""
    ids = list(groups)
    dets = [d for i in ids for d in groups[i]]
    n = len(dets)
    counts = np.fromiter((len(groups[i]) for i in ids), dtype=np.int64, count=len(ids))
    off = np.zeros(len(ids) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    boxes = np.array([d["bbox"] for d in dets], dtype=np.float64).reshape(n, 4)
    scores = np.array([d["score"] for d in dets], dtype=np.float64).reshape(n)
    if not (np.isfinite(boxes).all() and np.isfinite(scores).all()):
        raise ValueError("pseudo-label filtering needs finite boxes and scores")
    det_cls = np.array([d["category_id"] for d in dets], dtype=np.int64).reshape(n)
    img_gt = [class_dict[i] for i in ids]
    gt_flat = np.array([c for cs in img_gt for c in cs], dtype=np.int64)
    # the kernel sees dense class indices 0..K-1 over every class that occurs; membership tests are unchanged by the renaming
    universe = np.unique(np.concatenate([det_cls, gt_flat]))
    K = max(len(universe), 1)
    if K > 256:
        raise ValueError(f"{K} distinct classes: the filter supports up to 256")
    words = (K + 31) // 32
    gt_mask = np.zeros((len(ids), words), dtype=np.uint32)
    if len(gt_flat):
        gi = np.repeat(np.arange(len(ids)), [len(cs) for cs in img_gt])
        gc = np.searchsorted(universe, gt_flat)
        np.bitwise_or.at(gt_mask, (gi, gc >> 5), (np.uint32(1) << (gc & 31).astype(np.uint32)))
    diff_mask = np.zeros(words, dtype=np.uint32)
    for c in diff_classes:
        k = np.searchsorted(universe, c)
        if k < len(universe) and universe[k] == c:
            diff_mask[k >> 5] |= np.uint32(1) << np.uint32(k & 31)
    return {"ids": ids, "dets": dets, "off": off, "boxes": boxes, "scores": scores, "universe": universe, "K": K,
            "classes": np.searchsorted(universe, det_cls).astype(np.int32), "gt_mask": gt_mask, "diff_mask": diff_mask}


def filter_groups(groups, class_dict, t_con=T_CON, t_keep=T_KEEP, use_diff=False, diff_classes=()):
    """Stages 3-5 of the reference (class_filter, then pgf) over {image_id: [detection dict]} on the GPU.
    -> ({image_id: [kept detection dicts]} in the same order, stats dict)"""
    import torch
    from . import ops

    t_con, t_keep = float(t_con), float(t_keep)
    g = pack_groups(groups, class_dict, diff_classes)
    ids, dets, off, n = g["ids"], g["dets"], g["off"], len(g["dets"])

    dev = torch.device("cuda", torch.cuda.current_device())

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    packed = ops.pgf_keep(up(off), up(g["boxes"]), up(g["scores"]), up(g["classes"]), g["K"], up(g["gt_mask"].view(np.int32)),
                          up(g["diff_mask"].view(np.int32)), t_keep, t_con, use_diff)
    host = packed.cpu().numpy()                   # the split's one device-to-host copy
    stats = dict(zip(STAT_KEYS, (int(v) for v in host[:32].view(np.int64))))
    assert stats["before_class_filter"] == n, (stats, n)
    keep = host[32:].astype(bool)
    out = {}
    for k, i in enumerate(ids):
        a, b = int(off[k]), int(off[k + 1])
        out[i] = [d for d, kp in zip(dets[a:b], keep[a:b]) if kp]
    return out, stats


def pgf_voc(detections, dataset_dicts, t_con=T_CON, t_keep=T_KEEP, use_diff=False, diff_classes=VOC_DIFF_CLASSES):
    """pgf_voc of the reference for one split (pgf.py:23-104).  detections: the list VOCDetectionWriter.records() returns
    (its category_id is decremented IN PLACE, as the reference does); dataset_dicts: the split's ground-truth dataset dicts.
    -> ({image_id: [kept records]} in first-appearance order, stats)"""
    class_dict = gt_classes(dataset_dicts, key=int)
    groups = {}
    for rec in detections:
        rec["category_id"] = rec["category_id"] - 1
        if rec["image_id"] not in class_dict:
            continue
        groups.setdefault(rec["image_id"], []).append(rec)
    return filter_groups(groups, class_dict, t_con, t_keep, use_diff, diff_classes)


def pgf_coco(detections, dataset_dicts, t_con=T_CON, t_keep=T_KEEP, use_diff=True):
    """pgf_coco of the reference for one split (pgf.py:106-189).  detections: [{"image_id", "instances": [{"bbox" XYWH,
    "category_id" contiguous 0-based, "score", ...}]}], the last entry of a repeated image id winning.
    -> ({image_id: [kept instances]}, stats); gen_annotations() turns the result into COCO annotations"""
    if not use_diff:
        raise ValueError("COCO has no difficult-class list: the reference fails without use_diff (pass --use-diff)")
    class_dict = gt_classes(dataset_dicts)
    groups = {}
    for rec in detections:
        if rec["image_id"] in class_dict:
            groups[rec["image_id"]] = list(rec["instances"])
    return filter_groups(groups, class_dict, t_con, t_keep, True, ())


def gen_annotations(result, id2cat=COCO_ID2CAT):
    """COCO annotations of the kept instances (pgf.py:191-207): running "id" from 0, category mapped back by id2cat"""
    anns = []
    for img_id, preds in result.items():
        for p in preds:
            anns.append({"image_id": img_id, "bbox": p["bbox"], "category_id": id2cat[p["category_id"]], "id": len(anns)})
    return anns


def coco_pseudo_labels(base, result, id2cat=COCO_ID2CAT):
    """the COCO annotation dict `base` with its "annotations" replaced by the pseudo labels (pgf.py:176-185)"""
    out = dict(base)
    out["annotations"] = gen_annotations(result, id2cat)
    return out


def add_multi_label(pgt, dataset_dicts, coco=False):
    """pgt["multi_label"] = {image id: ground-truth classes, unique, first-appearance order} (add_multi_label.py:15-42); VOC keys
    are str(int(image_id)), COCO keys the image ids.  Mutates and returns pgt."""
    pgt["multi_label"] = gt_classes(dataset_dicts) if coco else gt_classes(dataset_dicts, key=lambda i: str(int(i)))
    return pgt


def write_json(obj, path):
    """json.dump as the reference writes its outputs (default separators; int keys become strings)"""
    with open(path, "w") as f:
        json.dump(obj, f)


def load_voc_pseudo_labels(pgt, images):
    """The Stage-3 dataset dicts of a VOC pseudo-label file (the Stage-3 tree's load_voc_instances_wsl,
    detectron2/data/datasets/pascal_voc.py:89-156).  pgt: the file's dict (or its path); images: the split's image records in
    split order, {"image_id": file id string, "file_name", "height", "width"}.  Boxes become int lists in XYXY_ABS — the
    writer's +1 on x1 / y1 is never undone — category ids stay as stored, "multi_label" is copied when the file has one."""
    if isinstance(pgt, str):
        with open(pgt) as f:
            pgt = json.load(f)
    multi = pgt.get("multi_label")
    dicts = []
    for im in images:
        fileid = im["image_id"]
        key = str(int(fileid))
        r = {"file_name": im["file_name"], "image_id": fileid, "height": im["height"], "width": im["width"]}
        r["annotations"] = [{"category_id": o["category_id"], "bbox": [int(v) for v in o["bbox"]], "bbox_mode": XYXY_ABS}
                            for o in pgt[key]]
        if multi is not None:
            r["multi_label"] = multi[key]
        dicts.append(r)
    return dicts


def parse_args(argv=None):
    p = argparse.ArgumentParser("python -m sos_wsod_amd.pseudo_labels",
                                description="Stage 2: filter Stage-1 detections into Stage-3 pseudo labels (PGF).")
    p.add_argument("--det-path", default="datasets/VOC2007/detection_results/")
    p.add_argument("--save-path", default="datasets/VOC2007/pseudo_labels/")
    p.add_argument("--prefix", default="oicr_plus_")
    p.add_argument("--dataset", default="voc2007", choices=("voc2007", "voc2012", "coco"))
    p.add_argument("--coco-path", default="datasets/coco/", help="COCO root: annotations/instances_*2014.json are the base files")
    p.add_argument("--gt-dicts", required=True,
                   help="JSON {dataset name: [dataset dicts]} with the ground truth of both splits, e.g. voc_2007_train and "
                        "voc_2007_val, or coco_2014_train and coco_2014_valminusminival")
    p.add_argument("--t-con", type=float, default=T_CON)
    p.add_argument("--t-keep", type=float, default=T_KEEP)
    p.add_argument("--use-diff", action="store_true")
    p.add_argument("--multi-label", action="store_true", help="also add the multi_label entry (add_multi_label.py)")
    args = p.parse_args(argv)
    if args.dataset == "coco" and not args.use_diff:
        p.error("--dataset coco needs --use-diff: COCO has no difficult-class list")
    return args


def main(argv=None):
    args = parse_args(argv)
    with open(args.gt_dicts) as f:
        gt = json.load(f)
    os.makedirs(args.save_path, exist_ok=True)
    if args.dataset == "coco":
        splits = [("coco_2014_train", "instances_train2014.json", "coco_2014_train"),
                  ("coco_2014_valminusminival", "instances_valminusminival2014.json", "coco_2014_valminusminival2014")]
        for name, base_file, out_name in splits:
            with open(os.path.join(args.det_path, f"{args.prefix}{name}.json")) as f:
                dets = json.load(f)
            result, stats = pgf_coco(dets, gt[name], args.t_con, args.t_keep, args.use_diff)
            with open(os.path.join(args.coco_path, "annotations", base_file)) as f:
                out = coco_pseudo_labels(json.load(f), result)
            if args.multi_label:
                add_multi_label(out, gt[name], coco=True)
            write_json(out, os.path.join(args.save_path, f"{args.prefix}{out_name}.json"))
            print(name, json.dumps(stats))
    else:
        year = args.dataset[3:]
        for split in ("train", "val"):
            name = f"voc_{year}_{split}"
            with open(os.path.join(args.det_path, f"{args.prefix}{name}.json")) as f:
                dets = json.load(f)
            result, stats = pgf_voc(dets, gt[name], args.t_con, args.t_keep, args.use_diff)
            if args.multi_label:
                add_multi_label(result, gt[name])
            write_json(result, os.path.join(args.save_path, f"{args.prefix}{name}.json"))
            print(name, json.dumps(stats))


if __name__ == "__main__":
    main()

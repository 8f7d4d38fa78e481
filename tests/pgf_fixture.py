"""The Stage-2 fixtures tests/golden/pgf_voc.npz and pgf_coco.npz (written by tests/golden/make_pgf_golden.py): the arrays they
hold and the JSON records they stand for.  The reference's output files are kept as their SHA-256 and their four counts."""
import hashlib
import json
import os

import numpy as np

CASES = {"voc_a": "voc", "voc_b": "voc", "coco_a": "coco"}
SPLITS = ("train", "val")


def sha256(text):
    return hashlib.sha256(text.encode()).hexdigest()


def load(golden_dir, dataset):
    with np.load(os.path.join(golden_dir, f"pgf_{dataset}.npz")) as z:
        return dict(z)


def params(z, case):
    """-> (t_con, t_keep, use_diff)"""
    t_con, t_keep, use_diff = z[f"{case}_params"].tolist()
    return t_con, t_keep, bool(use_diff)


def _det(z, s):
    return (z[f"{s}_det_{k}"].tolist() for k in ("image", "cat", "score", "bbox"))


def voc_records(z, s):
    """VOCDetectionWriter.records() of the split: {"image_id", "category_id" (1-based), "score", "bbox"}"""
    return [{"image_id": i, "category_id": c, "score": p, "bbox": b} for i, c, p, b in zip(*_det(z, s))]


def coco_records(z, s):
    """[{"image_id", "instances": [{"image_id", "category_id", "bbox" XYWH, "score"}]}] of the split"""
    inst = [{"image_id": i, "category_id": c, "bbox": b, "score": p} for i, c, p, b in zip(*_det(z, s))]
    off = z[f"{s}_entry_off"].tolist()
    return [{"image_id": e, "instances": inst[off[k]:off[k + 1]]} for k, e in enumerate(z[f"{s}_entry_image"].tolist())]


def gt_dicts(z, s, voc):
    """the ground-truth dataset dicts (only what PGF reads: image_id — a file id string for VOC — and annotation classes)"""
    ids, off, cls = z[f"{s}_gt_image"].tolist(), z[f"{s}_gt_off"].tolist(), z[f"{s}_gt_cls"].tolist()
    return [{"image_id": f"{i:06d}" if voc else i, "annotations": [{"category_id": c} for c in cls[off[k]:off[k + 1]]]}
            for k, i in enumerate(ids)]


def coco_base(z, s):
    return json.loads(str(z[f"{s}_base"]))


def voc_images(z, s):
    """the image records the Stage-3 loader was run over, in split order"""
    return [{"image_id": f"{i:06d}", "file_name": f"VOC2007/JPEGImages/{i:06d}.jpg", "height": h, "width": w}
            for i, h, w in zip(*(z[f"{s}_img_{k}"].tolist() for k in ("id", "h", "w")))]


def voc_unfiltered_pgt(z, s):
    """{image_id: records, category ids made 0-based} for every detection of an image in the ground truth: the pseudo-label file
    the fixtures' add_voc07 and load_voc_instances_wsl runs read (host-only parts, checked without the filter)"""
    gt = set(z[f"{s}_gt_image"].tolist())
    pgt = {}
    for r in voc_records(z, s):
        if r["image_id"] in gt:
            r["category_id"] -= 1
            pgt.setdefault(r["image_id"], []).append(r)
    return pgt

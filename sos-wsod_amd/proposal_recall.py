"""Proposal conversion and proposal recall: the file Stage 1 trains from, and how good it is.

Port of the reference's `uwsod/projects/WSL/tools/proposal_convert.py` (`convert_ss_box`, `convert_mcg_box`) and
`uwsod/projects/WSL/tools/proposal_recall.py` (`recall_mcg`, `recall_ss`, `recall_eb` and the budget loop of its `__main__`).

Recall is the share of ground-truth boxes whose best overlap with the `m` best proposals of their image reaches an IoU threshold,
for m = 4 ... 2048 and the thresholds 0.50:0.05:1.00.  The reference runs its whole loop once per budget, re-reading every `.mat`
file; the budgets are nested prefixes of one ranked list, so here the host reads and ranks once and one kernel launch
(`ops.proposal_recall`) gives every row.  The overlaps, the maxima and the counts are computed on the GPU in float64, in the
reference's operation order, so `ovmax`, `jmax`, `cnt_yes` and `recall` are bit-identical to the reference's.

What stays on the host: reading the files, the reference's own `[:, (1, 0, 3, 2)] - 1` in the file's dtype (for an unsigned dtype a
0 coordinate wraps, as there), and the ranking `np.argsort(-(scores.flatten()))` — NumPy's default sort is not stable, so among
equal scores the order is whatever that call gives on this host, as in the reference; a device-side sort could not reproduce it.
The `ss` mode has no ranking: the reference draws `np.random.choice(n, size=min(n, m), replace=False)` per image inside the
budget loop, so the draws of one budget are not a prefix of the next; `ss` takes a `np.random.RandomState`, makes the same draws
in the same order and launches once per budget.

What differs from the reference:
  * float32 (or float16) box arrays are a ValueError: the reference computes those in float32 with scalar promotion that depends
    on the NumPy version; promoting silently would change results.  Integer and float64 arrays are computed in float64, which is
    what NumPy does for them there.  One corner is kept bit for bit: `boxes[:, 2] - boxes[:, 0]` of an integer array wraps in the
    array's dtype before `+ 1.0` makes it a float (a uint16 box whose 0 coordinate became 65535).  Such a box has no intersection
    with any ground truth; it is handed to the kernel as a box of the same wrapped width and height far outside every image.
  * The sign of a zero `ovmax`.  A signed-integer box with xmax < xmin (the converted pickle holds them: uint16 65535 became int16
    -1) has a negative area, and its zero overlap is -0.0.  For a prefix that holds both zeros `np.max` returns either, depending
    on how the host's vector unit folds the array; here `ovmax` is always the overlap at `jmax`, the first of equal values.
    Recall and `jmax` are not affected.
  * Ground-truth coordinates are read as Python floats (the reference would compute integer-typed annotations against an integer
    box array in that integer dtype).  Non-finite boxes, and ground-truth coordinates of magnitude 2^39 or more, are a ValueError.
  * An image with ground truth and no proposals is a ValueError up front (the reference raises from `np.max` of an empty array
    when it gets there); a split without ground truth is a ValueError (the reference divides by zero).
  * `recall_ssopg` (one experiment's dump) and `convert_mcg_seg*` (superpixel masks, which nothing here consumes) are not ported.

    python -m sos_wsod_amd.proposal_recall recall  --mode {mcg,ss,eb,pkl} --proposals PATH (--voc-root DIR [--split S] [--year Y] | --coco-json FILE)
    python -m sos_wsod_amd.proposal_recall convert --mode {mcg,ss} --proposals PATH --out FILE.pkl (the same ground-truth flags)
"""
import argparse
import json
import os
import pickle
import xml.etree.ElementTree as ET

import numpy as np

from .proposals import read_proposal_file

IOU_THRESHOLDS = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95, 1.0)          # proposal_recall.py:9
BUDGETS = (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)                                # proposal_recall.py:390
MAX_CUTS, MAX_THRESHOLDS = 16, 16                     # SW_PROPOSAL_RECALL_MAX_CUTS / SW_PROPOSAL_RECALL_MAX_THRESHOLDS
RANKED_MODES = ("mcg", "eb", "pkl")
MODES = RANKED_MODES + ("ss",)
_FAR = float(2 ** 40)                                 # where a wrapped box goes: exact in f64 with any integer extent added


# ---------------------------------------------------------------------------------------------------------------------- readers
def file_stem(record, dataset_name):
    """the name of an image's `.mat` file (proposal_recall.py:158-163)"""
    if "flickr" in dataset_name or "coco" in dataset_name:
        return os.path.basename(record["file_name"])[:-4]
    return record["image_id"]


def read_mcg_dir(dataset_dicts, dir_in, dataset_name):
    """One `.mat` per image (proposal_recall.py:158-176) -> {"boxes": [n_i x 4 arrays, xyxy 0-based, the file's dtype],
    "scores": [the file's score arrays, n_i x 1]}"""
    import scipy.io as sio
    boxes, scores = [], []
    for d in dataset_dicts:
        mat_data = sio.loadmat(os.path.join(dir_in, "{}.mat".format(file_stem(d, dataset_name))))
        if "flickr" in dataset_name:
            boxes_data, scores_data = mat_data["bboxes"], mat_data["bboxes_scores"]
        else:
            boxes_data, scores_data = mat_data["boxes"], mat_data["scores"]
        boxes.append(boxes_data[:, (1, 0, 3, 2)] - 1)              # 1-indexed (y1, x1, y2, x2) in the file
        scores.append(scores_data)
    return {"boxes": boxes, "scores": scores}


def read_ss_mat(file_in):
    """The Selective Search file: one cell per image, no scores (proposal_recall.py:244, 255-257) -> {"boxes": [...]}"""
    import scipy.io as sio
    raw_data = sio.loadmat(file_in)["boxes"].ravel()
    return {"boxes": [raw_data[i][:, (1, 0, 3, 2)] - 1 for i in range(raw_data.shape[0])]}


def read_eb_mat(file_in):
    """The EdgeBoxes file: `boxes` and `boxScores` cells per image (proposal_recall.py:316-331)"""
    import scipy.io as sio
    mat_data = sio.loadmat(file_in)
    boxes_data = mat_data["boxes"].ravel()
    scores_data = mat_data["boxScores"].ravel()
    assert boxes_data.shape[0] == scores_data.shape[0]
    n = boxes_data.shape[0]
    return {"boxes": [boxes_data[i][:, (1, 0, 3, 2)] - 1 for i in range(n)], "scores": [scores_data[i][:] for i in range(n)]}


def read_proposal_pkl(path):
    """A converted proposal pickle, through `proposals.read_proposal_file` -> {"boxes", "scores", "ids"}; the boxes are already
    0-based xyxy"""
    p = read_proposal_file(path)
    return {"boxes": list(p["boxes"]), "scores": list(p["objectness_logits"]), "ids": list(p["ids"])}


# ---------------------------------------------------------------------------------------------------------------------- recall
def _aligned(dataset_dicts, proposals):
    """the per-image box and score lists in dataset order (by image id where the proposals carry ids, as the loader matches them)"""
    boxes, scores = proposals["boxes"], proposals.get("scores")
    if proposals.get("ids") is not None:
        at = {str(i): k for k, i in enumerate(proposals["ids"])}
        try:
            sel = [at[str(d["image_id"])] for d in dataset_dicts]
        except KeyError as e:
            raise ValueError(f"image {e.args[0]} has no entry in the proposal file") from None
        boxes = [boxes[k] for k in sel]
        scores = None if scores is None else [scores[k] for k in sel]
    if len(boxes) != len(dataset_dicts) or (scores is not None and len(scores) != len(dataset_dicts)):
        raise ValueError(f"{len(boxes)} proposal entries for {len(dataset_dicts)} images")          # the reference asserts
    return [np.asarray(b) for b in boxes], scores


def _boxes_f64(b):
    """an image's box array as the float64 rows the reference's arithmetic sees"""
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"a proposal box array has shape {b.shape}, not (n, 4)")
    if b.dtype.kind == "f" and b.dtype != np.float64:
        raise ValueError(f"proposal boxes of dtype {b.dtype} are not supported: the reference computes them in {b.dtype}; "
                         "convert them to float64 or to an integer dtype on purpose")
    if b.dtype.kind not in "iuf":
        raise ValueError(f"proposal boxes of dtype {b.dtype} are not supported")
    out = b.astype(np.float64)
    if not np.isfinite(out).all():
        raise ValueError("proposal boxes must be finite")
    if b.dtype.kind in "iu" and len(b):
        for lo, hi in ((0, 2), (1, 3)):
            ext = (b[:, hi] - b[:, lo]).astype(np.float64)          # in the array's dtype, as `boxes[:, 2] - boxes[:, 0]` there
            wrapped = ext != out[:, hi] - out[:, lo]
            if b.dtype.kind == "i" and wrapped.any():          # an extent beyond the signed dtype: such a box may still intersect
                raise ValueError(f"a proposal box extent overflows {b.dtype}")
            out[wrapped, lo] = _FAR
            out[wrapped, hi] = _FAR + ext[wrapped]
    return out


def _ground_truth(dataset_dicts, dataset_name):
    """-> gt_off [n_img + 1] i64, gt_box [G, 4] f64 xyxy (proposal_recall.py:197-202)"""
    off, box = [0], []
    for d in dataset_dicts:
        for a in d["annotations"]:
            bbgt = [float(v) for v in a["bbox"]]
            if "coco" in dataset_name:
                bbgt = [bbgt[0], bbgt[1], bbgt[0] + bbgt[2], bbgt[1] + bbgt[3]]
            box.append(bbgt)
        off.append(len(box))
    gt_box = np.asarray(box, dtype=np.float64).reshape(-1, 4)
    if not np.isfinite(gt_box).all():
        raise ValueError("ground-truth boxes must be finite")
    if gt_box.size and np.abs(gt_box).max() >= _FAR / 2:          # it could reach a wrapped proposal box where `_boxes_f64` puts it
        raise ValueError(f"ground-truth coordinates must be below {_FAR / 2:.0f} in magnitude")
    return np.asarray(off, dtype=np.int64), gt_box


def _launch(per_image, gt_off, gt_box, cuts, thresholds, device):
    """per_image: each image's f64 [n_i, 4] boxes in rank order -> (ovmax [G, n_cut], jmax [G, n_cut], cnt_yes [n_cut, n_thr])"""
    import torch
    from . import ops
    n = [len(b) for b in per_image]
    for i, k in enumerate(n):
        if k == 0 and gt_off[i + 1] > gt_off[i]:
            raise ValueError(f"image {i} has ground truth and no proposals")          # np.max of an empty array raises there
    prop_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    prop_box = np.concatenate(per_image).reshape(-1, 4) if per_image else np.zeros((0, 4), dtype=np.float64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)          # noqa: E731
    ovmax, jmax, cnt = ops.proposal_recall(up(prop_off), up(prop_box), up(gt_off), up(gt_box),
                                           up(np.asarray(cuts, dtype=np.int32)), up(np.asarray(thresholds, dtype=np.float64)))
    return ovmax.cpu().numpy(), jmax.cpu().numpy(), cnt.cpu().numpy()


def proposal_recall(dataset_dicts, proposals, dataset_name, budgets=BUDGETS, thresholds=IOU_THRESHOLDS, mode="mcg", rng=None,
                    device="cuda", return_matches=False):
    """Recall of the ground-truth boxes of `dataset_dicts` (records with "annotations"[*]["bbox"], XYWH when `dataset_name`
    contains "coco", else XYXY) by `proposals` ({"boxes": per-image [n_i, 4] arrays, "scores": per-image arrays, optional "ids"},
    as the readers above return them; without ids they are in dataset order).

    mode "mcg" / "eb" / "pkl": the proposals are ranked by `np.argsort(-(scores.flatten()))` and cut to the largest budget, as
    the reference does.  That sort is not stable: the order among equal scores is NumPy's on this host, as in the reference.
    mode "ss": no ranking; per budget (outer loop) and image, `rng.choice(n, size=min(n, budget), replace=False)` picks the
    boxes, so `rng = np.random.RandomState(s)` repeats the reference run after `np.random.seed(s)`.

    -> {"recall": [n_budget, n_thr] f64 (Python `cnt_yes / cnt_gt`), "cnt_yes": [n_budget, n_thr] i64, "cnt_gt": int,
        "budgets", "thresholds"}; with return_matches also "ovmax" [G, n_budget] f64 and "jmax" [G, n_budget] i32 (the best
    overlap of each ground-truth box and its index into the image's ranked, or drawn, list)."""
    budgets = [int(m) for m in budgets]
    thresholds = [float(t) for t in thresholds]
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {MODES}")
    if not budgets or budgets[0] < 1 or any(b <= a for a, b in zip(budgets, budgets[1:])):
        raise ValueError("budgets must be positive and strictly ascending")
    if not 1 <= len(thresholds) <= MAX_THRESHOLDS or (mode != "ss" and len(budgets) > MAX_CUTS):
        raise ValueError(f"at most {MAX_CUTS} budgets and {MAX_THRESHOLDS} thresholds per call")
    boxes, scores = _aligned(dataset_dicts, proposals)
    gt_off, gt_box = _ground_truth(dataset_dicts, dataset_name)
    cnt_gt = int(gt_off[-1])
    if cnt_gt == 0:
        raise ValueError("the split has no ground-truth boxes")
    if mode == "ss":
        if rng is None:
            raise ValueError('mode "ss" draws its boxes at random: pass rng=np.random.RandomState(seed)')
        f64 = [_boxes_f64(b) for b in boxes]
        ov, jm, cnt = [], [], []
        for m in budgets:
            drawn = []
            for b in f64:
                number_of_rows = b.shape[0]
                drawn.append(b[rng.choice(number_of_rows, size=min(number_of_rows, m), replace=False), ...])
            o, j, c = _launch(drawn, gt_off, gt_box, [m], thresholds, device)
            ov.append(o); jm.append(j); cnt.append(c)
        ovmax, jmax, cnt_yes = np.concatenate(ov, 1), np.concatenate(jm, 1), np.concatenate(cnt, 0)
    else:
        if scores is None:
            raise ValueError(f'mode {mode!r} ranks by score and the proposals carry none (mode "ss" draws at random)')
        ranked = []
        for b, s in zip(boxes, scores):
            sorted_ind = np.argsort(-(np.asarray(s).flatten()))
            ranked.append(_boxes_f64(b[sorted_ind, :][:budgets[-1], ...]))
        ovmax, jmax, cnt_yes = _launch(ranked, gt_off, gt_box, budgets, thresholds, device)
    recall = np.array([[1.0 * int(a) / cnt_gt for a in row] for row in cnt_yes], dtype=np.float64)
    out = {"recall": recall, "cnt_yes": cnt_yes, "cnt_gt": cnt_gt, "budgets": budgets, "thresholds": thresholds}
    if return_matches:
        out.update(ovmax=ovmax, jmax=jmax)
    return out


# ---------------------------------------------------------------------------------------------------------------------- conversion
def _dump(boxes, scores, ids, file_out):
    with open(file_out, "wb") as f:
        pickle.dump(dict(boxes=boxes, scores=scores, indexes=ids), f, pickle.HIGHEST_PROTOCOL)


def convert_ss_box(dataset_dicts, file_in, file_out, dataset_name):
    """The Selective Search `.mat` file -> the proposal pickle Stage 1 loads (proposal_convert.py:17-50): int16 boxes, scores of
    1.0, the records' image ids.  `dataset_name` is accepted for symmetry; the reference does not use it either."""
    boxes = read_ss_mat(file_in)["boxes"]
    assert len(boxes) == len(dataset_dicts)
    _dump([b.astype(np.int16) for b in boxes], [np.squeeze(np.ones((b.shape[0]), dtype=np.float32)) for b in boxes],
          [d["image_id"] for d in dataset_dicts], file_out)


def convert_mcg_box(dataset_dicts, dir_in, file_out, dataset_name):
    """A directory of MCG `.mat` files -> the proposal pickle (proposal_convert.py:53-95): int16 boxes, float32 scores"""
    p = read_mcg_dir(dataset_dicts, dir_in, dataset_name)
    _dump([b.astype(np.int16) for b in p["boxes"]], [np.squeeze(s.astype(np.float32)) for s in p["scores"]],
          [d["image_id"] for d in dataset_dicts], file_out)


# ---------------------------------------------------------------------------------------------------------------------- records
def voc_records(dirname, split, keep_difficult=False):
    """The records the reference's `load_voc_instances` builds (uwsod/detectron2/data/datasets/pascal_voc.py:36-85), as far as
    these tools read them: image_id, file_name and the boxes with xmin / ymin minus 1.  That loader leaves out the objects
    marked difficult; `keep_difficult` keeps them."""
    with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
        fileids = [x.strip() for x in f if x.strip()]
    dicts = []
    for fileid in fileids:
        r = {"file_name": os.path.join(dirname, "JPEGImages", fileid + ".jpg"), "image_id": fileid, "annotations": []}
        anno_file = os.path.join(dirname, "Annotations", fileid + ".xml")
        if os.path.isfile(anno_file):
            for obj in ET.parse(anno_file).findall("object"):
                if int(obj.find("difficult").text) == 1 and not keep_difficult:
                    continue
                bbox = obj.find("bndbox")
                bbox = [float(bbox.find(x).text) for x in ["xmin", "ymin", "xmax", "ymax"]]
                bbox[0] -= 1.0
                bbox[1] -= 1.0
                r["annotations"].append({"bbox": bbox})
        dicts.append(r)
    return dicts


def coco_records(json_file):
    """The records of a COCO annotation file, sorted by image id as detectron2's `load_coco_json` returns them (the cells of an
    `ss` or `eb` file are in that order): image_id, file_name, and the XYWH boxes `evaluation.COCOGroundTruth` read, in annotation
    order"""
    from .evaluation import COCOGroundTruth
    with open(json_file) as f:
        dataset = json.load(f)
    gt = COCOGroundTruth(dataset)
    names = {im["id"]: im.get("file_name", f"{im['id']}.jpg") for im in dataset.get("images", [])}
    records = [{"file_name": names[i], "image_id": i, "annotations": []} for i in gt.img_ids]
    for k, box in zip(gt.ann_img.tolist(), gt.ann_box.tolist()):
        records[k]["annotations"].append({"bbox": box})
    return records


# ---------------------------------------------------------------------------------------------------------------------- CLI
def format_table(result):
    head = "budget " + " ".join(f"{t:>7.2f}" for t in result["thresholds"])
    rows = [f"{m:>6d} " + " ".join(f"{v:>7.4f}" for v in row) for m, row in zip(result["budgets"], result["recall"])]
    return "\n".join([head] + rows)


def parse_args(argv=None):
    p = argparse.ArgumentParser("python -m sos_wsod_amd.proposal_recall",
                                description="Recall of a proposal set at IoU 0.50:0.05:1.00 for the 4 ... 2048 best proposals per "
                                            "image, or conversion of MCG / Selective Search .mat files to the Stage-1 pickle.")
    sub = p.add_subparsers(dest="command", required=True)
    for name, modes in (("recall", MODES), ("convert", ("mcg", "ss"))):
        q = sub.add_parser(name)
        q.add_argument("--mode", required=True, choices=modes,
                       help="mcg: a directory of .mat files; ss / eb: one .mat file" + ("; pkl: a converted pickle" if name == "recall" else ""))
        q.add_argument("--proposals", required=True, help="the directory or file to read")
        q.add_argument("--voc-root", default=None, help="dataset directory holding Annotations/ and ImageSets/Main/")
        q.add_argument("--split", default="test")
        q.add_argument("--year", type=int, default=2007, choices=(2007, 2012))
        q.add_argument("--keep-difficult", action="store_true", help="VOC: keep the objects marked difficult")
        q.add_argument("--coco-json", default=None, help="COCO annotation file instead of --voc-root")
        q.add_argument("--dataset-name", default=None, help="default: voc_{year}_{split}, or coco_ + the JSON's name")
        if name == "recall":
            q.add_argument("--seed", type=int, default=0, help="mode ss: the seed of the random draws")
            q.add_argument("--out", default=None, help="also write the table here as JSON")
        else:
            q.add_argument("--out", required=True, help="the pickle to write")
    args = p.parse_args(argv)
    if (args.voc_root is None) == (args.coco_json is None):
        p.error("give one of --voc-root and --coco-json")
    if not os.path.exists(args.proposals):
        p.error(f"--proposals: no file or directory {args.proposals}")
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.coco_json is not None:
        records = coco_records(args.coco_json)
        name = args.dataset_name or "coco_" + os.path.splitext(os.path.basename(args.coco_json))[0]
    else:
        records = voc_records(args.voc_root, args.split, args.keep_difficult)
        name = args.dataset_name or f"voc_{args.year}_{args.split}"
    if args.command == "convert":
        (convert_mcg_box if args.mode == "mcg" else convert_ss_box)(records, args.proposals, args.out, name)
        print(f"wrote {args.out}: {len(records)} images")
        return None
    read = {"mcg": lambda: read_mcg_dir(records, args.proposals, name), "ss": lambda: read_ss_mat(args.proposals),
            "eb": lambda: read_eb_mat(args.proposals), "pkl": lambda: read_proposal_pkl(args.proposals)}[args.mode]
    result = proposal_recall(records, read(), name, mode=args.mode,
                             rng=np.random.RandomState(args.seed) if args.mode == "ss" else None)
    print(format_table(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"dataset": name, "mode": args.mode, "budgets": result["budgets"], "thresholds": result["thresholds"],
                       "recall": result["recall"].tolist(), "cnt_yes": result["cnt_yes"].tolist(), "cnt_gt": result["cnt_gt"]}, f)
    return result


if __name__ == "__main__":
    main()

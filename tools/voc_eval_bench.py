"""VOC mAP / CorLoc evaluation at VOC07-test size: a synthetic split of 4,952 images, 20 classes, 1-4 objects per image (10 %
difficult) and --dets detections per image (scores at 3 decimals, coordinates at 1).  Prints one JSON line with

  kernel_ms        ops.voc_eval alone (match + AP kernels, every class at the ten IoU thresholds, both AP metrics and CorLoc) on
                   device-resident inputs (HIP events; median of --reps after a warm-up)
  e2e_s            PascalVOCDetectionEvaluator.evaluate() from the evaluator's lines: annotation XML and image set read, lines
                   parsed, ranked, uploaded, the kernels, one copy back, the means — wall clock
  reference_loop_s the reference's evaluate() loops (evaluation/pascal_voc_evaluation.py: voc_eval and voc_eval_corloc once per
                   class and threshold, restated below in plain Python; parse_rec is cached there, so XML is not counted) on the
                   first --ref-images images, extrapolated linearly to the split.  voc_eval_corloc's `in T or in F` list tests
                   grow with the split, so the linear extrapolation is a lower bound.

    python tools/voc_eval_bench.py [--images 4952] [--dets 100] [--ref-images 200] [--reps 20]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_split(n_img, n_det, seed=0):
    rng = np.random.default_rng(seed)
    names = [f"{i + 1:06d}" for i in range(n_img)]
    objs = []
    for _ in range(n_img):
        o = []
        for _ in range(int(rng.integers(1, 5))):
            x1, y1 = int(rng.integers(1, 400)), int(rng.integers(1, 300))
            o.append((int(rng.integers(0, 20)), [x1, y1, x1 + int(rng.integers(10, 100)), y1 + int(rng.integers(10, 75))],
                      int(rng.random() < 0.1)))
        objs.append(o)
    lines = {k: [] for k in range(20)}
    for i, o in enumerate(objs):
        for _ in range(n_det):
            if rng.random() < 0.5:
                c, b, _ = o[int(rng.integers(0, len(o)))]
                box = [b[q] + rng.integers(-100, 101) / 10 for q in range(4)]
            else:
                c = int(rng.integers(0, 20))
                x, y = rng.integers(0, 4000) / 10, rng.integers(0, 3000) / 10
                box = [x, y, x + rng.integers(50, 1500) / 10, y + rng.integers(50, 1000) / 10]
            lines[c].append(f"{names[i]} {rng.integers(0, 1000) / 1000:.3f} {box[0]:.1f} {box[1]:.1f} {box[2]:.1f} {box[3]:.1f}")
    return names, objs, lines


def write_devkit(root, names, objs, class_names):
    os.makedirs(os.path.join(root, "Annotations"))
    os.makedirs(os.path.join(root, "ImageSets", "Main"))
    for n, o in zip(names, objs):
        with open(os.path.join(root, "Annotations", n + ".xml"), "w") as f:
            f.write("<annotation>" + "".join(
                f"<object><name>{class_names[c]}</name><pose>Unspecified</pose><truncated>0</truncated><difficult>{d}</difficult>"
                f"<bndbox><xmin>{b[0]}</xmin><ymin>{b[1]}</ymin><xmax>{b[2]}</xmax><ymax>{b[3]}</ymax></bndbox></object>"
                for c, b, d in o) + "</annotation>")
    with open(os.path.join(root, "ImageSets", "Main", "test.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))


# ---- the reference's loops (pascal_voc_evaluation.py:295-408, 411-505), file reading replaced by the same lists ----------------

def _ref_class_recs(imagenames, recs, classname):
    class_recs, npos, npos_im = {}, 0, 0
    for imagename in imagenames:
        R = [obj for obj in recs[imagename] if obj["name"] == classname]
        bbox = np.array([x["bbox"] for x in R])
        difficult = np.array([x["difficult"] for x in R]).astype(bool)
        npos = npos + sum(~difficult)
        class_recs[imagename] = {"bbox": bbox, "difficult": difficult, "det": [False] * len(R)}
        if len(R) > 0:
            npos_im += min(1, sum(~difficult))
    return class_recs, npos, npos_im


def _ref_overlap(R, bb):
    BBGT = R["bbox"].astype(float)
    if BBGT.size == 0:
        return -np.inf, 0
    ixmin = np.maximum(BBGT[:, 0], bb[0])
    iymin = np.maximum(BBGT[:, 1], bb[1])
    ixmax = np.minimum(BBGT[:, 2], bb[2])
    iymax = np.minimum(BBGT[:, 3], bb[3])
    iw = np.maximum(ixmax - ixmin + 1.0, 0.0)
    ih = np.maximum(iymax - iymin + 1.0, 0.0)
    inters = iw * ih
    uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (BBGT[:, 2] - BBGT[:, 0] + 1.0) * (BBGT[:, 3] - BBGT[:, 1] + 1.0) - inters
    overlaps = inters / uni
    return np.max(overlaps), np.argmax(overlaps)


def _ref_parse(lines):
    splitlines = [x.strip().split(" ") for x in lines]
    image_ids = [x[0] for x in splitlines]
    confidence = np.array([float(x[1]) for x in splitlines])
    BB = np.array([[float(z) for z in x[2:]] for x in splitlines]).reshape(-1, 4)
    sorted_ind = np.argsort(-confidence, kind="stable")
    return BB[sorted_ind, :], [image_ids[x] for x in sorted_ind]


def ref_voc_eval(lines, imagenames, recs, classname, ovthresh, use_07_metric):
    from sos_wsod_amd.evaluation import RECALL_LEVELS
    class_recs, npos, _ = _ref_class_recs(imagenames, recs, classname)
    BB, image_ids = _ref_parse(lines)
    nd = len(image_ids)
    tp, fp = np.zeros(nd), np.zeros(nd)
    for d in range(nd):
        R = class_recs[image_ids[d]]
        ovmax, jmax = _ref_overlap(R, BB[d, :].astype(float))
        if ovmax > ovthresh:
            if not R["difficult"][jmax]:
                if not R["det"][jmax]:
                    tp[d] = 1.0
                    R["det"][jmax] = 1
                else:
                    fp[d] = 1.0
        else:
            fp[d] = 1.0
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    if use_07_metric:
        ap = 0.0
        for t in RECALL_LEVELS:
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def ref_voc_eval_corloc(lines, imagenames, recs, classname, ovthresh):
    class_recs, _, npos_im = _ref_class_recs(imagenames, recs, classname)
    if len(lines) == 0:
        return 0.0
    BB, image_ids = _ref_parse(lines)
    T, F = [], []
    for d in range(len(image_ids)):
        if image_ids[d] in T or image_ids[d] in F:
            continue
        R = class_recs[image_ids[d]]
        if all(R["difficult"]):
            continue
        ovmax, _ = _ref_overlap(R, BB[d, :].astype(float))
        (T if ovmax > ovthresh else F).append(image_ids[d])
    return 1.0 * len(T) / npos_im


def reference_seconds(names, objs, lines, class_names, n_ref):
    keep = set(names[:n_ref])
    recs = {n: [{"name": class_names[c], "bbox": b, "difficult": d} for c, b, d in o] for n, o in zip(names[:n_ref], objs[:n_ref])}
    sub = {k: [x for x in v if x.split(" ", 1)[0] in keep] for k, v in lines.items()}
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        for k, name in enumerate(class_names):
            for th in range(50, 100, 5):
                ref_voc_eval(sub[k], names[:n_ref], recs, name, th / 100.0, True)
            for th in range(50, 100, 5):
                ref_voc_eval_corloc(sub[k], names[:n_ref], recs, name, th / 100.0)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--ref-images", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    import torch
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import evaluation as E
    from sos_wsod_amd import ops
    from sos_wsod_amd.inference import VOCDetectionWriter

    names, objs, lines = synthetic_split(args.images, args.dets)
    out = {"images": args.images, "detections": sum(len(v) for v in lines.values())}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "VOC2007")
        write_devkit(root, names, objs, E.VOC_CLASS_NAMES)
        gt = E.GroundTruth.load(root, "test")
        dets = E.Detections.from_lines(lines, gt)

        # kernels alone: the same arrays voc_eval_arrays uploads
        K = len(gt.class_names)
        orders = [np.argsort(-s, kind="stable") for _, s, _ in dets.per_class]
        det_off = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in dets.per_class])]).astype(np.int64)
        det_img = np.concatenate([i[o] for (i, _, _), o in zip(dets.per_class, orders)]).astype(np.int32)
        det_box = np.concatenate([b[o] for (_, _, b), o in zip(dets.per_class, orders)])
        thr = np.array([t / 100.0 for t in E.IOU_THRESHOLDS])
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
               (det_off, det_img, det_box, gt.gt_off, gt.gt_box, gt.gt_diff, gt.npos, gt.npos_im, thr, E.RECALL_LEVELS)]
        ref_out = ops.voc_eval(*dev)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            o = ops.voc_eval(*dev)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
            assert torch.equal(o, ref_out)
        out["kernel_ms"] = round(float(np.median(times)), 3)
        assert K == 20

        if not args.no_e2e:
            ev = E.PascalVOCDetectionEvaluator(root, "test", 2007)
            ev.reset()
            ev._writer = VOCDetectionWriter.from_lines(lines)
            t0 = time.perf_counter()
            res = ev.evaluate()
            out["e2e_s"] = round(time.perf_counter() - t0, 3)
            out["mAP50"] = round(float(res["bbox"]["AP50"]), 4)

    t = reference_seconds(names, objs, lines, E.VOC_CLASS_NAMES, args.ref_images)
    out["reference_subset_s"] = round(t, 3)
    out["reference_subset_images"] = args.ref_images
    out["reference_loop_s"] = round(t * args.images / args.ref_images, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""The VOC evaluation fixtures tests/golden/voc_eval_*.npz (written by tests/golden/make_voc_eval_golden.py): the arrays they hold,
the devkit tree, detection lines and JSON records those arrays stand for, and a float64 NumPy restatement of the reference's
voc_eval / voc_ap / voc_eval_corloc (evaluation/pascal_voc_evaluation.py) in stable tie order, for fuzzing.

A fixture holds, per case: the image ids (`names`, written as %06d), the objects (`obj_off` per image, `obj_cls` (an index into
CLASS_NAMES, -1 for an object of another class), `obj_box` int, `obj_diff`, `obj_trunc`, `obj_pose`) and the detections
(`det_cls`, `det_img` (an index into names), `det_score`, `det_box` f64 — or `det_score_milli` / `det_box_deci` int, the values
times 1000 / 10), and the reference's per-class `ap_07`, `ap_area`, `corloc` [K, 10] (percent; NaN where not run) and its
evaluate() dicts (`dict_2007`, `dict_2012`: AP, AP50, AP75, CL, CL50, CL75; absent where not run)."""
import os

import numpy as np

CLASS_NAMES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
               "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
POSES = ("Unspecified", "Left", "Right", "Frontal", "Rear")
FOREIGN = "unlisted"                             # an object name outside CLASS_NAMES
CASES = ("hand", "random", "noties", "npos0")
SPLIT = "val"
DICT_KEYS = (("bbox", "AP"), ("bbox", "AP50"), ("bbox", "AP75"), ("bbox CorLoc", "CL"), ("bbox CorLoc", "CL50"),
             ("bbox CorLoc", "CL75"))


def load(golden_dir, case):
    with np.load(os.path.join(golden_dir, f"voc_eval_{case}.npz")) as z:
        return dict(z)


def names(z):
    """the image-set lines; det_img indexes the distinct names in first-appearance order"""
    return [f"{i:06d}" for i in z["names"].tolist()]


def recs(z):
    """{name: parse_rec objects} of the distinct images"""
    out = {}
    off = z["obj_off"].tolist()
    for k, n in enumerate(dict.fromkeys(names(z))):
        objs = []
        for o in range(off[k], off[k + 1]):
            c = int(z["obj_cls"][o])
            objs.append({"name": CLASS_NAMES[c] if c >= 0 else FOREIGN, "pose": POSES[int(z["obj_pose"][o])],
                         "truncated": int(z["obj_trunc"][o]), "difficult": int(z["obj_diff"][o]),
                         "bbox": [int(v) for v in z["obj_box"][o]]})
        out[n] = objs
    return out


def _xml(objs):
    parts = ["<annotation>\n"]
    for o in objs:
        b = o["bbox"]
        parts.append(f"\t<object>\n\t\t<name>{o['name']}</name>\n\t\t<pose>{o['pose']}</pose>\n"
                     f"\t\t<truncated>{o['truncated']}</truncated>\n\t\t<difficult>{o['difficult']}</difficult>\n"
                     f"\t\t<bndbox>\n\t\t\t<xmin>{b[0]}</xmin>\n\t\t\t<ymin>{b[1]}</ymin>\n\t\t\t<xmax>{b[2]}</xmax>\n"
                     f"\t\t\t<ymax>{b[3]}</ymax>\n\t\t</bndbox>\n\t</object>\n")
    parts.append("</annotation>\n")
    return "".join(parts)


def write_devkit(z, root):
    """Annotations/{id}.xml and ImageSets/Main/val.txt under root (the split file lists every name, repeats included)"""
    os.makedirs(os.path.join(root, "Annotations"), exist_ok=True)
    os.makedirs(os.path.join(root, "ImageSets", "Main"), exist_ok=True)
    for n, objs in recs(z).items():
        with open(os.path.join(root, "Annotations", n + ".xml"), "w") as f:
            f.write(_xml(objs))
    with open(os.path.join(root, "ImageSets", "Main", SPLIT + ".txt"), "w") as f:
        f.write("".join(n + "\n" for n in names(z)))
    return str(root)


def detections(z):
    """(cls [n], img [n] index into names, score [n] f64, box [n, 4] f64) in line order"""
    if "det_score" in z:
        score, box = z["det_score"], z["det_box"]
    else:
        score = np.array([v / 1000 for v in z["det_score_milli"].tolist()], dtype=np.float64)
        box = np.array([v / 10 for v in z["det_box_deci"].reshape(-1).tolist()], dtype=np.float64).reshape(-1, 4)
    return z["det_cls"].astype(np.int64), z["det_img"].astype(np.int64), score, box


def line(name, score, box):
    """the reference evaluator's line for a detection whose box already carries the +1 shift"""
    return f"{name} {score:.3f} {box[0]:.1f} {box[1]:.1f} {box[2]:.1f} {box[3]:.1f}"


def lines(z):
    """{class index: [line]} as PascalVOCDetectionEvaluator.process makes them"""
    nm = names(z)
    cls, img, score, box = detections(z)
    out = {k: [] for k in range(len(CLASS_NAMES))}
    for c, i, s, b in zip(cls.tolist(), img.tolist(), score.tolist(), box.tolist()):
        out[c].append(line(nm[i], s, b))
    return out


def records(z):
    """VOCDetectionWriter.records() of the lines: grouped by class, line order within a class"""
    nm = names(z)
    cls, img, score, box = detections(z)
    out = []
    for k in range(len(CLASS_NAMES)):
        for i in np.flatnonzero(cls == k).tolist():
            out.append({"image_id": int(nm[img[i]]), "category_id": k + 1, "score": float(score[i]),
                        "bbox": [float(v) for v in box[i]]})
    return out


def result_dict(z, year):
    key = f"dict_{year}"
    if key not in z:
        return None
    v = z[key].tolist()
    return {"bbox": {"AP": v[0], "AP50": v[1], "AP75": v[2]}, "bbox CorLoc": {"CL": v[3], "CL50": v[4], "CL75": v[5]}}


# ---- float64 NumPy restatement of the reference (stable tie order) -----------------------------------------------------------

def _overlaps(BBGT, bb):
    ixmin = np.maximum(BBGT[:, 0], bb[0])
    iymin = np.maximum(BBGT[:, 1], bb[1])
    ixmax = np.minimum(BBGT[:, 2], bb[2])
    iymax = np.minimum(BBGT[:, 3], bb[3])
    iw = np.maximum(ixmax - ixmin + 1.0, 0.0)
    ih = np.maximum(iymax - iymin + 1.0, 0.0)
    inters = iw * ih
    uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (BBGT[:, 2] - BBGT[:, 0] + 1.0) * (BBGT[:, 3] - BBGT[:, 1] + 1.0) - inters
    return inters / uni


def voc_ap_terms(rec, prec):
    """the array voc_ap's area metric hands to np.sum: one term per recall change point of the sentinel-extended curve"""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return (mrec[i + 1] - mrec[i]) * mpre[i + 1]


def sequential_sum(terms):
    """the same terms added left to right in f64, which is not the order np.sum takes"""
    s = 0.0
    for v in np.asarray(terms, dtype=np.float64).tolist():
        s += v
    return s


def _pairwise(a, s, n):
    """numpy's pairwise_sum of the Python floats a[s : s + n]: leaves of at most 128 with eight accumulators"""
    if n < 8:
        res = 0.0
        for k in range(s, s + n):
            res += a[k]
        return res
    if n <= 128:
        r = a[s:s + 8]
        i = 8
        while i < n - n % 8:
            for k in range(8):
                r[k] += a[s + i + k]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for k in range(s + i, s + n):
            res += a[k]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a, s, n2) + _pairwise(a, s + n2, n - n2)


def pairwise_sum(terms, chunk=8192):
    """np.sum of a contiguous f64 array spelled out: the identity, then one pairwise sum per `chunk` elements (the ufunc buffer);
    chunk=None is one pairwise block over the whole array, which np.sum does not do beyond 8192 elements"""
    a = np.asarray(terms, dtype=np.float64).tolist()
    res = 0.0
    step = len(a) if chunk is None else chunk
    for s in range(0, len(a), max(step, 1)):
        res += _pairwise(a, s, min(step, len(a) - s))
    return res


VARIANTS = ("ge", "last_max", "reversed_ties", "sequential_sum")    # deliberately wrong restatements, for sensitivity tests


def voc_ap(rec, prec, use_07_metric):
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.0
        return ap
    return np.sum(voc_ap_terms(rec, prec))


def restated(objs_by_img, n_img, dets_by_class, K, corloc=True, variant=None):
    """objs_by_img: [n_img] lists of (class, box [4] int, difficult); every image once in the split.  dets_by_class: [K] of
    (img [n], score [n], box [n, 4]) in line order.  -> (ap_07, ap_area, corloc) [K, 10] in percent (corloc None if not asked).
    variant: one of VARIANTS, a restatement that is wrong on purpose in that one rule."""
    return restated_detail(objs_by_img, n_img, dets_by_class, K, corloc, variant)[:3]


def restated_detail(objs_by_img, n_img, dets_by_class, K, corloc=True, variant=None):
    """restated() and what it went through, per class: -> (ap_07, ap_area, corloc, detail) with detail[c] = {"order" [nd] (line
    index of each rank), "img" [nd], "ovmax" [nd], "jmax" [nd] (within the image's objects of the class), "tp" / "fp" [10, nd]
    flags in rank order, "terms" [10] (the arrays voc_ap sums), "holder" {image: rank of the detection CorLoc reads}}"""
    assert variant is None or variant in VARIANTS, variant
    above = (lambda o, thr: o >= thr) if variant == "ge" else (lambda o, thr: o > thr)
    total = sequential_sum if variant == "sequential_sum" else np.sum
    detail = []
    with np.errstate(all="ignore"):
        out = np.full((3, K, 10), np.nan)
        for c in range(K):
            gtb = [np.array([o[1] for o in objs_by_img[i] if o[0] == c], dtype=np.float64).reshape(-1, 4) for i in range(n_img)]
            dif = [np.array([bool(o[2]) for o in objs_by_img[i] if o[0] == c], dtype=bool) for i in range(n_img)]
            npos = sum(int((~d).sum()) for d in dif)
            npos_im = sum(1 for d in dif if len(d) and (~d).any())
            img, score, box = dets_by_class[c]
            score = np.asarray(score, dtype=np.float64)
            if variant == "reversed_ties":
                order = np.lexsort((-np.arange(len(score)), -score))
            else:
                order = np.argsort(-score, kind="stable")
            img, box = np.asarray(img)[order], np.asarray(box, dtype=np.float64).reshape(-1, 4)[order]
            nd = len(img)
            ov, jm = np.full(nd, -np.inf), np.zeros(nd, dtype=np.int64)
            for d in range(nd):
                if gtb[img[d]].size:
                    o = _overlaps(gtb[img[d]], box[d])
                    ov[d], jm[d] = np.max(o), (len(o) - 1 - np.argmax(o[::-1])) if variant == "last_max" else np.argmax(o)
            det = {"order": order, "img": img, "ovmax": ov, "jmax": jm, "tp": np.zeros((10, nd)), "fp": np.zeros((10, nd)),
                   "terms": [], "holder": {}}
            detail.append(det)
            for t, th in enumerate(range(50, 100, 5)):
                thr = th / 100.0
                tp, fp = det["tp"][t], det["fp"][t]
                claimed = [np.zeros(len(d), dtype=bool) for d in dif]
                for d in range(nd):
                    if above(ov[d], thr):
                        if not dif[img[d]][jm[d]]:
                            if not claimed[img[d]][jm[d]]:
                                tp[d] = 1.0
                                claimed[img[d]][jm[d]] = True
                            else:
                                fp[d] = 1.0
                    else:
                        fp[d] = 1.0
                fp, tp = np.cumsum(fp), np.cumsum(tp)
                rec = tp / float(npos)
                prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
                out[0, c, t] = voc_ap(rec, prec, True) * 100
                det["terms"].append(voc_ap_terms(rec, prec))
                out[1, c, t] = total(det["terms"][-1]) * 100              # voc_ap(rec, prec, False)
                if corloc:
                    if nd == 0:
                        out[2, c, t] = 0.0 * 100
                        continue
                    seen, hits = set(), 0
                    for d in range(nd):
                        if img[d] in seen or not (~dif[img[d]]).any():
                            continue
                        seen.add(img[d])
                        det["holder"][int(img[d])] = d
                        hits += above(ov[d], thr)
                    out[2, c, t] = 1.0 * hits / npos_im * 100
    return out[0], out[1], (out[2] if corloc else None), detail

"""COCO evaluation fixtures (tests/golden/coco_eval_*.npz, made by tests/golden/make_coco_eval_golden.py from the reference's
cocoeval.cpp): loaders, builders of the annotation / result JSON, and a float64 NumPy restatement of the whole path
(pycocotools' _prepare, loadRes, computeIoU -> maskApi.c bbIou; cocoeval.cpp EvaluateImages and Accumulate; summarize;
COCOEvaluator._derive_coco_results) that the GPU fuzz compares against."""
import binascii
import hashlib
import os

import numpy as np

CASES = ("hand", "random", "coco")
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]


def load(golden_dir, case):
    return dict(np.load(os.path.join(golden_dir, f"coco_eval_{case}.npz")))


def dataset(z):
    """the annotation file's dict of a fixture"""
    names = [str(n) for n in z["cat_names"]]
    anns = []
    box = z["ann_box"] if "ann_box" in z else z["ann_box_deci"] / 10.0
    area = z["ann_area"] if "ann_area" in z else z["ann_area_centi"] / 100.0
    for k in range(len(z["ann_id"])):
        anns.append({"id": int(z["ann_id"][k]), "image_id": int(z["ann_img"][k]), "category_id": int(z["ann_cat"][k]),
                     "bbox": [float(v) for v in box[k]], "area": float(area[k]), "iscrowd": int(z["ann_crowd"][k])})
    return {"images": [{"id": int(i), "height": 480, "width": 640, "file_name": f"{int(i):012d}.jpg"} for i in z["img_ids"]],
            "categories": [{"id": int(c), "name": n} for c, n in zip(z["cat_ids"], names)], "annotations": anns}


def results(z):
    """the result list (coco_instances_results.json) of a fixture"""
    box = z["det_box"] if "det_box" in z else z["det_box_deci"] / 10.0
    score = z["det_score"] if "det_score" in z else z["det_score_milli"] / 1000.0
    return [{"image_id": int(z["det_img"][k]), "category_id": int(z["det_cat"][k]), "bbox": [float(v) for v in box[k]],
             "score": float(score[k])} for k in range(len(z["det_img"]))]


def pack(ds, res, compact):
    """the inverse of dataset() / results(): the arrays a fixture stores"""
    z = {"img_ids": np.asarray([im["id"] for im in ds["images"]], dtype=np.int32),
         "cat_ids": np.asarray([c["id"] for c in ds["categories"]], dtype=np.int32),
         "cat_names": np.asarray([c["name"] for c in ds["categories"]]),
         "ann_id": np.asarray([a["id"] for a in ds["annotations"]], dtype=np.int32),
         "ann_img": np.asarray([a["image_id"] for a in ds["annotations"]], dtype=np.int32),
         "ann_cat": np.asarray([a["category_id"] for a in ds["annotations"]], dtype=np.int32),
         "ann_crowd": np.asarray([a["iscrowd"] for a in ds["annotations"]], dtype=np.uint8),
         "det_img": np.asarray([r["image_id"] for r in res], dtype=np.int32),
         "det_cat": np.asarray([r["category_id"] for r in res], dtype=np.int32)}
    ab = np.asarray([a["bbox"] for a in ds["annotations"]], dtype=np.float64).reshape(-1, 4)
    aa = np.asarray([a["area"] for a in ds["annotations"]], dtype=np.float64)
    db = np.asarray([r["bbox"] for r in res], dtype=np.float64).reshape(-1, 4)
    sc = np.asarray([r["score"] for r in res], dtype=np.float64)
    if compact:
        z["ann_box_deci"] = np.round(ab * 10).astype(np.int32)
        z["ann_area_centi"] = np.round(aa * 100).astype(np.int64)
        z["det_box_deci"] = np.round(db * 10).astype(np.int32)
        z["det_score_milli"] = np.round(sc * 1000).astype(np.int16)
        assert np.array_equal(z["ann_box_deci"] / 10.0, ab) and np.array_equal(z["ann_area_centi"] / 100.0, aa)
        assert np.array_equal(z["det_box_deci"] / 10.0, db) and np.array_equal(z["det_score_milli"] / 1000.0, sc)
    else:
        z.update(ann_box=ab, ann_area=aa, det_box=db, det_score=sc)
    return z


def digest(a):
    """what a fixture stores of an array too large to commit: SHA-256 of its bytes and a CRC-32 per category slice [:, :, k]"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    crc = np.asarray([binascii.crc32(np.ascontiguousarray(a[:, :, k]).tobytes()) for k in range(a.shape[2])], dtype=np.uint32)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy(), crc


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def bb_iou(d, g, crowd):
    """maskApi.c bbIou for one detection and one ground truth, boxes [x, y, w, h] (Python floats are IEEE f64)"""
    da, ga = d[2] * d[3], g[2] * g[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def prepare(ds, res, img_ids=None):
    """COCO(ds), loadRes(res) and COCOeval._prepare: (imgIds, catIds, {(img, cat): [gt]}, {(img, cat): [dt]}); raises ValueError
    where loadRes asserts"""
    all_imgs = sorted({im["id"] for im in ds["images"]})
    img_list = all_imgs if img_ids is None else sorted(set(img_ids))
    cat_list = sorted({c["id"] for c in ds["categories"]})
    if not set(r["image_id"] for r in res) <= set(all_imgs):
        raise ValueError("Results do not correspond to current coco set")
    gts = {(i, c): [] for i in img_list for c in cat_list}
    dts = {(i, c): [] for i in img_list for c in cat_list}
    for a in ds["annotations"]:
        if (a["image_id"], a["category_id"]) in gts:
            g = dict(a)
            g["ignore"] = "iscrowd" in g and g["iscrowd"]
            gts[a["image_id"], a["category_id"]].append(g)
    for k, r in enumerate(res):
        if (r["image_id"], r["category_id"]) in dts:
            bb = r["bbox"]
            dts[r["image_id"], r["category_id"]].append(dict(r, area=bb[2] * bb[3], id=k + 1, iscrowd=0))
    return img_list, cat_list, gts, dts


def compute_iou(gt, dt):
    """COCOeval.computeIoU for boxes: rows are the detections in stable descending score order, cut at maxDets[-1]"""
    if len(gt) == 0 or len(dt) == 0:
        return []
    inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in inds][:MAX_DETS[-1]]
    return [[bb_iou(d["bbox"], g["bbox"], bool(g["iscrowd"])) for g in gt] for d in dt]


VARIANTS = ("gt_walk", "no_break", "closed_area", "crowd_once")   # deliberately wrong restatements, for sensitivity tests


def evaluate_pair(gt, dt, ious, area_range, variant=None):
    """cocoeval.cpp: SortInstancesByDetectionScore, SortInstancesByIgnore, MatchDetectionsToGroundTruth for one area range
    -> (detection_matches [T][D] ids, detection_ignores [T][D], detection_scores [D], ground_truth_ignores [G]).
    variant: one of VARIANTS, a restatement that is wrong on purpose in that one rule."""
    assert variant is None or variant in VARIANTS, variant
    if variant == "closed_area":
        def outside(area):
            return area <= area_range[0] or area >= area_range[1]
    else:
        def outside(area):
            return area < area_range[0] or area > area_range[1]
    dind = sorted(range(len(dt)), key=lambda j: -dt[j]["score"])[:MAX_DETS[-1]]          # sorted() is stable
    ignores = [bool(g["ignore"]) or outside(g["area"]) for g in gt]
    gind = sorted(range(len(gt)), key=lambda j: int(ignores[j]))
    gt_ign = [ignores[j] for j in gind]
    T, D, G = len(IOU_THRS), len(dind), len(gind)
    gtm = [[0] * G for _ in range(T)]
    dtm = [[0] * D for _ in range(T)]
    dtig = [[False] * D for _ in range(T)]
    for t in range(T):
        for d in range(D):
            best = min(float(IOU_THRS[t]), 1 - 1e-10)
            m = -1
            for g in range(G):
                if gtm[t][g] > 0 and (variant == "crowd_once" or not gt[gind[g]]["iscrowd"]):
                    continue
                if m >= 0 and not gt_ign[m] and gt_ign[g] and variant != "no_break":
                    break
                o = ious[d][gind[g]]
                if (o > best) if variant == "gt_walk" else (o >= best):
                    best = o
                    m = g
            if m >= 0:
                dtig[t][d] = gt_ign[m]
                dtm[t][d] = gt[gind[m]]["id"]
                gtm[t][m] = dt[dind[d]]["id"]
            det = dt[dind[d]]
            dtig[t][d] = dtig[t][d] or (dtm[t][d] == 0 and outside(det["area"]))
    return dtm, dtig, [dt[j]["score"] for j in dind], gt_ign


def _pair_record(dt, ev):
    dind = sorted(range(len(dt)), key=lambda j: -dt[j]["score"])[:MAX_DETS[-1]]
    return {"ids": [dt[j]["id"] for j in dind], "matched": np.asarray([e[0] for e in ev], dtype=np.int64) > 0,
            "ignored": np.asarray([e[1] for e in ev], dtype=bool), "gt_ignored": [e[3] for e in ev]}


def pair_matches(ds, res, img_ids=None, variant=None):
    """what evaluate_pair decides for every (image, category) that has detections: {(image id, category id): {"ids" [D] (the
    detections' loadRes ids, 1-based positions in res, in the pair's score order cut at 100), "matched" / "ignored" bool
    [A, T, D] (detection_matches > 0, detection_ignores), "gt_ignored" [A][G] in the partition's order}}; restated(pairs={})
    fills the same dict on its way"""
    pairs = {}
    restated(ds, res, img_ids, variant, pairs, accumulate=False)
    return pairs


def restated(ds, res, img_ids=None, variant=None, pairs=None, accumulate=True):
    """-> {"precision" [T, R, K, A, M], "recall" [T, K, A, M], "scores" [T, R, K, A, M], "counts"}; pairs: a dict that receives
    pair_matches()'s records"""
    img_list, cat_list, gts, dts = prepare(ds, res, img_ids)
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_list), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, c in enumerate(cat_list):
        evals = [[None] * len(img_list) for _ in range(A)]
        for n, i in enumerate(img_list):
            gt, dt = gts[i, c], dts[i, c]
            ious = compute_iou(gt, dt)
            for a in range(A):
                evals[a][n] = evaluate_pair(gt, dt, ious, AREA_RNG[a], variant)
            if pairs is not None and dt:
                pairs[i, c] = _pair_record(dt, [evals[a][n] for a in range(A)])
        if not accumulate:
            continue
        for a in range(A):
            npig = sum(1 for e in evals[a] for ig in e[3] if not ig)
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                sc = np.asarray([s for e in evals[a] for s in e[2][:max_det]], dtype=np.float64)
                order = np.argsort(-sc, kind="stable")
                for t in range(T):
                    match = np.asarray([v for e in evals[a] for v in e[0][t][:max_det]], dtype=np.int64)[order]
                    ign = np.asarray([v for e in evals[a] for v in e[1][t][:max_det]], dtype=bool)[order]
                    tp = np.cumsum((match > 0) & ~ign, dtype=np.int64)
                    fp = np.cumsum((match == 0) & ~ign, dtype=np.int64)
                    rc = tp / npig
                    with np.errstate(invalid="ignore", divide="ignore"):
                        pr = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
                    recall[t, k, a, m] = rc[-1] if len(rc) else 0
                    if len(pr):
                        pr = np.maximum.accumulate(pr[::-1])[::-1]
                    inds = np.searchsorted(rc, REC_THRS, side="left")
                    ok = inds < len(pr)
                    q, s = np.zeros(R), np.zeros(R)
                    q[ok] = pr[inds[ok]]
                    s[ok] = sc[order][inds[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = s
    return {"precision": precision, "recall": recall, "scores": scores, "counts": [T, R, K, A, M]}


def summarize(ev):
    """COCOeval.summarize -> stats [12]"""
    def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
        aind = [i for i, aRng in enumerate(AREA_LBL) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(MAX_DETS) if mDet == maxDets]
        if ap == 1:
            s = ev["precision"]
            if iouThr is not None:
                t = np.where(iouThr == IOU_THRS)[0]
                s = s[t]
            s = s[:, :, :, aind, mind]
        else:
            s = ev["recall"]
            if iouThr is not None:
                t = np.where(iouThr == IOU_THRS)[0]
                s = s[t]
            s = s[:, :, aind, mind]
        if len(s[s > -1]) == 0:
            return -1
        return np.mean(s[s > -1])

    stats = np.zeros((12,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5, maxDets=MAX_DETS[2])
    stats[2] = _summarize(1, iouThr=.75, maxDets=MAX_DETS[2])
    stats[3] = _summarize(1, areaRng="small", maxDets=MAX_DETS[2])
    stats[4] = _summarize(1, areaRng="medium", maxDets=MAX_DETS[2])
    stats[5] = _summarize(1, areaRng="large", maxDets=MAX_DETS[2])
    stats[6] = _summarize(0, maxDets=MAX_DETS[0])
    stats[7] = _summarize(0, maxDets=MAX_DETS[1])
    stats[8] = _summarize(0, maxDets=MAX_DETS[2])
    stats[9] = _summarize(0, areaRng="small", maxDets=MAX_DETS[2])
    stats[10] = _summarize(0, areaRng="medium", maxDets=MAX_DETS[2])
    stats[11] = _summarize(0, areaRng="large", maxDets=MAX_DETS[2])
    return stats


def derive(ev, stats, class_names):
    """COCOEvaluator._derive_coco_results for bbox -> {metric: value}"""
    out = {metric: float(stats[idx] * 100 if stats[idx] >= 0 else "nan") for idx, metric in enumerate(METRICS)}
    if class_names is None or len(class_names) <= 1:
        return out
    for idx, name in enumerate(class_names):
        precision = ev["precision"][:, :, idx, 0, -1]
        precision = precision[precision > -1]
        ap = np.mean(precision) if precision.size else float("nan")
        out["AP-" + name] = float(ap * 100)
    return out


def expected_results(z):
    """the result dict a fixture stores: {metric: value}, per-class entries included"""
    names = [str(n) for n in z["cat_names"]]
    order = np.argsort(z["cat_ids"], kind="stable")
    keys = METRICS + ["AP-" + names[k] for k in order]
    return dict(zip(keys, (float(v) for v in z["result_values"])))


# ---- synthetic splits ---------------------------------------------------------------------------------------------------------

def random_split(rng, n_img, K, max_det, crowd_p=0.08, max_obj=6, one_class=False, no_gt=False, score_steps=1000):
    """boxes on a 0.1 grid over small / medium / large sizes, scores at 3 decimals, category ids with gaps, image ids unsorted"""
    cat_ids = sorted(rng.choice(np.arange(1, 3 * K + 2), K, replace=False).tolist())
    img_ids = rng.choice(np.arange(1, 20 * n_img + 2), n_img, replace=False).tolist()
    ds = {"images": [{"id": int(i), "height": 480, "width": 640, "file_name": f"{int(i):012d}.jpg"} for i in img_ids],
          "categories": [{"id": int(c), "name": f"c{c}"} for c in cat_ids], "annotations": []}
    res = []
    sizes = (8, 24, 60, 150, 320)
    for i in img_ids:
        objs = []
        for _ in range(0 if no_gt else int(rng.integers(0, max_obj + 1))):
            c = cat_ids[0] if one_class else cat_ids[int(rng.integers(0, K))]
            s = sizes[int(rng.integers(0, len(sizes)))]
            w, h = int(rng.integers(s // 2, 2 * s) * 10) / 10, int(rng.integers(s // 2, 2 * s) * 10) / 10
            x, y = int(rng.integers(0, 5000)) / 10, int(rng.integers(0, 4000)) / 10
            crowd = int(rng.random() < crowd_p)
            area = round(w * h * float(rng.uniform(0.4, 1.0)), 2)
            objs.append((c, [x, y, w, h]))
            ds["annotations"].append({"id": len(ds["annotations"]) + 1, "image_id": int(i), "category_id": int(c),
                                      "bbox": [x, y, w, h], "area": area, "iscrowd": crowd})
        for _ in range(int(rng.integers(0, max_det + 1))):
            if objs and rng.random() < 0.65:
                c, b = objs[int(rng.integers(0, len(objs)))]
                b = [max(0.0, b[0] + int(rng.integers(-b[2] * 2, b[2] * 2 + 1)) / 10), max(0.0, b[1] + int(rng.integers(-b[3] * 2, b[3] * 2 + 1)) / 10),
                     max(0.0, b[2] + int(rng.integers(-b[2] * 2, b[2] * 2 + 1)) / 10), max(0.0, b[3] + int(rng.integers(-b[3] * 2, b[3] * 2 + 1)) / 10)]
                b = [round(v * 10) / 10 for v in b]
            else:
                c = cat_ids[0] if one_class else cat_ids[int(rng.integers(0, K))]
                s = sizes[int(rng.integers(0, len(sizes)))]
                b = [int(rng.integers(0, 5000)) / 10, int(rng.integers(0, 4000)) / 10, int(rng.integers(s // 2, 2 * s) * 10) / 10,
                     int(rng.integers(s // 2, 2 * s) * 10) / 10]
            res.append({"image_id": int(i), "category_id": int(c), "bbox": b,
                        "score": round(int(rng.integers(0, score_steps)) / score_steps, 3)})
    return ds, res

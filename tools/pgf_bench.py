"""Stage-2 pseudo-label filtering (PGF) at COCO scale: a synthetic split of 117,266 images (train2014 + valminusminival) x 100
detections, 80 classes, 1-3 ground-truth classes per image.  Prints one JSON line with

  kernel_ms        sw_pgf_keep alone on device-resident inputs (HIP events; median of --reps after a warm-up)
  e2e_s            the whole split through sos_wsod_amd.pseudo_labels: json.load of the detections and ground truth, pgf_coco
                   (grouping, upload, kernel, one copy back), COCO annotations, json.dump — wall clock
  reference_loop_s the reference's class_filter + pgf loops (tools/pgf.py:221-292, restated below in plain Python, deepcopy in
                   contain_cal included) on the first --ref-images images, extrapolated linearly to the split

    python tools/pgf_bench.py [--images 117266] [--dets 100] [--ref-images 1000] [--no-e2e]
"""
import argparse
import copy
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
    n_gt = rng.integers(1, 4, n_img)
    gt = [rng.choice(80, k, replace=False) for k in n_gt]
    own = rng.random((n_img, n_det)) < 0.7
    cls = np.where(own, np.stack([g[rng.integers(0, len(g), n_det)] for g in gt]), rng.integers(0, 80, (n_img, n_det)))
    xy = rng.uniform(0, 500, (n_img, n_det, 2)).round(2)
    wh = rng.uniform(1, 200, (n_img, n_det, 2)).round(2)
    boxes = np.concatenate([xy, wh], axis=2)
    scores = rng.random((n_img, n_det)).round(4)
    return gt, cls.astype(np.int32), boxes, scores


def as_records(gt, cls, boxes, scores, n_img):
    dets, dicts = [], []
    for i in range(n_img):
        b, c, s = boxes[i].tolist(), cls[i].tolist(), scores[i].tolist()
        dets.append({"image_id": i, "instances": [{"image_id": i, "category_id": c[k], "bbox": b[k], "score": s[k]}
                                                  for k in range(len(c))]})
        dicts.append({"image_id": i, "annotations": [{"category_id": int(g)} for g in gt[i]]})
    return dets, dicts


# ---- plain-Python restatement of the reference's loops (what the kernel replaces) -------------------------------------------
def _contain(a_, b_):
    a, b = copy.deepcopy(a_), copy.deepcopy(b_)
    a[2] += a[0]; a[3] += a[1]; b[2] += b[0]; b[3] += b[1]
    c = [max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])]
    return max(0, c[2] - c[0]) * max(0, c[3] - c[1]) / (max(0, a[2] - a[0]) * max(0, a[3] - a[1]) + 1e-6)


def reference_loop(result, class_dict, t_con=0.85, t_keep=0.2):
    for img, preds in result.items():
        result[img] = [p for p in preds if p["category_id"] in class_dict[img]]
    for img, preds in result.items():
        seen, kept = [], []
        for p in preds:
            if p["category_id"] not in seen:
                seen.append(p["category_id"]); kept.append(p)
            elif not p["score"] < t_keep:
                kept.append(p)
        result[img] = kept
    for img, anns in result.items():
        save = [True] * len(anns)
        for i in range(len(anns)):
            for j in range(len(anns)):
                if i == j or anns[i]["category_id"] != anns[j]["category_id"]:
                    continue
                if _contain(anns[i]["bbox"], anns[j]["bbox"]) >= t_con:
                    save[i] = False
        result[img] = [copy.deepcopy(a) for a, s in zip(anns, save) if s]
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=117266)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--ref-images", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()

    import torch
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import ops
    from sos_wsod_amd import pseudo_labels as P
    assert torch.cuda.is_available(), "pgf_bench needs the GPU"
    n_img, n_det = args.images, args.dets
    gt, cls, boxes, scores = synthetic_split(n_img, n_det)
    out = {"images": n_img, "detections": n_img * n_det}

    # kernel alone
    gt_mask = np.zeros((n_img, 3), dtype=np.uint32)
    for i, g in enumerate(gt):
        for c in g:
            gt_mask[i, c >> 5] |= np.uint32(1 << (int(c) & 31))
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    off = up(np.arange(n_img + 1, dtype=np.int64) * n_det)
    args_dev = (off, up(boxes.reshape(-1, 4)), up(scores.reshape(-1)), up(cls.reshape(-1)), 80, up(gt_mask.view(np.int32)),
                up(np.zeros(3, dtype=np.int32)), 0.2, 0.85, True)
    packed = ops.pgf_keep(*args_dev)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.pgf_keep(*args_dev)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    out["kernel_ms"] = round(float(np.median(times)), 3)
    out["kernel_ms_min"] = round(float(np.min(times)), 3)
    counts = packed[:32].cpu().numpy().view(np.int64).tolist()
    out["counts"] = counts

    # the reference loop on a subset, extrapolated
    m = min(args.ref_images, n_img)
    dets, dicts = as_records(gt, cls, boxes, scores, m)
    result = {d["image_id"]: list(d["instances"]) for d in dets}
    class_dict = P.gt_classes(dicts)
    t = time.perf_counter()
    ref = reference_loop(result, class_dict)
    dt = time.perf_counter() - t
    out["reference_loop_subset_images"] = m
    out["reference_loop_subset_s"] = round(dt, 3)
    out["reference_loop_s"] = round(dt * n_img / m, 1)
    mine, _ = P.pgf_coco(json.loads(json.dumps(dets)), dicts)
    out["subset_matches_reference_loop"] = json.dumps(mine) == json.dumps(ref)

    if not args.no_e2e:
        with tempfile.TemporaryDirectory() as tmp:
            dets, dicts = as_records(gt, cls, boxes, scores, n_img)
            with open(f"{tmp}/det.json", "w") as f:
                json.dump(dets, f)
            with open(f"{tmp}/gt.json", "w") as f:
                json.dump(dicts, f)
            del dets, dicts
            t = time.perf_counter()
            with open(f"{tmp}/det.json") as f:
                dets = json.load(f)
            with open(f"{tmp}/gt.json") as f:
                dicts = json.load(f)
            t_load = time.perf_counter()
            result, stats = P.pgf_coco(dets, dicts)
            t_pgf = time.perf_counter()
            P.write_json(P.coco_pseudo_labels({"images": [], "categories": []}, result), f"{tmp}/out.json")
            t_end = time.perf_counter()
            out["e2e_s"] = round(t_end - t, 2)
            out["e2e_load_s"] = round(t_load - t, 2)
            out["e2e_pgf_s"] = round(t_pgf - t_load, 2)
            out["e2e_write_s"] = round(t_end - t_pgf, 2)
            out["e2e_stats"] = stats
    print(json.dumps(out))


if __name__ == "__main__":
    main()

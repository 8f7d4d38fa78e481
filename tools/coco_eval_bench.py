"""COCO bbox evaluation at minival size: a synthetic split of 5,000 images, 80 categories, 1-15 objects per image (3 % crowd) and
--dets detections per image (scores at 3 decimals, coordinates at 1).  Prints one JSON line with

  kernel_ms          ops.coco_eval alone (coco_match_kernel + coco_accum_kernel: every (image, category) pair at 4 area ranges x 10
                     thresholds, then the 80 x 4 x 3 x 10 precision / recall curves) on device-resident inputs (HIP events; median
                     of --reps after a warm-up).  For the split between the two kernels run it under
                     `rocprofv3 --kernel-trace --stats -- python tools/coco_eval_bench.py --kernels-only`.
  e2e_s              COCOEvaluator.evaluate() from the per-image records: the annotation JSON read, the records flattened and
                     mapped to dataset ids, grouped and sorted, uploaded, the kernels, one copy back, summarize — wall clock
  restatement_s      the float64 NumPy restatement of COCOeval_opt (tests/coco_eval_fixture.restated: the reference's loops in
                     Python) on the first --ref-images images, EXTRAPOLATED linearly to the split (labelled so: it is a Python
                     comparator, not the reference's C++)

    python tools/coco_eval_bench.py [--images 5000] [--dets 100] [--ref-images 250] [--reps 20] [--kernels-only]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic_split(n_img, n_det, K=80, seed=0):
    rng = np.random.default_rng(seed)
    cat_ids = sorted(rng.choice(np.arange(1, 91), K, replace=False).tolist())
    ds = {"images": [{"id": i + 1, "height": 480, "width": 640, "file_name": f"{i + 1:012d}.jpg"} for i in range(n_img)],
          "categories": [{"id": int(c), "name": f"c{c}"} for c in cat_ids], "annotations": []}
    preds = []
    for i in range(n_img):
        n_obj = int(rng.integers(1, 16))
        oc = rng.choice(K, size=max(1, n_obj // 3))[rng.integers(0, max(1, n_obj // 3), n_obj)]   # a few classes per image
        ob = np.stack([rng.integers(0, 5000, n_obj), rng.integers(0, 4000, n_obj), rng.integers(50, 3000, n_obj),
                       rng.integers(50, 2500, n_obj)], 1) / 10
        for c, b in zip(oc, ob):
            ds["annotations"].append({"id": len(ds["annotations"]) + 1, "image_id": i + 1, "category_id": cat_ids[int(c)],
                                      "bbox": b.tolist(), "area": round(float(b[2] * b[3]) * 0.7, 2),
                                      "iscrowd": int(rng.random() < 0.03)})
        near = rng.random(n_det) < 0.6
        pick = rng.integers(0, n_obj, n_det)
        cls = np.where(near, oc[pick], rng.integers(0, K, n_det))
        box = np.where(near[:, None], ob[pick] + rng.integers(-150, 151, (n_det, 4)) / 10,
                       np.stack([rng.integers(0, 5000, n_det), rng.integers(0, 4000, n_det), rng.integers(50, 3000, n_det),
                                 rng.integers(50, 2500, n_det)], 1) / 10)
        box = np.round(np.maximum(box, 0.0) * 10) / 10
        score = rng.integers(0, 1000, n_det) / 1000
        preds.append({"image_id": i + 1, "instances": [
            {"image_id": i + 1, "category_id": int(c), "bbox": b, "score": float(s)} for c, b, s in zip(cls, box.tolist(), score)]})
    return ds, preds, cat_ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--ref-images", type=int, default=250)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    import torch
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import evaluation as E
    from sos_wsod_amd import ops
    import coco_eval_fixture as F

    ds, preds, cat_ids = synthetic_split(args.images, args.dets)
    results = [dict(r, category_id=cat_ids[r["category_id"]]) for p in preds for r in p["instances"]]
    out = {"images": args.images, "detections": len(results), "annotations": len(ds["annotations"])}
    gt = E.COCOGroundTruth(ds)
    L = E.coco_eval_layout(gt, E.COCODetections.from_results(results, gt))
    D, G = np.diff(L["pair_off"]), L["gt_off"][L["pair_gt"] + 1] - L["gt_off"][L["pair_gt"]]
    out.update(pairs=int(len(D)), pairs_with_gt=int((G > 0).sum()), workspace_pairs=int((L["pair_ws"] >= 0).sum()),
               mean_dets_per_pair=round(float(D.mean()), 2), max_gt_per_pair=int(G.max()))

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)

    i64, f64 = torch.int64, torch.float64
    a = (dev(L["pair_off"], i64), dev(L["pair_gt"], i64), dev(L["pair_ws"], i64), L["ws_words"], dev(L["det_box"], f64),
         dev(L["gt_off"], i64), dev(L["gt_box"], f64), dev(L["gt_area"], f64), dev(L["gt_flags"], torch.uint8),
         dev(np.asarray(E.COCO_AREA_RNG, dtype=np.float64), f64), dev(E.COCO_IOU_THRS, f64), dev(E.COCO_REC_THRS, f64),
         dev(np.asarray(E.COCO_MAX_DETS), torch.int32), dev(L["cat_off"], i64), dev(L["order"], torch.int32),
         dev(L["det_rank"], torch.uint8), dev(L["det_score"], f64), dev(L["npig"], i64))
    ref_out, _ = ops.coco_eval(*a)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o, _ = ops.coco_eval(*a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        assert torch.equal(o, ref_out)
    out["kernel_ms"] = round(float(np.median(times)), 3)
    if args.kernels_only:
        print(json.dumps(out))
        return

    with tempfile.TemporaryDirectory() as tmp:
        ann = os.path.join(tmp, "instances_minival.json")
        with open(ann, "w") as f:
            json.dump(ds, f)
        ev = E.COCOEvaluator(ann)
        ev.reset()
        ev.set_predictions(preds)
        t0 = time.perf_counter()
        res = ev.evaluate()
        out["e2e_s"] = round(time.perf_counter() - t0, 3)
        out["AP"], out["AP50"] = round(res["bbox"]["AP"], 4), round(res["bbox"]["AP50"], 4)

    keep = set(range(1, args.ref_images + 1))
    sub_ds = {"images": ds["images"][:args.ref_images], "categories": ds["categories"],
              "annotations": [x for x in ds["annotations"] if x["image_id"] in keep]}
    sub_res = [r for r in results if r["image_id"] in keep]
    t0 = time.perf_counter()
    want = F.restated(sub_ds, sub_res)
    t = time.perf_counter() - t0
    got = E.coco_eval_arrays(gt, E.COCODetections.from_results(results, gt), img_ids=sorted(keep))
    assert all(np.array_equal(got[k], want[k]) for k in ("precision", "recall", "scores")), "GPU and restatement differ"
    out.update(restatement_subset_s=round(t, 2), restatement_subset_images=args.ref_images,
               restatement_s_extrapolated=round(t * args.images / args.ref_images, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

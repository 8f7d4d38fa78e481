"""Box-proposal AR at two sizes: --size minival, a synthetic split of 5,000 images x 1,000 scored proposals with 1-90 ground-truth
boxes per image, at the evaluator's 2 limits x 4 area ranges; --size mcg, 4,952 images x 2,048 proposals with 1-5 boxes per image,
at limits 100 / 1000 / none x 4 ranges (the unlimited items read more proposals than the kernel stages in LDS).  Prints one JSON
line with

  kernel_ms      ops.box_proposal_ar alone (every limit and range in one launch) on device-resident inputs: HIP events, the median
                 of at least --reps launches and at least 0.5 s of them, after a warm-up (the wrapper's offset check is off, as in
                 the module's call)
  e2e_s          box_proposals.box_proposal_metrics() from in-memory records to the numbers: ranking, CSR build, upload, the
                 kernel, the copy back, sorting, recalls — wall clock ending in a synchronise
  host_prep_s    e2e_s minus the kernel: what the host spends around it, and host_share, that as a share of e2e_s
  restated_s     the NumPy restatement (tests/box_proposal_ref.evaluate, once per limit and range, as the reference runs) on the
                 same host over the first --restate-images images (restated_images), whose counts the launch must equal;
                 restated_full_s_est scales it to the whole split by ground-truth boxes

    python tools/box_proposal_ar_bench.py [--size minival|mcg] [--images N] [--props N] [--reps 30] [--restate-images 250]
                                          [--kernel-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"minival": dict(images=5000, props=1000, max_gt=90, limits=(100, 1000)),
         "mcg": dict(images=4952, props=2048, max_gt=5, limits=(100, 1000, None))}
AREAS = ("all", "small", "medium", "large")


def synthetic_split(n_img, n_prop, max_gt, seed=0):
    """-> (annotation dict, [{"image_id", "boxes" f32 xyxy, "logits" f32}]); two thirds of the proposals lie around objects"""
    rng = np.random.default_rng(seed)
    ds = {"images": [{"id": k + 1} for k in range(n_img)], "categories": [{"id": 1, "name": "thing"}], "annotations": []}
    preds = []
    for k in range(n_img):
        g = int(rng.integers(1, max_gt + 1))
        wh = np.exp(rng.uniform(np.log(8), np.log(400), (g, 2)))
        xy = rng.uniform(0, 1, (g, 2)) * np.array([640.0, 480.0])
        gt = np.round(np.concatenate([xy, wh], 1), 2)
        area = np.round(gt[:, 2] * gt[:, 3] * rng.uniform(0.3, 1.0, g), 2)
        crowd = rng.random(g) < 0.03
        for b, a, c in zip(gt.tolist(), area.tolist(), crowd.tolist()):
            ds["annotations"].append({"id": len(ds["annotations"]) + 1, "image_id": k + 1, "category_id": 1, "bbox": b, "area": a, "iscrowd": int(c)})
        src = gt[rng.integers(0, g, n_prop)]
        near = rng.random(n_prop) < 0.66
        cx = np.where(near, src[:, 0] + src[:, 2] / 2 + rng.normal(0, 0.15, n_prop) * src[:, 2], rng.uniform(0, 640, n_prop))
        cy = np.where(near, src[:, 1] + src[:, 3] / 2 + rng.normal(0, 0.15, n_prop) * src[:, 3], rng.uniform(0, 480, n_prop))
        w = np.where(near, src[:, 2] * np.exp(rng.normal(0, 0.2, n_prop)), np.exp(rng.uniform(np.log(8), np.log(400), n_prop)))
        h = np.where(near, src[:, 3] * np.exp(rng.normal(0, 0.2, n_prop)), np.exp(rng.uniform(np.log(8), np.log(400), n_prop)))
        preds.append({"image_id": k + 1, "boxes": np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32),
                      "logits": (rng.permutation(n_prop) / np.float32(16.0)).astype(np.float32)})
    return ds, preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="minival", choices=sorted(SIZES))
    ap.add_argument("--images", type=int, default=None)
    ap.add_argument("--props", type=int, default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--restate-images", type=int, default=250)
    ap.add_argument("--kernel-only", action="store_true", help="the launches alone (for a kernel trace)")
    args = ap.parse_args()
    import torch
    import box_proposal_ref as R
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import box_proposals as BP
    from sos_wsod_amd import ops
    from sos_wsod_amd.evaluation import COCOGroundTruth

    size = dict(SIZES[args.size])
    n_img, n_prop = args.images or size["images"], args.props or size["props"]
    limits = list(size["limits"])
    ds, preds = synthetic_split(n_img, n_prop, size["max_gt"])
    gt = COCOGroundTruth(ds)
    out = {"size": args.size, "images": n_img, "proposals": n_img * n_prop, "gt_boxes": len(ds["annotations"]),
           "limits": [0 if l is None else l for l in limits], "areas": list(AREAS)}

    if not args.kernel_only:
        BP.box_proposal_metrics(preds[:8], gt, AREAS, limits)                                   # library load, first launch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, stats = BP.box_proposal_metrics(preds, gt, AREAS, limits, return_matches=False), None
        torch.cuda.synchronize()
        out["e2e_s"] = round(time.perf_counter() - t0, 3)
        out["metrics"] = {k: round(v, 4) for k, v in res.items()}

    t0 = time.perf_counter()
    L = BP.box_proposal_layout(preds, gt, list(AREAS), limits)
    out["layout_s"] = round(time.perf_counter() - t0, 3)
    thr = BP.default_thresholds().tolist()
    dev = [torch.from_numpy(np.ascontiguousarray(L[k])).cuda() for k in ("prop_off", "prop_box", "gt_off", "gt_box", "gt_area")]
    item_off = torch.from_numpy(L["item_off"]).cuda()
    n_out = int(L["item_off"][-1])
    bufs = (torch.empty(n_out, device="cuda"), torch.empty(n_out, device="cuda", dtype=torch.int32), torch.empty(n_out, device="cuda", dtype=torch.int32))

    def launch():
        return ops.box_proposal_ar(*dev, L["area_rng"].tolist(), L["limits"].tolist(), thr, item_off, overlap=bufs[0], match_gt=bufs[1],
                                   match_box=bufs[2], max_boxes=L["max_boxes"], max_props=L["max_props"], check_offsets=False)

    ref = launch()
    torch.cuda.synchronize()
    assert int(ref[4].item()) == 0
    ref_cnt, ref_ov = ref[3].clone(), ref[0].clone()
    times = []
    while len(times) < args.reps or sum(times) < 500.0:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        o = launch()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
        assert torch.equal(o[3], ref_cnt)
    assert torch.equal(o[0], ref_ov)                                                            # launches are bit-identical
    out["kernel_ms"] = round(float(np.median(times)), 3)
    out["kernel_launches"] = len(times)
    out["items_elements"] = n_out
    if args.kernel_only:
        print(json.dumps(out))
        return
    out["host_prep_s"] = round(out["e2e_s"] - out["kernel_ms"] / 1000, 3)
    out["host_share"] = round(out["host_prep_s"] / out["e2e_s"], 3)

    # the restatement on a prefix of the split, and the launch's counts against it
    m = min(args.restate_images, n_img)
    sub_ids = {p["image_id"] for p in preds[:m]}
    sub_ds = dict(ds, annotations=[a for a in ds["annotations"] if a["image_id"] in sub_ids])
    t0 = time.perf_counter()
    restated = {(a, l): R.evaluate(sub_ds, preds[:m], area=a, limit=l) for l in limits for a in AREAS}
    out["restated_s"] = round(time.perf_counter() - t0, 3)
    out["restated_images"] = m
    out["restated_full_s_est"] = round(out["restated_s"] * len(ds["annotations"]) / max(len(sub_ds["annotations"]), 1), 1)
    _, sub = BP.box_proposal_metrics(preds[:m], COCOGroundTruth(sub_ds), AREAS, limits, return_matches=True)
    for k, r in restated.items():
        s = sub[k]
        assert s["num_pos"] == r["num_pos"] and np.array_equal(s["gt_overlaps"].numpy().view(np.uint32), r["gt_overlaps"].view(np.uint32)), k
        assert np.array_equal(s["recalls"].numpy(), r["recalls"]), k
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Proposal recall at VOC07-test size: a synthetic split of --images images (4,952), --props scored proposals each (2,048, uint16
boxes as the MCG files hold them) and 1-5 ground-truth boxes per image (3 on average).  Prints one JSON line with

  kernel_ms      ops.proposal_recall alone (all ten budgets, eleven thresholds) on device-resident inputs: HIP events, the median
                 of at least --reps launches and at least 0.5 s of them, after a warm-up; the events span the whole call on an
                 idle stream, so the wrapper's check of the cuts (a copy of ten integers to the host) is inside
  e2e_s          proposal_recall.proposal_recall() from the in-memory arrays a reader returns: ranking, float64 conversion, CSR
                 build, upload, the kernel, the copy back — wall clock
  host_prep_s    e2e_s minus the kernel: what the host spends around it
  restated_s     the float64 NumPy restatement (tests/proposal_fixture.restated: one overlap pass per ground-truth box, every
                 budget read off as a prefix) on the same host for the same ranked input; restated_ten_pass_s is that pass run
                 once per budget, as the reference's script does (file reading not included)
and checks that the kernel's counts equal the restatement's.

    python tools/proposal_recall_bench.py [--images 4952] [--props 2048] [--reps 30]
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


def synthetic_split(n_img, n_prop, seed=0):
    rng = np.random.default_rng(seed)
    recs, boxes, scores = [], [], []
    for k in range(n_img):
        n_gt = int(rng.integers(1, 6))
        xy = rng.integers(0, 350, (n_gt, 2))
        gt = np.concatenate([xy, xy + rng.integers(20, 150, (n_gt, 2))], 1)
        pxy = rng.integers(0, 400, (n_prop, 2))
        b = np.concatenate([pxy, pxy + rng.integers(5, 200, (n_prop, 2))], 1)
        near = rng.integers(0, n_prop, min(40, n_prop))
        b[near] = np.maximum(gt[rng.integers(0, n_gt, len(near))] + rng.integers(-15, 16, (len(near), 4)), 0)
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2])
        recs.append({"file_name": f"{k + 1:06d}.jpg", "image_id": f"{k + 1:06d}",
                     "annotations": [{"bbox": [float(v) for v in g]} for g in gt]})
        boxes.append(b.astype(np.uint16))
        scores.append(rng.permutation(n_prop).reshape(-1, 1) / n_prop)
    return recs, boxes, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--props", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    import proposal_fixture as F
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import ops
    from sos_wsod_amd import proposal_recall as PR

    recs, boxes, scores = synthetic_split(args.images, args.props)
    out = {"images": args.images, "proposals": sum(len(b) for b in boxes), "gt_boxes": sum(len(d["annotations"]) for d in recs)}

    PR.proposal_recall(recs[:8], {"boxes": boxes[:8], "scores": scores[:8]}, "voc_2007_test")          # library load, first launch
    t0 = time.perf_counter()
    res = PR.proposal_recall(recs, {"boxes": boxes, "scores": scores}, "voc_2007_test")
    out["e2e_s"] = round(time.perf_counter() - t0, 3)

    lists = F.ranked(boxes, scores)
    gt_off, gt_box = PR._ground_truth(recs, "voc_2007_test")
    prop_off = np.concatenate([[0], np.cumsum([len(b) for b in lists])]).astype(np.int64)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
           (prop_off, np.concatenate([PR._boxes_f64(b) for b in lists]), gt_off, gt_box,
            np.asarray(PR.BUDGETS, dtype=np.int32), np.asarray(PR.IOU_THRESHOLDS, dtype=np.float64))]
    _, _, ref_cnt = ops.proposal_recall(*dev)
    torch.cuda.synchronize()
    times = []
    while len(times) < args.reps or sum(times) < 500.0:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _, _, cnt = ops.proposal_recall(*dev)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
        assert torch.equal(cnt, ref_cnt)
    out["kernel_ms"] = round(float(np.median(times)), 3)
    out["kernel_launches"] = len(times)
    out["host_prep_s"] = round(out["e2e_s"] - out["kernel_ms"] / 1000, 3)

    t0 = time.perf_counter()
    _, _, cnt, recall = F.restated(recs, lists, "voc_2007_test")
    out["restated_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    for m in PR.BUDGETS:
        F.restated(recs, [b[:m] for b in lists], "voc_2007_test", budgets=(m,))
    out["restated_ten_pass_s"] = round(time.perf_counter() - t0, 3)
    assert np.array_equal(cnt, res["cnt_yes"]) and np.array_equal(cnt, ref_cnt.cpu().numpy()) and F.same(recall, res["recall"])
    out["recall_at_0.5"] = [round(float(v), 4) for v in res["recall"][:, 0]]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

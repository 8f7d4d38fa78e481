"""Throughput of the Stage-3 split scorer (sos_wsod_amd.split.score_images): synthetic VOC-sized images (500 x 375, random
pixels, 1-4 boxes) through a voc_split.yaml detector (CE, smooth_l1_mean, positive fraction 1.0; random weights) at
images_per_batch 1, 4 and 8 -> images/s and the speed-up of batching, one JSON line.

    python tools/split_bench.py [--images 48] [--min-size 800] [--max-size 1333] [--repeats 2]

One shortest-edge size is used (--min-size) so that every image lands in one padded-shape bucket: the batches are then full, as
they are on a real training set, where each of the recipe's (size, orientation) buckets holds hundreds of images.  Kernel times
come from a separate run under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/split_bench.py ...` (sw_det_loss_per_image is
det_loss_partial_kernel + det_loss_fold_kernel)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--min-size", type=int, default=800)
    ap.add_argument("--max-size", type=int, default=1333)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import split
    from sos_wsod_amd.config import CfgNode
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN
    torch.manual_seed(0)
    cfg = CfgNode({"MODEL": {"BACKBONE": {"NAME": "build_resnet_fpn_backbone", "FREEZE_AT": 2},
                             "RPN": {"POSITIVE_FRACTION": 1.0, "BBOX_REG_LOSS_TYPE": "smooth_l1_mean"},
                             "ROI_HEADS": {"NAME": "StandardROIHeadsPseudoLab", "LOSS": "CrossEntropy", "POSITIVE_FRACTION": 1.0,
                                           "NUM_CLASSES": 20},
                             "ROI_BOX_HEAD": {"BBOX_REG_LOSS_TYPE": "smooth_l1_mean"},
                             "PIXEL_MEAN": [103.53, 116.28, 123.675], "PIXEL_STD": [1.0, 1.0, 1.0]}})
    model = TwoStagePseudoLabGeneralizedRCNN(cfg).cuda()
    g = np.random.default_rng(0)
    h, w = 375, 500
    imgs = [torch.from_numpy(g.integers(0, 256, (3, h, w), dtype=np.uint8)).cuda() for _ in range(args.images)]
    dicts = []
    for i in range(args.images):
        k = int(g.integers(1, 5))
        xy = g.random((k, 2)) * [w * 0.6, h * 0.6]
        wh = 24 + g.random((k, 2)) * [w * 0.35, h * 0.35]
        dicts.append({"height": h, "width": w, "i": i, "annotations": [
            {"bbox": [float(a) for a in np.concatenate([xy[j], xy[j] + wh[j]])], "bbox_mode": 0, "category_id": int(g.integers(0, 20))}
            for j in range(k)]})
    kw = dict(seed=0, min_sizes=(args.min_size,), max_size=args.max_size)
    res = {"images": args.images, "image_hw": [h, w], "min_size": args.min_size}
    scores = {}
    for ipb in (1, 4, 8):
        split.score_images(model, dicts[:max(ipb, 2)], lambda d: imgs[d["i"]], images_per_batch=ipb, **kw)     # warm-up
        torch.cuda.synchronize()
        best = None
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            s = split.score_images(model, dicts, lambda d: imgs[d["i"]], images_per_batch=ipb, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        scores[ipb] = s
        res[f"ipb{ipb}_images_per_s"] = round(args.images / best, 2)
    res["speedup_ipb4"] = round(res["ipb4_images_per_s"] / res["ipb1_images_per_s"], 3)
    res["speedup_ipb8"] = round(res["ipb8_images_per_s"] / res["ipb1_images_per_s"], 3)
    fin = np.isfinite(scores[1])
    res["max_rel_diff_ipb8_vs_alone"] = float(np.max(np.abs(scores[8][fin] - scores[1][fin]) / np.abs(scores[1][fin]))) if fin.any() else None
    res["nan_scores"] = int((~fin).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()

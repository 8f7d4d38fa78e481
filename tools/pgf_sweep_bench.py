"""The PGF threshold sweep at dataset scale: a VOC07-trainval-sized split (5,011 images x 100 detections, 20 classes, VOC records)
and a COCO-sized one (117,266 images x 100 detections, 80 classes, XYWH), synthetic as tools/pgf_bench.py builds them (1-3
ground-truth classes per image, 70 % of the detections of those classes) with 1-3 boxes per ground-truth class, at grids of
1 x 1, 8 x 8 and 32 x 32 and the ten IoU thresholds.  Prints one JSON line; per split and grid:

  kernel_ms        sw_pgf_sweep alone on device-resident inputs (HIP events around the call, its four memsets included; median of
                   --reps after a warm-up)
  module_s         sos_wsod_amd.pgf_sweep.sweep_voc / sweep_coco from records and dataset dicts to the SweepResult: grouping,
                   packing, upload, kernel, one copy back — wall clock
  composition_s    the same tables without the sweep: one pseudo_labels.filter_groups call per cell plus NumPy matching of the
                   kept rows (each detection's ovmax / jmax computed once, composition_setup_s, then counted per cell).  Timed on
                   --cells cells and extrapolated linearly to the grid; the timed cells are compared with the sweep's
                   (cells_equal).

    python tools/pgf_sweep_bench.py [--voc-images 5011] [--coco-images 117266] [--dets 100] [--cells 2] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IOU = [round(0.5 + 0.05 * i, 2) for i in range(10)]


def synthetic_split(n_img, n_det, K, voc, seed=0):
    """-> (detections, dataset dicts) in the dataset's own formats"""
    rng = np.random.default_rng(seed)
    dets, dicts, records = [], [], []
    for i in range(n_img):
        gt = rng.choice(K, int(rng.integers(1, 4)), replace=False)
        anns = []
        for c in gt:
            for _ in range(int(rng.integers(1, 4))):
                x, y = rng.uniform(0, 400, 2).round(1)
                w, h = rng.uniform(20, 200, 2).round(1)
                box = [x, y, x + w, y + h] if voc else [x, y, w, h]
                anns.append({"category_id": int(c), "bbox": [float(v) for v in box], "bbox_mode": 0 if voc else 1,
                             "difficult" if voc else "iscrowd": int(rng.random() < 0.1)})
        own = rng.random(n_det) < 0.7
        cls = np.where(own, gt[rng.integers(0, len(gt), n_det)], rng.integers(0, K, n_det))
        xy = rng.uniform(0, 500, (n_det, 2)).round(2)
        wh = rng.uniform(1, 200, (n_det, 2)).round(2)
        near = rng.random(n_det) < 0.3                                     # a third of the detections sit on an object of their class
        for k in np.nonzero(near)[0]:
            mine = [a for a in anns if a["category_id"] == cls[k]]
            if mine:
                b = mine[int(rng.integers(0, len(mine)))]["bbox"]
                xy[k] = np.round(np.array(b[:2]) + rng.uniform(-8, 8, 2), 2)
                wh[k] = np.round((np.array(b[2:]) - np.array(b[:2]) if voc else np.array(b[2:])) + rng.uniform(-8, 8, 2), 2)
        wh = np.maximum(wh, 1.0)
        scores = rng.random(n_det).round(4)
        if voc:
            boxes = np.concatenate([xy + 1.0, xy + wh], axis=1).tolist()     # the writer's [x1 + 1, y1 + 1, x2, y2]
            records += [{"image_id": i, "category_id": int(cls[k]) + 1, "score": float(scores[k]), "bbox": boxes[k]}
                        for k in range(n_det)]
        else:
            boxes = np.concatenate([xy, wh], axis=1).tolist()
            dets.append({"image_id": i, "instances": [{"image_id": i, "category_id": int(cls[k]), "bbox": boxes[k],
                                                       "score": float(scores[k])} for k in range(n_det)]})
        dicts.append({"image_id": f"{i:06d}" if voc else i, "annotations": anns})
    return (records if voc else dets), dicts


def numpy_overlaps(boxes, classes, off, gt_off, gt_box, gt_cls, xywh, p1):
    """each detection's ovmax and jmax (a ground-truth row, -1 without a candidate) by voc_eval's lines, vectorised per image"""
    n = len(classes)
    ovmax, jmax = np.full(n, -np.inf), np.full(n, -1, dtype=np.int64)
    bb = boxes.copy()
    if xywh:
        bb[:, 2:] = boxes[:, :2] + boxes[:, 2:]
    for k in range(len(off) - 1):
        a, b, ga, gb = off[k], off[k + 1], gt_off[k], gt_off[k + 1]
        if a == b or ga == gb:
            continue
        d, g = bb[a:b, None, :], gt_box[None, ga:gb, :]
        iw = np.maximum(np.minimum(g[..., 2], d[..., 2]) - np.maximum(g[..., 0], d[..., 0]) + p1, 0.0)
        ih = np.maximum(np.minimum(g[..., 3], d[..., 3]) - np.maximum(g[..., 1], d[..., 1]) + p1, 0.0)
        inters = iw * ih
        uni = (d[..., 2] - d[..., 0] + p1) * (d[..., 3] - d[..., 1] + p1) + (g[..., 2] - g[..., 0] + p1) * (g[..., 3] - g[..., 1] + p1) - inters
        with np.errstate(invalid="ignore", divide="ignore"):
            ov = np.where(classes[a:b, None] == gt_cls[None, ga:gb], inters / uni, -np.inf)
        j = np.argmax(ov, axis=1)
        best = ov[np.arange(b - a), j]
        has = best > -np.inf
        ovmax[a:b] = np.where(has, best, -np.inf)
        jmax[a:b] = np.where(has, ga + j, -1)
    return ovmax, jmax


def count_cell(rows, classes, ovmax, jmax, gt_cls, gt_ign, K):
    """kept [K], tp [10, K], ign [10, K] of the kept detection rows"""
    kept = np.bincount(classes[rows], minlength=K)
    tp, ign = np.zeros((len(IOU), K), dtype=np.int64), np.zeros((len(IOU), K), dtype=np.int64)
    ov, j = ovmax[rows], jmax[rows]
    ig = (j >= 0) & (gt_ign[np.maximum(j, 0)] != 0)
    for t, thr in enumerate(IOU):
        hit = ov > thr
        ign[t] = np.bincount(classes[rows][hit & ig], minlength=K)
        tp[t] = np.bincount(gt_cls[np.unique(j[hit & ~ig])], minlength=K)
    return kept, tp, ign


def run_split(name, voc, n_img, n_det, K, grids, cells, reps):
    import torch
    from sos_wsod_amd import ops
    from sos_wsod_amd import pgf_sweep as S
    from sos_wsod_amd import pseudo_labels as P
    t = time.perf_counter()
    dets, dicts = synthetic_split(n_img, n_det, K, voc)
    out = {"images": n_img, "detections": n_img * n_det, "build_s": round(time.perf_counter() - t, 1), "grids": {}}
    use_diff = not voc
    diff = P.VOC_DIFF_CLASSES if voc else ()
    groups, anns = (S.voc_groups if voc else S.coco_groups)(dets, dicts)
    class_dict = {i: P._unique(a["category_id"] for a in anns[i]) for i in groups}
    g = P.pack_groups(groups, class_dict, diff)
    shift = (1.0, 1.0, 0.0, 0.0) if voc else (0.0,) * 4
    gt_off, gt_box, gt_cls, gt_ign = S.pack_ground_truth(g["ids"], anns, g["universe"], "difficult" if voc else "iscrowd", shift)
    Kd = g["K"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    dev = [up(g["off"]), up(g["boxes"]), up(g["scores"]), up(g["classes"]), Kd, up(g["gt_mask"].view(np.int32)),
           up(g["diff_mask"].view(np.int32)), use_diff]
    dev_gt = [up(gt_off), up(gt_box), up(gt_cls), up(gt_ign), not voc, voc]

    # the composition's cell-independent part
    for k, d in enumerate(g["dets"]):
        d["_row"] = k
    t = time.perf_counter()
    ovmax, jmax = numpy_overlaps(g["boxes"], g["classes"], g["off"], gt_off, gt_box, gt_cls, not voc, 1.0 if voc else 0.0)
    out["composition_setup_s"] = round(time.perf_counter() - t, 2)
    print(name, "split built and packed", json.dumps({k: v for k, v in out.items() if k != "grids"}), file=sys.stderr, flush=True)

    rng = np.random.default_rng(1)
    for nk, nc in grids:
        t_keep = [0.2] if nk == 1 else np.linspace(0.0, 0.95, nk).round(4).tolist()
        t_con = [0.85] if nc == 1 else np.linspace(0.5, 1.0, nc).round(4).tolist()
        res = {}
        packed = ops.pgf_sweep(*dev, t_keep, t_con, IOU, *dev_gt)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.pgf_sweep(*dev, t_keep, t_con, IOU, *dev_gt)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        res["kernel_ms"] = round(float(np.median(times)), 3)
        res["kernel_ms_min"] = round(float(np.min(times)), 3)
        tables = ops.pgf_sweep_unpack(packed.cpu().numpy(), nk, nc, len(IOU), Kd)

        t = time.perf_counter()
        if voc:
            r = S.sweep_voc(dets, dicts, t_keep, t_con, IOU, use_diff)
        else:
            r = S.sweep_coco(dets, dicts, t_keep, t_con, IOU, use_diff)
        res["module_s"] = round(time.perf_counter() - t, 2)
        assert all(np.array_equal(getattr(r, key), tables[key]) for key in ("kept", "tp", "ign", "npos"))
        res["best_f1"] = r.best()

        picks = [(int(rng.integers(0, nk)), int(rng.integers(0, nc))) for _ in range(min(cells, nk * nc))]
        t = time.perf_counter()
        equal = True
        for a, b in picks:
            kept_groups, _ = P.filter_groups(groups, class_dict, t_con[b], t_keep[a], use_diff, diff)
            rows = np.fromiter((d["_row"] for ds in kept_groups.values() for d in ds), dtype=np.int64)
            kept, tp, ign = count_cell(rows, g["classes"], ovmax, jmax, gt_cls, gt_ign, Kd)
            equal &= bool(np.array_equal(kept, tables["kept"][a, b]) and np.array_equal(tp, tables["tp"][:, a, b])
                          and np.array_equal(ign, tables["ign"][:, a, b]))
        per_cell = (time.perf_counter() - t) / len(picks)
        res["composition_cells_timed"] = len(picks)
        res["composition_per_cell_s"] = round(per_cell, 3)
        res["composition_s"] = round(per_cell * nk * nc + out["composition_setup_s"], 1)
        res["cells_equal"] = equal
        out["grids"][f"{nk}x{nc}"] = res
        print(name, f"{nk}x{nc}", json.dumps(res), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voc-images", type=int, default=5011)
    ap.add_argument("--coco-images", type=int, default=117266)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--cells", type=int, default=2, help="cells of each grid the per-cell composition is timed on")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()

    import torch
    import sos_wsod_amd  # noqa: F401
    assert torch.cuda.is_available(), "pgf_sweep_bench needs the GPU"
    grids = [(1, 1), (8, 8), (32, 32)]
    out = {}
    if args.voc_images:
        out["voc07_trainval"] = run_split("voc", True, args.voc_images, args.dets, 20, grids, args.cells, args.reps)
    if args.coco_images:
        out["coco_2014_train_valminusminival"] = run_split("coco", False, args.coco_images, args.dets, 80, grids, args.cells, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

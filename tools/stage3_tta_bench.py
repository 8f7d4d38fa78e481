"""Cost of Stage-3 test-time augmentation (tta.GeneralizedRCNNWithTTA): one synthetic 375 x 500 image as the loader hands it over
(resized to 688 x 917), the VOC configuration's 8 sizes x flip = 16 views, K = 20, random weights -> one JSON line:

  * `wrapper_ms_per_image`: wall time of the wrapper per image (host clock around calls that end in the wrapper's own count read);
  * `merge_kernel_us`: device time of sw_tta_merge by HIP events, median of --launches (>= 200) single launches on resident inputs (the
    detections of the image above), with the minimum beside it — an event pair around one launch includes the launch's own gap, so
    this is an upper bound of the kernel time; a `rocprofv3 --kernel-trace --stats -- python tools/stage3_tta_bench.py --merge-only`
    run gives tta_merge_kernel alone;
  * with `--baseline`, `baseline_ms_per_image`: the same result composed ONLY from entry points of the parent commit — per-view batches
    through the default `model.inference` (one count read-back per view), the union concatenated and inverse-transformed in ATen, then
    the dense `ops.detect_postprocess` on a (N, K + 1) score matrix with one non-zero per row and every box repeated K times — timed
    alternately with the wrapper in the same process, and `baseline_equal`: whether both give the same detections.

    python tools/stage3_tta_bench.py [--baseline] [--images 20] [--launches 400] [--merge-only]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOC_SIZES = (480, 576, 672, 768, 864, 960, 1056, 1152)
K = 20


def baseline_image(model, w, inp):
    """parent-commit entry points only"""
    from sos_wsod_amd import ops
    from sos_wsod_amd.tta import _scale_xyxy
    h, wd = inp["image"].shape[-2:]
    orig = (inp["height"], inp["width"])
    views = w.tta_mapper(dict(inp))
    boxes, scores, classes = [], [], []
    for i in range(0, len(views), w.batch_size):
        for r, (_, t) in zip(model.inference([v for v, _ in views[i:i + w.batch_size]], do_postprocess=False), views[i:i + w.batch_size]):
            b = t.inverse_box(r.pred_boxes.tensor)
            if (h, wd) != orig:
                b = _scale_xyxy(b, orig[1] / wd, orig[0] / h)
            boxes.append(b); scores.append(r.scores); classes.append(r.pred_classes)
    boxes, scores, classes = torch.cat(boxes), torch.cat(scores), torch.cat(classes)
    N = boxes.shape[0]
    s2 = torch.zeros(N, K + 1, device=boxes.device)
    s2[torch.arange(N, device=boxes.device), classes] = scores
    cnt, b, s, c, _ = ops.detect_postprocess(s2, boxes.repeat(1, K).contiguous(), orig[0], orig[1], 1e-8, w.nms_thresh, w.topk)
    n = int(cnt.item())
    return b[:n], s[:n], c[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--merge-only", action="store_true")
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--launches", type=int, default=400)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from sos_wsod_amd import ops
    from sos_wsod_amd.config import get_cfg
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN
    from sos_wsod_amd.tta import GeneralizedRCNNWithTTA
    torch.manual_seed(0)
    model = TwoStagePseudoLabGeneralizedRCNN(num_classes=K, compute_dtype=torch.bfloat16).cuda().eval()
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.ROI_HEADS.NUM_CLASSES", K, "TEST.AUG.MIN_SIZES", VOC_SIZES, "TEST.AUG.ENABLED", True])
    w = GeneralizedRCNNWithTTA(cfg, model)
    g = torch.Generator().manual_seed(1)
    inp = {"image": torch.randint(0, 256, (3, 688, 917), generator=g, dtype=torch.uint8).cuda(), "height": 375, "width": 500}
    out = {"views": 2 * len(VOC_SIZES), "K": K, "compute_dtype": "bf16", "batch_size": w.batch_size}

    with torch.no_grad():
        block, tab, orig = w.merge_inputs(inp)
    args = (block.boxes, block.scores, block.classes, block.counts, tab, orig[0], orig[1], w.nms_thresh, w.topk, K)
    res = ops.tta_merge(*args)
    out["union_rows"] = int(block.counts.sum().item()); out["merged"] = ops.tta_merge_count(res[0])
    for _ in range(20):
        ops.tta_merge(*args, out=res)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(a.launches, 200))]
    for s, e in ev:
        s.record(); ops.tta_merge(*args, out=res); e.record()
    torch.cuda.synchronize()
    us = [s.elapsed_time(e) * 1e3 for s, e in ev]
    out["merge_kernel_us"] = round(statistics.median(us), 2); out["merge_kernel_us_min"] = round(min(us), 2)
    out["merge_launches"] = len(us)
    if a.merge_only:
        print(json.dumps(out))
        return

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, r
    new = lambda: w([inp])[0]["instances"]                                # noqa: E731
    old = lambda: baseline_image(model, w, inp)                           # noqa: E731
    with torch.no_grad():
        for _ in range(3):                                              # every view-batch shape warm on both paths
            new()
            if a.baseline:
                old()
        rounds, per = 4, max(a.images // 4, 1)
        tn, tb = [], []
        for _ in range(rounds):                                         # alternating windows
            t, inst = timed(new, per); tn.append(t)
            if a.baseline:
                t, base = timed(old, per); tb.append(t)
    out["wrapper_ms_per_image"] = round(statistics.median(tn), 3); out["wrapper_ms_windows"] = [round(t, 3) for t in tn]
    if a.baseline:
        out["baseline_ms_per_image"] = round(statistics.median(tb), 3); out["baseline_ms_windows"] = [round(t, 3) for t in tb]
        out["baseline_equal"] = bool(len(inst) == len(base[1]) and torch.equal(inst.pred_boxes.tensor, base[0])
                                     and torch.equal(inst.scores, base[1]) and torch.equal(inst.pred_classes.int(), base[2]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

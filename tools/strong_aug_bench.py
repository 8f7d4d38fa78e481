"""Cost of the Stage-3 strong augmentation (ops.strong_augment_multi_u8): the full recipe (four jitter ops with contrast in the
middle, blur at sigma 2.0, three rectangles) on a batch of 8 images of 800 x 1216 through the batched entry point -> one JSON line:
device time per batch and per image (HIP events around --iters calls after warm-up), host wall time per call, the bytes the
kernels move by construction (the L sum reads the image once, each blur direction reads and writes it once: 5 x 3HW, against the
2 x 3HW of one read and one write) and that traffic over the event time as a share of the 8 TB/s HBM peak; the same recipe
through Pillow on the host in one process (the reference's per-worker cost; skipped with a note when Pillow is absent); the
batch's share of the 12.7-13.2 ms Stage-3 iteration; and the time of the same call enqueued on the "side" worker stream while
a stand-in for the step (a chain of GEMMs) runs on the main stream.

    python tools/strong_aug_bench.py [--batch 8] [--hw 800 1216] [--iters 200]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/strong_aug_bench.py --iters 20
--no-host` (aug_lsum_kernel, aug_blur_h_kernel, aug_blur_v_kernel; aug_point_kernel for recipes without blur)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
STEP_MS = (12.7, 13.2)            # one GPU's share of a Stage-3 iteration


def pillow_ms(img_hwc, rc, repeats):
    try:
        from PIL import Image, ImageEnhance, ImageFilter
    except ImportError:
        return None
    g = np.random.default_rng(0)

    def once():
        im = Image.fromarray(img_hwc, "RGB")
        for op in rc.order:
            if op == "brightness":
                im = ImageEnhance.Brightness(im).enhance(rc.brightness)
            elif op == "contrast":
                im = ImageEnhance.Contrast(im).enhance(rc.contrast)
            elif op == "saturation":
                im = ImageEnhance.Color(im).enhance(rc.saturation)
            else:
                h, s, v = im.convert("HSV").split()
                nh = ((np.array(h, dtype=np.int32) + int(rc.hue * 255) % 256) & 255).astype(np.uint8)
                im = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
        im = im.filter(ImageFilter.GaussianBlur(radius=rc.blur_sigma))
        a = np.array(im).astype(np.float32) / 255.0                          # ToTensor
        for t, l, h, w in rc.rects:
            a[t:t + h, l:l + w] = g.standard_normal((h, w, 3), dtype=np.float32)
        return (a * 255.0).astype(np.int32).astype(np.uint8)                 # ToPILImage's byte()
    once()
    t0 = time.perf_counter()
    for _ in range(repeats):
        once()
    return (time.perf_counter() - t0) / repeats * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, nargs=2, default=(800, 1216))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-host", action="store_true", help="skip the Pillow timing (profiling runs)")
    args = ap.parse_args()
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd.strong_aug import Recipe
    assert torch.cuda.is_available(), "this benchmark measures the GPU path; there is no fallback"
    H, W = args.hw
    g = np.random.default_rng(0)
    host = [g.integers(0, 256, (3, H, W), dtype=np.uint8) for _ in range(args.batch)]
    imgs = [torch.from_numpy(a).cuda() for a in host]
    outs = [torch.empty_like(im) for im in imgs]
    rects = ((H // 8, W // 10, H // 3, W // 3), (H // 2, W // 2, H // 4, W // 3), (H // 3, W // 4, H // 2, W // 12))
    recipes = [Recipe(order=("brightness", "hue", "contrast", "saturation"), brightness=1.3, contrast=0.7, saturation=1.35, hue=0.08,
                      blur_sigma=2.0, rects=rects, seed=1, key=i) for i in range(args.batch)]
    for _ in range(10):
        ops.strong_augment_multi_u8(imgs, recipes, outs)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(args.iters):
        ops.strong_augment_multi_u8(imgs, recipes, outs)
    b.record()
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_wall = time.perf_counter() - t0
    batch_ms = a.elapsed_time(b) / args.iters
    px = 3 * H * W
    moved = 5 * px * args.batch
    res = {"batch": args.batch, "hw": [H, W], "iters": args.iters,
           "batch_ms_events": round(batch_ms, 4), "per_image_ms_events": round(batch_ms / args.batch, 4),
           "wall_ms_per_call": round(t_wall / args.iters * 1e3, 4), "host_enqueue_ms_per_call": round(t_enq / args.iters * 1e3, 4),
           "bytes_moved_per_image": 5 * px, "bytes_minimum_per_image": 2 * px,
           "traffic_over_event_time_share_of_hbm_peak": round(moved / (batch_ms * 1e-3) / HBM_PEAK, 4),
           "share_of_stage3_iteration": [round(batch_ms / s, 4) for s in STEP_MS]}
    # on the side stream, behind a stand-in for the step on the main stream
    side = ops.worker_stream("side")
    x = torch.randn(4096, 4096, device="cuda", dtype=torch.bfloat16)

    def step_standin():
        y = x
        for _ in range(24):
            y = y @ x
        return y
    def both():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.strong_augment_multi_u8(imgs, recipes, outs)
        step_standin()
        torch.cuda.current_stream().wait_stream(side)

    def timed(fn, n=10):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        t.record()
        torch.cuda.synchronize()
        return s.elapsed_time(t) / n
    for _ in range(3):                                       # warm-up of both forms (stream creation, first launches)
        step_standin(); both()
    torch.cuda.synchronize()
    alone, beside = [], []
    for _ in range(3):                                       # alternating, the smaller of three each
        alone.append(timed(step_standin)); beside.append(timed(both))
    res["standin_step_ms_alone"] = round(min(alone), 3)
    res["standin_step_ms_with_augmentation_on_side_stream"] = round(min(beside), 3)
    if not args.no_host:
        ms = pillow_ms(np.ascontiguousarray(host[0].transpose(1, 2, 0)), recipes[0], 5)
        res["pillow_ms_per_image_one_process"] = None if ms is None else round(ms, 2)
        if ms is None:
            res["pillow_note"] = "Pillow not installed: host path not measured"
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The elementwise / gather / loss kernels of csrc/detector.hip (and focal_loss of heads.hip) alone, at the sizes the Stage-3 step
(tools/stage3_step.py) launches them for two 800 x 1216 images in bf16: the ResNet-50-FPN maps are 400 x 608 (stem), 200 x 304
(res2 / P2), 100 x 152 (P3), 50 x 76 (P4), 25 x 38 (P5), the ROI heads sample 512 rows per image, the RPN sees 3 anchors per pixel of
P2 .. P6.  One line per entry, microseconds per call (median of 5 windows of 20 calls); TAG labels the lines (A/B of library builds
with SW_LIB_PATH)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sos_wsod_amd.ops as ops  # noqa: E402
from sos_wsod_amd import frcnn  # noqa: E402

dev, bf = "cuda", torch.bfloat16
torch.manual_seed(0)
N, K = 2, 20
LEVELS = [(200, 304), (100, 152), (50, 76), (25, 38), (13, 19)]          # P2 .. P6


def timeit(fn, n=20, windows=5):
    for _ in range(3):
        fn()
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n * 1e3)
    return sorted(out)[windows // 2]


def line(name, fn):
    print(f"{os.environ.get('TAG', '-'):8s} {name:58s} {timeit(fn):9.1f} us", flush=True)


def act(*shape):
    return torch.randn(*shape, device=dev).to(bf)


def boxes(n, lo, hi, W, H):
    wh = lo + torch.rand(n, 2, device=dev) * (hi - lo)
    xy = torch.rand(n, 2, device=dev) * (torch.tensor([W, H], device=dev) - wh)
    return torch.cat([xy, xy + wh], 1)


# ---- backbone / FPN
stem, pooled = act(N, 400, 608, 64), torch.empty(N, 200, 304, 64, device=dev, dtype=bf)
line("maxpool3x3s2: stem output 2x400x608x64", lambda: ops.maxpool3x3s2(stem, pooled))
res2, half = act(N, 200, 304, 256), torch.empty(N, 100, 152, 256, device=dev, dtype=bf)
res2b, res2o = act(N, 200, 304, 256), torch.empty(N, 200, 304, 256, device=dev, dtype=bf)
line("subsample2x: res2 output 2x200x304x256", lambda: ops.subsample2x(res2, half))
line("scatter2x: onto 2x200x304x256", lambda: ops.scatter2x(half, res2o))
line("add_relu: res2 size, 31.1 M elements", lambda: ops.add_relu(res2, res2b, res2o))
for name, (h, w) in zip(("P4", "P3", "P2"), LEVELS[2::-1]):
    lat, top, out = act(N, h, w, 256), act(N, h // 2, w // 2, 256), torch.empty(N, h, w, 256, device=dev, dtype=bf)
    down = torch.empty(N, h // 2, w // 2, 256, device=dev, dtype=bf)
    line(f"upsample2x_add: {name} 2x{h}x{w}x256", lambda: ops.upsample2x_add(lat, top, out))
    line(f"downsample2x_sum: from {name} 2x{h}x{w}x256", lambda: ops.downsample2x_sum(lat, down))

# ---- ROIAlign on the P2 map: the sampled rows of both images
R = N * 512
p2 = act(N, 200, 304, 256)
rois = torch.cat([torch.arange(N, device=dev).repeat_interleave(512)[:, None].float(), boxes(R, 16., 112., 1216., 800.)], 1)
sel = torch.arange(R, device=dev, dtype=torch.int32)
pooled_rows = torch.empty(R, 256 * 49, device=dev, dtype=bf)
gout = (torch.randn(R, 256 * 49, device=dev) * 1e-3).to(bf)
dfeat, acc = torch.zeros(N, 200, 304, 256, device=dev), torch.zeros(N, 200, 304, 256, device=dev, dtype=torch.int64)
amax, dmap = ops.absmax(gout), torch.empty(N, 200, 304, 256, device=dev, dtype=bf)
line("roi_align_fwd: 1024 rows, P2, 7x7x256", lambda: ops.roi_align_fwd(p2, rois, sel, pooled_rows, 0.25))
line("roi_align_bwd: 1024 rows, P2 (f32 atomics)", lambda: ops.roi_align_bwd(gout, rois, sel, dfeat, 0.25))
line("roi_align_bwd_fx: 1024 rows, P2 (fixed point)", lambda: ops.roi_align_bwd_fx(gout, rois, sel, acc, 0.25, amax))
line("fx_to_float: P2 map, 31.1 M elements", lambda: ops.fx_to_float(acc, amax, dmap))

# ---- losses
A = 3 * sum(h * w for h, w in LEVELS)
anchors = boxes(A, 32., 512., 1216., 800.)
matched = boxes(N * A, 32., 512., 1216., 800.).view(N, A, 4)
logits, deltas = torch.randn(N, A, device=dev), torch.randn(N, A, 4, device=dev) * 0.1
labels = torch.full((N, A), -1, dtype=torch.int8, device=dev)                        # 256 sampled anchors per image, half foreground
for i in range(N):
    pick = torch.randperm(A, device=dev)[:256]
    labels[i, pick[:128]] = 1; labels[i, pick[128:]] = 0
losses2, dl, dd = torch.empty(2, device=dev), torch.empty(N, A, device=dev), torch.empty(N, A, 4, device=dev)
line(f"rpn_loss: 2 x {A} anchors, with gradients",
     lambda: ops.rpn_loss(logits.view(-1), deltas.view(-1, 4), labels.view(-1), anchors, matched.view(-1, 4), (1., 1., 1., 1.), 1. / (256 * N),
                          losses2, dl.view(-1), dd.view(-1, 4)))
roi_logits = torch.randn(R, 5 * K + 1, device=dev)
roi_cls = torch.randint(0, K + 1, (R,), device=dev, dtype=torch.int32)
roi_boxes, roi_gt = boxes(R, 16., 400., 1216., 800.), boxes(R, 16., 400., 1216., 800.)
counts = torch.full((N,), 512, device=dev, dtype=torch.int32)
line("det_loss_per_image: 2 images, 512 rows each",
     lambda: ops.det_loss_per_image(logits, deltas, labels, anchors, matched, (1., 1., 1., 1.), 256, "smooth_l1", roi_logits, K, roi_cls,
                                    roi_boxes, roi_gt, counts, 512, (10., 10., 5., 5.), 1.5, "smooth_l1"))
floss, fgrad = torch.empty(1, device=dev), torch.empty(R, K + 1, device=dev)
line("focal_loss: 1024 x 21, with gradient", lambda: ops.focal_loss(roi_logits[:, :K + 1], roi_cls, 1.5, floss, fgrad))

# ---- weight staging: every weight of the detector in one launch
model = frcnn.TwoStagePseudoLabGeneralizedRCNN(num_classes=K, compute_dtype=bf).to(dev)
plan = frcnn.WeightStage(model, bf).plan
line(f"stage_weights_multi: the detector's {plan.n} weights", plan.run)

"""The step's second tier alone, at the VGG16 step's sizes: multi-tensor SGD (conv tiles, 64x64 tiles, vectors), the single-tensor SGD,
the batched column sums (partial rows + fold), the batched conv weight-gradient fold, the batched and single split-K folds and a split-K
GEMM whose fold runs the epilogue.  One line per kernel group, microseconds per call (median of 5 windows of 20 calls); TAG labels the
lines (A/B of library builds with SW_LIB_PATH)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sos_wsod_amd.ops as ops  # noqa: E402

dev, bf = "cuda", torch.bfloat16
torch.manual_seed(0)


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


rnd = lambda *s: torch.randn(*s, device=dev) * 0.01
convs = [(256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512), (512, 512), (512, 512), (512, 512)]   # conv3_1 .. conv5_3


def entry(p, staging):
    return dict(param=p, grad=rnd(*p.shape), buf=torch.zeros_like(p), lr=1e-3, weight_decay=5e-4, first=False, staging=staging, hyper=None)


es = []
for co, ci in convs:                                           # kind 2: OIHW master + both compute layouts (32 x 32 x 9 tiles)
    es.append(entry(rnd(co, ci, 3, 3), dict(kind=2, dtype=bf, stage0=torch.empty(co, 9, ci, device=dev, dtype=bf),
                                            stage1=torch.empty(ci, 9, co, device=dev, dtype=bf), d0=co, d1=ci, d2=ci, ld0=0)))
    es.append(entry(rnd(co), None))                            # biases: vector / scalar chunks
w2 = rnd(4096, 4096)                                           # fc7.weight: kind 3, row-major + transposed copy (64 x 64 tiles)
s0, s1 = torch.empty(4096, 4096, device=dev, dtype=bf), torch.empty(4096, 4096, device=dev, dtype=bf)
es.append(entry(w2, dict(kind=3, dtype=bf, stage0=s0, stage1=s1, d0=4096, d1=0, d2=0, ld0=4096, ld1=4096)))
wp = rnd(21 * 4, 4096)                                         # a predictor weight: kind 1
es.append(entry(wp, dict(kind=1, dtype=bf, stage0=torch.empty(84, 4096, device=dev, dtype=bf), stage1=None, d0=4096, d1=0, d2=0, ld0=4096)))
line("sgd_multi: 9 conv weights + biases, fc7.weight, a predictor", lambda: ops.sgd_multi(es, 0.9, 1.0))
f32e = dict(es[-2], staging=dict(kind=3, dtype=torch.float32, stage0=s0.float(), stage1=s1.float(), d0=4096, d1=0, d2=0, ld0=4096, ld1=4096))
line("sgd_multi: fc7.weight with float32 copies (64x64 tiles)", lambda: ops.sgd_multi([f32e], 0.9, 1.0))
p1, g1, b1 = rnd(4096 * 4096), rnd(4096 * 4096), torch.zeros(4096 * 4096, device=dev)
line("sgd_momentum_step: 16.8 M elements", lambda: ops.sgd_momentum_step(p1, g1, b1, 1e-3, 0.9, 5e-4, False, 1.0))

# bias gradients of a backward pass: dY of the nine layers at two view batches (2 x 63 x 63 ... 2 x 126 x 126 pixels)
parts, folds = [], []
for k, (co, ci) in enumerate(convs):
    for px in (2 * 63 * 63, 2 * 94 * 94) if k >= 3 else (2 * 126 * 126, 2 * 188 * 188):
        X = (torch.randn(px, co, device=dev) * 0.1).to(bf)
        rows = ops.colsum_nrows(bf, px, co)
        ws = torch.empty(rows, co, device=dev)
        parts.append((X, ws)); folds.append((ws, rows, torch.empty(co, device=dev)))
line("colsum_partial_multi: 18 dY matrices", lambda: ops.colsum_partial_multi(parts))
line("colsum_fold_multi: 18 folds", lambda: ops.colsum_fold_multi(folds))

wf = [(torch.randn(6, co * 9 * ci, device=dev), 6, torch.empty(co, ci, 3, 3, device=dev)) for co, ci in convs]
line("conv3x3_wgrad_fold_multi: 9 layers x 6 slabs", lambda: ops.conv3x3_wgrad_fold_multi(wf))
cs = torch.ones(512, device=dev)
line("conv3x3_wgrad_fold: conv5_3, 6 slabs, with a channel scale", lambda: ops.conv3x3_wgrad_fold(wf[-1][0], 6, wf[-1][2], cout_scale=cs))
sf = [(torch.randn(5, M * N, device=dev), 5, torch.empty(M, N, device=dev), torch.ones(M, device=dev), False)
      for M, N in ((256, 1024), (512, 2048), (1024, 256), (2048, 512), (512, 512), (64, 256))]
line("splitk_fold_multi: 6 folds x 5 slabs, row scale", lambda: ops.splitk_fold_multi(sf))
M, N, K = 950, 512, 2048
A, B = torch.randn(M, K, device=dev).to(bf), torch.randn(N, K, device=dev).to(bf)
bias, res, C = torch.randn(N, device=dev), torch.randn(M, N, device=dev).to(bf), torch.empty(M, N, device=dev, dtype=bf)
line("gemm 950x512x2048 split-K 4, bias + residual + ReLU in the fold",
     lambda: ops.gemm(A, B, C, M, N, K, ep=ops.make_epilogue(bias=bias, relu=True, residual=res, out_dtype=bf), splitk=4))
Cf = torch.empty(M, N, device=dev)
line("gemm 950x512x2048 split-K 4, plain float32 (ordered fold)", lambda: ops.gemm(A, B, Cf, M, N, K, splitk=4))

"""float64 restatements of the Stage-3 detector's dense kernels (csrc/detector.hip, the RPN layout kernels of csrc/proposals.hip),
the case tables of tests/test_gpu_detector_kernels.py and the tolerance table those tests read.  Checkers, not product code; CPU only.

Every reference takes the values the kernel gets (for bf16: the inputs rounded to bf16 first) upcast to float64, so input rounding is
common to both sides.  tests/test_detector_ref_cpu.py pins each restatement to torch (conv2d, max_pool2d, interpolate, avg_pool2d x 4)
or to the C ROIAlign oracle, and asserts that each case table reaches the edge it is named for.

Tolerances.  Selection, copy and a single rounded add are compared bit for bit.  The accumulating kernels (stem, downsample sum,
ROIAlign, the RPN / ROI cotangent scalings) are compared with float64 as max|got - ref| / max|ref|, and the bar is taken from the
reference, never from the kernel: the float32 form of the same formula in the reference's own order (torch conv2d, (a + b) + (c + d),
the C ROIAlign oracle, a float32 multiply) runs on the case inputs, e32 = max|f32 - f64| / max|f64| per (kind, dtype), and the bar is
max(2e-5, 8 * e32) of max|ref| (floor and factor of heads_ref: a different but legitimate summation order), plus half a bf16 ulp of
max|ref| where the output is bf16.  E32 below is that table; test_detector_ref_cpu.py recomputes it and asserts it is current.
"""
import functools
import math

import numpy as np
import torch

BAR_FLOOR = 2e-5
BAR_FACTOR = 8.0
DTYPES = ("f32", "bf16")
VEC = {"f32": 4, "bf16": 8}                # elements of a 16-byte piece: the vector kernels need C % VEC == 0 and 16-byte alignment
ESIZE = {"f32": 4, "bf16": 2}
SLACK = 16                                 # sentinel elements behind every output
AXIS_MAX = 9                               # csrc/detector.hip: the per-axis register form of the ROIAlign backward takes grids < AXIS_MAX


def torch_dtype(d):
    return torch.float32 if d == "f32" else torch.bfloat16


def rel_err(got, ref):
    """max|got - ref| / max|ref| (0 / 0 -> 0: an all-zero reference asks for exact zeros; NaN -> inf)"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    d = float(np.max(np.abs(got - ref))); m = float(np.max(np.abs(ref)))
    if not d <= math.inf:
        return math.inf
    return 0.0 if d == 0.0 else (math.inf if m == 0.0 else d / m)


def bf16_half_ulp(m):
    """half a bf16 unit in the last place at magnitude m (8 significant bits: ulp = 2^(floor(log2 m) - 7))"""
    return 0.0 if m == 0.0 else 2.0 ** (math.floor(math.log2(m)) - 8)


def bar(kind, dtype):
    """allowed max|got - ref| / max|ref| of float32 arithmetic for `kind` with `dtype` inputs"""
    return max(BAR_FLOOR, BAR_FACTOR * E32[(kind, dtype)])


def allowed(kind, dtype, ref, out_bf16):
    """allowed max|got - ref| (absolute): the bar times max|ref|, plus half a bf16 ulp of max|ref| for a bf16 output"""
    m = float(np.max(np.abs(ref))) if np.size(ref) else 0.0
    return bar(kind, dtype) * m + (bf16_half_ulp(m) if out_bf16 else 0.0)


def round_to(x, dtype):
    """float32 array with the values `dtype` holds (bf16: round to nearest even)"""
    x = np.ascontiguousarray(x, np.float32)
    return x if dtype == "f32" else torch.from_numpy(x).to(torch.bfloat16).float().numpy()


def same_bits(got, want):
    """bit equality of two float32 arrays, any NaN equal to any NaN"""
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(np.all((got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))))


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


# ============================================================================================ preprocess_pad
DEFAULT_MEAN, DEFAULT_STD = (103.530, 116.280, 123.675), (1.0, 1.0, 1.0)
OTHER_MEAN, OTHER_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
# (h, w, H, W, mean, std): padded; no padding at all; one pixel; non-default mean / std (a division that rounds)
PREPROCESS_CASES = [(37, 50, 64, 64, DEFAULT_MEAN, DEFAULT_STD), (32, 48, 32, 48, DEFAULT_MEAN, DEFAULT_STD),
                    (1, 1, 32, 32, DEFAULT_MEAN, DEFAULT_STD), (37, 50, 64, 64, OTHER_MEAN, OTHER_STD),
                    (1, 1, 32, 32, OTHER_MEAN, OTHER_STD)]


def preprocess_inputs(h, w):
    return _rng(11, h, w).integers(0, 256, (3, h, w), dtype=np.uint8)


def preprocess_ref(img_u8, H, W, mean, std):
    """-> (H, W, 4) float32 = (u8 - m) / s in float32 (m, s the float32 values the launch receives), 0 in the padding and channel 3"""
    _, h, w = img_u8.shape
    out = np.zeros((H, W, 4), np.float32)
    m = np.asarray(mean, np.float32).reshape(3, 1, 1); s = np.asarray(std, np.float32).reshape(3, 1, 1)
    out[:h, :w, :3] = ((img_u8.astype(np.float32) - m) / s).transpose(1, 2, 0)
    return out


# ============================================================================================ stem: conv 7x7 s2 p3 + affine + ReLU
STEM_TILE = 8                              # the workgroup is an 8 x 8 tile of output pixels (21 x 21 input patch)
# the last: partial tiles behind full ones on both axes (the others end on a tile boundary in x)
STEM_HW = [(16, 16), (17, 15), (5, 9), (33, 47), (70, 96), (21, 37)]
STEM_CASES = [(N, H, W) for (H, W) in STEM_HW for N in (1, 3)]


def stem_out_hw(H, W):
    return (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1


@functools.lru_cache(maxsize=None)
def stem_inputs(N, H, W, dtype):
    """-> x (N, H, W, 4) float32 (values of `dtype`; channel 3 holds NaN: never read), w (64, 3, 7, 7), scale (64,) of both signs,
    bias (64,)"""
    r = _rng(21, N, H, W)
    x = np.full((N, H, W, 4), np.nan, np.float32)
    x[..., :3] = round_to(r.normal(0.0, 50.0, (N, H, W, 3)), dtype)
    w = r.normal(0.0, 0.05, (64, 3, 7, 7)).astype(np.float32)
    scale = ((r.random(64) + 0.5) * r.choice([-1.0, 1.0], 64)).astype(np.float32)
    bias = r.normal(0.0, 0.1, 64).astype(np.float32)
    return x, w, scale, bias


def stem_ref(x, w, scale, bias):
    """x (N, H, W, >= 3) -> (N, OH, OW, 64) float64 = relu(conv7x7(stride 2, padding 3) * scale + bias), index by index"""
    x = np.asarray(x, np.float64)[..., :3]
    N, H, W, _ = x.shape
    xp = np.zeros((N, H + 6, W + 6, 3)); xp[:, 3:3 + H, 3:3 + W] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, (7, 7), axis=(1, 2))[:, ::2, ::2]       # (N, OH, OW, 3, 7, 7)
    y = np.einsum("nyxcij,ocij->nyxo", win, np.asarray(w, np.float64))
    y = y * np.asarray(scale, np.float64) + np.asarray(bias, np.float64)
    return np.where(y < 0, 0.0, y)


def stem_f32(x, w, scale, bias):
    """the same through torch's float32 conv2d (the reference's own form: resnet.py BasicStem with the FrozenBN fold)"""
    import torch.nn.functional as F
    xt = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)[..., :3])).permute(0, 3, 1, 2)
    y = F.conv2d(xt, torch.from_numpy(w), None, stride=2, padding=3) * torch.from_numpy(scale).view(1, -1, 1, 1) \
        + torch.from_numpy(bias).view(1, -1, 1, 1)
    return F.relu(y).permute(0, 2, 3, 1).numpy()


# ============================================================================================ maxpool 3x3 s2 p1
POOL_HW = [(1, 1), (2, 2), (1, 7), (8, 8), (9, 13), (35, 48)]
POOL_C = [6, 12, 16, 64]
POOL_CASES = [(H, W, C) for (H, W) in POOL_HW for C in POOL_C]
POOL_REGIMES = ("normal", "negative", "special")


def takes_vector_path(C, dtype, misaligned=False):
    return C % VEC[dtype] == 0 and not misaligned


@functools.lru_cache(maxsize=None)
def pool_inputs(N, H, W, C, dtype, regime):
    """normal N(0,1); negative: all below 0 (the padding can never win); special: -inf windows, NaN, zeros of both signs"""
    r = _rng(31, N, H, W, C, POOL_REGIMES.index(regime))
    x = r.normal(0.0, 1.0, (N, H, W, C)).astype(np.float32)
    if regime == "negative":
        x = -np.abs(x) - np.float32(0.5)
    if regime == "special":
        k = r.integers(0, 8, x.shape)
        x[k == 0] = -np.inf; x[k == 1] = 0.0; x[k == 2] = -0.0
        x[r.random(x.shape) < 0.04] = np.nan
        x[:, : (H + 1) // 2, : (W + 1) // 2, 0] = -np.inf       # whole windows of -inf in channel 0
    return round_to(x, dtype)


def maxpool_ref(x):
    """x (N, H, W, C) float32 -> (N, OH, OW, C) float32: the nine taps in row-major order, max = v where v > max or v is NaN, from
    -inf (aten/src/ATen/native/cpu/MaxPoolKernel.cpp).  A selection: exact in any precision."""
    x = np.asarray(x, np.float32)
    N, H, W, C = x.shape
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    xp = np.full((N, 2 * OH + 1, 2 * OW + 1, C), -np.inf, np.float32)
    xp[:, 1:1 + H, 1:1 + W] = x
    m = np.full((N, OH, OW, C), -np.inf, np.float32)
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]
            with np.errstate(invalid="ignore"):
                m = np.where((v > m) | np.isnan(v), v, m)
    return m


# ============================================================================================ subsample2x / scatter2x
SUB_HW = [(1, 1), (1, 6), (9, 13), (8, 8)]
SUB_C = [3, 8, 12, 16]                     # 12: whole 16-byte pieces in f32, a multiple of 4 but not of 8 elements in bf16
SUB_CASES = [(H, W, C) for (H, W) in SUB_HW for C in SUB_C]


def takes_copy16_path(C, dtype, misaligned=False):
    return (C * ESIZE[dtype]) % 16 == 0 and not misaligned


def dense_inputs(tag, shape, dtype, sd=1.0):
    return round_to(_rng(41, tag, *shape).normal(0.0, sd, shape), dtype)


def subsample_ref(x):
    return np.ascontiguousarray(x[:, ::2, ::2])


def scatter_ref(g, H, W):
    out = np.zeros((g.shape[0], H, W, g.shape[3]), g.dtype)
    out[:, ::2, ::2] = g
    return out


# ============================================================================================ add_relu
ADD_N = [1, 255, 256, 257, 100003]


@functools.lru_cache(maxsize=None)
def add_inputs(n, dtype):
    """-> a, b float32 (values of `dtype`); from n >= 255 on: NaN in a, NaN in b, (-0) + (-0), (-0) + (+0), x + (-x), -inf"""
    r = _rng(51, n)
    a = round_to(r.normal(0.0, 2.0, n), dtype); b = round_to(r.normal(0.0, 2.0, n), dtype)
    if n >= 255:
        a[3] = np.nan; b[7] = np.nan; a[11] = -0.0; b[11] = -0.0; a[13] = -0.0; b[13] = 0.0; b[17] = -a[17]
        a[19] = -np.inf; a[n - 1] = np.nan; b[n - 2] = -0.0; a[n - 2] = -0.0
    return a, b


def add_relu_ref(a, b, relu, dtype):
    """one float32 add, torch's relu (clamp_min: NaN stays, -0 stays), one rounding to `dtype`"""
    with np.errstate(invalid="ignore"):
        v = np.asarray(a, np.float32) + np.asarray(b, np.float32)
        if relu:
            v = np.where(v < 0, np.float32(0.0), v)
    return round_to(v, dtype)


# ============================================================================================ upsample2x_add / downsample2x_sum
FPN_HW = [(1, 1), (1, 5), (4, 6), (13, 19)]
FPN_C = [3, 8, 12, 256]
FPN_N = [1, 3]
FPN_CASES = [(h, w, C) for (h, w) in FPN_HW for C in FPN_C]


def upsample_add_ref(lateral, top, dtype):
    """lateral (N, 2h, 2w, C) + nearest 2x of top (N, h, w, C): one float32 add, one rounding"""
    up = np.repeat(np.repeat(np.asarray(top, np.float32), 2, axis=1), 2, axis=2)
    return round_to(np.asarray(lateral, np.float32) + up, dtype)


def downsample_sum_f32(g):
    """(a + b) + (c + d) over each 2 x 2 block in float32: a, b the upper pixels left to right, c, d the lower ones"""
    g = np.asarray(g, np.float32)
    return (g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + (g[:, 1::2, 0::2] + g[:, 1::2, 1::2])


def downsample_sum_ref(g):
    g = np.asarray(g, np.float64)
    return g[:, 0::2, 0::2] + g[:, 0::2, 1::2] + g[:, 1::2, 0::2] + g[:, 1::2, 1::2]


# ============================================================================================ ROIAlign (aligned, NHWC kernels)
ROI_N, ROI_H, ROI_W, ROI_SCALE = 3, 72, 80, 0.25
ROI_C = [3, 8]
ROI_CONFIGS = [(7, 7, 0), (14, 14, 0), (7, 3, 0), (7, 7, 2)]          # (PH, PW, sampling_ratio)
ROI_GRIDS = (1, 2, 6, 7, 8, 9, 12)
ROI_GRID_PAIRS = ((8, 8), (8, 9), (9, 8), (9, 9), (12, 1))
# (image, x0, y0, width, height) in feature pixels (x 4 = image coordinates); grid = ceil(size / 7) at 7 x 7 bins
_ROI_FIXED = [
    (0, 3.3, 2.7, 5.1, 4.2),            # 1 x 1
    (1, 10.0, 20.0, 7.0, 7.0),          # bin == grid == 1
    (2, 30.5, 11.25, 10.3, 13.1),       # 2 x 2
    (0, 8.0, 9.0, 14.0, 14.0),          # bin == grid == 2
    (1, 20.4, 15.2, 38.7, 40.1),        # 6 x 6
    (2, 5.5, 3.5, 45.3, 47.9),          # 7 x 7
    (0, 12.0, 8.0, 49.0, 49.0),         # bin == grid == 7
    (1, 9.3, 4.1, 52.6, 54.2),          # 8 x 8: all nine slots of the register form
    (2, 16.0, 12.0, 56.0, 56.0),        # bin == grid == 8 (a 56-pixel ROI: sample spacing exactly 1)
    (0, 7.7, 6.2, 58.4, 53.3),          # (8, 9): one axis below, one above the limit
    (1, 11.1, 3.9, 51.7, 60.2),         # (9, 8)
    (2, 6.4, 5.8, 60.9, 59.5),          # (9, 9): the sample-by-sample form
    (0, 13.0, 4.0, 63.0, 63.0),         # bin == grid == 9
    (1, 40.2, -3.0, 4.4, 80.5),         # (12, 1), over the top and the bottom border
    (2, 1.0, 30.3, 78.9, 5.5),          # (1, 12)
    (0, 0.5, 0.5, 79.0, 71.0),          # the whole map: (11, 12)
    (1, 2.2, 1.1, 80.1, 13.0),          # (2, 12)
    (2, 33.0, 2.0, 40.3, 66.6),         # (10, 6)
    (0, 4.0, 10.0, 65.0, 44.0),         # (7, 10)
    (1, -20.3, 10.2, 53.1, 52.2),       # grid 8 across the left border: the clamp at 0 inside a nine-slot span
    (2, 45.6, 9.9, 55.2, 51.0),         # ... the right border: the clamp at W - 1
    (0, 14.4, -18.6, 50.5, 55.5),       # ... the top border
    (1, 12.1, 38.3, 54.4, 52.8),        # ... the bottom border
    (2, -10.5, -12.5, 55.0, 55.0),      # the top left corner
    (0, 40.0, 35.0, 55.9, 54.1),        # the bottom right corner
    (1, 100.0, 90.0, 20.0, 20.0),       # wholly outside (right, below): output 0
    (2, -60.0, -50.0, 30.0, 30.0),      # wholly outside (left, above)
    (0, 85.0, 10.0, 30.0, 30.0),        # wholly outside in x only
    (1, 20.0, 20.0, 0.0, 0.0),          # zero area
    (2, 79.6, 71.7, 6.0, 6.0),          # the last pixel and beyond
]
ROI_RANDOM = 30


@functools.lru_cache(maxsize=None)
def roi_set():
    """-> rois (R, 5) float32 = (image, x1, y1, x2, y2) in image coordinates, R = 60"""
    r = _rng(61)
    rows = list(_ROI_FIXED)
    for i in range(ROI_RANDOM):
        gh, gw = (int(r.choice(ROI_GRIDS)) for _ in range(2))
        h, w = (float(r.uniform(7.0 * (g - 1) + 0.2, 7.0 * g - 0.2)) for g in (gh, gw))
        y0 = float(r.uniform(-5.0, max(ROI_H - h + 5.0, -3.0))); x0 = float(r.uniform(-5.0, max(ROI_W - w + 5.0, -3.0)))
        rows.append((i % ROI_N, x0, y0, w, h))
    a = np.asarray(rows, np.float64)
    rois = np.stack([a[:, 0], a[:, 1] * 4, a[:, 2] * 4, (a[:, 1] + a[:, 3]) * 4, (a[:, 2] + a[:, 4]) * 4], 1)
    return np.ascontiguousarray(rois, np.float32)


def roi_geometry(rois, PH, PW, sampling_ratio, scale=ROI_SCALE):
    """the float32 geometry of ROIAlign_cpu.cpp:137-169, operation by operation -> dict of per-ROI arrays: batch, start_h, start_w,
    bin_h, bin_w (float32), grid_h, grid_w (int), count"""
    f = np.float32
    rois = np.asarray(rois, f); s = f(scale); half = f(0.5)
    sw = rois[:, 1] * s - half; sh = rois[:, 2] * s - half
    ew = rois[:, 3] * s - half; eh = rois[:, 4] * s - half
    rw = ew - sw; rh = eh - sh
    bh = rh / f(PH); bw = rw / f(PW)
    if sampling_ratio > 0:
        gh = np.full(len(rois), sampling_ratio, np.int64); gw = gh.copy()
    else:
        gh = np.ceil(rh / f(PH)).astype(np.int64); gw = np.ceil(rw / f(PW)).astype(np.int64)
    return dict(batch=rois[:, 0].astype(np.int64), start_h=sh, start_w=sw, bin_h=bh, bin_w=bw, grid_h=gh, grid_w=gw,
                count=np.maximum(gh * gw, 1).astype(np.float64))


def roi_bwd_form(g, i):
    """'axis' (per-axis register form) or 'sample' (sample by sample): the guard of roi_align_bwd_kernel for ROI i"""
    ok = (g["grid_h"][i] < AXIS_MAX and g["grid_w"][i] < AXIS_MAX and g["bin_h"][i] <= np.float32(g["grid_h"][i])
          and g["bin_w"][i] <= np.float32(g["grid_w"][i]))
    return "axis" if ok else "sample"


def _axis_matrix(start, bin_, grid, P, size):
    """(P, size) float64: the summed interpolation weights of bin p's `grid` samples on each pixel of one axis.  The sample
    coordinates are the float32 values of the reference (start + p * bin + (i + .5) * bin / grid, left to right); the weights and
    their sums are float64.  Samples outside [-1, size] contribute nothing; coordinates clamp to [0, size - 1]."""
    f = np.float32
    Wm = np.zeros((P, size))
    if grid <= 0:
        return Wm
    p = np.arange(P, dtype=f)[:, None]; i = np.arange(grid, dtype=f)[None, :]
    y = (f(start) + p * f(bin_)) + ((i + f(0.5)) * f(bin_)) / f(grid)             # float32 throughout
    assert y.dtype == np.float32
    valid = ~((y < f(-1.0)) | (y > f(size)))
    y = np.where(y <= 0, f(0.0), y)
    lo = y.astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo); hi = np.where(top, size - 1, lo + 1)
    y64 = np.where(top, float(size - 1), y.astype(np.float64))
    l = y64 - lo; h = 1.0 - l
    pp = np.broadcast_to(np.arange(P)[:, None], y.shape)
    np.add.at(Wm, (pp[valid], lo[valid]), h[valid])
    np.add.at(Wm, (pp[valid], hi[valid]), l[valid])
    return Wm


def roi_align_fwd_ref(feat_nhwc, rois, PH, PW, sampling_ratio, scale=ROI_SCALE):
    """feat (N, H, W, C) -> (R, C, PH, PW) float64"""
    feat = np.asarray(feat_nhwc, np.float64)
    _, H, W, C = feat.shape
    g = roi_geometry(rois, PH, PW, sampling_ratio, scale)
    out = np.zeros((len(rois), C, PH, PW))
    for r in range(len(rois)):
        Wy = _axis_matrix(g["start_h"][r], g["bin_h"][r], int(g["grid_h"][r]), PH, H)
        Wx = _axis_matrix(g["start_w"][r], g["bin_w"][r], int(g["grid_w"][r]), PW, W)
        out[r] = np.einsum("py,qx,yxc->cpq", Wy, Wx, feat[g["batch"][r]], optimize=True) / g["count"][r]
    return out


def roi_align_bwd_ref(gout, rois, PH, PW, sampling_ratio, feat_shape, scale=ROI_SCALE):
    """gout (R, C, PH, PW) -> dfeat (N, H, W, C) float64"""
    gout = np.asarray(gout, np.float64)
    N, H, W, C = feat_shape
    g = roi_geometry(rois, PH, PW, sampling_ratio, scale)
    d = np.zeros((N, H, W, C))
    for r in range(len(rois)):
        Wy = _axis_matrix(g["start_h"][r], g["bin_h"][r], int(g["grid_h"][r]), PH, H)
        Wx = _axis_matrix(g["start_w"][r], g["bin_w"][r], int(g["grid_w"][r]), PW, W)
        d[g["batch"][r]] += np.einsum("py,qx,cpq->yxc", Wy, Wx, gout[r], optimize=True) / g["count"][r]
    return d


@functools.lru_cache(maxsize=None)
def roi_feat(C, dtype):
    return dense_inputs(62, (ROI_N, ROI_H, ROI_W, C), dtype)


@functools.lru_cache(maxsize=None)
def roi_gout(C, PH, PW, dtype):
    """(R, C, PH, PW) float32 (values of `dtype`), magnitudes that differ from ROI to ROI"""
    R = len(roi_set())
    r = _rng(63, C, PH, PW)
    return round_to(r.normal(0.0, 1.0, (R, C, PH, PW)) * np.exp(r.normal(0.0, 1.0, (R, 1, 1, 1))), dtype)


@functools.lru_cache(maxsize=None)
def roi_fwd_expected(C, cfg, dtype):
    return roi_align_fwd_ref(roi_feat(C, dtype), roi_set(), *cfg)


@functools.lru_cache(maxsize=None)
def roi_bwd_expected(C, cfg, dtype):
    return roi_align_bwd_ref(roi_gout(C, cfg[0], cfg[1], dtype), roi_set(), *cfg, (ROI_N, ROI_H, ROI_W, C))


def roi_sel_shuffled():
    """about two thirds of the rows in shuffled order (gaps: the other rows must keep the sentinel)"""
    R = len(roi_set())
    return np.ascontiguousarray(_rng(64).permutation(R)[: 2 * R // 3], np.int32)


# ============================================================================================ rpn_unpack / rpn_unpack_bwd
# (N, A, hw per level, ld): one pixel; five levels with ld = 5A exactly; ld > 5A; many anchors
RPN_CASES = [(1, 1, (1,), 5), (3, 3, (12, 6, 2, 1, 1), 15), (2, 3, (35, 9, 4), 16), (3, 15, (20, 5), 80)]


def rpn_rows(N, hw):
    return N * int(sum(hw))


def rpn_inputs(N, A, hw, ld):
    """-> y (rows, ld) float32 with NaN in the padding columns (never read), dlogits (N, At), ddeltas (N, At, 4), g_logits, g_deltas"""
    r = _rng(71, N, A, ld, *hw)
    rows, At = rpn_rows(N, hw), A * int(sum(hw))
    y = np.full((rows, ld), np.nan, np.float32)
    y[:, :5 * A] = r.normal(0.0, 1.0, (rows, 5 * A))
    return (y, r.normal(0.0, 1.0, (N, At)).astype(np.float32), r.normal(0.0, 1.0, (N, At, 4)).astype(np.float32),
            np.float32(r.uniform(0.3, 1.7)), np.float32(r.uniform(0.3, 1.7)))


def rpn_index(N, A, hw):
    """the layout comment above rpn_unpack_kernel as index arrays: for anchor j of image n -> (row, logit column); its four deltas
    sit at columns A + 4 a + b.  Row = row_off[level] + n * hw[level] + pixel, row_off[l] = N * sum(hw[:l]); anchor order of an
    image: level-major, pixel-major, anchor-minor."""
    At = A * int(sum(hw))
    row = np.zeros((N, At), np.int64); col = np.zeros((N, At), np.int64)
    for n in range(N):
        j = 0; row_off = 0
        for h in hw:
            for pix in range(h):
                for a in range(A):
                    row[n, j] = row_off + n * h + pix; col[n, j] = a; j += 1
            row_off += N * h
    return row, col


def rpn_unpack_ref(y, N, A, hw):
    row, col = rpn_index(N, A, hw)
    logits = y[row, col]
    deltas = np.stack([y[row, A + 4 * col + b] for b in range(4)], 2)
    return logits, deltas


def rpn_unpack_bwd_ref(dl, dd, gl, gd, N, A, hw, ld, dtype=np.float32):
    """dy (rows, ld) in `dtype` arithmetic: dlogits * gl and ddeltas * gd at their places (None = zero / 1), 0 in the padding"""
    row, col = rpn_index(N, A, hw)
    dy = np.zeros((rpn_rows(N, hw), ld), dtype)
    if dl is not None:
        dy[row, col] = np.asarray(dl, dtype) * dtype(1.0 if gl is None else gl)
    if dd is not None:
        for b in range(4):
            dy[row, A + 4 * col + b] = np.asarray(dd, dtype)[:, :, b] * dtype(1.0 if gd is None else gd)
    return dy


# ============================================================================================ scale_col_blocks
# (M, N, split, pitch): split at both ends, a padded pitch.  Source and destination are __restrict__ in the kernel and its one
# caller hands it a fresh destination: it is not meant to work in place, so no such case.
SCALE_BLOCK_CASES = [(1, 5, 1, 5), (37, 15, 3, 16), (300, 75, 15, 80), (64, 8, 0, 8), (64, 8, 8, 8)]


def scale_blocks_inputs(M, N, split, pitch):
    r = _rng(81, M, N, split, pitch)
    src = np.full((M, pitch), np.nan, np.float32)
    src[:, :N] = r.normal(0.0, 2.0, (M, N))
    return src, np.float32(r.uniform(0.3, 1.7)), np.float32(r.uniform(0.3, 1.7))


def scale_blocks_ref(src, N, split, g0, g1, dtype=np.float32):
    out = np.zeros(src.shape, dtype)
    out[:, :split] = src[:, :split].astype(dtype) * dtype(g0)
    out[:, split:N] = src[:, split:N].astype(dtype) * dtype(g1)
    return out


# ============================================================================================ tolerance table
def fresh_table():
    """(kind, dtype) -> e32 = max over the cases of max|float32 form - float64| / max|float64|"""
    from oracle import frcnn_oracle as FO
    tab = {}

    def note(kind, dtype, f32, f64):
        tab[(kind, dtype)] = max(tab.get((kind, dtype), 0.0), rel_err(f32, f64))
    for dtype in DTYPES:
        for c in STEM_CASES:
            i = stem_inputs(*c, dtype)
            note("stem", dtype, stem_f32(*i), stem_ref(*i))
        for (h, w, C) in FPN_CASES:
            for N in FPN_N:
                g = dense_inputs(45, (N, 2 * h, 2 * w, C), dtype)
                note("downsample", dtype, downsample_sum_f32(g), downsample_sum_ref(g))
        rois = roi_set()
        for C in ROI_C:
            feat = roi_feat(C, dtype)
            for cfg in ROI_CONFIGS:
                PH, PW, sr = cfg
                note("roi_fwd", dtype, FO.roi_align_fwd(feat.transpose(0, 3, 1, 2), rois, ROI_SCALE, PH, PW, sr), roi_fwd_expected(C, cfg, dtype))
                gout = roi_gout(C, PH, PW, dtype)
                b32 = FO.roi_align_bwd(gout, rois, ROI_SCALE, (ROI_N, C, ROI_H, ROI_W), sr)
                note("roi_bwd", dtype, b32.transpose(0, 2, 3, 1), roi_bwd_expected(C, cfg, dtype))
    for (N, A, hw, ld) in RPN_CASES:
        _, dl, dd, gl, gd = rpn_inputs(N, A, hw, ld)
        note("rpn_scale", "f32", rpn_unpack_bwd_ref(dl, dd, gl, gd, N, A, hw, ld), rpn_unpack_bwd_ref(dl, dd, gl, gd, N, A, hw, ld, np.float64))
    for (M, N, split, pitch) in SCALE_BLOCK_CASES:
        src, g0, g1 = scale_blocks_inputs(M, N, split, pitch)
        src = np.nan_to_num(src)
        note("scale_col_blocks", "f32", scale_blocks_ref(src, N, split, g0, g1), scale_blocks_ref(src, N, split, g0, g1, np.float64))
    return tab


# (kind, input dtype) -> e32, measured by tests/test_detector_ref_cpu.py::test_tolerance_table_is_current (which fails when a bar
# this table gives is off a freshly computed one by more than a factor 2); `python tests/test_detector_ref_cpu.py` prints a fresh one
E32 = {
    ('downsample', 'bf16'): 2.60e-08,
    ('downsample', 'f32'): 8.33e-08,
    ('roi_bwd', 'bf16'): 2.11e-07,
    ('roi_bwd', 'f32'): 3.20e-07,
    ('roi_fwd', 'bf16'): 9.03e-08,
    ('roi_fwd', 'f32'): 1.01e-07,
    ('rpn_scale', 'f32'): 4.23e-08,
    ('scale_col_blocks', 'f32'): 4.78e-08,
    ('stem', 'bf16'): 5.82e-07,
    ('stem', 'f32'): 5.76e-07,
}

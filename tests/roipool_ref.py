"""NumPy restatement of max ROI pooling for the ROIPool tests (tests/test_roipool_ref_cpu.py, tests/test_gpu_roipool_bwd.py,
tests/test_gpu_roipool_fwd.py).

* forward geometry and argmax of ROILoopPool_cpu.cpp:26-79 in float32 (roi_extent / bin_edges / roi_pool_fwd);
* the backward of :98-123 as a float64 scatter-add, with what the error bars need beside it (roi_pool_bwd_ref);
* bwd_plan: a mirror of roi_bwd_dispatch (csrc/roipool.hip) — which kernel a call takes and how it is sized;
* overshoot_heights: the ROI heights whose last bin reaches one row past the ROI's end row;
* bwd_bar: the per-element error bars, derived below, never from a kernel's output;
* fwd_plan: a mirror of the forward's dispatch (sw_roi_pool_fwd, launch_fwd_tasks, roi_fwd_dispatch, launch_fwd_sparse, launch_fwd_plane)
  — which of the six forms a call takes, its channels per lane, band geometry, chunk and zsplit;
* the forward's constructed cases (FwdCase): forms, thresholds, chunks, classes, values, slabs, untouched.

NumPy only: nothing here touches the GPU or the package under test.
"""
from dataclasses import dataclass

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


# ------------------------------------------------------------------------------------------------ forward geometry
def _roundf(x32):
    """C roundf of float32 values (half away from zero), as int64.  x + 0.5 is formed in float64, where it is exact."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def roi_extent(lo, hi, scale):
    """(start, end, extent) of one ROI axis: round(coordinate * scale) in float32, extent = max(end - start + 1, 1)"""
    s = _roundf(np.asarray(lo, F32) * F32(scale))
    e = _roundf(np.asarray(hi, F32) * F32(scale))
    return s, e, np.maximum(e - s + 1, 1)


def bin_edges_unclipped(extent, P):
    """bins of an axis of `extent` pixels relative to its start: [floor(p * bin), ceil((p + 1) * bin)) with bin = extent / P
    and every product rounded to float32 (ROILoopPool_cpu.cpp:38-45).  Returns (starts, ends), each of P ints."""
    b = F32(extent) / F32(P)
    p = np.arange(P, dtype=np.float32)
    s = np.floor((p * b).astype(np.float32)).astype(np.int64)
    e = np.ceil(((p + F32(1)) * b).astype(np.float32)).astype(np.int64)
    return s, e


def bin_edges(start, extent, P, size):
    """the same, moved to the ROI's start and clipped to [0, size]"""
    s, e = bin_edges_unclipped(extent, P)
    return np.clip(s + start, 0, size), np.clip(e + start, 0, size)


def overshoot_heights(P, max_h=255):
    """ROI extents h (in feature pixels) whose last bin ends past h: ceil(float32(P) * float32(h / P)) > h, so the bin takes
    in the row after the ROI's end row.  Computed from the float32 arithmetic, not listed."""
    out = []
    for h in range(1, max_h + 1):
        _, e = bin_edges_unclipped(h, P)
        if int(e[-1]) > h:
            out.append(h)
    return out


def roi_pool_fwd(feat, rois, scale, PH=7, PW=7):
    """feat (N, C, H, W) float32, rois (R, 5) float32 -> out (R, C, PH, PW) float32, argmax int32 (h * W + w, or -1).
    Strict '>' from -FLT_MAX, first maximum in row-major order; an empty bin gives 0 / -1."""
    feat = np.asarray(feat, np.float32)
    rois = np.asarray(rois, np.float32)
    _, C, H, W = feat.shape
    R = rois.shape[0]
    out = np.zeros((R, C, PH, PW), np.float32)
    arg = np.full((R, C, PH, PW), -1, np.int32)
    sw, _, ew = roi_extent(rois[:, 1], rois[:, 3], scale)
    sh, _, eh = roi_extent(rois[:, 2], rois[:, 4], scale)
    for r in range(R):
        img = int(rois[r, 0])
        hs, he = bin_edges(int(sh[r]), int(eh[r]), PH, H)
        ws, we = bin_edges(int(sw[r]), int(ew[r]), PW, W)
        for ph in range(PH):
            for pw in range(PW):
                h0, h1, w0, w1 = int(hs[ph]), int(he[ph]), int(ws[pw]), int(we[pw])
                if h1 <= h0 or w1 <= w0:
                    continue                                               # empty: 0 / -1
                win = feat[img, :, h0:h1, w0:w1].reshape(C, -1)
                ok = win > -FLT_MAX                                        # what can beat the start value; NaN cannot
                k = np.argmax(np.where(ok, win, -np.inf), axis=1)          # first maximum, row-major
                won = ok.any(axis=1)
                pix = (h0 + k // (w1 - w0)) * W + (w0 + k % (w1 - w0))
                out[r, :, ph, pw] = np.where(won, win[np.arange(C), k], -FLT_MAX)
                arg[r, :, ph, pw] = np.where(won, pix, -1)
    return out, arg


# ------------------------------------------------------------------------------------------------ backward, float64
@dataclass
class BwdRef:
    ref: np.ndarray      # (nimg, H, W, C) float64: the exact sum of the terms, masked by relu_ref > 0
    n: np.ndarray        # terms per element
    S: np.ndarray        # sum of |term| per element
    tmax: np.ndarray     # largest |term| per element


def row_multiplier(row_scale, add, R):
    """float32(row_scale[r] + add) as the kernels form it; 1 without a row scale"""
    if row_scale is None:
        return np.ones(R, np.float32)
    return (np.asarray(row_scale, np.float32) + F32(add)).astype(np.float32)


def roi_pool_bwd_ref(dout, argmax, rois, shape, row_scale=None, add=0.0, relu_ref=None):
    """dout (R, C, nb) — the values the kernel reads, already rounded to its type —, argmax (R, C, nb) int (pixel or < 0),
    shape = (nimg, H, W, C), relu_ref (nimg, H, W, C) or None.
    ref[img, p, c] = sum over (r, c, bin) with argmax == p of float64(dout) * float64(float32(row_scale[r] + add))."""
    nimg, H, W, C = shape
    R = dout.shape[0]
    mul = row_multiplier(row_scale, add, R).astype(np.float64)
    img = np.asarray(rois, np.float32)[:, 0].astype(np.int64)
    a = np.asarray(argmax).astype(np.int64)
    ok = a >= 0
    term = (np.asarray(dout).astype(np.float64) * mul[:, None, None])[ok]
    idx = ((img[:, None, None] * (H * W) + a) * C + np.arange(C, dtype=np.int64)[None, :, None])[ok]
    N = nimg * H * W * C
    with np.errstate(invalid="ignore"):
        ref = np.bincount(idx, weights=term, minlength=N)
        at = np.abs(term)
        S = np.bincount(idx, weights=at, minlength=N)
    n = np.bincount(idx, minlength=N)
    tmax = np.zeros(N)
    if at.size and at.min() == at.max():
        tmax[idx] = at[0]
    else:
        order = np.argsort(at, kind="stable")       # NaN last: a repeated index keeps its LAST assignment, the largest
        tmax[idx[order]] = at[order]
    if relu_ref is not None:
        keep = np.asarray(relu_ref, np.float64).reshape(-1) > 0          # NaN, -0.0 and negatives all mask
        ref = np.where(keep, ref, 0.0)
    s4 = (nimg, H, W, C)
    return BwdRef(ref.reshape(s4), n.reshape(s4), S.reshape(s4), tmax.reshape(s4))


# ------------------------------------------------------------------------------------------------ dispatch mirror
FX_CHUNK = 1024
ACC_BUDGET = 150 * 1024


@dataclass
class BwdPlan:
    path: str            # "fx", "float" or "refused"
    accmode: int = -1    # fx: 0 = one 64-bit word, 2 = hi / lo pair of 32-bit words
    CB: int = 0          # channels per slab
    nsplit: int = 1      # pixel ranges per plane
    px_per: int = 0      # pixels per range
    nb: int = 0

    def bits(self, n_img):
        """(term_bits, lo_bits) of the fx kernel for an image with n_img ROIs"""
        if self.accmode == 0:
            return 40, 41
        terms = max(self.nb * max(n_img, 1), 1)
        tb = max(30 - terms.bit_length(), 1)
        return tb, tb + 1


def bwd_plan(dtype, argmax_bits, nimg, H, W, C, PH, PW, R, ld, has_absmax, aligned):
    """Mirror of sw_roi_pool_bwd / roi_bwd_dispatch.  dtype "bf16" or "f32"; ld = row pitch in elements (0 = dense);
    aligned = dout 8-byte and argmax 16-byte aligned."""
    nb = PH * PW
    ld = ld if ld > 0 else C * nb
    if ld < C * nb or dtype not in ("bf16", "f32") or argmax_bits not in (16, 32):
        return BwdPlan("refused")
    small_terms = dtype == "bf16" and R > 0 and nb * R < (1 << 30) and 30 - (nb * R).bit_length() >= 8
    accmode = 2 if small_terms else 0
    cbx = 8
    while cbx > 4 and (H * W * cbx * 8 > ACC_BUDGET or C % cbx or (C // cbx) * nimg < 256):
        cbx >>= 1
    if C % cbx:
        cbx = 0
    nsplit = -(-(H * W * cbx * 8) // ACC_BUDGET) if cbx else 1
    if cbx >= 4 and nsplit <= 16 and has_absmax and aligned and ld % 4 == 0:
        return BwdPlan("fx", accmode, cbx, nsplit, -(-(H * W) // nsplit), nb)
    CB = 64
    while CB > 1 and (H * W * CB * 4 > 64 * 1024 or C % CB or (C // CB) * nimg < 512):
        CB >>= 1
    if H * W * CB * 4 > 160 * 1024:
        return BwdPlan("refused")
    return BwdPlan("float", -1, CB, 1, H * W, nb)


def pixel_ranges(plan, H, W):
    """[p0, p1) of every range of an fx plan"""
    return [(z * plan.px_per, min(H * W, (z + 1) * plan.px_per)) for z in range(plan.nsplit)]


# ------------------------------------------------------------------------------------------------ error bars
def half_ulp(x, dtype):
    """half a unit in the last place of the output type at |x| (the smallest subnormal's at 0)"""
    mant, emin = (7, -126) if dtype == "bf16" else (23, -126)
    ax = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    e = np.where(ax > 0, np.maximum(e, emin), emin)
    return np.ldexp(0.5, (e - mant).astype(np.int64))


def fx_frac(absmax, smax, term_bits):
    """the fx kernel's scaling exponent: bound = float32(absmax * smax), frac = term_bits - (ilogb(bound) + 1); 0 at bound 0"""
    bound = F32(absmax) * F32(smax)
    if not bound > 0:
        return 0
    return term_bits - (int(np.floor(np.log2(np.float64(bound)))) + 1)


def bwd_bar(plan, br, dtype, absmax=None, smax=None, n_img=None):
    """Per-element bound on |kernel - br.ref|.

    Every path forms a term as the float32 product dout * mul, which differs from the exact product by at most |term| * 2^-24:
    S * 2^-24 over an element's terms.  (S >= |ref|, so this term also covers the float32 value the fx kernel forms from its
    integer sum before it rounds to the output type.)
      fx, mode 0: a term is rounded once to a multiple of 2^-frac: at most 2^-(frac + 1) each, n * 2^-(frac + 1); integer sums
                  are exact.
      fx, mode 2: hi = rint(t * 2^frac) is exact in the hi word; the remainder is rounded to a multiple of 2^-(frac + lo_bits):
                  n * 2^-(frac + lo_bits + 1).
      float path: n float32 additions in any order, each off by at most 2^-24 of a partial sum <= S: S * 2^-24 * n, plus the
                  products' S * 2^-24.
    All paths then round once to the output type: half an ulp at |ref|.
    absmax, smax: max |dout| and max |row multiplier| as the kernel sees them (fx only); n_img: ROIs of each image (fx, mode 2).
    """
    eps = 2.0 ** -24
    hu = half_ulp(br.ref, dtype)
    if plan.path == "float":
        return br.S * eps * (br.n + 1) + hu
    assert plan.path == "fx"
    bar = np.empty_like(br.ref)
    for i in range(br.ref.shape[0]):
        tb, lb = plan.bits(int(n_img[i]) if n_img is not None else 0)
        frac = fx_frac(absmax, smax, tb)
        q = np.ldexp(1.0, -(frac + 1)) if plan.accmode == 0 else np.ldexp(1.0, -(frac + lb + 1))
        bar[i] = br.S[i] * eps + br.n[i] * q + hu[i]
    return bar


# ------------------------------------------------------------------------------------------------ constructed cases
def round_bf16(x):
    """float32 values rounded to bfloat16 (nearest even), kept as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def round_to(x, dtype):
    return round_bf16(x) if dtype == "bf16" else np.asarray(x, np.float32)


@dataclass
class Case:
    """One call of the backward: what the kernel reads, and the plan it must take."""
    name: str
    dtype: str                      # "bf16" / "f32"
    argmax_bits: int
    shape: tuple                    # (nimg, H, W, C)
    PH: int
    PW: int
    rois: np.ndarray                # (R, 5) float32
    argmax: np.ndarray              # (R, C, nb) int32: pixel, or -1
    dout: np.ndarray                # (R, C, nb) float32, representable in dtype
    path: str                       # the plan the case is built for
    CB: int
    nsplit: int = 1
    accmode: int = -1
    row_scale: np.ndarray = None
    add: float = 0.0
    relu_ref: np.ndarray = None     # (nimg, H, W, C) float32
    scale: float = 0.0              # the forward's scale where argmax comes from the forward's geometry, else 0
    pad: int = 0                    # pitch - C * nb, in elements
    has_absmax: bool = True
    offset: int = 0                 # dout starts this many elements into its allocation

    @property
    def R(self):
        return self.rois.shape[0]

    def plan(self):
        nimg, H, W, C = self.shape
        return bwd_plan(self.dtype, self.argmax_bits, nimg, H, W, C, self.PH, self.PW, self.R, C * self.PH * self.PW + self.pad,
                        self.has_absmax, self.offset == 0)

    def reference(self):
        return roi_pool_bwd_ref(self.dout, self.argmax, self.rois, self.shape, self.row_scale, self.add, self.relu_ref)

    def n_img(self):
        return np.bincount(self.rois[:, 0].astype(np.int64), minlength=self.shape[0])

    def bar(self, br):
        mul = row_multiplier(self.row_scale, self.add, self.R)
        return bwd_bar(self.plan(), br, self.dtype, np.abs(self.dout).max() if self.dout.size else 0.0,
                       np.abs(mul).max() if mul.size else 0.0, self.n_img())


def _rois_from_boxes(img, boxes):
    return np.concatenate([np.asarray(img, np.float32)[:, None], np.asarray(boxes, np.float32)], 1).astype(np.float32)


def _grad(rng, shape, dtype):
    return round_to(rng.standard_normal(shape).astype(np.float32), dtype)


def row_ramp(nimg, C, H, W):
    """a map that grows with the row and is flat along it: every bin's argmax is the first pixel of its LAST row"""
    return np.broadcast_to(np.arange(H, dtype=np.float32)[None, None, :, None], (nimg, C, H, W)).copy()


# group 1: ROIs whose last bin reaches the row after their end row, on maps whose second pixel range starts at that row
OVERSHOOT_MAPS = {                       # name: (H, W, rs, re, (x1, x2) feature columns of the ROIs)
    "120x64_h57": (120, 64, 3, 59, [(0, 63), (5, 40), (33, 34)]),
    "240x32_h114": (240, 32, 6, 119, [(0, 31), (3, 20)]),
    "240x32_h121": (240, 32, -1, 119, [(0, 31), (10, 30)]),
    "75x100_h57": (75, 100, -20, 36, [(0, 99), (50, 99), (60, 80), (2, 45)]),
}


def overshoot_case(name, dtype, argmax_bits):
    H, W, rs, re, cols = OVERSHOOT_MAPS[name]
    rng = np.random.default_rng(11)
    boxes = [[8.0 * x1, 8.0 * rs, 8.0 * x2, 8.0 * re] for x1, x2 in cols]
    boxes += [[8.0, 8.0, 8.0 * (W - 2), 8.0 * (H - 2)], [16.0, 8.0 * (H // 2 + 3), 8.0 * (W // 2), 8.0 * (H - 1)]]   # ordinary company
    rois = _rois_from_boxes(np.zeros(len(boxes)), boxes)
    _, arg = roi_pool_fwd(row_ramp(1, 4, H, W), rois, 1.0 / 8, 7, 7)
    return Case(f"overshoot_{name}", dtype, argmax_bits, (1, H, W, 4), 7, 7, rois, arg.reshape(len(boxes), 4, 49),
                _grad(rng, (len(boxes), 4, 49), dtype), "fx", 4, 2, 2 if dtype == "bf16" else 0, scale=1.0 / 8)


# group 2: synthetic argmax on both sides of every range boundary
RANGE_MAPS = {1: (60, 80), 2: (61, 79), 5: (139, 139), 16: (240, 301)}


def range_edge_case(nsplit, dtype):
    H, W = RANGE_MAPS[nsplit]
    nimg, C, PH, PW = 2, 4, 2, 2
    plan = bwd_plan(dtype, 32, nimg, H, W, C, PH, PW, 8, 0, True, True)
    tgt = sorted({p for p0, p1 in pixel_ranges(plan, H, W) for p in (p0 - 1, p0, p1 - 1) if 0 <= p < H * W} | {H * W - 1})
    nT = len(tgt)
    R = 2 * nT
    rng = np.random.default_rng(20 + nsplit)
    r, c, b = np.meshgrid(np.arange(R), np.arange(C), np.arange(4), indexing="ij")
    arg = np.asarray(tgt, np.int32)[(r + 7 * b + c) % nT]
    arg[rng.random(arg.shape) < 0.1] = -1
    rois = _rois_from_boxes(np.arange(R) % nimg, np.zeros((R, 4)))
    return Case(f"ranges_{nsplit}", dtype, 32, (nimg, H, W, C), PH, PW, rois, arg, _grad(rng, (R, C, 4), dtype), "fx", 4, nsplit,
                2 if dtype == "bf16" else 0)


# group 3: pooled sizes, argmax from the forward on a small map
POOLED = [(1, 1), (1, 2), (1, 3), (2, 2), (3, 3), (7, 7), (14, 14)]


def pooled_case(PH, PW, dtype, C, has_absmax=True):
    nimg = 2 if C >= 1024 else 1
    H = W = 6
    R = 12
    rng = np.random.default_rng(PH * 100 + PW + C)
    feat = round_to(rng.standard_normal((nimg, C, H, W)).astype(np.float32), dtype)
    x1 = rng.uniform(-8, 40, R); y1 = rng.uniform(-8, 40, R)
    boxes = np.stack([x1, y1, x1 + rng.uniform(0, 40, R), y1 + rng.uniform(0, 40, R)], 1)
    rois = _rois_from_boxes(np.arange(R) % nimg, boxes)
    _, arg = roi_pool_fwd(feat, rois, 1.0 / 8, PH, PW)
    nb = PH * PW
    if dtype == "f32":                                                       # every channel its own gradient, exactly
        dout = (np.arange(C, dtype=np.float32)[None, :, None] + 1 + np.arange(R, dtype=np.float32)[:, None, None] / 16
                + np.arange(nb, dtype=np.float32)[None, None, :] / 1024) * np.where(np.arange(C) % 2, -1, 1)[None, :, None]
        dout = dout.astype(np.float32)
    else:
        dout = _grad(rng, (R, C, nb), dtype)
    if not has_absmax:
        CB = 4 if C >= 1024 else 1
        return Case(f"pooled_{PH}x{PW}_C{C}_float", dtype, 16, (nimg, H, W, C), PH, PW, rois, arg.reshape(R, C, nb), dout, "float", CB,
                    scale=1.0 / 8, has_absmax=False)
    return Case(f"pooled_{PH}x{PW}_C{C}", dtype, 16, (nimg, H, W, C), PH, PW, rois, arg.reshape(R, C, nb), dout, "fx",
                8 if C >= 1024 else 4, 1, 2 if dtype == "bf16" else 0, scale=1.0 / 8)


def _synthetic(rng, R, nimg, img, H, W, C, nb, none=0.1):
    arg = rng.integers(0, H * W, (R, C, nb)).astype(np.int32)
    arg[rng.random(arg.shape) < none] = -1
    return _rois_from_boxes(img, np.zeros((R, 4))), arg


# group 4: ROI counts around the compaction chunk (1024) and the 8-ROI step; image 2 of 4 has no ROI
CHUNK_R = [1, 7, 8, 9, 1023, 1024, 1025, 2049]


def chunk_case(R, relu, dtype="bf16"):
    nimg, H, W, C = 4, 8, 8, 4
    rng = np.random.default_rng(400 + R)
    img = rng.choice([0, 1, 3], size=R, p=[0.6, 0.3, 0.1])
    rois, arg = _synthetic(rng, R, nimg, img, H, W, C, 4)
    relu_ref = rng.standard_normal((nimg, H, W, C)).astype(np.float32) if relu else None
    return Case(f"chunk_R{R}_relu{int(relu)}", dtype, 16, (nimg, H, W, C), 2, 2, rois, arg, _grad(rng, (R, C, 4), dtype), "fx", 4, 1,
                2 if dtype == "bf16" else 0, relu_ref=relu_ref)


# group 5: every bin of every ROI on ONE pixel of every channel, every term +absmax
def pile_case(P, R, absmax, dtype="bf16"):
    C, H, W = 4, 4, 4
    nb = P * P
    rois = _rois_from_boxes(np.zeros(R), np.zeros((R, 4)))
    arg = np.full((R, C, nb), 5, np.int32)
    dout = np.full((R, C, nb), absmax, np.float32)
    assert np.array_equal(round_to(dout, dtype), dout)
    mode = 2 if dtype == "bf16" and 30 - (nb * R).bit_length() >= 8 else 0
    return Case(f"pile_{P}x{P}_R{R}_{absmax!r}_{dtype}", dtype, 16, (1, H, W, C), P, P, rois, arg, dout, "fx", 4, 1, mode)


def lognormal_case(dtype="bf16"):
    """magnitudes over many decades (log-normal, sigma 3), half the rows scaled by 1e-6, objectness-like row scales"""
    nimg, H, W, C, R = 2, 10, 12, 4, 600
    rng = np.random.default_rng(55)
    rois, arg = _synthetic(rng, R, nimg, np.arange(R) % nimg, H, W, C, 49, none=0.3)
    g = np.exp(3.0 * rng.standard_normal((R, C, 49))) * np.sign(rng.standard_normal((R, C, 49)))
    g *= np.where(rng.random(R) < 0.5, 1e-6, 1.0)[:, None, None]
    return Case("lognormal", dtype, 16, (nimg, H, W, C), 7, 7, rois, arg, round_to(g.astype(np.float32), dtype), "fx", 4, 1,
                2 if dtype == "bf16" else 0, row_scale=rng.random(R).astype(np.float32), add=1.0)


# group 6: row scales and ReLU masks
def scale_case(kind, dtype):
    nimg, H, W, C, R = 2, 8, 8, 4, 64
    rng = np.random.default_rng(60 + len(kind))
    rois, arg = _synthetic(rng, R, nimg, np.arange(R) % nimg, H, W, C, 9)
    add = 0.0
    if kind == "negative":
        rs = -rng.random(R).astype(np.float32) * 3
    elif kind == "decades":
        rs = (10.0 ** rng.uniform(-30, 0, R) * np.sign(rng.standard_normal(R))).astype(np.float32)
    else:                                                                   # "zero": row_scale + add == 0 on every row: bound 0
        rs, add = np.full(R, -1.0, np.float32), 1.0
    relu = rng.standard_normal((nimg, H, W, C)).astype(np.float32)
    relu.reshape(-1)[::7] = np.nan
    relu.reshape(-1)[1::7] = -0.0
    relu.reshape(-1)[2::7] = 0.0
    return Case(f"scale_{kind}", dtype, 16, (nimg, H, W, C), 3, 3, rois, arg, _grad(rng, (R, C, 9), dtype), "fx", 4, 1,
                2 if dtype == "bf16" else 0, row_scale=rs, add=add, relu_ref=round_to(relu, dtype))


# group 7: non-finite inputs; the poisoned ROI is row 3 and belongs to image 0
POISONS = ["dout_nan", "dout_inf", "scale_inf", "scale_nan"]


def poison_case(kind, dtype, has_absmax):
    nimg, H, W, C, R = 2, 8, 8, 4, 40
    rng = np.random.default_rng(70)
    rois, arg = _synthetic(rng, R, nimg, np.arange(R) % nimg, H, W, C, 9)
    rois[3, 0] = 0
    arg[3, 1, 4] = 17                                                       # the poisoned term does reach a pixel
    dout = _grad(rng, (R, C, 9), dtype)
    rs = rng.random(R).astype(np.float32)
    if kind == "dout_nan":
        dout[3, 1, 4] = np.nan
    elif kind == "dout_inf":
        dout[3, 1, 4] = np.inf
    elif kind == "scale_inf":
        rs[3] = np.inf
    else:
        rs[3] = np.nan
    return Case(f"poison_{kind}", dtype, 16, (nimg, H, W, C), 3, 3, rois, arg, dout, "fx" if has_absmax else "float",
                4 if has_absmax else 1, 1, (2 if dtype == "bf16" else 0) if has_absmax else -1, row_scale=rs, add=1.0,
                has_absmax=has_absmax)


# groups 8 and 9: what sends a call to the float atomics, and pitch gaps on either path
FALLBACKS = ["no_absmax", "pitch", "C6", "C2", "offset"]


def fallback_case(kind, dtype):
    nimg, H, W, R = 2, 9, 11, 40
    C = {"C6": 6, "C2": 2}.get(kind, 4)
    rng = np.random.default_rng(80)
    rois, arg = _synthetic(rng, R, nimg, np.arange(R) % nimg, H, W, C, 9)
    return Case(f"fallback_{kind}", dtype, 16, (nimg, H, W, C), 3, 3, rois, arg, _grad(rng, (R, C, 9), dtype), "float", 1,
                row_scale=rng.random(R).astype(np.float32), add=1.0, has_absmax=kind != "no_absmax", pad=2 if kind == "pitch" else 0,
                offset=1 if kind == "offset" else 0)


def gap_case(dtype, argmax_bits, path):
    nimg, H, W, C, R = 2, 9, 11, 4, 40
    rng = np.random.default_rng(90)
    rois, arg = _synthetic(rng, R, nimg, np.arange(R) % nimg, H, W, C, 9)
    fx = path == "fx"
    return Case(f"gaps_{path}", dtype, argmax_bits, (nimg, H, W, C), 3, 3, rois, arg, _grad(rng, (R, C, 9), dtype), path, 4 if fx else 1, 1,
                (2 if dtype == "bf16" else 0) if fx else -1, pad=8 if fx else 6)


# ================================================================================================ forward: dispatch mirror
# The constants of csrc/roipool.hip.  The workgroup targets of the two zsplit rules (256; 768 / 2048) are what the library assumes
# of the chip — one workgroup per CU of a 256-CU part, a few rounds of it — and are taken from there, never from a device query.
SP_NT, SP_CH, SP_NLEV, SP_NHC = 1024, 128, 6, 7
SP_NCLS = SP_NLEV * SP_NHC
TK_MAXB, TK_SEG, TK_PREP_NT = 16, SP_NCLS + 1, 256
PLANE_NT, PLANE_CHUNK = 1024, 256
ROIGEO_BYTES = 48
LDS_CU = 160 * 1024
PLANE_BUDGET = 150 * 1024
PLANE_LDS_MAX = LDS_CU - 256         # beside the plane kernel's 208 bytes of static LDS
SPARSE_LDS_MAX = LDS_CU - 1536
TASKS_LDS_ALL = LDS_CU - 1024
GATHER_LDS_MAX = 64 * 1024
SPARSE_WG_TARGET = 256
PLANE_WG_TARGETS = (768, 2048)            # LDS above / up to 80 KiB per workgroup
FORMS = ("tasks", "sparse_whole", "sparse_band", "plane_band", "plane", "gather")


def _up(x, a):
    return (x + a - 1) // a * a


def plane_lds_bytes(rows, W, pxb, chunk, PH, PW, band):
    """PlaneLds::bytes"""
    o = _up(rows * W * pxb, 16)
    o += chunk * 4 + chunk * PH * 2 + chunk * PW * 2
    o += 4 + chunk * 4                     # (mul is aligned up inside these 4 bytes)
    if band:
        o += chunk * PH * 4
    return o


def sparse_lds_bytes(table_bytes, R, chunk, PH, PW, band):
    """SparseLds::bytes"""
    o = table_bytes + ((R + 1) & ~1) * 2 + chunk * 4 + chunk * 4 + chunk * PH * 2 + chunk * PW * 2 + 4
    if band:
        o += chunk * PH * 4
    return o + 16


def tasks_lds_bytes(rows, W, PW, n_waves=16):
    """TasksLds::bytes"""
    n_rec = (62 + PW) // PW + 1
    return _up(rows * W * 16, 16) + n_waves * 2 * n_rec * 32


def fwd_workspace_bytes(nimg, R, PH, PW):
    """sw_roi_pool_fwd_workspace_bytes"""
    if nimg <= 0 or R <= 0 or PH <= 0 or PW <= 0:
        return 0
    seg = _up(nimg * TK_MAXB * TK_SEG * 4, 256)
    geo = _up(R * ROIGEO_BYTES, 256)
    hist = _up(-(-R // TK_PREP_NT) * nimg * TK_MAXB * SP_NCLS * 4, 256)
    return seg + geo + hist + nimg * R * PH * 32


@dataclass(frozen=True)
class BandRule:
    min_own: int
    equal_bands: bool
    clamp_last: bool
    whole_if_fits: bool


PLANE_BANDS = BandRule(8, False, False, False)
SPARSE_BANDS = BandRule(8, False, False, True)
TASK_BANDS = BandRule(4, True, True, True)


def band_geometry(H, PH, fit, rule):
    """band_geometry: (S, rows, n_bands) or None where the form declines"""
    if rule.whole_if_fits and fit >= H:
        return H, H, 1
    halo = -(-H // PH) + 1
    if fit - halo < rule.min_own:
        return None
    S = fit - halo
    if rule.equal_bands:
        n = -(-H // S)
        S = -(-H // n)
    return S, fit, -(-H // S)


def band_owner(first_row, S, n_bands):
    """BandGeom::owner"""
    return min(first_row // S, n_bands - 1)


def band_y0(band, S, rows, H, clamp_last):
    """BandGeom::y0"""
    y, top = band * S, max(H - rows, 0)
    return top if clamp_last and y > top else y


@dataclass
class FwdPlan:
    form: str            # one of FORMS, "refused", or "none" (R <= 0: the entry returns 0 before it decides anything)
    code: int = 0        # the refusal code
    CB: int = 0          # channels per lane
    S: int = 0           # rows a band owns (whole-map forms: H)
    rows: int = 0        # rows a band holds
    n_bands: int = 1
    chunk: int = 0       # ROIs per chunk (tasks: none; gather: one ROI per workgroup)
    nz: int = 1          # workgroups per (slab, image, band)
    n_chunks: int = 0    # what nz is capped at (tasks: not capped)
    clamp_last: bool = False
    lds: int = 0
    key: bool = False    # packed-key scan (every bf16 form but the gather one)
    kernels: tuple = ()  # the roi_pool_* kernels a kernel trace of the call shows (compared once per form; see test_gpu_roipool_fwd.py)


def _fwd_zsplit(wg_per_z, n_chunks, lds):
    """fwd_zsplit (plane forms)"""
    target = PLANE_WG_TARGETS[0] if lds > 80 * 1024 else PLANE_WG_TARGETS[1]
    return min(max(-(-target // wg_per_z), 1), n_chunks)


def _sparse_zsplit(wg_per_z, n_blocks):
    """launch_fwd_sparse's zsplit"""
    return min(max((SPARSE_WG_TARGET + wg_per_z // 2) // wg_per_z, 1), n_blocks)


def _plan_tasks(nimg, H, W, C, PH, PW, R):
    """launch_fwd_tasks: a plan, or None for its -100"""
    if PW < 3:
        return None
    ring = tasks_lds_bytes(0, W, PW)
    # (H * W <= 5 * 1024 cannot be false once the first inequality holds: H * W * 32 <= TASKS_LDS_ALL gives H * W <= 5088)
    if H * W * 32 + ring <= TASKS_LDS_ALL and H * W <= 5 * 1024:
        return None
    fit = (TASKS_LDS_ALL - ring) // (W * 16)
    if fit * W > 10 * 1024:
        fit = 10 * 1024 // W
    bg = band_geometry(H, PH, fit, TASK_BANDS)
    if bg is None or bg[2] > TK_MAXB:
        return None
    if nimg * bg[2] > 64:
        return None
    slabs = (C // 4) * nimg * bg[2]
    nz = max((SPARSE_WG_TARGET + slabs // 2) // slabs, 1)
    # (n_bands * nz > 65535 cannot hold: n_bands <= TK_MAXB and nz <= 256)
    return FwdPlan("tasks", 0, 4, bg[0], bg[1], bg[2], 0, nz, 0, True, tasks_lds_bytes(bg[1], W, PW), True,
                   ("roi_pool_geo_kernel", "roi_pool_tasks_kernel", "roi_pool_fwd_tasks_kernel"))


def _plan_sparse(nimg, H, W, C, PH, PW, R):
    """launch_fwd_sparse: a plan, or None for its -100"""
    n_blocks = (R + 127) // 128
    plane8 = sparse_lds_bytes(H * W * 32, R, SP_CH, PH, PW, False)
    # (H * W <= 5 * SP_NT cannot be false once plane8 fits: H * W * 32 <= SPARSE_LDS_MAX gives H * W <= 5072)
    if plane8 <= SPARSE_LDS_MAX and H * W <= 5 * SP_NT:
        return FwdPlan("sparse_whole", 0, 8, H, H, 1, SP_CH, _sparse_zsplit((C // 8) * nimg, n_blocks), n_blocks, False, plane8, True,
                       ("roi_pool_fwd_sparse_kernel",))
    tb = sparse_lds_bytes(0, R, SP_CH, PH, PW, True)
    # (PH > 255 cannot hold: the caller admits PH <= 8.  tb + W * 16 * 8 > SPARSE_LDS_MAX cannot hold either: R <= 16384, PH, PW <= 8
    #  and W <= 255 give tb <= 42004 and W * 128 <= 32640)
    if PH > 255 or tb + W * 16 * 8 > SPARSE_LDS_MAX:
        return None
    fit = (SPARSE_LDS_MAX - tb) // (W * 16)
    if fit * W > 10 * SP_NT:
        fit = 10 * SP_NT // W
    bg = band_geometry(H, PH, fit, SPARSE_BANDS)
    if bg is None:
        return None
    nz = _sparse_zsplit((C // 4) * nimg * bg[2], n_blocks)
    # (n_bands * nz > 65535 cannot hold: n_bands <= 255 / 8 and nz <= 256)
    return FwdPlan("sparse_band", 0, 4, bg[0], bg[1], bg[2], SP_CH, nz, n_blocks, False,
                   sparse_lds_bytes(bg[1] * W * 16, R, SP_CH, PH, PW, True), True, ("roi_pool_fwd_sparse_kernel",))


def plane_band_geometry(H, W, PH, PW):
    """plane_band_geometry: None where the form declines (tables of a tall pooled size that leave no LDS for a band included)"""
    budget = LDS_CU - 1024 - plane_lds_bytes(0, W, 16, PLANE_CHUNK, PH, PW, True)
    return band_geometry(H, PH, budget // (W * 16), PLANE_BANDS) if PH <= 255 and budget > 0 else None


def _plan_plane(dtype, nimg, H, W, C, PH, PW, R, CB, bg, band):
    """launch_fwd_plane"""
    es = 2 if dtype == "bf16" else 4
    lds = plane_lds_bytes(bg[1], W, CB * es, PLANE_CHUNK, PH, PW, band)
    n_chunks = -(-R // PLANE_CHUNK)
    nz = _fwd_zsplit((C // CB) * nimg * bg[2], n_chunks, lds)
    # (n_bands * nz > 65535 cannot hold: n_bands <= 32 and nz <= ceil(2048 / n_bands))
    return FwdPlan("plane_band" if band else "plane", 0, CB, bg[0], bg[1], bg[2], PLANE_CHUNK, nz, n_chunks, False, lds,
                   dtype == "bf16" and H * W < 65535, ("roi_pool_fwd_plane_kernel",))


def fwd_plan(dtype, argmax_bits, nimg, H, W, C, PH, PW, R, ld, feat_aligned16, workspace):
    """Mirror of sw_roi_pool_fwd / launch_fwd_tasks / roi_fwd_dispatch / launch_fwd_sparse / launch_fwd_plane.
    dtype "bf16" or "f32"; ld = row pitch in elements (0 = dense); workspace: None, "auto" (aligned and large enough) or
    (bytes, 16-byte aligned)."""
    if R <= 0:
        return FwdPlan("none")
    nb = PH * PW
    ld = ld if ld > 0 else C * nb
    if ld < C * nb:
        return FwdPlan("refused", -5)
    if dtype not in ("bf16", "f32"):
        return FwdPlan("refused", -1)
    es = 2 if dtype == "bf16" else 4
    tasks_shape_ok = (dtype == "bf16" and nimg > 0 and C % 8 == 0 and H * W < 65535 and H <= 255 and W <= 255 and R <= 65535 and PH <= 8
                      and PW <= 8 and feat_aligned16)
    if workspace is not None and argmax_bits in (16, 32) and tasks_shape_ok:
        ws_bytes, ws_aligned = (fwd_workspace_bytes(nimg, R, PH, PW), True) if isinstance(workspace, str) else workspace
        if not ws_aligned or ws_bytes < fwd_workspace_bytes(nimg, R, PH, PW):
            return FwdPlan("refused", -5)
        p = _plan_tasks(nimg, H, W, C, PH, PW, R)
        if p is not None:
            return p
    if argmax_bits != 32:
        if argmax_bits != 16:
            return FwdPlan("refused", -1)
        if H * W >= 65535:
            return FwdPlan("refused", -6)
    # roi_fwd_dispatch
    if nimg > 0 and feat_aligned16 and H <= 255 and W <= 255:
        pxb = 0
        for cand in (16, 8, 4):
            if C % (cand // es) == 0 and H * W * cand <= PLANE_BUDGET and plane_lds_bytes(H, W, cand, PLANE_CHUNK, PH, PW, False) <= PLANE_LDS_MAX:
                pxb = cand
                break
        if dtype == "bf16" and C % 8 == 0 and H * W < 65535 and R <= 16384 and PH <= 8 and PW <= 8:
            p = _plan_sparse(nimg, H, W, C, PH, PW, R)
            if p is not None:
                return p
        if dtype == "bf16" and pxb < 16 and C % 8 == 0 and H * W < 65535:
            bg = plane_band_geometry(H, W, PH, PW)
            if bg is not None:
                return _plan_plane(dtype, nimg, H, W, C, PH, PW, R, 8, bg, True)
        if pxb:
            return _plan_plane(dtype, nimg, H, W, C, PH, PW, R, pxb // es, (H, H, 1), False)
    vec = 2 if dtype == "bf16" else 1
    if C % vec:
        return FwdPlan("refused", -5)
    lds = 64 * vec * nb * (4 + es)
    if lds > GATHER_LDS_MAX:
        return FwdPlan("refused", -6)
    return FwdPlan("gather", 0, vec, H, H, 1, 1, 1, R, False, lds, False, ("roi_pool_fwd_kernel",))


# ================================================================================================ forward: classes, in NumPy
def np_bin_size_class(b):
    """bin_size_class of float32 bin extents"""
    return np.searchsorted(np.asarray([1, 2, 3, 4, 6, 8], np.float32), np.asarray(b, np.float32), side="right")


def np_roi_classes(rois, scale, PH, PW):
    """(level, height class, width class, narrowest unclipped bin width) of every ROI, as roi_level_class / bin_size_class see them"""
    rois = np.asarray(rois, np.float32)
    _, _, ew = roi_extent(rois[:, 1], rois[:, 3], scale)
    _, _, eh = roi_extent(rois[:, 2], rois[:, 4], scale)
    narrow = np.empty(len(rois), np.int64)
    for i, e in enumerate(ew):
        s, t = bin_edges_unclipped(int(e), PW)
        narrow[i] = max(int((t - s).min()), 1)
    level = np.minimum(np.floor(np.log2(narrow)).astype(np.int64), SP_NLEV - 1)
    return (level, np_bin_size_class(eh.astype(np.float32) / F32(PH)), np_bin_size_class(ew.astype(np.float32) / F32(PW)), narrow)


# ================================================================================================ forward: constructed cases
SCALE = 1.0 / 8


def px_box(x0, y0, w, h):
    """image coordinates of the ROI that starts at feature pixel (x0, y0) and is w x h feature pixels (scale 1 / 8: exact)"""
    return [8.0 * x0, 8.0 * y0, 8.0 * (x0 + w - 1), 8.0 * (y0 + h - 1)]


@dataclass
class FwdCase:
    """One call of the forward and the form it is built to take."""
    name: str
    group: str
    form: str                        # aimed form: one of FORMS, "refused" or "none"
    dtype: str
    argmax_bits: int
    shape: tuple                     # (nimg, H, W, C)
    PH: int
    PW: int
    rois: np.ndarray                 # (R, 5) float32
    workspace: object = None         # None, "auto", "short" (one byte less than declared) or "misaligned" (8 bytes past a 16-byte boundary)
    layout: str = "interleaved"      # image index of the ROIs: "interleaved", "grouped", "grouped_gap" (image 1 owns none), "single"
    feat_kind: str = "ties"          # "ties": quantised normal values; "values": the special-value map
    feat_offset: int = 0             # feat starts this many BYTES past a 16-byte boundary
    pad: int = 0                     # row pitch - C * PH * PW, in elements; negative: the pitch handed over is too small
    row_scale: bool = False
    code: int = 0                    # refusal code
    CB: int = 0                      # expected channels per lane where the case is about them
    expect: dict = None              # further plan fields the case pins, e.g. {"n_bands": 2}

    @property
    def R(self):
        return self.rois.shape[0]

    def plan_workspace(self):
        nimg, H, W, C = self.shape
        need = fwd_workspace_bytes(nimg, self.R, self.PH, self.PW)
        return {None: None, "auto": "auto", "short": (need - 1, True), "misaligned": (need, False)}[self.workspace]

    def plan(self):
        nimg, H, W, C = self.shape
        row = C * self.PH * self.PW
        return fwd_plan(self.dtype, self.argmax_bits, nimg, H, W, C, self.PH, self.PW, self.R, row + self.pad if self.pad else 0,
                        self.feat_offset % 16 == 0, self.plan_workspace())

    def feat(self):
        nimg, H, W, C = self.shape
        return values_map(nimg, C, H, W, self.dtype) if self.feat_kind == "values" else ties_map(nimg, C, H, W)

    def scales(self):
        """(row_scale, add) or (None, 0)"""
        if not self.row_scale:
            return None, 0.0
        return np.random.default_rng(self.R).random(self.R).astype(np.float32), 1.0


def ties_map(nimg, C, H, W):
    """normal values quantised to halves (exact in bf16): many equal maxima inside a window"""
    rng = np.random.default_rng(nimg * 7 + C * 3 + H * 1000 + W)
    return (np.round(rng.standard_normal((nimg, C, H, W)) * 2) / 2).astype(np.float32)


VALUE_CHANNELS = ["-inf", "nan_rows", "signed_zero", "lowest", "neg_nan_cols", "+inf", "plateaus", "pow2_pairs"]


def values_map(nimg, C, H, W, dtype):
    """the map of test_roi_pool_ties_and_special_values, for any shape: channel c holds VALUE_CHANNELS[c % 8]; the other values are small
    integers (plateaus).  "pow2_pairs": row y is -1 but for two pixels of value 5 that lie 2^(y % 6) apart, the first at column
    (3 * y) % max(W - 2^L, 1) — a window that holds both must name the first."""
    rng = np.random.default_rng(5 + H * 1000 + W)
    feat = rng.integers(-2, 3, size=(nimg, C, H, W)).astype(np.float32)
    lowest = float(np.finfo(np.float32).min) if dtype == "f32" else -3.3895313892515355e38      # the most negative bf16
    for c in range(C):
        kind = VALUE_CHANNELS[c % 8]
        if kind == "-inf":
            feat[:, c] = -np.inf
        elif kind == "nan_rows":
            feat[:, c, ::2, :] = np.nan
        elif kind == "signed_zero":
            feat[:, c] = np.where(rng.random((nimg, H, W)) < 0.5, -0.0, 0.0)
        elif kind == "lowest":
            feat[:, c] = lowest
        elif kind == "neg_nan_cols":
            feat[:, c, :, ::3] = -np.nan
        elif kind == "+inf":
            feat[:, c] = np.inf
        elif kind == "pow2_pairs":
            feat[:, c] = -1.0
            for y in range(H):
                d = 1 << (y % 6)
                if d >= W:
                    d = 1
                x0 = (3 * y) % max(W - d, 1)
                feat[:, c, y, x0] = 5.0
                feat[:, c, y, x0 + d] = 5.0
    return feat


def image_index(layout, R, nimg):
    if layout == "interleaved":
        return np.arange(R) % nimg
    if layout == "single":
        return np.zeros(R, np.int64)
    owners = [i for i in range(nimg) if not (layout == "grouped_gap" and i == 1)]
    return np.asarray(owners)[np.minimum(np.arange(R) * len(owners) // max(R, 1), len(owners) - 1)]


SPECIAL_BOXES = [[0, 0, 1e4, 1e4], [-500, -500, -100, -100], [100, 100, 90, 90], [3.9, 3.9, 4.1, 4.1], [-1e4, -1e4, 1e4, 1e4],
                 [60, 60, 67.9, 68.1], [40, 16, 16, 90], [40, 90, 90, 16]]


def mixed_boxes(R, H, W, seed=0, max_px=None):
    """R boxes: random ones (a third small), a tenth out on the left / top, a tenth out on the right / bottom, and, from row 2R/10 on, what
    the forms have to survive: the whole map, far outside, malformed (end < start), one pixel, everything, half-integer edges, boxes
    past the last row / column, around the map's edges.  max_px: largest extent in feature pixels (keeps a large R cheap)."""
    rng = np.random.default_rng(H * 1000 + W + seed)
    IH, IW = 8 * H, 8 * W
    x1 = rng.random(R) * (IW - 16)
    y1 = rng.random(R) * (IH - 16)
    bw = 8 + rng.random(R) * (IW - x1)
    bh = 8 + rng.random(R) * (IH - y1)
    small = rng.random(R) < 0.35
    bw[small] = 8 + rng.random(int(small.sum())) * 100
    bh[small] = 8 + rng.random(int(small.sum())) * 100
    if max_px:
        bw = np.minimum(bw, 8.0 * max_px)
        bh = np.minimum(bh, 8.0 * max_px)
    boxes = np.stack([x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32)
    k = R // 10
    boxes[:k, 0] -= rng.random(k) * 150
    boxes[:k, 1] -= rng.random(k) * 150
    boxes[k:2 * k, 2] += rng.random(k) * 150
    boxes[k:2 * k, 3] += rng.random(k) * 150
    if max_px:
        return boxes
    special = SPECIAL_BOXES + [[IW - 9, IH - 9, IW + 40, IH + 40], [-40, 10, IW + 50, 30], [20, -30, 40, IH + 90], [4, 4, 12, IH],
                               [0, IH - 8, IW, IH + 300], [IW - 8, 0, IW + 300, IH], [0, IH, IW, IH + 64], [IW, 0, IW + 64, IH]]
    n = min(len(special), max(R - 2 * k, 0))
    boxes[2 * k:2 * k + n] = np.asarray(special[:n], np.float32).reshape(-1, 4)
    return boxes


def make_rois(layout, nimg, boxes):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    return _rois_from_boxes(image_index(layout, len(boxes), nimg), boxes)


def _case(name, group, form, dtype, bits, nimg, H, W, C, PH, PW, R=200, ws=None, layout="interleaved", boxes=None, **kw):
    if boxes is None:
        boxes = mixed_boxes(R, H, W, max_px=kw.pop("max_px", None))
    else:
        kw.pop("max_px", None)
    return FwdCase(f"{group}/{name}", group, form, dtype, bits, (nimg, H, W, C), PH, PW, make_rois(layout, nimg, boxes), ws, layout, **kw)


def _form_of(*a, **k):
    return fwd_plan(*a, **k).form


# The shapes that reach each form with few channels.  What keeps the earlier forms out is in the comment.
TASKS_MAP = (72, 72)          # more than 5088 pixels: not whole at 8 channels per lane; one band
BAND_MAP = (110, 100)         # more than 10240 pixels: row bands in the task, sparse and plane-band forms
WHOLE_MAP = (40, 50)
FORM_SHAPES = {               # form id: (dtype, H, W, C, PH, PW, workspace, CB)
    "tasks": ("bf16", *TASKS_MAP, 16, 7, 7, "auto", 4),
    "tasks_bands": ("bf16", *BAND_MAP, 16, 7, 7, "auto", 4),
    "sparse_whole": ("bf16", *WHOLE_MAP, 16, 7, 7, None, 8),
    "sparse_band": ("bf16", *BAND_MAP, 16, 7, 7, None, 4),
    "plane_band": ("bf16", *BAND_MAP, 8, 9, 7, None, 8),                # PH = 9: not sparse; 16-byte pixels do not fit: bands
    "plane_bf16_cb8": ("bf16", *WHOLE_MAP, 8, 9, 7, None, 8),           # PH = 9: not sparse; fits: whole plane
    "plane_bf16_cb4": ("bf16", 24, 30, 12, 7, 7, None, 4),              # C % 8 != 0
    "plane_bf16_cb2": ("bf16", 24, 30, 6, 7, 7, None, 2),
    "plane_f32_cb4": ("f32", *WHOLE_MAP, 8, 7, 7, None, 4),
    "plane_f32_cb2": ("f32", 24, 30, 6, 7, 7, None, 2),
    "plane_f32_cb1": ("f32", 24, 30, 3, 7, 7, None, 1),
    "gather_bf16": ("bf16", 256, 12, 8, 7, 7, None, 2),                 # H = 256
    "gather_f32": ("f32", 256, 12, 8, 7, 7, None, 1),
}
FORM_NAME = {                 # form id: FwdPlan.form
    "tasks": "tasks",
    "tasks_bands": "tasks",
    "sparse_whole": "sparse_whole",
    "sparse_band": "sparse_band",
    "plane_band": "plane_band",
    "plane_bf16_cb8": "plane",
    "plane_bf16_cb4": "plane",
    "plane_bf16_cb2": "plane",
    "plane_f32_cb4": "plane",
    "plane_f32_cb2": "plane",
    "plane_f32_cb1": "plane",
    "gather_bf16": "gather",
    "gather_f32": "gather",
}
assert FORM_NAME.keys() == FORM_SHAPES.keys()


def form_case(fid, bits=16, group="forms", name=None, nimg=2, R=200, **kw):
    dtype, H, W, C, PH, PW, ws, CB = FORM_SHAPES[fid]
    C = kw.pop("C", C)
    ws = kw.pop("ws", ws)
    expect = kw.pop("expect", None)
    if fid in ("tasks_bands", "sparse_band", "plane_band") and expect is None:
        expect = {"multi_band": True}
    return _case(name or f"{fid}_a{bits}", group, FORM_NAME[fid], dtype, bits, nimg, H, W, C, PH, PW, R, ws, CB=kw.pop("CB", CB), expect=expect, **kw)


def forms_cases():
    return [form_case(fid, bits, row_scale=(i + bits // 16) % 2 == 0) for i, fid in enumerate(FORM_SHAPES) for bits in (16, 32)]


# ------------------------------------------------------------------------------------------------ thresholds
def _largest_whole_W(H, R, C=8, PH=7, PW=7):
    """the widest map of H rows the sparse form still holds whole at R ROIs (from the mirror's LDS arithmetic)"""
    W = 8
    while _form_of("bf16", 16, 2, H, W + 1, C, PH, PW, R, 0, True, None) == "sparse_whole":
        W += 1
    return W


def _first_R_not_whole(H, W, C=8, PH=7, PW=7):
    R = 1
    while _form_of("bf16", 16, 2, H, W, C, PH, PW, R, 0, True, None) == "sparse_whole":
        R += 1
    return R


def _whole_misses_by_a_row(R, PH=7, PW=7):
    """(H, W) of the smallest map whose whole sparse table is larger than a CU's LDS while that of H - 1 rows still fits whole"""
    best = None
    for W in range(50, 256):
        for H in range(20, 256):
            if (sparse_lds_bytes((H - 1) * W * 32, R, SP_CH, PH, PW, False) <= SPARSE_LDS_MAX < LDS_CU < sparse_lds_bytes(H * W * 32, R, SP_CH, PH, PW, False)
                    and (best is None or H * W < best[0] * best[1])):
                best = (H, W)
    return best


def _task_bands(H, W, PH, PW=7):
    """band_geometry as launch_fwd_tasks calls it, or "whole" where the map stays with the sparse form"""
    ring = tasks_lds_bytes(0, W, PW)
    if H * W * 32 + ring <= TASKS_LDS_ALL:
        return "whole"
    return band_geometry(H, PH, min((TASKS_LDS_ALL - ring) // (W * 16), 10 * 1024 // W), TASK_BANDS)


def _sparse_bands(H, W, PH, R, PW=7):
    if sparse_lds_bytes(H * W * 32, R, SP_CH, PH, PW, False) <= SPARSE_LDS_MAX:
        return "whole"
    return band_geometry(H, PH, min((SPARSE_LDS_MAX - sparse_lds_bytes(0, R, SP_CH, PH, PW, True)) // (W * 16), 10 * SP_NT // W), SPARSE_BANDS)


def _band_refusal_shape(rule, R=100):
    """the smallest bf16 map (H, W, PH) on which `rule`'s band_geometry declines while the form's other conditions hold — from the
    mirror's arithmetic.  Pooled heights 1 and 2 make the halo (ceil(H / PH) + 1 rows) as tall as the map."""
    best = None
    for PH in ((9, 10, 12) if rule == "plane_band" else (1, 2, 3)):
        for H in range(40, 256, 3):
            for W in range(40, 256, 3):
                if rule == "tasks":
                    hit = _task_bands(H, W, PH) is None
                elif rule == "sparse":
                    hit = _sparse_bands(H, W, PH, R) is None
                else:
                    hit = H * W * 16 > PLANE_BUDGET and plane_band_geometry(H, W, PH, 7) is None
                if hit and (best is None or H * W < best[0] * best[1]):
                    best = (H, W, PH)
    return best


def _maxb_straddle():
    """(PH, H, W): the task form's bands number TK_MAXB on H rows and more on H + 1"""
    best = None
    for PH in (2, 3):
        for H in range(40, 255):
            for W in range(100, 256):
                a, b = _task_bands(H, W, PH), _task_bands(H + 1, W, PH)
                if a and b and a != "whole" and b != "whole" and a[2] == TK_MAXB and b[2] > TK_MAXB and (best is None or H * W < best[1] * best[2]):
                    best = (PH, H, W)
    return best


def threshold_pairs():
    """[(what, [case, case, ...])]: the cases of one entry straddle one inequality; neighbours land on different forms (or CB)"""
    T = "thresholds"
    out = []

    def pair(what, *cases):
        out.append((what, list(cases)))

    # H, W <= 255
    pair("H 255/256", _case("H255", T, "sparse_whole", "bf16", 16, 2, 255, 12, 8, 7, 7), _case("H256", T, "gather", "bf16", 16, 2, 256, 12, 8, 7, 7))
    pair("W 255/256", _case("W255", T, "sparse_whole", "bf16", 16, 2, 12, 255, 8, 7, 7), _case("W256", T, "gather", "bf16", 16, 2, 12, 256, 8, 7, 7))
    # feat alignment
    pair("feat 16-byte aligned / +8 bytes (no workspace)", form_case("sparse_whole", 16, T, "feat_aligned"),
         _case("feat_off8", T, "gather", "bf16", 16, 2, *WHOLE_MAP, 16, 7, 7, feat_offset=8, CB=2))
    pair("feat 16-byte aligned / +8 bytes (workspace)", form_case("tasks", 32, T, "feat_aligned_ws"),
         _case("feat_off8_ws", T, "gather", "bf16", 32, 2, *TASKS_MAP, 16, 7, 7, ws="auto", feat_offset=8, CB=2))
    # H * W * {16, 8, 4} against 150 KiB
    for (a, b), cbs in (((96, 100), (97, 99)), (4, 2)), (((120, 160), (113, 170)), (2, 1)):
        pair(f"f32 plane {a[0]}x{a[1]} / {b[0]}x{b[1]}",
             _case(f"f32_{a[0]}x{a[1]}", T, "plane", "f32", 32, 2, *a, 4, 7, 7, R=100, CB=cbs[0]),
             _case(f"f32_{b[0]}x{b[1]}", T, "plane", "f32", 32, 2, *b, 4, 7, 7, R=100, CB=cbs[1], row_scale=True))
    pair("f32 plane 160x240 / gather 161x239", _case("f32_160x240", T, "plane", "f32", 16, 1, 160, 240, 4, 7, 7, R=100, CB=1),
         _case("f32_161x239", T, "gather", "f32", 16, 1, 161, 239, 4, 7, 7, R=100, CB=1))
    pair("bf16 plane 120x160 / 113x170 (C = 4)", _case("bf16_120x160", T, "plane", "bf16", 16, 2, 120, 160, 4, 7, 7, R=100, CB=4),
         _case("bf16_113x170", T, "plane", "bf16", 16, 2, 113, 170, 4, 7, 7, R=100, CB=2))
    pair("bf16 plane 160x240 / gather 161x239 (C = 4)", _case("bf16_160x240", T, "plane", "bf16", 32, 1, 160, 240, 4, 7, 7, R=100, CB=2),
         _case("bf16_161x239", T, "gather", "bf16", 32, 1, 161, 239, 4, 7, 7, R=100, CB=2))
    pair("bf16 plane 96x100 / plane-band 97x99 (9 x 6)", _case("bf16_96x100_9x6", T, "plane", "bf16", 16, 2, 96, 100, 8, 9, 6, R=100, CB=8),
         _case("bf16_97x99_9x6", T, "plane_band", "bf16", 16, 2, 97, 99, 8, 9, 6, R=100, CB=8, row_scale=True))
    # the plane AND its ROI tables must fit: a 150 KiB plane has room for the tables of PH + PW <= 15
    pair("tables beside a 150 KiB plane: 9 x 6 / 9 x 7 (bf16)", _case("bf16_96x100_9x6_tables", T, "plane", "bf16", 32, 2, 96, 100, 8, 9, 6, R=100, CB=8),
         _case("bf16_96x100_9x7", T, "plane_band", "bf16", 16, 2, 96, 100, 8, 9, 7, R=100, CB=8))
    pair("tables beside a 150 KiB plane: 8 x 7 / 9 x 7 (f32)", _case("f32_96x100_8x7", T, "plane", "f32", 32, 2, 96, 100, 4, 8, 7, R=100, CB=4),
         _case("f32_96x100_9x7", T, "plane", "f32", 32, 2, 96, 100, 4, 9, 7, R=100, CB=2))
    # channel divisibility
    pair("bf16 C 8/12/6/2/3", *[_case(f"bf16_C{C}", T, form, "bf16", 16, 2, 24, 30, C, 7, 7, CB=cb, code=code, row_scale=C == 6)
                               for C, form, cb, code in ((8, "sparse_whole", 8, 0), (12, "plane", 4, 0), (6, "plane", 2, 0), (2, "plane", 2, 0),
                                                         (3, "refused", 0, -5))])
    pair("f32 C 4/6/3/1", *[_case(f"f32_C{C}", T, "plane", "f32", 32, 2, 24, 30, C, 7, 7, CB=cb, row_scale=C == 3)
                            for C, cb in ((4, 4), (6, 2), (3, 1), (1, 1))])
    # R <= 16384 (sparse) and R <= 65535 (tasks); pooled 3 x 3, small ROIs
    big = dict(max_px=6)
    pair("R 16384/16385", _case("R16384", T, "sparse_band", "bf16", 16, 2, *TASKS_MAP, 8, 3, 3, R=16384, **big),
         _case("R16385", T, "plane", "bf16", 16, 2, *TASKS_MAP, 8, 3, 3, R=16385, CB=8, **big))
    pair("R 65535/65536 (workspace)", _case("R65535", T, "tasks", "bf16", 16, 2, *TASKS_MAP, 8, 3, 3, R=65535, ws="auto", row_scale=True, **big),
         _case("R65536", T, "plane", "bf16", 16, 2, *TASKS_MAP, 8, 3, 3, R=65536, ws="auto", CB=8, **big))
    # pooled size <= 8
    pair("PH 8/9", _case("PH8", T, "sparse_whole", "bf16", 16, 2, *WHOLE_MAP, 8, 8, 8), _case("PH9", T, "plane", "bf16", 16, 2, *WHOLE_MAP, 8, 9, 8, CB=8))
    pair("PW 8/9", _case("PW8", T, "sparse_whole", "bf16", 32, 2, *WHOLE_MAP, 8, 8, 8, row_scale=True),
         _case("PW9", T, "plane", "bf16", 32, 2, *WHOLE_MAP, 8, 8, 9, CB=8))
    pair("PH 8/9 (workspace)", _case("PH8_ws", T, "tasks", "bf16", 16, 2, *TASKS_MAP, 8, 8, 8, ws="auto"),
         _case("PH9_ws", T, "plane", "bf16", 16, 2, *TASKS_MAP, 8, 9, 8, ws="auto", CB=8))
    # PW >= 3 of the task form
    pair("PW 3/2 (workspace)", _case("PW3_ws", T, "tasks", "bf16", 16, 2, *TASKS_MAP, 8, 7, 3, ws="auto"),
         _case("PW2_ws", T, "sparse_band", "bf16", 16, 2, *TASKS_MAP, 8, 7, 2, ws="auto", row_scale=True))
    # workspace
    pair("workspace present / absent", form_case("tasks", 16, T, "ws_present", row_scale=True),
         _case("ws_absent", T, "sparse_band", "bf16", 16, 2, *TASKS_MAP, 16, 7, 7))
    pair("workspace whole / one byte short", form_case("tasks", 16, T, "ws_whole"),
         _case("ws_short", T, "refused", "bf16", 16, 2, *TASKS_MAP, 16, 7, 7, ws="short", code=-5))
    pair("workspace aligned / 8 bytes off", form_case("tasks", 32, T, "ws_aligned"),
         _case("ws_misaligned", T, "refused", "bf16", 32, 2, *TASKS_MAP, 16, 7, 7, ws="misaligned", code=-5))
    # whole map -> row bands of the sparse form: by map size at R = 200, by R on that map
    Hs = 64
    Wmax = _largest_whole_W(Hs, 200)
    pair(f"sparse whole {Hs}x{Wmax} / bands {Hs}x{Wmax + 1} at R = 200", _case("whole_W", T, "sparse_whole", "bf16", 16, 2, Hs, Wmax, 8, 7, 7),
         _case("band_W", T, "sparse_band", "bf16", 16, 2, Hs, Wmax + 1, 8, 7, 7, row_scale=True))
    Rflip = _first_R_not_whole(Hs, Wmax)
    pair(f"sparse whole R = {Rflip - 1} / bands R = {Rflip} on {Hs}x{Wmax}",
         _case("whole_R", T, "sparse_whole", "bf16", 16, 2, Hs, Wmax, 8, 7, 7, R=Rflip - 1, max_px=20),
         _case("band_R", T, "sparse_band", "bf16", 16, 2, Hs, Wmax, 8, 7, 7, R=Rflip, max_px=20))
    # the same flip by one ROW, where the whole table of the taller map is more than a CU has: taking the whole form a row early cannot launch
    Hr, Wr = _whole_misses_by_a_row(200)
    assert sparse_lds_bytes(Hr * Wr * 32, 200, SP_CH, 7, 7, False) > LDS_CU
    pair(f"sparse whole {Hr - 1}x{Wr} / bands {Hr}x{Wr}, whose whole table exceeds LDS", _case("whole_H", T, "sparse_whole", "bf16", 32, 2, Hr - 1, Wr, 8, 7, 7),
         _case("band_H_past_lds", T, "sparse_band", "bf16", 32, 2, Hr, Wr, 8, 7, 7))
    # the same flip of the task form (no R in its LDS): by map size
    Wt = 8
    while _form_of("bf16", 16, 2, Hs, Wt + 1, 8, 7, 7, 200, 0, True, "auto") == "sparse_whole":
        Wt += 1
    pair(f"workspace: sparse whole {Hs}x{Wt} / tasks {Hs}x{Wt + 1}", _case("ws_whole_W", T, "sparse_whole", "bf16", 16, 2, Hs, Wt, 8, 7, 7, ws="auto"),
         _case("ws_tasks_W", T, "tasks", "bf16", 16, 2, Hs, Wt + 1, 8, 7, 7, ws="auto"))
    # nimg * n_bands <= 64
    pair("nimg * n_bands 64/65", _case("nimg64", T, "tasks", "bf16", 16, 64, *TASKS_MAP, 8, 7, 7, R=260, ws="auto", expect={"n_bands": 1}),
         _case("nimg65", T, "sparse_band", "bf16", 16, 65, *TASKS_MAP, 8, 7, 7, R=260, ws="auto", row_scale=True))
    # n_bands <= TK_MAXB: reachable (pooled height 2 on a wide map leaves bands of 4 or 5 rows)
    PHm, Hm, Wm = _maxb_straddle()
    pair("n_bands 16/17 (workspace)", _case("bands16", T, "tasks", "bf16", 16, 1, Hm, Wm, 8, PHm, 7, R=100, ws="auto", expect={"n_bands": TK_MAXB}),
         _case("bands17", T, "plane", "bf16", 16, 1, Hm + 1, Wm, 8, PHm, 7, R=100, ws="auto", CB=4))      # (the sparse form declines too)
    # band_geometry declining, per rule: the next form takes the call
    for rule, then, cb in (("tasks", "sparse_band", 4), ("sparse", "plane", 4), ("plane_band", "gather", 2)):
        H, W, PH = _band_refusal_shape(rule)
        ws = "auto" if rule == "tasks" else None
        pair(f"band_geometry declines for {rule}", _case(f"declined_{rule}", T, then, "bf16", 16, 1, H, W, 8, PH, 7, R=100, ws=ws, CB=cb))
    # pooled 103 x 7: the band form's ROI tables alone are larger than a CU's LDS; it declines (a signed budget) and the plane form at 4
    # channels per lane, whose tables have no owned-pair list, takes the call
    assert LDS_CU - 1024 - plane_lds_bytes(0, BAND_MAP[1], 16, PLANE_CHUNK, 103, 7, True) < 0
    pair("plane-band tables larger than LDS", _case("declined_plane_band_tables", T, "plane", "bf16", 16, 2, *BAND_MAP, 8, 103, 7, R=60, CB=4))
    # gather's LDS bound, through a misaligned 8 x 8 map
    pair("gather bf16 PH * PW 85/86", _case("g85", T, "gather", "bf16", 16, 1, 8, 8, 8, 5, 17, R=40, feat_offset=8),
         _case("g86", T, "refused", "bf16", 16, 1, 8, 8, 8, 2, 43, R=40, feat_offset=8, code=-6))
    pair("gather f32 PH * PW 128/129", _case("g128", T, "gather", "f32", 32, 1, 8, 8, 8, 8, 16, R=40, feat_offset=8, row_scale=True),
         _case("g129", T, "refused", "f32", 32, 1, 8, 8, 8, 3, 43, R=40, feat_offset=8, code=-6))
    # pitch
    pair("ld too small / dense / + 8", _case("ld_small", T, "refused", "bf16", 16, 2, *WHOLE_MAP, 16, 7, 7, pad=-8, code=-5),
         form_case("sparse_whole", 16, T, "ld_dense"), form_case("sparse_whole", 16, T, "ld_plus8", pad=8))
    # R = 0
    pair("R 1/0", form_case("sparse_whole", 16, T, "R1", R=1), _case("R0", T, "none", "bf16", 16, 2, *WHOLE_MAP, 16, 7, 7, R=0))
    # 16-bit argmax needs < 65535 pixels
    pair("16-bit argmax at 65535 pixels", _case("a32_65535px", T, "gather", "bf16", 32, 1, 255, 257, 2, 3, 3, R=60),
         _case("a16_65535px", T, "refused", "bf16", 16, 1, 255, 257, 2, 3, 3, R=60, code=-6))
    return out


def thresholds_cases():
    return [c for _, cs in threshold_pairs() for c in cs]


# ------------------------------------------------------------------------------------------------ chunks
CHUNK_COUNTS = [127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
CHUNK_FORMS = ["sparse_whole", "tasks", "plane_bf16_cb4"]
LAYOUT_FORMS = ["tasks_bands", "sparse_whole", "sparse_band", "plane_band", "plane_bf16_cb4", "plane_f32_cb4", "gather_bf16"]


def one_class_boxes(R, H, W):
    """R ROIs of 14 x 14 feature pixels (7 x 7 bins of 2 x 2: level 1, height class 2) at different places"""
    i = np.arange(R)
    return [px_box(int(a) % (W - 14), int(a * 7) % (H - 14), 14, 14) for a in i]


def chunks_cases():
    G = "chunks"
    out = []
    for fid in CHUNK_FORMS:
        for R in CHUNK_COUNTS:
            out.append(form_case(fid, 16, G, f"{fid}_R{R}", R=R, C=FORM_SHAPES[fid][3] if "plane" in fid else 8, max_px=24,
                                 row_scale=R % 2 == 1))
    for fid in LAYOUT_FORMS:
        for layout in ("interleaved", "grouped", "grouped_gap"):
            out.append(form_case(fid, 32 if layout == "grouped" else 16, G, f"{fid}_{layout}", nimg=3, R=600, layout=layout, max_px=30,
                                 row_scale=layout == "grouped"))
    for fid in ("sparse_whole", "sparse_band", "tasks", "tasks_bands"):
        dtype, H, W, C, PH, PW, ws, CB = FORM_SHAPES[fid]
        out.append(form_case(fid, 16, G, f"{fid}_one_class", R=300, boxes=one_class_boxes(300, H, W), layout="grouped"))
    # zsplit: nz == 1, nz > 1 below the number of chunks, nz capped at it (3 x 3 bins, small ROIs: the maps have 512 channels)
    for name, fid, nimg, R, want in (("nz1", "sparse_whole", 3, 300, "one"), ("nz_free", "sparse_whole", 1, 700, "free"),
                                     ("nz_capped", "sparse_whole", 2, 200, "capped"), ("nz1", "tasks", 2, 300, "one"),
                                     ("nz_free", "tasks", 1, 300, "free")):
        dtype, H, W, _, _, _, ws, CB = FORM_SHAPES[fid]
        out.append(_case(f"{fid}_{name}", G, FORM_NAME[fid], dtype, 16, nimg, H, W, 512, 3, 3, R, ws, max_px=8, CB=CB, expect={"nz": want}))
    out.append(form_case("plane_bf16_cb4", 16, G, "plane_nz_capped", R=600, max_px=24, expect={"nz": "capped"}))
    # One workgroup per (slab, image): for_my_rois deals 8 row blocks of 128 ROIs a round, so R = 1024 is the last single round, 1025
    # starts a second one and 2177 a third (192 slabs x images leave nz == 1).  The band form the same way.
    for R, rounds in ((1023, 1), (1024, 1), (1025, 2), (2177, 3)):
        out.append(_case(f"sparse_whole_rounds_R{R}", G, "sparse_whole", "bf16", 16, 3, *WHOLE_MAP, 512, 3, 3, R, None, max_px=8, CB=8,
                         layout="grouped" if R == 2177 else "interleaved", row_scale=R == 1025, expect={"nz": "one", "rounds": rounds}))
    out.append(_case("sparse_band_rounds_R1025", G, "sparse_band", "bf16", 16, 2, *BAND_MAP, 256, 3, 3, 1025, None, max_px=8, CB=4,
                     layout="grouped", expect={"nz": "one", "rounds": 2, "multi_band": True}))
    # Plane forms with fewer workgroups than chunks (many slabs): a workgroup walks chunks z, z + nz, ...  Grouped by image, the
    # workgroups of the last image meet chunks that hold none of its ROIs first and load the plane at a later one.
    for fid, dtype, (H, W), C, PH, PW, CB in (("plane_f32_cb4", "f32", TASKS_MAP, 512, 3, 3, 4), ("plane_bf16_cb8", "bf16", TASKS_MAP, 512, 9, 2, 8),
                                             ("plane_band", "bf16", BAND_MAP, 256, 9, 2, 8)):
        for layout in ("interleaved", "grouped", "grouped_gap"):
            out.append(_case(f"{fid}_walk_{layout}", G, FORM_NAME[fid], dtype, 16, 3, H, W, C, PH, PW, 1500, None, layout=layout, max_px=8, CB=CB,
                             row_scale=layout == "grouped", expect={"walk": "two_chunks" if layout == "interleaved" else "empty_first"}))
    return out


def sparse_rounds(plan):
    """rounds of the sparse kernel's for_my_rois: a round deals 8 row blocks of 128 ROIs to each of the nz workgroups"""
    return -(-plan.n_chunks // (8 * plan.nz))


def plane_walks(case, plan):
    """{(image, z): ROIs of the image in each chunk the plane kernel's workgroup z walks (z, z + nz, ...)}"""
    img = case.rois[:, 0].astype(np.int64)
    return {(i, z): [int((img[c * plan.chunk:(c + 1) * plan.chunk] == i).sum()) for c in range(z, plan.n_chunks, plan.nz)]
            for i in range(case.shape[0]) for z in range(plan.nz)}


# ------------------------------------------------------------------------------------------------ classes
SIZE_BOUNDS = [1, 2, 3, 4, 6, 8]
LEVEL_WIDTHS = [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 33, 64, 65]
CLASS_FORMS = ["sparse_whole", "sparse_band", "tasks", "tasks_bands", "plane_band", "plane_bf16_cb4", "plane_f32_cb4", "gather_bf16"]
CLASS_MAPS = {"sparse_whole": (56, 86), "plane_bf16_cb4": (56, 86), "plane_f32_cb4": (56, 86), "gather_bf16": (256, 20)}     # W >= 65: a window past the level cap
CLASS_POOLED = [(7, 7), (4, 5)]


def class_extents(P):
    """extents one feature pixel below, on and above every boundary of bin_size_class: bin = extent / P against 1, 2, 3, 4, 6, 8"""
    return sorted({P * b + d for b in SIZE_BOUNDS for d in (-1, 0, 1) if P * b + d >= 1})


def class_boxes(H, W, PH, PW, plan):
    """The ROI set of a `classes` case (feature pixels), for a map of H x W under `plan`:
    heights around every size-class boundary x vertical placements, widths around every boundary and every level width x horizontal
    placements, band placements from the plan's geometry, overshoot heights ending on the map's and a band's last row, malformed and
    one-pixel ROIs."""
    boxes = []
    S, nbd = plan.S, plan.n_bands
    w_fix = [min(2 * PW, W - 2), min(5 * PW + 1, W - 2)]
    h_fix = [min(2 * PH, H - 2), min(5 * PH + 1, H - 2)]
    for i, h in enumerate(class_extents(PH)):
        w = w_fix[i % 2]
        x0 = (5 * i) % max(W - w, 1)
        ys = [max((H - h) // 2, 0), -(h // 2), H - (h + 1) // 2, -h - 3, H + 2, -1, H - h, H - h + 1]   # inside, cut above / below, outside, touching
        ys += [b * S + d for b in range(1, nbd) for d in (-1, 0, 1)]                                    # first row on S - 1, S, S + 1
        ys += [b * S - h for b in range(1, nbd)]                                                        # ending on a band's last owned row
        boxes += [px_box(x0, y, w, h) for y in ys]
    widths = sorted(set(class_extents(PW)) | {PW * v for v in LEVEL_WIDTHS} | {PW * v + 1 for v in LEVEL_WIDTHS} | {PW * v - 1 for v in LEVEL_WIDTHS if PW * v > 1})
    for i, w in enumerate(widths):
        h = h_fix[i % 2]
        y0 = (7 * i) % max(H - h, 1)
        xs = [max((W - w) // 2, 0), -(w // 2), W - (w + 1) // 2, -w - 3, W + 2, -1, W - w, W - w + 1, 0, 1]
        boxes += [px_box(x, y0, w, h) for x in xs]
        if nbd > 1:
            boxes.append(px_box(xs[i % 3], S - 1, w, h))
    boxes += [px_box(1, -2, W - 2, H + 4), px_box(-2, 0, W + 4, H), px_box(3, 0, 9, H)]                 # spanning every band
    for h in overshoot_heights(PH)[:8]:                                                                 # last bin one row past the end row
        boxes.append(px_box(2, H - h, 11, h))                                                          # ending on the map's last row
        boxes += [px_box(4, b * S - h, 9, h) for b in range(1, nbd)]                                    # and on a band's last owned row
    boxes += [[8.0 * 9, 8.0 * 9, 8.0 * 4, 8.0 * 20], [8.0 * 9, 8.0 * 20, 8.0 * 30, 8.0 * 4], [80, 80, 16, 16]]   # malformed
    boxes += [px_box(x, y, 1, h) for x, y, h in ((0, 0, 1), (W - 1, H - 1, 1), (5, 3, 20), (W - 1, 0, H), (W, 2, 5))]   # one pixel wide
    boxes += [px_box(x, y, w, 1) for x, y, w in ((0, H - 1, W), (3, 0, 30), (2, H, 9))]
    return boxes


def classes_cases():
    out = []
    for fid in CLASS_FORMS:
        dtype, H, W, C, PH0, PW0, ws, CB = FORM_SHAPES[fid]
        H, W = CLASS_MAPS.get(fid, (H, W))
        for PH, PW in CLASS_POOLED if PH0 <= 8 else [(9, 7), (10, 5)]:
            R = 700
            for _ in range(4):                                                    # the sparse form's band geometry depends on R: settle it
                plan = fwd_plan(dtype, 16, 2, H, W, C, PH, PW, R, 0, True, ws)
                boxes = class_boxes(H, W, PH, PW, plan)
                R = len(boxes)
            out.append(_case(f"{fid}_{PH}x{PW}", "classes", FORM_NAME[fid], dtype, 16, 2, H, W, C if "plane_b" in fid or "f32" in fid else 8,
                             PH, PW, ws=ws, boxes=boxes, CB=CB, row_scale=PH == 7,
                             expect={"multi_band": True, "S": plan.S} if plan.n_bands > 1 else None))
    # maps whose last band ends on the map's last row (H == n_bands * S): a bin row that starts at H, below the map, belongs to the last
    # band only through the cap of BandGeom::owner
    for fid in ("sparse_band", "plane_band"):
        dtype, _, W, C, PH, PW, ws, CB = FORM_SHAPES[fid]
        H, boxes = _band_multiple_map(fid)
        out.append(_case(f"{fid}_H_multiple_of_S", "classes", fid, dtype, 16, 2, H, W, 8, PH, PW, ws=ws, boxes=boxes, CB=CB,
                         expect={"multi_band": True, "H_multiple": True}))
    return out


def _band_multiple_map(fid):
    """(H, boxes): the lowest map of BAND_MAP's width that `fid` cuts into bands with H == n_bands * S, with its settled ROI set"""
    dtype, _, W, C, PH, PW, ws, CB = FORM_SHAPES[fid]
    for H in range(100, 256):
        R = 700
        for _ in range(4):
            plan = fwd_plan(dtype, 16, 2, H, W, 8, PH, PW, R, 0, True, ws)
            if plan.form != fid:
                break
            boxes = class_boxes(H, W, PH, PW, plan)
            R = len(boxes)
        if plan.form == fid and plan.n_bands > 1 and plan.n_bands * plan.S == H:
            return H, boxes
    raise AssertionError(fid)


# ------------------------------------------------------------------------------------------------ values
VALUE_FORMS = list(FORM_SHAPES)


def pow2_boxes(H, W, PH, PW):
    """windows that hold both maxima of a "pow2_pairs" row: ROIs of every level width starting at the first maximum's column of their row"""
    boxes = []
    for y in range(0, min(H, 48)):
        d = 1 << (y % 6)
        if d >= W:
            d = 1
        x0 = (3 * y) % max(W - d, 1)
        for width in (d + 1, 2 * d, 2 * d + 1):
            boxes.append(px_box(x0 - (y % 2), y, PW * width, PH))               # bin column 0 spans x0 .. x0 + width - 1 on row y
    return boxes


def values_cases():
    out = []
    for i, fid in enumerate(VALUE_FORMS):
        dtype, H, W, C, PH, PW, ws, CB = FORM_SHAPES[fid]
        boxes = np.concatenate([mixed_boxes(160, H, W, seed=3), np.asarray(pow2_boxes(H, W, PH, PW), np.float32)])
        bits = 32 if i % 2 else 16
        C8 = C if fid.startswith("plane_") and fid != "plane_band" and C % 8 else max(C, 8)
        if fid in ("plane_bf16_cb4", "plane_f32_cb2"):
            C8 = 12 if dtype == "bf16" else 10                                   # every special channel, still C % 8 != 0 / C % 4 != 0
        if fid == "plane_bf16_cb2":
            C8 = 10
        if fid == "plane_f32_cb1":
            C8 = 9
        out.append(form_case(fid, bits, "values", f"{fid}_a{bits}", C=C8, boxes=boxes, feat_kind="values", layout="single", nimg=1))
    return out


# ------------------------------------------------------------------------------------------------ slabs
SLAB_COUNTS = [1, 7, 8, 9, 16]


def slabs_cases():
    out = []
    for fid, mult in (("sparse_whole", 8), ("plane_f32_cb4", 4), ("plane_band", 8), ("sparse_band", 4), ("tasks", 4)):
        for n in SLAB_COUNTS:
            C = n * mult
            if mult == 4 and fid != "plane_f32_cb4":
                C = 2 * n * mult                                                  # 4 channels per lane of C % 8 == 0: 2, 14, 16, 18, 32 slabs
            out.append(form_case(fid, 16, "slabs", f"{fid}_{C // mult}slabs", C=C, R=130, max_px=16, expect={"slabs": C // mult}))
    for n in (1, 7, 9):                                                           # bf16 key plane at 4 channels per lane: C % 8 != 0
        out.append(form_case("plane_bf16_cb4", 32, "slabs", f"plane_bf16_cb4_{n}slabs", C=4 * n, R=130, max_px=16, expect={"slabs": n}))
    return out


# ------------------------------------------------------------------------------------------------ untouched
def untouched_cases():
    # (two in three with a workspace: the forms other than the task one keep their shapes with it, and must leave it alone)
    return [form_case(fid, 16 if i % 2 else 32, "untouched", f"{fid}", pad=8, R=150, ws="auto" if i % 3 else FORM_SHAPES[fid][6])
            for i, fid in enumerate(FORM_SHAPES)]


GROUPS = {"forms": forms_cases, "thresholds": thresholds_cases, "chunks": chunks_cases, "classes": classes_cases, "values": values_cases,
          "slabs": slabs_cases, "untouched": untouched_cases}
_ALL = {}


def fwd_cases(group):
    """the cases of a group, built once"""
    if group not in _ALL:
        _ALL[group] = GROUPS[group]()
        names = [c.name for c in _ALL[group]]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return _ALL[group]


def check_fwd_plan(case, plan=None):
    """the plan of a case is the one it was built for"""
    p = plan or case.plan()
    nimg, H, W, C = case.shape
    assert p.form == case.form and p.code == case.code, (case.name, case.form, case.code, p)
    if case.CB:
        assert p.CB == case.CB, (case.name, case.CB, p)
    for k, v in (case.expect or {}).items():
        if k == "multi_band":
            assert p.n_bands > 1, (case.name, p)
        elif k == "H_multiple":
            assert p.n_bands * p.S == H, (case.name, p)
        elif k == "slabs":
            assert C // p.CB == v, (case.name, p)
        elif k == "nz":
            ok = {"one": p.nz == 1, "free": 1 < p.nz and (p.form == "tasks" or p.nz < p.n_chunks), "capped": p.nz == p.n_chunks > 1}[v]
            assert ok, (case.name, v, p)
        elif k == "rounds":
            assert p.form.startswith("sparse") and sparse_rounds(p) == v, (case.name, v, p)
        elif k == "walk":
            walks = plane_walks(case, p)
            assert p.form.startswith("plane") and p.nz < p.n_chunks, (case.name, p)
            if v == "empty_first":             # some workgroup's first chunk holds no ROI of its image and a later one does
                assert any(w[0] == 0 and any(w[1:]) for w in walks.values()), (case.name, walks)
            else:                              # some workgroup works on a second chunk after a first
                assert any(len(w) > 1 and w[0] > 0 and w[1] > 0 for w in walks.values()), (case.name, walks)
        else:
            assert getattr(p, k) == v, (case.name, k, v, p)
    return p

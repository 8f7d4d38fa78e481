"""NumPy restatement of max ROI pooling for the backward's tests (tests/test_roipool_ref_cpu.py, tests/test_gpu_roipool_bwd.py).

* forward geometry and argmax of ROILoopPool_cpu.cpp:26-79 in float32 (roi_extent / bin_edges / roi_pool_fwd);
* the backward of :98-123 as a float64 scatter-add, with what the error bars need beside it (roi_pool_bwd_ref);
* bwd_plan: a mirror of roi_bwd_dispatch (csrc/roipool.hip) — which kernel a call takes and how it is sized;
* overshoot_heights: the ROI heights whose last bin reaches one row past the ROI's end row;
* bwd_bar: the per-element error bars, derived below, never from a kernel's output.

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

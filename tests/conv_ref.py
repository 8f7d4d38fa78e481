"""float64 references of the 3x3 convolution family (csrc/conv_direct.hip, the implicit-GEMM fallback, weight-gradient slabs and folds of
csrc/gemm.hip, csrc/conv_wgrad_direct.hip, the small-map weight gradient of csrc/proposals.hip), restatements of their dispatch, and the
case tables of tests/test_gpu_conv_kernels.py.  Checkers, not product code; CPU only.  tests/test_conv_ref_cpu.py pins the references
to torch.nn.functional.conv2d / autograd in float64 and asserts that every case table reaches the edge it is named for.

Layouts: maps NHWC, weights OIHW, a mask reference (rows = pixels, columns = channels).  The references never call conv2d: nine shifted
matrix products over a zero-padded map.

Two operand generators, both seeded.

Integer operands (placement: no tolerance).  x and dy take values in {-2..2}, weights in {-1, 0, 1}, bias in {-3..3}, mask references
in {-1, -0.0, 0.0, 1, NaN}, cout_scale is a signed power of two (one case per entry point: a general float32, where the expectation is
float32(exact sum) * float32(scale) rounded once, as __fmul_rn does, then one float32 add for `accumulate`).  Every product and every
partial sum is an integer below 2^24, so every float32 accumulation order gives the same bits, and a bf16 output is exact while
|ref| <= 256: these cases demand equality with the float64 reference for every element.  test_conv_ref_cpu.py asserts the two ranges
(max|ref| <= 256 where the output is bf16, the sum of absolute values below 2^24) and that the operands exercise every position (a
non-zero weight for every (tap, ci), every input pixel non-zero in some channel, all five mask values present).  The weight density
is min(1, 112 / Cin): a sum of 9 Cin products, each of variance 2 * density, has sigma <= 45, and 256 is more than 5 sigma.

Gaussian operands (rounding).  x ~ 0.7 N, w ~ 0.05 N, rounded to the input type first, so input rounding is common to both sides.  The
bar is per element and comes from the reference alone:

    allowed = u_out * |ref| + 2 * (K + 2) * 2^-24 * S

S is the float64 convolution of the absolute values (plus |bias|): the sum of the magnitudes that are accumulated for this element.
K is the number of accumulated products (9 Cin for forward and data gradient, n H W for a weight gradient, the slab count for a fold):
a float32 sum of K terms in any order is within K * 2^-24 * S of the exact one to first order (each partial sum is rounded once, and
is bounded by S), and + 2 covers the bias add and a scale multiply.  The factor 2 covers a matrix unit that does not round to nearest
at every step (truncation doubles the unit roundoff).  u_out is the rounding of the stored value: 2^-8 for bf16 (half an ulp is
2^-9 relative at worst; 2^-8 also covers the double rounding f32 -> bf16 of a value already off by the second term), 2^-23 for f32.
ReLU, max and the 0 / 1 mask are 1-Lipschitz, so the same bar holds behind them, with |ref| the reference after them.
"""
import functools
import math

import numpy as np
import torch

from elementwise_ref import conv_direct_form, pool_fused_covered, weight_prep_ref  # noqa: F401  (restated once, there)
from sos_wsod_amd.wgrad import wgrad_direct_covers, wgrad_nslab  # noqa: F401

SLACK = 16                                 # sentinel elements in front of and behind every output (a multiple of 16 bytes in both types)
U_OUT = {"bf16": 2.0 ** -8, "f32": 2.0 ** -23}
EPC = {"bf16": 8, "f32": 4}                # elements of a 16-byte piece
BK = {"bf16": 64, "f32": 32}               # K tile of the implicit GEMM (the pixel range of a weight-gradient split is a multiple)
MASK_VALUES = np.array([-1.0, -0.0, 0.0, 1.0, np.nan], np.float32)


def torch_dtype(d):
    return torch.float32 if d == "f32" else torch.bfloat16


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _t(a):
    return a.double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def round_to(x, dtype):
    """float32 array with the values `dtype` holds (bf16: round to nearest even)"""
    x = np.ascontiguousarray(x, np.float32)
    return x if dtype == "f32" else torch.from_numpy(x).to(torch.bfloat16).float().numpy()


# ============================================================================================ references (float64)
def conv3x3(x, w, bias, dil):
    """x (n, H, W, Cin), w (Cout, Cin, 3, 3), bias (Cout,) or None -> (n, H, W, Cout) float64: stride 1, padding = dilation"""
    x, w = _t(x), _t(w)
    n, H, W, Cin = x.shape
    Cout, d = w.shape[0], int(dil)
    xp = torch.zeros(n, H + 2 * d, W + 2 * d, Cin, dtype=torch.float64)
    xp[:, d:d + H, d:d + W] = x
    out = torch.zeros(n * H * W, Cout, dtype=torch.float64)
    for ty in range(3):
        for tx in range(3):
            out += xp[:, ty * d:ty * d + H, tx * d:tx * d + W].reshape(n * H * W, Cin) @ w[:, :, ty, tx].t()
    if bias is not None:
        out += _t(bias)
    return out.view(n, H, W, Cout).numpy()


def dgrad_weights(w):
    """OIHW of the forward convolution -> OIHW of the convolution that is its data gradient (taps flipped, in / out swapped)"""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def relu_mask(ref):
    """1 where the reference map is > 0 (NaN and -0.0 give 0)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(ref) > 0).astype(np.float64)


def conv_dgrad(dy, w, dil, mask_ref=None, ref_scale=1.0):
    """dy (n, H, W, O), w (O, I, 3, 3) of the forward convolution -> dx (n, H, W, I), times ref_scale where mask_ref (n H W, I) > 0 and
    0 elsewhere"""
    dx = conv3x3(dy, dgrad_weights(w), None, dil)
    if mask_ref is not None:
        dx = dx * ref_scale * relu_mask(mask_ref).reshape(dx.shape)
    return dx


def relu(y):
    return np.maximum(y, 0.0)


def pool_out_hw(H, W):
    return (H - 2) // 2 + 1, (W - 2) // 2 + 1


def maxpool2x2s2(y):
    """(n, H, W, C) -> (n, (H-2)//2+1, (W-2)//2+1, C): a last odd row / column falls in no window"""
    OH, OW = pool_out_hw(y.shape[1], y.shape[2])
    v = y[:, :2 * OH, :2 * OW]
    return np.maximum(np.maximum(v[:, 0::2, 0::2], v[:, 0::2, 1::2]), np.maximum(v[:, 1::2, 0::2], v[:, 1::2, 1::2]))


def wgrad(x, dy, dil):
    """x (n, H, W, Cin), dy (n, H, W, Cout) -> dW (Cout, Cin, 3, 3) float64 = sum over pixels of dy[p][co] * x[p + (tap - 1) dil][ci]"""
    x, dy = _t(x), _t(dy)
    n, H, W, Cin = x.shape
    Cout, d = dy.shape[3], int(dil)
    xp = torch.zeros(n, H + 2 * d, W + 2 * d, Cin, dtype=torch.float64)
    xp[:, d:d + H, d:d + W] = x
    g = dy.reshape(n * H * W, Cout).t().contiguous()
    out = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
    for ty in range(3):
        for tx in range(3):
            out[:, :, ty, tx] = g @ xp[:, ty * d:ty * d + H, tx * d:tx * d + W].reshape(n * H * W, Cin)
    return out.numpy()


def fold(slabs, cout_scale=None, old=None):
    """slabs (nslab, Cout, 9, Cin) -> dW (Cout, Cin, 3, 3) float64: the ordered slab sum, then cout_scale[co], then + old"""
    s = np.asarray(slabs, np.float64)
    tot = np.zeros(s.shape[1:], np.float64)
    for z in range(s.shape[0]):
        tot += s[z]
    Cout, _, Cin = tot.shape
    dw = tot.transpose(0, 2, 1).reshape(Cout, Cin, 3, 3)
    if cout_scale is not None:
        dw = dw * np.asarray(cout_scale, np.float64).reshape(Cout, 1, 1, 1)
    if old is not None:
        dw = dw + np.asarray(old, np.float64)
    return dw


def scaled_f32(exact, cout_scale=None, old=None):
    """what a kernel must store for an exactly summed (integer) gradient: float32(sum) * float32(scale) rounded once, then one float32
    add of the gradient that was there"""
    v = np.asarray(exact, np.float64).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), exact), "the sum is not a float32 number"
    if cout_scale is not None:
        v = v * np.asarray(cout_scale, np.float32).reshape(-1, 1, 1, 1)
    if old is not None:
        v = v + np.asarray(old, np.float32)
    return v.astype(np.float32)


def allowed(ref, S, K, out):
    """per-element bar (module docstring): u_out |ref| + 2 (K + 2) 2^-24 S"""
    return U_OUT[out] * np.abs(ref) + 2.0 * (K + 2) * 2.0 ** -24 * np.asarray(S, np.float64)


def worst(got, ref, S, K, out):
    """max over the elements of |got - ref| / allowed (inf for a non-finite value)"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return math.inf
    a = allowed(ref, S, K, out)
    e = np.abs(got - ref)
    return float(np.max(np.where(e == 0, 0.0, e / np.maximum(a, 1e-300)))) if e.size else 0.0


# ============================================================================================ operands
def density(Cin):
    return min(1.0, 112.0 / Cin)


def int_weights(key, Cout, Cin):
    """(Cout, Cin, 3, 3) in {-1, 0, 1}; every (ci, tap) holds a non-zero weight for some output channel"""
    r = _rng(31, *key, Cout, Cin)
    w = (r.choice([-1.0, 1.0], (Cout, Cin, 3, 3)) * (r.random((Cout, Cin, 3, 3)) < density(Cin))).astype(np.float32)
    dead = np.argwhere(~w.any(axis=0))
    for ci, ty, tx in dead:
        w[(ci + 3 * ty + tx) % Cout, ci, ty, tx] = 1.0 if (ci + tx) % 2 else -1.0
    return w


def int_map(key, shape, lo=-2, hi=2):
    """integers in lo..hi; every pixel (all but the last axis) non-zero in some channel"""
    r = _rng(32, *key, *shape)
    x = r.integers(lo, hi + 1, shape).astype(np.float32)
    flat = x.reshape(-1, shape[-1])
    dead = ~flat.any(axis=1)
    flat[dead, np.arange(flat.shape[0])[dead] % shape[-1]] = 1.0
    return x


def int_bias(key, C):
    return _rng(33, *key, C).integers(-3, 4, C).astype(np.float32)


def mask_ref(key, rows, cols):
    """(rows, cols) float32 from MASK_VALUES, each of the five present"""
    r = _rng(34, *key, rows, cols)
    m = MASK_VALUES[r.integers(0, 5, rows * cols)]
    if m.size >= 5:
        m[r.permutation(m.size)[:5]] = MASK_VALUES
    return m.reshape(rows, cols)


def pow2_scale(key, C):
    r = _rng(35, *key, C)
    return (r.choice([-1.0, 1.0], C) * 2.0 ** r.integers(-3, 3, C)).astype(np.float32)


def general_scale(key, C):
    r = _rng(36, *key, C)
    return ((r.random(C) + 0.5) * r.choice([-1.0, 1.0], C)).astype(np.float32)


def scale_of(kind, key, C):
    return None if kind is None else (pow2_scale(key, C) if kind == "pow2" else general_scale(key, C))


def gauss(key, shape, sigma, dtype="bf16"):
    return round_to(_rng(37, *key, *shape).normal(0.0, sigma, shape), dtype)


# ============================================================================================ the direct kernel: dispatch
TH, TW, CK = 8, 32, 32


def direct_census(n, H, W, Cin, Cout):
    """sw_conv3x3_direct_try + conv3x3_direct_body for a covered shape: the form, channel tile, K groups, work list and its edge forms.
    left_wgs: workgroups on the LEFT form (tx0 + 16 >= W); empty_waves: waves on the EMPTY form (ty0 + 2 * wave >= H, four waves per
    K group); chunks: 32-channel chunks a group walks; idle: launched workgroups without a work item (the XCD map rounds up to 8)"""
    form = conv_direct_form(n, H, W, Cin, Cout)
    assert form in ("kgroup", "fourwave32", "fourwave64")
    kg = 2 if form == "kgroup" else 1
    tn = 32 if form == "fourwave32" else 64
    return _census(n, H, W, Cin, Cout, form, kg, tn)


def _census(n, H, W, Cin, Cout, form, kg, tn):
    tiles_x, tiles_y = -(-W // TW), -(-H // TH)
    n_co = -(-Cout // tn)
    total = tiles_x * tiles_y * n * n_co
    left_cols = sum(1 for tx in range(tiles_x) if tx * TW + 16 >= W)
    empty_rows = sum(1 for ty in range(tiles_y) for wv in range(4) if ty * TH + 2 * wv >= H)
    return dict(form=form, kg=kg, tn=tn, tiles_x=tiles_x, tiles_y=tiles_y, n_co_blocks=n_co, total=total, launched=-(-total // 8) * 8,
                idle=-(-total // 8) * 8 - total, mod8=total % 8, chunks=Cin // (CK * kg), left_wgs=left_cols * tiles_y * n * n_co,
                empty_waves=empty_rows * tiles_x * n * n_co * kg, cout_tail=Cout % tn)


def multi_covered(problems):
    """sw_conv3x3_multi takes the list ((n, H, W, Cin, Cout) each; bf16, dilation 1, unit-scale tight mask): 2 to 8 problems (the
    wrapper launches a single one or more than eight one by one), every Cin a multiple of 32 and >= 64, every Cout a multiple of 8"""
    return 1 < len(problems) <= 8 and all(Cin % 32 == 0 and Cin >= 64 and Cout % 8 == 0 for (_, _, _, Cin, Cout) in problems)


def multi_first(problems):
    """the workgroup-range table of the multi launch: first[i] = start of problem i, ranges rounded up to 8 (64-channel tiles, one
    K group), first[n] = the grid"""
    first, wgs = [], 0
    for (n, H, W, Cin, Cout) in problems:
        first.append(wgs)
        wgs += _census(n, H, W, Cin, Cout, "multi", 1, 64)["launched"]
    return first + [wgs]


def first_layer_counts(n, H, W):
    """conv3x3_first_kernel: 64-pixel row segments, blocks (four segments each, at most 4096), turns of the grid-stride loop"""
    segs = -(-W // 64)
    nseg = n * H * segs
    blocks = min(-(-nseg // 4), 4096)
    return dict(segs=segs, nseg=nseg, blocks=blocks, turns=-(-nseg // (blocks * 4)), last_width=W - (segs - 1) * 64)


def igemm_refusal(dtype, Cin):
    """error code of sw_conv3x3_igemm for a shape (None: it runs): the input channels must fill 16-byte pieces"""
    return 5 if Cin % EPC[dtype] else None


# ============================================================================================ weight gradients: dispatch
def gather_admits(H, W):
    """the guard of the weight-gradient gather: (64 / W) + 1 > 2 * H is refused (code -6)"""
    return not (64 // W + 1 > 2 * H)


def nslab(dtype, n, H, W, nsplit):
    return wgrad_nslab(n * H * W, nsplit, BK[dtype])


def wgrad_direct_taken(dtype, problems):
    """sw_conv3x3_wgrad_direct_try takes the grouped list ((n, H, W, Cin, Cout, dil, nsplit) each): wgrad_direct_covers, and at least
    eight (image, strip, row) steps per effective split"""
    if not wgrad_direct_covers([p[:6] for p in problems], torch_dtype(dtype)):
        return False
    return all(-(-wgrad_direct_steps(n, H, W) // nslab(dtype, n, H, W, ns)) >= 8 for (n, H, W, _, _, _, ns) in problems)


def wgrad_direct_steps(n, H, W):
    return n * (-(-W // 32)) * H


FOLD_MAX = 32
FOLD_UNROLL = 8
SMALL_GRID = 4096 * 256                    # sw_conv3x3_wgrad_small: threads of one grid-stride turn


def fold_accepts(Cin):
    return Cin % 4 == 0 and 36 * Cin <= 65536


def fold_parts(Cin, Cout):
    """input-channel ranges per output channel of the fold, and why the doubling stopped: 'cout' (Cout * parts >= 1024), 'divide'
    (Cin % (8 * parts) != 0) or 'size' (a range would fall below 32 channels)"""
    parts = 1
    while True:
        if Cout * parts >= 1024:
            return parts, "cout"
        if Cin % (parts * 2 * 4):
            return parts, "divide"
        if Cin // (parts * 2) < 32:
            return parts, "size"
        parts *= 2


# ============================================================================================ case tables
# (n, H, W, Cin, Cout, dil)
DIRECT_KGROUP = [(1, 1, 1, 64, 8, 1), (1, 8, 32, 128, 64, 2), (1, 9, 16, 128, 64, 1), (2, 9, 33, 192, 72, 2), (1, 7, 17, 64, 136, 1)]
DIRECT_TILE32 = [(1, 1, 1, 96, 8, 2), (1, 8, 32, 96, 32, 1), (1, 7, 17, 96, 40, 1), (2, 9, 33, 160, 72, 2), (1, 16, 48, 224, 104, 1)]
DIRECT_FOURWAVE64 = [(1, 50, 200, 64, 520, 1), (1, 50, 215, 96, 456, 2), (3, 17, 130, 128, 640, 1)]
DIRECT_FAMILIES = {"kgroup": DIRECT_KGROUP, "fourwave32": DIRECT_TILE32, "fourwave64": DIRECT_FOURWAVE64}
DIRECT_CASES = DIRECT_KGROUP + DIRECT_TILE32 + DIRECT_FOURWAVE64
# the six-product bf16x3 form (f32 operands as three bf16 pieces each, K-concatenated: the kernel's Cin is six times the layer's)
X3_CASES = [(2, 9, 33, 192, 72, 2), (1, 8, 32, 96, 32, 1), (1, 50, 215, 96, 456, 2)]
# one per family and dilation
DIRECT_GAUSS = [(1, 9, 16, 128, 64, 1), (2, 9, 33, 192, 72, 2), (1, 7, 17, 96, 40, 1), (2, 9, 33, 160, 72, 2), (1, 50, 200, 64, 520, 1),
                (1, 50, 215, 96, 456, 2)]


def case_id(c):
    return "x".join(str(v) for v in c)


@functools.lru_cache(maxsize=4)
def direct_int_operands(case):
    """x (n, H, W, Cin), w (Cout, Cin, 3, 3), bias (Cout,), wd (Cin, Cout, 3, 3): OIHW of the forward convolution whose data gradient
    maps Cin -> Cout channels, mask (n H W, Cout)"""
    n, H, W, Cin, Cout, dil = case
    return dict(x=int_map(case, (n, H, W, Cin)), w=int_weights(case + (0,), Cout, Cin), bias=int_bias(case, Cout),
                wd=dgrad_weights(int_weights(case + (1,), Cout, Cin)), mask=mask_ref(case, n * H * W, Cout))


def direct_int_refs(case):
    """float64: plain = conv(x, w), fwd = relu(plain + bias), dgrad = masked data-gradient form"""
    o = direct_int_operands(case)
    plain = conv3x3(o["x"], o["w"], None, case[5])
    return dict(plain=plain, fwd=relu(plain + o["bias"].astype(np.float64)), dgrad=conv_dgrad(o["x"], o["wd"], case[5], o["mask"]))


@functools.lru_cache(maxsize=2)
def direct_gauss_operands(case):
    n, H, W, Cin, Cout, dil = case
    return dict(x=gauss(case, (n, H, W, Cin), 0.7), w=gauss(case + (0,), (Cout, Cin, 3, 3), 0.05),
                bias=gauss(case, (Cout,), 0.1, "f32"), wd=gauss(case + (1,), (Cin, Cout, 3, 3), 0.05),
                mask=gauss(case + (2,), (n * H * W, Cout), 0.5))


def x3_operands(case):
    """f32 operands of the six-product form: x = p + r * 2^-9 (p in -2..2, r in -1..1: two bf16 pieces) with integer weights w, and the
    integer map x_int with weights w2 = w + r * 2^-9: every product is a multiple of 2^-9 and every sum stays below 2^15, so the f32
    result is exact"""
    n, H, W, Cin6, Cout, dil = case
    cin = Cin6 // 6
    x = int_map(case + (6,), (n, H, W, cin)) + _rng(38, *case).integers(-1, 2, (n, H, W, cin)).astype(np.float32) * np.float32(2.0 ** -9)
    w = int_weights(case + (6,), Cout, cin)
    w2 = w + _rng(38, *case, 2).integers(-1, 2, w.shape).astype(np.float32) * np.float32(2.0 ** -9)
    return dict(x=x.astype(np.float32), w=w, bias=int_bias(case + (6,), Cout), mask=mask_ref(case + (6,), n * H * W, Cout),
                x_int=int_map(case + (6,), (n, H, W, cin)), w2=w2.astype(np.float32))


# ---- fused conv + ReLU + pool (dilation 1): (n, H, W, Cin, Cout)
POOL_COVERED = (1, 51, 201, 64, 512)
POOL_REFUSED = [(2, 24, 100, 96, 512), (1, 51, 201, 64, 520)]

# ---- sw_conv3x3_multi: (n, H, W, Cin, Cout, epilogue) with epilogue in 'relu' (bias + ReLU), 'mask', 'plain'; `weight`: problems with
# the same number share one weight
MULTI_8 = [(2, 40, 56, 64, 64, "relu"), (2, 20, 28, 96, 72, "mask"), (2, 10, 14, 128, 8, "plain"), (2, 5, 7, 256, 256, "relu"),
           (1, 1, 1, 64, 8, "mask"), (1, 8, 32, 96, 64, "plain"), (1, 9, 33, 128, 72, "relu"), (3, 7, 17, 256, 8, "mask")]
MULTI_SHARED = [(1, 50, 200, 64, 520, "relu"), (1, 9, 33, 64, 520, "mask")]          # one weight; the first alone is a four-wave launch
MULTI_CIN32 = [(1, 8, 32, 64, 64, "relu"), (1, 9, 33, 32, 64, "relu"), (2, 5, 7, 128, 8, "mask")]
MULTI_9 = MULTI_8 + [(1, 9, 16, 192, 40, "relu")]
MULTI_LISTS = {"eight": MULTI_8, "shared_weight": MULTI_SHARED, "cin32": MULTI_CIN32, "nine": MULTI_9}


def multi_operands(name):
    """per problem: the integer operands of a direct case (dilation 1); the shared list uses one weight and bias"""
    out = []
    for i, (n, H, W, Cin, Cout, epi) in enumerate(MULTI_LISTS[name]):
        key = (n, H, W, Cin, Cout, 1, i)
        wkey = (Cin, Cout, 77) if name == "shared_weight" else key
        out.append(dict(x=int_map(key, (n, H, W, Cin)), w=int_weights(wkey, Cout, Cin), bias=int_bias(wkey, Cout),
                        mask=mask_ref(key, n * H * W, Cout), epi=epi))
    return out


def multi_ref(o):
    y = conv3x3(o["x"], o["w"], None, 1)
    if o["epi"] == "relu":
        return relu(y + o["bias"].astype(np.float64))
    return y * relu_mask(o["mask"]).reshape(y.shape) if o["epi"] == "mask" else y


# ---- first layer (Cin 8, Cout 64, dilation 1): (n, H, W)
FIRST_CASES = [(1, 1, 1), (2, 3, 15), (1, 5, 64), (1, 2, 65), (2, 19, 130), (1, 16500, 5)]
FIRST_CASES_SHAPES = [c + (8, 64) for c in FIRST_CASES]


@functools.lru_cache(maxsize=None)
def first_operands(case):
    n, H, W = case
    x = int_map(case + (8,), (n, H, W, 8))
    x[x == 0] = 1.0                                   # all eight input channels non-zero
    return dict(x=x, w=int_weights(case + (8,), 64, 8), bias=int_bias(case + (8,), 64))


# ---- implicit-GEMM fallback
IGEMM_BF16_CH = [(8, 32), (16, 24), (32, 64), (48, 40), (72, 64), (64, 12)]
IGEMM_MAPS = [(1, 1, 1), (1, 3, 70), (2, 19, 23)]
IGEMM_VARIANTS = ("relu", "pitched_mask", "ref_scale", "dil2")
IGEMM_REFUSED_BF16 = (2, 5, 7, 12, 16)               # (n, H, W, Cin, Cout): Cin is no multiple of 8
IGEMM_DIRECT_SHAPE = (1, 9, 33, 64, 64)                 # covered by the direct kernel, but for its epilogue
IGEMM_F32_CIN = [4, 12, 32, 36, 64]
IGEMM_F32_COUT = [4, 20, 64]
IGEMM_F32_MAP = (2, 7, 19)
REF_PITCH_ADD = 8                                     # a mask whose row pitch is Cout + 8


def igemm_operands(n, H, W, Cin, Cout):
    key = (n, H, W, Cin, Cout, 5)
    return dict(x=int_map(key, (n, H, W, Cin)), w=int_weights(key, Cout, Cin), bias=int_bias(key, Cout),
                mask=mask_ref(key, n * H * W, Cout))


def igemm_ref(o, variant, dil):
    y = conv3x3(o["x"], o["w"], None, dil)
    if variant == "relu":
        return relu(y + o["bias"].astype(np.float64))
    if variant == "pitched_mask":
        return y * relu_mask(o["mask"]).reshape(y.shape)
    if variant == "ref_scale":
        return 0.5 * y * relu_mask(o["mask"]).reshape(y.shape)
    return y


# ---- weight gradients.  sw_conv3x3_wgrad: (n, H, W, Cin, Cout, dil, splits, scale kind, accumulate)
WGRAD_CASES = [(2, 19, 23, 64, 128, 1, 3, "pow2", True), (1, 33, 1, 8, 8, 1, 1, None, False), (1, 5, 13, 16, 24, 2, 2, "general", False),
               (1, 5, 13, 16, 24, 1, 40, None, True), (2, 19, 23, 64, 128, 2, 1, None, False)]
WGRAD_REFUSED = (1, 32, 1, 8, 8, 1)
# grouped: (n, H, W, Cin, Cout, dil, nsplit)
GROUPED_DIRECT = [(1, 8, 1, 64, 64, 1, 1), (1, 8, 33, 64, 128, 2, 1), (2, 12, 70, 128, 64, 2, 4)]
GROUPED_IGEMM = [("bf16", (1, 7, 40, 64, 64, 1, 1)), ("bf16", (1, 8, 33, 64, 72, 1, 1)), ("f32", (1, 8, 33, 64, 64, 1, 2)),
                 ("bf16", (1, 8, 33, 64, 64, 1, 3))]                # H < 8; Cout 72; f32; six steps per split
WGRAD_GAUSS = (2, 19, 23, 64, 128, 1, 3)
GROUPED_GAUSS = (2, 12, 70, 128, 64, 2, 4)


def wgrad_operands(case, gaussian=False, dtype="bf16"):
    n, H, W, Cin, Cout = case[:5]
    if gaussian:
        return gauss(case[:6], (n, H, W, Cin), 0.7, dtype), gauss(case[:6] + (1,), (n, H, W, Cout), 0.5, dtype)
    return int_map(case[:6], (n, H, W, Cin)), int_map(case[:6] + (1,), (n, H, W, Cout))


def old_gradient(key, shape):
    """the gradient that `accumulate` adds to: integers in -8..8"""
    return _rng(39, *key).integers(-8, 9, shape).astype(np.float32)


# sw_conv3x3_wgrad_small: maps x images, odd channel counts; one list above one grid-stride turn
SMALL_MAPS = [(1, 1), (1, 5), (2, 2), (4, 4), (7, 3)]
SMALL_N = (1, 2)
SMALL_CIN, SMALL_COUT = 12, 20                       # a bf16 row of 12 channels is no whole number of 16-byte pieces
SMALL_LARGE = (1, 1, 1, 1028, 1024)                  # (n, H, W, Cin, Cout): Cout * Cin threads > 4096 x 256

# sw_conv3x3_wgrad_fold: (nslab, Cin, Cout, scale kind, accumulate)
FOLD_CASES = [(1, 64, 8, None, False), (7, 64, 8, "pow2", False), (8, 64, 8, None, True), (9, 64, 8, "pow2", True), (16, 64, 8, None, False),
              (17, 64, 8, "general", True), (3, 4, 1024, None, False), (3, 8, 64, "pow2", False), (9, 36, 8, None, True),
              (3, 72, 8, None, False), (9, 128, 8, "pow2", True), (9, 256, 1, None, False), (3, 256, 64, None, True),
              (2, 256, 1024, "pow2", False), (3, 256, 256, None, False), (9, 1820, 1, None, True), (2, 1820, 8, "pow2", False),
              (2, 64, 1024, None, False)]
FOLD_REFUSED_CIN = 1824
FOLD_MULTI = [((4, 64, 256, 36, 72)[i % 5], (8, 1, 64)[i % 3], (1, 3, 9)[(i // 3) % 3]) for i in range(35)]          # (Cin, Cout, nslab)


def fold_slabs(key, nslab_, Cin, Cout):
    """(nslab, Cout, 9, Cin) integers in -3..3"""
    return _rng(40, *key, nslab_, Cin, Cout).integers(-3, 4, (nslab_, Cout, 9, Cin)).astype(np.float32)


# sw_conv_weight_prep: (Cout, Cin, cin_pad for mode 0)
PREP_CASES = [(8, 64, 64), (72, 96, 104), (5, 3, 8), (64, 8, 8)]

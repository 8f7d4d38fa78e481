"""Plain restatements of the pooling, layout, optimizer and scalar kernels of csrc/elementwise.hip, the case tables of
tests/test_gpu_elementwise_kernels.py and the tolerance rules those tests read.  Checkers, not product code; CPU only.

Every reference takes the float32 values the kernel gets (for bf16: rounded to bf16 first).  Selections, copies, casts, one rounded
product, the EMA (two rounded products, one add) and the up-to-four-term sum of the stride-1 pool backward (float32, in the kernel's
window order) are compared bit for bit.  The optimizer is compared with float64: see sgd_bounds.  tests/test_elementwise_ref_cpu.py
pins each restatement to torch (max_pool2d forward and backward, F.relu, .to(bfloat16), torch.optim.SGD in float64, permute
expressions, oracle.semisup_oracle.update_teacher) and asserts that each case table reaches the edge it is named for.

rel_err, the bf16 rounding helpers and the sentinel convention (outputs pre-filled with a NaN payload no kernel writes, SLACK elements behind
the end, asserted untouched) are those of tests/detector_ref.py.
"""
import functools

import numpy as np

from detector_ref import DTYPES, ESIZE, SLACK, VEC, _rng, rel_err, round_to, same_bits, torch_dtype  # noqa: F401  (re-exported to the tests)

GRID_CAP = 2048 * 256                      # grid_for: at most 2048 blocks of 256 threads; more work items take a second grid-stride pass
F32_MIN_NORMAL = np.float32(2.0 ** -126)
F32_MAX = np.float32(np.finfo(np.float32).max)


def bits(x):
    """the int32 bit patterns of a float32 array"""
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def is_subnormal(x):
    x = np.asarray(x, np.float32)
    return (np.abs(x) < F32_MIN_NORMAL) & (x != 0)


# ============================================================================================ the value set of every cast
def cast_values():
    """float32: halfway between two bf16 neighbours (rounding down to even: 1 + 2^-8 -> 1; up to even: 1.0078125 + 2^-8 -> 1.015625;
    both signs), the largest finite float32 (-> inf), +-0, +-inf, NaN, three float32 subnormals (the last is halfway between two bf16
    subnormals)"""
    f = np.float32
    return np.array([f(1.0) + f(2.0 ** -8), f(1.0078125) + f(2.0 ** -8), -(f(1.0) + f(2.0 ** -8)), -(f(1.0078125) + f(2.0 ** -8)),
                     F32_MAX, 0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -149, -(2.0 ** -130), 2.0 ** -127 + 2.0 ** -133 + 2.0 ** -134], np.float32)


N_CAST_VALUES = 13
N_CAST_NORMAL = 10                         # the first ten are no subnormals


def cast_matrix(tag, rows, cols, pitch):
    """-> (rows, pitch) float32: N(0, 1) times a log-normal magnitude, the value set in the first elements of the row-major (rows, cols)
    part, NaN in the padding columns (never read)"""
    r = _rng(91, tag, rows, cols, pitch)
    m = np.full((rows, pitch), np.nan, np.float32)
    v = (r.normal(0.0, 1.0, (rows, cols)) * np.exp(r.normal(0.0, 2.0, (rows, cols)))).astype(np.float32)
    cv = cast_values()
    flat = v.reshape(-1)
    flat[: min(flat.size, cv.size)] = cv[: flat.size]
    m[:, :cols] = flat.reshape(rows, cols)
    return m


# ============================================================================================ 2x2 max pool
POOL_N = 2
POOL_HW = [(2, 2), (3, 3), (5, 4), (4, 7)]
POOL_STRIDES = (1, 2)
POOL_C = [8, 12, 5]
POOL_REGIMES = ("finite", "inf", "nan")    # the backward with relu_mask = 1 takes the first two
# (H, W, stride, C, misaligned): every shape, plus C = 8 on a base one element into a buffer (the scalar form with C % vn == 0)
POOL_CASES = [(H, W, s, C, False) for (H, W) in POOL_HW for s in POOL_STRIDES for C in POOL_C] + \
             [(H, W, s, 8, True) for (H, W) in POOL_HW for s in POOL_STRIDES]


def pool_out_hw(H, W, stride):
    return (H - 2) // stride + 1, (W - 2) // stride + 1


def pool_fwd_form(C, dtype, misaligned):
    return "vector" if (C % VEC[dtype] == 0 and not misaligned) else "scalar"


def pool_bwd_form(C, dtype, stride, misaligned):
    if C % VEC[dtype] == 0 and not misaligned:
        return "window" if stride == 2 else "vector"
    return "scalar"


@functools.lru_cache(maxsize=None)
def pool_inputs(H, W, C, dtype, regime):
    """(2, H, W, C) float32 (values of `dtype`), signed.  Image 1: channel 1 all ties, channel 2 zeros of both signs (+0 first in one
    window, -0 first in its neighbour), channel 3 all negative; "inf": +-inf sprinkled, channel 4 of image 1 all -inf; "nan": NaN at
    window position k of the top-left window in channel k of image 0, at positions 0 and 3 in channel 4, at 1 and 2 in channel 0 of
    image 1"""
    r = _rng(92, H, W, C, POOL_REGIMES.index(regime))
    x = r.normal(0.0, 1.0, (POOL_N, H, W, C)).astype(np.float32)
    x[1, :, :, 1] = 0.5
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    x[1, :, :, 2] = np.where((yy + xx + xx // 2) % 2 == 0, 0.0, -0.0)                  # also at stride 2: windows that start with -0
    x[1, H - 1, W - 1, 2] = -1.0
    x[1, :, :, 3] = -np.abs(x[1, :, :, 3]) - 0.5
    if regime in ("inf", "nan"):
        k = r.integers(0, 12, x.shape)
        k[1, :, :, 1:4] = 5
        x[k == 0] = np.inf; x[k == 1] = -np.inf
        x[1, :, :, 4] = -np.inf
    if regime == "nan":
        for pos in range(4):
            x[0, pos >> 1, pos & 1, pos] = np.nan
        x[0, 0, 0, 4] = x[0, 1, 1, 4] = np.nan
        x[1, 0, 1, 0] = x[1, 1, 0, 0] = np.nan
    return round_to(x, dtype)


@functools.lru_cache(maxsize=None)
def pool_dout(H, W, C, stride, dtype):
    OH, OW = pool_out_hw(H, W, stride)
    return round_to(_rng(93, H, W, C, stride).normal(0.0, 1.0, (POOL_N, OH, OW, C)), dtype)


def _pool_windows(x, stride):
    """-> (4, N, OH, OW, C): the window elements in scan order (0,0), (0,1), (1,0), (1,1)"""
    N, H, W, C = x.shape
    OH, OW = pool_out_hw(H, W, stride)
    return np.stack([x[:, dy:dy + stride * (OH - 1) + 1:stride, dx:dx + stride * (OW - 1) + 1:stride] for dy in (0, 1) for dx in (0, 1)])


def maxpool_fwd_ref(x, stride):
    """x (N, H, W, C) float32 -> (values (N, OH, OW, C) float32, window position 0..3 of the selected element): start from the first
    element, take v where v > max or v is NaN (aten MaxPoolKernel.cpp) — the last NaN in scan order, else the first maximum"""
    w = _pool_windows(np.asarray(x, np.float32), stride)
    m = w[0].copy(); am = np.zeros(m.shape, np.int64)
    for k in (1, 2, 3):
        with np.errstate(invalid="ignore"):
            take = (w[k] > m) | np.isnan(w[k])
        m = np.where(take, w[k], m); am = np.where(take, k, am)
    return m, am


def maxpool_bwd_ref(x, dout, stride, relu_mask, dtype):
    """-> din (N, H, W, C) float32 (values of `dtype`): every window's dout goes to the element maxpool_fwd_ref selects; a pixel's
    (up to four, stride 1) terms are added in float32 from 0 in the order (oy, ox) ascending and rounded once; relu_mask: 0 where not
    x > 0; pixels of the odd last row / column that no window holds get 0"""
    x = np.asarray(x, np.float32); dout = np.asarray(dout, np.float32)
    N, H, W, C = x.shape
    OH, OW = pool_out_hw(H, W, stride)
    _, am = maxpool_fwd_ref(x, stride)
    din = np.zeros((N, H, W, C), np.float32)
    n_i, c_i = np.meshgrid(np.arange(N), np.arange(C), indexing="ij")
    for oy in range(OH):
        for ox in range(OW):
            a = am[:, oy, ox, :]
            din[n_i, oy * stride + (a >> 1), ox * stride + (a & 1), c_i] += dout[:, oy, ox, :]
    if relu_mask:
        with np.errstate(invalid="ignore"):
            din = np.where(x > 0, din, np.float32(0.0))
    return round_to(din, dtype)


# ============================================================================================ relu_bwd
RELU_N = [1, 7, 8, 9, 4104]
RELU_SPECIALS = np.array([F32_MIN_NORMAL, np.nan, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0], np.float32)     # all exact in bf16


def relu_bwd_form(n, dtype, misaligned):
    return "vector" if (n % VEC[dtype] == 0 and not misaligned) else "scalar"


@functools.lru_cache(maxsize=None)
def relu_inputs(n, dtype):
    """-> ref, g float32 (values of `dtype`): ref cycles through RELU_SPECIALS in its first 16 elements (n = 1: the smallest positive
    normal), g holds a NaN, a -0 and an inf among them"""
    r = _rng(94, n)
    ref = round_to(r.normal(0.0, 1.0, n), dtype); g = round_to(r.normal(0.0, 1.0, n), dtype)
    k = min(n, 16)
    ref[:k] = np.resize(RELU_SPECIALS, k)
    if n >= 7:
        g[0] = np.nan; g[4] = -0.0; g[6] = np.inf; g[1] = np.inf; g[2] = np.nan
    return ref, g


def relu_bwd_ref(ref, g):
    """the documented rule `ref > 0 ? g : 0` on bit patterns (g passes with its bits; a NaN ref gives +0)"""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(ref, np.float32) > 0, bits(g), 0).astype(np.int32)


# ============================================================================================ conversions and layouts
CONVERT_SHAPES = [(3, 5), (3, 8), (64, 4)]
CONVERT_PITCH_ADD = (0, 4, 3)              # tight, padded with % 4 kept (where cols % 4 == 0), padded off % 4
# (rows, cols, ld_src, ld_dst, src misaligned, dst misaligned)
CONVERT_CASES = [(r, c, c + ps, c + pd, ms, md) for (r, c) in CONVERT_SHAPES for ps in CONVERT_PITCH_ADD for pd in CONVERT_PITCH_ADD
                 for ms in (0, 1) for md in (0, 1)]


def convert_2d_form(cols, ld_src, ld_dst, src_mis, dst_mis):
    """sw_convert_2d's dispatch: 4 columns per thread when everything is a multiple of 4 and both bases are aligned (src to 16 bytes,
    dst to 4 elements: 8 bytes of bf16, 16 of f32); a base `mis` elements into an aligned buffer is aligned iff mis % 4 == 0"""
    return "vec4" if (cols % 4 == 0 and ld_src % 4 == 0 and ld_dst % 4 == 0 and src_mis % 4 == 0 and dst_mis % 4 == 0) else "scalar"


CONVERT_FLAT_SHAPES = [(3, 5), (3, 8), (64, 4), (2, 3, 8), (13,)]

# (rows, cols, ld_dst - rows): rows + 8 keeps every bf16 row 16-byte aligned, rows + 4 puts the odd ones 8 bytes off
CONVERT_T_CASES = [(64, 64, 8), (64, 64, 4), (128, 64, 8), (128, 64, 4)]


def convert_t_row_forms(rows, ld_dst, dtype):
    """the store branch of each destination row: 16-byte row pieces (bf16 rows that start on 16 bytes) or element by element"""
    if dtype != "bf16":
        return {"scalar"}
    return {"vector" if (c * ld_dst * 2) % 16 == 0 else "scalar" for c in range(64)}


WEIGHT_PREP_SHAPES = [(5, 3), (64, 32)]
WEIGHT_PREP_PADS = {(5, 3): (3, 8), (64, 32): (32, 40)}          # mode 0: cin_pad = Cin and a padded one


def weight_matrix(tag, shape):
    r = _rng(95, tag, *shape)
    w = (r.normal(0.0, 1.0, shape) * np.exp(r.normal(0.0, 2.0, shape))).astype(np.float32)
    cv = cast_values()
    flat = w.reshape(-1)
    flat[: min(flat.size, cv.size)] = cv[: flat.size]
    return w


def weight_prep_ref(w, mode, cin_pad=None):
    """w (Cout, Cin, 3, 3).  mode 0: wk[co][tap][ci] (ci < cin_pad, zero beyond Cin); mode 1: wk[ci][8 - tap][co]"""
    Cout, Cin = w.shape[:2]
    w9 = np.asarray(w, np.float32).reshape(Cout, Cin, 9)
    if mode == 0:
        out = np.zeros((Cout, 9, Cin if cin_pad is None else cin_pad), np.float32)
        out[:, :, :Cin] = w9.transpose(0, 2, 1)
        return out
    return np.ascontiguousarray(w9[:, :, ::-1].transpose(1, 2, 0))


def weight_prep_loops(w, mode, cin_pad=None):
    """the same index by index, as the header states the layouts (pins the vector form on small shapes)"""
    Cout, Cin = w.shape[:2]
    out = np.zeros((Cout, 9, Cin if cin_pad is None else cin_pad), np.float32) if mode == 0 else np.zeros((Cin, 9, Cout), np.float32)
    for co in range(Cout):
        for ci in range(Cin):
            for tap in range(9):
                if mode == 0:
                    out[co, tap, ci] = w[co, ci, tap // 3, tap % 3]
                else:
                    out[ci, 8 - tap, co] = w[co, ci, tap // 3, tap % 3]
    return out


NCHW_SHAPE = (2, 3, 3, 5)
NCHW_CPADS = (3, 4, 8)


def nchw_to_nhwc_ref(x, cpad):
    N, C, H, W = x.shape
    out = np.zeros((N, H, W, cpad), np.float32)
    for c in range(C):
        out[..., c] = x[:, c]
    return out


SCALE_COLS_CASES = [(5, 7, 9, 12), (64, 8, 12, 8), (64, 8, 8, 11)]            # (M, N, ld_in, ld_out)


def scale_cols_inputs(M, N, ld_in):
    """-> in (M, ld_in) float32 (the value set in front: subnormal inputs and subnormal products; NaN in the padding), colscale (N,)
    with 1 in column 0"""
    src = cast_matrix(96, M, N, ld_in)
    cs = _rng(96, M, N).uniform(0.3, 1.7, N).astype(np.float32) * np.where(np.arange(N) % 3 == 2, -1, 1).astype(np.float32)
    cs[0] = 1.0
    return src, cs


def scale_cols_ref(src, cs, N):
    """one float32 product (then rounded to the output type by the caller)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(src, np.float32)[:, :N] * np.asarray(cs, np.float32)[None, :]


SPLIT_SHAPES = [(3, 8), (64, 4)]
SPLIT_PATTERNS = {0: (0, 0, 1, 0, 1, 2), 1: (0, 1, 0, 2, 1, 0)}             # [a1|a1|a2|a1|a2|a3] / [b1|b2|b1|b3|b2|b1]
# (rows, cols, side, along_rows)
SPLIT_CASES = [(r, c, side, ar) for (r, c) in SPLIT_SHAPES for side in (0, 1) for ar in (0, 1)]


def split_pieces_ref(a):
    """a float32 -> three float32 arrays holding bf16 values: a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2), both
    differences float32 subtractions (exact for finite normal inputs)"""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a1 = round_to(a, "bf16"); r1 = a - a1
        a2 = round_to(r1, "bf16"); r2 = r1 - a2
        a3 = round_to(r2, "bf16")
    return a1, a2, a3


def split_layout_ref(a, side, along_rows):
    """-> (rows, 6 cols) or, along_rows, (6 rows, cols): block p holds piece SPLIT_PATTERNS[side][p]"""
    pieces = split_pieces_ref(a)
    return np.concatenate([pieces[k] for k in SPLIT_PATTERNS[side]], axis=0 if along_rows else 1)


# ============================================================================================ optimizer
SGD_MAX_TENSORS = 24                       # SW_SGD_MAX_TENSORS: entries of one launch
SGD_CHUNK = 4096
SGD_ELEMENT_N = [1, 4095, 4096, 4097, 8195]
U32 = 2.0 ** -24                           # float32 unit roundoff


def sgd_entries():
    """the 28 entries (two launches) as dicts: name, shape of the parameter, mis (float32 elements in front of the 16-byte boundary),
    kind, and the staging geometry.  s0 / s1: which copies exist.  Index 23 (the last of the first launch's range) is a kind-3 entry."""
    E = []
    for n in SGD_ELEMENT_N:
        E.append(dict(name=f"el{n}", shape=(n,), mis=0, kind=0))
    for n in SGD_ELEMENT_N:
        E.append(dict(name=f"el{n}+12B", shape=(n,), mis=3, kind=0))
    # (a bf16 row pitch of 76 elements is 152 bytes: every row still starts on 8 bytes; 74 puts the odd rows 4 bytes off)
    for ld0 in (72, 80, 76, 74):
        E.append(dict(name=f"k1-72/{ld0}", shape=(11, 72), mis=0, kind=1, d0=72, ld0=ld0))
    E.append(dict(name="k1-1001", shape=(3, 1001), mis=0, kind=1, d0=1001, ld0=1004))
    E.append(dict(name="k1-f32", shape=(11, 72), mis=0, kind=1, d0=72, ld0=80, f32=True))
    E.append(dict(name="k2-40x24", shape=(40, 24, 3, 3), mis=0, kind=2, d0=40, d1=24, d2=24, s0=True, s1=True))
    E.append(dict(name="zero", shape=(0,), mis=0, kind=0))
    for (co, ci, d2, forms) in ((64, 32, 32, ("s0", "s1", "s01")), (32, 96, 96, ("s0", "s1", "s01")), (96, 64, 72, ("s0", "s01"))):
        for f in forms:
            E.append(dict(name=f"k2-{co}x{ci}/{d2}-{f}", shape=(co, ci, 3, 3), mis=0, kind=2, d0=co, d1=ci, d2=d2, s0="0" in f, s1="1" in f))
    k3a = dict(name="k3-64x128", shape=(64, 128), mis=0, kind=3, d0=128, ld0=128 + 8, ld1=64 + 8)
    k3b = dict(name="k3-128x192", shape=(128, 192), mis=0, kind=3, d0=192, ld0=192 + 2, ld1=128 + 4)
    E.insert(23, k3a)
    E.append(k3b)
    return E


def sgd_form(e):
    """which code updates the entry: 'tile64' (kind 3), 'conv_tile' (kind 2 with Cout, Cin multiples of 32), else 'vector' (all
    three float32 arrays on 16 bytes) or 'scalar'"""
    if e["kind"] == 3:
        return "tile64"
    if e["kind"] == 2 and e["d0"] % 32 == 0 and e["d1"] % 32 == 0:
        return "conv_tile"
    return "vector" if e["mis"] % 4 == 0 else "scalar"


def stage_row_forms(e, dtype):
    """the store branches the rows of a row-major bf16 copy take: kind 1 in the vector form (d0 % 4 == 0) and kind 3 store 4 columns
    as 8 bytes where the row starts on 8 bytes, else element by element"""
    rows = e["shape"][0]
    if dtype != "bf16" or e.get("f32") or e["d0"] % 4:
        return {"scalar"}
    return {"8B" if (r * e["ld0"] * 2) % 8 == 0 else "scalar" for r in range(rows)}


def sgd_hyper(i):
    """(lr, weight_decay) host fields of entry i, and the different pair a device tensor gives instead"""
    lr, wd = 0.01 * (1 + i % 3), 5e-4 * (i % 2)
    return (lr, wd), (0.5 * lr + 0.001, wd + 1e-4)


def sgd_ref(w, g, buf, lr, wd, mom, gscale, first):
    """float64 torch.optim.SGD step from the float32 state, the hyper-parameters rounded to float32 first (the kernel receives
    floats): d = g * gscale + wd * w; buf = first ? d : mom * buf + d; p = w - lr * buf.  -> (p, buf, S) with
    S = mom |buf| + |g gscale| + wd |w| (no buffer term on a first step)"""
    lr, wd, mom, gscale = (float(np.float32(v)) for v in (lr, wd, mom, gscale))
    w = np.asarray(w, np.float64); g = np.asarray(g, np.float64)
    d = g * gscale + wd * w
    S = np.abs(g * gscale) + wd * np.abs(w)
    if first:
        b = d
    else:
        buf = np.asarray(buf, np.float64)
        b = mom * buf + d
        S = S + mom * np.abs(buf)
    return w - lr * b, b, S


def sgd_bounds(w, S, lr):
    """allowed |buf - ref| and |p - ref| per element, from the operation count: the buffer is three products and two sums (each
    within u of its exact value, the errors of the inner ones amplified by at most 1): <= 4 u S; the parameter adds one product and
    one difference: <= u (6 lr S + 2 |w|).  Holds with and without fused multiply-add (checked on 2e6 heavy-tailed samples: worst
    error / bound 0.65)."""
    lr = float(np.float32(lr))
    return 4 * U32 * S, U32 * (6 * lr * S + 2 * np.abs(np.asarray(w, np.float64)))


def sgd_f32(w, g, buf, lr, wd, mom, gscale, first, fma=False):
    """the kernel's formula in float32 (optionally with the products fused into the sums): what sgd_bounds must cover"""
    f = np.float32
    w = np.asarray(w, f); g = np.asarray(g, f); lr, wd, mom, gscale = f(lr), f(wd), f(mom), f(gscale)
    if not fma:
        d = g * gscale + wd * w
        b = d if first else mom * np.asarray(buf, f) + d
        return w - lr * b, b
    d = (g.astype(np.float64) * float(gscale)).astype(f).astype(np.float64) + float(wd) * w.astype(np.float64)
    d = d.astype(f)
    b = d if first else (float(mom) * np.asarray(buf, np.float64) + d.astype(np.float64)).astype(f)
    return (w.astype(np.float64) - float(lr) * b.astype(np.float64)).astype(f), b


def sgd_state(i, e, step):
    """-> w, g, buf float32 of entry i: heavy-tailed (normal times log-normal)"""
    r = _rng(97, i, step)
    def draw():
        return (r.normal(0.0, 1.0, e["shape"]) * np.exp(r.normal(0.0, 1.5, e["shape"]))).astype(np.float32)
    return draw(), draw(), draw()


def stage_kind2_ref(p, d2):
    """p (Cout, Cin, 3, 3) -> stage0 [co][tap][ci] in a (Cout, 9, d2) block (NaN = not written), stage1 [ci][8 - tap][co]"""
    Cout, Cin = p.shape[:2]
    s0 = np.full((Cout, 9, d2), np.nan, np.float32)
    s0[:, :, :Cin] = weight_prep_ref(p, 0)
    return s0, weight_prep_ref(p, 1)


# ============================================================================================ EMA
EMA_COUNT = 50                             # EMA_MAX = 48 tensors per launch
EMA_SIZES = (1, 4095, 4096, 4097, 0)
EMA_KEEPS = (0.9996, 0.0, 1.0)
EMA_INF_AT = (3, 17)                       # (tensor, element): an inf teacher entry


def ema_inputs():
    r = _rng(98)
    te = [r.normal(0.0, 1.0, EMA_SIZES[i % 5]).astype(np.float32) for i in range(EMA_COUNT)]
    st = [r.normal(0.0, 1.0, EMA_SIZES[i % 5]).astype(np.float32) for i in range(EMA_COUNT)]
    te[EMA_INF_AT[0]][EMA_INF_AT[1]] = np.inf
    return te, st


def ema_ref(teacher, student, keep):
    """float32: student * f32(1 - keep) + teacher * f32(keep), two rounded products and one add"""
    k, omk = np.float32(keep), np.float32(1.0 - keep)
    with np.errstate(invalid="ignore"):
        return [(s * omk + t * k).astype(np.float32) for t, s in zip(teacher, student)]


# ============================================================================================ scalars and packing
WS_MAX = 32
WS_N = [1, 3, 32]


def weighted_sum_inputs(n):
    """values (1e8, 1, -1e8, 3, ...) with weight 1 in front (only the left-to-right float32 order gives 3), random pairs behind"""
    r = _rng(99, n)
    v = r.normal(0.0, 1.0, n).astype(np.float32); w = r.uniform(0.1, 2.0, n).astype(np.float32)
    head = np.array([1e8, 1.0, -1e8, 3.0], np.float32)
    if n >= 3:
        k = min(n, 4)
        v[:k] = head[:k]; w[:k] = 1.0
    return v, w


def weighted_sum_ref(v, w):
    """-> float32 (n + 1,): the rounded products, then ((p0 + p1) + p2) + ... in float32"""
    p = (np.asarray(v, np.float32) * np.asarray(w, np.float32)).astype(np.float32)
    s = p[0]
    for x in p[1:]:
        s = np.float32(s + x)
    return np.concatenate([p, [s]]).astype(np.float32)


COUNTER_CASES = [(2 ** 32 - 5, 10), (2 ** 64 - 3, 10), (0, 2 ** 63 + 1), (2 ** 63, 2 ** 63)]      # (start, increment)

DROPOUT_N = [1000, 70001]
DROPOUT_P = (0.0, 0.3, 1.0)
DROPOUT_SEEDS = (0x1234567, 2 ** 63 + 0xABCDEF0123)
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def dropout_ref(n, seed, offset, p):
    """keep[i] = u_i >= p, u_i = (splitmix64(splitmix64(seed) + offset + i) >> 40) / 2^24 (exact in float32), all modulo 2^64"""
    with np.errstate(over="ignore"):
        s = _splitmix64(np.array([seed & _M64], np.uint64))[0]
        z = _splitmix64(s + np.uint64(offset & _M64) + np.arange(n, dtype=np.uint64))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (u >= np.float32(p)).astype(np.uint8)


def splitmix64_int(x):
    """the same on Python integers (pins the numpy form)"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


PACK_R = [1, 64, 257]


def pack_views_ref(boxes4, obj4):
    """4 x (R, 4), 4 x (R,) -> boxes (4, R, 4), obj (4, R), rois (2, 2R, 5): scale s holds view 2s with batch index 0 in rows
    [0, R) and view 2s + 1 with batch index 1 in rows [R, 2R)"""
    R = boxes4[0].shape[0]
    rois = np.zeros((2, 2 * R, 5), np.float32)
    for s in range(2):
        for b in range(2):
            rois[s, b * R:(b + 1) * R, 0] = b
            rois[s, b * R:(b + 1) * R, 1:] = boxes4[2 * s + b]
    return np.stack(boxes4), np.stack(obj4), rois


# ============================================================================================ grid-stride second pass
# work items just over GRID_CAP: pool forward (vector form, bf16: 8 channels per item), relu_bwd (vector form, f32: 4 per item),
# convert_2d (4 columns per item)
GRID_POOL = dict(N=8193, H=2, W=128, C=8, stride=2, dtype="bf16")
GRID_RELU_N = 4 * (GRID_CAP + 37)
GRID_CONVERT = (1025, 2048)


def grid_items():
    p = GRID_POOL
    OH, OW = pool_out_hw(p["H"], p["W"], p["stride"])
    return dict(pool=p["N"] * OH * OW * p["C"] // VEC[p["dtype"]], relu=GRID_RELU_N // VEC["f32"], convert=GRID_CONVERT[0] * GRID_CONVERT[1] // 4)


# ============================================================================================ NaN through the forward ReLU / max sites
# One case per forward site of conv_direct.hip / gemm.hip that applied fmaxf.  Conv: (n, H, W, Cin, Cout, out dtype); the direct
# kernel's form is restated by conv_direct_form.  GEMM: rows of the tile-form edge table of tests/test_gpu_kernels.py.
NAN_CONV_CASES = {
    "first_layer": (2, 19, 23, 8, 64, "bf16"),               # conv3x3_first_kernel (Cin padded to 8, Cout 64)
    "kgroup_bf16": (1, 9, 16, 128, 64, "bf16"),              # two K groups, bf16 epilogue
    "kgroup_f32": (1, 9, 16, 128, 64, "f32"),                # two K groups, f32 epilogue
    "fourwave_bf16": (1, 9, 16, 96, 64, "bf16"),             # four waves (an odd number of 32-channel chunks), bf16 epilogue
    "fourwave_f32": (1, 9, 16, 96, 64, "f32"),               # four waves, f32 epilogue
}
NAN_POOL_CASE = (1, 56, 224, 64, 512)                        # sw_conv3x3_relu_pool2: > 384 workgroups (7 x 7 pixel tiles x 8 channel blocks)
NAN_KINDS = ("nan_input", "inf_times_zero", "nan_bias")


def conv_direct_form(n, H, W, Cin, Cout):
    """sw_conv3x3_direct_try: 'first' (Cin 8, Cout 64), None (not covered), else 'kgroup' (few tiles, an even number of 32-channel
    chunks), 'fourwave32' (few tiles otherwise: 32-channel tiles) or 'fourwave64'"""
    if Cin == 8 and Cout == 64:
        return "first"
    if Cin % 32 or Cout % 8 or Cin < 64:
        return None
    px = ((W + 31) // 32) * ((H + 7) // 8) * n
    few = px * ((Cout + 63) // 64) <= 384
    if few and Cin % 64 == 0:
        return "kgroup"
    return "fourwave32" if few else "fourwave64"


def pool_fused_covered(n, H, W, Cin, Cout):
    """sw_conv3x3_relu_pool2 takes the launch (more than 384 workgroups of 8 x 32 pixels x 64 channels)"""
    if Cin % 32 or Cin < 64 or Cout % 64 or H < 2 or W < 2:
        return False
    return ((W + 31) // 32) * ((H + 7) // 8) * n * (Cout // 64) > 384


# (site, M, N, K, input dtype, output dtype, split-K): the ping-pong form's row-wise epilogue, the register epilogue of the other
# forms, the split-K fold with an epilogue
NAN_GEMM_CASES = [("pp256", 3841, 3583, 1024, "bf16", "bf16", 1), ("256x64", 8193, 61, 1048, "bf16", "bf16", 1),
                  ("fold", 300, 1028, 4096, "bf16", "bf16", 4)]


def gemm_relu_site(M, N, K, in_dtype, splitk, bias_or_relu=True):
    """which ReLU epilogue of gemm.hip a K-contiguous (A [M][K], B [N][K]) GEMM with bias + ReLU reaches, restating sw_gemm and
    launch_auto: 'fold' (split-K with an epilogue and a workspace, which ops.gemm allocates: the slabs are plain, the fold applies the
    epilogue; needs N % 4 == 0), 'pp256' (the ping-pong form's row-wise epilogue: N > 128, at least 200 tiles of 256 x 256,
    K >= 1024, bf16, K % 64 == 0, one split), else 'register' (the epilogue every other tile form shares; '256x64' is the form for
    N <= 64)"""
    cdiv = lambda a, b: (a + b - 1) // b
    if splitk > 1 and bias_or_relu:
        return "fold" if N % 4 == 0 else None
    if N > 128 and cdiv(M, 256) * cdiv(N, 256) >= 200 and K >= 1024 and in_dtype == "bf16" and K % 64 == 0:
        return "pp256"
    return "register"

"""Plain references and case tables for the index-side kernels of the Stage-3 detector (csrc/proposals.hip: sw_rpn_select_pack,
sw_rpn_label_anchors, sw_roi_label_sample, sw_roi_assign_levels), read by tests/test_gpu_proposal_kernels.py.  Checkers, not product
code; CPU only.  tests/test_proposals_ref_cpu.py pins every reference to torch / the oracle and proves, with the key model below, that
each case lands on the edge it is named for (which radix pass decides, which digit, the size of the tied group and the chunks it spans).

References.  Selection: torch.sort(descending=True, stable=True)[:k] of the float32 logits on the CPU (NaN first, -0 == +0, ties by
ascending index).  Decode: apply_deltas in float64 (bar: 4 x the float32 oracle's own max error against it on the same inputs).
Matching / sampling / levels: oracle.frcnn_oracle with its closed-form permutation.  Level edges: the float64 level value, used only to
measure the distance to an integer.

The kernel's limits the tables aim at: 1024-element chunks, three radix passes of 11 + 11 + 10 key bits, an LDS sort whose capacity is
the next power of two >= max(pre_topk, 1024) (more than 8192 -> more than 64 KiB of LDS), 40 segments / 8 images / 64 images per
launch (more run as image ranges), 4096 rows per image in the ROI sampler, 1024-row slabs in the level kernel."""
import functools
import math

import numpy as np
import torch

from oracle import detgen
from oracle import frcnn_oracle as FO

CHUNK = 1024
MAX_SEG = 40
LABEL_MAX_IMG = 8
ROI_MAX_IMG = 64
ROI_CAP = 4096
PRE_TOPK_MAX = 16384
KEY_NONE = 0xFFFFFFFF
SCALE_CLAMP = float(np.float32(math.log(1000.0 / 16)))        # the float32 the kernel receives
DECODE_FACTOR = 4.0                                            # expf differs by ulps between libraries
LEVEL_EDGE_EPS = 1e-6


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def seed_of(tag, k):
    """the kernel seed that reproduces oracle.frcnn_oracle.Perm(tag)'s k-th permutation"""
    return detgen.fnv1a64(f"{tag}perm{k}")


def same_bits(got, want):
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(np.all(got.view(np.int32) == want.view(np.int32)))


# ============================================================================================ key model
def desc_key(v):
    """the kernel's selection key of float32 logits: ascending unsigned order == descending float order, -0 folded onto +0, NaN = 0"""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    b = np.where(b == 0x80000000, 0, b)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    mono = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    k = ~mono & 0xFFFFFFFF
    k = np.where(k == KEY_NONE, KEY_NONE - 1, k)
    return np.where(nan, 0, k).astype(np.uint32)


def float_of_key(key):
    """the float32 whose key is `key` (the inverse of desc_key away from NaN and -0)"""
    mono = ~np.asarray(key, np.uint64) & 0xFFFFFFFF
    b = np.where(mono & 0x80000000, mono ^ 0x80000000, ~mono & 0xFFFFFFFF)
    return b.astype(np.uint32).view(np.float32)


SHIFTS, DMASKS = (21, 10, 0), (0x7FF, 0x7FF, 0x3FF)


def digits(key):
    key = np.asarray(key, np.uint32)
    return tuple(((key >> s) & m).astype(np.int64) for s, m in zip(SHIFTS, DMASKS))


def model_order(v):
    """indices by (key, index): what the kernel's selection + sort produce"""
    return np.lexsort((np.arange(len(v)), desc_key(v)))


def radix_walk(v, k):
    """the kernel's three passes on one segment.  -> dict(mode, T, passes = [(digit, bucket size, bucket is one key)], deciding = first
    pass after which only the threshold key is left, k_rem, group = size of the tied group at T, chunks = chunks the group touches,
    cut_chunk = chunk of the last tie taken, cut_index = its index)"""
    keys = desc_key(v)
    n = len(keys)
    if k <= 0:
        return dict(mode=2)
    if n <= k:
        return dict(mode=1)
    cand = np.arange(n)
    want, passes, deciding = k, [], None
    for p in range(3):
        d = digits(keys[cand])[p]
        cnt = np.bincount(d, minlength=DMASKS[p] + 1)
        cum = np.cumsum(cnt)
        dig = int(np.searchsorted(cum, want))                  # first digit whose running count reaches `want`
        before = int(cum[dig] - cnt[dig])
        cand = cand[d == dig]
        pure = bool(np.all(keys[cand] == keys[cand[0]]))
        passes.append((dig, int(cnt[dig]), pure))
        if pure and deciding is None:
            deciding = p
        want -= before
    T = int(keys[cand[0]])
    assert np.all(keys[cand] == T) and T == int(np.sort(keys, kind="stable")[k - 1])
    return dict(mode=0, T=T, passes=passes, deciding=deciding, k_rem=want, group=len(cand), chunks=sorted(set((cand // CHUNK).tolist())),
                cut_chunk=int(cand[want - 1] // CHUNK), cut_index=int(cand[want - 1]))


# ============================================================================================ selection through rpn_select_pack
SEL_IMG_HW = (4096, 4096)                  # nothing clips: anchors live in [0, 264) x [0, 8 + n / 256)
W1 = (1.0, 1.0, 1.0, 1.0)


def index_anchors(n):
    """8 x 8 integer anchors that encode their own index: with zero deltas the decode is exact, box == anchor"""
    i = np.arange(n)
    x1 = (i % 256).astype(np.float32); y1 = (i // 256).astype(np.float32)
    return np.stack([x1, y1, x1 + 8, y1 + 8], 1).astype(np.float32)


def sort_ref(v, k):
    """THE selection reference: torch.sort(descending, stable)[:k] of a CPU float32 tensor"""
    return torch.sort(torch.from_numpy(np.ascontiguousarray(v, np.float32)), descending=True, stable=True).indices[:k].numpy()


def select_expected(levels, pre_topk):
    """levels: per level (N, n_l) float32 logits, anchors = index_anchors, zero deltas.  -> cand_scores (N, L pre, L + 1), cand_boxes
    (N, L pre, 4 L), finite (N,) as the entry point documents them: rows of level l at [l pre, l pre + k), the score in column l (-inf
    when the logit is not finite: proposal_utils.py:86-94 filters it), -inf elsewhere, the box repeated L times; unused rows -inf / 0"""
    L, N = len(levels), levels[0].shape[0]
    sc = np.full((N, L * pre_topk, L + 1), -np.inf, np.float32)
    bx = np.zeros((N, L * pre_topk, 4 * L), np.float32)
    fin = np.ones(N, np.int64)
    for l, lg in enumerate(levels):
        n = lg.shape[1]
        k = min(n, pre_topk)
        an = index_anchors(n)
        for img in range(N):
            idx = sort_ref(lg[img], k)
            s = lg[img][idx]
            ok = np.isfinite(s)
            if not ok.all():
                fin[img] = 0
            sc[img, l * pre_topk:l * pre_topk + k, l] = np.where(ok, s, -np.inf)
            bx[img, l * pre_topk:l * pre_topk + k] = np.tile(an[idx], (1, L))
    return sc, bx, fin


def quantised_logits(N, n, *key):
    """Gaussian logits rounded to 1 / 4: ties everywhere, the cut almost always inside a tied group"""
    return (np.round(_rng(101, N, n, *key).standard_normal((N, n)) * 4) / 4).astype(np.float32)


SEG_N = (1, 255, 1023, 1024, 1025, 2048, 2049, 4097)


def seg_pre_topks(n):
    return sorted({p for p in (1, n - 1, n, n + 1) if p >= 1})


# capacity edges of the LDS sort: (n, pre_topk, capacity)
CAP_CASES = [(3000, 1024, 1024), (3000, 1025, 2048), (13000, 12000, 16384), (16500, 16384, 16384)]


def sort_capacity(pre_topk):
    cap = 1024
    while cap < pre_topk:
        cap <<= 1
    return cap


# ---- radix edges: logits built from key bit patterns
# Top digits 1, 2 and 2045..2047 are NaN bit patterns (their key is 0), 3 holds only +inf and 2044 only -inf: with the low 21 bits zero
# the reachable top digits are 0 (NaN), 4 (FLT_MAX's exponent) .. 2043 and 2044 (-inf).
def _radix_keys(which):
    r = _rng(202, {"top": 0, "mid": 1, "low": 2, "pair": 3}[which])
    if which == "top":
        d = np.concatenate([r.integers(4, 2044, 2400), [4, 4, 4, 2043, 2043, 2043]])
        d[d == 1024] = 1025                                     # 1024 << 21 is -0.0, which the key folds onto +0.0's
        keys = d.astype(np.uint64) << 21
    elif which == "mid":
        d = np.concatenate([r.integers(0, 2048, 2400), [0, 0, 0, 2047, 2047, 2047]])
        keys = (0x300 << 21) | (d.astype(np.uint64) << 10) | 0x155
    elif which == "pair":                                       # two middle digits that differ in their lowest bit only, any low digit
        d1 = r.choice([0x2AA, 0x2AB], 2400).astype(np.uint64)
        keys = (0x300 << 21) | (d1 << 10) | r.integers(0, 1024, 2400).astype(np.uint64)
    else:
        d = np.concatenate([r.integers(0, 1024, 2400), [0, 0, 0, 1023, 1023, 1023]])
        keys = (0x300 << 21) | (0x2AA << 10) | d.astype(np.uint64)
    return r.permutation(keys)


@functools.lru_cache(None)
def radix_logits(which):
    """"top" / "mid" / "low": 2406 finite logits whose keys differ only in the top 11 / middle 11 / low 10 bits, every digit group a
    tie of several; "top_special": the top set with NaN (digit 0) and -inf (digit 2044, the last one a float can have) added; "pair":
    2400 logits in two neighbouring middle-digit buckets (the pass-2 prefix must keep all 22 decided bits to tell them apart)"""
    if which == "top_special":
        v = radix_logits("top").copy()
        r = _rng(203)
        pos = r.choice(len(v), 9, replace=False)
        v[pos[:4]] = np.float32(np.nan)
        v[pos[4:]] = -np.float32(np.inf)
        return v
    return float_of_key(_radix_keys(which)).copy()


def radix_ks(which):
    """pre_topk values: the threshold in the first digit group (one taken / all of it), in the middle, in the last group (all but one
    element / one into it)"""
    v = radix_logits(which)
    n = len(v)
    if which == "pair":                                         # the threshold inside the first bucket, inside the second, near its end
        return [n // 4, n // 2 + 300, n - 5]
    keys = np.sort(desc_key(v))
    first = int((keys == keys[0]).sum()); last = int((keys == keys[-1]).sum())
    return [1, first, n // 2, n - last + 1, n - 1]


RADIX_ONE_DIGIT = ("top", "mid", "low", "top_special")
RADIX_SETS = RADIX_ONE_DIGIT + ("pair",)


# ---- tie edges
def tie_cases():
    """name -> (logits (n,), pre_topk)"""
    i = np.arange(3000)
    inter = np.where(i % 3 == 0, -1.5, np.where(i % 3 == 1, 0.25, 2.0)).astype(np.float32)       # below / the tied group / above
    return {"all_equal": (np.full(5000, 0.75, np.float32), 2500),
            "interleaved_mid": (inter, 1500),          # 1000 above + 500 of the 1000 tied: the cut in the middle of chunk 1
            "interleaved_end": (inter, 2000),          # the cut exactly at the group's end
            "interleaved_one": (inter, 1001)}          # exactly one element of the group


# ---- special values: three images, the same layout (400 above, 600 tied, 500 below, shuffled), pre_topk 700 cuts the tied group
SPECIAL_PRE = 700
DEN_MIN = np.uint32(1).view(np.float32)
FLT_MAX = np.float32(np.finfo(np.float32).max)


def special_logits():
    r = _rng(303)
    out = np.zeros((3, 1500), np.float32)
    den = np.array([1, 2, 3, 0x7FFFFF], np.uint32).view(np.float32)                        # denormals, the largest included
    # image 0: positive denormals > (+0 / -0 mixed) > negative denormals
    a = np.concatenate([r.choice(den, 400), np.where(r.integers(0, 2, 600) == 1, np.float32(0.0), np.float32(-0.0)), -r.choice(den, 500)])
    out[0] = a.astype(np.float32)[r.permutation(1500)]
    # image 1: 7 NaN among the values above; the tied group is 1.0
    b = np.concatenate([np.full(7, np.nan), 2 + r.random(393), np.full(600, 1.0), -r.random(500)])
    out[1] = b.astype(np.float32)[r.permutation(1500)]
    # image 2: +inf, FLT_MAX, denormals above; the tied group is -FLT_MAX; -inf below
    c = np.concatenate([np.full(3, np.inf), np.full(5, FLT_MAX), r.choice(den, 392), np.full(600, -FLT_MAX), np.full(500, -np.inf)])
    out[2] = c.astype(np.float32)[r.permutation(1500)]
    return out


# ---- call shapes: name -> (N, per-level lengths, pre_topk, single-tensor form)
SHAPE_CASES = {"L1": (2, [1500], 700, False),
               "L8_mixed": (2, [2100, 1025, 1024, 700, 300, 64, 7, 1], 700, False),       # levels shorter than pre_topk beside longer ones
               "seg40": (5, [1300, 700, 300, 200, 100, 50, 20, 5], 256, False),           # N L == 40 exactly
               "seg45": (9, [1500, 700, 300, 100, 20], 500, False),                       # N L == 45: image ranges of 8 + 1
               "single_tensor": (3, [1500, 700, 300], 500, True),
               "single_tensor_ranges": (9, [1100, 300, 100, 40, 9], 200, True)}


def shape_logits(name):
    N, n_l, pre, _ = SHAPE_CASES[name]
    return [quantised_logits(N, n, l, len(name)) for l, n in enumerate(n_l)]


# ============================================================================================ decode through rpn_select_pack
DEC_HW = (300, 400)
DEC_N, DEC_LEVELS = 2, (1100, 300)


def apply_deltas64(deltas, anchors, weights, scale_clamp=SCALE_CLAMP):
    """box_regression.py:88-116 in float64 on the float32 inputs"""
    d = np.asarray(deltas, np.float64); a = np.asarray(anchors, np.float64)
    w = a[:, 2] - a[:, 0]; h = a[:, 3] - a[:, 1]
    cx = a[:, 0] + 0.5 * w; cy = a[:, 1] + 0.5 * h
    with np.errstate(all="ignore"):
        dx = d[:, 0] / weights[0]; dy = d[:, 1] / weights[1]
        dw = np.where(d[:, 2] / weights[2] > scale_clamp, scale_clamp, d[:, 2] / weights[2])
        dh = np.where(d[:, 3] / weights[3] > scale_clamp, scale_clamp, d[:, 3] / weights[3])
        px = dx * w + cx; py = dy * h + cy
        pw = np.exp(dw) * w; ph = np.exp(dh) * h
        return np.stack([px - 0.5 * pw, py - 0.5 * ph, px + 0.5 * pw, py + 0.5 * ph], 1)


def apply_deltas32(deltas, anchors, weights):
    """the existing float32 CPU reference"""
    return FO.O.apply_deltas(torch.from_numpy(np.ascontiguousarray(deltas, np.float32)), torch.from_numpy(np.ascontiguousarray(anchors, np.float32)),
                             tuple(float(x) for x in weights), SCALE_CLAMP).numpy()


def exact_div_delta(target, w):
    """a float32 d with float32(d / w) == target exactly (searched around target * w)"""
    d = np.float32(np.float32(target) * np.float32(w))
    for _ in range(8):
        q = np.float32(d / np.float32(w))
        if q == np.float32(target):
            return d
        d = np.nextafter(d, np.float32(np.inf) if q < target else -np.float32(np.inf))
    raise AssertionError("no exact quotient")


# rows of level 0 with a fixed purpose: name -> row
DEC_NAMED = {"zero_w_left": 0, "zero_w_right": 1, "outside": 2, "dw_eq": 3, "dw_above": 4, "dw_below": 5, "dh_eq": 6, "dh_above": 7}
DEC_INF_ROW = (1, 0, 9)                    # (image, level, row): an inf delta -> finite[1] == 0


@functools.lru_cache(None)
def decode_case(weights):
    """-> dict(anchors [per level (n, 4)], logits [(N, n)], deltas [(N, n, 4)], weights).  Distinct logits (the order is not what
    is under test), every row selected (pre_topk = the longest level)."""
    r = _rng(404, int(weights[0]), int(weights[2]))
    H, W = DEC_HW
    anchors, logits, deltas = [], [], []
    wv = np.asarray(weights, np.float32)
    for l, n in enumerate(DEC_LEVELS):
        x1 = r.random(n) * (W + 80) - 60; y1 = r.random(n) * (H + 80) - 60
        an = np.stack([x1, y1, x1 + 4 + r.random(n) * 150, y1 + 4 + r.random(n) * 120], 1).astype(np.float32)
        dl = (r.standard_normal((DEC_N, n, 4)) * np.array([0.5, 0.5, 1.2, 1.2]) * wv).astype(np.float32)
        dl[:, ::7, 2:] *= 4                                    # a good share of dw / dh beyond the clamp
        lg = r.permutation(DEC_N * n).reshape(DEC_N, n).astype(np.float32) / 16 - 20
        if l == 0:
            z = np.zeros(4, np.float32)
            an[0] = [-20, 5, 0, 30]; dl[:, 0] = z              # x2 == 0 exactly: clipped width 0
            an[1] = [W, 5, W + 16, 20]; dl[:, 1] = z           # x1 == W exactly
            an[2] = [W + 50, H + 50, W + 90, H + 70]; dl[:, 2] = z
            c = np.float32(SCALE_CLAMP)
            for row, (col, val) in {3: (2, c), 4: (2, np.nextafter(c, np.float32(np.inf))), 5: (2, np.nextafter(c, np.float32(0))),
                                    6: (3, c), 7: (3, np.float32(2) * c)}.items():
                an[row] = [100, 100, 104, 103]; dl[:, row] = z
                dl[:, row, col] = exact_div_delta(val, wv[col]) if row in (3, 6) else np.float32(val * wv[col])
        anchors.append(an); logits.append(lg); deltas.append(dl)
    img, l, row = DEC_INF_ROW
    deltas[l][img, row, 0] = np.inf
    return dict(anchors=anchors, logits=logits, deltas=deltas, weights=tuple(float(x) for x in weights))


DEC_WEIGHTS = ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0))


@functools.lru_cache(None)
def decode_expected(weights):
    """-> dict(order[l][img] = selected anchor indices, box64[l][img] (k, 4) float64, bar = DECODE_FACTOR x the float32 reference's max
    error against float64 over every finite coordinate of the case, keep[l][img] = expected 'kept' flag, sure[l][img] = rows whose
    clipped float64 width and height are farther than `bar` from 0 (or which are not finite), finite (N,), e32)"""
    c = decode_case(weights)
    H, W = DEC_HW
    e32 = 0.0
    box64, order = [], []
    for an, lg, dl in zip(c["anchors"], c["logits"], c["deltas"]):
        b64, od = [], []
        for img in range(DEC_N):
            idx = sort_ref(lg[img], len(lg[img]))
            r64 = apply_deltas64(dl[img], an, weights)[idx]
            r32 = apply_deltas32(dl[img], an, weights)[idx].astype(np.float64)
            ok = np.isfinite(r64)
            assert np.array_equal(ok, np.isfinite(r32))
            e32 = max(e32, float(np.abs(r32[ok] - r64[ok]).max()))
            b64.append(r64); od.append(idx)
        box64.append(b64); order.append(od)
    bar = DECODE_FACTOR * e32
    keep, sure, fin = [], [], np.ones(DEC_N, np.int64)
    for l, b64 in enumerate(box64):
        kp, su = [], []
        for img in range(DEC_N):
            b = b64[img]
            okr = np.isfinite(b).all(1)
            if not okr.all():
                fin[img] = 0
            with np.errstate(invalid="ignore"):
                cw = np.clip(b[:, 2], 0, W) - np.clip(b[:, 0], 0, W); ch = np.clip(b[:, 3], 0, H) - np.clip(b[:, 1], 0, H)
                kp.append(okr & (cw > 0) & (ch > 0))
                # empty beyond doubt: the whole box lies outside the image by more than the bar (both clipped ends meet on one border)
                out = (b[:, 0] >= W + bar) | (b[:, 2] <= -bar) | (b[:, 1] >= H + bar) | (b[:, 3] <= -bar)
                su.append(~okr | out | ((cw > bar) & (ch > bar)))
        keep.append(kp); sure.append(su)
    return dict(order=order, box64=box64, bar=bar, e32=e32, keep=keep, sure=sure, finite=fin)


# ============================================================================================ rpn_label_anchors
# Integer boxes, exact IoUs.  The ground-truth box g0 = [0, 0, 100, 1] (area 100) and anchors [0, 0, m, 1] inside it: IoU == m / 100
# correctly rounded, so m = 70 is float32(0.7) (label 1 by the threshold, not by the low-quality rule: m = 100 is g0's best) and m = 30
# is float32(0.3) (label -1, not 0).
G0 = np.array([0, 0, 100, 1], np.float32)
SPECIAL_M = (70, 30, 100, 71, 69, 31, 29, 1)
SPLIT_ANCHOR = np.array([0, 10, 10, 20], np.float32)           # IoU 0.5 with both halves below: the first ground-truth box wins
SPLIT_GT = np.array([[0, 10, 10, 15], [0, 15, 10, 20]], np.float32)
FAR_GT = np.array([[50000, 50000, 50010, 50010]], np.float32)  # overlaps no anchor: best IoU 0 -> every zero-IoU anchor is positive


def label_anchors(A):
    """A integer anchors: a grid of disjoint 10 x 10 boxes (y >= 100), with the special anchors written over positions spread through
    the array (the chunk boundary 1023 / 1024 included when A reaches it)"""
    i = np.arange(A)
    x = 20.0 * (i % 64); y = 100 + 20.0 * (i // 64)
    an = np.stack([x, y, x + 10, y + 10], 1).astype(np.float32)
    sp = [np.array([0, 0, m, 1], np.float32) for m in SPECIAL_M] + [SPLIT_ANCHOR]
    for j, p in enumerate(special_positions(A)):
        an[p] = sp[j]
    return an


def special_positions(A):
    n = min(A, len(SPECIAL_M) + 1)
    want = [0, 1023, 1024, A - 1, A // 2, A // 3, 1, 2 * A // 3, A // 5]
    pos = []
    for p in want + list(range(A)):
        if 0 <= p < A and p not in pos:
            pos.append(p)
        if len(pos) == n:
            break
    return pos


def label_gt(kind, A):
    """ground-truth boxes of one image"""
    an = label_anchors(A)
    if kind == "none":
        return np.zeros((0, 4), np.float32)
    if kind == "thr":                                           # the threshold ladder + the split pair + one box on a grid anchor
        free = [p for p in range(A) if p not in special_positions(A)]
        return np.concatenate([G0[None], SPLIT_GT, an[free[len(free) // 2]][None] if free else G0[None][:0]], 0)
    if kind == "twins":                                         # two identical boxes (the first wins), then the ladder
        return np.concatenate([G0[None], G0[None], SPLIT_GT], 0)
    if kind == "far":                                           # a box that overlaps nothing, beside the ladder
        return np.concatenate([G0[None], FAR_GT], 0)
    if kind == "far_only":
        return FAR_GT.copy()
    if kind == "exact5":                                        # exactly min(5, A) positives: boxes that ARE grid anchors
        free = [p for p in range(A) if p not in special_positions(A)][:5]
        return an[free].copy() if free else an[:1].copy()
    raise KeyError(kind)


# (name, A, gt kinds per image, batch, max_pos)
LABEL_CASES = [
    ("A1", 1, ["thr", "none"], 256, 64),
    ("A1023_all", 1023, ["thr", "twins"], 2048, 2048),                  # A < batch: everything is taken, labels == the matcher's
    ("A1024_all", 1024, ["thr", "far"], 2048, 2048),
    ("A1025_all", 1025, ["thr", "twins", "none"], 2048, 2048),
    ("A3073_all", 3073, ["thr", "twins"], 4096, 4096),
    ("A3073_sampled", 3073, ["thr", "twins", "far"], 256, 64),
    ("no_gt_at_all", 1025, ["none", "none"], 256, 64),                  # 0 positives: a zero draw through the device count
    ("no_gt_in_one", 1024, ["thr", "none", "twins"], 256, 64),
    ("far_only_more_pos_than_cap", 1025, ["far_only"], 256, 64),        # 1025 positives > 64, 0 negatives < 192
    ("pos_eq_cap", 1025, ["exact5"], 64, 5),
    ("max_pos_0", 1025, ["thr", "exact5"], 64, 0),
    ("nine_images", 1025, ["thr", "none", "twins", "far", "exact5", "thr", "far_only", "none", "twins"], 128, 32),   # ranges of 8 + 1
]


def label_expected(case):
    name, A, kinds, batch, max_pos = case
    an = label_anchors(A)
    gts = [label_gt(k, A) for k in kinds]
    tag = "plab" + name
    labels, matched = FO.rpn_label_and_sample(an, gts, FO.Perm(tag), batch_size=batch, positive_fraction=(max_pos + 0.5) / batch)
    seeds = [seed_of(tag, k) for k in range(2 * len(kinds))]
    return an, gts, seeds, labels, matched


def matcher_labels(an, gtb):
    """labels before sampling (1 / 0 / -1) by the oracle's matcher"""
    if len(gtb) == 0:
        return np.zeros(len(an), np.int64)
    return FO.matcher(FO.O.pairwise_iou(gtb, an), (0.3, 0.7), (0, -1, 1), True)[1].astype(np.int64)


# ============================================================================================ roi_label_sample
ROI_K = 20


def roi_gt(G, *key):
    """G disjoint 100 x 1 integer boxes stacked at y = 10 j, classes in [0, K)"""
    j = np.arange(G)
    gb = np.stack([0 * j, 10 * j, 100 + 0 * j, 10 * j + 1], 1).astype(np.float32).reshape(G, 4)
    return gb, _rng(505, G, *key).integers(0, ROI_K, G)


def roi_props(P, G, mode, *key):
    """P integer proposals.  "mixed": [0, 10 j, m, 10 j + 1] with m in (100, 51, 50, 49, 20) (IoU m / 100 with box j: 50 is EXACTLY the
    threshold) and far background boxes; "fg": m in (100, 51, 50) only; "bg": far boxes only"""
    r = _rng(506, P, G, *key)
    far = np.stack([1000 + r.integers(0, 500, P), 1000 + r.integers(0, 500, P)], 1)
    far = np.concatenate([far, far + 10], 1).astype(np.float32)
    if mode == "bg" or G == 0:
        return far
    j = r.integers(0, G, P)
    m = r.choice([100, 51, 50] if mode == "fg" else [100, 51, 50, 49, 20], P)
    near = np.stack([0 * j, 10 * j, m, 10 * j + 1], 1).astype(np.float32)
    return near if mode == "fg" else np.where((r.random(P) < 0.5)[:, None], near, far).astype(np.float32)


# (name, per image (p_cnt, G, mode), p_stride, append_gt, batch, max_pos)
ROI_CASES = [
    ("empty_props_gt_appended", [(0, 3, "mixed"), (0, 1, "mixed")], 16, True, 64, 16),
    ("empty_everything", [(0, 0, "bg"), (5, 0, "bg")], 16, True, 64, 16),                 # count 0 for the first image
    ("n1023", [(1020, 3, "mixed")], 1020, True, 512, 128),
    ("n1024", [(1021, 3, "mixed")], 1024, True, 512, 128),
    ("n1025", [(1022, 3, "mixed")], 1022, True, 512, 128),
    ("n2048", [(2045, 3, "mixed")], 2048, True, 512, 128),
    ("n2049", [(2046, 3, "mixed")], 2050, True, 512, 128),
    ("n4096_stride_plus_gt", [(4093, 3, "mixed"), (100, 3, "mixed")], 4093, True, 512, 128),
    ("all_foreground", [(300, 4, "fg")], 300, True, 512, 128),                           # 304 foreground > 128, no background: 128 rows
    ("no_foreground", [(300, 4, "bg")], 300, False, 512, 128),
    ("no_gt_append_on", [(300, 0, "bg")], 300, True, 512, 128),
    ("split_pair", [(40, -1, "split")], 40, True, 64, 64),
    ("images65", [(20 - (i % 3), i % 3, "mixed") for i in range(65)], 20, True, 32, 8),   # ranges of 64 + 1
]
ROI_REFUSED = ("stride_plus_gt_4097", [(10, 3, "mixed")], 4094, True, 512, 128)


def roi_inputs(case):
    """-> (props per image, gts [(boxes, classes)] per image)"""
    name, imgs, p_stride, append, batch, max_pos = case
    props, gts = [], []
    for i, (p, G, mode) in enumerate(imgs):
        if mode == "split":                                     # one proposal halves two boxes: IoU 0.5 with both, the first wins
            gb, gc = SPLIT_GT.copy(), np.array([7, 3])
            pb = roi_props(p, 0, "bg", i, len(name)); pb[p // 2] = SPLIT_ANCHOR
        else:
            gb, gc = roi_gt(G, i, len(name))
            pb = roi_props(p, G, mode, i, len(name))
        props.append(pb); gts.append((gb, gc))
    return props, gts


def roi_expected(case):
    name, imgs, p_stride, append, batch, max_pos = case
    props, gts = roi_inputs(case)
    tag = "proi" + name
    want = FO.roi_label_and_sample([{"boxes": p} for p in props], gts, ROI_K, FO.Perm(tag), batch_size=batch,
                                   positive_fraction=(max_pos + 0.5) / batch, append_gt=append)
    return props, gts, [seed_of(tag, k) for k in range(2 * len(imgs))], want


# ============================================================================================ roi_assign_levels
def level_value64(boxes):
    """4 + log2(sqrt(area) / 224 + 1e-8) in float64 from the float32 boxes (NaN for a negative area)"""
    b = np.asarray(boxes, np.float64)
    with np.errstate(all="ignore"):
        return 4.0 + np.log2(np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / 224.0 + 1e-8)


def near_level_edge(boxes):
    """rows whose float64 level value lies within LEVEL_EDGE_EPS of an integer: the only rows where float32 log2 ulps may move a level"""
    v = level_value64(boxes)
    with np.errstate(invalid="ignore"):
        return np.abs(v - np.round(v)) < LEVEL_EDGE_EPS


def _sq(s, w=None):
    w = s if w is None else w
    return [16.0, 32.0, 16.0 + w, 32.0 + s * s / w]


LEVEL_EDGES = np.array([_sq(112), _sq(224), _sq(448), _sq(112, 56), _sq(112, 224), _sq(224, 112), _sq(224, 448), _sq(448, 224), _sq(448, 896),
                        _sq(112, 28)], np.float32)             # exact powers of two of sqrt(area) / 224: levels 1, 2, 3 start here
LEVEL_EDGE_WANT = np.array([1, 2, 3, 1, 1, 2, 2, 3, 3, 1])


def _neighbours():
    out = []
    for s in (112.0, 224.0, 448.0):
        for to in (np.inf, -np.inf):
            out.append([0.0, 0.0, np.nextafter(np.float32(s), np.float32(to)), s])          # one ulp to either side of the edge
    return np.array(out, np.float32)


LEVEL_NEIGHBOURS = _neighbours()
LEVEL_ODD = np.array([[5, 5, 5, 5], [5, 5, 50, 5], [0, 0, 1e-3, 1e-3], [0, 0, 1e4, 1e4], [3, 3, 3.001, 900]], np.float32)   # zero area, tiny, huge
LEVEL_ODD_WANT = np.array([0, 0, 0, 3, 0])
LEVEL_NEGATIVE = np.array([[10, 10, 5, 20], [10, 10, 20, 5]], np.float32)        # negative width / height: NaN size -> level 0 (kernel rule)
LEVEL_R = (1, 1023, 1024, 1025, 2049)


@functools.lru_cache(None)
def level_case(R):
    """-> (boxes (R, 4), kind (R,) with 0 random, 1 edge, 2 neighbour, 3 odd, 4 negative, row_cnt [a, 0, b])"""
    r = _rng(606, R)
    named = np.concatenate([LEVEL_EDGES, LEVEL_NEIGHBOURS, LEVEL_ODD, LEVEL_NEGATIVE], 0)
    kinds = np.concatenate([np.full(len(LEVEL_EDGES), 1), np.full(len(LEVEL_NEIGHBOURS), 2), np.full(len(LEVEL_ODD), 3), np.full(len(LEVEL_NEGATIVE), 4)])
    if R == 1:
        return LEVEL_EDGES[1:2].copy(), np.array([1]), [0, 0, 1]
    reps = 3 if R > 3 * len(named) else 1
    x1 = r.random(R) * 300; y1 = r.random(R) * 300
    side = 2.0 ** (r.random(R) * 8 + 2)                         # 4 .. 1024: every level
    boxes = np.stack([x1, y1, x1 + side, y1 + side * (0.5 + r.random(R))], 1).astype(np.float32)
    kind = np.zeros(R, np.int64)
    forced = [p for p in (0, R - 1, 1022, 1023, 1024, R // 2) if p < R]              # the slab boundary and both ends hold named boxes
    pos = list(dict.fromkeys(forced + [int(p) for p in r.choice(R, reps * len(named), replace=False)]))[:reps * len(named)]
    for j, p in enumerate(pos):
        boxes[p] = named[j % len(named)]; kind[p] = kinds[j % len(named)]
    a = R // 3
    return boxes, kind, [a, 0, R - a]


def level_expected(boxes, kind):
    """float32 oracle levels (the negative-area rows: 0, the kernel's documented rule; numpy's cast of NaN is platform-defined)"""
    ok = kind != 4
    want = np.zeros(len(boxes), np.int64)
    want[ok] = FO.assign_levels(boxes[ok])
    return want


def small_boxes(R):
    """every box below 112 / sqrt(2) a side: level 0 only, levels 1..3 receive no rows"""
    r = _rng(607, R)
    x1 = r.random(R) * 300; y1 = r.random(R) * 300
    return np.stack([x1, y1, x1 + 4 + r.random(R) * 60, y1 + 4 + r.random(R) * 60], 1).astype(np.float32)

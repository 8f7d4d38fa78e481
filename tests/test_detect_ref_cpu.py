"""CPU: pins tests/detect_ref.py (the checker of sw_detect_postprocess) and the constructed inputs of test_gpu_detect_postprocess.py.
The vectorised reference equals the pair-by-pair one and, on the NMS step, oracle.oicr_oracle.nms_keep in batched_nms's one-pass form;
every edge input has the property its GPU test relies on (`check_conditions`, asserted again on the GPU side): the form each class
takes, the IoU-at-the-threshold pair, the offset-sensitive pair, the rows beyond the resolver's LDS window, the tile count, the cuts."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as D  # noqa: E402
from detect_ref import detect_ref, detect_ref_scalar, route, same  # noqa: E402

F = np.float32
NEG = -3.0e38                                                                  # the RPN use's "no threshold"
ALL = 1800                                                                     # a top-k no case of up to 9 classes reaches: every survivor is compared


# ------------------------------------------------------------------------------------------------------------ input builders
def _blank(R, K, thr):
    """nothing is a candidate: -inf (the RPN form's unused rows) or, for a real threshold, a score exactly AT it (excluded by `>`)"""
    s = np.full((R, K + 1), -np.inf if thr < -1e38 else F(thr), F)
    s[:, K] = F(0.5)                                                           # the background column is never read
    return s, np.zeros((R, K, 4), F)


def _rand_boxes(rng, n, H, W, size):
    cx = rng.uniform(-10, W + 10, n); cy = rng.uniform(-10, H + 10, n)         # partly outside the image: clipping
    w = rng.uniform(size[0], size[1], n); h = rng.uniform(size[0], size[1], n)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(F)


def _rand_scores(rng, n, thr, quant, negative=False):
    if negative:
        s = -0.1 - np.abs(rng.randn(n)) * 3
    else:
        lo = 0.0 if thr < -1e38 else thr
        s = lo + (1 - lo) * rng.uniform(0.02, 1.0, n)
    if quant:
        s = np.round(s * quant) / quant
    s = s.astype(F)
    if thr > -1e38:
        s[s <= F(thr)] = F(thr) + F(1.0 / (quant or 64))
    return s


def dense(seed, R, nvs, H=240, W=320, thr=0.05, nms=0.5, topk=100, size=(8, 80), quant=None, negative=False, **expect):
    """class c has exactly nvs[c] candidates on random rows; everything else sits at or below the threshold"""
    rng = np.random.RandomState(seed)
    K = len(nvs)
    s, b = _blank(R, K, thr)
    for c, n in enumerate(nvs):
        rows = np.sort(rng.permutation(R)[:n])
        s[rows, c] = _rand_scores(rng, n, thr, quant, negative)
        b[:, c] = _rand_boxes(rng, R, H, W, size)
        if thr > -1e38:                                                        # the rest: below the threshold, not only at it
            rest = np.setdiff1d(np.arange(R), rows)[::2]
            s[rest, c] = (F(thr) * rng.uniform(0, 1, len(rest))).astype(F)
    return dict(scores=s, boxes=b.reshape(R, 4 * K), H=H, W=W, thr=thr, nms=nms, topk=topk, nv=list(nvs), **expect)


SPECIAL_ROWS = 16


def special(specials, n_fill, K, fill_classes, H=800, W=1333, thr=0.05, nms=0.5, topk=200, seed=0, fill_scores=(0.1, 0.7), fill_size=(8, 60),
            **expect):
    """hand-made (row, class, box, score) entries on rows < 16 plus n_fill random fillers per class of fill_classes on the rows from 16
    on, inside x, y >= 100 (the specials live at the image's origin unless a test says otherwise) with scores in fill_scores"""
    rng = np.random.RandomState(seed)
    R = SPECIAL_ROWS + n_fill
    s, b = _blank(R, K, thr)
    for c in fill_classes:
        x = rng.uniform(100, W - 70, n_fill); y = rng.uniform(100, H - 70, n_fill)
        w = rng.uniform(fill_size[0], fill_size[1], n_fill); h = rng.uniform(fill_size[0], fill_size[1], n_fill)
        b[SPECIAL_ROWS:, c] = np.stack([x, y, x + w, y + h], 1).astype(F)
        s[SPECIAL_ROWS:, c] = rng.uniform(fill_scores[0], fill_scores[1], n_fill).astype(F)
    nv = [n_fill if c in fill_classes else 0 for c in range(K)]
    for r, c, box, score in specials:
        assert r < SPECIAL_ROWS
        b[r, c] = np.asarray(box, F); s[r, c] = F(score)
        nv[c] += 1
    return dict(scores=s, boxes=b.reshape(R, 4 * K), H=H, W=W, thr=thr, nms=nms, topk=topk, nv=nv, **expect)


REACH = [15, 79, [1300.0, 700.0, 1400.0, 790.0], 0.09]                       # clipped to x2 = 1333 = W: max_coord 1333, class 79's offset 105386
PAIRS = {0.5: ([0, 0, 2, 1], [0, 0, 1, 1]), 0.3: ([0, 0, 10, 1], [0, 0, 3, 1]), 0.7: ([0, 0, 10, 1], [0, 0, 7, 1])}
OFFSET_PAIR = ([0, 0, 2, 1], [0, 0, 1 + 1 / 512, 1])


def pair_case(pair, nms, n_fill, **expect):
    """the pair (first at 0.9, second at 0.8) in class 0 and in class 79 of 80, fillers (lower scores, far away) in both"""
    sp = [[0, 0, pair[0], 0.9], [1, 0, pair[1], 0.8], [0, 79, pair[0], 0.9], [1, 79, pair[1], 0.8], REACH]
    return special(sp, n_fill, 80, [0, 79], nms=nms, seed=int(nms * 10) + n_fill, **expect)


def neg_thresh_case(n_fill):
    """nms_thresh = -1: IoU 0 suppresses, only NaN (two empty boxes) does not.  Class 0's best box has area: it stands alone.
    Class 1's best box is empty: every empty box of the class is kept with it, every box with area falls."""
    rng = np.random.RandomState(40 + n_fill)
    sp = [[0, 0, [10, 10, 50, 40], 0.95], [1, 0, [300, 300, 300, 340], 0.9], [2, 0, [60, 60, 60, 60], 0.85],
          [0, 1, [20, 20, 20, 60], 0.95], [1, 1, [500, 20, 560, 20], 0.9], [2, 1, [20, 20, 20, 60], 0.85], [3, 1, [5, 5, 30, 30], 0.8]]
    case = special(sp, n_fill, 2, [0, 1], nms=-1.0, topk=ALL, seed=41 + n_fill, neg_thresh=True)
    b = case["boxes"].reshape(-1, 2, 4)
    empty = SPECIAL_ROWS + np.nonzero(rng.uniform(size=n_fill) < 0.3)[0]      # a third of the fillers have no area
    b[empty, :, 2] = b[empty, :, 0]
    return case


def zero_case(n_fill):
    """+0.0 and -0.0 are one score: position decides.  Class 0: -0.0 on row 2 and +0.0 on row 7, overlapping boxes: row 2 wins and row 7
    falls.  Class 1: +0.0 on row 1, -0.0 on row 3, apart: both stay, and the final order over both classes is by r * K + c."""
    sp = [[2, 0, [0, 0, 40, 40], -0.0], [7, 0, [2, 2, 42, 42], 0.0], [1, 1, [0, 0, 30, 30], 0.0], [3, 1, [50, 50, 90, 90], -0.0],
          [4, 0, [0, 60, 20, 80], -1.5], [5, 1, [60, 0, 80, 20], 2.5]]
    return special(sp, n_fill, 2, [0, 1], thr=NEG, nms=0.5, topk=ALL, seed=50 + n_fill, fill_scores=(-3.0, -0.5), zeros=True)


def boxes_case():
    H, W = 300, 500
    sp = [[0, 0, [-50, -40, -10, -5], 0.99],                                  # wholly outside, top left: clipped to the point (0, 0)
          [1, 0, [600, 100, 700, 200], 0.98],                                 # wholly outside, right: clipped to a line on x = W
          [2, 0, [100, 400, 200, 500], 0.97],                                 # below: a line on y = H
          [3, 0, [-20, -20, 900, 900], 0.96],                                 # clipped on all four sides: the whole image
          [4, 0, [100, 100, 200, 180], 0.95], [5, 0, [100, 100, 200, 180], 0.94],          # duplicates with area: the second falls
          [6, 0, [250, 50, 250, 90], 0.93], [7, 0, [250, 50, 250, 90], 0.92],              # empty duplicates: IoU NaN, both stay
          [8, 0, [-5, 120, 40, 310], 0.91], [9, 0, [480, -3, 520, 20], 0.90]]
    return special(sp, 0, 1, [], H=H, W=W, thr=0.05, nms=0.5, topk=50, boxes_edge=True)


def scores_case(kind):
    if kind == "negative":                                                     # RPN logits: all negative, -inf on the unused rows
        return dense(60, 300, [200, 0, 90], thr=NEG, nms=0.7, topk=ALL, negative=True, forms=("BAA", "BAA"), negative_scores=True)
    c = dense(61, 200, [50, 60], thr=0.05, nms=0.5, topk=ALL, forms=("AA", "AA"), at_thresh=True)       # the blanks sit exactly at thr
    return c


@functools.lru_cache(maxsize=None)
def _topk_base():
    """one class of 300 candidates (per-class workspace: form A; full: form C), light overlap and scores in steps of 1/64: many survivors,
    equal scores inside the class"""
    return dense(30, 1000, [300], H=600, W=900, thr=0.05, nms=0.5, topk=16384, size=(20, 70), quant=64)


def topk_case(kind):
    base = _topk_base()
    full = detect_ref(base["scores"], base["boxes"], base["H"], base["W"], base["thr"], base["nms"], 16384)
    rank = full.rank
    if kind == "mid_chunk":                                                    # the cut-th survivor sits in the middle of the second chunk
        t = int(np.nonzero((rank >= 64 + 20) & (rank < 64 + 44))[0][0])
    elif kind == "chunk_end":                                                  # ... is a chunk's last candidate
        t = int(np.nonzero(rank % 64 == 63)[0][0])
    elif kind == "one":
        t = 0
    else:
        t = full.count + 9                                                     # more than survive
    return dict(base, topk=t + 1, forms=("A", "C"), topk_kind=kind, uncut=full)


@functools.lru_cache(maxsize=None)
def _tie_base():
    return dense(31, 1000, [300, 300, 40, 40], H=600, W=900, thr=0.05, nms=0.5, topk=4096, size=(20, 70), quant=16)


def tie_cut_case():
    """scores in steps of 1/16 over four classes: the global cut goes through a group of equal scores that spans several classes"""
    base = _tie_base()
    full = detect_ref(base["scores"], base["boxes"], base["H"], base["W"], base["thr"], base["nms"], 4096)
    s, c = full.scores, full.classes
    for t in range(20, full.count - 1):
        if s[t - 1] == s[t] and c[t - 1] != c[t] and full.rows[t - 1] * 4 + c[t - 1] < full.rows[t] * 4 + c[t] and s[t + 1] == s[t]:
            return dict(base, topk=t, forms=("AAAA", "CCAA"), tie_cut=True, uncut=full)
    raise AssertionError("no tie group at a cut")


FUZZ_SEED, FUZZ_N = 7, 40


def fuzz_case(i):
    rng = np.random.RandomState(FUZZ_SEED * 1000 + i)
    R = int(rng.randint(1, 701)); K = int(rng.choice([1, 3, 20, 80]))
    H, W = int(rng.randint(60, 700)), int(rng.randint(60, 1000))
    thr = float(rng.choice([NEG, 0.05, 0.3])); nms = float(rng.choice([0.3, 0.5, 0.7]))
    topk = int(min(rng.choice([1, 7, 100, 700]), 16384 // K))
    frac = float(rng.choice([0.05, 0.3, 0.6, 1.0]))
    quant = int(rng.choice([0, 50]))
    nvs = [int(rng.binomial(R, frac)) if frac < 1 else R for _ in range(K)]
    hi = float(rng.choice([30, 120, 400]))
    return dense(int(rng.randint(1 << 30)), R, nvs, H=H, W=W, thr=thr, nms=nms, topk=topk, size=(2, hi), quant=quant)


CASES = {
    # form boundaries of the per-class workspace: A -> B at nv*16+16 <= (NP-nv)*8, plus 0 / 1 / the chunk edges
    "boundary_R64": lambda: dense(1, 64, [20, 21, 0, 1, 63, 64], topk=ALL, forms=("ABAABB", "ABAABB")),
    "boundary_R256": lambda: dense(2, 256, [84, 85, 0, 1, 63, 64, 65, 128, 129], topk=ALL, forms=("ABAAAAABB", "ABAAAAABB")),
    "boundary_R257": lambda: dense(3, 257, [170, 171, 0, 1, 63, 64, 65, 128, 129], topk=ALL, forms=("ABAAAAAAA", "ABAAAAAAA")),
    # mask boundary of the full workspace: 255 stays in det_class_nms_kernel, 256 / 257 / 320 / 321 go to the mask form
    "mask_R400": lambda: dense(4, 400, [255, 256, 257, 320, 321, 3, 0, 70], topk=ALL, size=(8, 50), forms=("BBBBBAAA", "BCCCCAAA")),
    "mask_R255": lambda: dense(5, 255, [255], topk=ALL, size=(8, 50), forms=("B", "B"), mask_offered_not_taken=True),
    # one class past the resolver's 4096-row LDS window, survivors there; per-class workspace: the 4160 candidates through form B
    "resolver_beyond_lds": lambda: dense(12, 4160, [4160], H=600, W=900, thr=NEG, nms=0.5, topk=4160, size=(40, 120), forms=("B", "C"),
                                         beyond_lds=True),
    # more than 4096 tiles: det_mask_kernel's grid-stride loop; a second class in the same tile list
    "mask_grid_stride": lambda: dense(7, 5800, [5770, 300], H=600, W=900, thr=NEG, nms=0.5, topk=8192, size=(40, 120), forms=("BA", "CC"),
                                      grid_stride=True),
    # the row limit: NB = 256 column blocks, ties everywhere
    "row_limit": lambda: dense(8, 16384, [16384], H=800, W=1333, thr=NEG, nms=0.5, topk=16384, size=(20, 100), quant=200, forms=("B", "C"),
                               row_limit=True),
    "topk_mid_chunk": lambda: topk_case("mid_chunk"), "topk_chunk_end": lambda: topk_case("chunk_end"),
    "topk_one": lambda: topk_case("one"), "topk_beyond": lambda: topk_case("beyond"), "topk_tie_cut": tie_cut_case,
    "scores_negative": lambda: scores_case("negative"), "scores_at_thresh": lambda: scores_case("at_thresh"),
    "zeros_A": lambda: zero_case(5), "zeros_C": lambda: zero_case(300),
    "neg_thresh_A": lambda: neg_thresh_case(5), "neg_thresh_C": lambda: neg_thresh_case(300),
    "boxes_edge": boxes_case,
}
for _thr, _pair in PAIRS.items():
    CASES["at_thresh_%g_A" % _thr] = functools.partial(pair_case, _pair, _thr, 5, at_equal=True)
    CASES["at_thresh_%g_C" % _thr] = functools.partial(pair_case, _pair, _thr, 300, at_equal=True)
CASES["class_offset_A"] = functools.partial(pair_case, OFFSET_PAIR, 0.5, 5, offset_pair=True)
CASES["class_offset_C"] = functools.partial(pair_case, OFFSET_PAIR, 0.5, 300, offset_pair=True)


def ref_of(c, **kw):
    return detect_ref(c["scores"], c["boxes"], c["H"], c["W"], c["thr"], c["nms"], c["topk"], **kw)


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, reference result), built once per process and shared by every test; callers must not write into them"""
    c = CASES[name]()
    for a in (c["scores"], c["boxes"]):
        a.setflags(write=False)
    return c, ref_of(c)


def forms(c, ref, full_workspace):
    R, K = c["scores"].shape[0], c["scores"].shape[1] - 1
    return "".join(route(int(n), R, K, full_workspace) for n in ref.nv)


def _kept(ref, row, cls):
    return bool(np.any((ref.rows[:ref.count] == row) & (ref.classes[:ref.count] == cls)))


def check_conditions(c, ref):
    """the properties a case's GPU test relies on, from the reference side only"""
    R, K = c["scores"].shape[0], c["scores"].shape[1] - 1
    assert list(ref.nv) == c["nv"]
    if "forms" in c:
        assert (forms(c, ref, False), forms(c, ref, True)) == c["forms"]
    if c.get("mask_offered_not_taken"):
        assert D.mask_bytes(R, K) > 0 and "C" not in forms(c, ref, True)
    if c.get("beyond_lds"):
        assert 4097 <= ref.nv[0] <= 4160 and int((ref.rank >= D.RES_CAP).sum()) >= 5          # survivors the resolver reads from global memory
    if c.get("grid_stride"):
        assert ref.nv[0] >= 5761 and D.mask_tiles(ref.nv, R, K) > D.MASK_GRID
    if c.get("row_limit"):
        assert R == D.MAX_ROWS and (R + 63) // 64 == 256 and ref.nv[0] == R and ref.count > 1000
        s = ref.scores[:ref.count]
        assert int((s[1:] == s[:-1]).sum()) > 500                                             # equal scores side by side: row order decided
    if "topk_kind" in c:
        u, kind, t = c["uncut"], c["topk_kind"], c["topk"]
        assert int((u.scores[1:u.count] == u.scores[:u.count - 1]).sum()) > 10                # equal scores inside the class
        if kind == "beyond":
            assert t > u.count and ref.count == u.count
        else:
            assert ref.count == t < u.count and same(ref, (t,) + tuple(x[:t] for x in u[1:5]))
            last = int(u.rank[t - 1])
            assert {"mid_chunk": 64 <= last < 128 and 20 <= last % 64 < 44, "chunk_end": last % 64 == 63, "one": t == 1}[kind]
    if c.get("tie_cut"):
        u, t = c["uncut"], c["topk"]
        assert ref.count == t and u.scores[t - 1] == u.scores[t] == u.scores[t + 1] and u.classes[t - 1] != u.classes[t]
        assert len(set(u.classes[:u.count][u.scores[:u.count] == u.scores[t]].tolist())) >= 2
        assert u.rows[t - 1] * K + u.classes[t - 1] < u.rows[t] * K + u.classes[t]             # r * K + c decided which one stayed
    if c.get("at_equal"):
        wrong = ref_of(c, suppress_at_equal=True)
        for cls in (0, 79):                                                                    # IoU == threshold exactly: `>` keeps both, `>=` one
            assert _kept(ref, 0, cls) and _kept(ref, 1, cls) and _kept(wrong, 0, cls) and not _kept(wrong, 1, cls)
    if c.get("offset_pair"):
        wrong = ref_of(c, class_offset=False)
        assert _kept(ref, 0, 0) and not _kept(ref, 1, 0)                                       # class 0: no offset, IoU just above 0.5
        assert _kept(ref, 0, 79) and _kept(ref, 1, 79) and not _kept(wrong, 1, 79)             # class 79: x2 rounds to 105387, IoU == 0.5
        assert not same(ref, wrong)
    if c.get("at_equal") or c.get("offset_pair"):
        b = np.minimum(c["boxes"].reshape(R, K, 4)[c["scores"][:, :K] > F(c["thr"])][:, 2], F(c["W"]))
        assert b.max() == 1333 and F(79) * F(b.max() + F(1)) == 105386
        assert forms(c, ref, True)[0] == forms(c, ref, True)[79] == ("C" if R >= 256 else "A")
        assert forms(c, ref, False)[0] == forms(c, ref, False)[79] == ("B" if R >= 256 else "A")
    if c.get("neg_thresh"):
        n0 = int((ref.classes[:ref.count] == 0).sum()); k1 = ref.rows[:ref.count][ref.classes[:ref.count] == 1]
        assert n0 == 1 and _kept(ref, 0, 0)                                                    # a best box with area stands alone
        assert len(k1) >= 3 and _kept(ref, 0, 1) and _kept(ref, 1, 1) and _kept(ref, 2, 1) and not _kept(ref, 3, 1)
        b = c["boxes"].reshape(R, K, 4)[k1, 1]
        assert bool(np.all((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) == 0))                    # all of them empty: NaN never suppresses
        assert set(forms(c, ref, True)) == ({"C"} if R >= 256 else {"A"}) and set(forms(c, ref, False)) == ({"B"} if R >= 256 else {"A"})
    if c.get("zeros"):
        assert np.signbit(c["scores"][2, 0]) and not np.signbit(c["scores"][7, 0]) and c["scores"][2, 0] == c["scores"][7, 0] == 0
        assert _kept(ref, 2, 0) and not _kept(ref, 7, 0) and _kept(ref, 1, 1) and _kept(ref, 3, 1)
        z = np.nonzero(ref.scores[:ref.count] == 0)[0]
        assert list(zip(ref.rows[z].tolist(), ref.classes[z].tolist())) == [(1, 1), (2, 0), (3, 1)]     # by r * K + c, whatever the sign
        assert set(forms(c, ref, True)) == ({"C"} if R >= 256 else {"A"}) and set(forms(c, ref, False)) == ({"B"} if R >= 256 else {"A"})
    if c.get("negative_scores"):
        assert bool(np.all(ref.scores[:ref.count] < 0)) and ref.count > 60 and bool(np.isneginf(c["scores"][:, :K]).any())
    if c.get("at_thresh"):
        assert int((c["scores"][:, :K] == F(c["thr"])).sum()) > 20                             # scores exactly at the threshold: not candidates
    if c.get("boxes_edge"):
        keep = sorted(ref.rows[:ref.count].tolist())
        assert keep == [0, 1, 2, 3, 4, 6, 7, 8, 9] and c["H"] != c["W"]                        # only the duplicate with area (row 5) falls
        b = ref.boxes[np.argsort(ref.rows[:ref.count])]
        assert b[0].tolist() == [0, 0, 0, 0] and b[1].tolist() == [500, 100, 500, 200] and b[2].tolist() == [100, 300, 200, 300]
        assert b[3].tolist() == [0, 0, 500, 300]
    return True


# ------------------------------------------------------------------------------------------------------------------ the tests
def _small_random(rng):
    n = int(rng.randint(0, 61)); K = int(rng.choice([1, 2, 5]))
    R = max(1, n)
    H, W = int(rng.randint(20, 200)), int(rng.randint(20, 200))
    thr = float(rng.choice([NEG, 0.1]))
    s = np.round(rng.uniform(0, 1, (R, K + 1)) * rng.choice([4, 20, 1000])).astype(F) / F(rng.choice([4, 20, 1000]))
    s[rng.uniform(size=s.shape) < 0.1] = 0.0
    s[rng.uniform(size=s.shape) < 0.05] = -0.0
    grid = float(rng.choice([1, 8, 0.37]))
    b = (np.round(rng.uniform(-20, max(H, W) + 20, (R, K, 4)) / grid) * grid).astype(F)
    b[..., 2:] = np.maximum(b[..., 2:], b[..., :2])
    deg = rng.uniform(size=(R, K)) < 0.15
    b[deg, 2] = b[deg, 0]                                                      # empty boxes
    dup = rng.uniform(size=R) < 0.2
    b[dup] = b[0]; s[dup] = s[0]                                               # exact duplicates, scores included
    return s, b.reshape(R, 4 * K), H, W, thr, float(rng.choice([0.3, 0.5, 0.7, 0.0, -1.0])), int(rng.choice([1, 5, 1000]))


def test_vectorised_equals_scalar_on_small_inputs():
    rng = np.random.RandomState(11)
    kept = 0
    for _ in range(200):
        a = _small_random(rng)
        v, s = detect_ref(*a), detect_ref_scalar(*a)
        assert same(v, s) and np.array_equal(v.nv, s.nv) and np.array_equal(v.rank, s.rank)
        assert np.array_equal(v.scores.view(np.uint32), s.scores.view(np.uint32))
        kept += v.count
    assert kept > 1000


def test_nms_step_equals_the_oracle_in_one_pass_form():
    """batched_nms as the reference runs it: ONE greedy pass over all classes on the offset boxes (oracle.oicr_oracle.nms_keep)"""
    from oracle import oicr_oracle as O
    for name in ("boundary_R257", "mask_R400", "scores_at_thresh", "at_thresh_0.5_A", "class_offset_C", "topk_tie_cut", "boxes_edge"):
        c, ref = case(name)
        R, K = c["scores"].shape[0], c["scores"].shape[1] - 1
        s = c["scores"][:, :K]; pb = c["boxes"].reshape(R, K, 4).copy()
        pb[..., 0::2] = pb[..., 0::2].clip(0, c["W"]); pb[..., 1::2] = pb[..., 1::2].clip(0, c["H"])
        r_idx, c_idx = np.nonzero(s > F(c["thr"]))
        bsel, ssel = pb[r_idx, c_idx], s[r_idx, c_idx]
        off = c_idx.astype(F) * F(bsel.max() + 1)
        keep = O.nms_keep((bsel + off[:, None]).astype(F), ssel, c["nms"])[:c["topk"]]
        assert same(ref, (len(keep), bsel[keep], ssel[keep], c_idx[keep], r_idx[keep])), name


@pytest.mark.parametrize("name", [n for n in CASES])
def test_case_has_the_property_its_gpu_test_relies_on(name):
    c, ref = case(name)
    assert check_conditions(c, ref)


def test_fuzz_seed_reaches_every_form():
    reached = {"A": 0, "B": 0, "C": 0}
    for i in range(FUZZ_N):
        c = fuzz_case(i)
        R, K = c["scores"].shape[0], c["scores"].shape[1] - 1
        seen = set("".join(route(n, R, K, full) for n in c["nv"]) for full in (False, True))
        seen = set("".join(seen))
        for f in seen:
            reached[f] += 1
    assert min(reached.values()) >= 5, reached


def test_route_restates_the_entry():
    assert [route(n, 64, 1, True) for n in (20, 21)] == ["A", "B"] and [route(n, 256, 1, False) for n in (84, 85)] == ["A", "B"]
    assert [route(n, 257, 1, False) for n in (170, 171)] == ["A", "B"] and [route(n, 400, 1, True) for n in (255, 256)] == ["B", "C"]
    assert route(255, 255, 1, True) == "B" and route(300, 1000, 1, False) == "A" and route(16384, 16384, 1, True) == "C"
    assert D.mask_bytes(16384, 1) > 0 and D.mask_bytes(16385, 1) == 0 and D.mask_bytes(16384, 4) == 0      # 96 MiB at most

"""The inputs of the evaluation kernels' edge tests (test_eval_edges_cpu.py, test_gpu_eval_edges.py), generated from seeds and
built once per process, with the restatements' answers (voc_eval_fixture.restated_detail, coco_eval_fixture.restated) cached
beside them.  Nothing here reads the code under test: the CPU tests assert that each case reaches the edge it is named for, the
GPU tests compare the kernels with the cached answers bit for bit.

VOC (csrc/evaluation.hip voc_match_kernel: 256 lanes per workgroup; voc_ap_kernel: tiles of 1024, np.sum's 8192-element chunks,
128-element leaves and eight accumulators):
  voc_tile_split      13 classes, three of them empty, the others at 1 .. 2049 detections around the 256 and 1024 edges
  voc_sum_split       one class per number of summed terms around 8, 128, 8192 and two chunks
  voc_tie_splits      hand-built ties and special values in exact arithmetic
  voc_contention_split  3000 detections claiming one object
COCO (coco_match_kernel: a pair in a wave's LDS slice when G <= 64 and D * G <= lds_doubles, else in the global workspace with
W = ceil(G / 64) words per walk; coco_accum_kernel: tiles of 1024 walked backward):
  coco_shape_split    one pair per (D, G) of COCO_SHAPES, each alone in its image and category
  coco_count_split    P small pairs; coco_trivial_split: P pairs of one detection and one object
  coco_accum_split    categories of 1023 .. 2049 listed detections with score ties, ignored detections and npig 1, 3, 100, 101
  coco_refusal_layout the kernel's arrays of one pair of D detections, which coco_eval_layout would have cut at 100"""
import functools

import numpy as np

import coco_eval_fixture as CF
import voc_eval_fixture as VF

VOC_TILE, VOC_LANES = 1024, 256

# ---- VOC ----------------------------------------------------------------------------------------------------------------------
TILE_ND = (0, 1, 255, 256, 257, 1023, 0, 1024, 1025, 2047, 2048, 2049, 0)      # detections per class; 0, 6 and 12 are empty
FAR = np.array([900.0, 900.0, 960.0, 950.0])                                       # overlaps no object of any case


@functools.lru_cache(maxsize=None)
def voc_tile_split():
    """-> (objs, dets, K).  Every image holds up to six objects of a class in a row of slots (41 x 41 pixels, 60 apart), a fifth
    of them difficult; a detection copies an object exactly, copies it shifted by up to 12 pixels (IoU on either side of every
    threshold), or lies far from all objects; scores have three decimals, so they tie.  Later ranks find most objects claimed."""
    rng = np.random.default_rng(101)
    K, n_img = len(TILE_ND), 300
    objs = [[] for _ in range(n_img)]
    for c, nd in enumerate(TILE_ND):
        if nd == 0 and c != 6:                        # class 6 has objects and no detection; 0 and 12 have neither
            continue
        for i in range(n_img):
            if rng.random() < 0.15:
                continue
            for k in range(int(rng.integers(1, 7))):
                objs[i].append((c, [10 + 60 * k, 10, 50 + 60 * k, 50], int(rng.random() < 0.2)))
    for o in objs:
        rng.shuffle(o)                                # classes interleave in annotation order
    dets = []
    for c, nd in enumerate(TILE_ND):
        img = rng.integers(0, n_img, nd)
        score = rng.integers(0, 1000, nd) / 1000
        box = np.empty((nd, 4))
        for d in range(nd):
            g = [o for o in objs[img[d]] if o[0] == c]
            if g and rng.random() < 0.8:
                b = np.array(g[int(rng.integers(0, len(g)))][1], dtype=np.float64)
                amp = (0, 0, 15, 40, 120)[int(rng.integers(0, 5))]
                box[d] = b + rng.integers(-amp, amp + 1, 4) / 10
            else:
                box[d] = FAR + rng.integers(0, 200, 4) / 10
        if nd >= 2:                                   # pass 2's last tile holds ranks 0 and 1 when nd is 1025 or 2049: a TP and an FP
            first, second = np.argsort(-score, kind="stable")[:2]
            i, o = next((i, o) for i in range(n_img) for o in objs[i] if o[0] == c and not o[2])
            img[first], box[first], box[second] = i, o[1], FAR
        dets.append((img, score, box))
    return objs, dets, K


SUM_TERMS = ((7, 8, 9, 127, 128, 129, 136), (8191, 8192), (8193, 16389))          # summed terms per class, one tuple per call
SUM_SEEDS = (201, 202, 212)                          # seeds at which every class meets test_eval_edges_cpu's order conditions


@functools.lru_cache(maxsize=None)
def voc_sum_split(call):
    """-> (objs, dets, K) with SUM_TERMS[call][c] terms in class c's area sum at every threshold.  M images hold one object of
    the class and one exact detection each, at distinct scores; every true positive is a recall change point.  A class at an even
    position has npos == M == n (the last recall is 1.0, so the closing sentinel adds nothing); one at an odd position has
    M == n - 1 and three more objects that nothing detects (recall ends below 1, the sentinel adds the n-th term).  False
    positives at random scores in between bend the precision envelope."""
    ns = SUM_TERMS[call]
    rng = np.random.default_rng(SUM_SEEDS[call])
    K = len(ns)
    n_img = max(ns) + 3
    objs = [[] for _ in range(n_img)]
    dets = []
    for c, n in enumerate(ns):
        M = n if c % 2 == 0 else n - 1
        for i in range(M + (0 if c % 2 == 0 else 3)):
            objs[i].append((c, [5 + i % 7, 5, 50 + i % 7, 45 + c], 0))
        n_fp = M // 3 + 2
        img = np.concatenate([np.arange(M), rng.integers(0, n_img, n_fp)])
        hit = np.array([objs[i][-1][1] for i in range(M)], dtype=np.float64).reshape(-1, 4)
        box = np.concatenate([hit, np.tile(FAR, (n_fp, 1))])
        score = np.concatenate([(rng.permutation(M) + 1) / (M + 1), rng.random(n_fp)])
        line = rng.permutation(M + n_fp)
        dets.append((img[line], score[line], box[line]))
    return objs, dets, K


@functools.lru_cache(maxsize=None)
def voc_tie_splits():
    """-> {name: (objs, dets, K)}.  All boxes are small integers or halves, so every IoU below is exact in f64.
    "ties": class 0 IoU exactly 0.5 and 0.75 (a match needs >); 1 two objects at equal IoU, difficult first in one image and second
    in the other (the first wins), a false positive ranked between them; 2 two detections of equal score on one object (the
    earlier line ranks first); 3 a best match that is difficult; 4 an image whose only object is difficult (no CorLoc slot);
    5 a NaN coordinate; 6 x2 < x1 with union 0.
    "npos0": class 1 has detections and only a difficult object.  "one_image": n_img == 1."""
    O = [1, 1, 10, 10]                                # 10 x 10 pixels
    ties_objs = [
        [(0, O, 0)], [(0, O, 0)], [(0, O, 0)],
        [(1, O, 1), (1, [3, 1, 12, 10], 0)], [(1, O, 0), (1, [3, 1, 12, 10], 1)],
        [(2, O, 0)],
        [(3, O, 1), (3, [1, 1, 10, 6], 0)],
        [(4, O, 1)], [(4, O, 0), (5, [20, 20, 40, 40], 0)],
        [(6, O, 0)],
    ]
    nan = float("nan")
    ties_dets = [
        ([0, 1, 2, 2], [0.9, 0.8, 0.7, 0.6], [[1, 1, 10, 5], [1, 1, 10, 7.5], O, O]),
        ([3, 4, 3], [0.9, 0.8, 0.85], [[2, 1, 11, 10], [2, 1, 11, 10], FAR]),
        ([5, 5, 5], [0.5, 0.5, 0.25], [O, [1, 1, 10, 9], FAR]),
        ([6, 6, 6], [0.9, 0.8, 0.7], [O, [1, 1, 10, 6], FAR]),
        ([7, 8, 7], [0.9, 0.8, 0.7], [O, [1, 1, 10, 8], O]),
        ([8, 8], [0.9, 0.8], [[nan, 20, 40, 40], [20, 20, 40, 40]]),
        ([9, 9, 9], [0.9, 0.8, 0.7], [[20, 1, 9, 10], O, [10, 1, 8, 10]]),
    ]
    npos0_objs = [[(0, O, 0)], [(1, O, 1)], []]
    npos0_dets = [([0, 2], [0.9, 0.5], [O, FAR]), ([1, 2, 1], [0.9, 0.8, 0.7], [O, FAR, [1, 1, 10, 7]])]
    one_objs = [[(0, O, 0), (1, [30, 30, 49, 49], 0), (0, [20, 1, 29, 10], 0)]]
    one_dets = [([0, 0, 0], [0.5, 0.75, 0.25], [[20, 1, 29, 10], [1, 1, 10, 8], FAR]), ([0, 0], [0.5, 0.5], [FAR, [30, 30, 49, 44]])]

    def arrays(dets):
        return [(np.asarray(i, dtype=np.int64), np.asarray(s, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(-1, 4))
                for i, s, b in dets]

    return {"ties": (ties_objs, arrays(ties_dets), 7), "npos0": (npos0_objs, arrays(npos0_dets), 2),
            "one_image": (one_objs, arrays(one_dets), 2)}


CONTENTION_DETS = 3000


@functools.lru_cache(maxsize=None)
def voc_contention_split():
    """-> (objs, dets, K): one 100 x 100 object and 3000 detections of it shifted right by dx whole pixels, IoU (100 - dx) /
    (100 + dx), at distinct scores; the lines are shuffled against the ranks.  The 600 best-ranked stay below IoU 0.7, so the
    claim of a threshold from 0.7 up is won by a lane of a later workgroup than the claims of the lower thresholds."""
    rng = np.random.default_rng(401)
    n = CONTENTION_DETS
    dx = rng.integers(0, 41, n)                       # by rank
    dx[:600] = rng.integers(18, 41, 600)
    score = 1.0 - np.arange(n) / n                    # rank r has the r-th largest score
    box = np.stack([10.0 + dx, np.full(n, 10.0), 109.0 + dx, np.full(n, 109.0)], 1)
    line = rng.permutation(n)
    objs = [[(0, [10, 10, 109, 109], 0)], []]
    return objs, [(np.zeros(n, dtype=np.int64), score[line], box[line])], 1


@functools.lru_cache(maxsize=None)
def voc_restated(name, call=None):
    """restated_detail of a VOC case, computed once: -> (ap_07, ap_area, corloc or None, detail)"""
    objs, dets, K = voc_case(name, call)
    corloc = not (name == "ties" and call == "npos0")
    return VF.restated_detail(objs, len(objs), dets, K, corloc=corloc)


def voc_case(name, call=None):
    if name == "tile":
        return voc_tile_split()
    if name == "sum":
        return voc_sum_split(call)
    if name == "ties":
        return voc_tie_splits()[call]
    assert name == "contention", name
    return voc_contention_split()


# ---- COCO ---------------------------------------------------------------------------------------------------------------------
# (D, G, crowd objects): "none", "some", or "all" (nvalid == 0 in every area range)
COCO_SHAPES = ((1, 1, "none"), (100, 16, "none"), (100, 17, "some"), (25, 64, "some"), (25, 65, "some"), (1, 64, "all"),
               (1, 65, "some"), (3, 128, "some"), (3, 129, "none"), (100, 200, "some"), (5, 0, "none"))
SIZES = ((10, 10), (32, 32), (50, 50), (96, 96), (200, 200), (20, 30), (64, 16), (16, 576))     # 32 * 32 and 96 * 96 are range edges
CELL = 500


def _cell(k):
    return float(CELL * (k % 20) + 100), float(CELL * (k // 20) + 100)


def coco_pair(rng, D, G, crowd):
    """-> (gts [(bbox, area, iscrowd)], dets [(bbox, score)]) of one (image, category).  The objects sit in cells 500 apart, so
    they overlap only inside the two clusters:
      area cluster   A [x, y, 40, 40] (medium) and B [x, y, 30, 34] (small) with a detection equal to B: in the medium range the
                     walk holds A (IoU 0.6375) when it reaches the ignored B (IoU 1) and stops there;
      crowd cluster  a crowd box around a plain one, the detection inside both: it holds the plain one (IoU 0.64) and stops at the
                     crowd box (IoU 1), the hand fixture's category 4.
    The detections, most wanted first: the clusters' two, IoU exactly 0.5 on a plain object, an exact copy and its duplicate, two
    inside one crowd box (a crowd box matches again), a miss of area exactly 32 * 32, then copies shifted on a 0.5 grid and
    misses of every size."""
    gts, cand, k = [], [], 0
    if G >= 2:
        x, y = _cell(k)
        k += 1
        gts += [([x, y, 40.0, 40.0], 1600.0, 0), ([x, y, 30.0, 34.0], 1020.0, 0)]
        cand.append([x, y, 30.0, 34.0])
    if G >= 4 and crowd != "none":
        x, y = _cell(k)
        k += 1
        gts += [([x - 10, y - 10, 80.0, 80.0], 6400.0, 1), ([x, y, 25.0, 25.0], 625.0, 0)]
        cand.append([x, y, 20.0, 20.0])
    singles = []
    while len(gts) < G:
        x, y = _cell(k)
        w, h = SIZES[k % len(SIZES)]
        is_crowd = int(crowd == "some" and len(singles) % 5 == 1)
        singles.append((len(gts), is_crowd))
        gts.append(([x, y, float(w), float(h)], float(w * h), is_crowd))
        k += 1
    if crowd == "all":
        gts = [(b, a, 1) for b, a, _ in gts]
    plain = [j for j, c in singles if not c and crowd != "all"]
    crowds = [j for j, c in singles if c or crowd == "all"]
    if plain:
        b = gts[plain[0]][0]
        cand.append([b[0], b[1], b[2], b[3] / 2])                             # IoU exactly 0.5
        b = gts[plain[-1]][0]
        cand += [list(b), list(b)]                                            # exact, and its duplicate
    if crowds:
        b = gts[crowds[0]][0]
        cand += [[b[0] + 1, b[1] + 1, b[2] / 2, b[3] / 2], [b[0] + 2, b[1] + 1, b[2] / 2, b[3] / 2]]
    x, y = _cell(k + 3)
    cand.append([x, y, 32.0, 32.0])
    if G == 1 and D == 1:
        cand = cand[:1]                                                       # the IoU 0.5 detection
    while len(cand) < D:
        u = rng.random()
        if singles and u < 0.7:
            b = gts[singles[int(rng.integers(0, len(singles)))][0]][0]
            s = (0, 1, 4, 10)[int(rng.integers(0, 4))]
            j = rng.integers(-s, s + 1, 4) / 2
            cand.append([b[0] + j[0], b[1] + j[1], max(1.0, b[2] + j[2]), max(1.0, b[3] + j[3])])
        else:
            x, y = _cell(k + 4 + int(rng.integers(0, 40)))
            w, h = SIZES[int(rng.integers(0, len(SIZES)))]
            cand.append([x + 250, y + 250, float(w), float(h)])
    dets = [([float(v) for v in b], int(rng.integers(1, 1000)) / 1000) for b in cand[:D]]
    return gts, dets


def _coco_split(pairs, extra_cats=()):
    """pairs: [(image id, category id, gts, dets)] -> (ds, res); image and category lists are written unsorted"""
    img_ids = list(dict.fromkeys(p[0] for p in pairs))
    cat_ids = list(dict.fromkeys([p[1] for p in pairs] + [c for c, _, _ in extra_cats]))
    ds = {"images": [{"id": int(i), "height": 480, "width": 640, "file_name": f"{int(i):012d}.jpg"} for i in img_ids[::-1]],
          "categories": [{"id": int(c), "name": f"c{c}"} for c in cat_ids[::-1]], "annotations": []}
    res = []
    for i, c, gts, dets in list(pairs) + [(i, c, g, []) for c, i, g in extra_cats]:
        for b, a, crowd in gts:
            ds["annotations"].append({"id": len(ds["annotations"]) + 1, "image_id": int(i), "category_id": int(c), "bbox": list(b),
                                      "area": float(a), "iscrowd": int(crowd)})
        for b, s in dets:
            res.append({"image_id": int(i), "category_id": int(c), "bbox": list(b), "score": float(s)})
    return ds, res


@functools.lru_cache(maxsize=None)
def coco_shape_split():
    """-> (ds, res, {(image id, category id): (D, G)}).  Shape s is alone in image 100 - 3 s and category 2 + 2 s; category 90 has
    ground truth (in the first shape's image) and no detection, so it forms no pair.  One annotation of the largest pair has id 0."""
    rng = np.random.default_rng(501)
    pairs, shape_of = [], {}
    for s, (D, G, crowd) in enumerate(COCO_SHAPES):
        gts, dets = coco_pair(rng, D, G, crowd)
        assert len(gts) == G and len(dets) == D
        pairs.append((100 - 3 * s, 2 + 2 * s, gts, dets))
        shape_of[100 - 3 * s, 2 + 2 * s] = (D, G)
    nodet = [([50.0, 50.0, 40.0, 40.0], 1600.0, 0)]
    ds, res = _coco_split(pairs, extra_cats=[(90, 100, nodet)])
    big = [a for a in ds["annotations"] if a["category_id"] == 2 + 2 * 9 and not a["iscrowd"]]
    big[-1]["id"] = 0                                 # takes its detection, never counts as matched
    order = rng.permutation(len(res))
    return ds, [res[k] for k in order], shape_of


COUNT_SHAPES = ((3, 2, "none"), (1, 1, "none"), (2, 5, "some"), (4, 1, "none"), (2, 66, "some"))


@functools.lru_cache(maxsize=None)
def coco_count_split(P):
    """P pairs, one image each, all in one category (a second category has no detection): P = 1 .. 5 leaves waves of the one
    workgroup without a pair"""
    rng = np.random.default_rng(600 + P)
    pairs = [(7 * p + 3, 4) + coco_pair(rng, *COUNT_SHAPES[p % len(COUNT_SHAPES)]) for p in range(P)]
    return _coco_split(pairs, extra_cats=[(9, 3, [([0.0, 0.0, 10.0, 10.0], 100.0, 0)])])


@functools.lru_cache(maxsize=None)
def coco_trivial_split(P):
    """P pairs of one detection and one object: an exact copy, IoU exactly 0.5, or a miss, with scores at fifty levels"""
    pairs = []
    for p in range(P):
        w, h = SIZES[p % len(SIZES)]
        b = [10.0, 20.0, float(w), float(h)]
        d = (b, [10.0, 20.0, float(w), h / 2], [300.0, 300.0, float(h), float(w)])[p % 3]
        pairs.append((p + 1, 1, [(b, float(w * h), int(p % 11 == 5))], [(d, (p * 7 % 50) / 50)]))
    return _coco_split(pairs)


# (listed detections after the cut at 100 per image, non-ignored objects in the "all" range, all false positives)
ACCUM_CATS = ((1023, 1, False), (1024, 3, False), (1025, 100, False), (2048, 101, False), (2049, 100, False), (1030, 3, True))
ACCUM_SEED = 707                                      # a seed at which the single true positive of category 0 is not at the list's head
ACCUM_PER_IMAGE = (1, 4, 12, 35, 60, 110)             # detections of the category in its images, in turn; 110 is cut to 100


@functools.lru_cache(maxsize=None)
def coco_accum_split():
    """-> (ds, res).  110 images shared by the categories.  A category's images take 1, 4, 12, 35, 60, 110 detections in turn
    until the listed count is reached, so in-image ranks 0, 1 .. 9 and 10 .. 99 all occur; the objects sit in the images of 12
    detections and more, each with an exact copy among them and shifted copies besides; scores have 200 levels, so they tie
    across images; every third image holds a crowd box with detections inside it (ignored), misses come in every size (ignored
    outside their area range)."""
    rng = np.random.default_rng(ACCUM_SEED)
    n_img = 110
    pairs = []
    for k, (n, npig, all_fp) in enumerate(ACCUM_CATS):
        counts, listed = [], 0
        while listed < n:
            raw = ACCUM_PER_IMAGE[len(counts) % len(ACCUM_PER_IMAGE)]
            take = min(raw, 100)
            if listed + take > n:
                raw = take = n - listed
            counts.append(raw)
            listed += take
        imgs = [(11 * k + j) % n_img + 1 for j in range(len(counts))]
        gts = [[] for _ in counts]
        roomy = [j for j, raw in enumerate(counts) if raw >= 12]
        for o in range(npig):
            j = roomy[(3 * o + 2) % len(roomy)]
            x, y = _cell(len(gts[j]))
            w, h = SIZES[o % len(SIZES)]
            gts[j].append(([x, y, float(w), float(h)], float(w * h), 0))
        for j in range(0, len(counts), 3):
            x, y = _cell(len(gts[j]))
            gts[j].append(([x, y, 120.0, 120.0], 14400.0, 1))
        for j, raw in enumerate(counts):
            plain = [g for g in gts[j] if not g[2]]
            crowd = [g for g in gts[j] if g[2]]
            dets = []
            for q in range(raw):
                u = rng.random()
                if q < len(plain) and not all_fp:     # every object has an exact copy, at whatever rank its score gives it
                    box = list(plain[q][0])
                elif plain and not all_fp and u < 0.5:
                    b = plain[int(rng.integers(0, len(plain)))][0]
                    s = (0, 0, 2, 8)[int(rng.integers(0, 4))]
                    q = rng.integers(-s, s + 1, 4) / 2
                    box = [b[0] + q[0], b[1] + q[1], max(1.0, b[2] + q[2]), max(1.0, b[3] + q[3])]
                elif crowd and u < 0.7:
                    b = crowd[0][0]
                    box = [b[0] + int(rng.integers(0, 60)), b[1] + int(rng.integers(0, 60)), 30.0, 40.0]
                else:
                    x, y = _cell(40 + int(rng.integers(0, 40)))
                    w, h = SIZES[int(rng.integers(0, len(SIZES)))]
                    box = [x + 250, y + 250, float(w), float(h)]
                dets.append((box, int(rng.integers(0, 200)) / 200))
            pairs.append((imgs[j], 10 + k, gts[j], dets))
    ds, res = _coco_split(pairs)
    order = rng.permutation(len(res))
    return ds, [res[q] for q in order]


def coco_case(name, arg=None):
    """-> (ds, res)"""
    if name == "shapes":
        return coco_shape_split()[:2]
    if name == "count":
        return coco_count_split(arg)
    if name == "trivial":
        return coco_trivial_split(arg)
    assert name == "accum", name
    return coco_accum_split()


@functools.lru_cache(maxsize=None)
def coco_restated(name, arg=None):
    """coco_eval_fixture.restated of a COCO case and its per-pair records, computed once: -> (ev, pairs)"""
    ds, res = coco_case(name, arg)
    pairs = {}
    return CF.restated(ds, res, pairs=pairs), pairs


def coco_expected_words(L, img_ids, cat_ids, pairs):
    """the kernel's match words [N, 2] i64 from the restatement's per-pair records: bit a * 10 + t of word 0 is detection_matches
    > 0, of word 1 detection_ignores, of area range a and threshold t; bits 40 .. 63 are zero.  L: coco_eval_layout's arrays (the
    host side's grouping, checked here against the restatement's order); img_ids / cat_ids: the sorted ids"""
    K = len(cat_ids)
    words = np.zeros((len(L["det_score"]), 2), dtype=np.int64)
    shift = (np.arange(4)[:, None] * 10 + np.arange(10)[None, :]).astype(np.int64)
    for p in range(len(L["pair_gt"])):
        rec = pairs[img_ids[int(L["pair_gt"][p]) // K], cat_ids[int(L["pair_gt"][p]) % K]]
        lo, hi = int(L["pair_off"][p]), int(L["pair_off"][p + 1])
        assert (L["det_index"][lo:hi] + 1).tolist() == rec["ids"], p
        for w, key in enumerate(("matched", "ignored")):
            words[lo:hi, w] = (rec[key].astype(np.int64) << shift[:, :, None]).sum((0, 1))
    return words


def coco_refusal_layout(D):
    """coco_eval_layout's arrays for one image, one category, one object and one pair of D detections (D up to 256: the in-image
    rank is a byte).  Detection 0 is the object's box, the others miss it."""
    assert 1 <= D <= 256
    box = np.tile(np.array([300.0, 300.0, 20.0, 20.0]), (D, 1))
    box[0] = [10.0, 10.0, 40.0, 40.0]
    box[1:, 0] += np.arange(1, D)
    return dict(n_img=1, K=1, pair_off=np.array([0, D], dtype=np.int64), pair_gt=np.zeros(1, dtype=np.int64),
                pair_ws=np.full(1, -1, dtype=np.int64), ws_words=0, det_box=box, det_rank=np.arange(D).astype(np.uint8),
                det_score=1.0 - np.arange(D) / 256, det_index=np.arange(D), gt_off=np.array([0, 1], dtype=np.int64),
                gt_box=np.array([[10.0, 10.0, 40.0, 40.0]]), gt_area=np.array([1600.0]), gt_flags=np.array([2], dtype=np.uint8),
                cat_off=np.array([0, D], dtype=np.int64), order=np.arange(D, dtype=np.int32),
                npig=np.array([[1, 0, 1, 0]], dtype=np.int64))

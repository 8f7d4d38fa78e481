"""NumPy references for the PGF threshold sweep (sos_wsod_amd.pgf_sweep over ops.pgf_sweep), and the case tables its tests share.

Two forms of the same tables (kept [nk, nc, K], tp / ign [nt, nk, nc, K], npos [K]):
  literal_tables     per cell: the reference's loops (tools/pgf.py class_filter :273-292, pgf :221-271, contain_cal :209-219) in
                     plain Python, then voc_eval's sequential loop (evaluation/pascal_voc_evaluation.py:357-397) over the kept
                     detections of each class in rank order (score descending, ties in list order);
  decomposed_tables  what the kernel computes: stage-4 bits per t_keep, the largest quotient per (detection, t_keep) compared
                     with every t_con, one ovmax / jmax per detection, claimed objects counted per cell.
A case is a dict of arrays in the kernel's own layout (see make_case).  Nothing here reads a GPU."""
import functools

import numpy as np

VOC_DIFF = (4, 5, 6, 8, 9, 15, 16)
IOU10 = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))


# ---- the reference's arithmetic ---------------------------------------------------------------------------------------------------
def contain_cal(a, b):
    """tools/pgf.py:209-219 on Python floats"""
    a, b = list(a), list(b)
    a[2] += a[0]; a[3] += a[1]; b[2] += b[0]; b[3] += b[1]
    c = [max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])]
    area_c = max(0, c[2] - c[0]) * max(0, c[3] - c[1])
    area_a = max(0, a[2] - a[0]) * max(0, a[3] - a[1])
    return area_c / (area_a + 1e-6)


def match_box(case, i):
    """the corners a detection is matched with"""
    x, y, w, h = case["boxes"][i]
    return np.array([x, y, x + w, y + h]) if case["xywh"] else np.array([x, y, w, h])


def overlaps(case):
    """per detection: (ovmax, jmax as a ground-truth row, or -1 without a candidate), voc_eval's lines on its image's objects of
    its class; computed once per case"""
    if "_ov" in case:
        return case["_ov"]
    p1 = 1.0 if case["plus_one"] else 0.0
    n = len(case["scores"])
    ovmax, jmax = np.full(n, -np.inf), np.full(n, -1, dtype=np.int64)
    for k in range(len(case["off"]) - 1):
        ga, gb = case["gt_off"][k], case["gt_off"][k + 1]
        for i in range(case["off"][k], case["off"][k + 1]):
            rows = ga + np.nonzero(case["gt_cls"][ga:gb] == case["classes"][i])[0]
            BBGT = case["gt_box"][rows]
            if BBGT.size == 0:
                continue
            bb = match_box(case, i)
            ixmin = np.maximum(BBGT[:, 0], bb[0]); iymin = np.maximum(BBGT[:, 1], bb[1])
            ixmax = np.minimum(BBGT[:, 2], bb[2]); iymax = np.minimum(BBGT[:, 3], bb[3])
            iw = np.maximum(ixmax - ixmin + p1, 0.0); ih = np.maximum(iymax - iymin + p1, 0.0)
            inters = iw * ih
            uni = (bb[2] - bb[0] + p1) * (bb[3] - bb[1] + p1) + (BBGT[:, 2] - BBGT[:, 0] + p1) * (BBGT[:, 3] - BBGT[:, 1] + p1) - inters
            with np.errstate(invalid="ignore", divide="ignore"):
                ov = inters / uni
            ovmax[i], jmax[i] = np.max(ov), rows[np.argmax(ov)]
    case["_ov"] = (ovmax, jmax)
    return case["_ov"]


def npos_of(case):
    npos = np.zeros(case["K"], dtype=np.int64)
    np.add.at(npos, case["gt_cls"][case["gt_ign"] == 0], 1)
    return npos


def match_cell(case, keep):
    """voc_eval's sequential loop over the kept detections (keep: bool [N]) -> (kept [K], tp [nt, K], ign [nt, K])"""
    K, nt = case["K"], len(case["iou"])
    ovmax, jmax = overlaps(case)
    kept, tp, ign = np.zeros(K, dtype=np.int64), np.zeros((nt, K), dtype=np.int64), np.zeros((nt, K), dtype=np.int64)
    idx = np.nonzero(keep)[0]
    np.add.at(kept, case["classes"][idx], 1)
    for c in np.unique(case["classes"][idx]):
        d = idx[case["classes"][idx] == c]
        d = d[np.argsort(-case["scores"][d], kind="stable")]
        for t, thr in enumerate(case["iou"]):
            det = set()
            for i in d:
                if ovmax[i] > thr:
                    j = jmax[i]
                    if case["gt_ign"][j]:
                        ign[t, c] += 1
                    elif j not in det:
                        tp[t, c] += 1
                        det.add(j)
    return kept, tp, ign


# ---- literal form -----------------------------------------------------------------------------------------------------------------
def literal_keep(case, t_keep, t_con, quotients=None):
    """class_filter, then the two loops of pgf, per image, on Python lists -> bool [N]"""
    keep = np.zeros(len(case["scores"]), dtype=bool)
    quotients = {} if quotients is None else quotients
    for k in range(len(case["off"]) - 1):
        a = int(case["off"][k])
        preds = [i for i in range(a, int(case["off"][k + 1])) if int(case["classes"][i]) in case["gt_sets"][k]]
        seen, mid = [], []
        for i in preds:
            c = int(case["classes"][i])
            if c not in seen:
                seen.append(c)
                mid.append(i)
                continue
            if case["scores"][i] < t_keep:
                continue
            mid.append(i)
        save = [True] * len(mid)
        for bi, i in enumerate(mid):
            for bj, j in enumerate(mid):
                if bi == bj or case["classes"][i] != case["classes"][j]:
                    continue
                if not case["use_diff"] and int(case["classes"][i]) in case["diff"]:
                    continue
                if (i, j) not in quotients:
                    quotients[(i, j)] = contain_cal(case["boxes"][i].tolist(), case["boxes"][j].tolist())
                if quotients[(i, j)] >= t_con:
                    save[bi] = False
        for bi, i in enumerate(mid):
            keep[i] = save[bi]
    return keep


def literal_tables(case):
    nk, nc, nt, K = len(case["t_keep"]), len(case["t_con"]), len(case["iou"]), case["K"]
    kept = np.zeros((nk, nc, K), dtype=np.int64)
    tp, ign = np.zeros((nt, nk, nc, K), dtype=np.int64), np.zeros((nt, nk, nc, K), dtype=np.int64)
    quotients = {}
    for a, tk in enumerate(case["t_keep"]):
        for b, tc in enumerate(case["t_con"]):
            kept[a, b], tp[:, a, b], ign[:, a, b] = match_cell(case, literal_keep(case, tk, tc, quotients))
    return {"kept": kept, "tp": tp, "ign": ign, "npos": npos_of(case)}


# ---- decomposed form --------------------------------------------------------------------------------------------------------------
def decomposed_tables(case):
    nk, nc, nt, K = len(case["t_keep"]), len(case["t_con"]), len(case["iou"]), case["K"]
    t_keep, t_con, iou = (np.asarray(case[g], dtype=np.float64) for g in ("t_keep", "t_con", "iou"))
    kept = np.zeros((nk, nc, K), dtype=np.int64)
    tp, ign = np.zeros((nt, nk, nc, K), dtype=np.int64), np.zeros((nt, nk, nc, K), dtype=np.int64)
    ovmax, jmax = overlaps(case)
    for k in range(len(case["off"]) - 1):
        lo, hi = int(case["off"][k]), int(case["off"][k + 1])
        cls = case["classes"][lo:hi]
        for c in sorted(set(cls.tolist()) & case["gt_sets"][k]):
            mem = lo + np.nonzero(cls == c)[0]
            s = case["scores"][mem]
            surv = ~(s[:, None] < t_keep[None, :])                                   # [n, nk]
            surv[0] = True                                                           # the first of its class stays
            bx = case["boxes"][mem]
            x2, y2 = bx[:, 0] + bx[:, 2], bx[:, 1] + bx[:, 3]
            cx1 = np.where(bx[None, :, 0] > bx[:, None, 0], bx[None, :, 0], bx[:, None, 0])
            cy1 = np.where(bx[None, :, 1] > bx[:, None, 1], bx[None, :, 1], bx[:, None, 1])
            cx2 = np.where(x2[None, :] < x2[:, None], x2[None, :], x2[:, None])
            cy2 = np.where(y2[None, :] < y2[:, None], y2[None, :], y2[:, None])
            w, h = cx2 - cx1, cy2 - cy1
            area_c = np.where(w > 0, w, 0.0) * np.where(h > 0, h, 0.0)
            aw, ah = x2 - bx[:, 0], y2 - bx[:, 1]
            area_a = np.where(aw > 0, aw, 0.0) * np.where(ah > 0, ah, 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                q = area_c / (area_a + 1e-6)[:, None]                                # [i, j]
            np.fill_diagonal(q, np.nan)
            m = np.full((len(mem), nk), -np.inf)
            for j in range(len(mem)):                                                # `v > m ? v : m`, a NaN never enters
                v = np.where(surv[j][None, :], q[:, j][:, None], np.nan)
                m = np.where(v > m, v, m)
            leaves = m[:, :, None] >= t_con[None, None, :]
            if not case["use_diff"] and c in case["diff"]:
                leaves[:] = False
            cell = surv[:, :, None] & ~leaves                                        # [n, nk, nc]
            kept[:, :, c] += cell.sum(0)
            hit = ovmax[mem][:, None] > iou[None, :]                                 # [n, nt]
            ig = np.array([j >= 0 and case["gt_ign"][j] != 0 for j in jmax[mem]], dtype=bool)
            ign[:, :, :, c] += np.einsum("it,iab->tab", (hit & ig[:, None]).astype(np.int64), cell.astype(np.int64))
            for g in np.unique(jmax[mem][(jmax[mem] >= 0) & ~ig]):
                of = jmax[mem] == g
                claim = (hit[of][:, :, None, None] & cell[of][:, None, :, :]).any(0)  # [nt, nk, nc]
                tp[:, :, :, c] += claim
    return {"kept": kept, "tp": tp, "ign": ign, "npos": npos_of(case)}


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _image(rng, n_det, K, own, n_obj, xywh, all_ignored=False, force_class=None):
    """one image: `own` its ground-truth classes, n_obj[c] objects of each; detections are jittered copies of objects and of each
    other on a coarse lattice, so that nesting, duplicates, exact quotients and equal overlaps occur"""
    gt_box, gt_cls = [], []
    for c in own:
        for _ in range(n_obj[c]):
            x1, y1 = rng.integers(0, 12, 2) * 8.0 + 1.0
            w, h = rng.integers(2, 12, 2) * 8.0
            gt_box.append([x1, y1, x1 + w, y1 + h]); gt_cls.append(c)
    gt_box = np.array(gt_box, dtype=np.float64).reshape(-1, 4)
    gt_cls = np.array(gt_cls, dtype=np.int32)
    gt_ign = np.ones(len(gt_cls), dtype=np.uint8) if all_ignored else (rng.random(len(gt_cls)) < 0.2).astype(np.uint8)
    own_list = np.array(sorted(own))
    if force_class is not None:
        classes = np.full(n_det, force_class, dtype=np.int32)
    else:
        classes = np.where(rng.random(n_det) < 0.8, rng.choice(own_list, n_det), rng.integers(0, K, n_det)).astype(np.int32)
    corners = np.empty((n_det, 4))
    for i in range(n_det):
        rows = np.nonzero(gt_cls == classes[i])[0]
        if len(rows) and rng.random() < 0.7:
            b = gt_box[rng.choice(rows)].copy()
            b += rng.integers(-2, 3, 4) * 4.0 * (rng.random() < 0.7)
        else:
            x1, y1 = rng.integers(0, 12, 2) * 8.0 + 1.0
            b = np.array([x1, y1, x1 + rng.integers(0, 12) * 8.0, y1 + rng.integers(0, 12) * 8.0])
        corners[i] = b
    boxes = corners.copy()
    if xywh:
        boxes[:, 2:] = np.maximum(corners[:, 2:] - corners[:, :2], 0.0)
    scores = rng.integers(0, 101, n_det) / 100.0
    return boxes, scores, classes, gt_box, gt_cls, gt_ign


def _grid(rng, case, nk, nc):
    """unsorted grids with repeats: t_keep holds a negative value, 0, a value above every score and scores themselves; t_con holds
    0, a value above 1, and a pair's quotient with its two float64 neighbours"""
    scores, off, cls = case["scores"], case["off"], case["classes"]
    tk = [0.2, -0.5, 0.0, 0.2, 1.5] + (rng.choice(scores, 4).tolist() if len(scores) else [])
    q = None
    for k in range(len(off) - 1):                                                    # the first same-class pair with 0 < quotient < 1
        for i in range(off[k], off[k + 1]):
            for j in range(off[k], off[k + 1]):
                if i != j and cls[i] == cls[j] and int(cls[i]) in case["gt_sets"][k]:
                    v = contain_cal(case["boxes"][i].tolist(), case["boxes"][j].tolist())
                    if 0.0 < v < 1.0:
                        q = v
                        break
            if q is not None:
                break
        if q is not None:
            break
    q = 0.85 if q is None else q
    tc = [q, float(np.nextafter(q, -np.inf)), float(np.nextafter(q, np.inf)), 0.0, 1.25, 0.85, 0.85]
    while len(tk) < nk:
        tk.append(float(rng.integers(0, 101)) / 100.0)
    while len(tc) < nc:
        tc.append(float(rng.integers(30, 101)) / 100.0)
    tk = [tk[i] for i in rng.permutation(len(tk))][:nk] if nk >= 9 else tk[:nk]
    tc = [tc[i] for i in rng.permutation(len(tc))][:nc] if nc >= 7 else tc[:nc]
    return [float(v) for v in tk], [float(v) for v in tc]


def _assemble(images, K, gt_sets, xywh, use_diff):
    off = np.zeros(len(images) + 1, dtype=np.int64)
    gt_off = np.zeros(len(images) + 1, dtype=np.int64)
    for k, im in enumerate(images):
        off[k + 1] = off[k] + len(im[1])
        gt_off[k + 1] = gt_off[k] + len(im[4])

    def cat(j, shape, dtype):
        """field j of every image (_image's order), back to back"""
        return np.concatenate([np.asarray(im[j], dtype=dtype).reshape(shape) for im in images])

    return {"off": off, "boxes": cat(0, (-1, 4), np.float64), "scores": cat(1, (-1,), np.float64), "classes": cat(2, (-1,), np.int32),
            "K": K, "gt_sets": gt_sets, "gt_off": gt_off, "gt_box": cat(3, (-1, 4), np.float64), "gt_cls": cat(4, (-1,), np.int32),
            "gt_ign": cat(5, (-1,), np.uint8), "diff": VOC_DIFF, "use_diff": use_diff, "xywh": xywh, "plus_one": not xywh}


def _random_case(seed, det_counts, K, nk, nc, iou, xywh, use_diff, obj_counts=(0, 1, 2, 3), all_ignored=False, one_class=()):
    """det_counts: detections per image; one_class: images whose detections are all of one ground-truth class (member counts at
    the lane-batch edges)"""
    rng = np.random.default_rng(seed)
    images, gt_sets = [], []
    for k, n in enumerate(det_counts):
        own = set(rng.choice(K, min(K, int(rng.integers(1, 4))), replace=False).tolist())
        n_obj = {c: int(rng.choice(obj_counts)) for c in own}
        force = sorted(own)[0] if k in one_class else None
        if force is not None:
            n_obj[force] = 3                                                         # objects to claim from more than one lane batch
        images.append(_image(rng, n, K, own, n_obj, xywh, all_ignored, force))
        gt_sets.append(own)
    case = _assemble(images, K, gt_sets, xywh, use_diff)
    case["t_keep"], case["t_con"] = _grid(rng, case, nk, nc)
    case["iou"] = [float(v) for v in iou]
    return case


def _edge_case():
    """hand-made, VOC mode, one class per image unless said: IoU exactly at a threshold; two objects with equal IoU; two identical
    kept detections on one object; the best object ignored"""
    ims = []
    # IoU 100 / 200 = 0.5 exactly: no match at 0.5
    ims.append(([[1, 1, 10, 10]], [0.9], [0], [[1, 1, 10, 20]], [0], [0]))
    # two objects with equal IoU: the first wins; the second is never claimed
    ims.append(([[11, 11, 30, 30]], [0.9], [1], [[11, 11, 30, 40], [11, 1, 30, 30]], [1, 1], [0, 0]))
    # two identical detections claim one object (class 4 is exempt from containment without use_diff: both stay)
    ims.append(([[5, 5, 24, 24], [5, 5, 24, 24]], [0.9, 0.8], [4, 4], [[5, 5, 24, 24]], [4], [0]))
    # the best object is ignored, a worse one is not: ign only
    ims.append(([[3, 3, 22, 22]], [0.7], [2], [[3, 3, 22, 22], [3, 3, 22, 30]], [2, 2], [1, 0]))
    # a detection of a ground-truth class that has no object row (the class mask alone admits it), and one of a foreign class
    ims.append(([[3, 3, 22, 22], [3, 3, 22, 22]], [0.7, 0.6], [3, 7], np.zeros((0, 4)), [], []))
    gt_sets = [{0}, {1}, {4}, {2}, {3}]
    case = _assemble(ims, 20, gt_sets, False, False)
    case["t_keep"], case["t_con"], case["iou"] = [0.2], [0.85], [0.5, 0.45, 0.75]
    return case


CASES = {
    # detections per image at every staging and lane-batch edge; 11 images: no multiple of the waves per workgroup
    "sizes_voc": lambda: _random_case(1, [0, 1, 2, 63, 64, 65, 255, 256, 257, 600, 30], 20, 7, 5, IOU10, False, False),
    "sizes_voc_diff": lambda: _random_case(2, [0, 1, 2, 63, 64, 65, 255, 256, 257, 600, 30], 20, 7, 5, IOU10, False, True),
    # all detections of one class: 63 / 64 / 65 / 130 / 300 members
    "members": lambda: _random_case(3, [63, 64, 65, 130, 300], 20, 3, 5, (0.5, 0.75), True, True, one_class=(0, 1, 2, 3, 4)),
    "grid_1x1": lambda: _random_case(4, [20, 0, 40, 7, 33], 20, 1, 1, (0.5,), False, False),
    "grid_1x32": lambda: _random_case(5, [20, 9, 40], 80, 1, 32, IOU10, True, True),
    "grid_32x1": lambda: _random_case(6, [20, 9, 40], 80, 32, 1, IOU10, True, True),
    "grid_32x32": lambda: _random_case(7, [24, 3, 40, 0, 31, 12, 18], 80, 32, 32, IOU10, True, True),
    "objects": lambda: _random_case(8, [30, 30, 30, 30, 30], 20, 7, 5, IOU10, False, False, obj_counts=(0, 1, 64, 65)),
    "all_ignored": lambda: _random_case(9, [30, 12, 1], 20, 3, 3, IOU10, False, True, all_ignored=True),
    "K1": lambda: _random_case(10, [12, 5, 70], 1, 3, 2, (0.5, 0.6), True, True),
    "K32": lambda: _random_case(11, [40, 5, 9], 32, 3, 2, (0.5, 0.6), False, False),
    "K33": lambda: _random_case(12, [40, 5, 9], 33, 3, 2, (0.5, 0.6), True, True),
    "K256": lambda: _random_case(13, [90, 5, 9], 256, 3, 2, (0.5, 0.6), True, True),
    "edges": _edge_case,
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """the case and its tables (decomposed form), computed once and shared: treat both as read-only"""
    case = CASES[name]()
    case["expected"] = decomposed_tables(case)
    return case


def masks(case):
    """gt_mask [n_img, words] and diff_mask [words] as uint32"""
    K = case["K"]
    words = (K + 31) // 32
    gt_mask = np.zeros((len(case["gt_sets"]), words), dtype=np.uint32)
    for k, s in enumerate(case["gt_sets"]):
        for c in s:
            gt_mask[k, c >> 5] |= np.uint32(1 << (c & 31))
    diff_mask = np.zeros(words, dtype=np.uint32)
    for c in case["diff"]:
        if c < K:
            diff_mask[c >> 5] |= np.uint32(1 << (c & 31))
    return gt_mask, diff_mask

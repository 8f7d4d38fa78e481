"""Checker for sw_detect_postprocess: the tail of the reference's fast_rcnn_inference_single_image (fast_rcnn_oicr.py:116-141: clip,
score filter, batched_nms on class-offset boxes, keep[:topk]) with torchvision's nms_cpu arithmetic, restated in NumPy float32 with ONE
rounding per operation in the reference's order.  The keep set is a chain of float32 comparisons, so float32 IS the truth here: a
float64 restatement decides IoU-at-the-threshold pairs and the rounding of the class offset differently, i.e. wrongly.

  clip to (W, H)  ->  score > thresh over the K foreground columns, positions in nonzero order r * K + c  ->  max_coord over the filtered
  clipped boxes  ->  box + float32(c) * float32(max_coord + 1)  ->  per class: score descending (by VALUE: -0.0 == +0.0), ties by position
  ascending; greedy, a later box falls when iou > float32(nms_thresh) against an earlier KEPT one, area = (x2 - x1) * (y2 - y1),
  inter = max(0, .) * max(0, .), iou = inter / ((a_i + a_j) - inter)  ->  all survivors by score descending, position ascending  ->  [:topk]

batched_nms runs ONE greedy pass over all classes; boxes of different classes never meet after the offset (inter == 0, so iou is 0 or
NaN, never > a threshold >= 0), so the pass per class below keeps the same set (test_detect_ref_cpu.py pins that against
oracle.oicr_oracle.nms_keep on the one-pass form).  For nms_thresh < 0 the per-class pass is the project's contract (include/soswsod_hip.h).

Two implementations: detect_ref_scalar (a pure-Python loop over pairs, small inputs) and detect_ref (one vectorised pass per kept box).
Both return DetRef(count, boxes, scores, classes, rows, nv, rank): nv[c] = candidates of class c, rank[t] = position of detection t in
its class's sorted candidate list.  `route` restates which of the entry's three forms a class of nv candidates takes.  NumPy only.
"""
from collections import namedtuple

import numpy as np

DetRef = namedtuple("DetRef", "count boxes scores classes rows nv rank")
F = np.float32

MASK_MIN = 256          # sw_detect_postprocess: a class of this many candidates takes the mask form when the workspace offers it
RES_CAP = 4096          # det_resolve_kernel: mask rows of a chunk staged in LDS
MASK_GRID = 4096        # det_mask_kernel: workgroups at most; more tiles than this are walked by its grid-stride loop
MAX_ROWS = 16384        # R and K * topk at most


def next_pow2(n):
    p = 64
    while p < n:
        p <<= 1
    return p


def _align256(v):
    return (v + 255) // 256 * 256


def base_bytes(K, topk):
    """sw_detect_workspace_bytes(0, K, topk): the per-class form's workspace"""
    return _align256(K * topk * 8 + K * 4 + 64)


def mask_bytes(R, K):
    """what sw_detect_workspace_bytes(R, K, topk) adds for the mask form; 0 = not offered"""
    if R < 1 or K < 1 or R > MAX_ROWS:
        return 0
    NB = (R + 63) // 64
    b = _align256(K * 4) + _align256(K * R * 8) + _align256(K * R * 16) + K * NB * R * 8
    return b if b <= (96 << 20) else 0


def route(nv, R, K, full_workspace):
    """'A' chunked LDS form, 'B' one-box-at-a-time loop, 'C' mask form (det_mask_kernel + det_resolve_kernel)"""
    if full_workspace and mask_bytes(R, K) > 0 and R >= MASK_MIN and nv >= MASK_MIN:
        return "C"
    return "A" if nv * 16 + 16 <= (next_pow2(R) - nv) * 8 else "B"


def mask_tiles(nvs, R, K):
    """64 x 64 tiles det_mask_kernel walks for these per-class counts (full workspace)"""
    return sum(nb * (nb + 1) // 2 for nb in ((n + 63) // 64 for n in nvs if route(n, R, K, True) == "C"))


def _candidates(all_scores, all_boxes, img_h, img_w, thresh, class_offset):
    s = np.ascontiguousarray(all_scores, dtype=F)
    R, K = s.shape[0], s.shape[1] - 1
    b = np.array(all_boxes, dtype=F).reshape(R, K, 4)
    assert np.isfinite(b).all(), "finite boxes only (the reference drops non-finite rows, the kernel does not)"
    b[..., 0::2] = np.minimum(np.maximum(b[..., 0::2], F(0)), F(img_w))
    b[..., 1::2] = np.minimum(np.maximum(b[..., 1::2], F(0)), F(img_h))
    r_idx, c_idx = np.nonzero(s[:, :K] > F(thresh))
    bsel, ssel = b[r_idx, c_idx], s[r_idx, c_idx]
    max_coord = bsel.max() if len(r_idx) else F(0)
    off = c_idx.astype(F) * F(max_coord + F(1)) if class_offset else np.zeros(len(r_idx), F)
    ob = (bsel + off[:, None]).astype(F)
    return R, K, r_idx, c_idx, bsel, ssel, ob


def _finish(K, topk, r_idx, c_idx, bsel, ssel, kept, kept_rank, nv):
    kept = np.asarray(kept, np.int64); kept_rank = np.asarray(kept_rank, np.int64)
    pos = r_idx[kept] * K + c_idx[kept]
    final = np.lexsort((pos, -ssel[kept].astype(np.float64)))[:topk]          # -x in float64 of a float32 is exact; -0.0 == 0.0
    k = kept[final]
    return DetRef(len(k), bsel[k].copy(), ssel[k].copy(), c_idx[k].astype(np.int32), r_idx[k].astype(np.int32), nv, kept_rank[final])


def detect_ref(all_scores, all_boxes, img_h, img_w, thresh, nms_thresh, topk, class_offset=True, suppress_at_equal=False):
    """vectorised: one float32 NumPy pass per kept box.  class_offset=False / suppress_at_equal=True are the two WRONG variants the
    tests use to show that an input is sensitive to the offset's rounding / to `>` against `>=`."""
    R, K, r_idx, c_idx, bsel, ssel, ob = _candidates(all_scores, all_boxes, img_h, img_w, thresh, class_offset)
    thr = F(nms_thresh)
    nv = np.bincount(c_idx, minlength=K).astype(np.int64)
    kept, kept_rank = [], []
    for c in range(K):
        idx = np.nonzero(c_idx == c)[0]                                         # position ascending
        if not len(idx):
            continue
        order = idx[np.argsort(-ssel[idx], kind="stable")]                      # compares by value; stable keeps position order in ties
        b = ob[order]
        area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F)
        sup = np.zeros(len(order), bool)
        nk = 0
        for t in range(len(order)):
            if sup[t]:
                continue
            kept.append(order[t]); kept_rank.append(t); nk += 1
            if nk >= topk:
                break                                                           # the global cut cannot reach deeper into a class
            r = b[t + 1:]
            w = np.maximum(F(0), (np.minimum(b[t, 2], r[:, 2]) - np.maximum(b[t, 0], r[:, 0])).astype(F))
            h = np.maximum(F(0), (np.minimum(b[t, 3], r[:, 3]) - np.maximum(b[t, 1], r[:, 1])).astype(F))
            inter = (w * h).astype(F)
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = (inter / ((area[t] + area[t + 1:]).astype(F) - inter).astype(F)).astype(F)
            sup[t + 1:] |= (iou >= thr) if suppress_at_equal else (iou > thr)
    return _finish(K, topk, r_idx, c_idx, bsel, ssel, kept, kept_rank, nv)


def detect_ref_scalar(all_scores, all_boxes, img_h, img_w, thresh, nms_thresh, topk, class_offset=True, suppress_at_equal=False):
    """the same with every pair in a Python loop on np.float32 scalars (nms_cpu.cpp line by line); O(n^2): small inputs only"""
    R, K, r_idx, c_idx, bsel, ssel, ob = _candidates(all_scores, all_boxes, img_h, img_w, thresh, class_offset)
    thr = F(nms_thresh)
    nv = np.zeros(K, np.int64)
    kept, kept_rank = [], []
    for c in range(K):
        idx = [i for i in range(len(c_idx)) if c_idx[i] == c]
        nv[c] = len(idx)
        order = sorted(idx, key=lambda i: (-float(ssel[i]), i))                 # -0.0 == 0.0 as floats; then position
        area = [F(F(ob[i, 2] - ob[i, 0]) * F(ob[i, 3] - ob[i, 1])) for i in order]
        sup = [False] * len(order)
        for ti, i in enumerate(order):
            if sup[ti]:
                continue
            kept.append(i); kept_rank.append(ti)
            for tj in range(ti + 1, len(order)):
                if sup[tj]:
                    continue
                j = order[tj]
                xx1 = max(ob[i, 0], ob[j, 0]); yy1 = max(ob[i, 1], ob[j, 1])
                xx2 = min(ob[i, 2], ob[j, 2]); yy2 = min(ob[i, 3], ob[j, 3])
                w = max(F(0), F(xx2 - xx1)); h = max(F(0), F(yy2 - yy1))
                inter = F(w * h)
                with np.errstate(divide="ignore", invalid="ignore"):
                    iou = F(inter / F(F(area[ti] + area[tj]) - inter))
                if (iou >= thr) if suppress_at_equal else (iou > thr):
                    sup[tj] = True
    return _finish(K, topk, r_idx, c_idx, bsel, ssel, kept, kept_rank, nv)


def same(a, b):
    """two DetRef-like results (count, boxes, scores, classes, rows, ...) agree: rows, classes and box bits exactly, score bits exactly
    except that +0.0 and -0.0 are one value"""
    n = int(a[0])
    if n != int(b[0]):
        return False
    sa, sb = np.asarray(a[2][:n], F), np.asarray(b[2][:n], F)
    score_ok = np.array_equal(np.where(sa == 0, F(0), sa).view(np.uint32), np.where(sb == 0, F(0), sb).view(np.uint32))
    return bool(score_ok and np.array_equal(np.asarray(a[1][:n], F).reshape(n, 4).view(np.uint32), np.asarray(b[1][:n], F).reshape(n, 4).view(np.uint32))
                and np.array_equal(np.asarray(a[3][:n]), np.asarray(b[3][:n])) and np.array_equal(np.asarray(a[4][:n]), np.asarray(b[4][:n])))

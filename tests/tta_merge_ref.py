"""NumPy float32 restatement of sw_tta_merge (include/soswsod_hip.h): the merge of Stage-3 test-time augmentation, i.e.
GeneralizedRCNNWithTTA._get_augmented_boxes + _merge_detections + fast_rcnn_inference_single_image at score_thresh 1e-8.
A helper for tests/test_tta_merge_cpu.py (pinned there by tests/golden/tta_merge.npz, which the reference's own code wrote) and for
tests/test_gpu_stage3_tta.py; every step is a float32 operation in the kernel's order, one rounding each."""
import numpy as np

F = np.float32


def inverse_box(box, tab):
    """one row through un-flip (x -> W - x, x corners re-sorted by min / max), view -> loader ratios, loader -> dataset ratios; finite in"""
    x0, y0, x1, y1 = (F(v) for v in box)
    flip, W, rx, ry, px, py = (F(v) for v in tab)
    if flip != 0:
        a, b = F(W - x0), F(W - x1)
        x0, x1 = min(a, b), max(a, b)
    x0, x1 = F(F(x0 * rx) * px), F(F(x1 * rx) * px)
    y0, y1 = F(F(y0 * ry) * py), F(F(y1 * ry) * py)
    return x0, y0, x1, y1


def _iou(a, b):
    w = max(F(0), F(min(a[2], b[2]) - max(a[0], b[0])))
    h = max(F(0), F(min(a[3], b[3]) - max(a[1], b[1])))
    inter = F(w * h)
    area_a, area_b = F(F(a[2] - a[0]) * F(a[3] - a[1])), F(F(b[2] - b[0]) * F(b[3] - b[1]))
    return F(inter / F(F(area_a + area_b) - inter))                       # 0 / 0 = NaN: never above a threshold


def tta_merge_ref(boxes, scores, classes, counts, view_tab, img_h, img_w, nms_thresh, topk, num_classes):
    """boxes (V, T, 4), scores (V, T), classes (V, T), counts (V,), view_tab (V, 6) -> dict(count, boxes (topk, 4), scores, classes, src),
    rows beyond count zero; count = -1 (nothing else) when a count lies outside [0, T]"""
    boxes, scores, view_tab = np.asarray(boxes, F), np.asarray(scores, F), np.asarray(view_tab, F)
    classes, counts = np.asarray(classes, np.int32), np.asarray(counts, np.int32)
    V, T = scores.shape
    K = int(num_classes)
    out = dict(count=np.zeros(1, np.int32), boxes=np.zeros((topk, 4), F), scores=np.zeros(topk, F), classes=np.zeros(topk, np.int32),
               src=np.zeros(topk, np.int32))
    if ((counts < 0) | (counts > T)).any():
        out["count"][0] = -1
        return out
    imw, imh, thr = F(img_w), F(img_h), F(nms_thresh)
    cand = []                                                            # (class, score, union index, clipped box)
    with np.errstate(all="ignore"):
        for v in range(V):
            for s in range(int(counts[v])):
                sc, c = scores[v, s], int(classes[v, s])
                if not (np.isfinite(boxes[v, s]).all() and np.isfinite(sc)):
                    continue
                b = inverse_box(boxes[v, s], view_tab[v])
                if not np.isfinite(np.array(b)).all():
                    continue
                b = (min(max(b[0], F(0)), imw), min(max(b[1], F(0)), imh), min(max(b[2], F(0)), imw), min(max(b[3], F(0)), imh))
                if sc > F(1e-8) and 0 <= c < K:
                    cand.append((c, sc, v * T + s, b))
        if not cand:
            return out
        maxp1 = F(max(max(b) for _, _, _, b in cand) + F(1))
        kept = []
        for c in sorted({k[0] for k in cand}):
            off = F(F(c) * maxp1)
            seg = sorted((k for k in cand if k[0] == c), key=lambda k: (-float(k[1]), k[2]))
            ob = [tuple(F(x + off) for x in k[3]) for k in seg]
            alive = [True] * len(seg)
            for i in range(len(seg)):
                if not alive[i]:
                    continue
                kept.append(seg[i])
                for j in range(i + 1, len(seg)):
                    if alive[j] and _iou(ob[i], ob[j]) > thr:
                        alive[j] = False
    kept.sort(key=lambda k: (-float(k[1]), k[2]))
    kept = kept[:topk]
    out["count"][0] = len(kept)
    for t, (c, sc, i, b) in enumerate(kept):
        out["boxes"][t] = b; out["scores"][t] = sc; out["classes"][t] = c; out["src"][t] = i
    return out

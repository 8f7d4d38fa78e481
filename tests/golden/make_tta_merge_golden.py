"""Generate tests/golden/tta_merge.npz by RUNNING the reference's own Stage-3 TTA merge
(/root/reference/detectron2/detectron2/modeling/test_time_augmentation.py: GeneralizedRCNNWithTTA._merge_detections :242-259, which calls
fast_rcnn_inference_single_image, detectron2/detectron2/modeling/roi_heads/fast_rcnn.py:118-179) on hand-built per-view outputs, in the
build container only:

    python tests/golden/make_tta_merge_golden.py

ref_shim_d2.install() loads the reference's second tree file by file (its torchvision NMS is the greedy restatement stated there); the
TTA file's remaining imports are stubbed HERE: `fvcore.transforms` (HFlipTransform / NoOpTransform: names only) and
`detectron2.data.transforms` (RandomFlip, ResizeShortestEdge, ResizeTransform, apply_augmentations: names only) — the mapper and the
transform classes are not run.  fvcore is not installed, so the inverse transforms that `_get_augmented_boxes` applies
(`tfm.inverse().apply_box`: un-flip, un-resize, inverse of `pre_tfm`) come from the float32 restatement the project already carries for
them, `sos_wsod_amd.tta.ViewTransform.inverse_box` and `_scale_xyxy`; what the reference's code does from there on — the (N, K + 1)
score matrix, the finite filter, the clip, score > 1e-8, batched NMS, top-k — is the reference's.

The fixture holds, per case, the padded inputs of sw_tta_merge (boxes, scores, classes, counts, view table, sizes) and the reference's
outputs (boxes, scores, classes) with `src`, the union index v * T + slot of every output row, recovered from the row indices
fast_rcnn_inference_single_image returns.

Asserted here: apart from cases 5-6 no two candidates of a class have equal scores; no pair's IoU lies within 1e-6 of the threshold
(case 6 sits EXACTLY on it, on integer coordinates where every float32 step is exact), so the fixture does not depend on the rounding
differences between the shim's NMS and torchvision's; in case 5 the shim's order (stable sorts: ties by ascending index) equals the
stated rule — score descending, then union index ascending."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import ref_shim_d2  # noqa: E402
from tta_merge_ref import _iou  # noqa: E402

F = np.float32
VOC_SIZES = (480, 576, 672, 768, 864, 960, 1056, 1152)


def load_reference_tta():
    ns = ref_shim_d2.install()
    ft = ref_shim_d2._pkg("fvcore.transforms")
    ft.HFlipTransform = type("HFlipTransform", (), {}); ft.NoOpTransform = type("NoOpTransform", (), {})
    sys.modules["detectron2.data.detection_utils"].read_image = None
    dt = ref_shim_d2._pkg("detectron2.data.transforms")
    for n in ("RandomFlip", "ResizeShortestEdge", "ResizeTransform", "apply_augmentations"):
        setattr(dt, n, None)
    sys.modules["detectron2.modeling.meta_arch"].GeneralizedRCNN = ns.rcnn.GeneralizedRCNN
    mod = ref_shim_d2._load("detectron2.modeling.test_time_augmentation", ref_shim_d2.D2 + "/modeling/test_time_augmentation.py")
    return ns, mod


def run_case(mod, name, boxes, scores, classes, counts, views, loader_hw, orig_hw, nms, topk, K, out, exact_iou=False, ties=False):
    """views: [(view (h, w), flip)]; boxes (V, T, 4) in view coordinates"""
    from sos_wsod_amd.tta import ViewTransform, _scale_xyxy, view_table
    V, T = scores.shape
    boxes, scores = np.ascontiguousarray(boxes, F), np.ascontiguousarray(scores, F)
    classes, counts = np.ascontiguousarray(classes, np.int32), np.ascontiguousarray(counts, np.int32)
    tfms = [ViewTransform(loader_hw, hw, flip) for hw, flip in views]
    all_boxes, all_scores, all_classes, union = [], [], [], []
    for v, t in enumerate(tfms):
        n = int(counts[v])
        b = torch.from_numpy(boxes[v, :n].copy())
        fin = torch.isfinite(b).all(1)
        assert bool(((b[:, 0] <= b[:, 2]) & (b[:, 1] <= b[:, 3]))[fin].all())        # inverse_box swaps, fvcore re-sorts: the same for these
        back = t.inverse_box(b)
        if tuple(loader_hw) != tuple(orig_hw):
            back = _scale_xyxy(back, orig_hw[1] / loader_hw[1], orig_hw[0] / loader_hw[0])
        all_boxes.append(back)
        all_scores.extend(torch.from_numpy(scores[v, :n].copy()))
        all_classes.extend(torch.from_numpy(classes[v, :n].astype(np.int64)))
        union += [v * T + s for s in range(n)]
    all_boxes = torch.cat(all_boxes, 0)
    rec = {}
    orig_fn = mod.fast_rcnn_inference_single_image

    def recorder(b, s, *a):
        rec["valid"] = (torch.isfinite(b).all(1) & torch.isfinite(s).all(1)).numpy()
        res, rows = orig_fn(b, s, *a)
        rec["rows"] = rows.numpy()
        rec["all"] = orig_fn(b, s, a[0], a[1], a[2], -1)[0]
        return res, rows
    w = object.__new__(mod.GeneralizedRCNNWithTTA)
    w.__dict__["cfg"] = types.SimpleNamespace(MODEL=types.SimpleNamespace(ROI_HEADS=types.SimpleNamespace(NUM_CLASSES=K, NMS_THRESH_TEST=nms)),
                                              TEST=types.SimpleNamespace(DETECTIONS_PER_IMAGE=topk))
    mod.fast_rcnn_inference_single_image = recorder
    try:
        res = w._merge_detections(all_boxes, all_scores, all_classes, tuple(orig_hw))
    finally:
        mod.fast_rcnn_inference_single_image = orig_fn
    valid_rows = np.nonzero(rec["valid"])[0]
    src = np.array([union[valid_rows[r]] for r in rec["rows"]], np.int32)
    eb, es, ec = res.pred_boxes.tensor.numpy(), res.scores.numpy(), res.pred_classes.numpy().astype(np.int32)
    assert eb.dtype == F and es.dtype == F and len(es) <= topk
    # ---- the fixture's conditions
    cb = all_boxes.numpy().copy()
    cb[:, 0::2] = np.clip(cb[:, 0::2], 0, orig_hw[1]); cb[:, 1::2] = np.clip(cb[:, 1::2], 0, orig_hw[0])
    sc_all, cl_all = np.array([float(s) for s in all_scores], F), np.array([int(c) for c in all_classes])
    cand = rec["valid"] & (sc_all > F(1e-8))
    n_cand = int(cand.sum())
    if n_cand:
        maxp1 = F(cb[cand].max() + F(1))
        for c in np.unique(cl_all[cand]):
            idx = np.nonzero(cand & (cl_all == c))[0]
            if not ties:
                assert len(np.unique(sc_all[idx])) == len(idx), (name, c, "equal scores inside a class")
            ob = cb[idx] + F(F(c) * maxp1)
            with np.errstate(all="ignore"):
                for i in range(len(idx)):
                    for j in range(i + 1, len(idx)):
                        d = abs(float(_iou(ob[i], ob[j])) - nms)
                        assert d > 1e-6 or (exact_iou and d == 0.0) or np.isnan(d), (name, c, idx[i], idx[j], d)
    pre = f"{name}/"
    out.update({pre + "boxes": boxes, pre + "scores": scores, pre + "classes": classes, pre + "counts": counts,
                pre + "view_tab": view_table(tfms, loader_hw, orig_hw, "cpu").numpy(), pre + "hw": np.array(orig_hw, np.int32),
                pre + "nms": np.array(nms, np.float64), pre + "topk": np.array(topk, np.int32), pre + "K": np.array(K, np.int32),
                pre + "exp_boxes": eb, pre + "exp_scores": es, pre + "exp_classes": ec, pre + "exp_src": src})
    n_all = len(rec["all"])
    print(f"[{name}] V={V} T={T} K={K}: {n_cand} candidates, {n_all} survive the NMS, {len(es)} kept; src[:6]={src[:6].tolist()}")
    return dict(n_cand=n_cand, n_all=n_all, src=src, scores=es, classes=ec, boxes=eb)


def to_view(box_loader, hw, loader_hw, flip):
    """loader-image box -> view coordinates (float64 arithmetic, then float32: the inputs only have to be plausible detections)"""
    sx, sy = hw[1] / loader_hw[1], hw[0] / loader_hw[0]
    x0, y0, x1, y1 = box_loader[0] * sx, box_loader[1] * sy, box_loader[2] * sx, box_loader[3] * sy
    if flip:
        x0, x1 = hw[1] - x1, hw[1] - x0
    return [x0, y0, x1, y1]


def shortest_edge(h, w, size, max_size=4000):
    from sos_wsod_amd.tta import DeviceTTAMapper
    return DeviceTTAMapper._shortest_edge(h, w, size, max_size)


def main():
    ns, mod = load_reference_tta()
    out = {}
    # 1: identity
    r = run_case(mod, "c1", np.array([[[10, 20, 50, 60]]]), np.array([[0.9]]), np.array([[2]]), np.array([1]), [((100, 100), False)],
                 (100, 100), (100, 100), 0.5, 100, 3, out)
    assert r["src"].tolist() == [0] and r["boxes"].tolist() == [[10, 20, 50, 60]]
    # 2: a scale and its flip, the flipped duplicates fall
    lo, hw = (96, 128), (144, 192)
    objs = [[10, 12, 60, 70], [70, 20, 120, 90], [30, 60, 50, 80]]
    b = np.zeros((2, 3, 4)); s = np.zeros((2, 3))
    for i, o in enumerate(objs):
        b[0, i] = to_view(o, hw, lo, False); s[0, i] = 0.9 - 0.1 * i
        b[1, i] = to_view([o[0] + 1, o[1], o[2] + 1, o[3] + 0.5], hw, lo, True); s[1, i] = 0.85 - 0.1 * i
    r = run_case(mod, "c2", b, s, np.zeros((2, 3)), np.array([3, 3]), [(hw, False), (hw, True)], lo, lo, 0.5, 100, 1, out)
    assert r["src"].tolist() == [0, 1, 2]
    # 3: the VOC configuration
    rng = np.random.RandomState(7)
    orig, lo = (375, 500), (688, 917)
    views = [(shortest_edge(lo[0], lo[1], sz), f) for sz in VOC_SIZES for f in (False, True)]
    V, T, K = 16, 100, 20
    counts = rng.randint(70, 100, size=V); counts[3] = 0; counts[10] = 0; counts[6] = 100
    objects = [(rng.randint(0, K), x, y, x + rng.uniform(80, 300), y + rng.uniform(80, 300))
               for x, y in zip(rng.uniform(-40, 800, 18), rng.uniform(-40, 560, 18))]
    b = np.zeros((V, T, 4)); s = np.zeros((V, T)); c = np.zeros((V, T), np.int64)
    all_s = rng.permutation(np.linspace(0.02, 0.999, V * T))              # distinct in float32 (spacing 6e-4)
    for v, (hw, f) in enumerate(views):
        for t in range(counts[v]):
            if rng.rand() < 0.3:
                k, x0, y0, x1, y1 = objects[rng.randint(len(objects))]
                box = [x0 + rng.uniform(-6, 6), y0 + rng.uniform(-6, 6), x1 + rng.uniform(-6, 6), y1 + rng.uniform(-6, 6)]
            else:
                k = rng.randint(0, K)
                x0, y0 = rng.uniform(-30, lo[1] - 20), rng.uniform(-30, lo[0] - 20)
                box = [x0, y0, x0 + rng.uniform(30, 140), y0 + rng.uniform(30, 140)]
            b[v, t] = to_view(box, hw, lo, f); s[v, t] = all_s[v * T + t]; c[v, t] = k
    r = run_case(mod, "c3", b, s, c, counts, views, lo, orig, 0.5, 100, K, out)
    assert r["n_cand"] > 1024 and r["n_all"] > 100 and len(r["scores"]) == 100
    bb = out["c3/boxes"]
    assert (bb[..., 0] < 0).any() and (bb[..., 2] * out["c3/view_tab"][:, None, 2] > lo[1]).any()      # boxes leave the image before the clip
    # 4: K = 80, 70 classes empty
    lo = (120, 160)
    views = [((120, 160), False), ((120, 160), True), ((180, 240), False), ((180, 240), True)]
    used = [3, 7, 11, 19, 23, 42, 57, 64, 71, 79]
    V, T = 4, 20
    b = np.zeros((V, T, 4)); s = np.zeros((V, T)); c = np.zeros((V, T), np.int64)
    counts = np.array([20, 13, 17, 9])
    all_s = rng.permutation(np.linspace(0.05, 0.95, V * T))
    for v, (hw, f) in enumerate(views):
        for t in range(counts[v]):
            x0, y0 = rng.uniform(0, 110), rng.uniform(0, 80)
            b[v, t] = to_view([x0, y0, x0 + rng.uniform(15, 50), y0 + rng.uniform(15, 40)], hw, lo, f)
            s[v, t] = all_s[v * T + t]; c[v, t] = used[rng.randint(len(used))]
    r = run_case(mod, "c4", b, s, c, counts, views, lo, lo, 0.5, 100, 80, out)
    assert set(r["classes"].tolist()) <= set(used)
    # 5: exact ties
    hw = (300, 300)
    b = np.zeros((2, 4, 4)); s = np.zeros((2, 4)); c = np.zeros((2, 4), np.int64)
    b[0, 0] = [10, 10, 50, 50]; s[0, 0] = 0.8
    b[0, 1] = [100, 100, 150, 150]; s[0, 1] = 0.6
    b[1, 0] = [10, 10, 50, 50]; s[1, 0] = 0.8                               # identical box, equal score: union index 0 survives
    b[1, 1] = [200, 200, 250, 250]; s[1, 1] = 0.6                           # disjoint, equal score: union index order
    r = run_case(mod, "c5", b, s, c, np.array([2, 2]), [(hw, False), (hw, False)], hw, hw, 0.5, 100, 2, out, ties=True)
    assert r["src"].tolist() == [0, 1, 5], r["src"]                         # the shim's order is the stated rule
    # 6: IoU exactly at the threshold, integer coordinates
    hw = (64, 64)
    rows = [([0, 0, 10, 10], 0.95, 0), ([0, 0, 10, 5], 0.90, 0),           # 50 / 100: not above 0.5, both kept
            ([20, 20, 30, 30], 0.85, 0), ([20, 20, 30, 26], 0.80, 0),       # 60 / 100: the later one falls
            ([0, 0, 10, 10], 0.75, 2), ([0, 0, 10, 5], 0.70, 2),           # the same in a class with a non-zero offset
            ([20, 20, 30, 30], 0.65, 2), ([20, 20, 30, 26], 0.60, 2), ([30, 30, 40, 40], 0.55, 1)]
    b = np.zeros((1, 9, 4)); s = np.zeros((1, 9)); c = np.zeros((1, 9), np.int64)
    for i, (bx, sc, k) in enumerate(rows):
        b[0, i] = bx; s[0, i] = sc; c[0, i] = k
    r = run_case(mod, "c6", b, s, c, np.array([9]), [(hw, False)], hw, hw, 0.5, 100, 3, out, exact_iou=True)
    assert r["src"].tolist() == [0, 1, 2, 4, 5, 6, 8]
    # 7: scores around float32(1e-8)
    e = F(1e-8)
    b = np.zeros((1, 3, 4)); c = np.zeros((1, 3), np.int64)
    b[0, 0] = [0, 0, 10, 10]; b[0, 1] = [20, 20, 30, 30]; b[0, 2] = [40, 40, 50, 50]
    s = np.array([[e, np.nextafter(e, F(1)), np.nextafter(e, F(0))]], F)
    r = run_case(mod, "c7", b, s, c, np.array([3]), [(hw, False)], hw, hw, 0.5, 100, 1, out)
    assert r["src"].tolist() == [1]
    # 8: NaN coordinate, infinite score, two boxes of one class that are empty after the clip (both kept: 0 / 0 suppresses nothing)
    b = np.zeros((1, 5, 4)); s = np.zeros((1, 5)); c = np.zeros((1, 5), np.int64)
    b[0, 0] = [5, np.nan, 20, 20]; s[0, 0] = 0.9
    b[0, 1] = [5, 5, 20, 20]; s[0, 1] = np.inf
    b[0, 2] = [74, 10, 84, 50]; s[0, 2] = 0.7; c[0, 2] = 1
    b[0, 3] = [94, 20, 114, 60]; s[0, 3] = 0.6; c[0, 3] = 1
    b[0, 4] = [5, 5, 20, 20]; s[0, 4] = 0.5
    r = run_case(mod, "c8", b, s, c, np.array([5]), [(hw, False)], hw, hw, 0.5, 100, 2, out)
    assert r["src"].tolist() == [2, 3, 4] and r["boxes"][0].tolist() == [64, 10, 64, 50]
    np.savez_compressed(os.path.join(HERE, "tta_merge.npz"), **out)
    print("wrote tta_merge.npz,", os.path.getsize(os.path.join(HERE, "tta_merge.npz")), "bytes")


if __name__ == "__main__":
    main()

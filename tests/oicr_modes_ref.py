"""NumPy restatements of OICRPlusHeads' other mining rules (top-1 seeds, box update), the case tables and the decode bar.

Built on oracle.oicr_oracle by import (topk_desc, nms_keep, pairwise_iou, matcher, apply_deltas, get_deltas); everything that
decides a label is float32 arithmetic in the reference's order, the decode and the loss are float64.
Reference: uwsod/projects/WSL/wsl/modeling/roi_heads/roi_heads_oicrplus.py:302-425 (the rounds), :607-757 (get_pgt_top_k),
:560-605 (get_pgt_mist), roi_heads.py:266-375 (labels), detectron2 box_regression.py:38-110.
"""
import math
import os

import numpy as np
import torch

from oracle import oicr_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCALE_CLAMP = math.log(1000.0 / 16)
WEIGHTS = O.BBOX_REG_WEIGHTS
DX_SIGN = (1, -1, 1, -1)                      # views [1, 1_flip, 2, 2_flip]: a flipped view enters dx with a minus sign (:407)
EPS32 = 2.0 ** -24                            # one float32 rounding, relative

# end-to-end cases: name -> (shape case of make_golden.E2E_CASES, refine_mist, bbox_update)
CASES = {"top1": ("s0", False, False), "upd": ("s0m", True, True), "both": ("s0m", False, True)}
# H, W, R, n_gt, dan, head_scale.  s0m = the s0 shape with milder heads: at head_scale 30 the MIL logits reach |x| ~ 50 and carry
# |x| * 1e-6 of relative float32 noise into the scores, the round-0 weights and the WSDDN gradient (the draws of `upd` / `both` at 30
# came out 2e-4 .. 4e-4 apart between hosts in exactly those, against bars of 1e-4 / 2e-4); at 10 that noise is a third
SHAPES = {"s0": (96, 128, 37, 2, (256, 256), 30.0), "s1": (128, 160, 64, 3, (256, 256), 60.0), "s0m": (96, 128, 37, 2, (256, 256), 10.0)}
IOU_MARGIN = 2e-3                             # what the generator demands of every IoU a label hangs on (see iou_sensitivity)
SCORE_MARGIN = 1e-5                           # relative gap of every score comparison that selects or orders a seed


def load_case(name):
    return np.load(os.path.join(GOLDEN, f"oicr_modes_{name}.npz"))


def case_inputs(meta):
    """closed-form parameters, views, labels and dropout masks of a fixture (regenerated from its recipe, not stored)"""
    H, W, R, n_gt, K = (int(meta[k]) for k in ("H", "W", "R", "n_gt", "K"))
    dan = tuple(int(x) for x in meta["dan"])
    tag = str(meta["tag"])
    P = O.make_params(K, dan, tag="p" + tag, head_scale=float(meta["head_scale"]))
    for k in range(4):                        # larger box deltas than the init statistics give: the update must move labels
        for n in ("weight", "bias"):
            P[f"roi_heads.box_refinery_{k}.bbox_pred.{n}"] = P[f"roi_heads.box_refinery_{k}.bbox_pred.{n}"] * np.float32(meta["box_scale"])
    views, gt = O.make_views(H, W, R, n_gt=n_gt, K=K, tag="v" + tag)
    masks = O.make_masks(R, dan, tag="m" + tag)
    return P, views, gt, masks


# --------------------------------------------------------------------------- decode (float64) and its bar
def mean_deltas(deltas, signs=DX_SIGN, dtype=np.float64):
    """deltas [V][R][C][4] -> [R][C][4]: (d_0 -+ d_1 + ...) / V, left to right, the sign on dx only (:406-410)"""
    d = np.asarray(deltas, dtype)
    acc = d[0].copy()
    acc[..., 0] *= signs[0]
    for v in range(1, d.shape[0]):
        t = d[v].copy()
        t[..., 0] *= signs[v]
        acc = (acc + t).astype(dtype)
    return (acc / dtype(d.shape[0])).astype(dtype)


def decode(deltas, boxes, signs=DX_SIGN, dtype=np.float64, weights=WEIGHTS, clamp=SCALE_CLAMP):
    """[V][R][C][4] deltas, [R][4] view-0 proposals -> [R][C][4] boxes (apply_deltas, box_regression.py:73-110), not clipped"""
    d = mean_deltas(deltas, signs, dtype)
    b = np.asarray(boxes, dtype)
    w = (b[:, 2] - b[:, 0])[:, None]; h = (b[:, 3] - b[:, 1])[:, None]
    cx = b[:, 0:1] + dtype(0.5) * w; cy = b[:, 1:2] + dtype(0.5) * h
    dx = d[..., 0] / dtype(weights[0]); dy = d[..., 1] / dtype(weights[1])
    dw = np.minimum(d[..., 2] / dtype(weights[2]), dtype(clamp)); dh = np.minimum(d[..., 3] / dtype(weights[3]), dtype(clamp))
    px = dx * w + cx; py = dy * h + cy
    pw = np.exp(dw) * w; ph = np.exp(dh) * h
    return np.stack([px - dtype(0.5) * pw, py - dtype(0.5) * ph, px + dtype(0.5) * pw, py + dtype(0.5) * ph], -1).astype(dtype)


def decode_bar(deltas, boxes, weights=WEIGHTS, clamp=SCALE_CLAMP):
    """absolute float32 error bar of every decoded coordinate, [R][C][4], from the operation count.
    A delta is a sign-mixed sum of V terms (V - 1 additions), one division by V and one by the weight: 5 roundings for V = 4,
    each at most EPS32 of S = sum_v |d_v| / V / weight (the terms may cancel, so the sum of magnitudes bounds it, not the result).
      centre  px = dx * w + cx: 5 roundings of dx, 1 of w, 1 of the product (<= 7 EPS32 S w); cx = x1 + 0.5 w is 2 roundings
              (<= 2 EPS32 (|cx| + w)); the addition 1 more of |px| <= S w + |cx|                       -> 8 (S w + |cx|) + 2 w
      size    pw = exp(dw) * w: the 5 roundings of dw shift it by <= 5 EPS32 S and exp turns a shift into a relative error; expf is
              good to 2 ulp; w and the product are 1 each                                                   -> (5 S + 4) e^dw w
      corner  px -+ 0.5 pw: half the size error (0.5 * pw is exact) and 1 rounding of |px| + 0.5 pw
    doubled for the second-order terms.  Scale: |ctr| + e^dw w, as the terms show."""
    d = np.abs(np.asarray(deltas, np.float64))
    V = d.shape[0]
    b = np.asarray(boxes, np.float64)
    w = (b[:, 2] - b[:, 0])[:, None]; h = (b[:, 3] - b[:, 1])[:, None]
    cx = np.abs(b[:, 0:1] + 0.5 * w); cy = np.abs(b[:, 1:2] + 0.5 * h)
    S = d.sum(0) / V
    mean = mean_deltas(deltas)
    out = []
    for q, side, ctr in ((0, w, cx), (1, h, cy)):
        Sc, Ss = S[..., q] / weights[q], S[..., 2 + q] / weights[2 + q]
        e = np.exp(np.minimum(mean[..., 2 + q] / weights[2 + q], clamp)) * side
        centre = 8 * (Sc * side + ctr) + 2 * side
        size = (5 * Ss + 4) * e
        out.append(2 * EPS32 * (centre + 0.5 * size + (Sc * side + ctr + 0.5 * e)))
    return np.stack([out[0], out[1], out[0], out[1]], -1)


def iou_sensitivity(min_side, n_boxes=2):
    """|d IoU / d coordinate| of boxes whose sides are >= min_side: moving one coordinate by t moves the intersection by <= t h and
    the union by <= 2 t h, with U >= w h and I <= U: |dIoU| <= t / w + 2 t / w = 3 t / min_side; 4 coordinates per perturbed box"""
    return 12.0 * n_boxes / min_side


# --------------------------------------------------------------------------- mining on class-specific boxes (float32 decisions)
def cand_of(boxes, cand, G):
    """candidate boxes [R][G][4]: the class-specific ones, or the proposal boxes for every class"""
    boxes = np.asarray(boxes, np.float32)
    return np.broadcast_to(boxes[:, None, :], (boxes.shape[0], G, 4)) if cand is None else np.asarray(cand, np.float32)


def mine(scores, boxes, gt_int, cand=None, seed_rule=0, top_p=0.10, thres=0.05, nms_thr=0.01):
    """the pseudo-GT list of one round: seed_rule 0 = get_pgt_mist (top-p%, threshold with rank 0 kept, class-agnostic NMS,
    score-descending list), 1 = get_pgt_top_k with top_k = 1 (G entries in class order).  The box of slot (rank, g) is
    cand[row][g] (index_select + gather, :650-653, :675-678)."""
    scores = np.asarray(scores, np.float32)
    gt_int = np.asarray(gt_int, np.int64)
    R, G = scores.shape[0], gt_int.shape[0]
    cb = cand_of(boxes, cand, G)
    sel = scores[:, gt_int]
    k = max(int(R * top_p), 1) if seed_rule == 0 else min(R, 1)
    idx = np.stack([O.topk_desc(sel[:, g], k) for g in range(G)], axis=1)              # (k, G)
    val = np.take_along_axis(sel, idx, axis=0)
    mask = np.ones_like(val, bool)
    if seed_rule == 0:
        mask = val >= np.float32(thres)
        mask[0:1, :] = True
    gnum = np.broadcast_to(np.arange(G)[None, :], (k, G))
    s, i, g = val[mask].astype(np.float32), idx[mask].astype(np.int64), gnum[mask]
    b = cb[i, g].astype(np.float32)
    keep = np.arange(len(s)) if seed_rule == 1 else O.nms_keep(b, s, nms_thr)
    return dict(scores=s[keep], boxes=b[keep], classes=gt_int[g][keep], weights=s[keep], index=i[keep],
                pre_nms=dict(scores=s, boxes=b, classes=gt_int[g], index=i), keep=keep)


def label(pgt, boxes, K):
    """label_and_sample_proposals on pseudo boxes that need not be proposal boxes: O.label_proposals is already that"""
    return O.label_proposals(pgt, np.asarray(boxes, np.float32), K)


def mine_and_label(scores, boxes, gt_int, K, cand=None, seed_rule=0):
    p = mine(scores, boxes, gt_int, cand, seed_rule)
    l = label(p, boxes, K)
    return p, l


# --------------------------------------------------------------------------- refine loss with view-0 targets (float64)
def refine_loss(logits, deltas, boxes_v, lab_class, lab_weight, lab_index, K, tgt_box0=None, pred_view=(0, 1, 2, 2)):
    """per-view (loss_cls, loss_box) in float64: logits [V][R][K+1], deltas [V][R][4K], boxes_v [V][R][4]; view v's targets are paired
    with the predictions of view pred_view[v]; its target box is boxes_v[v][lab_index], view 0's is tgt_box0 when given"""
    out = []
    for v in range(len(boxes_v)):
        gtb = np.asarray(boxes_v[v], np.float64)[lab_index]
        if v == 0 and tgt_box0 is not None:
            gtb = np.asarray(tgt_box0, np.float64)
        lc, lb = O.oicr_losses(torch.from_numpy(np.asarray(logits[pred_view[v]], np.float64)),
                               torch.from_numpy(np.asarray(deltas[pred_view[v]], np.float64)),
                               np.asarray(boxes_v[v], np.float64), gtb, lab_class, lab_weight, K)
        out.append((float(lc), float(lb)))
    return out


# --------------------------------------------------------------------------- synthetic edge cases of the mining
EDGE_CASES = ("same_seed2", "same_seed3", "g1", "r1", "r9", "nms_sides", "iou_exact", "nan_inf")


def edge_case(name):
    """-> dict(scores (R, K+1) f32, boxes (R, 4) f32, gt (G,) int64, cand (R, G, 4) f32 or None, seed_rule, K)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    K, R = 20, 24
    gx, gy = np.meshgrid(np.arange(6), np.arange(4))
    boxes = np.stack([gx.ravel() * 40.0, gy.ravel() * 40.0, gx.ravel() * 40.0 + 30.0, gy.ravel() * 40.0 + 30.0], 1).astype(np.float32)
    scores = (rng.permutation(R * (K + 1)).reshape(R, K + 1).astype(np.float32) + 1) / np.float32(4 * R * (K + 1))   # distinct, < 0.25
    gt, cand, seed_rule = np.array([3, 11], np.int64), None, 0
    if name.startswith("same_seed"):                       # top-1: every class seeds proposal 5; 4, 6 overlap it at IoU >= 0.6
        gt = np.array([2, 7, 15][:int(name[-1])], np.int64)
        scores[5, gt] = 0.9
        boxes[4] = boxes[5] + np.float32([2, 0, 2, 0]); boxes[6] = boxes[5] + np.float32([0, 3, 0, 3])
        seed_rule = 1
    elif name == "g1":
        gt = np.array([19], np.int64)
        cand = (boxes[:, None, :] + rng.uniform(-3, 3, (R, 1, 4))).astype(np.float32)
    elif name == "r1":
        R = 1; boxes, scores = boxes[:1], scores[:1]
        cand = (boxes[:, None, :] + np.float32([[1, -1, 2, 3], [0, 2, -2, 1]])[None]).astype(np.float32)
    elif name == "r9":                                     # top_k = max(int(0.9), 1) = 1
        R = 9; boxes, scores = boxes[:9], scores[:9]
        cand = (boxes[:, None, :] + rng.uniform(-3, 3, (R, 2, 4))).astype(np.float32)
        seed_rule = 1
    elif name == "nms_sides":                              # both classes' best proposal is 5; its refined boxes are disjoint
        scores[:, gt] *= np.float32(0.1)                   # everything else below the threshold
        scores[5, 3], scores[5, 11] = 0.9, 0.8
        scores[6, 3], scores[6, 11] = 0.02, 0.01           # rank 1 (top_k = 2): under the threshold
        cand = np.repeat(boxes[:, None, :], 2, 1).copy()
        cand[5, 0] = [200, 40, 230, 70]; cand[5, 1] = [235, 40, 265, 70]          # IoU 0 < 0.01, the proposal box itself gives 1
    elif name == "iou_exact":                              # seeds 0 and 23 (disjoint); proposals at IoU exactly 0.5 / 0.6 with seed 0
        scores[:, gt] *= np.float32(0.1)
        scores[0, 3], scores[23, 11] = 0.9, 0.8
        boxes[0] = [0, 0, 40, 30]
        boxes[1] = [0, 0, 20, 30]                          # inside: 600 / 1200 = 0.5
        boxes[2] = [0, 0, 24, 30]                          # 720 / 1200 = 0.6
        boxes[3] = [0, 0, 80, 30]                          # contains: 1200 / 2400 = 0.5
    elif name == "nan_inf":                                # refined boxes with a NaN / an infinite coordinate head the list
        seed_rule = 1
        scores[5, 3], scores[9, 11] = 0.9, 0.8
        cand = np.repeat(boxes[:, None, :], 2, 1).copy()
        cand[5, 0, 0] = np.nan
        cand[9, 1, 2] = np.inf
    return dict(scores=scores, boxes=boxes, gt=gt, cand=cand, seed_rule=seed_rule, K=K)


def decode_inputs(V, R, K, G, seed):
    """-> logits (V*R, ld) f32 with NaN guard columns around one head's 4K box columns, box_col, boxes (R, 4), gt (G,), signs (V,):
    dw / dh on both sides of the clamp, and dx terms that cancel exactly to +-0"""
    rng = np.random.default_rng(seed)
    box_col, ld = 5, 4 * K + 11
    lg = np.full((V * R, ld), np.nan, np.float32)
    d = rng.normal(0.0, 4.0, (V, R, K, 4)).astype(np.float32)
    d[..., 2:] *= np.float32(4.0)                          # dw = d / 5: well beyond log(1000 / 16) = 4.1 in a good share of the rows
    signs = np.array([1, -1, 1, -1][:V] if V == 4 else [1] * V, np.int32)
    if V == 4:
        d[1, ::3, :, 0] = d[0, ::3, :, 0]; d[2, ::3, :, 0] = 0; d[3, ::3, :, 0] = 0          # d0 - d0 + 0 - 0 = +0
        d[0, 1::3, :, 1] = -d[1, 1::3, :, 1]; d[2, 1::3, :, 1] = -0.0; d[3, 1::3, :, 1] = 0   # -a + a + -0 + 0
    lg[:, box_col:box_col + 4 * K] = d.reshape(V * R, 4 * K)
    xy = rng.uniform(0.0, 400.0, (R, 2)); wh = rng.uniform(4.0, 200.0, (R, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    gt = np.sort(rng.choice(K, G, replace=False)).astype(np.int64)
    return lg, box_col, boxes, gt, signs, d

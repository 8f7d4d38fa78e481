"""float64 restatements of the Stage-3 loss kernels (checkers, not product code), the inputs of their edge tests, and the tolerance
table those tests read: sw_rpn_loss (csrc/detector.hip), sw_focal_loss (csrc/heads.hip), sw_det_loss_per_image (csrc/detector.hip),
sw_wsddn_scores_bwd (csrc/proposals.hip) and the case table of sw_threshold_select (csrc/elementwise.hip; its reference is
oracle.semisup_oracle.threshold_bbox).

Every reference takes the float32 inputs the kernel gets, upcast to float64, so input rounding is common to both sides.  The formulas
are the ones the kernels' comments cite; tests/test_losses_ref_cpu.py pins each restatement to float64 autograd of the reference's
own expression and to the oracles.

Tolerances: the rule of tests/heads_ref.py.  The plain float32 torch evaluation of the same formula (the *_f32 functions) runs on the
same inputs, e32 = max|f32 - f64| / max|f64| per (kernel, output kind, value regime), and a float output may differ from the float64
reference by max(BAR_FLOOR, BAR_FACTOR * e32) of max|ref|.  E32 below is that table; test_losses_ref_cpu.py recomputes it and asserts
it is current.  Two kernels keep the bar their first test gave them: sw_det_loss_per_image (rtol 2e-5, atol 1e-6 per element) and
sw_wsddn_scores_bwd (double arithmetic rounded once: 2e-7 max|ref| + 1e-12); their e32 rows are kept for the record only.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from heads_ref import BAR_FACTOR, BAR_FLOOR, REG_WEIGHTS, rel_err  # noqa: F401  (rel_err: re-exported to the tests)

UNIT_WEIGHTS = (1.0, 1.0, 1.0, 1.0)
WEIGHTS = {"w1": UNIT_WEIGHTS, "wreg": REG_WEIGHTS}
SCORES_BWD_REL, SCORES_BWD_ABS = 2e-7, 1e-12
DETLOSS_RTOL, DETLOSS_ATOL = 2e-5, 1e-6


def bar(kind, regime):
    """allowed max|got - ref| / max|ref| of output `kind` in value regime `regime`"""
    return max(BAR_FLOOR, BAR_FACTOR * E32[(kind, regime)])


def _deltas64(src, tgt, w):
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tx, ty = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    return np.stack([w[0] * (tx - sx) / sw, w[1] * (ty - sy) / sh, w[2] * np.log(tw / sw), w[3] * np.log(th / sh)], 1)


def _deltas_t(src, tgt, w):
    """get_deltas (box_regression.py:38-71) on torch tensors of either precision"""
    sw = src[:, 2] - src[:, 0]; sh = src[:, 3] - src[:, 1]
    sx = src[:, 0] + 0.5 * sw; sy = src[:, 1] + 0.5 * sh
    tw = tgt[:, 2] - tgt[:, 0]; th = tgt[:, 3] - tgt[:, 1]
    tx = tgt[:, 0] + 0.5 * tw; ty = tgt[:, 1] + 0.5 * th
    return torch.stack((w[0] * (tx - sx) / sw, w[1] * (ty - sy) / sh, w[2] * torch.log(tw / sw), w[3] * torch.log(th / sh)), 1)


# ============================================================================================ sw_rpn_loss
def rpn_loss_ref(logits, deltas, labels, anchors, matched, weights, inv_norm):
    """logits (n,), deltas (n, 4), labels (n,) in {-1, 0, 1}, anchors (A, 4) repeating over the images (row i uses anchor i % A),
    matched (n, 4).  -> dict: loss_cls = sum over label >= 0 of BCE-with-logits * inv_norm, loss_loc = sum over label == 1 of
    |delta - get_deltas(anchor, matched)|_1 * inv_norm, dlogits (n,) = (sigmoid(x) - y) * inv_norm, ddeltas (n, 4) = sign(e) * inv_norm
    (both 0 where the anchor takes no part), err (n_fg, 4) = the residuals e, fg = their anchor rows"""
    x = np.asarray(logits, np.float64).reshape(-1); d = np.asarray(deltas, np.float64).reshape(-1, 4)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    an = np.asarray(anchors, np.float64).reshape(-1, 4); ma = np.asarray(matched, np.float64).reshape(-1, 4)
    n, A = x.shape[0], an.shape[0]
    s = float(inv_norm)
    valid, fg = lab >= 0, np.nonzero(lab == 1)[0]
    y = (lab == 1).astype(np.float64)
    bce = np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))
    sig = 1.0 / (1.0 + np.exp(-x))
    e = d[fg] - _deltas64(an[fg % A], ma[fg], weights)
    dd = np.zeros((n, 4)); dd[fg] = np.sign(e) * s
    return dict(loss_cls=bce[valid].sum() * s, loss_loc=np.abs(e).sum() * s, dlogits=np.where(valid, (sig - y) * s, 0.0), ddeltas=dd,
                err=e, fg=fg)


def rpn_loss_f32(logits, deltas, labels, anchors, matched, weights, inv_norm):
    """the same in float32 torch: F.binary_cross_entropy_with_logits + L1 on get_deltas, gradients by autograd"""
    x = torch.from_numpy(np.ascontiguousarray(logits, np.float32).reshape(-1)).requires_grad_(True)
    d = torch.from_numpy(np.ascontiguousarray(deltas, np.float32).reshape(-1, 4)).requires_grad_(True)
    lab = torch.from_numpy(np.asarray(labels).reshape(-1).astype(np.int64))
    an = torch.from_numpy(np.ascontiguousarray(anchors, np.float32)); ma = torch.from_numpy(np.ascontiguousarray(matched, np.float32))
    s = float(np.float32(inv_norm))
    valid = lab >= 0; fg = torch.nonzero(lab == 1)[:, 0]
    cls = F.binary_cross_entropy_with_logits(x[valid], (lab[valid] == 1).float(), reduction="sum") * s
    loc = (d[fg] - _deltas_t(an[fg % an.shape[0]], ma[fg], weights)).abs().sum() * s
    (cls + loc).backward()
    return dict(loss_cls=cls.detach().numpy(), loss_loc=loc.detach().numpy(), dlogits=x.grad.numpy(), ddeltas=d.grad.numpy())


def _rc(N, A, labels, w):
    return dict(N=N, A=A, labels=labels, w=w, id=f"{N}x{A}-{labels}-{w}")


# n = N * A around the 256-thread workgroup, the 256 x 256 launch cap (65,536: the last size with one grid-stride pass) and beyond it,
# where A = 21,900 does not divide the 65,536 stride and the anchor index wraps inside the second pass.
# labels: mixed = -1 / 0 / 1; ignore = all -1; nofg = -1 / 0; allfg = all 1
RPN_CASES = [
    _rc(1, 1, "allfg", "w1"), _rc(1, 1, "ignore", "wreg"), _rc(1, 255, "mixed", "w1"), _rc(1, 256, "mixed", "wreg"),
    _rc(1, 257, "mixed", "w1"), _rc(1, 257, "nofg", "wreg"), _rc(2, 417, "mixed", "wreg"), _rc(2, 417, "ignore", "w1"),
    _rc(2, 417, "nofg", "w1"), _rc(2, 417, "allfg", "wreg"), _rc(1, 65536, "mixed", "w1"), _rc(1, 65537, "mixed", "wreg"),
    _rc(3, 21900, "mixed", "wreg"), _rc(3, 21900, "mixed", "w1"), _rc(3, 21900, "allfg", "w1"), _rc(3, 21900, "ignore", "wreg"),
    _rc(3, 21900, "nofg", "wreg"),
]
RPN_PLANTED = np.array([0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0], np.float32)
RPN_ZERO_BOX = np.array([[16.0, 32.0, 64.0, 128.0], [8.0, 8.0, 512.0, 256.0], [1.0, 2.0, 4.0, 8.0]], np.float32)


def rpn_inputs(c):
    """-> dict(logits (n,) f32 N(0, 3^2) with RPN_PLANTED at random places, deltas (n, 4) f32, labels (n,) i8, anchors (A, 4) f32, matched
    (n, 4) f32, weights, inv_norm f32, zero = the anchor rows of the exact-zero group: foreground anchors with power-of-two corner
    coordinates, matched == anchor and delta == 0, so target and residual are exactly 0 in float32 and in float64).
    Every other foreground delta is float32(target64) + r with 0.01 <= |r| <= 1: away from the kink of the L1 loss."""
    N, A, mode = c["N"], c["A"], c["labels"]
    n = N * A
    rng = np.random.default_rng(11000 + 31 * N + 7 * A + sum(map(ord, mode + c["w"])))
    xy = rng.uniform(0.0, 600.0, (A, 2)); wh = 8.0 + rng.uniform(0.0, 200.0, (A, 2))
    anchors = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    rep = np.tile(anchors, (N, 1)).astype(np.float64)
    mxy = rep[:, :2] + rng.normal(0.0, 10.0, (n, 2)); mwh = 8.0 + rng.uniform(0.0, 200.0, (n, 2))
    matched = np.concatenate([mxy, mxy + mwh], 1).astype(np.float32)
    logits = rng.normal(0.0, 3.0, n).astype(np.float32)
    if mode == "mixed":
        labels = rng.integers(-1, 2, n).astype(np.int8)
    elif mode == "nofg":
        labels = rng.integers(-1, 1, n).astype(np.int8)
    else:
        labels = np.full(n, -1 if mode == "ignore" else 1, np.int8)
    if n >= 64:
        at = rng.choice(n, 2 * len(RPN_PLANTED), replace=False)
        logits[at] = np.tile(RPN_PLANTED, 2)
        if mode == "mixed":
            labels[at] = np.repeat([0, 1], len(RPN_PLANTED))            # every planted value once as a negative, once as a positive
        elif mode == "nofg":
            labels[at] = 0
    zero = np.zeros(0, np.int64)
    if mode in ("mixed", "allfg") and A >= 255:
        # one anchor slot per zero box; the group sits in the LAST image (beyond the 65,536 stride where n allows it)
        slots = rng.choice(A, len(RPN_ZERO_BOX), replace=False)
        anchors[slots] = RPN_ZERO_BOX
        zero = (N - 1) * A + slots
        labels[zero] = 1
        # images that share the slot see an ordinary pair: their matched boxes follow the new anchor
        for k, s in enumerate(slots):
            for img in range(N):
                i = img * A + s
                o = rng.normal(0.0, 3.0, 2)
                matched[i] = np.concatenate([RPN_ZERO_BOX[k][:2] + o, RPN_ZERO_BOX[k][:2] + o + 4.0 + rng.uniform(0.0, 50.0, 2)])
        matched[zero] = RPN_ZERO_BOX
    weights = WEIGHTS[c["w"]]
    deltas = rng.normal(0.0, 0.5, (n, 4)).astype(np.float32)
    fg = np.nonzero(labels == 1)[0]
    if len(fg):
        tgt = _deltas64(anchors.astype(np.float64)[fg % A], matched.astype(np.float64)[fg], weights).astype(np.float32)
        r = rng.uniform(0.01, 1.0, tgt.shape) * rng.choice([-1.0, 1.0], tgt.shape)
        deltas[fg] = (tgt.astype(np.float64) + r).astype(np.float32)
    deltas[zero] = 0.0
    return dict(logits=logits, deltas=deltas, labels=labels, anchors=anchors, matched=matched, weights=weights,
                inv_norm=np.float32(1.0 / (256 * N)), zero=zero)


# ============================================================================================ sw_focal_loss
def focal_ref(logits, targets, gamma):
    """CE_r = logsumexp(x_r) - x_r[t_r], p_r = exp(-CE_r), loss = sum_r (1 - p_r)^gamma CE_r / N;
    dloss/dx_j = ((1 - p)^gamma + gamma (1 - p)^(gamma - 1) p CE) (softmax_j - [j == t]) / N.  -> loss, dlogits (N, C)"""
    x = np.asarray(logits, np.float64); t = np.asarray(targets).astype(np.int64)
    N = x.shape[0]
    rows = np.arange(N)
    z = x - x.max(1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(1, keepdims=True))
    ce = -logp[rows, t]
    p = np.exp(-ce)
    om = np.maximum(1.0 - p, 0.0)
    w = om ** gamma                                            # (0 ** 0 = 1: gamma 0 is the plain cross-entropy)
    with np.errstate(divide="ignore", invalid="ignore"):
        dw = np.where((om > 0) & (gamma > 0), gamma * om ** (gamma - 1.0) * p * ce, 0.0)
    oh = np.zeros_like(x); oh[rows, t] = 1.0
    return (w * ce).sum() / N, (w + dw)[:, None] * (np.exp(logp) - oh) / N


def focal_f32(logits, targets, gamma):
    """float32 torch: F.cross_entropy(reduction="none"), p = exp(-CE), sum((1 - p)^gamma CE) / N, gradient by autograd"""
    x = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(targets).astype(np.int64))
    ce = F.cross_entropy(x, t, reduction="none")
    loss = ((1.0 - torch.exp(-ce)).clamp_min(0.0) ** gamma * ce).sum() / x.shape[0]
    loss.backward()
    return loss.detach().numpy(), x.grad.numpy()


def _fc(N, C, gamma, regime):
    return dict(N=N, C=C, gamma=gamma, regime=regime, id=f"N{N}-C{C}-g{gamma:g}-{regime}")


# N around the 4 rows of a workgroup and the 1024 threads of the reduction, C around the 64 lanes of a wave.
# regimes: sd3 / sd40 = N(0, 3^2) / N(0, 40^2); shift = sd3 plus 3e4 on every logit (the loss is invariant; a logsumexp formed at 3e4
# keeps 2e-3 of absolute precision); sep = sd3 with the target logit 40 above (even rows) or below (odd rows) the rest (p = 1 - 1e-17
# and p = 1e-17: the clamp of 1 - p, the loss of a confidently wrong row)
FOCAL_SHAPES = [(1, 2), (3, 1), (4, 63), (5, 64), (7, 65), (1023, 21), (1024, 81), (1025, 81), (4097, 21), (37, 129), (9, 1231)]
FOCAL_CASES = (
    [_fc(N, C, 1.5, reg) for (N, C), reg in zip(FOCAL_SHAPES, ["sd3", "sd3", "sd40", "shift", "sep", "sd3", "sd40", "shift", "sep", "sd3",
                                                             "sd40"])]
    + [_fc(1, 2, 0.0, "sep"), _fc(3, 1, 0.0, "sd40"), _fc(7, 65, 0.0, "sd3"), _fc(1025, 81, 0.0, "sd40"), _fc(9, 1231, 0.0, "shift"),
       _fc(1, 2, 1.0, "sd40"), _fc(5, 64, 1.0, "sep"), _fc(1024, 81, 1.0, "sd3"), _fc(37, 129, 1.0, "shift"), _fc(3, 1, 1.0, "sd3"),
       _fc(4, 63, 2.0, "sd3"), _fc(1023, 21, 2.0, "sep"), _fc(4097, 21, 2.0, "sd40"), _fc(9, 1231, 2.0, "sd3"), _fc(7, 65, 2.0, "shift"),
       _fc(1, 2, 1.5, "shift"), _fc(4, 63, 1.5, "sep"), _fc(9, 1231, 1.5, "shift")])
FOCAL_BAD_TARGETS = (-1, None, 2 ** 31 - 1)                   # None stands for C


def focal_tol_regime(c):
    """N = 1 is a regime of its own: the loss is one row's term (1 - p)^gamma CE, and where that row is confidently right (CE of
    1e-2 and below) float32 keeps few digits of 1 - p and of CE itself; no mean over rows evens that out"""
    return c["regime"] + ("/N1" if c["N"] == 1 else "")


def focal_layout(C):
    """the hot path's rows [cls (K + 1) | box (4K) | pad] with K = C - 1: -> ld of the logits, ld_d of the gradient (different)"""
    w = 5 * (C - 1) + 1
    ld = (w + 7) // 8 * 8 + 8
    return ld, ld + 4


def focal_inputs(c):
    """-> logits (N, C) f32, targets (N,) i32"""
    N, C, reg = c["N"], c["C"], c["regime"]
    rng = np.random.default_rng(12000 + 31 * N + 7 * C + int(10 * c["gamma"]) + sum(map(ord, reg)))
    x = rng.normal(0.0, 40.0 if reg == "sd40" else 3.0, (N, C))
    t = rng.integers(0, C, N).astype(np.int32)
    if reg == "shift":
        x += 3e4
    if reg == "sep":
        assert C >= 2
        rows = np.arange(N)
        rest_hi = np.where(np.arange(C)[None] == t[:, None], -np.inf, x).max(1)
        rest_lo = np.where(np.arange(C)[None] == t[:, None], np.inf, x).min(1)
        x[rows, t] = np.where(rows % 2 == 0, rest_hi + 40.0, rest_lo - 40.0)
    return x.astype(np.float32), t


# ============================================================================================ sw_det_loss_per_image
def det_loss_ref(inp, rpn_bs, rpn_type, K, gamma, roi_type, rpn_weights=UNIT_WEIGHTS, roi_weights=REG_WEIGHTS):
    """float64 restatement of sw_det_loss_per_image (rpn.py:395-425, box_regression.py:229-268, fast_rcnn.py:73-105,497-564).
    inp = rpn logits (N, A), deltas (N, A, 4), labels (N, A), anchors (A, 4), matched (N, A, 4), roi logits (R, >= 5K + 1), classes (R,),
    boxes / gt boxes (R, 4), counts (N,) as torch tensors.  A class outside [0, K] makes its image's loss_cls (and the sum) NaN and
    takes the row out of the foreground set (include/soswsod_hip.h)."""
    lo, de, lab, an, ma, lg, cls, bx, gt, cnt = [t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy() for t in inp]
    N = lo.shape[0]
    res = np.zeros((N, 5))
    off = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for n in range(N):
            x, lb = lo[n], lab[n]
            v = lb >= 0
            bce = (np.maximum(x, 0) - x * (lb == 1) + np.log1p(np.exp(-np.abs(x))))[v].sum()
            fg = lb == 1
            l1 = np.abs(de[n][fg] - _deltas64(an[fg], ma[n][fg], rpn_weights)).sum()
            rc = bce / rpn_bs
            rl = (l1 / (4 * fg.sum())) / rpn_bs if rpn_type == "smooth_l1_mean" else l1 / rpn_bs
            c = int(cnt[n])
            rows = slice(off, off + c)
            off += c
            z = lg[rows, :K + 1]
            m = z.max(1, keepdims=True) if c else np.zeros((0, 1))
            lse = (m[:, 0] + np.log(np.exp(z - m).sum(1))) if c else np.zeros(0)
            t = cls[rows].astype(np.int64)
            bad = (t < 0) | (t > K)
            ce = np.where(bad, np.nan, lse - z[np.arange(c), np.where(bad, 0, t)])
            p = np.exp(-ce)
            lcls = ((1 - p) ** gamma * ce).sum() / c if c else 0.0
            f = (t < K) & ~bad
            pred = np.stack([lg[rows][f][i, K + 1 + 4 * t[f][i]: K + 5 + 4 * t[f][i]] for i in range(int(f.sum()))]) if f.any() else np.zeros((0, 4))
            bl = np.abs(pred - _deltas64(bx[rows][f], gt[rows][f], roi_weights)).sum()
            lbox = bl / (4 * f.sum()) if roi_type == "smooth_l1_mean" else bl / max(c, 1)
            res[n, :4] = lcls, lbox, rc, rl
            res[n, 4] = lcls + lbox + rc + rl
    return res


def det_loss_f32(inp, rpn_bs, rpn_type, K, gamma, roi_type, rpn_weights=UNIT_WEIGHTS, roi_weights=REG_WEIGHTS):
    """the same per image in float32 torch (binary_cross_entropy_with_logits, cross_entropy, get_deltas); NaN where det_loss_ref has one"""
    lo, de, lab, an, ma, lg, cls, bx, gt, cnt = [t.cpu() for t in inp]
    N = lo.shape[0]
    res = torch.zeros(N, 5)
    nan = float("nan")
    off = 0
    for n in range(N):
        v, fg = lab[n] >= 0, lab[n] == 1
        rc = F.binary_cross_entropy_with_logits(lo[n][v], fg[v].float(), reduction="sum") / rpn_bs
        l1 = (de[n][fg] - _deltas_t(an[fg], ma[n][fg], rpn_weights)).abs().sum()
        nfg = int(fg.sum())
        rl = ((l1 / (4 * nfg) if nfg else torch.tensor(nan)) / rpn_bs) if rpn_type == "smooth_l1_mean" else l1 / rpn_bs
        c = int(cnt[n])
        z, t = lg[off:off + c], cls[off:off + c].long()
        b, g = bx[off:off + c], gt[off:off + c]
        off += c
        bad = (t < 0) | (t > K)
        if c == 0:
            lcls = torch.tensor(0.0)
        elif bool(bad.any()):
            lcls = torch.tensor(nan)
        else:
            ce = F.cross_entropy(z[:, :K + 1], t, reduction="none")
            lcls = ((1.0 - torch.exp(-ce)).clamp_min(0.0) ** gamma * ce).sum() / c
        f = torch.nonzero((t < K) & ~bad)[:, 0]
        cols = (K + 1 + 4 * t[f])[:, None] + torch.arange(4)[None]
        bl = (z[f[:, None], cols] - _deltas_t(b[f], g[f], roi_weights)).abs().sum() if len(f) else torch.tensor(0.0)
        lbox = (bl / (4 * len(f)) if len(f) else torch.tensor(nan)) if roi_type == "smooth_l1_mean" else bl / max(c, 1)
        res[n, 0], res[n, 1], res[n, 2], res[n, 3] = lcls, lbox, rc, rl
        res[n, 4] = ((lcls + lbox) + rc) + rl
    return res.numpy()


def _dc(name, N, A, K, counts, max_rows, pad=3, bad_image=None, rpn_bs=256, shift=0.0):
    return dict(id=name, N=N, A=A, K=K, counts=list(counts), max_rows=max_rows, pad=pad, bad_image=bad_image, rpn_bs=rpn_bs, shift=shift)


# 65 images: the fold kernel's second workgroup; A at the 4096-anchor chunk; K + 1 = 81 logits: the wave's second pass over the classes;
# counts at the 64-row column; max_rows that is no multiple of 64, and 0; the exact pitch 5K + 1; one image with a class id K + 1; ROI
# logits shifted by 3e4 (as the focal kernel's regime "shift": the class term is invariant, the box term sees deltas of 3e4)
DETLOSS_CASES = (
    [_dc("img65", 65, 300, 20, [(0, 1, 63, 64, 65)[i % 5] for i in range(65)], 65)]
    + [_dc(f"A{A}", 2, A, 20, [5, 70], 128) for A in (1, 4095, 4096, 4097)]
    + [_dc(f"K{K}", 4, 300, K, [64, 65, 128, 129], 129) for K in (1, 80)]
    + [_dc("rows100", 2, 300, 20, [100, 37], 100, pad=0), _dc("rows0", 3, 300, 20, [0, 0, 0], 0),
       _dc("badclass", 3, 300, 20, [40, 70, 9], 128, bad_image=2), _dc("shift", 2, 300, 20, [5, 70], 128, shift=3e4)])
DETLOSS_TYPES = [("smooth_l1", 0.0), ("smooth_l1", 1.5), ("smooth_l1_mean", 0.0), ("smooth_l1_mean", 1.5)]


def detloss_inputs(c):
    """-> [rpn logits, deltas, labels i8, anchors, matched, roi logits (R, 5K + 1 + pad), classes i32, boxes, gt boxes, counts i32] CPU
    tensors, in det_loss_ref's order.  When N > 2, image 0 has no RPN foreground and image 1 no ROI foreground."""
    N, A, K, counts = c["N"], c["A"], c["K"], c["counts"]
    rng = np.random.default_rng(13000 + 31 * N + 7 * A + K + sum(counts))
    xy = rng.uniform(0.0, 600.0, (A, 2))
    an = np.concatenate([xy, xy + 8.0 + rng.uniform(0.0, 200.0, (A, 2))], 1).astype(np.float32)
    lab = np.full((N, A), -1, np.int8)
    for n in range(N):
        pick = rng.permutation(A)[:256]
        npos = 0 if (n == 0 and N > 2) else int(rng.integers(1, 129))
        lab[n, pick[:npos]] = 1; lab[n, pick[npos:]] = 0
    mxy = an[None, :, :2] + rng.normal(0.0, 10.0, (N, A, 2))
    ma = np.concatenate([mxy, mxy + 8.0 + rng.uniform(0.0, 200.0, (N, A, 2))], 2).astype(np.float32)
    lo = rng.normal(0.0, 3.0, (N, A)).astype(np.float32)
    de = rng.normal(0.0, 0.5, (N, A, 4)).astype(np.float32)
    R = int(sum(counts))
    lg = rng.normal(0.0, 2.0, (R, 5 * K + 1 + c["pad"])).astype(np.float32) + np.float32(c["shift"])
    cls = rng.integers(0, K + 1, R).astype(np.int32)
    if N > 2:
        cls[counts[0]:counts[0] + counts[1]] = K
    if c["bad_image"] is not None:
        o = int(sum(counts[:c["bad_image"]]))
        cls[o + 1] = K + 1; cls[o + counts[c["bad_image"]] - 1] = K + 1
    bxy = rng.uniform(0.0, 600.0, (R, 2))
    bx = np.concatenate([bxy, bxy + 4.0 + rng.uniform(0.0, 300.0, (R, 2))], 1).astype(np.float32)
    gxy = bxy + rng.normal(0.0, 20.0, (R, 2))
    gt = np.concatenate([gxy, gxy + 4.0 + rng.uniform(0.0, 300.0, (R, 2))], 1).astype(np.float32)
    out = [torch.from_numpy(np.ascontiguousarray(a)) for a in (lo, de, lab, an, ma, lg, cls, bx, gt, np.asarray(counts, np.int32))]
    return [t if t.numel() else torch.zeros(t.shape, dtype=t.dtype) for t in out]        # (NumPy gives an empty array strides of 0)


# ============================================================================================ sw_wsddn_scores_bwd
def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def wsddn_scores_bwd_ref(logits, K, g):
    """scores = softmax_k(C) * softmax_r(D), logits (R, >= 2K) = [C | D], g (R, K) the cotangent of the scores; with A = softmax_k(C),
    B = softmax_r(D):  dC = A (gB - sum_k A g B),  dD = B (gA - sum_r B g A).  -> dC, dD (R, K)"""
    x = np.asarray(logits, np.float64); g = np.asarray(g, np.float64)[:, :K]
    A, B = _softmax(x[:, :K], 1), _softmax(x[:, K:2 * K], 0)
    gB, gA = g * B, g * A
    return A * (gB - (A * gB).sum(1, keepdims=True)), B * (gA - (B * gA).sum(0, keepdims=True))


def wsddn_scores_bwd_f32(logits, K, g):
    """float32 torch softmaxes and autograd of sum(scores * g)"""
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(logits, np.float32)[:, :2 * K])).requires_grad_(True)
    gt = torch.from_numpy(np.ascontiguousarray(np.asarray(g, np.float32)[:, :K]))
    (F.softmax(x[:, :K], 1) * F.softmax(x[:, K:], 0) * gt).sum().backward()
    return x.grad[:, :K].numpy(), x.grad[:, K:].numpy()


def _sc(R, K, amp, shift=False):
    return dict(R=R, K=K, amp=amp, shift=shift, id=f"R{R}-K{K}-amp{amp:g}" + ("-shift" if shift else ""))


# R around the 128 rows of a workgroup; K = 63 / 64: the dynamic LDS (128 x (K + 1) x 8 B) crosses 64 KiB; K = 159: the last K that fits
SCORES_BWD_CASES = [_sc(1, 1, 3.0), _sc(127, 2, 12.0), _sc(128, 63, 3.0), _sc(129, 64, 30.0), _sc(300, 159, 12.0), _sc(37, 20, 3.0, True)]
SCORES_BWD_REFUSED = (160, 1025)


def scores_bwd_lds_bytes(K):
    return 128 * (K + 1) * 8


def scores_bwd_layout(K):
    """three different pitches: -> ld (logits), ld_g (cotangent), ld_d (gradient)"""
    return 2 * K + 3, K + 1, 2 * K + 5


def scores_bwd_inputs(c):
    """-> logits (R, 2K) f32, g (R, K) f32; shift: +-3e4 per row on the class block, per column on the detection block"""
    R, K = c["R"], c["K"]
    rng = np.random.default_rng(14000 + 31 * R + 7 * K)
    x = rng.normal(0.0, c["amp"], (R, 2 * K))
    if c["shift"]:
        x[:, :K] += 3e4 * rng.choice([-1.0, 1.0], (R, 1))
        x[:, K:] += 3e4 * rng.choice([-1.0, 1.0], (1, K))
    return x.astype(np.float32), rng.normal(0.0, 1.0, (R, K)).astype(np.float32)


# ============================================================================================ sw_threshold_select
SELECT_SIZES = (1023, 1025, 2048, 2049)                       # the 1024-thread pass: one short of it, one over, two full, two and one
SELECT_KINDS = ("all", "none", "ties", "nonfinite", "neginf")
SELECT_CASES = [dict(n=n, kind=k, id=f"n{n}-{k}") for n in SELECT_SIZES for k in SELECT_KINDS]
SELECT_FILTERS = {"rpn": ("no classes", None), "nofilter": ("classes", None), "three": ("classes", [3, 7, 19]), "empty": ("classes", [])}


def select_inputs(c):
    """-> scores (n,) f32, classes (n,) i32 in [0, 20), boxes (n, 4) f32, thres.  all / none: a threshold every / no score passes; ties:
    scores rounded to 0.01 with the threshold 0.7 among them (strict >); nonfinite: NaN, +inf and -inf scores at the pass edges;
    neginf: the same scores with thres = -inf (only NaN and -inf fail)"""
    n, kind = c["n"], c["kind"]
    rng = np.random.default_rng(15000 + n + sum(map(ord, kind)))
    scores = rng.uniform(0.0, 1.0, n).astype(np.float32)
    thres = 0.7
    if kind == "all":
        thres = -0.5
    elif kind == "none":
        thres = 1.0
    elif kind == "ties":
        scores = np.round(scores, 2)
    else:
        at = np.unique(np.concatenate([[0, 1, 2, n - 3, n - 2, n - 1], np.arange(1021, min(1027, n)), rng.choice(n, 30)]))
        scores[at] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(at)) % 3]
        thres = 0.5 if kind == "nonfinite" else -math.inf
    return scores, rng.integers(0, 20, n).astype(np.int32), rng.uniform(0.0, 500.0, (n, 4)).astype(np.float32), thres


# ============================================================================================ tolerance table
# (output kind, value regime) -> e32 = max over the cases of max|float32 restatement - float64| / max|float64|, measured by
# tests/test_losses_ref_cpu.py::test_tolerance_table_is_current (which fails when a bar this table gives is off a freshly computed one
# by more than a factor 2).  The detloss / scores_bwd rows decide no bar (fixed ones, above).
E32 = {
    ('detloss.out', 'all'): 2.23e-07,
    ('focal.dlogits', 'sd3'): 2.63e-07,
    ('focal.dlogits', 'sd3/N1'): 1.48e-05,
    ('focal.dlogits', 'sd40'): 2.18e-07,
    ('focal.dlogits', 'sd40/N1'): 0.00e+00,
    ('focal.dlogits', 'sep'): 2.24e-07,
    ('focal.dlogits', 'sep/N1'): 5.06e-07,
    ('focal.dlogits', 'shift'): 1.98e-07,
    ('focal.dlogits', 'shift/N1'): 2.98e-08,
    ('focal.loss', 'sd3'): 7.68e-08,
    ('focal.loss', 'sd3/N1'): 1.55e-05,
    ('focal.loss', 'sd40'): 5.78e-08,
    ('focal.loss', 'sd40/N1'): 0.00e+00,
    ('focal.loss', 'sep'): 9.60e-08,
    ('focal.loss', 'sep/N1'): 0.00e+00,
    ('focal.loss', 'shift'): 5.35e-08,
    ('focal.loss', 'shift/N1'): 3.38e-09,
    ('rpn.dlogits', 'w1'): 1.16e-07,
    ('rpn.dlogits', 'wreg'): 1.17e-07,
    ('rpn.loss_cls', 'w1'): 6.41e-08,
    ('rpn.loss_cls', 'wreg'): 7.00e-08,
    ('rpn.loss_loc', 'w1'): 1.07e-07,
    ('rpn.loss_loc', 'wreg'): 3.10e-07,
    ('scores_bwd.dC', 'amp12'): 4.66e-07,
    ('scores_bwd.dC', 'amp3'): 2.73e-07,
    ('scores_bwd.dC', 'amp30'): 3.52e-08,
    ('scores_bwd.dD', 'amp12'): 8.25e-08,
    ('scores_bwd.dD', 'amp3'): 3.41e-07,
    ('scores_bwd.dD', 'amp30'): 1.24e-07,
}

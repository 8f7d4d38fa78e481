"""float64 restatements of the WSDDN / OICR head kernels (checkers, not product code), the inputs of the head-kernel edge tests,
and the tolerance table those tests read.

Every reference takes the float32 inputs the kernel gets, upcast to float64, so input rounding is common to both sides.  The formulas
are the ones cited in csrc/heads.hip and oracle/oicr_oracle.py; tests/test_heads_ref_cpu.py pins each restatement to the oracle.

Tolerances.  The bar of a float output is taken against the reference, never against the kernel: the plain float32 torch restatement
of the same formula runs on the same inputs (the *_f32 functions here), e32 = max|f32 - f64| / max|f64| per output kind and value
regime, and the GPU bar is max(2e-5, 8 * e32) of max|ref| (2e-5: the bar these kernels already have; 8: a different but legitimate
summation order, expf versus libm).  E32 below is that table; test_heads_ref_cpu.py recomputes it and asserts it is current.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

# the clamp bounds of the image-level score are the float32 values (fast_rcnn_wsddn.py:340-375 clamps a float32 tensor)
CLAMP_LO = np.float32(1e-6)
CLAMP_HI = np.float32(1.0 - 1e-6)
BAR_FLOOR = 2e-5
BAR_FACTOR = 8.0
REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
SCALE_CLAMP = math.log(1000.0 / 16)


def bar(kind, regime):
    """allowed max|got - ref| / max|ref| of output `kind` in value regime `regime`"""
    return max(BAR_FLOOR, BAR_FACTOR * E32[(kind, regime)])


def rel_err(got, ref):
    """max|got - ref| / max|ref| (0 / 0 -> 0: an all-zero reference asks for exact zeros; NaN -> inf)"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    d = float(np.max(np.abs(got - ref))); m = float(np.max(np.abs(ref)))
    if not d <= math.inf:
        return math.inf
    return 0.0 if d == 0.0 else (math.inf if m == 0.0 else d / m)


def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


# ============================================================================================ WSDDN
def wsddn_ref(logits64, V, R, K, cls_col, det_col, gt_onehot, grad_scale):
    """logits64 (V*R, ld) float64.  -> dict: scores (V,R,K), loss (V,), dcls / ddet (V,R,K) = the gradient of
    sum_v loss_v / V * grad_scale wrt the two logit blocks, mean (R,K) view-mean scores, raw (V,K) image-level scores,
    clamped (V,K) bool (raw outside the float32 clamp bounds: zero gradient through that class)."""
    x = np.asarray(logits64, np.float64).reshape(V, R, -1)
    t = np.asarray(gt_onehot, np.float64).reshape(K)
    p = _softmax(x[:, :, cls_col:cls_col + K], 2)             # over classes
    q = _softmax(x[:, :, det_col:det_col + K], 1)             # over proposals
    s = p * q
    raw = s.sum(1)                                            # (V, K)
    lo, hi = float(CLAMP_LO), float(CLAMP_HI)
    y = np.clip(raw, lo, hi)
    loss = (-(t * np.log(y) + (1.0 - t) * np.log1p(-y))).mean(1)          # BCE(mean over K) / N_img, N_img = 1
    clamped = (raw < lo) | (raw > hi)
    g = np.where(clamped, 0.0, -(t / y - (1.0 - t) / (1.0 - y)) / K) * (float(grad_scale) / V)      # dL/draw (V, K)
    dot = (g[:, None, :] * s).sum(2, keepdims=True)           # sum_j g_j s_rj
    dcls = p * (g[:, None, :] * q - dot)
    ddet = g[:, None, :] * q * (p - raw[:, None, :])
    return dict(scores=s, loss=loss, dcls=dcls, ddet=ddet, mean=s.mean(0), raw=raw, clamped=clamped)


def wsddn_f32(logits32, V, R, K, cls_col, det_col, gt_onehot, grad_scale):
    """the same formula as the project already trusts it: float32 torch softmaxes, oracle.wsddn_loss, autograd"""
    from oracle import oicr_oracle as O
    x = torch.from_numpy(np.nan_to_num(np.asarray(logits32, np.float32))).clone().requires_grad_(True)
    t = torch.from_numpy(np.asarray(gt_onehot, np.float32)).view(1, K)
    xs = x.view(V, R, -1)
    sc, losses = [], []
    for v in range(V):
        s = F.softmax(xs[v, :, cls_col:cls_col + K], 1) * F.softmax(xs[v, :, det_col:det_col + K], 0)
        sc.append(s); losses.append(O.wsddn_loss(s, t))
    (sum(losses) / V * float(grad_scale)).backward()
    g = x.grad.view(V, R, -1).numpy()
    s = torch.stack(sc).detach()
    return dict(scores=s.numpy(), loss=torch.stack(losses).detach().numpy(), dcls=g[:, :, cls_col:cls_col + K],
                ddet=g[:, :, det_col:det_col + K], mean=s.mean(0).numpy())


def _offcol(c):
    return c if c % 4 else c + 1


def wsddn_layout(K, which):
    """-> cls_col, det_col, ld, ld_d, mean_pitch: block columns that are no multiples of 4, an odd row pitch, a gradient pitch that
    differs from it; which = 1 puts the detection block first and gives the mean scores the K + 1 pitch of the mining input"""
    if which == 0:
        cls_col = 3; det_col = _offcol(cls_col + K + 2); mean_pitch = K
    else:
        det_col = 1; cls_col = _offcol(det_col + K + 5); mean_pitch = K + 1
    ld = max(cls_col, det_col) + K + 3
    ld += 1 - ld % 2
    return cls_col, det_col, ld, ld + 4 + which, mean_pitch


def _wc(V, R, K, regime, layout, gt="mix", seed=0):
    return dict(V=V, R=R, K=K, regime=regime, layout=layout, gt=gt, seed=seed,
                id=f"V{V}-R{R}-K{K}-{regime}-L{layout}-{gt}")


# value regimes: a N(0,3^2); b15 / b40 N(0,15^2) / N(0,40^2); c = a plus a per-row constant of +-3e4 on the class block and a
# per-column constant of +-3e4 on the detection block (softmax invariant; overflows without the max subtraction); d = a with two
# detection columns whose row chunks differ by more than float32's exp range (column 0: maximum in the last, one-row chunk, 200 above
# every other row; column 1: maximum in the first chunk, 200 above every row of the other chunks); e = a with saturated classes (image
# score < 1e-6; K = 1 has image score 1; K = 2: both classes saturated)
WSDDN_CASES = [
    _wc(1, 1, 1, "a", 0), _wc(1, 2, 2, "a", 1), _wc(2, 255, 20, "a", 0), _wc(3, 256, 80, "a", 1), _wc(4, 257, 128, "a", 0),
    _wc(8, 513, 20, "a", 1), _wc(4, 2000, 20, "a", 0), _wc(1, 2000, 80, "a", 1), _wc(8, 1, 20, "a", 0), _wc(2, 2, 128, "a", 1),
    _wc(3, 513, 1, "a", 0), _wc(4, 255, 2, "a", 1), _wc(8, 256, 128, "a", 0),
    _wc(4, 257, 20, "b15", 1), _wc(1, 2000, 128, "b15", 0), _wc(8, 255, 80, "b15", 1), _wc(2, 1, 20, "b15", 0),
    _wc(4, 2000, 20, "b40", 0), _wc(3, 256, 2, "b40", 1), _wc(1, 1, 20, "b40", 0), _wc(2, 513, 80, "b40", 1),
    _wc(8, 257, 128, "b40", 0),
    _wc(4, 257, 20, "c", 0), _wc(1, 256, 128, "c", 1), _wc(8, 2000, 2, "c", 0), _wc(2, 513, 80, "c", 1), _wc(3, 1, 20, "c", 0),
    _wc(4, 255, 1, "c", 1),
    _wc(4, 257, 20, "d", 1), _wc(1, 513, 80, "d", 0), _wc(8, 513, 128, "d", 1), _wc(2, 257, 2, "d", 0),
    _wc(4, 257, 20, "e", 0, "mix"), _wc(2, 255, 1, "e", 1, "zero"), _wc(4, 256, 1, "e", 0, "one"), _wc(1, 513, 2, "e", 1, "zero"),
    _wc(8, 2, 2, "e", 0, "one"), _wc(3, 2000, 80, "e", 1, "mix"), _wc(4, 513, 128, "e", 0, "one"), _wc(2, 2000, 20, "e", 1, "zero"),
]


def wsddn_tol_regime(c):
    """R = 1 is a regime of its own: the detection softmax is exactly 1 there and the image score is one class probability, whose
    BCE gradient 1 / (1 - y) is ill conditioned in float32 in a way no larger R is"""
    return c["regime"] + ("/R1" if c["R"] == 1 else "")


def wsddn_inputs(c):
    """-> logits (V*R, ld) f32 (columns outside the two blocks hold NaN: the kernel must not read them), gt_onehot (K,) f32,
    grad_scale f32"""
    V, R, K, reg = c["V"], c["R"], c["K"], c["regime"]
    cls_col, det_col, ld, _, _ = wsddn_layout(K, c["layout"])
    rng = np.random.default_rng(1000 + 7919 * c["seed"] + 31 * V + 17 * R + K + sum(map(ord, reg)))
    sd = {"b15": 15.0, "b40": 40.0}.get(reg, 3.0)
    C = rng.normal(0.0, sd, (V, R, K)); D = rng.normal(0.0, sd, (V, R, K))
    if reg == "c":
        C += 3e4 * rng.choice([-1.0, 1.0], (V, R, 1))
        D += 3e4 * rng.choice([-1.0, 1.0], (V, 1, K))
    if reg == "d":
        assert R > 256 and (R - 1) % 256 == 0 and K >= 2
        D[:, R - 1, 0] = D[:, :R - 1, 0].max(1) + 200.0
        D[:, 256:, 1] -= 200.0 + (D[:, 256:, 1].max(1) - D[:, :256, 1].max(1))[:, None]
    if reg == "e":
        if K == 2:
            C[:, :, 0] += 60.0                                # class 0 -> image score 1, class 1 -> ~0: every class clamped
        elif K > 2:
            C[:, :, 1::3] -= 60.0
    lg = np.full((V, R, ld), np.nan, np.float32)
    lg[:, :, cls_col:cls_col + K] = C; lg[:, :, det_col:det_col + K] = D
    gt = np.zeros(K, np.float32)
    if c["gt"] == "one":
        gt[:] = 1
    elif c["gt"] == "mix":
        gt[[min(1, K - 1), K // 2]] = 1
    return lg.reshape(V * R, ld), gt, np.float32(0.7)


def clamp_distance_ok(raw):
    """no image-level score within 1e-4 relative of the lower clamp bound or 5e-7 absolute of the upper one (the clamp is a
    discontinuity of the gradient: float32 and float64 must fall on the same side)"""
    lo, hi = float(CLAMP_LO), float(CLAMP_HI)
    return bool(np.all(np.abs(raw - lo) > 1e-4 * lo) and np.all(np.abs(raw - hi) > 5e-7))


# ============================================================================================ mean probs
def mean_probs_ref(logits64, V, R, K, n_rounds, cls_col0, col_stride):
    x = np.asarray(logits64, np.float64).reshape(V, R, -1)
    return np.stack([_softmax(x[:, :, cls_col0 + k * col_stride:cls_col0 + k * col_stride + K + 1], 2).mean(0)
                     for k in range(n_rounds)])


def mean_probs_f32(logits32, V, R, K, n_rounds, cls_col0, col_stride):
    x = torch.from_numpy(np.ascontiguousarray(logits32, np.float32)).view(V, R, -1)
    return torch.stack([F.softmax(x[:, :, cls_col0 + k * col_stride:cls_col0 + k * col_stride + K + 1], 2).mean(0)
                        for k in range(n_rounds)]).numpy()


def _mc(V, R, K, NR, sd):
    return dict(V=V, R=R, K=K, NR=NR, sd=sd, id=f"V{V}-R{R}-K{K}-NR{NR}-sd{sd:g}")


MEAN_PROBS_CASES = [
    _mc(1, 1, 1, 1, 3.0), _mc(1, 63, 20, 3, 3.0), _mc(1, 2000, 80, 1, 40.0), _mc(4, 64, 20, 3, 3.0), _mc(4, 65, 1, 3, 40.0),
    _mc(4, 2000, 20, 3, 40.0), _mc(4, 63, 80, 1, 3.0), _mc(4, 65, 80, 3, 40.0), _mc(8, 1, 20, 3, 3.0), _mc(8, 64, 1, 1, 3.0),
    _mc(8, 65, 20, 1, 40.0), _mc(8, 2000, 20, 3, 3.0), _mc(1, 65, 1, 3, 3.0), _mc(4, 1, 80, 3, 3.0),
]
MEAN_PROBS_TOO_BIG = (8, 80)          # V * 64 * (K + 1) * 4 bytes > 150 KB: rejected


def mean_probs_lds_bytes(V, K):
    return V * 64 * (K + 1) * 4


def head_layout(K, NR):
    """refinement heads side by side: round k has its K + 1 class logits at cls_col + k * stride and its 4K box deltas behind them;
    -> cls_col, box_col, stride, ld (odd)"""
    cls_col, stride = 7, 5 * K + 1 + 2
    ld = cls_col + NR * stride + 3
    ld += 1 - ld % 2
    return cls_col, cls_col + K + 1, stride, ld


def mean_probs_inputs(c):
    V, R, K, NR = c["V"], c["R"], c["K"], c["NR"]
    cls_col, _, stride, ld = head_layout(K, NR)
    rng = np.random.default_rng(2000 + 31 * V + 17 * R + K + NR)
    lg = np.full((V * R, ld), np.nan, np.float32)
    for k in range(NR):
        lg[:, cls_col + k * stride:cls_col + k * stride + K + 1] = rng.normal(0.0, c["sd"], (V * R, K + 1))
    return lg


# ============================================================================================ refine loss
def _deltas64(src, tgt, w):
    sw = src[:, 2] - src[:, 0]; sh = src[:, 3] - src[:, 1]
    sx = src[:, 0] + 0.5 * sw; sy = src[:, 1] + 0.5 * sh
    tw = tgt[:, 2] - tgt[:, 0]; th = tgt[:, 3] - tgt[:, 1]
    tx = tgt[:, 0] + 0.5 * tw; ty = tgt[:, 1] + 0.5 * th
    return np.stack((w[0] * (tx - sx) / sw, w[1] * (ty - sy) / sh, w[2] * np.log(tw / sw), w[3] * np.log(th / sh)), 1)


def refine_ref(logits64, V, R, K, cls_col, box_col, boxes, lab_class, lab_weight, lab_index, pred_view, reg_weights, grad_scale,
               n_rounds=1, col_stride=0):
    """-> loss (n_rounds, 2, V) [term 0 = weighted CE (ignore_index -1, weight 0 for -1), term 1 = L1 on the gt-class deltas of
    0 <= gt < K; both over ALL R], dcls (n_rounds, V, R, K+1) and dbox (n_rounds, V, R, 4K): the gradient of
    sum_k sum_v (loss[k,0,v] * gs[2k] + loss[k,1,v] * gs[2k+1]) / V wrt the logits of PREDICTION view pv = the sum over the target
    views v with pred_view[v] == pv, and min_l1 = the smallest |pred - target| / (1 + |target|) among the differences that are not
    exactly zero."""
    x = np.asarray(logits64, np.float64).reshape(V, R, -1)
    B = np.asarray(boxes, np.float64).reshape(V, R, 4)
    lc = np.asarray(lab_class).reshape(n_rounds, R); lw = np.asarray(lab_weight, np.float64).reshape(n_rounds, R)
    li = np.asarray(lab_index).reshape(n_rounds, R); gs = np.asarray(grad_scale, np.float64).reshape(n_rounds, 2)
    K1 = K + 1
    loss = np.zeros((n_rounds, 2, V)); dcls = np.zeros((n_rounds, V, R, K1)); dbox = np.zeros((n_rounds, V, R, 4 * K))
    min_l1 = math.inf
    rows = np.arange(R)
    for k in range(n_rounds):
        gt = lc[k].astype(np.int64)
        w = np.where(gt == -1, 0.0, lw[k])
        valid = gt >= 0
        fg = np.nonzero(valid & (gt < K))[0]
        cols = 4 * gt[fg][:, None] + np.arange(4)
        oh = np.zeros((R, K1)); oh[rows[valid], gt[valid]] = 1.0
        for v in range(V):
            pv = int(pred_view[v])
            xc = x[pv, :, cls_col + k * col_stride:cls_col + k * col_stride + K1]
            xb = x[pv, :, box_col + k * col_stride:box_col + k * col_stride + 4 * K]
            m = xc.max(1, keepdims=True)
            logp = xc - m - np.log(np.exp(xc - m).sum(1, keepdims=True))
            ce = np.where(valid, -logp[rows, np.where(valid, gt, 0)], 0.0)
            loss[k, 0, v] = (ce * w).mean()
            dcls[k, pv] += (gs[k, 0] / V / R) * (w * valid)[:, None] * (np.exp(logp) - oh)
            if len(fg):
                tgt = _deltas64(B[v][fg], B[v][li[k][fg]], reg_weights)
                diff = xb[fg[:, None], cols] - tgt
                loss[k, 1, v] = np.abs(diff).sum() / R
                dbox[k, pv][fg[:, None], cols] += (gs[k, 1] / V / R) * np.sign(diff)
                nz = diff != 0.0
                if nz.any():
                    min_l1 = min(min_l1, float((np.abs(diff) / (1.0 + np.abs(tgt)))[nz].min()))
    return dict(loss=loss, dcls=dcls, dbox=dbox, min_l1=min_l1)


def refine_f32(logits32, V, R, K, cls_col, box_col, boxes, lab_class, lab_weight, lab_index, pred_view, reg_weights, grad_scale,
               n_rounds=1, col_stride=0):
    """the same losses through oracle.oicr_oracle.oicr_losses in float32 + autograd (what the project already trusts)"""
    from oracle import oicr_oracle as O
    assert tuple(reg_weights) == tuple(O.BBOX_REG_WEIGHTS)
    x = torch.from_numpy(np.nan_to_num(np.asarray(logits32, np.float32))).clone().requires_grad_(True)
    xs = x.view(V, R, -1)
    B = np.asarray(boxes, np.float32).reshape(V, R, 4)
    lc = np.asarray(lab_class).reshape(n_rounds, R); lw = np.asarray(lab_weight, np.float32).reshape(n_rounds, R)
    li = np.asarray(lab_index).reshape(n_rounds, R); gs = np.asarray(grad_scale, np.float32).reshape(n_rounds, 2)
    loss = np.zeros((n_rounds, 2, V), np.float32)
    total = 0.0
    for k in range(n_rounds):
        for v in range(V):
            blk = xs[int(pred_view[v])]
            a, b = O.oicr_losses(blk[:, cls_col + k * col_stride:cls_col + k * col_stride + K + 1],
                                 blk[:, box_col + k * col_stride:box_col + k * col_stride + 4 * K], B[v], B[v][li[k]], lc[k], lw[k], K)
            loss[k, 0, v], loss[k, 1, v] = float(a.detach()), float(b.detach())
            total = total + (a * float(gs[k, 0]) + b * float(gs[k, 1])) / V
    total.backward()
    g = x.grad.view(V, R, -1).numpy()
    dcls = np.stack([g[:, :, cls_col + k * col_stride:cls_col + k * col_stride + K + 1] for k in range(n_rounds)])
    dbox = np.stack([g[:, :, box_col + k * col_stride:box_col + k * col_stride + 4 * K] for k in range(n_rounds)])
    return dict(loss=loss, dcls=dcls, dbox=dbox)


PRED_VIEWS = {"v1": [0], "share2": [0, 1, 2, 2], "own": [0, 1, 2, 3], "all0": [0, 0, 0, 0], "rev": [3, 2, 1, 0],
              "v8": [0, 1, 2, 2, 5, 5, 7, 0]}          # v8: views 3, 4 and 6 serve no target


def _rc(pv, R, K, NR, labels, sd):
    return dict(pv=pv, V=len(PRED_VIEWS[pv]), R=R, K=K, NR=NR, labels=labels, sd=sd, id=f"{pv}-R{R}-K{K}-NR{NR}-{labels}-sd{sd:g}")


# labels: ignore = all -1; bg = all K; fg = all foreground; mixed = -1 .. K with weights that include exact 0; self = foreground with
# lab_index[r] == r and zero predicted deltas (target and difference exactly 0: the sign(0) branch of the L1 gradient)
REFINE_CASES = [
    _rc("v1", 1, 1, 1, "fg", 2.0), _rc("v1", 3, 20, 3, "mixed", 2.0), _rc("v1", 2000, 80, 1, "mixed", 40.0),
    _rc("v1", 257, 20, 4, "self", 2.0), _rc("v1", 5, 1, 4, "mixed", 40.0),
    _rc("share2", 1, 20, 1, "mixed", 2.0), _rc("share2", 4, 80, 3, "mixed", 2.0), _rc("share2", 257, 20, 4, "mixed", 40.0),
    _rc("share2", 2000, 20, 1, "fg", 2.0), _rc("share2", 5, 20, 1, "ignore", 2.0), _rc("share2", 3, 1, 3, "bg", 2.0),
    _rc("share2", 257, 1, 1, "self", 2.0),
    _rc("own", 4, 20, 3, "mixed", 40.0), _rc("own", 257, 80, 1, "fg", 2.0), _rc("own", 5, 1, 4, "fg", 2.0),
    _rc("own", 2000, 20, 3, "mixed", 2.0),
    _rc("all0", 3, 20, 1, "mixed", 2.0), _rc("all0", 257, 20, 3, "fg", 40.0), _rc("all0", 5, 80, 1, "self", 2.0),
    _rc("all0", 2000, 1, 1, "mixed", 2.0),
    _rc("rev", 1, 80, 4, "fg", 2.0), _rc("rev", 4, 20, 1, "bg", 40.0), _rc("rev", 257, 20, 3, "mixed", 2.0),
    _rc("rev", 2000, 80, 1, "mixed", 2.0),
    _rc("v8", 3, 20, 4, "mixed", 2.0), _rc("v8", 5, 1, 1, "fg", 40.0), _rc("v8", 257, 80, 1, "mixed", 2.0),
    _rc("v8", 2000, 20, 1, "mixed", 40.0), _rc("v8", 4, 20, 3, "ignore", 2.0), _rc("v8", 257, 20, 1, "self", 40.0),
]


def refine_tol_regime(c):
    return f"sd{c['sd']:g}"


def random_boxes(rng, n, size=300.0):
    """(n, 4) f32 boxes with sides >= 8"""
    xy = rng.uniform(0.0, size - 40.0, (n, 2)); wh = rng.uniform(8.0, 120.0, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def refine_inputs(c):
    """-> dict(logits (V*R, ld) f32 with NaN outside the heads' columns, boxes (V,R,4), lab_class / lab_index (NR,R) i32,
    lab_weight (NR,R) f32, pred_view i32, grad_scale (2*NR,) f32, cls_col, box_col, stride, ld)"""
    V, R, K, NR = c["V"], c["R"], c["K"], c["NR"]
    cls_col, box_col, stride, ld = head_layout(K, NR)
    rng = np.random.default_rng(3000 + 31 * V + 17 * R + K + 5 * NR + sum(map(ord, c["labels"] + c["pv"])))
    lg = np.full((V * R, ld), np.nan, np.float32)
    for k in range(NR):
        lg[:, cls_col + k * stride:cls_col + k * stride + 5 * K + 1] = rng.normal(0.0, c["sd"], (V * R, 5 * K + 1))
    boxes = random_boxes(rng, V * R).reshape(V, R, 4)
    mode = c["labels"]
    lab_i = rng.integers(0, R, (NR, R)).astype(np.int32)
    lab_w = rng.uniform(0.05, 1.0, (NR, R)).astype(np.float32)
    if mode == "ignore":
        lab_c = np.full((NR, R), -1, np.int32)
    elif mode == "bg":
        lab_c = np.full((NR, R), K, np.int32)
    elif mode in ("fg", "self"):
        lab_c = rng.integers(0, K, (NR, R)).astype(np.int32)
    else:
        lab_c = rng.integers(-1, K + 1, (NR, R)).astype(np.int32)
        lab_w[rng.random((NR, R)) < 0.25] = 0.0
    if mode == "self":
        lab_i[:] = np.arange(R, dtype=np.int32)[None]
        for k in range(NR):
            lg[:, box_col + k * stride:box_col + k * stride + 4 * K] = 0.0
    # the L1 gradient is a sign: move every predicted delta that lies within 2e-4 (1 + |target|) of a target it is compared with
    # away from it (a few passes: one prediction row can serve several target views)
    pvw = PRED_VIEWS[c["pv"]]
    for _ in range(8):
        moved = False
        for k in range(NR if mode != "self" else 0):
            fg = np.nonzero((lab_c[k] >= 0) & (lab_c[k] < K))[0]
            cols = box_col + k * stride + 4 * lab_c[k][fg].astype(np.int64)[:, None] + np.arange(4)
            for v in range(V):
                tgt = _deltas64(boxes[v][fg].astype(np.float64), boxes[v][lab_i[k][fg]].astype(np.float64), REG_WEIGHTS)
                rows = (pvw[v] * R + fg)[:, None]
                near = np.abs(lg[rows, cols].astype(np.float64) - tgt) < 2e-4 * (1.0 + np.abs(tgt))
                if near.any():
                    lg[rows, cols] = np.where(near, lg[rows, cols] + np.float32(0.013), lg[rows, cols]); moved = True
        if not moved:
            break
    gs = rng.uniform(0.5, 1.5, 2 * NR).astype(np.float32)
    return dict(logits=lg, boxes=boxes, lab_class=lab_c, lab_weight=lab_w, lab_index=lab_i,
                pred_view=np.asarray(PRED_VIEWS[c["pv"]], np.int32), grad_scale=gs, cls_col=cls_col, box_col=box_col, stride=stride,
                ld=ld)


# ============================================================================================ inference decode
def predict_ref(logits64, R, K, refine_k, base_col, round_stride, boxes, reg_weights, scale_clamp):
    """all_scores (R, K+1) = mean over rounds of softmax; all_boxes (R, 4K) = apply_deltas(mean over rounds of the deltas) with dw / dh
    clamped from above at scale_clamp (the float32 value the kernel receives)"""
    x = np.asarray(logits64, np.float64)[:R]
    K1 = K + 1
    sc = np.mean([_softmax(x[:, base_col + k * round_stride:base_col + k * round_stride + K1], 1) for k in range(refine_k)], 0)
    d = np.mean([x[:, base_col + k * round_stride + K1:base_col + k * round_stride + K1 + 4 * K] for k in range(refine_k)], 0)
    b = np.asarray(boxes, np.float64)[:R]
    w = (b[:, 2] - b[:, 0])[:, None]; h = (b[:, 3] - b[:, 1])[:, None]
    cx = b[:, 0:1] + 0.5 * w; cy = b[:, 1:2] + 0.5 * h
    clamp = float(np.float32(scale_clamp))
    dx = d[:, 0::4] / reg_weights[0]; dy = d[:, 1::4] / reg_weights[1]
    dw = np.minimum(d[:, 2::4] / reg_weights[2], clamp); dh = np.minimum(d[:, 3::4] / reg_weights[3], clamp)
    px = dx * w + cx; py = dy * h + cy; pw = np.exp(dw) * w; ph = np.exp(dh) * h
    out = np.zeros((R, 4 * K))
    out[:, 0::4] = px - 0.5 * pw; out[:, 1::4] = py - 0.5 * ph; out[:, 2::4] = px + 0.5 * pw; out[:, 3::4] = py + 0.5 * ph
    return sc, out


def predict_f32(logits32, R, K, refine_k, base_col, round_stride, boxes, reg_weights, scale_clamp):
    """float32 torch softmaxes and oracle.apply_deltas"""
    from oracle import oicr_oracle as O
    x = torch.from_numpy(np.ascontiguousarray(logits32, np.float32))[:R]
    K1 = K + 1
    probs, deltas = 0.0, 0.0
    for k in range(refine_k):
        probs = probs + F.softmax(x[:, base_col + k * round_stride:base_col + k * round_stride + K1], -1)
        deltas = deltas + x[:, base_col + k * round_stride + K1:base_col + k * round_stride + K1 + 4 * K]
    pb = O.apply_deltas(deltas / float(refine_k), torch.from_numpy(np.asarray(boxes, np.float32))[:R], reg_weights,
                        float(np.float32(scale_clamp)))
    return (probs / float(refine_k)).numpy(), pb.numpy()


def _pc(R, K, RK, layout, clamp):
    return dict(R=R, K=K, RK=RK, layout=layout, clamp=clamp, id=f"R{R}-K{K}-RK{RK}-{layout}-clamp{clamp:.3f}")


EXACT_CLAMP = 4.125           # 5 * 4.125 and 4.125 are exact in float32: a delta of 20.625 / weight 5 sits exactly at the clamp
# layout train: base_col 2K, round_stride 5K+1 (the packed training logits); api: base_col 0 (predictor_api.py); both with an odd ld
PREDICT_CASES = [
    _pc(1, 1, 1, "train", SCALE_CLAMP), _pc(1, 20, 4, "api", EXACT_CLAMP), _pc(255, 20, 3, "train", EXACT_CLAMP),
    _pc(255, 80, 1, "api", SCALE_CLAMP), _pc(256, 1, 4, "api", EXACT_CLAMP), _pc(256, 20, 4, "train", SCALE_CLAMP),
    _pc(257, 80, 3, "train", EXACT_CLAMP), _pc(257, 20, 1, "api", SCALE_CLAMP), _pc(4000, 20, 4, "train", EXACT_CLAMP),
    _pc(4000, 1, 3, "train", SCALE_CLAMP), _pc(4000, 80, 1, "api", EXACT_CLAMP), _pc(257, 1, 1, "train", EXACT_CLAMP),
    _pc(1, 80, 3, "api", SCALE_CLAMP),
]


def predict_inputs(c):
    """-> logits (R, ld) f32 (NaN outside the rounds' columns), boxes (R, 4) f32, base_col, round_stride"""
    R, K, RK = c["R"], c["K"], c["RK"]
    base = 2 * K if c["layout"] == "train" else 0
    stride = 5 * K + 1
    ld = base + RK * stride + 2
    ld += 1 - ld % 2
    rng = np.random.default_rng(4000 + 17 * R + K + 5 * RK)
    lg = np.full((R, ld), np.nan, np.float32)
    for k in range(RK):
        c0 = base + k * stride
        lg[:, c0:c0 + K + 1] = rng.normal(0.0, 10.0, (R, K + 1))
        d = rng.normal(0.0, 4.0, (R, K, 4))
        d[:, :, 2:] *= 4.0                                    # dw / dh / 5 beyond the clamp in a good share of the entries
        lg[:, c0 + K + 1:c0 + 5 * K + 1] = d.reshape(R, 4 * K)
    boxes = random_boxes(rng, R)
    boxes[0, 2:] = boxes[0, :2]                               # a zero-area proposal
    for k in range(RK):                   # last row, in every round (so the mean is exact): clamp active, exactly at it, negative
        c0 = base + k * stride + K + 1
        lg[R - 1, c0:c0 + 4] = (1.0, -2.0, 5.0 * EXACT_CLAMP, 40.0)
        if K > 1:
            lg[R - 1, c0 + 4:c0 + 8] = (-3.0, 0.5, -30.0, 5.0 * EXACT_CLAMP)
    return lg, boxes, base, stride


# ============================================================================================ small elementwise heads
def loss_finalize_ref(lv64):
    """lv (B, n, V) -> out (n,) mean over views and images, total = their sum"""
    out = np.asarray(lv64, np.float64).mean(2).mean(0)
    return out, out.sum()


def loss_finalize_f32(lv32):
    out = torch.from_numpy(np.asarray(lv32, np.float32)).mean(2).mean(0)
    return out.numpy(), out.sum().numpy()


def scale_cols_loss_ref(src64, g_losses, g_total, col_to_loss, mul, n_valid):
    """out[m][n] = src[m][n] * ((g_losses[col_to_loss[n]] or 0) + (g_total or 0)) * mul for n < n_valid, exactly 0 beyond (src is
    not read there)"""
    src = np.asarray(src64, np.float64)
    M, N = src.shape
    cs = np.zeros(n_valid)
    if g_losses is not None:
        cs += np.asarray(g_losses, np.float64)[np.asarray(col_to_loss)[:n_valid]]
    if g_total is not None:
        cs += float(np.asarray(g_total).reshape(-1)[0])
    out = np.zeros((M, N))
    out[:, :n_valid] = src[:, :n_valid] * (cs * float(np.float32(mul)))[None]
    return out


def scale_cols_loss_f32(src32, g_losses, g_total, col_to_loss, mul, n_valid):
    src = np.asarray(src32, np.float32)
    cs = np.zeros(n_valid, np.float32)
    if g_losses is not None:
        cs = cs + np.asarray(g_losses, np.float32)[np.asarray(col_to_loss)[:n_valid]]
    if g_total is not None:
        cs = cs + np.float32(np.asarray(g_total).reshape(-1)[0])
    out = np.zeros(src.shape, np.float32)
    out[:, :n_valid] = src[:, :n_valid] * (cs * np.float32(mul))[None]
    return out


def mean_views_ref(x64):
    return np.asarray(x64, np.float64).mean(0)


def mean_views_f32(x32):
    return torch.from_numpy(np.asarray(x32, np.float32)).mean(0).numpy()


FINALIZE_CASES = [(n, V, B) for n in (1, 9, 64) for V in (1, 4) for B in (1, 2, 3)]
# (M, N, n_valid, ld_in extra, ld_out extra, with g_losses)
SCALE_COLS_CASES = [(37, 21, 17, 0, 3, True), (300, 408, 405, 4, 0, True), (1, 5, 5, 2, 1, True), (129, 31, 1, 0, 0, False),
                    (2000, 104, 101, 8, 8, False), (3, 85, 80, 1, 2, True)]
MEAN_VIEWS_CASES = [(1, 1), (4, 1), (1, 255), (4, 257), (4, 2000 * 21), (3, 1000), (8, 513)]


def finalize_inputs(n, V, B):
    return np.random.default_rng(5000 + 64 * n + 8 * V + B).uniform(0.0, 3.0, (B, n, V)).astype(np.float32)


def scale_cols_inputs(M, N, n_valid, n_losses=9):
    """-> src (M, N) f32 with NaN in the pad columns, g_losses (n_losses,), g_total (1,), col_to_loss (N,) i32, mul"""
    rng = np.random.default_rng(6000 + 31 * M + N + n_valid)
    src = rng.normal(0.0, 2.0, (M, N)).astype(np.float32)
    src[:, n_valid:] = np.nan
    return (src, rng.uniform(0.5, 1.5, n_losses).astype(np.float32), rng.uniform(0.5, 1.5, 1).astype(np.float32),
            rng.integers(0, n_losses, N).astype(np.int32), np.float32(1.0 / 3.0))


def mean_views_inputs(V, n):
    return np.random.default_rng(7000 + 31 * V + n).normal(0.0, 5.0, (V, n)).astype(np.float32)


# ============================================================================================ mining sweep
MINE_SCORE_SET = np.array([0.0, 0.01, np.nextafter(np.float32(0.05), np.float32(0)), 0.05, 0.05, 0.2, 0.2, 0.5, 0.9], np.float32)
MINE_THRESH, MINE_NMS, MINE_TOP_P = 0.05, 0.01, 0.10


def _nc(R, K, G, NR):
    return dict(R=R, K=K, G=G, NR=NR, id=f"R{R}-K{K}-G{G}-NR{NR}")


# the last case is beyond the R the other kernels see: the first power-of-two step at which the sort keys leave LDS
MINE_CASES = [
    _nc(1, 1, 1, 1), _nc(1, 20, 3, 4), _nc(9, 1, 1, 2), _nc(9, 20, 18, 1), _nc(9, 80, 5, 3), _nc(64, 20, 1, 4), _nc(64, 80, 18, 2),
    _nc(64, 1, 1, 1), _nc(65, 20, 7, 3), _nc(65, 80, 2, 1), _nc(1000, 1, 1, 4), _nc(1000, 20, 18, 2), _nc(1000, 20, 2, 1),
    _nc(1000, 80, 11, 3), _nc(4097, 20, 1, 1), _nc(4097, 20, 4, 4), _nc(4097, 80, 18, 2), _nc(4097, 20, 10, 3), _nc(4097, 1, 1, 2),
    _nc(16385, 20, 2, 2),
]


def mine_top_k(R):
    return max(int(R * MINE_TOP_P), 1)


def mine_form(R, top_k, G):
    """which launch form sw_oicr_mine_label takes (the size rules beside mine_staged_lds in heads.hip): 'staged' (keys and slot lists
    in LDS), 'lds' (keys in LDS, lists in the workspace) or 'ws' (keys in the workspace too)"""
    np2 = 64
    while np2 < max(R, top_k * G):
        np2 <<= 1
    if np2 * 8 + top_k * G * 25 + 16 <= 144 * 1024:
        return "staged"
    return "ws" if np2 * 8 + top_k * G > 144 * 1024 else "lds"


def mine_inputs(c):
    """-> scores (NR, R, K+1) f32 drawn from a small value set (exact ties, values at and one ulp below the threshold), boxes (R, 4) f32
    with duplicated rows (IoU exactly 1), gt classes (G,) distinct"""
    R, K, G, NR = c["R"], c["K"], c["G"], c["NR"]
    rng = np.random.default_rng(8000 + 17 * R + K + 5 * G + NR)
    scores = MINE_SCORE_SET[rng.integers(0, len(MINE_SCORE_SET), (NR, R, K + 1))]
    boxes = random_boxes(rng, R, size=600.0)
    if R > 1:
        dup = rng.integers(0, R, max(R // 8, 1))
        boxes[dup] = boxes[rng.integers(0, R, len(dup))]
    gt = np.sort(rng.choice(K, G, replace=False)).astype(np.int64)
    return scores, boxes, gt


# ============================================================================================ tolerance table
# (output kind, value regime) -> e32 = max over the cases of max|float32 restatement - float64| / max|float64|, measured by
# tests/test_heads_ref_cpu.py::test_tolerance_table_is_current (which fails when a bar this table gives is off a freshly computed one
# by more than a factor 2)
E32 = {
    ('finalize.out', 'all'): 1.08e-07,
    ('finalize.total', 'all'): 1.01e-07,
    ('mean_probs', 'sd3'): 1.66e-07,
    ('mean_probs', 'sd40'): 1.82e-07,
    ('mean_views', 'all'): 1.06e-07,
    ('predict.boxes', 'all'): 4.76e-07,
    ('predict.scores', 'all'): 2.46e-07,
    ('refine.dbox', 'sd2'): 4.49e-08,
    ('refine.dbox', 'sd40'): 4.57e-08,
    ('refine.dcls', 'sd2'): 2.01e-07,
    ('refine.dcls', 'sd40'): 2.19e-07,
    ('refine.loss_box', 'sd2'): 1.25e-07,
    ('refine.loss_box', 'sd40'): 1.62e-07,
    ('refine.loss_cls', 'sd2'): 1.30e-07,
    ('refine.loss_cls', 'sd40'): 1.55e-07,
    ('scale_cols.f32', 'all'): 8.82e-08,
    ('wsddn.grad', 'a'): 1.83e-06,
    ('wsddn.grad', 'a/R1'): 6.26e-07,
    ('wsddn.grad', 'b15'): 1.24e-05,
    ('wsddn.grad', 'b15/R1'): 2.02e-04,
    ('wsddn.grad', 'b40'): 4.48e-03,
    ('wsddn.grad', 'b40/R1'): 0.00e+00,
    ('wsddn.grad', 'c'): 1.76e-06,
    ('wsddn.grad', 'c/R1'): 1.30e-07,
    ('wsddn.grad', 'd'): 4.99e-07,
    ('wsddn.grad', 'e'): 4.06e-06,
    ('wsddn.loss', 'a'): 8.50e-07,
    ('wsddn.loss', 'a/R1'): 7.33e-08,
    ('wsddn.loss', 'b15'): 3.68e-07,
    ('wsddn.loss', 'b15/R1'): 1.48e-06,
    ('wsddn.loss', 'b40'): 7.14e-05,
    ('wsddn.loss', 'b40/R1'): 2.61e-08,
    ('wsddn.loss', 'c'): 1.03e-06,
    ('wsddn.loss', 'c/R1'): 1.20e-07,
    ('wsddn.loss', 'd'): 1.35e-07,
    ('wsddn.loss', 'e'): 1.25e-06,
    ('wsddn.mean', 'a'): 1.76e-06,
    ('wsddn.mean', 'a/R1'): 8.13e-08,
    ('wsddn.mean', 'b15'): 3.22e-07,
    ('wsddn.mean', 'b15/R1'): 2.72e-08,
    ('wsddn.mean', 'b40'): 1.37e-07,
    ('wsddn.mean', 'b40/R1'): 1.05e-09,
    ('wsddn.mean', 'c'): 6.16e-07,
    ('wsddn.mean', 'c/R1'): 2.76e-08,
    ('wsddn.mean', 'd'): 4.81e-07,
    ('wsddn.mean', 'e'): 8.29e-07,
    ('wsddn.scores', 'a'): 1.73e-06,
    ('wsddn.scores', 'a/R1'): 1.30e-07,
    ('wsddn.scores', 'b15'): 3.22e-07,
    ('wsddn.scores', 'b15/R1'): 2.72e-08,
    ('wsddn.scores', 'b40'): 1.07e-07,
    ('wsddn.scores', 'b40/R1'): 1.05e-09,
    ('wsddn.scores', 'c'): 6.24e-07,
    ('wsddn.scores', 'c/R1'): 2.16e-08,
    ('wsddn.scores', 'd'): 5.05e-07,
    ('wsddn.scores', 'e'): 7.88e-07,
}

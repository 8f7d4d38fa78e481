"""Stage-3 detector on gfx950 (BASELINE config #5): the ResNet-50-FPN Faster R-CNN that the
Unbiased-Teacher step trains — `TwoStagePseudoLabGeneralizedRCNN` (unbias/ubteacher/modeling/meta_arch/rcnn.py:8-107) over
`build_resnet_fpn_backbone` (detectron2/detectron2/modeling/backbone/{resnet,fpn}.py, second tree, v0.4), `PseudoLabRPN`
(unbias/ubteacher/modeling/proposal_generator/rpn.py over detectron2/.../proposal_generator/{rpn,proposal_utils}.py,
anchor_generator.py) and `StandardROIHeadsPseudoLab` with the focal classification loss (unbias/.../roi_heads/{roi_heads,
fast_rcnn}.py over detectron2/.../{poolers,roi_heads/box_head,roi_heads/fast_rcnn}.py).  Same module tree / state-dict names
as the reference model (backbone.bottom_up.res3.0.conv1.{weight,norm.*}, backbone.fpn_lateral2, proposal_generator.rpn_head.*,
roi_heads.box_head.fc1, roi_heads.box_predictor.{cls_score,bbox_pred}), same branch interface
(`forward(batched_inputs, branch=...)`), so semisup.SemiSupStep drives it like the reference's trainer drives its model.

Execution plan (MI355X-first): NHWC activations end to end; a 1x1 convolution is sw_gemm over the pixels (stride 2 = a pixel
subsample in front, STRIDE_IN_1X1), a 3x3 convolution the implicit-GEMM / direct MFMA kernel with bias + ReLU fused (stride 2 and
the box head's convolutions on ROI maps, the SoS-WSOD+ forms: sw_im2col3x3 + sw_gemm, _Conv3x3ColFn), FrozenBN is
folded into the weight and bias; the frozen stem + res2 run without autograd; ROIAlign, the FPN joins, the RPN losses, the focal
/ L1 losses, box decoding and NMS are kernels of csrc/detector.hip / heads.hip.  Every dense layer is a torch.autograd.Function
around those kernels with an explicit backward; autograd only links the nodes.  The index side — per-level top-k of the RPN,
anchor <-> ground-truth matching, the label sampling of RPN and ROI heads, FPN level assignment — is device code as well
(csrc/proposals.hip); one host read per RPN call (the proposal counts after NMS) remains, where the reference has a dozen.

Random sampling (detectron2/modeling/sampling.py:49-50 draws torch.randperm per candidate list): `sampler.next_seed()` supplies one
64-bit seed per list, the kernels give the candidate at position i of the list the key splitmix64(seed + i) >> 40 and the `num`
smallest keys win; tests inject the seeds of the closed-form keys the fixtures were generated with."""
import math
import os
from collections import OrderedDict
from typing import Dict, List

import torch
import torch.nn as nn

from . import ops, staging, wgrad
from .ops import _splitmix64
from .registry import META_ARCH_REGISTRY
from .structures import Boxes, Instances

R50_STAGES = [("res2", 3, 64, 256, 1), ("res3", 4, 128, 512, 2), ("res4", 6, 256, 1024, 2), ("res5", 3, 512, 2048, 2)]
FPN_STAGES = (2, 3, 4, 5)
STRIDES = (4, 8, 16, 32, 64)
SCALE_CLAMP = math.log(1000.0 / 16)
GT_LOGIT = math.log((1.0 - 1e-10) / (1 - (1.0 - 1e-10)))        # proposal_utils.py:170


# layer flags (the `relu` argument of _LinearFn / _Conv3x3Fn; True / False keep their meaning).  A ReLU mask in the backward pass is a
# kernel of its own (relu_bwd: read the output and the gradient, write the masked gradient) unless the PRODUCER of that gradient — the
# data-gradient kernel of the layer's only consumer — applies it in its epilogue:
#   _MASK_INPUT_GRAD  on the consumer: its input is a ReLU output nobody else reads; d/d(input) leaves the layer masked by input > 0;
#   _GRAD_PREMASKED   on the producer of that input: the gradient it receives is already masked, its own relu_bwd is skipped.
# The two are set in pairs by the module that owns both layers (bottleneck chain of a stage, RPN head, box head -> predictor).
_RELU, _MASK_INPUT_GRAD, _GRAD_PREMASKED = 1, 2, 4
FUSED_BLOCKS = True      # BottleneckBlock as one autograd node (_BottleneckFn); False: layer by layer (the form the fused one is tested against)


def _pad8(n):
    return (n + 7) // 8 * 8


class _Staged:
    """what one layer reads from the model's stage plan: w (+ wd: 3x3 data-gradient layout), scale / shift (FrozenBN) or packed bias"""
    __slots__ = ("w", "wd", "scale", "shift", "bias")

    def __init__(self, w=None, wd=None, scale=None, shift=None, bias=None):
        self.w, self.wd, self.scale, self.shift, self.bias = w, wd, scale, shift, bias


def _staged_of(module):
    st = module.__dict__.get("_st")
    if st is None:
        raise RuntimeError(f"{type(module).__name__}: no staged weights — the detector's layers run under TwoStagePseudoLabGeneralizedRCNN, "
                           "whose forward refreshes the stage plan (sw_stage_weights_multi)")
    return st


class WeightStage:
    """Compute-dtype copies of every weight of one detector, rewritten by ONE launch (ops.StagePlan / sw_stage_weights_multi) when a
    parameter or a FrozenBN buffer changed: optimizer step (version counters / staging.params_written), teacher EMA (params_written and
    buffers_written), load_state_dict.  Replaces, per layer and per forward call, the fold `weight * scale`, the dtype conversion
    and the layout change (and their autograd nodes: the layers' backward multiplies by `scale` itself)."""

    def __init__(self, model, compute_dtype):
        self.layers = [m for m in model.modules() if hasattr(m, "_stage_entries")]
        entries = []
        for m in self.layers:
            entries += m._stage_entries(compute_dtype)
        self.plan = ops.StagePlan(entries, compute_dtype)
        self.sources = []
        for e in entries:
            self.sources.append(e["w"])
            if e.get("bn") is not None:
                self.sources += list(e["bn"])
        self.key = None

    def valid_for(self, compute_dtype):
        return self.plan.dtype == compute_dtype and all(e[0].data_ptr() == p for e, p in zip(self.plan._keep, self.plan.ptrs))

    def refresh(self):
        key = (staging.epochs()[:2], tuple(t._version for t in self.sources))
        if key != self.key:
            self.plan.run()
            self.key = key


# ====================================================================================================== autograd nodes
def _pad_scale(scale, ld):
    """the FrozenBN scale (out,) as a row-scale vector of the padded (ld, in) weight gradient (pad rows: 1); out % 8 == 0 for every
    ConvBN of the ResNet, so this is the tensor itself"""
    if scale.shape[0] == ld:
        return scale
    return torch.cat([scale, torch.ones(ld - scale.shape[0], device=scale.device, dtype=scale.dtype)])


class _LinearFn(wgrad.CountedFunction):
    """y (P, out) = x (P, in) @ W_eff^T (+ bias) (ReLU): sw_gemm with the epilogue fused; explicit backward (dgrad, wgrad GEMMs, column
    sums).  `staged` (ld, in) is the compute-dtype copy of the effective weight (rows beyond `out` zero), written by the model's
    stage plan; `bias` f32 or None; `scale` (out,) f32 or None = the FrozenBN fold (W_eff = W * scale: dW = scale * dW_eff).
    `splits`: the row counts of the parameters packed into `staged`; `params`: those weight parameters in packing order, then their
    bias parameters if they have any — autograd routes the gradient pieces to them.  y compute dtype or f32 (out_f32).
    `residual` (P, out) or None: added before the ReLU inside the GEMM epilogue (the bottleneck's shortcut); its gradient is the
    masked output gradient."""

    @staticmethod
    def forward(ctx, x, staged, bias, scale, relu, out_f32, splits, residual, *params):
        P, D = x.shape
        out_f = sum(splits)
        cd = x.dtype
        ld = staged.shape[0]
        flags = int(relu)
        relu = bool(flags & _RELU)
        ydt = torch.float32 if out_f32 else cd
        assert not (relu and out_f32) and ld == (out_f + 7) // 8 * 8 and staged.dtype == cd
        ybuf = torch.empty(P, ld, device=x.device, dtype=ydt)
        if ld != out_f and P > 0:
            ops.fill_zero(ybuf)                                      # columns beyond out_f stay 0
        y = ybuf[:, :out_f]
        if P > 0:
            ops.gemm(x, staged, y, P, out_f, D, ep=ops.make_epilogue(bias=bias, relu=relu, out_dtype=ydt,
                                                                residual=None if residual is None else residual.detach()),
                     splitk=_few_tile_splits(P, out_f, D) if ld == out_f else 1, tag="s3_gemm_fwd")
            if ops.TIMER is not None:            # bench.py's roofline_stage3: algorithmic FLOP and bytes (operands once, result once) of this launch
                es = 2 if cd == torch.bfloat16 else 4
                ops.TIMER.note("s3_gemm_fwd", 2.0 * P * out_f * D)
                ops.TIMER.note("s3_gemm_fwd_bytes", float(es) * (P * D + out_f * D) + (4.0 if out_f32 else es) * P * out_f)
        ctx.save_for_backward(x, staged, ybuf if relu else None, scale)
        assert residual is None or (residual.shape == (P, out_f) and residual.dtype == ydt and residual.is_contiguous())
        ctx.relu, ctx.out_f, ctx.splits = relu, out_f, tuple(splits)
        ctx.mask_in, ctx.premasked = bool(flags & _MASK_INPUT_GRAD), bool(flags & _GRAD_PREMASKED)
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.wkey = id(params[0]) if params else None
        if params and any(ctx.needs_input_grad[8:8 + len(splits)]):
            wgrad.count_use(("lin", ctx.wkey))
        ctx.bkey = id(params[len(splits)]) if len(params) > len(splits) else None
        return y

    @staticmethod
    def backward(ctx, g):
        x, ws, ybuf, scale = ctx.saved_tensors
        P, D = x.shape
        out_f, ld, cd, nw = ctx.out_f, ws.shape[0], x.dtype, len(ctx.splits)
        need = ctx.needs_input_grad
        need_w = any(need[8:8 + nw]); need_b = any(need[8 + nw:])
        if ld == out_f:
            if ctx.relu and not ctx.premasked:
                gs = ops.relu_bwd(ybuf, g.contiguous(), out=torch.empty(P, ld, device=g.device, dtype=cd)) if P > 0 else g.contiguous()
            else:
                gs = g.contiguous() if g.dtype == cd else g.to(cd)
        else:
            gs = torch.empty(P, ld, device=g.device, dtype=cd)
            if P > 0:
                ops.fill_zero(gs)
                gs[:, :out_f] = g
                if ctx.relu:
                    ops.relu_bwd(ybuf, gs)                              # in place on the padded buffers (pad columns: 0 stays 0)
        dx = None
        if need[0]:
            dx = torch.empty(P, D, device=g.device, dtype=cd)
            if P > 0:
                ops.gemm(gs, ws, dx, P, D, ld, b_kstrided=True, ep=ops.make_epilogue(out_dtype=cd, relu_ref=x if ctx.mask_in else None),
                         splitk=_few_tile_splits(P, D, ld))
            else:
                dx.zero_()
        dws, dbs = [None] * nw, [None] * (len(ctx.shapes) - nw)
        if need_w:
            # K = pixels (10^4 .. 10^5 for a 1x1 convolution), M x N = a handful of 128x128 tiles: K-split slabs + ordered fold inside
            # sw_gemm (deterministic; unsplit, 4 workgroups walked 60 000 pixels).  FrozenBN: dW = scale * dW_eff, applied to the rows
            # inside the fold; `scale` covers the out_f real rows, the pad rows of dwp are never handed out.  None: added to the
            # buffer an earlier node of this backward pass returned, or queued for the last use of this weight (wgrad.join)
            rs = None if scale is None else _pad_scale(scale, ld)
            dwp = wgrad.join(("lin", ctx.wkey), ((gs, x),) if P > 0 else None, ((ld, D),), (rs,), g.device, wgrad.flush_wgrad_1x1)
            if dwp is wgrad.NOT_QUEUED:
                dwp = wgrad.wgrad_1x1(gs, x, rs, ctx.wkey) if P > 0 else torch.zeros(ld, D, device=g.device, dtype=torch.float32)
            elif dwp is not None:
                dwp = dwp[0]
            r0 = 0
            for i, n in enumerate(ctx.splits):
                if need[8 + i] and dwp is not None:
                    dws[i] = dwp[r0:r0 + n].view(ctx.shapes[i])
                r0 += n
        if need_b:
            dbp = wgrad.bias_grad(gs, ld, ctx.bkey)                          # (packed biases: one buffer, registered under the first one)
            r0 = 0
            for i, n in enumerate(ctx.splits):
                if i < len(dbs) and need[8 + nw + i] and dbp is not None:
                    dbs[i] = dbp[r0:r0 + n]
                r0 += n
        dres = (gs if ld == out_f else gs[:, :out_f].contiguous()) if need[7] else None       # d(residual) = the masked output gradient
        return (dx, None, None, None, None, None, None, dres) + tuple(dws) + tuple(dbs)


class _Conv3x3Fn(wgrad.CountedFunction):
    """3x3, stride 1, padding 1 on NHWC: sw_conv3x3_igemm (+ bias, ReLU fused) on the staged [co][tap][ci] copy of the effective
    weight; backward = weight gradient (split-K slabs, ordered fold; x FrozenBN scale), column sums, data gradient through the
    staged flipped-tap layout `staged_d` [ci][tap][co].  `w` / `b`: the parameters the gradients go to (b may be None)."""

    @staticmethod
    def forward(ctx, x, staged, staged_d, bias, scale, relu, w, b):
        n, H, W, cin = x.shape
        cout = w.shape[0]
        cd = x.dtype
        flags = int(relu)
        relu = bool(flags & _RELU)
        ctx.premasked = bool(flags & _GRAD_PREMASKED)
        out = torch.empty(n, H, W, cout, device=x.device, dtype=cd)
        ops.conv3x3(x, staged, out, 1, ops.make_epilogue(bias=bias, relu=relu, out_dtype=cd))
        ctx.save_for_backward(x, staged_d, out if relu else None, scale)
        ctx.relu, ctx.cout, ctx.wkey, ctx.bkey = relu, cout, id(w), (None if b is None else id(b))
        if ctx.needs_input_grad[6]:
            wgrad.count_use(id(w))
        return out

    @staticmethod
    def backward(ctx, g):
        x, wkd, out, scale = ctx.saved_tensors
        n, H, W, cin = x.shape
        cout = ctx.cout
        cd = x.dtype
        g = g.contiguous()
        dz = ops.relu_bwd(out, g, out=torch.empty_like(g)) if (ctx.relu and not ctx.premasked) else g
        dx = dw = db = None
        if ctx.needs_input_grad[6]:
            dw = wgrad.wgrad_3x3(x, dz, scale, ctx.wkey)
        if ctx.needs_input_grad[7]:
            db = wgrad.bias_grad(dz.view(n * H * W, cout), cout, ctx.bkey)
        if ctx.needs_input_grad[0]:
            dx = torch.empty(n, H, W, cin, device=g.device, dtype=cd)
            ops.conv3x3(dz, wkd, dx, 1, ops.make_epilogue(out_dtype=cd))
        return dx, None, None, None, None, None, dw, db


COL_CHUNK_BYTES = 256 << 20     # _Conv3x3ColFn: images (ROIs) per pass so that one column matrix stays at or below this


class _Conv3x3ColFn(wgrad.CountedFunction):
    """3x3, padding 1, stride 1 or 2 on NHWC through an explicit column matrix: sw_im2col3x3, then sw_gemm on the staged
    [co][tap][ci] weight viewed as (cout, 9 cin) with bias (FrozenBN shift) + ReLU in its epilogue.  For the layers the direct /
    implicit-GEMM kernels do not take: the stride-2 conv2 of a torchvision-style bottleneck (a quarter of the stride-1 FLOP, no
    subsample) and the box head's convolutions on (R, 7, 7, C) ROI maps.  Backward: data gradient = GEMM gs W into dcol, then
    sw_col2im3x3 (gather, no atomics; masks by the input when `_MASK_INPUT_GRAD`); weight gradient = the (1,1)-form GEMM gs^T col into
    one f32 [co][tap][ci] slab per pass, folded to OIHW x FrozenBN scale by sw_conv3x3_wgrad_fold (deterministic); the column matrix
    is rebuilt in the backward (a data-movement pass) instead of kept.  The images are walked in passes of COL_CHUNK_BYTES of columns.
    Inside wgrad.grad_scope a second use of the weight adds to the first use's buffer in the fold (pending_grad), like wgrad_3x3."""

    @staticmethod
    def _chunks(n, rows_per_img, cin, es):
        per = max(1, COL_CHUNK_BYTES // max(1, rows_per_img * 9 * cin * es))
        return [(i, min(n, i + per)) for i in range(0, n, per)]

    @staticmethod
    def forward(ctx, x, staged, bias, scale, relu, stride, w, b):
        n, H, W, cin = x.shape
        cout = w.shape[0]
        cd = x.dtype
        flags = int(relu)
        relu = bool(flags & _RELU)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        x = x.contiguous()
        out = torch.empty(n, Ho, Wo, cout, device=x.device, dtype=cd)
        w2 = staged.view(cout, 9 * cin)
        ep = ops.make_epilogue(bias=bias, relu=relu, out_dtype=cd)
        col = None
        for i0, i1 in _Conv3x3ColFn._chunks(n, Ho * Wo, cin, x.element_size()):
            rows = (i1 - i0) * Ho * Wo
            if col is None or col.shape[0] != rows:
                col = torch.empty(rows, 9 * cin, device=x.device, dtype=cd)
            ops.im2col3x3(x[i0:i1], col, stride)
            ops.gemm(col, w2, out[i0:i1].view(rows, cout), rows, cout, 9 * cin, ep=ep)
        ctx.save_for_backward(x, staged, out if relu else None, scale)
        ctx.relu, ctx.stride, ctx.cout = relu, stride, cout
        ctx.mask_in, ctx.premasked = bool(flags & _MASK_INPUT_GRAD), bool(flags & _GRAD_PREMASKED)
        ctx.wkey, ctx.bkey = id(w), (None if b is None else id(b))
        return out

    @staticmethod
    def backward(ctx, g):
        x, staged, out, scale = ctx.saved_tensors
        n, H, W, cin = x.shape
        cout, stride, cd = ctx.cout, ctx.stride, x.dtype
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        g = g.contiguous()
        if g.dtype != cd:
            g = g.to(cd)
        gs = ops.relu_bwd(out, g, out=torch.empty_like(g)) if (ctx.relu and not ctx.premasked and n > 0) else g
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[6], ctx.needs_input_grad[7]
        w2 = staged.view(cout, 9 * cin)
        dx = torch.empty_like(x) if need_x else None
        chunks = _Conv3x3ColFn._chunks(n, Ho * Wo, cin, x.element_size())
        slabs = torch.empty(max(1, len(chunks)), cout * 9 * cin, device=x.device, dtype=torch.float32) if need_w else None
        col = None
        for c, (i0, i1) in enumerate(chunks):
            rows = (i1 - i0) * Ho * Wo
            g2 = gs[i0:i1].view(rows, cout)
            if col is None or col.shape[0] != rows:
                col = torch.empty(rows, 9 * cin, device=x.device, dtype=cd)
            if need_w:
                ops.im2col3x3(x[i0:i1], col, stride)
                tiles = ((cout + 127) // 128) * ((9 * cin + 127) // 128)
                ops.gemm(g2, col, slabs[c].view(cout, 9 * cin), cout, 9 * cin, rows, a_kstrided=True, b_kstrided=True,
                         splitk=max(1, min(32, 512 // tiles, rows // 1024)))
            if need_x:
                ops.gemm(g2, w2, col, rows, 9 * cin, cout, b_kstrided=True, ep=ops.make_epilogue(out_dtype=cd))
                ops.col2im3x3(col, dx[i0:i1], stride, relu_ref=x[i0:i1] if ctx.mask_in else None)
        dw = db = None
        if need_w:
            prev = wgrad.pending_grad(ctx.wkey, (cout, cin, 3, 3))
            dw = prev if prev is not None else torch.empty(cout, cin, 3, 3, device=x.device, dtype=torch.float32)
            if chunks:
                ops.conv3x3_wgrad_fold(slabs, len(chunks), dw, cout_scale=scale, accumulate=prev is not None)
            elif prev is None:
                dw.zero_()
            if prev is not None:
                dw = None
            else:
                wgrad.note_grad(ctx.wkey, dw)
                dw = dw.view(cout, cin, 3, 3)
        if need_b:
            db = wgrad.bias_grad(gs.view(n * Ho * Wo, cout), cout, ctx.bkey)
        return dx, None, None, None, None, None, dw, db


def _few_tile_splits(P, N, K):
    """K-splits of a bf16 / f32 GEMM with an epilogue whose tile grid fills a fraction of the chip (res5's 1x1 convolutions, the box
    head's fc6 on 512-1024 ROIs): slabs + the epilogue in the fold (sw_gemm).  Measured (tools/probes/gemm_splitk_ep_probe.py): pays from
    K = 2048 on — K = 12544, 64 tiles: 103 -> 46 us; K = 2048, 32-64 tiles: 28 -> 22 us; K = 1024: 19 -> 22 us (not split)."""
    if K < 2048:
        return 1
    tiles = ((P + 127) // 128) * ((N + 127) // 128)
    return max(1, min(8, 256 // max(tiles, 1), K // 512))


def _view4(dw, cout, cin):
    return None if dw is None else dw.view(cout, cin, 1, 1)


class _BottleneckFn(wgrad.CountedFunction):
    """One bottleneck block (conv1 1x1 [stride s] -> ReLU -> conv2 3x3 -> ReLU -> conv3 1x1, + shortcut, ReLU) as ONE autograd node
    with an explicit backward.  Layer by layer (`_LinearFn` / `_Conv3x3Fn` nodes) every ReLU mask was a kernel of its own in front of
    the layer's gradients and autograd added the two gradients of the block input with a torch kernel; here the masks of conv1's and
    conv2's outputs run in the epilogue of the data-gradient kernel that produces the gradient (`relu_ref`), the shortcut branch's
    gradient is the `residual` of conv1's data-gradient GEMM, and a stride-2 block subsamples its input once for conv1 and the
    shortcut (one scatter in the backward).  Per block 2 mask kernels, 1 add (stride 2: + 1 subsample, 1 scatter, 1 add) fewer.
    Against the layer-by-layer form (tests/test_gpu_stage3.py): same losses; fp32 gradients equal up to the association of the
    three-term sums at the stage outputs (1e-6), bf16: the block-input gradient is rounded once instead of twice.
    args: x NHWC, `blk` the BottleneckBlock (staged operands, strides), then conv1/conv2/conv3[/shortcut] weights for autograd."""

    @staticmethod
    def forward(ctx, x, blk, *weights):
        """x (n, H, W, cin) -> (n, H', W', cout); or, blk = (block, maps): x (rows, cin) = the rows of SEVERAL maps [(n, H, W), ...] back
        to back (the student's passes in lockstep: every 1x1 convolution is one GEMM over all rows, the 3x3 one multi-problem launch)
        -> (rows', cout) in the same map order"""
        single = not isinstance(blk, tuple)
        if single:
            maps = [tuple(x.shape[:3])]
            cin = x.shape[3]
            x = x.reshape(-1, cin)
        else:
            blk, maps = blk
            maps = [tuple(m) for m in maps]
            cin = x.shape[1]
        c1, c2, c3, sc = blk.conv1, blk.conv2, blk.conv3, blk.shortcut
        s1, s2, s3 = _staged_of(c1), _staged_of(c2), _staged_of(c3)
        cd = x.dtype
        in_maps = maps
        if c1.stride == 2:
            maps = [(n, (H + 1) // 2, (W + 1) // 2) for n, H, W in in_maps]
            xs = torch.empty(sum(n * H * W for n, H, W in maps), cin, device=x.device, dtype=cd)
            r0 = q0 = 0
            for (n, H, W), (_, h, w) in zip(in_maps, maps):
                ops.subsample2x(x[r0:r0 + n * H * W].view(n, H, W, cin), xs[q0:q0 + n * h * w].view(n, h, w, cin))
                r0 += n * H * W; q0 += n * h * w
            x = xs
        P = x.shape[0]
        offs = [0]
        for n, H, W in maps:
            offs.append(offs[-1] + n * H * W)
        assert offs[-1] == P
        mid, cout = c1.weight.shape[0], c3.weight.shape[0]
        x2 = x

        def lin(a, st, relu, out_f, residual=None):
            y = torch.empty(P, out_f, device=a.device, dtype=cd)
            D = a.shape[1]
            ops.gemm(a, st.w, y, P, out_f, D, ep=ops.make_epilogue(bias=st.shift, relu=relu, out_dtype=cd, residual=residual),
                     splitk=_few_tile_splits(P, out_f, D), tag="s3_gemm_fwd")
            if ops.TIMER is not None:
                es = 2 if cd == torch.bfloat16 else 4
                ops.TIMER.note("s3_gemm_fwd", 2.0 * P * out_f * D)
                ops.TIMER.note("s3_gemm_fwd_bytes", float(es) * (P * D + out_f * D + P * out_f))
            return y
        h1 = lin(x2, s1, True, mid)
        h2 = torch.empty(P, mid, device=x.device, dtype=cd)
        ops.conv3x3_multi([(h1[offs[i]:offs[i + 1]].view(n, H, W, mid), s2.w, h2[offs[i]:offs[i + 1]].view(n, H, W, mid),
                            ops.make_epilogue(bias=s2.shift, relu=True, out_dtype=cd)) for i, (n, H, W) in enumerate(maps)])
        short = x2 if sc is None else lin(x2, _staged_of(sc), False, cout)
        out = lin(h2, s3, True, cout, residual=short)
        ctx.save_for_backward(x2, h1, h2, out, s1.w, s2.wd, s3.w, None if sc is None else _staged_of(sc).w,
                              s1.scale, s2.scale, s3.scale, None if sc is None else _staged_of(sc).scale)
        ctx.geom = (maps, in_maps, offs, cin, mid, cout, c1.stride, single)
        ctx.flags = (bool(blk.mask_input_grad) and c1.stride == 1, bool(blk.grad_premasked))
        ctx.keys = tuple(id(w) for w in weights) + (None,) * (4 - len(weights))
        if ctx.needs_input_grad[3]:
            for _ in maps:
                wgrad.count_use(id(weights[1]))                            # conv2: every map's weight gradient joins one grouped launch
        if all(ctx.needs_input_grad[2:]):
            wgrad.count_use(("1x1", id(weights[0])))                      # the block's 1x1 weights: one grouped launch for all passes
        n, H, W = maps[0]
        return out.view(n, H, W, cout) if single else out

    @staticmethod
    def backward(ctx, g):
        x2, h1, h2, out, w1, w2d, w3, wsc, sc1, sc2, sc3, scs = ctx.saved_tensors
        maps, in_maps, offs, cin, mid, cout, stride, single = ctx.geom
        P = offs[-1]
        cd = x2.dtype
        need = ctx.needs_input_grad                                   # (x, blk, w1, w2, w3[, wsc])
        mask_in, premasked = ctx.flags
        g2 = g.contiguous().view(P, cout)
        # (premasked: this block's output is read by the next block only, whose conv1 data gradient left masked by it)
        gs = g2 if premasked else ops.relu_bwd(out, g2, out=torch.empty(P, cout, device=g.device, dtype=cd))

        def dgrad(a, w, D, **ep):
            d = torch.empty(P, D, device=a.device, dtype=cd)
            K = a.shape[1]
            ops.gemm(a, w, d, P, D, K, b_kstrided=True, ep=ops.make_epilogue(out_dtype=cd, **ep), splitk=_few_tile_splits(P, D, K))
            return d

        def m4(t, i, c):                                              # map i of a row-concatenated (P, c) tensor as NHWC
            n, H, W = maps[i]
            return t[offs[i]:offs[i + 1]].view(n, H, W, c)
        keys = ctx.keys
        dh2 = dgrad(gs, w3, mid, relu_ref=h2)                         # masked by conv2's ReLU
        dw2 = None
        if need[3]:
            for i in range(len(maps)):
                r = wgrad.wgrad_3x3(m4(h1, i, mid), m4(dh2, i, mid), sc2, keys[1])
                dw2 = r if dw2 is None else dw2                       # (inside wgrad.grad_scope only the first use hands out a buffer)
                if r is not None and r is not dw2:
                    dw2 = dw2 + r                                     # outside a scope: plain sums
        dh1 = torch.empty(P, mid, device=g.device, dtype=cd)
        ops.conv3x3_multi([(m4(dh2, i, mid), w2d, m4(dh1, i, mid), ops.make_epilogue(out_dtype=cd, relu_ref=h1[offs[i]:offs[i + 1]]))
                           for i in range(len(maps))])                # masked by conv1's ReLU (reference as (pixels, mid) rows)
        dx = None
        if need[0]:
            side = gs if wsc is None else dgrad(gs, wsc, cin)         # the shortcut branch's gradient of the (subsampled) block input
            dx = dgrad(dh1, w1, cin, residual=side, **({"relu_ref": x2} if mask_in else {}))
            if stride == 2:
                full = torch.empty(sum(n * H * W for n, H, W in in_maps), cin, device=g.device, dtype=cd)
                r0 = 0
                for i, (n, H, W) in enumerate(in_maps):
                    ops.scatter2x(m4(dx, i, cin), full[r0:r0 + n * H * W].view(n, H, W, cin))
                    r0 += n * H * W
                dx = full
            if single:
                n, H, W = in_maps[0]
                dx = dx.view(n, H, W, cin)
        # ---- the 1x1 weight gradients: conv1 (dh1^T x), conv3 (gs^T h2), shortcut (gs^T x)
        # every pass's three problems are queued; the last use runs all of them as ONE grouped launch + ONE multi-fold (several maps
        # in one call: the rows of all of them are one problem per weight — still one grouped launch, so one counted use is enough)
        nw = 2 if wsc is None else 3
        dws = wgrad.NOT_QUEUED
        if all(need[2:]):
            dws = wgrad.join(("1x1", keys[0]), ((dh1, x2), (gs, h2), (gs, x2))[:nw], ((mid, cin, 1, 1), (cout, mid, 1, 1), (cout, cin, 1, 1))[:nw],
                             (sc1, sc3, scs)[:nw], g.device, wgrad.flush_wgrad_1x1, force=len(maps) > 1)
        if dws is wgrad.NOT_QUEUED:
            dw3 = _view4(wgrad.wgrad_1x1(gs, h2, sc3, keys[2]), cout, mid) if need[4] else None
            dw1 = _view4(wgrad.wgrad_1x1(dh1, x2, sc1, keys[0]), mid, cin) if need[2] else None
            dws = (dw1, dw3, _view4(wgrad.wgrad_1x1(gs, x2, scs, keys[3]), cout, cin) if nw == 3 and need[5] else None)
        elif dws is None:
            dws = (None,) * nw
        return (dx, None, dws[0], dw2, dws[1], *dws[2:nw])


class _Conv3x3LevelsFn(wgrad.CountedFunction):
    """L independent 3x3 convolutions (stride 1, padding 1, + bias, optional ReLU) of L maps as ONE launch each way (ops.conv3x3_multi:
    the FPN levels — the RPN head's shared convolution on p2..p6, the four FPN output convolutions).  args: L, flags (the `relu`
    argument of _Conv3x3Fn), then L inputs, L staged forward weights, L staged data-gradient weights, L bias values, L weight parameters,
    L bias parameters (a shared layer repeats its tensors).  Weight / bias gradients go through the same helpers as _Conv3x3Fn."""

    @staticmethod
    def forward(ctx, L, relu, *ts):
        xs, sws, swds, bvs, ws, bs = (ts[i * L:(i + 1) * L] for i in range(6))
        flags = int(relu)
        relu = bool(flags & _RELU)
        cd = xs[0].dtype
        outs, probs = [], []
        global _LEVELS_CAT
        cat, _LEVELS_CAT = _LEVELS_CAT, None          # (rows, cout) buffer the caller wants the L outputs in, maps back to back (RPN head)
        r0 = 0
        for x, sw, bv, w in zip(xs, sws, bvs, ws):
            n, H, W, _ = x.shape
            if cat is not None:
                out = cat[r0:r0 + n * H * W].view(n, H, W, w.shape[0]); r0 += n * H * W
            else:
                out = torch.empty(n, H, W, w.shape[0], device=x.device, dtype=cd)
            probs.append((x, sw, out, ops.make_epilogue(bias=bv, relu=relu, out_dtype=cd)))
            outs.append(out)
        ops.conv3x3_multi(probs)
        ctx.save_for_backward(*xs, *swds, *(outs if relu else ()))
        ctx.L, ctx.relu, ctx.premasked = L, relu, bool(flags & _GRAD_PREMASKED)
        ctx.wkeys, ctx.bkeys, ctx.couts = [id(w) for w in ws], [id(b) for b in bs], [int(w.shape[0]) for w in ws]
        need = ctx.needs_input_grad
        for i, w in enumerate(ws):
            if need[2 + 4 * L + i]:
                wgrad.count_use(id(w))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        L = ctx.L
        sv = ctx.saved_tensors
        xs, swds, outs = sv[:L], sv[L:2 * L], sv[2 * L:]
        need = ctx.needs_input_grad
        cd = xs[0].dtype
        dzs = []
        for i, g in enumerate(gs):
            if g is None:                                             # an output nobody used in the loss
                n, H, W, _ = xs[i].shape
                g = ops.fill_zero(torch.empty(n, H, W, ctx.couts[i], device=xs[i].device, dtype=cd))
            g = g.contiguous()
            dzs.append(ops.relu_bwd(outs[i], g, out=torch.empty_like(g)) if (ctx.relu and not ctx.premasked) else g)
        dxs, dws, dbs = [None] * L, [None] * L, [None] * L
        for i in range(L):
            n, H, W, _ = xs[i].shape
            cout = dzs[i].shape[3]
            if need[2 + 4 * L + i]:
                dws[i] = wgrad.wgrad_3x3(xs[i], dzs[i], None, ctx.wkeys[i])
            if need[2 + 5 * L + i]:
                dbs[i] = wgrad.bias_grad(dzs[i].view(n * H * W, cout), cout, ctx.bkeys[i])
        probs = []
        for i in range(L):
            if need[2 + i]:
                dxs[i] = torch.empty_like(xs[i])
                probs.append((dzs[i], swds[i], dxs[i], ops.make_epilogue(out_dtype=cd)))
        ops.conv3x3_multi(probs)
        return (None, None) + tuple(dxs) + (None,) * (3 * L) + tuple(dws) + tuple(dbs)


_LEVELS_CAT = None


def _conv3x3_levels(convs, xs, relu=False, cat=None):
    """the 3x3 `Conv` modules `convs[i]` applied to `xs[i]` (convs may repeat one module: a layer shared by the levels).  cat: a
    (sum of the maps' pixels, cout) buffer — the outputs are then row blocks of it, written there by the convolution itself"""
    global _LEVELS_CAT
    L = len(xs)
    sts = [_staged_of(c) for c in convs]
    _LEVELS_CAT = cat
    return _Conv3x3LevelsFn.apply(L, relu, *xs, *[st.w for st in sts], *[st.wd for st in sts], *[c.bias.detach() for c in convs],
                                  *[c.weight for c in convs], *[c.bias for c in convs])


class _Subsample2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, H, W, C = x.shape
        ctx.shape = tuple(x.shape)
        return ops.subsample2x(x, torch.empty(n, (H + 1) // 2, (W + 1) // 2, C, device=x.device, dtype=x.dtype))

    @staticmethod
    def backward(ctx, g):
        return ops.scatter2x(g.contiguous(), torch.empty(ctx.shape, device=g.device, dtype=g.dtype))


class _UpsampleAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lateral, top):
        ctx.top_shape = tuple(top.shape)
        return ops.upsample2x_add(lateral, top, torch.empty_like(lateral))

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return g, ops.downsample2x_sum(g, torch.empty(ctx.top_shape, device=g.device, dtype=g.dtype))


class _RoIAlignFn(torch.autograd.Function):
    """(rois (R,5), per-level row lists sel (4, R) + their DEVICE lengths, scales, *level features NHWC) -> pooled (R, C*7*7) in the
    reference's (C,7,7) order.  Every row belongs to exactly one level, so the four launches together write every row."""

    @staticmethod
    def forward(ctx, rois, sel, sel_cnt, scales, *feats):
        R = rois.shape[0]
        C = feats[0].shape[3]
        out = torch.empty(R, C * 49, device=feats[0].device, dtype=feats[0].dtype)
        if R:
            for l, (f, sc) in enumerate(zip(feats, scales)):
                ops.roi_align_fwd(f, rois, sel[l], out, sc, n_sel_dev=sel_cnt[l:l + 1])
        ctx.rois, ctx.sel, ctx.sel_cnt, ctx.scales = rois, sel, sel_cnt, scales
        ctx.shapes = [tuple(f.shape) for f in feats]
        ctx.dtype = feats[0].dtype
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        grads = []
        amax = None
        R = ctx.rois.shape[0]
        for l, (shp, sc, need) in enumerate(zip(ctx.shapes, ctx.scales, ctx.needs_input_grad[4:])):
            if not need:
                grads.append(None)
                continue
            if not R:
                grads.append(ops.fill_zero(torch.empty(shp, device=g.device, dtype=ctx.dtype)))
                continue
            # deterministic (round 6): 64-bit fixed-point accumulation, one conversion into the map's dtype (csrc/detector.hip
            # roi_align_bwd_fx_kernel) — a float-atomic accumulation left the iteration irreproducible in the last bits
            if amax is None:
                amax = ops.absmax(g)
            acc = ops.fill_zero(torch.empty(shp, device=g.device, dtype=torch.int64))
            ops.roi_align_bwd_fx(g, ctx.rois, ctx.sel[l], acc, sc, amax, n_sel_dev=ctx.sel_cnt[l:l + 1])
            grads.append(ops.fx_to_float(acc, amax, torch.empty(shp, device=g.device, dtype=ctx.dtype)))
        return (None, None, None, None) + tuple(grads)


class _RpnLossFn(torch.autograd.Function):
    """y (rows, 5A) = the RPN head's packed output; logits (N, At) / deltas (N, At, 4) = its anchor-order form (ops.rpn_unpack, computed
    once outside autograd: the proposal selection reads it too) -> (loss_rpn_cls, loss_rpn_loc): one kernel for both values and both
    unit gradients; the backward maps them back onto y's layout, times the two cotangents, in one kernel"""

    @staticmethod
    def forward(ctx, y, logits, deltas, labels_i8, anchors, matched, weights, inv_norm, meta):
        out = torch.empty(2, device=logits.device, dtype=torch.float32)
        dl = torch.empty_like(logits); dd = torch.empty_like(deltas)
        ops.rpn_loss(logits.reshape(-1), deltas.reshape(-1, 4), labels_i8, anchors, matched, weights, inv_norm, out, dl.reshape(-1),
                     dd.reshape(-1, 4))
        ctx.save_for_backward(dl, dd)
        ctx.meta = meta + (y.shape[0], y.shape[1], y.stride(0))
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cls, g_loc):
        dl, dd = ctx.saved_tensors
        N, A, hw, rows, cols, ld = ctx.meta
        dy = ops.rpn_unpack_bwd(dl, dd, N, A, hw, rows, ld, dl.device, g_logits=g_cls.contiguous(), g_deltas=g_loc.contiguous())
        return dy[:, :cols], None, None, None, None, None, None, None, None


class _RoiLossFn(torch.autograd.Function):
    """packed logits (R, >= 5K+1) f32 = [cls_score K+1 | bbox_pred 4K] -> (focal loss_cls, L1 loss_box_reg), both / R
    (unbias/ubteacher/modeling/roi_heads/fast_rcnn.py:73-105; detectron2/modeling/roi_heads/fast_rcnn.py:245-317).
    boxes2 (2R, 4) = the sampled proposal boxes followed by their matched gt boxes (row R + i is row i's target)."""

    @staticmethod
    def forward(ctx, logits, K, gt_classes_i32, boxes2, reg_weights, gamma):
        R = logits.shape[0]
        dev = logits.device
        c = _consts(dev, R)
        loss_cls = ops.fill_zero(torch.empty(1, device=dev))
        unit = ops.fill_zero(torch.empty_like(logits))
        lg = logits.detach()
        # box term through the refinement-loss kernel: targets boxes2[R + i], class-specific columns, L1 / R (CE weights 0); it writes the
        # box columns of `unit` (and zeros into the class columns, which the focal kernel then overwrites)
        lv = torch.empty(1, 2, 1, device=dev)
        ops.oicr_refine_loss(lg, 1, R, K, 0, K + 1, boxes2, gt_classes_i32.view(1, R), c["zero_w"].view(1, R), c["idx"].view(1, R),
                             c["zero_i"], reg_weights, lv, unit, c["ones2"])
        ops.focal_loss(lg[:, :K + 1], gt_classes_i32, gamma, loss_cls, unit[:, :K + 1])
        ctx.save_for_backward(unit)
        ctx.K = K
        return loss_cls[0], lv[0, 1, 0]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        (unit,) = ctx.saved_tensors
        K = ctx.K
        d = torch.empty_like(unit)
        ops.scale_col_blocks(unit, d, K + 1, g_cls.contiguous(), g_box.contiguous())
        return d, None, None, None, None, None


_CONSTS = {}


def _consts(dev, R):
    """small constant device tensors of the ROI loss (zero CE weights, target row indices R + i, ...), built once per (device, R)"""
    key = (str(dev), R)
    hit = _CONSTS.get(key)
    if hit is None:
        if len(_CONSTS) > 64:
            _CONSTS.clear()
        hit = _CONSTS[key] = dict(zero_w=torch.zeros(R, device=dev), idx=(torch.arange(R, device=dev, dtype=torch.int32) + R).contiguous(),
                                  zero_i=torch.zeros(1, dtype=torch.int32, device=dev), ones2=torch.ones(2, device=dev))
    return hit


# ====================================================================================================== modules
class FrozenBatchNorm2d(nn.Module):
    """layers/batch_norm.py:15-100: buffers only; folded into the convolution in front of it"""

    def __init__(self, c):
        super().__init__()
        self.register_buffer("weight", torch.ones(c)); self.register_buffer("bias", torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c)); self.register_buffer("running_var", torch.ones(c) - 1e-5)

    def fold(self):
        """(scale, shift) of y = x * scale + shift; cached: the statistics are frozen buffers (rebuilt when one of them was written,
        e.g. by load_state_dict or the teacher's EMA, which bump the tensors' version counters)"""
        key = (self.weight._version, self.bias._version, self.running_mean._version, self.running_var._version, self.weight.device,
               staging.epochs()[1])        # (buffer writes: the teacher EMA writes the buffers behind torch's version counters)
        hit = self.__dict__.get("_fold")
        if hit is None or hit[0] != key:
            scale = self.weight * torch.rsqrt(self.running_var + 1e-5)
            shift = self.bias - self.running_mean * scale
            if hit is not None and hit[1][0].device == scale.device and hit[1][0].shape == scale.shape:
                # the SAME two tensors for the module's lifetime, rewritten in place: a captured launch that read them (the no-grad
                # backbone graph of TwoStagePseudoLabGeneralizedRCNN._features) sees the new values
                hit[1][0].copy_(scale); hit[1][1].copy_(shift)
                hit = (key, hit[1])
            else:
                hit = (key, (scale.contiguous(), shift.contiguous()))
            self.__dict__["_fold"] = hit
        return hit[1]


class ConvBN(nn.Module):
    """Conv2d(bias=False, norm=FrozenBN) of the reference: parameter `weight` (OIHW) + submodule `norm`.  The FrozenBN fold lives in
    the staged weight (W * scale) and the epilogue bias (shift); d/dweight = scale * d/dW_eff in the layer's backward."""

    def __init__(self, cin, cout, k, stride=1, col=False):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")
        self.norm = FrozenBatchNorm2d(cout)
        self.k, self.stride = k, stride
        # a 3x3 convolution through the column matrix (_Conv3x3ColFn): every stride-2 one, and stride-1 ones on request (ROI maps)
        self.col = k == 3 and (col or stride == 2)
        assert k == 3 or not col

    def _stage_entries(self, cd):
        if self.k == 7:
            return []                                               # the stem kernel reads the f32 weight and the fold directly
        cout, cin = self.weight.shape[:2]
        dev = self.weight.device
        n = self.norm
        bn = (n.weight, n.bias, n.running_mean, n.running_var)
        st = _Staged(scale=torch.empty(cout, device=dev), shift=torch.empty(cout, device=dev))
        if self.k == 3:
            st.w = torch.empty(cout, 9, cin, device=dev, dtype=cd)
            ent = [dict(kind=1, w=self.weight, dst=st.w, bn=bn, scale=st.scale, shift=st.shift)]
            if self.weight.requires_grad and not self.col:           # (the column form's data gradient reads st.w itself)
                st.wd = torch.empty(cin, 9, cout, device=dev, dtype=cd)
                ent.append(dict(kind=2, w=self.weight, dst=st.wd, bn=bn))
        else:
            st.w = torch.zeros(_pad8(cout), cin, device=dev, dtype=cd)
            ent = [dict(kind=0, w=self.weight, dst=st.w, bn=bn, scale=st.scale, shift=st.shift)]
        self.__dict__["_st"] = st
        return ent

    def forward(self, x, relu, residual=None):
        st = _staged_of(self)
        if self.k == 3:
            assert residual is None
            if self.col:
                return _Conv3x3ColFn.apply(x, st.w, st.shift, st.scale, relu, self.stride, self.weight, None)
            return _Conv3x3Fn.apply(x, st.w, st.wd, st.shift, st.scale, relu, self.weight, None)
        if self.stride == 2:
            x = _Subsample2Fn.apply(x)
        n, H, W, C = x.shape
        cout = self.weight.shape[0]
        res = None if residual is None else residual.reshape(n * H * W, cout)
        y = _LinearFn.apply(x.reshape(n * H * W, C), st.w, st.shift, st.scale, relu, False, (cout,), res, self.weight)
        return y.reshape(n, H, W, cout)


class Conv(nn.Module):
    """plain Conv2d with bias (FPN laterals / outputs, RPN head).  packed=True: staged by the owner as part of a packed GEMM."""

    def __init__(self, cin, cout, k, packed=False, col=False):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k)); self.bias = nn.Parameter(torch.zeros(cout))
        nn.init.kaiming_uniform_(self.weight, a=1)
        self.k, self.packed, self.col = k, packed, bool(col) and k == 3          # col: through _Conv3x3ColFn (ROI maps)

    def _stage_entries(self, cd):
        if self.packed:
            return []
        cout, cin = self.weight.shape[:2]
        dev = self.weight.device
        st = _Staged()
        if self.k == 3 and self.col:
            st.w = torch.empty(cout, 9, cin, device=dev, dtype=cd)
            ent = [dict(kind=1, w=self.weight, dst=st.w)]
        elif self.k == 3:
            st.w = torch.empty(cout, 9, cin, device=dev, dtype=cd); st.wd = torch.empty(cin, 9, cout, device=dev, dtype=cd)
            ent = [dict(kind=1, w=self.weight, dst=st.w), dict(kind=2, w=self.weight, dst=st.wd)]
        else:
            st.w = torch.zeros(_pad8(cout), cin, device=dev, dtype=cd)
            ent = [dict(kind=0, w=self.weight, dst=st.w)]
        self.__dict__["_st"] = st
        return ent

    def forward(self, x, relu=False):
        """relu: False / True or layer flags (_RELU | _GRAD_PREMASKED ...)"""
        st = _staged_of(self)
        if self.k == 3 and self.col:
            return _Conv3x3ColFn.apply(x, st.w, self.bias.detach(), None, relu, 1, self.weight, self.bias)
        if self.k == 3:
            return _Conv3x3Fn.apply(x, st.w, st.wd, self.bias.detach(), None, relu, self.weight, self.bias)
        n, H, W, C = x.shape
        cout = self.weight.shape[0]
        y = _LinearFn.apply(x.reshape(n * H * W, C), st.w, self.bias.detach(), None, relu, False, (cout,), None, self.weight, self.bias)
        return y.reshape(n, H, W, cout)


def _packed_linear_entries(weights, biases, cd):
    """stage entries of several (out_i, in) weights stacked into one (pad8(sum out_i), in) GEMM operand + their biases in one f32 row"""
    rows = [w.shape[0] for w in weights]
    cin = weights[0].numel() // rows[0]
    dev = weights[0].device
    st = _Staged(w=torch.zeros(_pad8(sum(rows)), cin, device=dev, dtype=cd), bias=torch.zeros(_pad8(sum(rows)), device=dev))
    ent, r0 = [], 0
    for w, b, n in zip(weights, biases, rows):
        ent.append(dict(kind=0, w=w, dst=st.w[r0:r0 + n]))
        ent.append(dict(kind=3, w=b, dst=st.bias[r0:r0 + n]))
        r0 += n
    return st, ent


class BottleneckBlock(nn.Module):
    """backbone/resnet.py:100-213.  stride_in_1x1 (RESNETS.STRIDE_IN_1X1, the MSRA form): the stride sits in conv1 and in the shortcut;
    False (the torchvision form): conv1 runs at full resolution and the 3x3 conv2 carries the stride (resnet.py:146-166) — a
    stride-2 block of that form runs layer by layer, its conv2 through _Conv3x3ColFn; with stride 1 the two forms are one."""

    def __init__(self, cin, cout, mid, stride, stride_in_1x1=True):
        super().__init__()
        self.stride_in_3x3 = stride == 2 and not stride_in_1x1
        s1, s3 = (1, stride) if self.stride_in_3x3 else (stride, 1)
        self.shortcut = ConvBN(cin, cout, 1, stride) if cin != cout else None
        self.conv1 = ConvBN(cin, mid, 1, s1); self.conv2 = ConvBN(mid, mid, 3, s3); self.conv3 = ConvBN(mid, cout, 1)
        # set by the owner of a chain of blocks (ResNet): this block's input is the previous block's output and nobody else reads it /
        # this block's output is read by the next block only (see _MASK_INPUT_GRAD / _GRAD_PREMASKED; fused form only)
        self.mask_input_grad = self.grad_premasked = False

    def forward(self, x):
        if self.stride_in_3x3:
            # conv1's and conv2's ReLU outputs have one reader each (conv2 / conv3): that reader's data gradient leaves masked
            # (col2im / the GEMM epilogue), the producer skips its relu_bwd; the block output's mask follows the chain's flag
            sc = self.shortcut(x, False)
            h = self.conv1(x.contiguous(), _RELU | _GRAD_PREMASKED)
            h = self.conv2(h, _RELU | _MASK_INPUT_GRAD | _GRAD_PREMASKED)
            return self.conv3(h, _RELU | _MASK_INPUT_GRAD | (_GRAD_PREMASKED if self.grad_premasked else 0), residual=sc.contiguous())
        if FUSED_BLOCKS:
            ws = (self.conv1.weight, self.conv2.weight, self.conv3.weight) + (() if self.shortcut is None else (self.shortcut.weight,))
            return _BottleneckFn.apply(x.contiguous(), self, *ws)
        sc = self.shortcut(x, False) if self.shortcut is not None else x
        # out = relu(conv3(...) + shortcut): the add and the ReLU run in conv3's GEMM epilogue (the stand-alone add + ReLU kernel
        # was 45 launches / 1.1 ms of HBM traffic per Stage-3 iteration)
        return self.conv3(self.conv2(self.conv1(x, True), True), True, residual=sc.contiguous())


class BasicStem(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = ConvBN(3, 64, 7, 2)

    @staticmethod
    def out_hw(H, W):
        h2, w2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1

    def forward(self, x4, out=None):                                # (N, H, W, 4) normalised + padded -> (N, H/4, W/4, 64) [written to `out`]
        n, H, W, _ = x4.shape
        scale, shift = self.conv1.norm.fold()
        y = ops.stem_conv7x7(x4, self.conv1.weight.detach().contiguous(), scale.contiguous(), shift.contiguous(),
                             torch.empty(n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64, device=x4.device, dtype=x4.dtype))
        if out is None:
            out = torch.empty(n, (y.shape[1] - 1) // 2 + 1, (y.shape[2] - 1) // 2 + 1, 64, device=y.device, dtype=y.dtype)
        return ops.maxpool3x3s2(y, out)


class ResNet(nn.Module):
    def __init__(self, freeze_at=2, stride_in_1x1=True):
        super().__init__()
        self.stride_in_1x1 = bool(stride_in_1x1)
        self.stem = BasicStem()
        cin = 64
        self.stage_names = []
        for name, nblk, mid, cout, stride in R50_STAGES:
            blocks = [BottleneckBlock(cin if b == 0 else cout, cout, mid, stride if b == 0 else 1, stride_in_1x1) for b in range(nblk)]
            for b, blk in enumerate(blocks):         # inside a stage block b's output feeds block b + 1 and nothing else (the LAST
                blk.mask_input_grad = b > 0          # block's is the stage output: the next stage and an FPN lateral read it)
                blk.grad_premasked = b < nblk - 1
            self.add_module(name, nn.Sequential(*blocks))
            self.stage_names.append(name)
            cin = cout
        self.freeze_at = freeze_at
        if freeze_at >= 1:
            for p in self.stem.parameters():
                p.requires_grad = False
        for i, name in enumerate(self.stage_names, start=2):
            if freeze_at >= i:
                for p in getattr(self, name).parameters():
                    p.requires_grad = False

    def forward(self, x4):
        feats = {}
        with torch.no_grad():
            x = self.stem(x4)
        for i, name in enumerate(self.stage_names, start=2):
            if self.freeze_at >= i:
                with torch.no_grad():
                    x = getattr(self, name)(x)
            else:
                x = getattr(self, name)(x)
            feats[name] = x
        return feats

    def forward_lockstep(self, x4s):
        """several independent batches (different padded sizes allowed) through the residual stages IN LOCKSTEP: after the stem of
        every batch, the batches' rows sit back to back in one matrix, every 1x1 convolution of res2..res5 is ONE GEMM over all rows
        and every 3x3 convolution one multi-problem launch over the batches' maps (_BottleneckFn with several maps).
        Rows are independent in every layer, so each image's features are what forward() gives for its own batch.
        -> one feature dict per batch.  Needs the fused block form (so STRIDE_IN_1X1) and freeze_at == 2; anything else runs the
        batches one by one."""
        if not (FUSED_BLOCKS and self.stride_in_1x1 and self.freeze_at == 2 and len(x4s) > 1):
            return [self.forward(x) for x in x4s]
        feats = [{} for _ in x4s]
        # the stems' max-pools write their outputs back to back into ONE matrix: from there on — res2 included (round 5; it ran per batch
        # and its outputs were then copied together: 93 MB, 123 us) — every block is one pass over all batches' rows
        maps = [(int(x4.shape[0]),) + self.stem.out_hw(int(x4.shape[1]), int(x4.shape[2])) for x4 in x4s]
        joint = torch.empty(sum(n * H * W for n, H, W in maps), 64, device=x4s[0].device, dtype=x4s[0].dtype)
        r0 = 0
        with torch.no_grad():
            for x4, (n, H, W) in zip(x4s, maps):
                self.stem(x4, out=joint[r0:r0 + n * H * W].view(n, H, W, 64)); r0 += n * H * W
        for name in self.stage_names:
            for blk in getattr(self, name):
                ws = (blk.conv1.weight, blk.conv2.weight, blk.conv3.weight) + (() if blk.shortcut is None else (blk.shortcut.weight,))
                joint = _BottleneckFn.apply(joint, (blk, maps), *ws)
                if blk.conv1.stride == 2:
                    maps = [(n, (H + 1) // 2, (W + 1) // 2) for n, H, W in maps]
            for f, v in zip(feats, _SplitRowsFn.apply(joint, maps)):
                f[name] = v
        return feats


class FPN(nn.Module):
    """backbone/fpn.py:18-188: laterals 1x1, top-down nearest upsampling + add, outputs 3x3, p6 = p5 subsampled (LastLevelMaxPool)"""
    size_divisibility = 32

    def __init__(self, bottom_up, norm=""):
        """norm (FPN.NORM): "" = convolutions with bias; "FrozenBN" = bias-free convolutions followed by a FrozenBN (fpn.py:69-91)"""
        super().__init__()
        assert norm in ("", "FrozenBN"), f"MODEL.FPN.NORM = {norm!r} is not implemented by this detector (implemented: '', 'FrozenBN')"
        self.bottom_up, self.norm = bottom_up, norm
        for s, c in zip(FPN_STAGES, (256, 512, 1024, 2048)):
            if norm:
                self.add_module(f"fpn_lateral{s}", ConvBN(c, 256, 1)); self.add_module(f"fpn_output{s}", ConvBN(256, 256, 3))
            else:
                self.add_module(f"fpn_lateral{s}", Conv(c, 256, 1)); self.add_module(f"fpn_output{s}", Conv(256, 256, 3))

    def forward(self, x4):
        return self.forward_top(self.bottom_up(x4))

    def forward_top(self, c):
        """the pyramid from the bottom-up features {res2..res5}"""
        prevs, prev = [], None
        for s in reversed(FPN_STAGES):
            lat = getattr(self, f"fpn_lateral{s}")(c[f"res{s}"], False)
            prev = lat if prev is None else _UpsampleAddFn.apply(lat, prev)
            prevs.insert(0, prev)
        # the four output convolutions are independent once the top-down sums exist: one launch (each way)
        if self.norm:                   # (FrozenBN: the weight gradients carry the fold's scale — level by level through _Conv3x3Fn)
            outs = [getattr(self, f"fpn_output{s}")(p.contiguous(), False) for s, p in zip(FPN_STAGES, prevs)]
        else:
            outs = list(_conv3x3_levels([getattr(self, f"fpn_output{s}") for s in FPN_STAGES], [p.contiguous() for p in prevs]))
        outs.append(_Subsample2Fn.apply(outs[-1]))
        return outs                                                  # [p2, p3, p4, p5, p6] NHWC


class StandardRPNHead(nn.Module):
    def __init__(self, num_anchors=3):
        super().__init__()
        self.conv = Conv(256, 256, 3)
        self.objectness_logits = Conv(256, num_anchors, 1, packed=True); self.anchor_deltas = Conv(256, 4 * num_anchors, 1, packed=True)
        for m in (self.conv, self.objectness_logits, self.anchor_deltas):
            nn.init.normal_(m.weight, std=0.01)
        self.A = num_anchors

    def _stage_entries(self, cd):
        st, ent = _packed_linear_entries([self.objectness_logits.weight, self.anchor_deltas.weight],
                                         [self.objectness_logits.bias, self.anchor_deltas.bias], cd)
        self.__dict__["_st"] = st
        return ent

    def forward(self, feats):
        """-> (y (rows, 5A) f32, N, pixels per level): the two 1x1 convolutions of ALL levels as ONE GEMM of 5A (+ pad) columns over the
        concatenated pixels (row = level offset + image * Hi*Wi + pixel, columns [objectness a | delta 4a + b]); ops.rpn_unpack re-orders
        it into the reference's anchor order for the losses and the proposal selection"""
        A = self.A
        st = _staged_of(self)
        # (each conv output is read by the packed 1x1 GEMM only: that GEMM's data gradient leaves masked by the conv's ReLU)
        # the five conv outputs ARE the row blocks of the GEMM's operand: the convolution writes them there (the copy that packed them
        # was 34 + 84 + 34 us per iteration)
        N, C = feats[0].shape[0], self.conv.weight.shape[0]
        hw = [f.shape[1] * f.shape[2] for f in feats]
        rows = sum(N * v for v in hw)
        x = torch.empty(rows, C, device=feats[0].device, dtype=feats[0].dtype)
        ts = _conv3x3_levels([self.conv] * len(feats), [f.contiguous() for f in feats], relu=_RELU | _GRAD_PREMASKED, cat=x)
        y = _LinearFn.apply(_CatRowsFn.apply(x, *[t.reshape(N * v, C) for t, v in zip(ts, hw)]), st.w, st.bias, None, _MASK_INPUT_GRAD, True,
                            (A, 4 * A), None, self.objectness_logits.weight, self.anchor_deltas.weight, self.objectness_logits.bias,
                            self.anchor_deltas.bias)
        return y, N, tuple(hw)


class _CatRowsFn(torch.autograd.Function):
    """rows of several (r_i, C) matrices back to back in `buf` (one copy launch, sw_copy_multi); backward: row slices of the gradient"""

    @staticmethod
    def forward(ctx, buf, *parts):
        r0, pairs = 0, []
        for p in parts:
            dst = buf[r0:r0 + p.shape[0]]
            if not (p.is_contiguous() and p.data_ptr() == dst.data_ptr() and p.shape == dst.shape):      # (already written in place)
                pairs.append((p.contiguous(), dst))
            r0 += p.shape[0]
        if pairs:
            ops.copy_multi(pairs)
        ctx.rows = [p.shape[0] for p in parts]
        return buf

    @staticmethod
    def backward(ctx, g):
        out, r0 = [], 0
        for r in ctx.rows:
            out.append(g[r0:r0 + r]); r0 += r
        return (None,) + tuple(out)


class _SplitRowsFn(torch.autograd.Function):
    """(rows, C) holding several maps back to back -> one (n, H, W, C) view per map (no copy); backward: the maps' gradients copied
    back to back into one (rows, C) gradient (one sw_copy_multi launch; a map nobody used: zeros)"""

    @staticmethod
    def forward(ctx, buf, maps):
        ctx.maps, ctx.C = [tuple(m) for m in maps], buf.shape[1]
        out, r0 = [], 0
        for n, H, W in ctx.maps:
            out.append(buf[r0:r0 + n * H * W].view(n, H, W, ctx.C))
            r0 += n * H * W
        ctx.rows = r0
        return tuple(out)

    @staticmethod
    def backward(ctx, *gs):
        ref = next(g for g in gs if g is not None)
        full = torch.empty(ctx.rows, ctx.C, device=ref.device, dtype=ref.dtype)
        pairs, r0 = [], 0
        for (n, H, W), g in zip(ctx.maps, gs):
            dst = full[r0:r0 + n * H * W]
            if g is None:
                ops.fill_zero(dst)
            else:
                pairs.append((g.contiguous().view(n * H * W, ctx.C), dst))
            r0 += n * H * W
        ops.copy_multi(pairs)
        return full, None


class Sampler:
    """seeds of the label sampling (sampling.py:49-50 draws one torch.randperm per candidate list): one 64-bit seed per list; the
    kernels derive every candidate's random key from (seed, position in the list)"""

    def __init__(self, seed=0):
        self.seed, self.k = int(seed), 0

    def next_seed(self):
        self.k += 1
        return _splitmix64(((self.seed & 0xFFFFFFFF) << 32) ^ self.k)


class Speculation:
    """Counts the training path would otherwise read back from the device, ASSUMED and checked once per iteration.

    A semi-supervised iteration read eight counts back (per model call the proposals left by the RPN's NMS and its finite flags, per
    student batch the sampled rows, the teacher's detections, two pseudo-label counts): every read drains the queue and the GPU then
    idles until new launches arrive — 16.0 -> 14.2 ms with the reads stubbed out (and 13.1 with the teacher's pass beside the
    student's, which only pays once the reads are gone).  In training the first three kinds are constants in all but degenerate cases:
    the NMS leaves its cap (post_nms_topk) whenever the image has that many distinct candidates, the sampler fills its batch whenever
    there are that many proposals.  While a ledger is open (`with Speculation() as sp:` sets frcnn.SPECULATE) those sites assume the
    constant, keep the device tensor and go on — their padded rows are defined (zero boxes, class -1, score 0) so that a wrong
    assumption computes garbage, never touches memory it should not.  `sp.holds()` compares everything in ONE read (all ranks agree
    through a MAX all-reduce when a process group is up); the caller (semisup.SemiSupStep) then either steps the optimizer or throws
    the attempt away and repeats the iteration with the exact, reading code."""

    def __init__(self):
        self.items, self._prev = [], None

    def __enter__(self):
        global SPECULATE
        self._prev, SPECULATE = SPECULATE, self
        return self

    def __exit__(self, *exc):
        global SPECULATE
        SPECULATE = self._prev
        return False

    def expect(self, dev_ints, values):
        """dev_ints (int32, any shape) is assumed to equal `values` (flat list of ints)"""
        self.items.append((dev_ints.reshape(-1), [int(v) for v in values]))

    def seal(self):
        """Call when the forward pass is queued (every assumption is on the ledger, the backward is not yet issued): the comparison —
        and the ranks' agreement on it — runs on a stream of its own behind the forward only, its one flag lands in pinned host memory;
        holds() then waits for THAT, which has long happened while the backward still runs: the optimizer step is queued without the
        GPU ever draining.  (Read on the main stream instead, the flag waited for the whole backward: 0.5 ms of empty queue per iteration.)"""
        if not self.items or not self.items[0][0].is_cuda:
            return
        import torch.distributed as dist
        dev = self.items[0][0].device
        main = torch.cuda.current_stream(dev)
        chk = _CHECK_STREAMS.get(dev.index)
        if chk is None:
            chk = _CHECK_STREAMS[dev.index] = ops.worker_stream("chk", dev)
        chk.wait_stream(main)
        want_l = tuple(v for _, vs in self.items for v in vs)
        const = _CHECK_CONST.get(dev.index)
        if const is None or const[0] != want_l:                          # the expectation is the same list every iteration: uploaded once
            const = _CHECK_CONST[dev.index] = (want_l, torch.tensor(want_l, dtype=torch.int32).to(dev), torch.empty(1, dtype=torch.int32).pin_memory())
            torch.cuda.current_stream(dev).synchronize()
        want, host = const[1], const[2]
        with torch.cuda.stream(chk):
            got = torch.cat([t for t, _ in self.items]) if len(self.items) > 1 else self.items[0][0]
            flag = (got != want).any().to(torch.int32).reshape(1)
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and dist.get_backend() == "nccl":
                dist.all_reduce(flag, op=dist.ReduceOp.MAX)               # (RCCL waits for `chk`, the current stream, only)
                self._agreed = True
            host.copy_(flag, non_blocking=True)
            ev = torch.cuda.Event(); ev.record(chk)
        main.wait_stream(chk)                                             # (the ledger's tensors are not freed under the comparison)
        self._sealed = (ev, host, got, want, flag)

    def holds(self):
        import torch.distributed as dist
        sealed, agreed = getattr(self, "_sealed", None), getattr(self, "_agreed", False)
        if sealed is not None:
            sealed[0].synchronize()
            ok = int(sealed[1][0]) == 0
        elif not self.items:
            ok = True
        else:
            got = torch.cat([t for t, _ in self.items]) if len(self.items) > 1 else self.items[0][0]
            want = [v for _, vs in self.items for v in vs]
            ok = got.tolist() == want
        if not agreed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dev = self.items[0][0].device if (self.items and dist.get_backend() == "nccl") else "cpu"
            flag = torch.tensor([0 if ok else 1], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            ok = int(flag.item()) == 0
        return ok


SPECULATE = None
_CHECK_STREAMS = {}
_CHECK_CONST = {}


class PseudoLabRPN(nn.Module):
    """unbias/ubteacher/modeling/proposal_generator/rpn.py:11-57 over detectron2's RPN"""

    def __init__(self, sampler, batch_size_per_image=256, positive_fraction=0.25, pre_nms_topk=(2000, 1000), post_nms_topk=(1000, 1000),
                 nms_thresh=0.7, anchor_sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1.0, 2.0), box_loss_type="smooth_l1"):
        super().__init__()
        assert box_loss_type in ("smooth_l1", "smooth_l1_mean"), box_loss_type
        self.rpn_head = StandardRPNHead(len(aspect_ratios))
        self.box_loss_type = box_loss_type
        self.keep_loss_inputs = False                 # set by TwoStagePseudoLabGeneralizedRCNN.image_losses for its one forward
        self.sampler = sampler
        self.batch_size_per_image, self.positive_fraction = batch_size_per_image, positive_fraction
        self.pre_nms_topk, self.post_nms_topk, self.nms_thresh = pre_nms_topk, post_nms_topk, nms_thresh
        self.anchor_sizes, self.aspect_ratios = anchor_sizes, aspect_ratios
        self.bbox_weights = (1.0, 1.0, 1.0, 1.0)
        self._anchor_cache = {}

    def anchors(self, grid_sizes, device):
        """anchor_generator.py:17-31,134-199 (offset 0): per level (Hi*Wi*A, 4), location-major"""
        key = (tuple(grid_sizes), str(device))
        hit = self._anchor_cache.get(key)
        if hit is None:
            res = []
            for (gh, gw), stride, size in zip(grid_sizes, STRIDES, self.anchor_sizes):
                cell = []
                for r in self.aspect_ratios:
                    w = math.sqrt(size ** 2.0 / r); h = r * w
                    cell.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
                cell = torch.tensor(cell, dtype=torch.float32, device=device)
                sx = torch.arange(0, gw * stride, step=stride, dtype=torch.float32, device=device)
                sy = torch.arange(0, gh * stride, step=stride, dtype=torch.float32, device=device)
                yy, xx = torch.meshgrid(sy, sx, indexing="ij")
                shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), dim=1)
                res.append((shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4).contiguous())
            hit = self._anchor_cache[key] = (res, torch.cat(res, 0).contiguous())
        return hit

    @torch.no_grad()
    def label_and_sample_anchors(self, anchors_all, gt_boxes_list):
        """detectron2 rpn.py:305-360: IoU thresholds [0.3, 0.7], labels [0, -1, 1], low-quality matches; 256 per image, <= 25 % positive.
        One launch sequence for all images (sw_rpn_label_anchors): -> labels int8 (N, A), matched gt boxes (N, A, 4); no host sync"""
        counts = [int(g.shape[0]) for g in gt_boxes_list]
        gts = [g for g in gt_boxes_list if g.shape[0]]
        gt_cat = gts[0].contiguous() if len(gts) == 1 else (torch.cat(gts, 0).contiguous() if gts else None)
        seeds = [self.sampler.next_seed() for _ in range(2 * len(counts))]          # (positives, negatives) per image, in that order
        return ops.rpn_label_anchors(anchors_all, gt_cat, counts, seeds, self.batch_size_per_image,
                                     int(self.batch_size_per_image * self.positive_fraction))

    def _image_hw(self, image_sizes, device):
        # (a dict: one iteration of the semi-supervised step calls this with three different batches — a one-entry cache rebuilt the
        # tensor and copied it to the device every call)
        key = (tuple((int(h), int(w)) for h, w in image_sizes), str(device))
        cache = self.__dict__.setdefault("_hw_cache", {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 64:
                cache.clear()
            hit = cache[key] = torch.tensor([list(k) for k in key[0]], dtype=torch.int32).to(device)
        return hit

    @torch.no_grad()
    def predict_proposals(self, anchors, logits, deltas, image_sizes):
        """detectron2 rpn.py:478-533 + proposal_utils.py:20-130: per-level top-k (sort, stable: ties -> ascending index), decode, clip, drop
        empty boxes (sw_rpn_select_pack), NMS per level (sw_detect_postprocess with level = class), the best post_nms_topk per image.
        logits (N, At), deltas (N, At, 4) in anchor order.  ONE host read per call: the images' proposal counts and finite flags."""
        N = logits.shape[0]
        dev = logits.device
        pre, post = self.pre_nms_topk[0 if self.training else 1], self.post_nms_topk[0 if self.training else 1]
        L = len(anchors)
        ints = torch.empty(2 * N, device=dev, dtype=torch.int32)                          # proposal counts | finite flags
        sc, bx, _ = ops.rpn_select_pack(logits, deltas, anchors, pre, self.bbox_weights, SCALE_CLAMP, self._image_hw(image_sizes, dev),
                                        ints_out=ints[N:])
        spec = SPECULATE if self.training else None
        if spec is not None:                                             # rows beyond an image's count stay zero boxes (see Speculation)
            dboxes = torch.zeros(N, post, 4, device=dev); dscores = torch.zeros(N, post, device=dev)
        else:
            dboxes = torch.empty(N, post, 4, device=dev); dscores = torch.empty(N, post, device=dev)
        scratch = torch.empty(2, post, device=dev, dtype=torch.int32)
        for n, (h, w) in enumerate(image_sizes):
            ops.detect_postprocess(sc[n], bx[n], int(h), int(w), -3.0e38, self.nms_thresh, post,
                                   out=(ints[n:n + 1], dboxes[n], dscores[n], scratch[0], scratch[1]))
        if spec is not None:
            host = [post] * N + [-1] * N                                 # every image at the cap, everything finite (sw_rpn_select_pack
            spec.expect(ints, host)                                      # leaves the flag at 0xFFFFFFFF): checked by spec.holds()
        else:
            host = ints.tolist()
        out = []
        for n, (h, w) in enumerate(image_sizes):
            k, fin = host[n], host[N + n]
            if self.training and not fin:
                raise FloatingPointError("Predicted boxes or scores contain Inf/NaN. Training has diverged.")
            p = Instances((int(h), int(w)))
            p.proposal_boxes = Boxes(dboxes[n, :k]); p.objectness_logits = dscores[n, :k]
            p._sw_src = (dboxes, ints, n, k)              # the (N, post, 4) block + device counts: the ROI heads sample from it directly
            out.append(p)
        return out

    def forward(self, image_sizes, feats, gt_instances=None, compute_loss=True, compute_val_loss=False):
        dev = feats[0].device
        anchors, anchors_all = self.anchors([tuple(f.shape[1:3]) for f in feats], dev)
        y, N, hw = self.rpn_head(feats)
        A = self.rpn_head.A
        logits, deltas = ops.rpn_unpack(y.detach(), N, A, hw)                              # (N, At), (N, At, 4), anchor order
        losses = {}
        if (self.training and compute_loss) or compute_val_loss:
            mean = self.box_loss_type == "smooth_l1_mean"
            if mean and torch.is_grad_enabled() and y.requires_grad:
                raise NotImplementedError("MODEL.RPN.BBOX_REG_LOSS_TYPE = 'smooth_l1_mean' is implemented for loss evaluation only "
                                          "(no gradient): run the forward under torch.no_grad()")
            labels, matched = self.label_and_sample_anchors(anchors_all, [g.gt_boxes.tensor.to(dev).float() for g in gt_instances])
            l_cls, l_loc = _RpnLossFn.apply(y, logits, deltas, labels.reshape(-1), anchors_all, matched.reshape(-1, 4), self.bbox_weights,
                                            1.0 / (self.batch_size_per_image * N), (N, A, hw))
            if mean:                  # box_regression.py:261-268: the mean over the (foreground anchors x 4) elements; 0 / 0 = NaN
                l_loc = l_loc / (4 * (labels == 1).sum()).to(l_loc.dtype)
            if self.keep_loss_inputs:
                self.last_loss_inputs = (logits, deltas, labels, matched, anchors_all)
            losses = {"loss_rpn_cls": l_cls, "loss_rpn_loc": l_loc}
            self.last_labels = labels
        proposals = self.predict_proposals(anchors, logits, deltas, image_sizes)
        return proposals, losses


class FastRCNNConvFCHead(nn.Module):
    """detectron2/modeling/roi_heads/box_head.py:25-117: `conv_dims` 3x3 convolutions (+ conv_norm "" / "FrozenBN", ReLU) on the
    (R, C, 7, 7) ROI maps, flatten, then `fc_dims` linear layers + ReLU (ROI_BOX_HEAD.NUM_CONV / CONV_DIM / NUM_FC / FC_DIM / NORM).
    The defaults are the 2-fc head of Base-RCNN-FPN.yaml; SoS-WSOD+ (sos_plus_test.yaml) runs 4 conv + 1 fc with FrozenBN.  The
    convolutions run on NHWC (R, 7, 7, C) maps through _Conv3x3ColFn (which walks the ROIs in passes of COL_CHUNK_BYTES of columns);
    the pooler's rows and fc1's weight stay in the reference's (C, 7, 7) order, so the rows are re-laid on the way in and out."""

    def __init__(self, conv_dims=(), fc_dims=(1024, 1024), conv_norm="", in_channels=256, resolution=7):
        super().__init__()
        assert conv_norm in ("", "FrozenBN"), \
            f"MODEL.ROI_BOX_HEAD.NORM = {conv_norm!r} is not implemented by this detector (implemented: '', 'FrozenBN')"
        assert len(conv_dims) + len(fc_dims) > 0 and all(c % 8 == 0 for c in tuple(conv_dims) + (in_channels,))
        self.resolution, self.in_channels = resolution, in_channels
        self.convs, self.fcs = [], []
        c = in_channels
        for k, d in enumerate(conv_dims, start=1):
            m = ConvBN(c, d, 3, col=True) if conv_norm else Conv(c, d, 3, col=True)
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")          # c2_msra_fill
            self.add_module(f"conv{k}", m); self.convs.append(m)
            c = d
        d_in = c * resolution * resolution
        for k, d in enumerate(fc_dims, start=1):
            m = nn.Linear(d_in, d)
            nn.init.kaiming_uniform_(m.weight, a=1); nn.init.constant_(m.bias, 0)
            self.add_module(f"fc{k}", m); self.fcs.append(m)
            d_in = d
        self.out_features = d_in

    def _stage_entries(self, cd):
        st = []
        ent = []
        for m in self.fcs:
            o, i = m.weight.shape
            st.append(_Staged(w=torch.zeros(_pad8(o), i, device=m.weight.device, dtype=cd)))
            ent.append(dict(kind=0, w=m.weight, dst=st[-1].w))
        self.__dict__["_st"] = st
        return ent

    def forward(self, x, out_grad_premasked=False):
        """x (R, C * 7 * 7) in (C, 7, 7) order.  out_grad_premasked: the caller's only consumer of the result masks its data
        gradient by result > 0 (_MASK_INPUT_GRAD)"""
        sts = _staged_of(self)
        R = x.shape[0]
        last = len(self.convs) + len(self.fcs) - 1
        if self.convs:
            P = self.resolution
            x = x.view(R, self.in_channels, P * P).permute(0, 2, 1).contiguous().view(R, P, P, self.in_channels)
            for k, m in enumerate(self.convs):
                # conv k > 0 reads a ReLU output nobody else reads: its col2im masks, its producer skips relu_bwd
                f = _RELU | (_MASK_INPUT_GRAD if k > 0 else 0) | (_GRAD_PREMASKED if (k < len(self.convs) - 1 or (k == last and out_grad_premasked)) else 0)
                x = m(x, f)
            x = x.view(R, P * P, x.shape[3]).permute(0, 2, 1).reshape(R, P * P * x.shape[3])
            if not self.fcs:
                return x
        for k, (m, st) in enumerate(zip(self.fcs, sts)):
            i = len(self.convs) + k
            # (the 2-fc head: fc1 _RELU | _GRAD_PREMASKED, fc2 _RELU | _MASK_INPUT_GRAD [| _GRAD_PREMASKED]; behind convolutions the
            # rows were re-laid by a copy, so fc1 does not mask its input gradient and the last convolution masks its own output's)
            f = _RELU | (_MASK_INPUT_GRAD if k > 0 else 0) | (_GRAD_PREMASKED if (k < len(self.fcs) - 1 or (i == last and out_grad_premasked)) else 0)
            x = _LinearFn.apply(x, st.w, m.bias.detach(), None, f, False, (m.out_features,), None, m.weight, m.bias)
        return x


class FastRCNNFocaltLossOutputLayers(nn.Module):
    """unbias/ubteacher/modeling/roi_heads/fast_rcnn.py:12-40 over detectron2's FastRCNNOutputLayers"""

    def __init__(self, d_in, num_classes, test_score_thresh=0.05, test_nms_thresh=0.5, test_topk_per_image=100):
        super().__init__()
        self.cls_score = nn.Linear(d_in, num_classes + 1); self.bbox_pred = nn.Linear(d_in, 4 * num_classes)
        nn.init.normal_(self.cls_score.weight, std=0.01); nn.init.normal_(self.bbox_pred.weight, std=0.001)
        nn.init.constant_(self.cls_score.bias, 0); nn.init.constant_(self.bbox_pred.bias, 0)
        self.num_classes = num_classes
        self.bbox_weights = (10.0, 10.0, 5.0, 5.0)
        self.test_score_thresh, self.test_nms_thresh, self.test_topk_per_image = test_score_thresh, test_nms_thresh, test_topk_per_image

    def _stage_entries(self, cd):
        st, ent = _packed_linear_entries([self.cls_score.weight, self.bbox_pred.weight], [self.cls_score.bias, self.bbox_pred.bias], cd)
        self.__dict__["_st"] = st
        return ent

    def forward(self, x, mask_input_grad=False):
        """-> packed f32 logits (R, 5K+1) = [cls_score | bbox_pred]: one GEMM.  mask_input_grad: x is a ReLU output that only this layer
        reads (the box head's): d/dx leaves masked by x > 0"""
        st = _staged_of(self)
        K = self.num_classes
        return _LinearFn.apply(x, st.w, st.bias, None, _MASK_INPUT_GRAD if mask_input_grad else 0, True, (K + 1, 4 * K), None, self.cls_score.weight, self.bbox_pred.weight,
                               self.cls_score.bias, self.bbox_pred.bias)


class PaddedDetections:
    """A (V, T) block for the inference form of StandardROIHeadsPseudoLab with `padded_detections` set to it: image after image the
    heads' detections land in row v = 0, 1, ... (boxes (V, T, 4), scores (V, T), classes (V, T) int32, device counts (V,) int32) — the
    input layout of ops.tta_merge, filled without a copy.  Rows beyond a count stay zero."""

    def __init__(self, V, T, device):
        self.boxes = torch.zeros(V, T, 4, device=device); self.scores = torch.zeros(V, T, device=device)
        self.classes = torch.zeros(V, T, dtype=torch.int32, device=device)
        self.counts = torch.zeros(V, dtype=torch.int32, device=device)
        self._rows = torch.empty(T, dtype=torch.int32, device=device)           # proposal indices: not kept
        self.filled = 0

    def next_out(self):
        v = self.filled
        if v >= self.counts.shape[0]:
            raise IndexError("PaddedDetections: more images than rows")
        self.filled += 1
        return self.counts[v:v + 1], self.boxes[v], self.scores[v], self.classes[v], self._rows


class StandardROIHeadsPseudoLab(nn.Module):
    """unbias/ubteacher/modeling/roi_heads/roi_heads.py:377-546"""

    def __init__(self, num_classes, sampler, batch_size_per_image=512, positive_fraction=0.25, proposal_append_gt=True, loss="FocalLoss",
                 box_loss_type="smooth_l1", box_head=None):
        super().__init__()
        # ROI_HEADS.LOSS (roi_heads.py:106-113, 405-406): "FocalLoss" (gamma 1.5) or detectron2's "CrossEntropy" (mean softmax CE
        # over the sampled rows) — the focal kernel with gamma 0 is that CE: (1 - p)^0 = 1, and its gradient term in gamma vanishes
        assert loss in ("FocalLoss", "CrossEntropy"), loss
        assert box_loss_type in ("smooth_l1", "smooth_l1_mean"), box_loss_type
        self.loss, self.gamma = loss, (1.5 if loss == "FocalLoss" else 0.0)
        self.box_loss_type = box_loss_type
        self.keep_loss_inputs = False                 # set by TwoStagePseudoLabGeneralizedRCNN.image_losses for its one forward
        self.padded_detections = False                # True / a PaddedDetections block: set and restored by tta.GeneralizedRCNNWithTTA
        self.box_head = FastRCNNConvFCHead(**(box_head or {}))
        self.box_predictor = FastRCNNFocaltLossOutputLayers(self.box_head.out_features, num_classes)
        self.num_classes, self.sampler = num_classes, sampler
        self.batch_size_per_image, self.positive_fraction, self.proposal_append_gt = batch_size_per_image, positive_fraction, proposal_append_gt

    @torch.no_grad()
    def label_and_sample_proposals(self, proposals, targets, append_gt):
        """roi_heads.py:324-375 for all images in ONE launch (sw_roi_label_sample): append the gt boxes, IoU-match at 0.5 (labels [0, 1], no
        low-quality matches), sample batch_size_per_image rows with at most positive_fraction foreground by the random-key rule; no host
        round trip (the proposal counts are read on the device where the RPN's NMS left them)"""
        K, B = self.num_classes, self.batch_size_per_image
        N = len(proposals)
        dev = proposals[0].proposal_boxes.tensor.device
        src = [getattr(p, "_sw_src", None) for p in proposals]
        if all(s_ is not None for s_ in src) and all(s_[0] is src[0][0] and s_[2] == i for i, s_ in enumerate(src)) and src[0][0].shape[0] == N:
            buf, cnt_dev = src[0][0], src[0][1][:N]
        else:                                                     # proposals from somewhere else: pack them into one block
            ps = max(max(len(p) for p in proposals), 1)
            buf = torch.empty(N, ps, 4, device=dev)
            pairs = [(p.proposal_boxes.tensor.float().contiguous(), buf[i, :len(p)]) for i, p in enumerate(proposals) if len(p)]
            if pairs:
                ops.copy_multi(pairs)
            cnt_dev = torch.tensor([len(p) for p in proposals], dtype=torch.int32).to(dev)
        counts = [len(t) for t in targets]
        gts = [(t.gt_boxes.tensor.to(dev).float(), t.gt_classes.to(dev)) for t in targets if len(t)]
        if gts:
            gt_b = gts[0][0].contiguous() if len(gts) == 1 else torch.cat([g[0] for g in gts], 0).contiguous()
            gt_c = (gts[0][1] if len(gts) == 1 else torch.cat([g[1] for g in gts], 0)).to(torch.int32).contiguous()
        else:
            gt_b = gt_c = None
        seeds = [self.sampler.next_seed() for _ in range(2 * N)]                            # (foreground, background) per image
        cnt, idx, cls, both = ops.roi_label_sample(cnt_dev, buf, gt_b, gt_c, counts, seeds, append_gt, 0.5, K, B, int(B * self.positive_fraction))
        # Rows per image = num_pos + num_neg of sampling.py:36-47 = min(n_pos, max_pos) + min(n_neg, B - num_pos): LESS than min(B, candidates)
        # when an image has more than max_pos foreground candidates and fewer than B - max_pos background ones (200 fg + 100 bg -> 228,
        # not 300).  Only the kernel knows n_pos, so its count is read (one host read per call; the rows beyond it are class -1 / empty
        # boxes, never stale memory).  Without ground truth every candidate is background: the count is min(B, candidates), no read.
        need = [i for i in range(N) if counts[i] > 0]
        if SPECULATE is not None and self.training and all(len(p) >= B for p in proposals):
            got = [B] * N                                                # full batches (padded rows: class -1, zero boxes): checked later
            SPECULATE.expect(cnt, got)
        else:
            got = cnt.tolist() if need else None
        if self.keep_loss_inputs:
            self.last_counts = cnt                   # each image's sampled-row count, on the device (min(B, candidates) without gt)
        out = []
        for i, p in enumerate(proposals):
            n = int(got[i]) if got is not None else min(B, len(p))
            s_ = Instances(p.image_size)
            s_.proposal_boxes = Boxes(both[0, i, :n]); s_.gt_classes = cls[i, :n]; s_.gt_boxes = Boxes(both[1, i, :n])
            s_._sw_dense = (both, cls, i, n)
            out.append(s_)
        return out

    def _pool(self, feats, boxes_per_image):
        """poolers.py:17-50,196-250: level = floor(4 + log2(sqrt(area) / 224 + 1e-8)) clamped to [2, 5]; ROIAlign 7x7 per level.  The dense
        (image, box) rows, the levels and the per-level row lists come from one kernel (sw_roi_assign_levels), the list lengths stay on the
        device (sw_roi_align_* read them): no host round trip"""
        bs = [b if (b.dtype == torch.float32 and b.dim() == 2 and (b.shape[0] == 0 or (b.stride(1) == 1 and b.stride(0) == 4))) else
              b.float().contiguous() for b in boxes_per_image]
        base = min((b for b in bs if b.shape[0]), key=lambda t: t.data_ptr(), default=bs[0])
        rois, lv, sel, cnt = ops.roi_assign_levels(base, [b.shape[0] for b in bs], [(b.data_ptr() - base.data_ptr()) // 4 for b in bs])
        self.last_levels = lv
        return _RoIAlignFn.apply(rois, sel, cnt, [1.0 / s for s in STRIDES[:4]], *feats[:4])

    def forward(self, feats, proposals, targets=None, compute_loss=True, branch="", compute_val_loss=False):
        if self.training and compute_loss:
            proposals = self.label_and_sample_proposals(proposals, targets, self.proposal_append_gt)
        elif compute_val_loss:
            proposals = self.label_and_sample_proposals(proposals, targets, False)
        pooled = self._pool(feats, [p.proposal_boxes.tensor for p in proposals])
        logits = self.box_predictor(self.box_head(pooled, out_grad_premasked=True), mask_input_grad=True)
        K = self.num_classes
        if (self.training and compute_loss) or compute_val_loss:
            self.last_sampled, self.last_logits = proposals, logits
            mean = self.box_loss_type == "smooth_l1_mean"
            if mean and torch.is_grad_enabled() and logits.requires_grad:
                raise NotImplementedError("MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = 'smooth_l1_mean' is implemented for loss evaluation "
                                          "only (no gradient): run the forward under torch.no_grad()")
            R = logits.shape[0]
            if R == 0:
                z = 0.0 * logits.sum()
                if self.keep_loss_inputs:
                    self.last_loss_inputs = (logits, torch.empty(0, dtype=torch.int32, device=logits.device),
                                             torch.empty(0, 4, device=logits.device),
                                             torch.zeros(len(proposals), dtype=torch.int32, device=logits.device))
                return proposals, {"loss_cls": z, "loss_box_reg": z / 0.0 if mean else z}
            dense = [getattr(p, "_sw_dense", None) for p in proposals]
            B = self.batch_size_per_image
            if all(d is not None and d[0] is dense[0][0] and d[3] == B for d in dense) and dense[0][0].shape[1] == len(proposals):
                both, cls = dense[0][0], dense[0][1]             # every image sampled a full batch: the sampler's blocks ARE the dense rows
                boxes2, gtc = both.view(2 * R, 4), cls.view(R)
            else:
                boxes2 = torch.cat([p.proposal_boxes.tensor for p in proposals] + [p.gt_boxes.tensor for p in proposals]).contiguous()
                gtc = torch.cat([p.gt_classes for p in proposals]).to(torch.int32).contiguous()
            l_cls, l_box = _RoiLossFn.apply(logits, K, gtc, boxes2, self.box_predictor.bbox_weights, self.gamma)
            if mean:                  # fast_rcnn.py:534-564: the mean over the (foreground rows x 4) elements, not / R; 0 / 0 = NaN
                l_box = l_box * R / (4 * ((gtc >= 0) & (gtc < K)).sum()).to(l_box.dtype)
            if self.keep_loss_inputs:
                self.last_loss_inputs = (logits, gtc, boxes2, self.last_counts)
            return proposals, {"loss_cls": l_cls, "loss_box_reg": l_box}
        # inference form (fast_rcnn.py:44-160): softmax, decode, clip, score > 0.05, per-class NMS 0.5, top 100
        pred, off = [], 0
        lg = logits.detach()
        bp = self.box_predictor
        for p in proposals:
            n = len(p)
            h, w = p.image_size
            sc = torch.empty(n, K + 1, device=lg.device); bx = torch.empty(n, 4 * K, device=lg.device)
            r = Instances((h, w))
            pad = self.padded_detections
            if pad is not False:
                # all topk rows and the DEVICE count, no read-back (tta.GeneralizedRCNNWithTTA: the rows beyond the count are zero, the
                # merge kernel never looks at them); a PaddedDetections block receives the rows in place, image after image
                out = None if pad is True else pad.next_out()
                if n:
                    ops.oicr_predict(lg[off:off + n], n, K, 1, 0, 5 * K + 1, p.proposal_boxes.tensor.float().contiguous(), bp.bbox_weights,
                                     SCALE_CLAMP, sc, bx)
                    out = ops.detect_postprocess(sc, bx, int(h), int(w), bp.test_score_thresh, bp.test_nms_thresh, bp.test_topk_per_image, out=out)
                elif out is None:
                    T = bp.test_topk_per_image
                    out = (torch.zeros(1, dtype=torch.int32, device=lg.device), torch.zeros(T, 4, device=lg.device), torch.zeros(T, device=lg.device),
                           torch.zeros(T, dtype=torch.int32, device=lg.device))
                else:
                    out[0].zero_()
                r.pred_boxes = Boxes(out[1]); r.scores = out[2]; r.pred_classes = out[3]           # (classes stay int32)
                r._sw_count = out[0]
                pred.append(r)
                off += n
                continue
            if n:
                ops.oicr_predict(lg[off:off + n], n, K, 1, 0, 5 * K + 1, p.proposal_boxes.tensor.float().contiguous(), bp.bbox_weights,
                                 SCALE_CLAMP, sc, bx)
                cnt, b, s, c, _ = ops.detect_postprocess(sc, bx, int(h), int(w), bp.test_score_thresh, bp.test_nms_thresh, bp.test_topk_per_image)
                if SPECULATE is not None and self.training:
                    # the teacher's weak pass inside a speculative iteration: all topk rows, the ones beyond the count with score 0 /
                    # zero box / class 0 (ops.detect_postprocess zero-fills) — the only consumer is the pseudo-label threshold
                    # (score > thres >= 0: semisup.threshold_bbox), which compacts on the device; no count is read here
                    r.pred_boxes = Boxes(b); r.scores = s; r.pred_classes = c.to(torch.int64)
                    r._sw_count = cnt
                else:
                    k = int(cnt.item())
                    r.pred_boxes = Boxes(b[:k].clone()); r.scores = s[:k].clone(); r.pred_classes = c[:k].to(torch.int64)
            else:
                r.pred_boxes = Boxes(torch.zeros(0, 4, device=lg.device)); r.scores = torch.zeros(0, device=lg.device)
                r.pred_classes = torch.zeros(0, dtype=torch.int64, device=lg.device)
            pred.append(r)
            off += n
        return pred, logits


def _loss_kwargs(M, default_loss="FocalLoss"):
    """The loss-selection keys of a detector config -> (RPN kwargs, ROI-head kwargs): ROI_HEADS.LOSS "FocalLoss" / "CrossEntropy"
    (code_release/voc_baseline.yaml, voc_split.yaml); RPN. and ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE "smooth_l1" / "smooth_l1_mean" (the
    split configs; without gradient only: the heads raise NotImplementedError on a forward that would need its gradient).  Anything
    else is refused."""
    def get(node, key, default):
        return node.get(key, default) if hasattr(node, "get") else default
    R, H, B = get(M, "RPN", {}), get(M, "ROI_HEADS", {}), get(M, "ROI_BOX_HEAD", {})
    loss = get(H, "LOSS", default_loss)
    assert loss in ("FocalLoss", "CrossEntropy"), \
        f"MODEL.ROI_HEADS.LOSS = {loss!r} is not implemented by this detector (implemented: 'FocalLoss', 'CrossEntropy')"
    types = {}
    for key, node in (("RPN", R), ("ROI_BOX_HEAD", B)):
        got = types[key] = get(node, "BBOX_REG_LOSS_TYPE", "smooth_l1")
        assert got in ("smooth_l1", "smooth_l1_mean"), \
            f"MODEL.{key}.BBOX_REG_LOSS_TYPE = {got!r} is not implemented by this detector (implemented: 'smooth_l1', 'smooth_l1_mean')"
    return dict(box_loss_type=types["RPN"]), dict(loss=loss, box_loss_type=types["ROI_BOX_HEAD"])


@META_ARCH_REGISTRY.register()
class TwoStagePseudoLabGeneralizedRCNN(nn.Module):
    """unbias/ubteacher/modeling/meta_arch/rcnn.py:8-107.  `TwoStagePseudoLabGeneralizedRCNN(cfg)` (the registry call of
    rcnn_multi.build_model, selected by MODEL.META_ARCHITECTURE of unbias/configs/code_release/voc_ssod.yaml) or explicit arguments."""

    # the module names of a config this class answers to, and the ROI_HEADS.LOSS of a config that does not name one
    PROPOSAL_GENERATOR_NAMES, ROI_HEADS_NAMES, DEFAULT_ROI_LOSS = ("PseudoLabRPN",), ("StandardROIHeadsPseudoLab",), "FocalLoss"

    def __init__(self, cfg=None, *, num_classes=20, compute_dtype=torch.float32, freeze_at=2, sampler=None,
                 pixel_mean=(103.530, 116.280, 123.675), pixel_std=(1.0, 1.0, 1.0), stride_in_1x1=True, fpn_norm="", box_head=None):
        """stride_in_1x1 / fpn_norm / box_head (keyword arguments of FastRCNNConvFCHead): RESNETS.STRIDE_IN_1X1, FPN.NORM and the
        ROI_BOX_HEAD.NUM_CONV / CONV_DIM / NUM_FC / NORM keys of a config (_arch_kwargs); the defaults are Base-RCNN-FPN.yaml's model,
        False / "FrozenBN" / 4 conv + 1 fc with FrozenBN the SoS-WSOD+ detectors (code_release/sos_plus*_test.yaml)"""
        super().__init__()
        if cfg is not None:
            M = cfg.MODEL
            # the configuration this class implements (Base-RCNN-FPN.yaml + voc_ssod.yaml); anything else is refused, not ignored
            # (the RPN / ROI-head / test keys: _cfg_kwargs; the architecture keys: _arch_kwargs)
            assert M.BACKBONE.get("NAME", "build_resnet_fpn_backbone") == "build_resnet_fpn_backbone"
            assert M.get("PROPOSAL_GENERATOR", {}).get("NAME", self.PROPOSAL_GENERATOR_NAMES[0]) in self.PROPOSAL_GENERATOR_NAMES
            assert M.ROI_HEADS.get("NAME", self.ROI_HEADS_NAMES[0]) in self.ROI_HEADS_NAMES
            assert M.get("RPN", {}).get("LOSS", "CrossEntropy") == "CrossEntropy"          # (ROI_HEADS.LOSS: _loss_kwargs)
            num_classes, freeze_at = M.ROI_HEADS.NUM_CLASSES, M.BACKBONE.get("FREEZE_AT", 2)
            pixel_mean, pixel_std = M.PIXEL_MEAN, M.PIXEL_STD
            dt_name = M.get("AMD", {}).get("COMPUTE_DTYPE", "fp32")
            compute_dtype = torch.bfloat16 if dt_name == "bf16" else torch.float32
            sampler = Sampler(int(cfg.get("SEED", 0)) if int(cfg.get("SEED", 0)) >= 0 else 0)
            rpn_kw, roi_kw, pred_kw = self._cfg_kwargs(M, cfg.get("TEST", {}))
            rpn_loss_kw, roi_loss_kw = _loss_kwargs(M, self.DEFAULT_ROI_LOSS)
            rpn_kw = dict(rpn_kw, **rpn_loss_kw); roi_kw = dict(roi_kw, **roi_loss_kw)
            stride_in_1x1, fpn_norm, box_head = self._arch_kwargs(M)
        else:
            rpn_kw, roi_kw, pred_kw = {}, dict(loss=self.DEFAULT_ROI_LOSS), {}
        sampler = sampler if sampler is not None else Sampler()
        self.backbone = FPN(ResNet(freeze_at, stride_in_1x1), fpn_norm)
        self.proposal_generator = PseudoLabRPN(sampler, **rpn_kw)
        self.roi_heads = StandardROIHeadsPseudoLab(num_classes, sampler, box_head=box_head, **roi_kw)
        bp = self.roi_heads.box_predictor
        for k, v in pred_kw.items():
            setattr(bp, k, v)
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std).view(-1, 1, 1), False)
        self.compute_dtype = compute_dtype
        self.sampler = sampler
        self.graph_nograd_backbone = False                       # _features

    @staticmethod
    def _cfg_kwargs(M, T):
        """The detectron2 keys this detector takes from a config (detectron2/detectron2/config/defaults.py values as defaults):
        passed on where the implementation is parametric, REFUSED where it is fixed — a config that changes one of them must not
        silently train or evaluate something else."""
        def get(node, key, default):
            return node.get(key, default) if hasattr(node, "get") else default
        R, H, B, A = get(M, "RPN", {}), get(M, "ROI_HEADS", {}), get(M, "ROI_BOX_HEAD", {}), get(M, "ANCHOR_GENERATOR", {})
        rpn_kw = dict(batch_size_per_image=get(R, "BATCH_SIZE_PER_IMAGE", 256), positive_fraction=get(R, "POSITIVE_FRACTION", 0.25),
                      pre_nms_topk=(get(R, "PRE_NMS_TOPK_TRAIN", 2000), get(R, "PRE_NMS_TOPK_TEST", 1000)),
                      post_nms_topk=(get(R, "POST_NMS_TOPK_TRAIN", 1000), get(R, "POST_NMS_TOPK_TEST", 1000)),
                      nms_thresh=get(R, "NMS_THRESH", 0.7),
                      anchor_sizes=tuple(s_[0] for s_ in get(A, "SIZES", [[32], [64], [128], [256], [512]])),
                      aspect_ratios=tuple(get(A, "ASPECT_RATIOS", [[0.5, 1.0, 2.0]])[0]))
        roi_kw = dict(batch_size_per_image=get(H, "BATCH_SIZE_PER_IMAGE", 512), positive_fraction=get(H, "POSITIVE_FRACTION", 0.25),
                      proposal_append_gt=get(H, "PROPOSAL_APPEND_GT", True))
        pred_kw = dict(test_score_thresh=get(H, "SCORE_THRESH_TEST", 0.05), test_nms_thresh=get(H, "NMS_THRESH_TEST", 0.5),
                       test_topk_per_image=get(T, "DETECTIONS_PER_IMAGE", 100))
        fixed = [(get(R, "IOU_THRESHOLDS", [0.3, 0.7]), [0.3, 0.7], "RPN.IOU_THRESHOLDS"), (get(R, "IOU_LABELS", [0, -1, 1]), [0, -1, 1], "RPN.IOU_LABELS"),
                 (get(R, "SMOOTH_L1_BETA", 0.0), 0.0, "RPN.SMOOTH_L1_BETA"),
                 (tuple(get(R, "BBOX_REG_WEIGHTS", (1.0, 1.0, 1.0, 1.0))), (1.0, 1.0, 1.0, 1.0), "RPN.BBOX_REG_WEIGHTS"),
                 (get(R, "LOSS_WEIGHT", 1.0), 1.0, "RPN.LOSS_WEIGHT"), (get(R, "BBOX_REG_LOSS_WEIGHT", 1.0), 1.0, "RPN.BBOX_REG_LOSS_WEIGHT"),
                 (get(R, "BOUNDARY_THRESH", -1), -1, "RPN.BOUNDARY_THRESH"),
                 (list(get(H, "IOU_THRESHOLDS", [0.5])), [0.5], "ROI_HEADS.IOU_THRESHOLDS"), (list(get(H, "IOU_LABELS", [0, 1])), [0, 1], "ROI_HEADS.IOU_LABELS"),
                 (get(B, "FC_DIM", 1024), 1024, "ROI_BOX_HEAD.FC_DIM"),                # (NUM_FC, NUM_CONV, CONV_DIM, NORM: _arch_kwargs)
                 (get(B, "POOLER_RESOLUTION", 7), 7, "ROI_BOX_HEAD.POOLER_RESOLUTION"), (get(B, "POOLER_SAMPLING_RATIO", 0), 0, "ROI_BOX_HEAD.POOLER_SAMPLING_RATIO"),
                 (get(B, "POOLER_TYPE", "ROIAlignV2"), "ROIAlignV2", "ROI_BOX_HEAD.POOLER_TYPE"), (get(B, "SMOOTH_L1_BETA", 0.0), 0.0, "ROI_BOX_HEAD.SMOOTH_L1_BETA"),
                 (tuple(get(B, "BBOX_REG_WEIGHTS", (10.0, 10.0, 5.0, 5.0))), (10.0, 10.0, 5.0, 5.0), "ROI_BOX_HEAD.BBOX_REG_WEIGHTS"),
                 (get(B, "CLS_AGNOSTIC_BBOX_REG", False), False, "ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG"), (get(B, "TRAIN_ON_PRED_BOXES", False), False, "ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES")]
        for got, want, name in fixed:
            if isinstance(want, float):
                ok = abs(float(got) - want) < 1e-12
            else:
                ok = (list(got) == list(want)) if isinstance(want, (list, tuple)) else got == want
            assert ok, f"MODEL.{name} = {got!r} is not implemented by this detector (implemented: {want!r})"
        return rpn_kw, roi_kw, pred_kw

    @staticmethod
    def _arch_kwargs(M):
        """The architecture keys of a config -> (stride_in_1x1, fpn_norm, box_head kwargs): RESNETS.STRIDE_IN_1X1, FPN.NORM ("" /
        "FrozenBN"), ROI_BOX_HEAD.NUM_CONV, CONV_DIM, NUM_FC and NORM ("" / "FrozenBN") are passed on (defaults: Base-RCNN-FPN.yaml's);
        the other RESNETS / FPN keys of detectron2/config/defaults.py are refused unless they name what is built (ResNet-50, FrozenBN,
        one group, no dilation / deformable convolution, 256 FPN channels fused by sum)."""
        def get(node, key, default):
            return node.get(key, default) if hasattr(node, "get") else default
        Rn, F, B = get(M, "RESNETS", {}), get(M, "FPN", {}), get(M, "ROI_BOX_HEAD", {})
        fixed = [(get(Rn, "DEPTH", 50), 50, "RESNETS.DEPTH"), (get(Rn, "NORM", "FrozenBN"), "FrozenBN", "RESNETS.NORM"),
                 (get(Rn, "NUM_GROUPS", 1), 1, "RESNETS.NUM_GROUPS"), (get(Rn, "WIDTH_PER_GROUP", 64), 64, "RESNETS.WIDTH_PER_GROUP"),
                 (get(Rn, "RES5_DILATION", 1), 1, "RESNETS.RES5_DILATION"), (get(Rn, "RES2_OUT_CHANNELS", 256), 256, "RESNETS.RES2_OUT_CHANNELS"),
                 (get(Rn, "STEM_OUT_CHANNELS", 64), 64, "RESNETS.STEM_OUT_CHANNELS"),
                 (any(get(Rn, "DEFORM_ON_PER_STAGE", [False])), False, "RESNETS.DEFORM_ON_PER_STAGE"),
                 (get(F, "OUT_CHANNELS", 256), 256, "FPN.OUT_CHANNELS"), (get(F, "FUSE_TYPE", "sum"), "sum", "FPN.FUSE_TYPE")]
        fpn_norm, head_norm = get(F, "NORM", ""), get(B, "NORM", "")
        fixed += [(fpn_norm in ("", "FrozenBN"), True, f"FPN.NORM {fpn_norm!r}"), (head_norm in ("", "FrozenBN"), True, f"ROI_BOX_HEAD.NORM {head_norm!r}")]
        n_conv, n_fc = int(get(B, "NUM_CONV", 0)), int(get(B, "NUM_FC", 2))
        conv_dim = int(get(B, "CONV_DIM", 256))
        fixed += [(n_conv >= 0 and n_fc >= 0 and n_conv + n_fc > 0, True, f"ROI_BOX_HEAD.NUM_CONV {n_conv} / NUM_FC {n_fc}"),
                  (n_conv == 0 or conv_dim % 8 == 0, True, f"ROI_BOX_HEAD.CONV_DIM {conv_dim}")]
        for got, want, name in fixed:
            assert got == want, f"MODEL.{name} = {got!r} is not implemented by this detector (implemented: {want!r})"
        return (bool(get(Rn, "STRIDE_IN_1X1", True)), fpn_norm,
                dict(conv_dims=(conv_dim,) * n_conv, fc_dims=(get(B, "FC_DIM", 1024),) * n_fc, conv_norm=head_norm))

    def refresh_staged_weights(self):
        """the layers' compute-dtype weight copies follow the parameters: one launch when anything changed since the last call"""
        ws = self.__dict__.get("_weight_stage")
        if ws is None or not ws.valid_for(self.compute_dtype):
            ws = self.__dict__["_weight_stage"] = WeightStage(self, self.compute_dtype)
            # the captured no-grad backbone graphs (_features) replay against the OLD stage's buffers: a re-homed parameter (.to(),
            # load_state_dict(assign=True), a flat-master re-pack, another compute dtype) would leave the teacher emitting features of
            # stale weights with no error — they go with the stage they were captured on
            self.__dict__.pop("_bb_graphs", None)
        ws.refresh()

    @property
    def device(self):
        return self.pixel_mean.device

    def preprocess_image(self, batched_inputs):
        """-> (N, H, W, 4) normalised, padded to the size divisibility, and the image sizes"""
        ims = [x["image"].to(self.device) for x in batched_inputs]
        sizes = [tuple(int(v) for v in im.shape[1:]) for im in ims]
        d = self.backbone.size_divisibility
        H = (max(s[0] for s in sizes) + d - 1) // d * d; W = (max(s[1] for s in sizes) + d - 1) // d * d
        out = torch.empty(len(ims), H, W, 4, device=self.device, dtype=self.compute_dtype)
        key = (self.pixel_mean._version, self.pixel_std._version, self.pixel_mean.data_ptr())
        hit = self.__dict__.get("_mean_std")
        if hit is None or hit[0] != key:                                 # (a device -> host read: once, not per call)
            hit = self.__dict__["_mean_std"] = (key, self.pixel_mean.flatten().tolist(), self.pixel_std.flatten().tolist())
        mean, std = hit[1], hit[2]
        for i, im in enumerate(ims):
            ops.preprocess_pad(im.contiguous(), out[i], mean, std)
        return out, sizes

    BACKBONE_GRAPHS = 6          # input shapes whose no-grad backbone pass is kept as a hipGraph (least recently used goes)

    def _features(self, x4, allow_graph=False):
        """FPN features of a preprocessed batch.  Under torch.no_grad() (the teacher's weak pass, inference) the ~105 launches of the
        ResNet-50 + FPN are shape-static and leave no autograd state: the second time an input shape is seen they are captured, from
        then on ONE hipGraph replay into the graph's own buffers (valid until the next call with this shape; every consumer runs on
        the same stream before that).  The staged weights live in persistent buffers the stage plan rewrites in place (WeightStage), so
        a replay reads the current teacher.  Off unless `graph_nograd_backbone` is set (semisup.SemiSupStep sets it on its teacher when
        it speculates; SW_S3_BACKBONE_GRAPH=0/1 overrides): bit-equal to plain launches
        (test_teacher_on_a_side_stream_and_its_backbone_as_a_graph_give_the_same_step); it holds one activation set per input shape.
        Alone it gained nothing (15.7-16.1 vs 15.8-16.0 ms: the iteration waited at its count read-backs, not for launches) — see
        semisup.SemiSupStep for what it does once those are gone."""
        env = os.environ.get("SW_S3_BACKBONE_GRAPH")
        on = self.graph_nograd_backbone if env is None else env == "1"
        # allow_graph: only the training iteration's weak pass (forward(branch="unsup_data_weak")) — evaluation (inference()) sees many
        # padded shapes once each; with 6 graphs kept it would capture, evict and re-capture (a synchronize + an activation pool each)
        if (not allow_graph or torch.is_grad_enabled() or not on or not x4.is_cuda or ops.TIMER is not None
                or torch.cuda.is_current_stream_capturing()):
            return self.backbone(x4)
        # What the backbone reads besides the input and the staged weights (refresh_staged_weights, done by the caller) must be brought
        # up to date HERE, outside the graph, into buffers that never move: the stem's FrozenBN fold is cached per buffer epoch — a
        # capture made while the cache was warm holds no launch that recomputes it (found by a replay that followed two calls inside
        # one EMA epoch: stale fold, 2 % off in the pseudo losses; tools/diag/s3_graph_debug.py)
        self.backbone.bottom_up.stem.conv1.norm.fold()
        cache = self.__dict__.setdefault("_bb_graphs", OrderedDict())
        # what a capture bakes in besides the shape: the stage's staged buffers and the stem's weight / fold buffers
        stem = self.backbone.bottom_up.stem.conv1
        key = (tuple(x4.shape), x4.dtype, x4.device.index, id(self.__dict__.get("_weight_stage")), stem.weight.data_ptr())
        hit = cache.get(key)
        if hit is None:
            cache[key] = 1                                               # seen once: eager (caches and workspaces warm up)
            while len(cache) > 4 * self.BACKBONE_GRAPHS:
                cache.popitem(last=False)
            return self.backbone(x4)
        cache.move_to_end(key)
        if hit == 1:
            n_graphs = sum(1 for v in cache.values() if v != 1)
            for k in [k for k, v in cache.items() if v != 1][:max(0, n_graphs + 1 - self.BACKBONE_GRAPHS)]:
                del cache[k]
            static_in = torch.empty_like(x4)
            static_in.copy_(x4)
            g = torch.cuda.CUDAGraph()
            with ops.capture_guard(), torch.cuda.graph(g):
                outs = self.backbone(static_in)
            hit = cache[key] = (g, static_in, outs)
        g, static_in, outs = hit
        static_in.copy_(x4)
        g.replay()
        return outs

    def forward(self, batched_inputs, branch="supervised", given_proposals=None, val_mode=False, second=None, second_targets=None):
        """second (branch "supervised" only): a SECOND, independent batch of the same branch — the semi-supervised step's pseudo-labelled
        views next to its labelled ones (unbias/ubteacher/engine/trainer.py:527-538 calls the model twice).  Both batches' backbones run
        in lockstep (ResNet.forward_lockstep), everything image- and loss-specific per batch, first batch first (the order of the two
        calls: the label samplers draw their keys in it) -> (result of the first batch, result of the second batch).
        second_targets: a callable returning the second batch's list of Instances, called only when its heads need them — after both
        backbones and the first batch's heads are queued: the teacher that produces the pseudo labels can run beside all of that on
        another stream (semisup.SemiSupStep)."""
        if (not self.training) and (not val_mode):
            return self.inference(batched_inputs)
        self.refresh_staged_weights()
        if second is not None:
            if branch != "supervised":
                raise ValueError("second batch: branch 'supervised' only")
            results = []
            pre = [self.preprocess_image(b) for b in (batched_inputs, second)]
            cs = self.backbone.bottom_up.forward_lockstep([x4 for x4, _ in pre])
            for bi, (b, (_, sizes), c) in enumerate(zip((batched_inputs, second), pre, cs)):
                if bi == 1 and second_targets is not None:
                    gt = second_targets()
                else:
                    gt = [x["instances"] for x in b] if "instances" in b[0] else None
                feats = self.backbone.forward_top(c)
                proposals, rpn_losses = self.proposal_generator(sizes, feats, gt)
                _, det_losses = self.roi_heads(feats, proposals, gt, branch=branch)
                losses = dict(det_losses); losses.update(rpn_losses)
                results.append((losses, [], [], None))
            return tuple(results)
        x4, sizes = self.preprocess_image(batched_inputs)
        gt = [x["instances"] for x in batched_inputs] if "instances" in batched_inputs[0] else None
        feats = self._features(x4, allow_graph=(branch == "unsup_data_weak"))
        if branch == "supervised":
            proposals, rpn_losses = self.proposal_generator(sizes, feats, gt)
            _, det_losses = self.roi_heads(feats, proposals, gt, branch=branch)
            losses = dict(det_losses); losses.update(rpn_losses)
            return losses, [], [], None
        if branch == "unsup_data_weak":
            proposals, _ = self.proposal_generator(sizes, feats, None, compute_loss=False)
            dets, preds = self.roi_heads(feats, proposals, targets=None, compute_loss=False, branch=branch)
            return {}, proposals, dets, preds
        if branch == "val_loss":
            proposals, rpn_losses = self.proposal_generator(sizes, feats, gt, compute_val_loss=True)
            _, det_losses = self.roi_heads(feats, proposals, gt, branch=branch, compute_val_loss=True)
            losses = dict(det_losses); losses.update(rpn_losses)
            return losses, [], [], None
        raise ValueError(branch)

    @torch.no_grad()
    def image_losses(self, batched_inputs):
        """Each image's four training losses as if it were alone in its batch (unbias/split_single.py:66-75 scores one image per
        forward) -> (N, 5) f32 on the device: loss_cls, loss_box_reg, loss_rpn_cls, loss_rpn_loc, their sum (ops.det_loss_per_image).
        The training-mode forward of the "supervised" branch (train-mode RPN top-k, label sampling, proposal_append_gt) without
        gradient; the model must be in training mode."""
        if not self.training:
            raise ValueError("image_losses: the model must be in training mode (the reference scores with the training forward)")
        if SPECULATE is not None:
            raise ValueError("image_losses: not inside a Speculation ledger (its padded rows would not match the sampled counts)")
        rpn, roi = self.proposal_generator, self.roi_heads
        rpn.keep_loss_inputs = roi.keep_loss_inputs = True
        try:
            self.forward(batched_inputs, branch="supervised")
            logits, deltas, labels, matched, anchors = rpn.__dict__.pop("last_loss_inputs")
            lg, gtc, boxes2, cnt = roi.__dict__.pop("last_loss_inputs")
            roi.__dict__.pop("last_counts", None)
        finally:
            rpn.keep_loss_inputs = roi.keep_loss_inputs = False
        R = lg.shape[0]
        return ops.det_loss_per_image(logits, deltas, labels, anchors, matched, rpn.bbox_weights, rpn.batch_size_per_image,
                                      rpn.box_loss_type, lg, roi.num_classes, gtc, boxes2[:R], boxes2[R:], cnt,
                                      roi.batch_size_per_image, roi.box_predictor.bbox_weights, roi.gamma, roi.box_loss_type)

    @torch.no_grad()
    def inference(self, batched_inputs, do_postprocess=True):
        """GeneralizedRCNN.inference (detectron2/detectron2/modeling/meta_arch/rcnn.py:177-219): detections of the ROI heads, then
        `_postprocess` (:243-259) -> `detector_postprocess` (modeling/postprocessing.py:9-59): boxes rescaled from the network's
        input resolution to each input's "height" / "width" (the dataset image: MIN_SIZE_TEST resizes every test image), clipped,
        empty ones dropped.  do_postprocess=False returns the raw list[Instances] in network-input coordinates."""
        from .inference import detector_postprocess
        self.refresh_staged_weights()
        x4, sizes = self.preprocess_image(batched_inputs)
        feats = self._features(x4)
        proposals, _ = self.proposal_generator(sizes, feats, None, compute_loss=False)
        dets, _ = self.roi_heads(feats, proposals, targets=None, compute_loss=False)
        if not do_postprocess:
            return dets
        return [{"instances": detector_postprocess(d, inp.get("height", s[0]), inp.get("width", s[1]))}
                for d, inp, s in zip(dets, batched_inputs, sizes)]


@META_ARCH_REGISTRY.register()
class GeneralizedRCNN(TwoStagePseudoLabGeneralizedRCNN):
    """detectron2/detectron2/modeling/meta_arch/rcnn.py:24-259 — the meta-architecture config.get_cfg() names by default and the
    SoS-WSOD+ test configs select (unbias/configs/code_release/sos_plus_test.yaml, sos_plus_wo_imagenet_test.yaml): the same detector
    with the reference's plain interface.  In training `forward(batched_inputs)` returns the four losses (rcnn.py:125-175), in
    eval mode `inference`.  PROPOSAL_GENERATOR.NAME "RPN" and ROI_HEADS.NAME "StandardROIHeads" build the modules of the base
    class — their pseudo-label branches are not reached through this interface — and a config without ROI_HEADS.LOSS trains with
    detectron2's cross entropy."""
    PROPOSAL_GENERATOR_NAMES, ROI_HEADS_NAMES, DEFAULT_ROI_LOSS = ("RPN", "PseudoLabRPN"), ("StandardROIHeads", "StandardROIHeadsPseudoLab"), "CrossEntropy"

    def forward(self, batched_inputs):
        if not self.training:
            return self.inference(batched_inputs)
        return super().forward(batched_inputs, branch="supervised")[0]


@META_ARCH_REGISTRY.register()
class ProposalNetwork(TwoStagePseudoLabGeneralizedRCNN):
    """detectron2/detectron2/modeling/meta_arch/rcnn.py:249-329 — the detector's backbone, preprocessing and proposal generator
    without ROI heads (MODEL.META_ARCHITECTURE: ProposalNetwork): the state-dict names are the reference's `backbone.*` and
    `proposal_generator.*` (with the `pixel_mean` / `pixel_std` buffers, not saved there either).  In training
    `forward(batched_inputs)` returns the two RPN losses; in eval mode [{"proposals": Instances(proposal_boxes,
    objectness_logits)}] after `detector_postprocess` to each input's "height" / "width".  The modules and the path are the
    detector's own, so with the same weights the proposals are the ones its `inference` hands to the ROI heads.  The ROI-head keys
    of a detector config are read and checked as the detector does, and otherwise unused."""

    PROPOSAL_GENERATOR_NAMES = ("RPN", "PseudoLabRPN")

    def __init__(self, cfg=None, *, compute_dtype=torch.float32, freeze_at=2, sampler=None, pixel_mean=(103.530, 116.280, 123.675),
                 pixel_std=(1.0, 1.0, 1.0), stride_in_1x1=True, fpn_norm="", rpn=None):
        """rpn: keyword arguments of PseudoLabRPN (pre_nms_topk, post_nms_topk, nms_thresh, ...) when there is no config"""
        nn.Module.__init__(self)
        rpn_kw = dict(rpn or {})
        if cfg is not None:
            M = cfg.MODEL
            assert M.BACKBONE.get("NAME", "build_resnet_fpn_backbone") == "build_resnet_fpn_backbone"
            assert M.get("PROPOSAL_GENERATOR", {}).get("NAME", "RPN") in self.PROPOSAL_GENERATOR_NAMES
            assert M.get("RPN", {}).get("LOSS", "CrossEntropy") == "CrossEntropy"
            freeze_at = M.BACKBONE.get("FREEZE_AT", 2)
            pixel_mean, pixel_std = M.PIXEL_MEAN, M.PIXEL_STD
            compute_dtype = torch.bfloat16 if M.get("AMD", {}).get("COMPUTE_DTYPE", "fp32") == "bf16" else torch.float32
            sampler = Sampler(int(cfg.get("SEED", 0)) if int(cfg.get("SEED", 0)) >= 0 else 0)
            rpn_kw = dict(self._cfg_kwargs(M, cfg.get("TEST", {}))[0], **_loss_kwargs(M)[0])
            stride_in_1x1, fpn_norm, _ = self._arch_kwargs(M)
        sampler = sampler if sampler is not None else Sampler()
        self.backbone = FPN(ResNet(freeze_at, stride_in_1x1), fpn_norm)
        self.proposal_generator = PseudoLabRPN(sampler, **rpn_kw)
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std).view(-1, 1, 1), False)
        self.compute_dtype = compute_dtype
        self.sampler = sampler
        self.graph_nograd_backbone = False

    def load_detector_state_dict(self, state_dict):
        """load a detector's checkpoint by name: its `backbone.*` and `proposal_generator.*` entries; `roi_heads.*` is ignored,
        anything else that does not fit is an error"""
        return self.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("roi_heads.")}, strict=True)

    def forward(self, batched_inputs):
        if not self.training:
            return self.inference(batched_inputs)
        self.refresh_staged_weights()
        x4, sizes = self.preprocess_image(batched_inputs)
        gt = [x["instances"] for x in batched_inputs] if "instances" in batched_inputs[0] else None
        _, losses = self.proposal_generator(sizes, self._features(x4), gt)
        return losses

    def image_losses(self, batched_inputs):
        raise NotImplementedError("ProposalNetwork has no ROI heads: image_losses scores the four losses of a detector")

    @torch.no_grad()
    def inference(self, batched_inputs, do_postprocess=True):
        """rcnn.py:301-329; do_postprocess=False returns the raw list[Instances] in network-input coordinates"""
        from .inference import detector_postprocess
        self.refresh_staged_weights()
        x4, sizes = self.preprocess_image(batched_inputs)
        proposals, _ = self.proposal_generator(sizes, self._features(x4), None, compute_loss=False)
        if not do_postprocess:
            return proposals
        return [{"proposals": detector_postprocess(p, inp.get("height", s[0]), inp.get("width", s[1]))}
                for p, inp, s in zip(proposals, batched_inputs, sizes)]

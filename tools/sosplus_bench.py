"""What the SoS-WSOD+ detector forms cost (frcnn._Conv3x3ColFn, csrc/conv_col.hip) -> one JSON line.

  * `stride2_layers`: the three stride-2 3x3 convolutions of the torchvision-style ResNet-50 at an 800 x 1216 input (conv2 of block 0 of
    res3 / res4 / res5: 100x152x128, 50x76x256, 25x38x512 inputs), bf16, FrozenBN shift + ReLU: the column-matrix path (sw_im2col3x3 +
    sw_gemm) against the composition of entry points that existed before it — a stride-1 `conv3x3` over the whole map followed by
    `subsample2x` (four times the FLOP) — forward alone and forward + backward (node against node), timed in alternating windows of
    one process (host clock around a window that ends in a synchronise); per layer the windows' medians, every window (the spread)
    and the largest difference of the two outputs relative to max|out|.
  * `kernels`: sw_im2col3x3 and sw_col2im3x3 alone on those layers' tensors, device time by HIP events (median of single launches:
    an upper bound, the pair includes the launch gap), their algorithmic bytes (input read once + columns written once, and the
    reverse) per second and that as a share of the 8 TB/s HBM peak of the MI355X.  Recorded, not a criterion.
  * `inference_ms_per_image`: `model.inference` of the three detector variants (the STRIDE_IN_1X1 / 2-fc model, "woi", "plus") on one
    688 x 917 image (a VOC image at MIN_SIZE_TEST 688), bf16, the closed-form parameters of the tests (random weights whose
    FrozenBN gains keep the activations O(1)); `proposals` / `detections`: what the image gave, so that the time can be read.
  * `box_head_train_ms`: forward + backward of the box head alone on 1024 pooled ROIs (2 images x 512), 2-fc against 4conv1fc.  The
    4conv1fc head goes through a (R * 49, 2304) column matrix per convolution; its cost is recorded here and not optimised.

    python tools/sosplus_bench.py [--windows 5] [--iters 30] [--launches 200] [--batch 1]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYERS = [("res3.0.conv2", 100, 152, 128), ("res4.0.conv2", 50, 76, 256), ("res5.0.conv2", 25, 38, 512)]
HBM_PEAK = 8.0e12
K = 20


def windows(fns, n_windows, iters):
    """alternating windows: -> per function the list of ms per call"""
    out = [[] for _ in fns]
    for _ in range(n_windows):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / iters * 1e3)
    return out


def event_us(fn, launches):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for s, e in ev:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    us = [s.elapsed_time(e) * 1e3 for s, e in ev]
    return statistics.median(us), min(us)


def summary(ws):
    return {"median_ms": round(statistics.median(ws), 4), "windows_ms": [round(w, 4) for w in ws]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from sos_wsod_amd import frcnn as fr, ops
    from sos_wsod_amd.config import add_wsl_config, get_cfg
    from sos_wsod_amd.rcnn_multi import build_model
    cd = torch.bfloat16
    g = torch.Generator().manual_seed(0)
    out = {"compute_dtype": "bf16", "batch": a.batch, "stride2_layers": {}, "kernels": {}}

    for name, H, W, C in LAYERS:
        n = a.batch
        x = torch.randn(n, H, W, C, generator=g).to(cd).cuda().requires_grad_(True)
        w = torch.nn.Parameter((torch.randn(C, C, 3, 3, generator=g) * (9 * C) ** -0.5).cuda())
        scale = (torch.rand(C, generator=g) + 0.5).cuda()
        shift = (torch.randn(C, generator=g) * 0.1).cuda()
        weff = w.detach() * scale.view(-1, 1, 1, 1)
        st = weff.permute(0, 2, 3, 1).reshape(C, 9, C).to(cd).contiguous()
        std = weff.flip(2, 3).permute(1, 2, 3, 0).reshape(C, 9, C).to(cd).contiguous()       # [ci][tap'][co]: the data-gradient layout
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        gy = torch.randn(n, Ho, Wo, C, generator=g).to(cd).cuda()
        full = torch.empty(n, H, W, C, device="cuda", dtype=cd)
        sub = torch.empty(n, Ho, Wo, C, device="cuda", dtype=cd)
        ep = ops.make_epilogue(bias=shift, relu=True, out_dtype=cd)

        def new_fwd():
            with torch.no_grad():
                return fr._Conv3x3ColFn.apply(x, st, shift, scale, True, 2, w, None)

        def old_fwd():
            ops.conv3x3(x.detach(), st, full, 1, ep)
            return ops.subsample2x(full, sub)

        def new_train():
            x.grad = w.grad = None
            fr._Conv3x3ColFn.apply(x, st, shift, scale, True, 2, w, None).backward(gy)

        def old_train():
            x.grad = w.grad = None
            fr._Subsample2Fn.apply(fr._Conv3x3Fn.apply(x, st, std, shift, scale, True, w, None)).backward(gy)
        for fn in (new_fwd, old_fwd, new_train, old_train):
            for _ in range(3):
                fn()
        diff = float((new_fwd().float() - old_fwd().float()).abs().max() / old_fwd().float().abs().max())
        new_train(); gn = (x.grad.float().clone(), w.grad.clone())
        old_train(); go = (x.grad.float().clone(), w.grad.clone())
        gdiff = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(gn, go)]
        wf = windows([new_fwd, old_fwd], a.windows, a.iters)
        wt = windows([new_train, old_train], a.windows, a.iters)
        out["stride2_layers"][name] = {
            "input": [n, H, W, C], "forward_col": summary(wf[0]), "forward_conv3x3_subsample2x": summary(wf[1]),
            "train_col": summary(wt[0]), "train_conv3x3_subsample2x": summary(wt[1]), "forward_max_rel_diff": diff,
            "dx_dw_max_rel_diff": gdiff}
        # ---- the two kernels alone
        col = torch.empty(n * Ho * Wo, 9 * C, device="cuda", dtype=cd)
        dx = torch.empty(n, H, W, C, device="cuda", dtype=cd)
        xd = x.detach()
        b_in, b_col = xd.numel() * 2, col.numel() * 2
        ku = {}
        for kname, fn in (("im2col3x3", lambda: ops.im2col3x3(xd, col, 2)), ("col2im3x3", lambda: ops.col2im3x3(col, dx, 2, relu_ref=xd))):
            med, mn = event_us(fn, a.launches)
            nbytes = b_in + b_col + (b_in if kname == "col2im3x3" else 0)                      # (col2im reads the mask as well)
            ku[kname] = {"us_median": round(med, 2), "us_min": round(mn, 2), "bytes": nbytes, "TB_per_s": round(nbytes / med / 1e6, 3),
                         "share_of_hbm_peak": round(nbytes / (med * 1e-6) / HBM_PEAK, 3)}
        out["kernels"][name] = ku
        del x, w, full, sub, col, dx

    # ---- per-image inference of the three variants
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sosplus_ref as SP
    from oracle import frcnn_oracle as FO
    models = {}
    torch.manual_seed(0)
    models["stride_in_1x1_2fc"] = fr.TwoStagePseudoLabGeneralizedRCNN(num_classes=K, compute_dtype=cd).cuda().eval()
    for variant, extra in (("woi", []), ("plus", ["MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.NUM_FC", 1, "MODEL.ROI_BOX_HEAD.NORM", "FrozenBN"])):
        cfg = add_wsl_config(get_cfg())
        cfg.merge_from_list(["MODEL.META_ARCHITECTURE", "GeneralizedRCNN", "MODEL.BACKBONE.NAME", "build_resnet_fpn_backbone",
                             "MODEL.RESNETS.STRIDE_IN_1X1", False, "MODEL.FPN.NORM", "FrozenBN", "MODEL.ROI_HEADS.NAME", "StandardROIHeads",
                             "MODEL.ROI_HEADS.NUM_CLASSES", K, "MODEL.ROI_BOX_HEAD.NUM_FC", 2, "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7,
                             "MODEL.AMD.COMPUTE_DTYPE", "bf16"] + extra)
        models[variant] = build_model(cfg).eval()
    for name, m in models.items():
        P = FO.make_params(K, tag="bench", head_scale=5.0) if name == "stride_in_1x1_2fc" else SP.make_params(name, "bench", 5.0)
        if name == "stride_in_1x1_2fc":                                  # (FO.make_params sizes the stem's gain for pixel std 1: that model's default)
            assert float(m.pixel_std.flatten()[0]) == 1.0
        sd = m.state_dict()
        with torch.no_grad():
            for k, v in P.items():
                sd[k].copy_(torch.from_numpy(v))
    inp = {"image": torch.randint(0, 256, (3, 688, 917), generator=g, dtype=torch.uint8).cuda(), "height": 375, "width": 500}
    fns = [(lambda m=m: m.inference([inp])) for m in models.values()]
    with torch.no_grad():
        for fn in fns:
            for _ in range(3):
                fn()
        ws = windows(fns, a.windows, max(a.iters // 3, 5))
    out["inference_ms_per_image"] = {k: summary(w_) for k, w_ in zip(models, ws)}
    with torch.no_grad():
        for k, m in models.items():
            m.inference([inp])
            out["inference_ms_per_image"][k]["proposals"] = int(m.roi_heads.last_levels.numel())
            out["inference_ms_per_image"][k]["detections"] = len(m.inference([inp])[0]["instances"])

    # ---- the box head alone, forward + backward, 1024 ROIs
    heads = {"2fc": models["woi"].roi_heads.box_head, "4conv1fc": models["plus"].roi_heads.box_head}
    for m in (models["woi"], models["plus"]):
        m.train(); m.refresh_staged_weights()
    pooled = torch.randn(1024, 256 * 49, generator=g).to(cd).cuda().requires_grad_(True)
    gy = torch.randn(1024, 1024, generator=g).to(cd).cuda()

    def head_step(h):
        pooled.grad = None
        for p in h.parameters():
            p.grad = None
        h(pooled).backward(gy)
    fns = [(lambda h=h: head_step(h)) for h in heads.values()]
    for fn in fns:
        for _ in range(3):
            fn()
    ws = windows(fns, a.windows, max(a.iters // 3, 5))
    out["box_head_train_ms"] = {k: summary(w_) for k, w_ in zip(heads, ws)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Full-size parity against the oracle for BASELINE configs #2 (4 views 512x512, R=2000, K=20) and #4 (800x1333, R=4000,
K=80) — the benchmarked shapes, not toy fixtures.

test_config2_fp32_end_to_end_against_the_oracle runs the WHOLE config-#2 iteration (images in, losses and every gradient out)
through the oracle on the host (~20 s on the GPU box) against the fp32 HIP path.  The other tests keep the dense half (convs,
fc6/fc7) on the GPU (its full-size contractions: test_gpu_e2e.py::test_full_size_contractions_match_torch_matmul) and check
everything downstream of the logits — the half with the integer outputs north_star wants bit exact, cheap on the host at any
size — for bf16, fp32, two images per GPU (config #3's per-GPU shape) and COCO: the GPU's own f32 logits (16000 x 1764 for COCO) and
boxes go to the CPU and the ORACLE recomputes WSDDN scores / loss, the view means, top-p% mining, NMS, IoU labels,
cross-view targets and the 8 refinement losses from them (roi_heads_oicrplus.py:560-757, fast_rcnn_oicr.py:157-352,
fast_rcnn_wsddn.py:340-375).  Integer stages are fed bit-identical float inputs (the GPU's mining scores, after those were
checked against the oracle's to float tolerance), so their outputs must agree bit for bit.
ROIPool: argmax / values of all 4R ROIs on the real 63x63 and 99x165 maps against the C oracle, one channel of each of the
64 eight-channel slabs the kernel works on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import oicr_oracle as O  # noqa: E402  (checker only)

VIEWS = ("1", "1_flip", "2", "2_flip")


def _peaky(model, scale):
    """random-init heads give near-uniform scores (everything below MIST_THRE, one pseudo box per class); scale the class
    predictors so that the mining / NMS / labelling stages see thousands of candidates like a trained model's"""
    with torch.no_grad():
        hd = model.roi_heads
        for w in [hd.box_predictor.cls.weight, hd.box_predictor.det.weight] + [r.cls_score.weight for r in hd.box_refinery]:
            w.mul_(scale)


def _run(H, W, R, K, n_gt, dtype, freeze_at, seed, scale, B=1):
    import bench
    from sos_wsod_amd.events import EventStorage
    dev = torch.device("cuda", 0)
    model = bench.build(dev, dtype, K=K, freeze_at=freeze_at)
    _peaky(model, scale)
    model.train()
    data = sum((bench.make_inputs(dev, seed + 1000 * b, H=H, W=W, R=R, K=K, n_gt=n_gt + b) for b in range(B)), [])
    with EventStorage(0):
        losses = model(data)
        losses.total().backward()
    torch.cuda.synchronize()
    return model, data, losses


def _check_heads_against_oracle(model, data, losses, R, K):
    """every image of the batch (the reference: one per GPU; B > 1 = the mean of B such iterations, what DDP forms over B ranks)"""
    hd = model.roi_heads
    cols = hd._col_layout()
    RK = hd.refine_K
    got = {k: float(v) for k, v in losses.items()}
    B = len(data)
    assert len(hd.last_aux["images"]) == B
    ref_sum, n_cand = {}, []
    for b in range(B):
        aux = hd.last_aux["images"][b]
        lt = aux["logits"].detach().cpu()                                       # (4R, ld) f32: the GPU's own logits
        boxes = [data[b]["proposals" + v].proposal_boxes.tensor.cpu().numpy() for v in VIEWS]
        gt_int, gt_oh = O.image_level_gt(data[b]["instances1"].gt_classes.numpy(), K)
        gt_oh_t = torch.from_numpy(gt_oh)
        # ---- WSDDN scores, loss, view mean (fast_rcnn_wsddn.py:556-567,340-375; roi_heads_oicrplus.py:283-294)
        sc, loss_cls = [], 0.0
        for v in range(4):
            rows = lt[v * R:(v + 1) * R]
            s = F.softmax(rows[:, cols["cls"]:cols["cls"] + K], dim=1) * F.softmax(rows[:, cols["det"]:cols["det"] + K], dim=0)
            loss_cls = loss_cls + O.wsddn_loss(s, gt_oh_t)
            sc.append(s)
            np.testing.assert_allclose(aux["scores"][v].cpu().numpy(), s.numpy(), rtol=1e-4, atol=1e-12)
        ref = {"loss_cls": float(loss_cls / 4.0)}
        ms = aux["mine_scores"].cpu().numpy()                                    # (RK, R, K+1): what the GPU mined from
        np.testing.assert_allclose(ms[0][:, :K], ((sc[0] + sc[1] + sc[2] + sc[3]) / 4.0).numpy(), rtol=1e-5, atol=1e-12)
        for k in range(RK):
            # ---- integer stages on bit-identical inputs: mined indices / classes / scores, labels, gt_index, weights
            pgt = O.get_pgt_mist(ms[k], boxes[0], gt_int)
            lab = O.label_proposals(pgt, boxes[0], K)
            r = aux["rounds"][k]
            n = int(r["pgt_count"].item())
            n_cand.append(len(pgt["pre_nms"]["scores"]))
            assert np.array_equal(r["pgt_index"][:n].cpu().numpy(), pgt["index"]), (b, k)
            assert np.array_equal(r["pgt_class"][:n].cpu().numpy(), pgt["classes"]), (b, k)
            assert np.array_equal(r["pgt_score"][:n].cpu().numpy(), pgt["scores"]), (b, k)
            assert np.array_equal(r["lab_class"].cpu().numpy(), lab["gt_classes"]), (b, k)
            assert np.array_equal(r["lab_index"].cpu().numpy(), lab["gt_index"]), (b, k)
            assert np.array_equal(r["lab_weight"].cpu().numpy(), lab["gt_weights"]), (b, k)
            # ---- refinement losses of this round from the GPU's logits and the oracle's labels (fast_rcnn_oicr.py:157-352)
            c0 = cols[f"cls_score{k}"]; b0 = cols[f"bbox_pred{k}"]
            lc, lb = 0.0, 0.0
            for v in range(4):
                gtb = lab["gt_boxes"] if v == 0 else boxes[v][lab["gt_index"]]     # cross-view targets (:327-371)
                pv = 2 if v == 3 else v                                            # quirk A.2 #1 (:381)
                rows = lt[pv * R:(pv + 1) * R]
                a, bb = O.oicr_losses(rows[:, c0:c0 + K + 1], rows[:, b0:b0 + 4 * K], boxes[v], gtb, lab["gt_classes"],
                                      lab["gt_weights"], K)
                lc = lc + a; lb = lb + bb
            ref[f"loss_cls_r{k}"] = float(lc / 4.0); ref[f"loss_box_reg_r{k}"] = float(lb / 4.0)
            if k + 1 < RK:                                                         # next round's mining input (:390-395)
                nxt = sum(F.softmax(lt[v * R:(v + 1) * R, c0:c0 + K + 1], dim=-1) for v in range(4)) / 4.0
                np.testing.assert_allclose(ms[k + 1], nxt.numpy(), rtol=1e-5, atol=1e-12)
        for name, v in ref.items():
            ref_sum[name] = ref_sum.get(name, 0.0) + v / B
    assert set(ref_sum) == set(got)
    for name, want in ref_sum.items():
        assert abs(got[name] - want) <= 1e-4 * abs(want) + 1e-9, (name, got[name], want)     # north_star: 1e-4 rel
    return n_cand


def _check_roipool_against_c_oracle(model, data, R, image=0):
    """all 4R ROIs on the real feature maps of this iteration, one channel per 8-channel slab (64 channels)"""
    import sos_wsod_amd.ops as ops
    hd = model.roi_heads
    dt_ = hd.compute_dtype
    dev = torch.device("cuda", 0)
    ch = torch.arange(3, 512, 8, device=dev)
    for s, (a, b) in enumerate((("1", "1_flip"), ("2", "2_flip"))):
        with torch.no_grad():
            f = model.backbone.forward_nhwc(model._views_to_nhwc([data[image]["image" + a], data[image]["image" + b]]))
        n, h, w, C = f.shape
        bx = torch.cat([data[image]["proposals" + a].proposal_boxes.tensor, data[image]["proposals" + b].proposal_boxes.tensor], 0)
        idx = (torch.arange(2 * R, device=dev) >= R).float()[:, None]
        rois = torch.cat([idx, bx], 1).contiguous()
        out = torch.empty(2 * R, C * 49, device=dev, dtype=dt_)
        arg = torch.empty(2 * R, C * 49, device=dev, dtype=ops.roi_argmax_dtype(h, w))
        ops.roi_pool_fwd(f, rois, out, arg, hd.box_pooler.scale, 7, 7)
        got_arg = ops.argmax_to_int32(arg).view(2 * R, C, 49)[:, ch].cpu().numpy()
        got_out = out.view(2 * R, C, 49)[:, ch].float().cpu().numpy()
        feat = f[..., ch].permute(0, 3, 1, 2).float().contiguous().cpu().numpy()      # NCHW f32 of the same values
        ref_out, ref_arg = O.roi_pool_fwd(feat, rois.cpu().numpy(), hd.box_pooler.scale, 7, 7)
        assert np.array_equal(got_arg, ref_arg.reshape(2 * R, len(ch), 49)), f"scale {s}: argmax differs"
        assert np.array_equal(got_out, ref_out.reshape(2 * R, len(ch), 49)), f"scale {s}: pooled values differ"
        assert (ref_arg >= 0).mean() > 0.5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_config2_voc_512_r2000_k20_against_the_oracle(dtype):
    """BASELINE configs[1]: the benchmarked workload (bf16) and the reference's own precision (fp32)"""
    R, K = 2000, 20
    model, data, losses = _run(512, 512, R, K, n_gt=3, dtype=dtype, freeze_at=2, seed=21, scale=40.0)
    assert tuple(model.roi_heads.last_aux["logits"].shape) == (4 * R, 448)
    n_cand = _check_heads_against_oracle(model, data, losses, R, K)
    assert max(n_cand) > 100, n_cand                    # the threshold / NMS stages saw a real candidate list
    _check_roipool_against_c_oracle(model, data, R)


def test_config3_per_gpu_shape_two_images_512_r2000_against_the_oracle():
    """BASELINE configs[2] per GPU: batch 16 over 8 GPUs = TWO images (8 views 512x512, R = 2000 each) per GPU per step, bf16.
    Every image's heads against the oracle (the losses are the mean over the two images) and image 1's ROIPool on its real maps."""
    R, K = 2000, 20
    model, data, losses = _run(512, 512, R, K, n_gt=2, dtype=torch.bfloat16, freeze_at=2, seed=31, scale=40.0, B=2)
    assert tuple(model.roi_heads.last_aux["images"][1]["logits"].shape) == (4 * R, 448)
    n_cand = _check_heads_against_oracle(model, data, losses, R, K)
    assert max(n_cand) > 100, n_cand
    _check_roipool_against_c_oracle(model, data, R, image=1)


@pytest.mark.parametrize("gemm", ["f32", "bf16x3"])
def test_config2_fp32_end_to_end_against_the_oracle(gemm):
    """gemm = "bf16x3": the same test with the fc6 / fc7 GEMMs AND the convolutions from conv1_2 on (forward, data and weight
    gradients) as six-product bf16x3 GEMMs (ops.gemm_f32x3 / backbone_vgg x3_layer: three bf16 pieces per operand, ~2^-24 |a||b| per
    product, f32 accumulation) — same bars.
    BASELINE configs[1] in the reference's own precision, WHOLE path, nothing shrunk: 4 u8 views 512x512 in, R = 2000, K = 20,
    fc 4096/4096 (136 M closed-form parameters), injected dropout masks -> the oracle's full iteration with autograd on the host
    (the same call bench.py's cpu_baseline times: ~20 s on the GPU box) against the HIP path: the 9 losses within 1e-4 relative,
    mined pseudo boxes / proposal labels bit exact, EVERY gradient tensor within 2e-3 of its largest element (see the note at the
    check)."""
    from helpers import build_model, load_params, to_batched_inputs
    from sos_wsod_amd.events import EventStorage
    K, R, H, W, dan = 20, 2000, 512, 512, (4096, 4096)
    nthreads = torch.get_num_threads()
    P = O.make_params(K, dan, tag="pcfg2", head_scale=30.0)
    views, gt = O.make_views(H, W, R, n_gt=3, K=K, scale2=1.0, tag="vcfg2")
    assert all(v["image"].shape == (3, H, W) for v in views)
    masks = O.make_masks(R, dan, tag="mcfg2")
    ol, oaux, og = O.oicr_plus_iteration(P, views, gt, masks, K=K, want_grads=True)
    model = build_model(K, dan, torch.float32)
    load_params(model, P)
    model.train()
    model.roi_heads.debug_drop_masks = [[torch.from_numpy(m) for m in v] for v in masks]
    model.roi_heads.fp32x3 = gemm == "bf16x3"
    model.backbone.fp32x3 = gemm == "bf16x3"                 # the convolutions (>= 64 channels each side) as bf16x3 too (round 6)
    with EventStorage(0):
        losses = model(to_batched_inputs(views, gt))
        sum(losses.values()).backward()
    torch.cuda.synchronize()
    aux = model.roi_heads.last_aux
    flips = []
    for k in range(4):
        r, o = aux["rounds"][k], oaux["rounds"][k]
        n = int(r["pgt_count"].item())
        same = np.array_equal(r["pgt_index"][:n].cpu().numpy(), o["pgt"]["index"]) and \
            np.array_equal(r["pgt_class"][:n].cpu().numpy(), o["pgt"]["classes"])
        lab_flips = int((r["lab_class"].cpu().numpy() != o["labels"]["gt_classes"]).sum()) + \
            int((r["lab_index"].cpu().numpy() != o["labels"]["gt_index"]).sum())
        flips.append((k, same, lab_flips, n))
    print("config #2 fp32 e2e: (round, mined set equal, label flips, pseudo boxes):", flips)
    assert all(f[1] and f[2] == 0 for f in flips), flips
    for k, v in losses.items():
        assert abs(v.item() - ol[k]) <= 1e-4 * abs(ol[k]) + 1e-7, (k, v.item(), ol[k])
    # Gradient bound at this size: 2e-3 of the tensor's largest element, backbone included.  The toy fixtures hold 2e-4
    # (test_gpu_e2e.py); here every gradient is a sum over 8000 proposal rows behind |logit| ~ 50 heads: an f32 summation-order
    # difference of 1e-6 in a logit is 5e-5 in its softmax and in dlogits, and the sums over 444 logit columns / 8000 rows cancel
    # heavily (measured: fc2.weight 8.0e-4, fc1.weight 6.7e-4, backbone 2.0e-4 ... 5.5e-4; the refinement heads 1e-6).
    worst, bad = {}, []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert p.grad is None and og.get(name) is not None      # the oracle differentiates everything; FREEZE_AT is the product's
            continue
        got, ref = p.grad.cpu().numpy(), og[name]
        assert np.isfinite(got).all(), name
        err = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
        worst[name] = err
        if float(np.abs(ref).max()) <= 1e-6:                         # d/d(det.bias): analytically 0, noise on both sides
            assert float(np.abs(got).max()) <= 1e-5, name
            continue
        if err > 2e-3:
            bad.append((name, err))
    print("config #2 fp32 e2e, gradient error / largest element per tensor:", {k.replace("roi_heads.", "").replace("backbone.", "bb."): "%.1e" % v
                                                                               for k, v in worst.items()})
    assert not bad, bad
    w = max(worst.items(), key=lambda t: t[1] if not t[0].startswith("backbone.") else 0.0)
    wb = max(worst.items(), key=lambda t: t[1] if t[0].startswith("backbone.") else 0.0)
    print(f"config #2 fp32 e2e: worst head gradient error {w[1]:.2e} ({w[0]}), worst backbone {wb[1]:.2e} ({wb[0]})")
    torch.set_num_threads(nthreads)


def test_config4_coco_800x1333_r4000_k80_against_the_oracle():
    """BASELINE configs[3] per GPU: 4 views 800x1333 (99x165 maps), R=4000, K=80, FREEZE_AT 3, heads 4096 x 1764
    (coco_oicr_plus.yaml:19)"""
    R, K = 4000, 80
    model, data, losses = _run(800, 1333, R, K, n_gt=7, dtype=torch.bfloat16, freeze_at=3, seed=22, scale=40.0)
    assert model.roi_heads.n_head_cols == 1764
    n_cand = _check_heads_against_oracle(model, data, losses, R, K)
    assert max(n_cand) > 100, n_cand
    _check_roipool_against_c_oracle(model, data, R)


def test_mining_coco_topk_10000_proposals_18_classes():
    """coco_oicr_plus.yaml:67 PRECOMPUTED_PROPOSAL_TOPK_TRAIN 10000 with 18 image-level classes: top_k * G = 18000 sort
    keys exceed LDS -> the workspace-resident sort; must equal the oracle bit for bit (and not return -6)"""
    import sos_wsod_amd.ops as ops
    R, K, G, NR = 10000, 80, 18, 2
    views, _ = O.make_views(800, 1344, R, n_gt=G, K=K, tag="coco10k")
    boxes = views[0]["boxes"]
    rng = np.random.RandomState(5)
    gt = np.sort(rng.choice(K, G, replace=False)).astype(np.int64)
    sc = np.zeros((NR, R, K + 1), np.float32)
    sc[0, :, :K] = rng.rand(R, K).astype(np.float32) ** 6                   # round 0: WSDDN-like, K columns
    sc[1] = np.round(rng.rand(R, K + 1).astype(np.float32), 2)              # round 1: many exact ties
    top_k = max(int(R * 0.10), 1)
    assert top_k * G > 16384
    dev = "cuda"
    lab_c = torch.empty(NR, R, dtype=torch.int32, device=dev); lab_w = torch.empty(NR, R, device=dev)
    lab_i = torch.empty(NR, R, dtype=torch.int32, device=dev); cnt = torch.zeros(NR, dtype=torch.int32, device=dev)
    pi = torch.empty(NR, top_k * G, dtype=torch.int32, device=dev); pc = torch.empty_like(pi)
    ps = torch.empty(NR, top_k * G, device=dev)
    ws = torch.empty(ops.mine_workspace_bytes(R, top_k, G, NR), dtype=torch.uint8, device=dev)
    ops.oicr_mine_label(torch.from_numpy(sc).cuda(), torch.from_numpy(gt.astype(np.int32)).cuda(),
                        torch.from_numpy(boxes).cuda(), K, top_k, 0.05, 0.01, 0.5, 0.6, lab_c, lab_w, lab_i, cnt, pi, pc, ps, ws)
    torch.cuda.synchronize()
    for k in range(NR):
        o = O.get_pgt_mist(sc[k], boxes, gt)
        l = O.label_proposals(o, boxes, K)
        n = int(cnt[k].item())
        assert np.array_equal(pi[k, :n].cpu().numpy(), o["index"])
        assert np.array_equal(pc[k, :n].cpu().numpy(), o["classes"])
        assert np.array_equal(ps[k, :n].cpu().numpy(), o["scores"])
        assert np.array_equal(lab_c[k].cpu().numpy(), l["gt_classes"])
        assert np.array_equal(lab_i[k].cpu().numpy(), l["gt_index"])
        assert np.array_equal(lab_w[k].cpu().numpy(), l["gt_weights"])


def test_stage3_supervised_branch_at_config5_image_size_against_the_oracle():
    """BASELINE config #5's per-GPU image shape: the Stage-3 detector's supervised branch on two views of 800 x 1216 and 768 x 1024
    (the second is padded to the first's grid: 200 x 304 ... 13 x 19 maps, 242 991 anchors per image, 2000 + 2000 + 2000 + 2000 + 741
    candidates through the mask-form NMS) in fp32 against oracle/frcnn_oracle.py, which the reference-generated fixtures pin at
    96 x 128: RPN losses 1e-4 and the sampled anchor labels bit for bit; the same proposals up to ulp-tied neighbours (set
    comparison at 1e-2 px, <= 1 % unmatched), ROI-head losses 1e-2 (position-based sampling: DESIGN §4); gradient samples."""
    from oracle import frcnn_oracle as FO
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN
    from sos_wsod_amd.structures import Boxes, Instances
    K = 20
    P = FO.make_params(K, tag="s3full", head_scale=12.0)
    sizes = [(800, 1216), (768, 1024)]
    imgs = [FO.make_image(h, w, f"s3full{i}") for i, (h, w) in enumerate(sizes)]
    gts = [FO.make_gt(h, w, 3, K, f"s3full{i}") for i, (h, w) in enumerate(sizes)]
    ref, aux, grads = FO.supervised_forward(P, imgs, gts, K, FO.Perm("s3full"), want_grads=True)

    class Keys:
        def __init__(self, tag):
            self.perm = FO.Perm(tag)

        def next_seed(self):
            from oracle import detgen
            k = self.perm.k
            self.perm.k += 1
            return detgen.fnv1a64(f"{self.perm.tag}perm{k}")
    model = TwoStagePseudoLabGeneralizedRCNN(num_classes=K, compute_dtype=torch.float32, sampler=Keys("s3full")).cuda()
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in P.items():
            sd[k].copy_(torch.from_numpy(v))
    model.train()
    data = []
    for img, (b, c), (h, w) in zip(imgs, gts, sizes):
        inst = Instances((h, w)); inst.gt_boxes = Boxes(torch.from_numpy(b).cuda()); inst.gt_classes = torch.from_numpy(c).cuda()
        data.append({"image": torch.from_numpy(img).cuda(), "height": h, "width": w, "instances": inst})
    losses, _, _, _ = model(data, branch="supervised")
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for k in ("loss_rpn_cls", "loss_rpn_loc"):
        assert abs(float(losses[k]) - ref[k]) <= 1e-4 * abs(ref[k]), (k, float(losses[k]), ref[k])
    lab = model.proposal_generator.last_labels.cpu().numpy()
    for i in range(2):
        assert np.array_equal(lab[i], aux["rpn_labels"][i]), i
    unmatched = 0
    for i in range(2):
        s = model.roi_heads.last_sampled[i].proposal_boxes.tensor.cpu().numpy()
        want = aux["sampled"][i]["boxes"]
        assert len(s) == len(want) == 512
        d = np.abs(s[:, None, :] - want[None, :, :]).max(2)
        unmatched += int((d.min(1) > 1e-2).sum())
    assert unmatched <= 10, unmatched
    for k in ("loss_cls", "loss_box_reg"):
        assert abs(float(losses[k]) - ref[k]) <= 1e-2 * abs(ref[k]) + 1e-6, (k, float(losses[k]), ref[k], unmatched)
    named = dict(model.named_parameters())
    worst = ("", 0.0)
    for k in ("backbone.bottom_up.res3.0.conv1.weight", "backbone.bottom_up.res5.2.conv3.weight", "backbone.fpn_lateral2.weight",
              "backbone.fpn_output5.weight", "proposal_generator.rpn_head.conv.weight", "proposal_generator.rpn_head.anchor_deltas.weight",
              "roi_heads.box_head.fc1.weight", "roi_heads.box_predictor.cls_score.weight"):
        g, got = grads[k], named[k].grad.cpu().numpy()
        err = float(np.linalg.norm(got - g) / (np.linalg.norm(g) + 1e-30))
        worst = max(worst, (k, err), key=lambda x: x[1])
        assert err <= (2e-2 if unmatched else 2e-3), (k, err, unmatched)
    print(f"stage-3 at 800x1216 / 768x1024: losses {dict((k, round(float(v), 5)) for k, v in losses.items())}, sampled ROIs not in the oracle's set: "
          f"{unmatched} of 1024, worst gradient relL2 {worst[1]:.1e} ({worst[0]})")


def test_stage3_teacher_weak_branch_at_config5_image_size_against_the_oracle():
    """The teacher's pass of config #5 at 800 x 1216 (training-mode top-k as the reference runs it, trainer.py:474-477): the 1000
    proposals as a set (1e-2 px; ulp-tied candidates may trade places at the cut), the <= 100 detections — classes, scores 1e-4,
    boxes 1e-2 px — and the pseudo labels that pass the 0.7 threshold."""
    from oracle import frcnn_oracle as FO
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN
    from sos_wsod_amd.semisup import process_pseudo_label
    K = 20
    P = FO.make_params(K, tag="s3wfull", head_scale=14.0)
    H, W = 800, 1216
    img = FO.make_image(H, W, "s3wfull0")
    props_ref, dets_ref = FO.weak_forward(P, [img], K)
    model = TwoStagePseudoLabGeneralizedRCNN(num_classes=K, compute_dtype=torch.float32).cuda()
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in P.items():
            sd[k].copy_(torch.from_numpy(v))
    model.train()
    data = [{"image": torch.from_numpy(img).cuda(), "height": H, "width": W}]
    with torch.no_grad():
        _, props, dets, _ = model(data, branch="unsup_data_weak")
    pb = props[0].proposal_boxes.tensor.cpu().numpy()
    rb = props_ref[0]["boxes"]
    assert len(pb) == len(rb) == 1000
    d = np.abs(pb[:, None, :] - rb[None, :, :]).max(2)
    assert int((d.min(1) > 1e-2).sum()) <= 5 and int((d.min(0) > 1e-2).sum()) <= 5
    want = dets_ref[0]
    got_b, got_s, got_c = dets[0].pred_boxes.tensor.cpu().numpy(), dets[0].scores.cpu().numpy(), dets[0].pred_classes.cpu().numpy()
    assert len(got_b) == len(want["pred_boxes"]) > 0
    # detections in score order; neighbours whose scores tie to 1e-6 may swap
    order_ok = np.array_equal(got_c, want["pred_classes"])
    if not order_ok:
        assert sorted(got_c.tolist()) == sorted(want["pred_classes"].tolist())
    np.testing.assert_allclose(np.sort(got_s), np.sort(want["scores"]), rtol=1e-4, atol=1e-6)
    dd = np.abs(got_b[:, None, :] - want["pred_boxes"][None, :, :]).max(2)
    assert (dd.min(1) <= 1e-2 + 1e-4 * np.abs(got_b).max()).all()
    pseudo, _ = process_pseudo_label(data, dets, 0.7, "roih")
    keep = want["scores"] > 0.7
    assert len(pseudo[0]) == int(keep.sum())
    print(f"stage-3 teacher at 800x1216: {len(got_b)} detections, {int(keep.sum())} pseudo labels above 0.7, order identical: {order_ok}")


def test_config2_bf16_backbone_backward_teacher_forced_against_the_oracle():
    """The bf16 conv backward — the benchmarked mode's data-gradient / weight-gradient / pool-routing kernels at config #2's
    real size — isolated against the ORACLE (vgg.py:104-122 through autograd on the host): the bf16-emulating oracle runs the
    whole config-#2 iteration, and its OWN stored activations (plain2's pooled output .. conv5_3, both backbone calls) and its
    OWN gradient at the backbone's output are fed to `VGG16`'s explicit backward.  Teacher forcing at the backbone boundary, as
    test_gpu_e2e.py does at fc7: ReLU masks, pool routes and the incoming gradient are the oracle's, so the chaos floor of two
    free-running bf16 evaluations (5-19 % per tensor) is gone and what is left is the kernels' own arithmetic: every
    plain3..plain5 weight / bias gradient within 2e-2 relative L2 and cosine >= 0.999 of the oracle's."""
    from types import SimpleNamespace
    from helpers import build_model, load_params
    from sos_wsod_amd.backbone_vgg import _VGGFunction
    K, R, H, W, dan = 20, 2000, 512, 512, (4096, 4096)
    nthreads = torch.get_num_threads()
    P = O.make_params(K, dan, tag="pcfg2", head_scale=30.0)
    views, gt = O.make_views(H, W, R, n_gt=3, K=K, scale2=1.0, tag="vcfg2")
    masks = O.make_masks(R, dan, tag="mcfg2")
    trace = {}
    _, _, og = O.oicr_plus_iteration(P, views, gt, masks, K=K, bf16=True, want_grads=True, trace=trace)
    model = build_model(K, dan, torch.bfloat16)
    load_params(model, P)
    bb = model.backbone
    bb.stage_all_weights(with_dgrad=True)
    dev = torch.device("cuda", 0)

    def nhwc(a):                                     # the oracle's stored activations are bf16 values held in f32: lossless
        t = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).to(dev)
        tb = t.to(torch.bfloat16)
        assert torch.equal(tb.float(), t), "the bf16-emulating oracle must store bf16-representable activations"
        return tb

    infos, gs = [], []
    for c in (0, 1):
        acts = trace["acts"][c]
        stage_info = []
        prev = None
        for si, (stage, cin, cout, nconv, pool_stride, dil) in enumerate(O.VGG_CFG):
            if si < 2:                               # frozen stages (FREEZE_AT 2): the backward never reads them
                stage_info.append(([(torch.empty(0, dtype=torch.bfloat16, device=dev), None)], None))
                prev = nhwc(acts["plain2"]) if si == 1 else None
                continue
            conv_io, cur = [], prev
            for i in range(nconv):
                out = nhwc(acts[f"backbone.{stage}.0.conv{i + 1}"])
                conv_io.append((cur, out))
                cur = out
            pre_pool = cur if pool_stride is not None else None
            stage_info.append((conv_io, pre_pool))
            prev = nhwc(acts[stage])
        infos.append(stage_info)
        g = torch.from_numpy(np.ascontiguousarray(trace["dfeat"][c].transpose(0, 2, 3, 1))).to(dev)      # f32: the backward rounds it
        gs.append(g)
    params = tuple(bb._flat_params())
    ctx = SimpleNamespace(module=bb, infos=infos, params=params)
    res = _VGGFunction.backward(ctx, *gs)
    torch.cuda.synchronize()
    grads = res[2 + len(gs):]
    names = [n for blk_name, _, _, nconv, _, _ in O.VGG_CFG for i in range(nconv)
             for n in (f"backbone.{blk_name}.0.conv{i + 1}.weight", f"backbone.{blk_name}.0.conv{i + 1}.bias")]
    rows, bad = [], []
    for name, got in zip(names, grads):
        if name.startswith(("backbone.plain1", "backbone.plain2")):
            assert got is None
            continue
        a, b = got.double().cpu().numpy().ravel(), np.asarray(og[name], np.float64).ravel()
        rel = float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))
        cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))
        rows.append((name, rel, cos))
        if not (rel <= 2e-2 and cos >= 0.999):
            bad.append((name, rel, cos))
    print("bf16 conv backward, teacher forced at the backbone boundary (config #2): name | rel L2 | cosine")
    for n, r, c in rows:
        print("   %-40s %.3e %.6f" % (n, r, c))
    assert len(rows) == 18 and not bad, bad
    torch.set_num_threads(nthreads)


@pytest.mark.parametrize("M", [8000, 16000])
def test_config2_bf16_fc6_dgrad_and_wgrad_isolated_against_float64(M):
    """(M = 16000: BASELINE config #4's row count, 4 views x 4000 ROIs — round 6.)  The fc6 pair of the backward at BASELINE config #2's size (M = 4 x 2000 ROIs, 25088 -> 4096), each GEMM ALONE and in the exact
    launch form the heads use (roi_heads_oicrplus._train_backward_fc6 / _train_backward_pool: data gradient = NT on the transposed weight
    copy with the |max| epilogue, weight gradient = transpose of dZ + NN GEMM with the tail peel) against a float64 contraction of the SAME
    bf16 operands on the host.  The conv family has such a check (…backbone_backward_teacher_forced…); the end-to-end bf16 tests only bound
    these two through the 5-19 % chaos floor of two free-running bf16 evaluations.  What is left here is the kernels' own arithmetic:
    f32 accumulation over K = 4096 / 8000 and the one rounding of a bf16 output.  Operands as in training: pooled >= 0 with zeros,
    dZ masked by ReLU x dropout (75 % zeros) with a heavy-tailed scale per row."""
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd.roi_heads_oicrplus import _padded
    dev = torch.device("cuda", 0)
    D0, D1 = 25088, 4096
    g = torch.Generator(device="cpu").manual_seed(11)
    bf = torch.bfloat16
    pooled = _padded(M, D0, dev, bf, pad=64)
    dz1 = _padded(M, D1, dev, bf)
    W1T = _padded(D0, D1, dev, bf)
    for r0 in range(0, M, 1000):                                         # filled in row blocks: the host side stays small
        x = torch.randn(1000, D0, generator=g).clamp_(min=0) * (0.5 + torch.rand(1000, 1, generator=g) * 3)
        pooled[r0:r0 + 1000] = x.to(bf).to(dev)
        z = torch.randn(1000, D1, generator=g) * torch.exp(torch.randn(1000, 1, generator=g) * 2.0) * 1e-4
        z = z * (torch.rand(1000, D1, generator=g) < 0.25)
        dz1[r0:r0 + 1000] = z.to(bf).to(dev)
    for r0 in range(0, D0, 3136):
        W1T[r0:r0 + 3136] = (torch.randn(3136, D1, generator=g) * 0.005).to(bf).to(dev)
    # ---- data gradient: dpooled = dZ1 . W1  (M x D0, K = D1), bf16 out, max|.| in the epilogue
    dpooled = _padded(M, D0, dev, bf, pad=64)
    amax = ops.fill_zero(torch.empty(1, device=dev, dtype=torch.float32))
    ops.gemm(dz1, W1T, dpooled, M, D0, D1, ep=ops.make_epilogue(out_dtype=bf, absmax_out=amax))
    # ---- weight gradient: dW1 = dZ1^T . pooled  (D1 x D0, K = M), f32 out
    dW1 = torch.empty(D1, D0, device=dev, dtype=torch.float32)
    dzt = ops.transpose_2d(dz1, torch.empty(D1, M + 64, device=dev, dtype=bf)[:, :M], M, D1)
    ops.gemm(dzt, pooled, dW1, D1, D0, M, b_kstrided=True)
    torch.cuda.synchronize()
    rows_m = torch.tensor(sorted({0, 1, 255, 256, 4095, 4096, M - 1} | {int(v) for v in torch.randint(0, M, (41,), generator=g)}))
    rows_o = torch.tensor(sorted({0, 255, 256, 2047, 4095} | {int(v) for v in torch.randint(0, D1, (43,), generator=g)}))
    W64 = W1T.cpu().double()                                             # (D0, D1)
    ref_d = dz1[rows_m.to(dev)].cpu().double() @ W64.t()                 # (48, D0)
    got_d = dpooled[rows_m.to(dev)].cpu().double()
    err = (got_d - ref_d).abs()
    # one bf16 rounding of the output (2^-9 relative) + f32 accumulation over K = 4096 (~1e-6 of the row's scale; bar 1e-5)
    scale = ref_d.abs().amax(dim=1, keepdim=True)
    assert bool((err <= ref_d.abs() * 2.0 ** -8 + scale * 1e-5).all()), float((err / (ref_d.abs() * 2.0 ** -8 + scale * 1e-5)).max())
    rel_d = float((got_d - ref_d).norm() / ref_d.norm())
    assert rel_d <= 3e-3, rel_d
    want_max = float((dz1.cpu().double() @ W64[:64].t()).abs().max())   # the |max| epilogue sees every element; checked on a slab it must dominate
    assert float(amax.item()) >= want_max * (1 - 2.0 ** -8)
    del W64
    dzs = dz1[:, rows_o.to(dev)].cpu().double().t().contiguous()         # (48, M)
    rel_w, worst = 0.0, 0.0
    num = den = 0.0
    for c0 in range(0, D0, 3584):
        ref = dzs @ pooled[:, c0:c0 + 3584].cpu().double()               # (48, 3584)
        got = dW1[rows_o.to(dev), c0:c0 + 3584].cpu().double()
        d = got - ref
        num += float((d * d).sum()); den += float((ref * ref).sum())
        worst = max(worst, float((d.abs() / ref.abs().amax(dim=1, keepdim=True)).max()))
    rel_w = (num / den) ** 0.5
    # f32 output, f32 accumulation over K = M in a fixed tile / split order (incl. the last 512 columns: the split-K tail peel)
    assert rel_w <= 1e-5 and worst <= 1e-5, (rel_w, worst)                      # (a bf16-sized error would be 4e-3)
    print(f"fc6 alone, bf16 operands vs float64: dgrad rel-L2 {rel_d:.2e} (bf16 out), wgrad rel-L2 {rel_w:.2e}, worst element / row max {worst:.2e}")


def test_config4_bf16_conv5_forward_dgrad_wgrad_at_99x165_against_float64():
    """BASELINE config #4's conv5 layers ALONE (round 6): 512 -> 512 channels, dilation 2, on the 99 x 165 map of an 800 x 1333 view pair —
    the direct kernel's four-wave form with ragged right-edge tiles (165 = 5 x 32 + 5: the LEFT edge form) forward and as the data
    gradient (flipped weights, ReLU mask from a reference map), and the direct weight-gradient kernel through the grouped entry with the
    backbone's own split plan — each against a float64 convolution of the SAME bf16 operands, on a subset of output channels (forward,
    weight gradient) / input channels (data gradient) the host can afford.  Operands as in training: inputs >= 0 with zeros, gradients
    masked (half zeros) with a heavy-tailed scale per pixel.  What is left is the kernels' own arithmetic: f32 accumulation over K = 4608
    (32 670 pixels for the weights) and one bf16 rounding of a bf16 output."""
    import torch.nn.functional as F
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd.wgrad import wgrad_direct_splits
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    n, H, W, C, dil = 2, 99, 165, 512, 2
    g = torch.Generator(device="cpu").manual_seed(23)
    x = (torch.randn(n, H, W, C, generator=g).clamp_(min=0) * (0.5 + 2 * torch.rand(n, H, W, 1, generator=g))).to(bf)
    w = (torch.randn(C, C, 3, 3, generator=g) * 0.02).to(bf)                                       # OIHW
    dy = (torch.randn(n, H, W, C, generator=g) * torch.exp(torch.randn(n, H, W, 1, generator=g) * 1.5) * 1e-3
          * (torch.rand(n, H, W, C, generator=g) < 0.5)).to(bf)
    bias = torch.randn(C, generator=g) * 0.1
    sub = torch.tensor(sorted({0, 63, 64, 511} | {int(v) for v in torch.randint(0, C, (12,), generator=g)}))
    xd, dyd, wd = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2), w.double()
    xg, dyg = x.to(dev), dy.to(dev)
    # ---- forward (+ bias + ReLU), bf16 out
    wk = torch.empty(C, 9, C, device=dev, dtype=bf); ops.conv_weight_prep(w.float().to(dev), wk, 0, C)
    out = torch.empty(n, H, W, C, device=dev, dtype=bf)
    ops.conv3x3(xg, wk, out, dil, ops.make_epilogue(bias=bias.to(dev), relu=True, out_dtype=bf))
    ref = F.relu(F.conv2d(xd, wd[sub], bias.double()[sub], padding=dil, dilation=dil)).permute(0, 2, 3, 1)      # (n, H, W, 16)
    got = out[..., sub.to(dev)].cpu().double()
    scale = ref.abs().amax()
    assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -8 + scale * 1e-5).all())
    rel_f = float((got - ref).norm() / ref.norm())
    assert rel_f <= 3e-3, rel_f
    # ---- data gradient: the same kernel on the flipped / transposed weight copy, masked by (x > 0)
    wkd = torch.empty(C, 9, C, device=dev, dtype=bf); ops.conv_weight_prep(w.float().to(dev), wkd, 1)
    dx = torch.empty(n, H, W, C, device=dev, dtype=bf)
    ops.conv3x3(dyg, wkd, dx, dil, ops.make_epilogue(relu_ref=xg.view(n * H * W, C), out_dtype=bf))
    wflip = wd.transpose(0, 1).flip(2, 3)                                                           # [ci][co][2-ky][2-kx]
    refd = F.conv2d(dyd, wflip[sub], None, padding=dil, dilation=dil).permute(0, 2, 3, 1) * (x[..., sub].double() > 0)
    gotd = dx[..., sub.to(dev)].cpu().double()
    scale = refd.abs().amax()
    assert bool(((gotd - refd).abs() <= refd.abs() * 2.0 ** -8 + scale * 1e-5).all())
    rel_d = float((gotd - refd).norm() / refd.norm())
    assert rel_d <= 3e-3, rel_d
    # ---- weight gradient: the grouped entry (direct kernel) with the backbone's split plan + the ordered fold, f32 out
    ns = wgrad_direct_splits([(n, H, W, C, C, dil)])[0]
    nslab = ops.conv3x3_wgrad_nslab(xg, C, ns)
    slabs = torch.empty(nslab, C * 9 * C, device=dev)
    ops.conv3x3_wgrad_grouped([(xg, dyg, slabs, dil, ns)])
    dw = torch.empty(C, C, 3, 3, device=dev)
    ops.conv3x3_wgrad_fold(slabs, nslab, dw)
    wsub = torch.zeros(len(sub), C, 3, 3, dtype=torch.float64, requires_grad=True)
    refw = torch.autograd.grad(F.conv2d(xd, wsub, None, padding=dil, dilation=dil), wsub, dyd[:, sub])[0]
    gotw = dw[sub.to(dev)].cpu().double()
    rel_w = float((gotw - refw).norm() / refw.norm())
    worst = float(((gotw - refw).abs().flatten(1).amax(1) / refw.abs().flatten(1).amax(1)).max())
    assert rel_w <= 2e-5 and worst <= 2e-5, (rel_w, worst)                      # (a bf16-sized error would be 4e-3)
    print(f"conv5 at 99x165 alone, bf16 operands vs float64: fwd rel-L2 {rel_f:.2e}, dgrad {rel_d:.2e} (bf16 out), wgrad {rel_w:.2e} "
          f"(worst row {worst:.2e}), {nslab} slab(s)")

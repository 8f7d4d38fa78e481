"""GPU: the SoS-WSOD+ detectors (sos_plus_wo_imagenet_test.yaml "woi", sos_plus_test.yaml "plus"): the column-matrix convolution
node against the existing stride-1 kernels and against float64 F.conv2d, the torchvision-style bottleneck block against a float64
restatement, both models against fixtures written by RUNNING the reference's own GeneralizedRCNN (tests/golden/
make_sosplus_golden.py) with the comparison rules and bars of the eval and supervised fixture tests of tests/test_gpu_stage3.py,
bf16 losses against the fp32 fixtures at that file's bf16 bars, and the default-argument model bit for bit against
TwoStagePseudoLabGeneralizedRCNN.

Bars of the node tests: fp32 3e-5 of max|ref| (what test_gpu_stage3.py holds its stride-1 node to); bf16 2^-7 of max|ref| (an f32
sum rounded to bf16, at most twice on the data-gradient path: dcol, then dx)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import sosplus_ref as SP  # noqa: E402

BAR = {torch.float32: 3e-5, torch.bfloat16: 2.0 ** -7}
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def fr():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.frcnn as fr
    assert torch.cuda.is_available()
    return fr


def _err(got, ref):
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _rand(g, *shape, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _stage3x3(w_oihw, scale, dtype):
    """the staged [co][tap][ci] copy of w * scale in the compute dtype (what sw_stage_weights_multi kind 1 writes)"""
    w = w_oihw if scale is None else w_oihw * scale.view(-1, 1, 1, 1)
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).to(dtype).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 13, 10, 128, 128), (1, 25, 38, 64, 64), (3, 8, 8, 32, 72)], ids=lambda s: "x".join(map(str, s)))
def test_stride2_forward_equals_stride1_kernel_subsampled(fr, dtype, shape):
    """the same numbers from existing kernels: conv3x3 at stride 1 (bias + ReLU fused), then every other pixel"""
    import sos_wsod_amd.ops as ops
    n, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(5)
    x = _rand(g, n, H, W, cin, dtype=dtype)
    w = torch.nn.Parameter(_rand(g, cout, cin, 3, 3, scale=(9 * cin) ** -0.5))
    shift = _rand(g, cout, scale=0.3)
    st = _stage3x3(w.detach(), None, dtype)
    with torch.no_grad():
        got = fr._Conv3x3ColFn.apply(x, st, shift, None, True, 2, w, None)
        full = ops.conv3x3(x, st, torch.empty(n, H, W, cout, device="cuda", dtype=dtype), 1, ops.make_epilogue(bias=shift, relu=True, out_dtype=dtype))
        ref = ops.subsample2x(full, torch.empty(n, (H + 1) // 2, (W + 1) // 2, cout, device="cuda", dtype=dtype))
    torch.cuda.synchronize()
    assert got.shape == ref.shape
    e = _err(got, ref)
    print(f"stride-2 column node vs conv3x3 + subsample2x [{dtype}] {shape}: {e:.2e} of max|ref| (bar {BAR[dtype]:.1e})")
    assert e <= BAR[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(5, 7, 7, 256, 256, 1, True), (2, 13, 10, 128, 128, 2, False), (3, 9, 12, 64, 136, 2, True)],
                         ids=["roi7x7-stride1-chunked", "odd-map-stride2", "stride2-bias"])
def test_column_node_against_float64_conv2d(fr, monkeypatch, dtype, case):
    """forward, data gradient (input mask off and on), weight gradient (x FrozenBN scale) and bias gradient against float64 F.conv2d
    on the node's own rounded operands; the ReLU mask of the reference is taken from the node's stored output, which defines it.
    "chunked": COL_CHUNK_BYTES lowered so that the 5 maps are walked in 3 passes (3 slabs in the fold)."""
    n, H, W, cin, cout, stride, with_bias = case
    g = torch.Generator().manual_seed(7)
    if stride == 1:
        monkeypatch.setattr(fr, "COL_CHUNK_BYTES", 2 * H * W * 9 * cin * (2 if dtype == torch.bfloat16 else 4))
        assert len(fr._Conv3x3ColFn._chunks(n, H * W, cin, 2 if dtype == torch.bfloat16 else 4)) == 3
    x = _rand(g, n, H, W, cin, dtype=dtype).requires_grad_(True)
    w = torch.nn.Parameter(_rand(g, cout, cin, 3, 3, scale=(9 * cin) ** -0.5))
    b = torch.nn.Parameter(_rand(g, cout, scale=0.3)) if with_bias else None
    scale = None if with_bias else (torch.rand(cout, generator=g) + 0.5).cuda()
    shift = b.detach() if with_bias else _rand(g, cout, scale=0.3)
    st = _stage3x3(w.detach(), scale, dtype)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gy = _rand(g, n, Ho, Wo, cout, dtype=dtype)
    for mask_in in (False, True):
        x.grad = w.grad = None
        if b is not None:
            b.grad = None
        y = fr._Conv3x3ColFn.apply(x, st, shift, scale, fr._RELU | (fr._MASK_INPUT_GRAD if mask_in else 0), stride, w, b)
        y.backward(gy)
        torch.cuda.synchronize()
        # ---- float64 on the rounded operands
        x64 = x.detach().double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
        w64 = st.double().cpu().view(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        z = F.conv2d(x64, w64, shift.double().cpu(), stride=stride, padding=1)
        fwd_ref = z.clamp_min(0).permute(0, 2, 3, 1)
        gs = (gy.double().cpu() * (y.detach().double().cpu() > 0)).permute(0, 3, 1, 2)
        z.backward(gs)
        dx_ref = x64.grad.permute(0, 2, 3, 1)
        if mask_in:
            dx_ref = dx_ref * (x.detach().double().cpu() > 0)
        dw_ref = w64.grad if scale is None else w64.grad * scale.double().cpu().view(-1, 1, 1, 1)
        errs = {"forward": _err(y.detach(), fwd_ref), "dgrad": _err(x.grad, dx_ref), "wgrad": _err(w.grad, dw_ref)}
        if b is not None:
            errs["bgrad"] = _err(b.grad, gs.sum((0, 2, 3)))
        print(f"column node [{dtype}] {case} mask_in={mask_in}:", {k: "%.2e" % v for k, v in errs.items()}, f"bar {BAR[dtype]:.1e}")
        assert y.dtype == dtype and x.grad.dtype == dtype and w.grad.dtype == torch.float32 and w.grad.shape == w.shape
        assert all(v <= BAR[dtype] for v in errs.values()), errs


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_weight_used_twice_inside_grad_scope_sums_in_the_fold(fr, dtype):
    """the student uses each parameter twice per iteration: inside wgrad.grad_scope the second node adds to the first one's buffer
    (no torch add), and the sum equals the two gradients computed apart"""
    from sos_wsod_amd import wgrad
    g = torch.Generator().manual_seed(9)
    cin, cout = 64, 64
    w = torch.nn.Parameter(_rand(g, cout, cin, 3, 3, scale=(9 * cin) ** -0.5))
    b = torch.nn.Parameter(_rand(g, cout, scale=0.3))
    st = _stage3x3(w.detach(), None, dtype)
    xs = [_rand(g, 2, 9, 7, cin, dtype=dtype), _rand(g, 1, 14, 12, cin, dtype=dtype)]
    gys = [_rand(g, 2, 5, 4, cout, dtype=dtype), _rand(g, 1, 7, 6, cout, dtype=dtype)]

    def run(parts):
        w.grad = b.grad = None
        ys = [fr._Conv3x3ColFn.apply(xs[i], st, b.detach(), None, True, 2, w, b) for i in parts]
        torch.autograd.backward(ys, [gys[i] for i in parts])
        torch.cuda.synchronize()
        return w.grad.clone(), b.grad.clone()
    apart = [run([0]), run([1])]
    with wgrad.grad_scope():
        both = run([0, 1])
        wgrad.finish()
    for k, name in enumerate(("weight", "bias")):
        e = _err(both[k], apart[0][k].double() + apart[1][k].double())
        print(f"two uses inside grad_scope [{dtype}] {name}: {e:.2e}")
        assert e <= 1e-6                                                             # f32 sums of the same f32 terms


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_box_head_with_convolutions_takes_zero_and_one_roi(fr, dtype):
    """an image without proposals: the 4conv1fc head returns (0, fc_dim) and its backward runs; one ROI alone gives what it gives in a batch"""
    import sos_wsod_amd.ops as ops
    torch.manual_seed(2)
    head = fr.FastRCNNConvFCHead(conv_dims=(16, 16), fc_dims=(24,), conv_norm="FrozenBN", in_channels=8).cuda()
    ops.StagePlan([e for m in head.modules() if hasattr(m, "_stage_entries") for e in m._stage_entries(dtype)], dtype).run()
    x0 = torch.zeros(0, 8 * 49, device="cuda", dtype=dtype, requires_grad=True)
    y0 = head(x0)
    assert tuple(y0.shape) == (0, 24)
    y0.sum().backward()
    assert tuple(x0.grad.shape) == (0, 8 * 49) and float(head.conv1.weight.grad.abs().sum()) == 0.0
    x = torch.randn(3, 8 * 49, device="cuda").to(dtype)
    with torch.no_grad():
        assert _err(head(x[1:2].contiguous()), head(x)[1:2]) <= BAR[dtype]


def _block_ref(blk, x, dtype):
    """float64 restatement of the torchvision-style stride-2 bottleneck (resnet.py:195-213 with stride_in_1x1 = False): every layer's
    input and effective weight rounded to the compute dtype as the product stores them, sums in float64"""
    def q(t):
        return t.to(dtype).double()

    def conv(m, t, stride, pad):
        scale, shift = m.norm.fold()
        w = q((m.weight.detach() * scale.view(-1, 1, 1, 1)).cpu())
        return F.conv2d(t, w, shift.double().cpu(), stride=stride, padding=pad)
    t = x.detach().double().cpu().permute(0, 3, 1, 2)
    h = q(conv(blk.conv1, t, 1, 0).clamp_min(0))
    h = q(conv(blk.conv2, h, 2, 1).clamp_min(0))
    sc = q(conv(blk.shortcut, t, 2, 0))
    return (conv(blk.conv3, h, 1, 0) + sc).clamp_min(0).permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_torchvision_style_block_against_float64(fr, dtype):
    import sos_wsod_amd.ops as ops
    g = torch.Generator().manual_seed(11)
    cin, mid, cout = 64, 32, 128
    blk = fr.BottleneckBlock(cin, cout, mid, 2, stride_in_1x1=False).cuda()
    assert blk.stride_in_3x3 and (blk.conv1.stride, blk.conv2.stride, blk.shortcut.stride) == (1, 2, 2)
    convs = [blk.conv1, blk.conv2, blk.conv3, blk.shortcut]
    with torch.no_grad():
        for c in convs:
            c.norm.weight.copy_(torch.rand(c.norm.weight.shape, generator=g) + 0.5)
            c.norm.bias.copy_(torch.randn(c.norm.bias.shape, generator=g) * 0.1)
            c.norm.running_var.copy_(torch.rand(c.norm.weight.shape, generator=g) + 0.5)
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) / (c.weight[0].numel() ** 0.5))
    ops.StagePlan([e for c in convs for e in c._stage_entries(dtype)], dtype).run()
    x = _rand(g, 2, 13, 18, cin, dtype=dtype).requires_grad_(True)
    y = blk(x)
    assert tuple(y.shape) == (2, 7, 9, cout)
    ref = _block_ref(blk, x, dtype)
    e = _err(y.detach(), ref)
    print(f"torchvision-style block forward [{dtype}]: {e:.2e} of max|ref| (bar {BAR[dtype]:.1e})")
    assert e <= BAR[dtype]
    # gradients: float64 autograd through the same restatement without the roundings (they have no gradient), at fp32 only
    if dtype == torch.float32:
        gy = _rand(g, 2, 7, 9, cout)
        y.backward(gy)
        torch.cuda.synchronize()
        ws = [c.weight.detach().double().cpu().requires_grad_(True) for c in convs]
        t = x.detach().double().cpu().permute(0, 3, 1, 2).requires_grad_(True)

        def conv(i, inp, stride, pad):
            scale, shift = convs[i].norm.fold()
            return F.conv2d(inp, ws[i] * scale.double().cpu().view(-1, 1, 1, 1), shift.double().cpu(), stride=stride, padding=pad)
        h = conv(1, conv(0, t, 1, 0).clamp_min(0), 2, 1).clamp_min(0)
        out = (conv(2, h, 1, 0) + conv(3, t, 2, 0)).clamp_min(0)
        out.backward(gy.double().cpu().permute(0, 3, 1, 2))
        errs = {"dx": _err(x.grad, t.grad.permute(0, 2, 3, 1))}
        for name, c, w64 in zip(("conv1", "conv2", "conv3", "shortcut"), convs, ws):
            errs[name] = _err(c.weight.grad, w64.grad)
        print("torchvision-style block gradients [fp32]:", {k: "%.2e" % v for k, v in errs.items()})
        assert all(v <= BAR[dtype] for v in errs.values()), errs


# ------------------------------------------------------------------------------------------ the two detectors against the reference's runs
def _model(variant, P, tag, dtype="fp32"):
    from sos_wsod_amd.config import add_wsl_config, get_cfg
    from sos_wsod_amd.rcnn_multi import build_model
    cfg = add_wsl_config(get_cfg())
    cfg.merge_from_list(SP.cfg_list(variant, device="cuda", dtype=dtype))
    m = build_model(cfg)
    m.sampler = m.proposal_generator.sampler = m.roi_heads.sampler = SP.Keys(tag)
    sd = m.state_dict()
    assert set(sd) == set(P)
    with torch.no_grad():
        for k, v in P.items():
            assert tuple(sd[k].shape) == tuple(v.shape), k
            sd[k].copy_(torch.from_numpy(v))
    return m


def _inputs(tag, with_gt):
    from sos_wsod_amd.structures import Boxes, Instances
    data, gts = [], SP.ground_truth(tag)
    for i, ((h, w), img) in enumerate(zip(SP.SIZES, SP.images(tag))):
        d = {"image": torch.from_numpy(img).cuda(), "height": h, "width": w}
        if with_gt:
            b, c = gts[i]
            inst = Instances((h, w)); inst.gt_boxes = Boxes(torch.from_numpy(b).cuda()); inst.gt_classes = torch.from_numpy(c).cuda()
            d["instances"] = inst
        data.append(d)
    return data, gts


@pytest.mark.parametrize("variant", SP.VARIANTS)
def test_eval_mode_matches_the_reference_run(golden_dir, variant):
    """the rules and bars of test_gpu_stage3.test_eval_mode_inference_rescales_to_the_dataset_frame_like_the_reference; every
    detection is compared (the fixture keeps its scores 1e-3 away from the threshold and its IoUs 1e-3 away from the NMS threshold)"""
    t = np.load(os.path.join(golden_dir, f"sosplus_{variant}_e.npz"))
    assert float(t["score_margin"]) > 1e-3 and float(t["iou_margin"]) > 1e-3
    tag = f"sp{variant}e"
    model = _model(variant, SP.make_params(variant, tag, float(t["head_scale"]), float(t["bg_bias"])), tag)
    model.eval()
    data, _ = _inputs(tag, with_gt=False)
    for d, (oh, ow) in zip(data, t["out_sizes"]):
        d["height"], d["width"] = int(oh), int(ow)
    res = model(data)
    raw = model.inference(data, do_postprocess=False)
    for i, r in enumerate(res):
        inst = r["instances"]
        print(f"sosplus {variant} eval image {i}: {len(inst)} detections (fixture {len(t[f'det_scores{i}'])})")
        assert tuple(inst.image_size) == tuple(int(v) for v in t["out_sizes"][i])
        assert np.array_equal(inst.pred_classes.cpu().numpy(), t[f"det_classes{i}"])
        np.testing.assert_allclose(inst.scores.cpu().numpy(), t[f"det_scores{i}"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(inst.pred_boxes.tensor.cpu().numpy(), t[f"det_boxes{i}"], rtol=1e-4, atol=1e-2)
        np.testing.assert_allclose(raw[i].pred_boxes.tensor.cpu().numpy(), t[f"raw_boxes{i}"], rtol=1e-4, atol=1e-2)


def _train_step(variant, t, dtype="fp32"):
    tag = f"sp{variant}a"
    model = _model(variant, SP.make_params(variant, tag, float(t["head_scale"])), tag, dtype=dtype)
    model.train()
    data, gts = _inputs(tag, with_gt=True)
    losses = model(data)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return model, losses, gts


@pytest.mark.parametrize("variant", SP.VARIANTS)
def test_training_step_matches_the_reference_run(golden_dir, variant):
    """the rules and bars of test_gpu_stage3.test_supervised_branch_matches_the_reference_generated_fixture: labels and sampled
    classes bit exact; a sampled box that is not the fixture's must be a fixture proposal (near-tied objectness logits may swap two
    proposals, at most 2 of 512 rows); losses 1e-4 (1e-3 for the ROI losses when rows were exchanged), gradients 2e-3 (5e-3)"""
    t = np.load(os.path.join(golden_dir, f"sosplus_{variant}_a.npz"))
    model, losses, gts = _train_step(variant, t)
    assert isinstance(losses, dict) and set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}
    lab = model.proposal_generator.last_labels.cpu().numpy()
    swapped, keep_rows = 0, []
    for i in range(2):
        assert np.array_equal(lab[i], t[f"rpn_labels{i}"]), i
        s = model.roi_heads.last_sampled[i]
        assert np.array_equal(s.gt_classes.cpu().numpy(), t[f"samp_classes{i}"]), i
        got, want = s.proposal_boxes.tensor.cpu().numpy(), t[f"samp_boxes{i}"]
        same = np.abs(got - want).max(1) <= 1e-2
        pool = np.concatenate([t[f"prop_boxes{i}"], gts[i][0]], 0)
        for r in np.nonzero(~same)[0]:
            assert np.abs(pool - got[r]).max(1).min() <= 1e-2, (i, r, got[r])
        assert (~same).sum() <= 2, (i, int((~same).sum()))
        swapped += int((~same).sum())
        keep_rows.append(same)
    keep_rows = np.concatenate(keep_rows)
    rel = {}
    for k, v in losses.items():
        ref = float(t["loss/" + k])
        rel[k] = abs(float(v) - ref) / abs(ref)
    print(f"sosplus {variant} training step: relative loss errors {dict((k, '%.1e' % v) for k, v in rel.items())}; exchanged rows {swapped}")
    for k, v in rel.items():
        assert v <= (1e-4 if (swapped == 0 or k.startswith("loss_rpn")) else 1e-3), (k, v, swapped)
    K1 = SP.K + 1
    lg = model.roi_heads.last_logits.detach().cpu().numpy()
    np.testing.assert_allclose(lg[keep_rows, :K1], t["scores"][keep_rows], rtol=1e-3, atol=1e-3)
    sd = dict(model.named_parameters())
    worst, n_checked = ("", 0.0), 0
    for key in t.files:
        if key.startswith("grad/"):
            ref, got = t[key], sd[key[5:]].grad.cpu().numpy()
        elif key.startswith("grads/"):
            ref, got = t[key], sd[key[6:]].grad.cpu().numpy().ravel()[::SP.STRIDE]
        else:
            continue
        n_checked += 1
        err = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
        worst = max(worst, (key, err), key=lambda x: x[1])
        assert err <= (2e-3 if swapped == 0 else 5e-3), (key, err, swapped)
    assert n_checked == len(SP.GRAD_FULL) + len(SP.GRAD_SAMPLED) + (len(SP.GRAD_SAMPLED_PLUS) if variant == "plus" else 0)
    for name in t["frozen"]:
        assert sd[str(name)].grad is None
    print(f"sosplus {variant} training step: {n_checked} gradients, worst error {worst[1]:.1e} ({worst[0]})")


@pytest.mark.parametrize("variant", SP.VARIANTS)
def test_bf16_losses_stay_close_to_the_fp32_fixture(golden_dir, variant):
    """the bars of test_gpu_stage3.test_supervised_branch_bf16_mode_stays_close_to_the_fp32_fixture"""
    t = np.load(os.path.join(golden_dir, f"sosplus_{variant}_a.npz"))
    model, losses, _ = _train_step(variant, t, dtype="bf16")
    rel = {k: abs(float(v) - float(t["loss/" + k])) / abs(float(t["loss/" + k])) for k, v in losses.items()}
    print(f"sosplus {variant} bf16 vs the fp32 fixture, relative loss differences:", {k: "%.1e" % v for k, v in rel.items()})
    assert rel["loss_rpn_cls"] <= 1e-2 and rel["loss_rpn_loc"] <= 1e-2, rel
    assert rel["loss_cls"] <= 5e-2 and rel["loss_box_reg"] <= 1e-1, rel
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.requires_grad)


def test_two_batches_inside_grad_scope_equal_two_plain_calls(fr):
    """the student's iteration: two batches through one call of the base class (`second=`: this backbone form runs them one after
    the other, forward_lockstep falls back) inside wgrad.grad_scope, every parameter used twice — against two plain calls whose
    gradients autograd adds.  fp32, the bars of test_gpu_stage3.test_student_passes_in_lockstep_equal_two_calls: losses 1e-5,
    gradients 1e-4 of the tensor's largest element."""
    from sos_wsod_amd import wgrad
    variant, tag = "plus", "spplusa"
    P = SP.make_params(variant, tag, 4.0)
    res = []
    for scoped in (True, False):
        model = _model(variant, P, tag)
        model.train()
        a, _ = _inputs(tag, with_gt=True)
        b, _ = _inputs("spwoia", with_gt=True)
        if scoped:
            with wgrad.grad_scope():
                ra, rb = fr.TwoStagePseudoLabGeneralizedRCNN.forward(model, a, branch="supervised", second=b)
                la, lb = ra[0], rb[0]
                (sum(la.values()) + sum(lb.values())).backward()
                wgrad.finish()
        else:
            la, lb = model(a), model(b)
            (sum(la.values()) + sum(lb.values())).backward()
        torch.cuda.synchronize()
        res.append(([float(v) for d in (la, lb) for _, v in sorted(d.items())],
                    {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    for x, y in zip(res[0][0], res[1][0]):
        assert abs(x - y) <= 1e-5 * abs(y) + 1e-7, (res[0][0], res[1][0])
    assert set(res[0][1]) == set(res[1][1])
    worst = max(((n, float((g - res[1][1][n]).abs().max() / (res[1][1][n].abs().max() + 1e-30))) for n, g in res[0][1].items()), key=lambda t: t[1])
    print(f"two batches inside grad_scope vs two plain calls: worst gradient difference {worst[1]:.1e} ({worst[0]})")
    assert worst[1] <= 1e-4, worst


def test_default_arguments_give_the_existing_detector_bit_for_bit(fr):
    """GeneralizedRCNN built with default arguments (+ the focal loss the other class defaults to) against
    TwoStagePseudoLabGeneralizedRCNN: same parameters, same inputs, same sampler keys -> identical losses, gradients and detections"""
    from oracle import frcnn_oracle as FO
    P = FO.make_params(SP.K, tag="s3a", head_scale=5.0)
    res = []
    for cls in (fr.TwoStagePseudoLabGeneralizedRCNN, fr.GeneralizedRCNN):
        m = cls(num_classes=SP.K, sampler=SP.Keys("s3a")).cuda()
        if cls is fr.GeneralizedRCNN:
            m.roi_heads.loss, m.roi_heads.gamma = "FocalLoss", 1.5
        sd = m.state_dict()
        with torch.no_grad():
            for k, v in P.items():
                sd[k].copy_(torch.from_numpy(v))
        m.train()
        data, _ = _inputs("s3a", with_gt=True)
        out = m(data, branch="supervised")[0] if cls is fr.TwoStagePseudoLabGeneralizedRCNN else m(data)
        sum(out.values()).backward()
        m.eval()
        dets = m([{"image": d["image"]} for d in data])
        torch.cuda.synchronize()
        res.append(({k: v.detach().clone() for k, v in out.items()}, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None},
                    [(d["instances"].pred_boxes.tensor.clone(), d["instances"].scores.clone()) for d in dets]))
    (la, ga, da), (lb, gb, db) = res
    assert set(la) == set(lb) and all(torch.equal(la[k], lb[k]) for k in la)
    assert set(ga) == set(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(da, db))

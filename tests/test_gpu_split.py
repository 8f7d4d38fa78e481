"""GPU: the Stage-3 split's device side — sw_det_loss_per_image (ops.det_loss_per_image) against a float64 NumPy restatement, the
detector's CrossEntropy ROI loss and smooth_l1_mean box losses (frcnn.py), the label samplers at positive fraction 1.0, and
split.score_images: a bucketed batch scores each image as it scores alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOSSES = ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc")


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    return ops


# ------------------------------------------------------------------------------------------ the kernel
from losses_ref import det_loss_ref as _restated  # noqa: E402  (the one float64 restatement of sw_det_loss_per_image)


def _random_inputs(N, A, K, counts, zero_rpn_fg, zero_roi_fg, seed=0):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(A, 2, generator=g) * 600
    an = torch.cat([xy, xy + 8 + torch.rand(A, 2, generator=g) * 200], 1)
    lab = torch.full((N, A), -1, dtype=torch.int8)
    for n in range(N):
        pick = torch.randperm(A, generator=g)[:256]
        npos = 0 if n in zero_rpn_fg else int(torch.randint(1, 129, (1,), generator=g))
        lab[n, pick[:npos]] = 1
        lab[n, pick[npos:]] = 0
    mxy = an[None, :, :2] + torch.randn(N, A, 2, generator=g) * 10
    ma = torch.cat([mxy, mxy + 8 + torch.rand(N, A, 2, generator=g) * 200], 2)
    lo = torch.randn(N, A, generator=g) * 3
    de = torch.randn(N, A, 4, generator=g) * 0.5
    R = int(sum(counts))
    lg = torch.randn(R, 5 * K + 1 + 3, generator=g) * 2                    # (+3: a row pitch wider than 5K + 1)
    cls = torch.randint(0, K + 1, (R,), generator=g, dtype=torch.int32)
    off = 0
    for n, c in enumerate(counts):
        if n in zero_roi_fg:
            cls[off:off + c] = K
        off += c
    bxy = torch.rand(R, 2, generator=g) * 600
    bx = torch.cat([bxy, bxy + 4 + torch.rand(R, 2, generator=g) * 300], 1)
    gxy = bxy + torch.randn(R, 2, generator=g) * 20
    gt = torch.cat([gxy, gxy + 4 + torch.rand(R, 2, generator=g) * 300], 1)
    cnt = torch.tensor(counts, dtype=torch.int32)
    return [t.cuda() for t in (lo, de, lab, an, ma, lg, cls, bx, gt, cnt)]


@pytest.mark.parametrize("box_type", ["smooth_l1", "smooth_l1_mean"])
@pytest.mark.parametrize("gamma", [0.0, 1.5])
def test_det_loss_per_image_matches_float64_restatement(ops, box_type, gamma):
    N, A, K = 9, 10_000, 20                                                 # A > 2 chunks of 4096 anchors
    counts = [0, 5, 512, 37, 100, 1, 64, 3, 200]
    inp = _random_inputs(N, A, K, counts, zero_rpn_fg={3}, zero_roi_fg={6})
    lo, de, lab, an, ma, lg, cls, bx, gt, cnt = inp

    def run():
        return ops.det_loss_per_image(lo, de, lab, an, ma, (1.0, 1.0, 1.0, 1.0), 256, box_type, lg, K, cls, bx, gt, cnt,
                                      512, (10.0, 10.0, 5.0, 5.0), gamma, box_type)
    a = run(); b = run()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))             # bit for bit across launches
    got = a.cpu().double().numpy()
    want = _restated(inp, 256, box_type, K, gamma, box_type)
    nan_w = np.isnan(want)
    assert (np.isnan(got) == nan_w).all(), (np.argwhere(np.isnan(got) != nan_w), got, want)
    if box_type == "smooth_l1_mean":
        assert nan_w[3, 3] and nan_w[6, 1] and nan_w[0, 1]                  # no RPN fg / no ROI fg / no rows: torch's empty mean
        assert got[0, 0] == 0.0                                              # CE over no rows: 0 (layers/wrappers.py:26-33)
    else:
        assert not nan_w.any() and got[0, 0] == 0.0 and got[0, 1] == 0.0
    np.testing.assert_allclose(got[~nan_w], want[~nan_w], rtol=2e-5, atol=1e-6)
    s = a.cpu()
    tot = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]                          # f32, left to right (split_single.py:74)
    assert torch.equal(tot[~torch.isnan(tot)], s[:, 4][~torch.isnan(s[:, 4])])


def test_det_loss_per_image_refuses_overrunning_counts(ops):
    inp = _random_inputs(2, 500, 4, [3, 4], set(), set())
    lo, de, lab, an, ma, lg, cls, bx, gt, cnt = inp
    bad = torch.tensor([3, 40], dtype=torch.int32, device="cuda")          # 43 rows claimed, 7 exist: NaN, no read beyond
    out = ops.det_loss_per_image(lo, de, lab, an, ma, (1.0,) * 4, 256, "smooth_l1", lg, 4, cls, bx, gt, bad, 512,
                                 (10.0, 10.0, 5.0, 5.0), 0.0, "smooth_l1").cpu()
    assert torch.isfinite(out[0]).all() and torch.isnan(out[1, 0]) and torch.isnan(out[1, 4])
    out = ops.det_loss_per_image(lo, de, lab, an, ma, (1.0,) * 4, 256, "smooth_l1", lg, 4, cls, bx, gt, cnt, 3,   # 4 rows > max 3
                                 (10.0, 10.0, 5.0, 5.0), 0.0, "smooth_l1").cpu()
    assert torch.isfinite(out[0]).all() and torch.isnan(out[1, 0]) and torch.isfinite(out[1, 2])


# ------------------------------------------------------------------------------------------ the detector's loss options
def _detector(loss="CrossEntropy", box="smooth_l1", pf=0.25, seed=0):
    from sos_wsod_amd.config import CfgNode
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN
    torch.manual_seed(seed)
    cfg = CfgNode({"MODEL": {"META_ARCHITECTURE": "TwoStagePseudoLabGeneralizedRCNN",
                             "BACKBONE": {"NAME": "build_resnet_fpn_backbone", "FREEZE_AT": 2},
                             "PROPOSAL_GENERATOR": {"NAME": "PseudoLabRPN"},
                             "RPN": {"POSITIVE_FRACTION": pf, "LOSS": "CrossEntropy", "BBOX_REG_LOSS_TYPE": box},
                             "ROI_HEADS": {"NAME": "StandardROIHeadsPseudoLab", "LOSS": loss, "POSITIVE_FRACTION": pf, "NUM_CLASSES": 20},
                             "ROI_BOX_HEAD": {"BBOX_REG_LOSS_TYPE": box},
                             "PIXEL_MEAN": [103.53, 116.28, 123.675], "PIXEL_STD": [1.0, 1.0, 1.0]}})
    return TwoStagePseudoLabGeneralizedRCNN(cfg).cuda()


def _batch(sizes, seed, K=20, n_gt=3):
    from sos_wsod_amd.structures import Boxes, Instances
    g = torch.Generator().manual_seed(seed)
    out = []
    for (h, w) in sizes:
        img = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
        xy = torch.rand(n_gt, 2, generator=g) * torch.tensor([w * 0.6, h * 0.6])
        wh = 16 + torch.rand(n_gt, 2, generator=g) * torch.tensor([w * 0.35, h * 0.35])
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(torch.cat([xy, xy + wh], 1).cuda()); inst.gt_classes = torch.randint(0, K, (n_gt,), generator=g).cuda()
        out.append({"image": img.cuda(), "instances": inst, "height": h, "width": w})
    return out


def test_cross_entropy_config_builds_and_its_roi_loss_is_mean_softmax_ce():
    from sos_wsod_amd.events import EventStorage
    m = _detector("CrossEntropy")
    assert m.roi_heads.gamma == 0.0 and m.roi_heads.loss == "CrossEntropy"
    m.train()
    m.roi_heads.keep_loss_inputs = True
    with EventStorage(0):
        losses, _, _, _ = m(_batch([(160, 224), (160, 224)], 1), branch="supervised")
    lg, gtc, _, cnt = m.roi_heads.last_loss_inputs
    m.roi_heads.keep_loss_inputs = False
    K = 20
    x = lg.detach()[:, :K + 1].double()
    ce = F.cross_entropy(x, gtc.long())
    assert abs(float(losses["loss_cls"]) - float(ce)) <= 1e-5 * abs(float(ce)) + 1e-7
    # gradient: the focal kernel at gamma 0 against torch's CE gradient, d loss_cls / d logits
    from sos_wsod_amd.frcnn import _RoiLossFn
    R = lg.shape[0]
    logits = lg.detach().clone().requires_grad_(True)
    boxes2 = torch.randn(2 * R, 4, device="cuda").abs().cumsum(1).contiguous()
    l_cls, _ = _RoiLossFn.apply(logits, K, gtc, boxes2, (10.0, 10.0, 5.0, 5.0), 0.0)
    l_cls.backward()
    xr = lg.detach()[:, :K + 1].double().requires_grad_(True)
    F.cross_entropy(xr, gtc.long()).backward()
    np.testing.assert_allclose(logits.grad[:, :K + 1].double().cpu().numpy(), xr.grad.cpu().numpy(), rtol=1e-4, atol=1e-7)
    # and the whole forward + backward runs (SemiSupStep's burn-in path on the Stage-2 baseline)
    with EventStorage(0):
        losses, _, _, _ = m(_batch([(160, 224)], 2), branch="supervised")
        sum(losses.values()).backward()
    assert m.roi_heads.box_predictor.cls_score.weight.grad is not None


def test_smooth_l1_mean_evaluates_without_gradient_and_refuses_training():
    from sos_wsod_amd.events import EventStorage
    m = _detector("CrossEntropy", "smooth_l1_mean", pf=1.0)
    m.train()
    with EventStorage(0):
        with pytest.raises(NotImplementedError, match="BBOX_REG_LOSS_TYPE"):
            m(_batch([(160, 224)], 3), branch="supervised")
        rpn, roi = m.proposal_generator, m.roi_heads
        rpn.keep_loss_inputs = roi.keep_loss_inputs = True
        with torch.no_grad():
            batch = _batch([(160, 224)], 4)
            losses, _, _, _ = m(batch, branch="supervised")
        rpn.keep_loss_inputs = roi.keep_loss_inputs = False
    labels = rpn.last_loss_inputs[2]
    gtc = roi.last_loss_inputs[1]
    n_fg = int((labels == 1).sum())
    assert 0 < n_fg <= 256 and int((labels >= 0).sum()) == 256
    assert 0 < int(((gtc >= 0) & (gtc < 20)).sum()) <= 512
    assert all(bool(torch.isfinite(v)) for v in losses.values()), losses          # foreground on both sides: finite means


def test_image_losses_equal_the_batch_losses_for_one_image():
    """one image: the per-image kernel and the batch path (focal / CE kernel + rpn_loss + the smooth_l1_mean rescaling) agree"""
    from sos_wsod_amd.frcnn import Sampler
    from sos_wsod_amd.events import EventStorage
    for loss, box in (("CrossEntropy", "smooth_l1_mean"), ("FocalLoss", "smooth_l1"), ("CrossEntropy", "smooth_l1")):
        m = _detector(loss, box, pf=1.0 if box == "smooth_l1_mean" else 0.25, seed=7)
        m.train()
        batch = _batch([(192, 256)], 11, n_gt=4)
        res = []
        for _ in range(2):
            m.proposal_generator.sampler = m.roi_heads.sampler = Sampler(5)
            with EventStorage(0), torch.no_grad():
                res.append(m(batch, branch="supervised")[0] if not res else m.image_losses(batch))
        bl, per = res
        want = [float(bl[k]) for k in ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc")]
        got = per[0, :4].tolist()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7, err_msg=f"{loss} {box}")


def test_samplers_at_positive_fraction_one(ops):
    """RPN.POSITIVE_FRACTION / ROI_HEADS.POSITIVE_FRACTION = 1.0 (voc_split.yaml): up to 256 / 512 positives, negatives fill the rest"""
    from sos_wsod_amd.frcnn import Sampler
    m = _detector("CrossEntropy", "smooth_l1", pf=1.0)
    rpn = m.proposal_generator
    assert rpn.positive_fraction == 1.0 and m.roi_heads.positive_fraction == 1.0
    A = 6000
    xy = torch.rand(A, 2, device="cuda") * 400
    anchors = torch.cat([xy, xy + 40], 1).contiguous()
    many = anchors[:600:2].clone() + 1.0                        # 300 gt boxes on anchors: more than 256 positives
    few = anchors[:5].clone() + 0.5
    rpn.sampler = Sampler(1)
    labels, _ = rpn.label_and_sample_anchors(anchors, [many, few])
    pos, neg = (labels == 1).sum(1).tolist(), (labels == 0).sum(1).tolist()
    assert pos[0] == 256 and neg[0] == 0                         # capped at the batch, no room for negatives
    assert 5 <= pos[1] < 256 and pos[1] + neg[1] == 256           # negatives fill the rest
    # ROI sampler (sw_roi_label_sample) at B = 512, max_pos = 512: image 0 has 800 foreground candidates (more than the batch),
    # image 1 has 100 foreground and 700 background ones
    K, B = 20, 512
    g = torch.Generator().manual_seed(0)
    gt = torch.tensor([[100.0, 100.0, 300.0, 300.0]])
    fg = gt + torch.rand(800, 4, generator=g) * 8                 # IoU with the gt box > 0.5
    bg = torch.cat([torch.rand(700, 2, generator=g) * 50 + 400, torch.zeros(700, 2)], 1)
    bg[:, 2:] = bg[:, :2] + 30                                    # far from the gt box: IoU 0
    buf = torch.stack([fg, torch.cat([fg[:100], bg], 0)]).contiguous().cuda()
    cnt_dev = torch.tensor([800, 800], dtype=torch.int32).cuda()
    gt_b = torch.cat([gt, gt]).cuda(); gt_c = torch.tensor([3, 7], dtype=torch.int32).cuda()
    cnt, _, cls, _ = ops.roi_label_sample(cnt_dev, buf, gt_b, gt_c, [1, 1], [11, 12, 13, 14], False, 0.5, K, B, int(B * 1.0))
    cls = cls.cpu()
    assert cnt.tolist() == [512, 512]
    assert int((cls[0] < K).sum()) == 512 and int((cls[0] == K).sum()) == 0          # capped at the batch
    assert int((cls[1] < K).sum()) == 100 and int((cls[1] == K).sum()) == 412        # negatives fill the rest


# ------------------------------------------------------------------------------------------ split.score_images
def _dicts_and_loader(n, h, w, seed):
    g = np.random.default_rng(seed)
    imgs = [torch.from_numpy(g.integers(0, 256, (3, h, w), dtype=np.uint8)) for _ in range(n)]
    dicts = []
    for i in range(n):
        k = int(g.integers(1, 5))
        xy = g.random((k, 2)) * [w * 0.6, h * 0.6]
        wh = 20 + g.random((k, 2)) * [w * 0.3, h * 0.3]
        dicts.append({"height": h, "width": w, "i": i, "annotations": [
            {"bbox": [float(a) for a in np.concatenate([xy[j], xy[j] + wh[j]])], "bbox_mode": 0, "category_id": int(g.integers(0, 20))}
            for j in range(k)]})
    return dicts, (lambda d: imgs[d["i"]])


def test_bucketed_batch_scores_each_image_as_alone():
    from sos_wsod_amd import split
    m = _detector("CrossEntropy", "smooth_l1_mean", pf=1.0, seed=3)
    dicts, loader = _dicts_and_loader(6, 150, 200, 5)
    kw = dict(seed=9, min_sizes=(160,), max_size=400)
    alone = split.score_images(m, dicts, loader, images_per_batch=1, all_losses=True, **kw)
    four = split.score_images(m, dicts, loader, images_per_batch=4, all_losses=True, **kw)
    assert alone.dtype == np.float32 and alone.shape == (6, 5)
    fin = np.isfinite(alone)
    assert (np.isfinite(four) == fin).all() and fin[:, 4].sum() >= 3
    for c in range(5):                                            # each of the four losses and the sum
        np.testing.assert_allclose(four[fin[:, c], c], alone[fin[:, c], c], rtol=1e-4, err_msg=str(c))
    again = split.score_images(m, dicts, loader, images_per_batch=4, **kw)
    assert again.tobytes() == np.ascontiguousarray(four[:, 4]).tobytes()
    obj, percent = split.loss_split(again, 2)
    assert len(list(obj.values())[0]["1"]) == 2


# ------------------------------------------------------------------------------------------ against the reference's detector
class _Keys:
    """the closed-form sampling keys of the fixtures (oracle.frcnn_oracle.Perm) as the detector's sampler"""

    def __init__(self, tag):
        from oracle import frcnn_oracle as FO
        self.perm = FO.Perm(tag)

    def next_seed(self):
        from oracle import detgen
        k = self.perm.k
        self.perm.k += 1
        return detgen.fnv1a64(f"{self.perm.tag}perm{k}")


def _fixture_model(t, tag, loss, box, pf):
    from oracle import frcnn_oracle as FO
    K = int(t["K"])
    m = _detector(loss, box, pf)
    P = FO.make_params(K, tag=tag, head_scale=float(t["head_scale"]))
    sd = m.state_dict()
    assert set(sd) == set(P), (sorted(set(sd) - set(P))[:5], sorted(set(P) - set(sd))[:5])
    with torch.no_grad():
        for k, v in P.items():
            sd[k].copy_(torch.from_numpy(v))
    m.train()
    return m


def _fixture_image(h, w, n, K, tag):
    from oracle import frcnn_oracle as FO
    from sos_wsod_amd.structures import Boxes, Instances
    b, c = FO.make_gt(h, w, n, K, tag)
    inst = Instances((h, w))
    inst.gt_boxes = Boxes(torch.from_numpy(b).reshape(-1, 4).cuda()); inst.gt_classes = torch.from_numpy(c).long().cuda()
    return {"image": torch.from_numpy(FO.make_image(h, w, tag)).cuda(), "instances": inst, "height": h, "width": w}


def test_cross_entropy_head_matches_the_reference_generated_fixture():
    """voc_baseline.yaml's heads (ROI_HEADS.LOSS CrossEntropy: detectron2's FastRCNNOutputLayers) against split_ce.npz, written by
    running the reference's detector (tests/golden/make_split_det_golden.py): the four losses and the gradients"""
    from sos_wsod_amd.events import EventStorage
    t = np.load(os.path.join(GOLDEN, "split_ce.npz"))
    K = int(t["K"])
    m = _fixture_model(t, "spce", "CrossEntropy", "smooth_l1", 0.25)
    m.proposal_generator.sampler = m.roi_heads.sampler = _Keys("spce")
    data = [_fixture_image(int(h), int(w), int(n), K, f"spce{i}") for i, ((h, w), n) in enumerate(zip(t["sizes"], t["n_gt"]))]
    with EventStorage(0):
        losses, _, _, _ = m(data, branch="supervised")
        sum(losses.values()).backward()
    torch.cuda.synchronize()
    for k in LOSSES:
        ref = float(t["loss/" + k])
        # (the Stage-3 bars: 1e-4 for the RPN; the ROI losses 1e-3, as when near-tied proposals exchange a sampled ROI)
        tol = 1e-4 if k.startswith("loss_rpn") else 1e-3
        assert abs(float(losses[k]) - ref) <= tol * abs(ref), (k, float(losses[k]), ref)
    sd = dict(m.named_parameters())
    for key in t.files:
        if key.startswith("grad/"):
            ref, got = t[key], sd[key[5:]].grad.cpu().numpy()
        elif key.startswith("grads/"):
            ref, got = t[key], sd[key[6:]].grad.cpu().numpy().ravel()[::997]
        else:
            continue
        err = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
        assert err <= 5e-3, (key, err)


def test_split_scores_match_the_reference_generated_fixture():
    """voc_split.yaml's settings (CE, smooth_l1_mean for RPN and ROI, positive fraction 1.0), each image alone as split_single.py
    scores it, against split_score.npz written by the reference's detector; image 1 has no foreground: NaN box losses"""
    from sos_wsod_amd.events import EventStorage
    t = np.load(os.path.join(GOLDEN, "split_score.npz"))
    K = int(t["K"])
    m = _fixture_model(t, "spsc", "CrossEntropy", "smooth_l1_mean", 1.0)
    ref = t["losses"]
    for i, ((h, w), n) in enumerate(zip(t["sizes"], t["n_gt"])):
        m.proposal_generator.sampler = m.roi_heads.sampler = _Keys(f"spsc{i}")
        with EventStorage(0):
            got = m.image_losses([_fixture_image(int(h), int(w), int(n), K, f"spsc{i}")]).cpu().numpy()[0]
        assert (np.isnan(got) == np.isnan(ref[i])).all(), (i, got, ref[i])
        f = np.isfinite(ref[i])
        np.testing.assert_allclose(got[f], ref[i][f], rtol=1e-3, atol=1e-7, err_msg=str(i))
    assert np.isnan(ref[1, 1]) and np.isnan(ref[1, 3]) and np.isfinite(ref[1, 0])


# ------------------------------------------------------------------------------------------ one rank against two
def test_one_rank_and_two_ranks_write_the_same_split_file(tmp_path):
    """the same plan through `python -m sos_wsod_amd.split loss` on one process and on two ranks sharing cuda:0 over gloo
    (torch.distributed.run): byte-identical data-seed files"""
    from PIL import Image
    from sos_wsod_amd.config import get_cfg
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN
    cfg_text = """MODEL:
  META_ARCHITECTURE: "TwoStagePseudoLabGeneralizedRCNN"
  BACKBONE:
    NAME: "build_resnet_fpn_backbone"
  PROPOSAL_GENERATOR:
    NAME: "PseudoLabRPN"
  RPN:
    POSITIVE_FRACTION: 1.0
    LOSS: "CrossEntropy"
    BBOX_REG_LOSS_TYPE: "smooth_l1_mean"
  ROI_HEADS:
    NAME: "StandardROIHeadsPseudoLab"
    LOSS: "CrossEntropy"
    POSITIVE_FRACTION: 1.0
    NUM_CLASSES: 20
  ROI_BOX_HEAD:
    NAME: "FastRCNNConvFCHead"
    NUM_FC: 2
    POOLER_RESOLUTION: 7
    BBOX_REG_LOSS_TYPE: "smooth_l1_mean"
INPUT:
  MIN_SIZE_TRAIN: (160, 192)
  MAX_SIZE_TRAIN: 400
"""
    cfg = tmp_path / "split.yaml"
    cfg.write_text(cfg_text)
    torch.manual_seed(3)
    c = get_cfg(); c.merge_from_file(str(cfg))                   # (as the CLI loads it)
    m = TwoStagePseudoLabGeneralizedRCNN(c)
    ckpt = tmp_path / "model.pth"
    torch.save({"model": {"modelStudent." + k: v for k, v in m.state_dict().items()}}, str(ckpt))
    g = np.random.default_rng(2)
    dicts = []
    for i in range(9):
        h, w = (150, 200) if i % 3 else (200, 150)
        fn = tmp_path / f"{i:06d}.png"
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(fn))
        k = int(g.integers(1, 4))
        xy = g.random((k, 2)) * [w * 0.6, h * 0.6]
        wh = 20 + g.random((k, 2)) * [w * 0.3, h * 0.3]
        dicts.append({"file_name": str(fn), "height": h, "width": w, "annotations": [
            {"bbox": [float(a) for a in np.concatenate([xy[j], xy[j] + wh[j]])], "bbox_mode": 0, "category_id": int(g.integers(0, 20))}
            for j in range(k)]})
    dj = tmp_path / "dicts.json"
    dj.write_text(json.dumps(dicts))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    worker = os.path.join(ROOT, "tests", "split_ddp_worker.py")
    one, two = tmp_path / "one.txt", tmp_path / "two.txt"
    r = subprocess.run([sys.executable, worker, str(cfg), str(ckpt), str(dj), str(one), "2"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with __import__("socket").socket() as s_:
        s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), worker, str(cfg), str(ckpt), str(dj), str(two), "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "The finded percent is:" in r.stdout
    assert one.read_bytes() == two.read_bytes(), (one.read_text(), two.read_text())
    assert len(list(json.loads(one.read_text()).values())[0]["1"]) == 3

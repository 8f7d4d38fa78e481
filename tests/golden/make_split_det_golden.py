"""Generate tests/golden/split_ce.npz and split_score.npz by RUNNING the reference's Stage-3 detector (loaded through ref_shim_d2.py,
as make_stage3_golden.py does) under the split recipes' head settings — build container only:

    python tests/golden/make_split_det_golden.py

Cases
  ce     code_release/voc_baseline.yaml's heads: ROI_HEADS.LOSS "CrossEntropy" (detectron2's FastRCNNOutputLayers, roi_heads.py:
         405-406), everything else as voc_ssod.  "supervised" branch, the two 96x128 / 128x112 images of stage3_a (own tag), forward +
         backward -> the four losses, the ROI logits, gradient samples.
  score  code_release/voc_split.yaml's heads: CE, RPN and ROI BBOX_REG_LOSS_TYPE "smooth_l1_mean", RPN and ROI POSITIVE_FRACTION
         1.0.  Each image ALONE through the training forward without gradient, as unbias/split_single.py:66-75 scores it -> its four
         losses and their f32 sum (split_single.py:74).  Image 1 has no ground truth: no RPN and no ROI foreground, so both
         smooth_l1_mean losses are the mean of an empty tensor (NaN) and the CE loss is finite.

torch.randperm inside detectron2/modeling/sampling.py is the closed-form oracle.frcnn_oracle.Perm (one Perm per case, one per image
for `score`); everything else is the reference's code."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import ref_shim_d2  # noqa: E402
from oracle import frcnn_oracle as FO  # noqa: E402

ns = ref_shim_d2.install()
Boxes, Instances = ns.boxes.Boxes, ns.instances.Instances

K = 20
CE_SIZES, CE_N_GT = [(96, 128), (128, 112)], [3, 2]
SC_SIZES, SC_N_GT = [(96, 128), (128, 112), (112, 96)], [3, 0, 2]
GRAD_FULL = ["proposal_generator.rpn_head.objectness_logits.bias", "roi_heads.box_predictor.cls_score.bias",
             "roi_heads.box_predictor.bbox_pred.bias", "roi_heads.box_head.fc2.bias", "backbone.fpn_output2.bias"]
GRAD_SAMPLED = ["roi_heads.box_head.fc1.weight", "roi_heads.box_predictor.cls_score.weight", "proposal_generator.rpn_head.conv.weight",
                "backbone.fpn_lateral2.weight", "backbone.bottom_up.res4.0.shortcut.weight"]
STRIDE = 997
LOSSES = ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc")


def build(box_type, pf):
    """build_reference_model (voc_ssod heads) with the CE predictor, the box-loss type and the positive fractions of a split recipe"""
    model = ref_shim_d2.build_reference_model(ns, K)
    rpn, heads = model.proposal_generator, model.roi_heads
    rpn.positive_fraction, rpn.box_reg_loss_type = pf, box_type
    heads.positive_fraction = pf
    C = ref_shim_d2._Cfg
    cfg = C(MODEL=C(ROI_HEADS=C(NUM_CLASSES=K, SCORE_THRESH_TEST=0.05, NMS_THRESH_TEST=0.5),
                    ROI_BOX_HEAD=C(BBOX_REG_WEIGHTS=(10.0, 10.0, 5.0, 5.0), CLS_AGNOSTIC_BBOX_REG=False, SMOOTH_L1_BETA=0.0,
                                   BBOX_REG_LOSS_TYPE=box_type, BBOX_REG_LOSS_WEIGHT=1.0)),
            TEST=C(DETECTIONS_PER_IMAGE=100))
    heads.box_predictor = ns.fast_rcnn.FastRCNNOutputLayers(cfg, heads.box_head.output_shape)
    assert type(heads.box_predictor).__name__ == "FastRCNNOutputLayers"
    return model


def load_params(model, P):
    sd = model.state_dict()
    missing = [k for k in sd if k not in P and "anchor_generator.cell_anchors" not in k]
    assert not missing, missing[:5]
    for k, v in P.items():
        sd[k].copy_(torch.from_numpy(v))


def image(h, w, n, tag):
    d = {"image": torch.from_numpy(FO.make_image(h, w, tag)), "height": h, "width": w}
    b, c = FO.make_gt(h, w, n, K, tag)
    inst = Instances((h, w)); inst.gt_boxes = Boxes(torch.from_numpy(b).reshape(-1, 4)); inst.gt_classes = torch.from_numpy(c).long()
    d["instances"] = inst
    return d


class PatchRandperm:
    def __init__(self, perm):
        self.perm = perm

    def __enter__(self):
        self.orig = ns.sampling.torch.randperm
        ns.sampling.torch.randperm = lambda n, device=None: torch.from_numpy(self.perm(int(n)))
        return self

    def __exit__(self, *a):
        ns.sampling.torch.randperm = self.orig


def run_ce():
    P = FO.make_params(K, tag="spce", head_scale=5.0)
    model = build("smooth_l1", 0.25)
    load_params(model, P)
    model.train()
    data = [image(h, w, n, f"spce{i}") for i, ((h, w), n) in enumerate(zip(CE_SIZES, CE_N_GT))]
    captured = {}
    pred = model.roi_heads.box_predictor
    orig = pred.forward

    def spy(x):
        out = orig(x)
        captured["scores"], captured["deltas"] = out[0].detach().numpy().copy(), out[1].detach().numpy().copy()
        return out
    pred.forward = spy
    with ns.events.EventStorage(0), PatchRandperm(FO.Perm("spce")):
        losses, _, _, _ = model(data, branch="supervised")
        sum(losses.values()).backward()
    out = {"K": np.array(K), "sizes": np.array(CE_SIZES), "n_gt": np.array(CE_N_GT), "head_scale": np.array(5.0),
           "scores": captured["scores"], "deltas": captured["deltas"]}
    for k in LOSSES:
        out["loss/" + k] = np.array(float(losses[k].detach()))
    sd = dict(model.named_parameters())
    for k in GRAD_FULL:
        out["grad/" + k] = sd[k].grad.numpy().copy()
    for k in GRAD_SAMPLED:
        out["grads/" + k] = sd[k].grad.numpy().ravel()[::STRIDE].copy()
    np.savez_compressed(os.path.join(HERE, "split_ce.npz"), **out)
    print("[split ce]", {k: round(float(out["loss/" + k]), 6) for k in LOSSES})


def run_score():
    P = FO.make_params(K, tag="spsc", head_scale=5.0)
    model = build("smooth_l1_mean", 1.0)
    load_params(model, P)
    model.train()
    out = {"K": np.array(K), "sizes": np.array(SC_SIZES), "n_gt": np.array(SC_N_GT), "head_scale": np.array(5.0)}
    rows = []
    for i, ((h, w), n) in enumerate(zip(SC_SIZES, SC_N_GT)):
        d = image(h, w, n, f"spsc{i}")
        with ns.events.EventStorage(0), torch.no_grad(), PatchRandperm(FO.Perm(f"spsc{i}")):
            losses, _, _, _ = model([d], branch="supervised")
        v = [losses[k].to(torch.float32) for k in LOSSES]
        total = (v[0] + v[1] + v[2] + v[3]).cpu().item()                     # split_single.py:74
        rows.append([float(t) for t in v] + [total])
    out["losses"] = np.array(rows, dtype=np.float32)
    np.savez_compressed(os.path.join(HERE, "split_score.npz"), **out)
    print("[split score]", out["losses"])
    assert np.isnan(out["losses"][1, 1]) and np.isnan(out["losses"][1, 3]) and np.isfinite(out["losses"][1, 0])
    assert np.isfinite(out["losses"][[0, 2]]).all()


if __name__ == "__main__":
    run_ce()
    run_score()

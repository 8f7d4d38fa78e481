"""What the SoS-WSOD+ tests and their fixture generator (tests/golden/make_sosplus_golden.py) share: the two detector variants of
unbias/configs/code_release/sos_plus_wo_imagenet_test.yaml ("woi": torchvision-style ResNet + FPN with FrozenBN, 2-fc box head) and
sos_plus_test.yaml ("plus": the same + the 4conv1fc box head with FrozenBN), their config keys, their closed-form parameters
(oracle.frcnn_oracle.make_params + the added tensors, drawn from oracle.detgen the same way) and the sampler keys of the fixtures."""
import math

import numpy as np

from oracle import detgen
from oracle import frcnn_oracle as FO

K = 20
SIZES = [(96, 128), (128, 112)]
N_GT = [3, 2]
EVAL_OUT = [(131, 175), (100, 70)]
PIXEL_MEAN, PIXEL_STD = (123.675, 116.280, 103.530), (58.395, 57.120, 57.375)       # both configs (RGB statistics)
VARIANTS = ("woi", "plus")
GRAD_FULL = ["proposal_generator.rpn_head.objectness_logits.bias", "roi_heads.box_predictor.cls_score.bias", "roi_heads.box_head.fc1.bias"]
GRAD_SAMPLED = ["backbone.fpn_lateral3.weight", "backbone.bottom_up.res3.0.conv2.weight", "backbone.bottom_up.res4.0.conv1.weight", "backbone.bottom_up.res4.0.conv2.weight",
                "backbone.bottom_up.res5.0.conv2.weight", "backbone.bottom_up.res3.0.shortcut.weight", "backbone.fpn_output2.weight",
                "proposal_generator.rpn_head.conv.weight", "roi_heads.box_head.fc1.weight", "roi_heads.box_predictor.cls_score.weight"]
GRAD_SAMPLED_PLUS = ["roi_heads.box_head.conv1.weight", "roi_heads.box_head.conv4.weight"]
STRIDE = 997


def cfg_list(variant, device="cuda", dtype="fp32"):
    """the keys of the variant's config (its _BASE_ chain included) for CfgNode.merge_from_list on top of config.get_cfg()"""
    keys = ["MODEL.DEVICE", device, "MODEL.META_ARCHITECTURE", "GeneralizedRCNN", "MODEL.BACKBONE.NAME", "build_resnet_fpn_backbone",
            "MODEL.RESNETS.OUT_FEATURES", ["res2", "res3", "res4", "res5"], "MODEL.RESNETS.DEPTH", 50, "MODEL.RESNETS.STRIDE_IN_1X1", False,
            "MODEL.FPN.IN_FEATURES", ["res2", "res3", "res4", "res5"], "MODEL.FPN.NORM", "FrozenBN",
            "MODEL.PIXEL_MEAN", list(PIXEL_MEAN), "MODEL.PIXEL_STD", list(PIXEL_STD),
            "MODEL.RPN.POSITIVE_FRACTION", 0.25, "MODEL.RPN.LOSS", "CrossEntropy",
            "MODEL.ROI_HEADS.NAME", "StandardROIHeads", "MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"], "MODEL.ROI_HEADS.NUM_CLASSES", K,
            "MODEL.ROI_BOX_HEAD.NAME", "FastRCNNConvFCHead", "MODEL.ROI_BOX_HEAD.NUM_FC", 2, "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7,
            "MODEL.AMD.COMPUTE_DTYPE", dtype]
    if variant == "plus":
        keys += ["MODEL.RESNETS.NORM", "FrozenBN", "MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.NUM_FC", 1,
                 "MODEL.ROI_BOX_HEAD.NORM", "FrozenBN"]
    return keys


def make_params(variant, tag, head_scale, bg_bias=0.0):
    """FO.make_params with the variant's differences: the FPN convolutions lose their bias and gain FrozenBN statistics; "plus":
    box_head.conv1..4 (c2_msra_fill) with FrozenBN in front of ONE fc.  The stem's FrozenBN gain is multiplied by the pixel std of
    these configs (FO.make_params sizes it for std 1), so that the activations keep the scale the other gains were chosen for.
    bg_bias is added to the background logit's bias (the eval fixtures: with random weights every proposal would otherwise carry a
    foreground class above the score threshold, and among a thousand candidates some pair always sits at the NMS threshold)."""
    assert variant in VARIANTS
    p = FO.make_params(K, tag=tag, head_scale=head_scale)
    p["backbone.bottom_up.stem.conv1.norm.weight"] = p["backbone.bottom_up.stem.conv1.norm.weight"] * np.float32(PIXEL_STD[0])

    if bg_bias:
        p["roi_heads.box_predictor.cls_score.bias"] = p["roi_heads.box_predictor.cls_score.bias"].copy()
        p["roi_heads.box_predictor.cls_score.bias"][K] += np.float32(bg_bias)

    def bn(name, c):
        p[name + ".norm.weight"] = detgen.uniform(tag + name + ".norm.weight", (c,), 0.5, 1.5)
        p[name + ".norm.bias"] = detgen.normal(tag + name + ".norm.bias", (c,), std=0.1)
        p[name + ".norm.running_mean"] = detgen.normal(tag + name + ".norm.running_mean", (c,), std=0.1)
        p[name + ".norm.running_var"] = detgen.uniform(tag + name + ".norm.running_var", (c,), 0.5, 1.5)
    for s in FO.FPN_STAGES:
        for nm in (f"backbone.fpn_lateral{s}", f"backbone.fpn_output{s}"):
            del p[nm + ".bias"]
            bn(nm, 256)
    if variant == "plus":
        for i in (1, 2):
            del p[f"roi_heads.box_head.fc{i}.weight"], p[f"roi_heads.box_head.fc{i}.bias"]
        for i in range(1, 5):
            name = f"roi_heads.box_head.conv{i}"
            p[name + ".weight"] = detgen.normal(tag + name + ".weight", (256, 256, 3, 3), std=math.sqrt(2.0 / (256 * 9)))
            bn(name, 256)
        name, d_in = "roi_heads.box_head.fc1", 256 * 7 * 7
        lim = math.sqrt(3.0 / d_in)
        p[name + ".weight"] = detgen.uniform(tag + name + ".weight", (1024, d_in), -lim, lim)
        p[name + ".bias"] = detgen.normal(tag + name + ".bias", (1024,), std=0.01)
    return p


class Keys:
    """the closed-form sampling keys of the fixtures (oracle.frcnn_oracle.Perm) as the product's sampler"""

    def __init__(self, tag):
        self.tag, self.k = tag, 0

    def next_seed(self):
        k = self.k
        self.k += 1
        return detgen.fnv1a64(f"{self.tag}perm{k}")


def images(tag):
    return [FO.make_image(h, w, f"{tag}{i}") for i, (h, w) in enumerate(SIZES)]


def ground_truth(tag):
    return [FO.make_gt(h, w, n, K, f"{tag}{i}") for i, ((h, w), n) in enumerate(zip(SIZES, N_GT))]

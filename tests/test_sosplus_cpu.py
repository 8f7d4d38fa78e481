"""CPU: the two SoS-WSOD+ detector configs (unbias/configs/code_release/sos_plus_wo_imagenet_test.yaml, sos_plus_test.yaml) build
from their keys on MODEL.DEVICE cpu (no kernel runs) with exactly the state-dict names, shapes and frozen parameters of the
reference's own GeneralizedRCNN (recorded in tests/golden/sosplus_*_a.npz by make_sosplus_golden.py); the architecture keys are
read or refused; default arguments still give the model that existed before."""
import os

import numpy as np
import pytest
import torch

import sosplus_ref as SP
from oracle import frcnn_oracle as FO


def _build(variant):
    from sos_wsod_amd.config import add_wsl_config, get_cfg
    from sos_wsod_amd.rcnn_multi import build_model
    cfg = add_wsl_config(get_cfg())
    assert cfg.MODEL.META_ARCHITECTURE == "GeneralizedRCNN"                        # the name get_cfg() defaults to is registered
    assert cfg.MODEL.RESNETS.STRIDE_IN_1X1 is True and cfg.MODEL.FPN.NORM == "" and cfg.MODEL.RESNETS.DEPTH == 50
    cfg.merge_from_list(SP.cfg_list(variant, device="cpu"))
    return build_model(cfg)


@pytest.mark.parametrize("variant", SP.VARIANTS)
def test_config_builds_with_the_reference_state_dict(golden_dir, variant):
    from sos_wsod_amd import frcnn
    t = np.load(os.path.join(golden_dir, f"sosplus_{variant}_a.npz"))
    m = _build(variant)
    assert type(m) is frcnn.GeneralizedRCNN and isinstance(m, frcnn.TwoStagePseudoLabGeneralizedRCNN)
    sd = m.state_dict()
    want = {str(k): tuple(int(v) for v in str(s).split(",") if v) for k, s in zip(t["names"], t["shapes"])}
    assert set(sd) == set(want), (sorted(set(sd) - set(want))[:5], sorted(set(want) - set(sd))[:5])
    assert all(tuple(sd[k].shape) == want[k] for k in want)
    assert {n for n, p in m.named_parameters() if not p.requires_grad} == {str(k) for k in t["frozen"]}
    P = SP.make_params(variant, "names", 1.0)
    assert set(P) == set(want) and all(tuple(v.shape) == want[k] for k, v in P.items())
    assert "backbone.fpn_lateral2.bias" not in sd and "backbone.fpn_lateral2.norm.running_var" in sd
    blk = m.backbone.bottom_up.res3[0]
    assert (blk.conv1.stride, blk.conv2.stride, blk.shortcut.stride, blk.conv2.col) == (1, 2, 2, True)
    assert not m.backbone.bottom_up.res3[1].conv2.col and m.backbone.bottom_up.res2[0].conv2.stride == 1
    assert m.roi_heads.gamma == 0.0 and m.roi_heads.loss == "CrossEntropy"         # detectron2's heads: cross entropy
    head = m.roi_heads.box_head
    assert (len(head.convs), len(head.fcs)) == ((4, 1) if variant == "plus" else (0, 2))
    assert [float(v) for v in m.pixel_std.flatten()] == pytest.approx(list(SP.PIXEL_STD))


def test_architecture_keys_are_read_or_refused():
    from sos_wsod_amd.config import CfgNode
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN as D
    assert D._arch_kwargs(CfgNode({})) == (True, "", dict(conv_dims=(), fc_dims=(1024, 1024), conv_norm=""))
    M = CfgNode({"RESNETS": {"STRIDE_IN_1X1": False}, "FPN": {"NORM": "FrozenBN"},
                 "ROI_BOX_HEAD": {"NUM_CONV": 4, "CONV_DIM": 128, "NUM_FC": 1, "NORM": "FrozenBN"}})
    assert D._arch_kwargs(M) == (False, "FrozenBN", dict(conv_dims=(128,) * 4, fc_dims=(1024,), conv_norm="FrozenBN"))
    for bad in ({"FPN": {"NORM": "GN"}}, {"ROI_BOX_HEAD": {"NORM": "SyncBN"}}, {"RESNETS": {"DEPTH": 101}}, {"RESNETS": {"NORM": "BN"}},
                {"FPN": {"FUSE_TYPE": "avg"}}, {"RESNETS": {"RES5_DILATION": 2}}, {"ROI_BOX_HEAD": {"NUM_CONV": 0, "NUM_FC": 0}},
                {"ROI_BOX_HEAD": {"NUM_CONV": 1, "CONV_DIM": 100}}):
        with pytest.raises(AssertionError, match="not implemented"):
            D._arch_kwargs(CfgNode(bad))
    with pytest.raises(AssertionError, match="not implemented"):
        D._cfg_kwargs(CfgNode({"ROI_BOX_HEAD": {"FC_DIM": 2048}}), {})               # still fixed


def test_default_arguments_build_the_model_that_existed_before():
    from sos_wsod_amd import frcnn
    torch.manual_seed(3)
    a = frcnn.TwoStagePseudoLabGeneralizedRCNN(num_classes=20)
    torch.manual_seed(3)
    b = frcnn.GeneralizedRCNN(num_classes=20)
    P = FO.make_params(20, tag="names")
    for m in (a, b):
        sd = m.state_dict()
        assert set(sd) == set(P) and all(tuple(sd[k].shape) == tuple(v.shape) for k, v in P.items())
        assert not any(getattr(mod, "col", False) for mod in m.modules()) and m.backbone.bottom_up.stride_in_1x1
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())   # same construction, same initial values
    assert a.roi_heads.gamma == 1.5 and b.roi_heads.gamma == 0.0                       # focal loss / detectron2's cross entropy

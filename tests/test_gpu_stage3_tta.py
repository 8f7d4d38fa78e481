"""GPU: Stage-3 test-time augmentation end to end (tta.GeneralizedRCNNWithTTA over a random-weight TwoStagePseudoLabGeneralizedRCNN):
the wrapper's padded, read-back-free path and its one merge launch against the composition made here from the detector's default
inference form (per-view detections cut at counts read on the host) and the NumPy restatement of the merge — exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tta_merge_ref import tta_merge_ref  # noqa: E402

pytestmark = pytest.mark.gpu

K, MIN_SIZES = 3, (64, 96)


@pytest.fixture(scope="module")
def setup():
    from sos_wsod_amd.config import get_cfg
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN
    torch.manual_seed(0)
    model = TwoStagePseudoLabGeneralizedRCNN(num_classes=K, compute_dtype=torch.float32).cuda().eval()
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.ROI_HEADS.NUM_CLASSES", K, "TEST.AUG.MIN_SIZES", MIN_SIZES, "TEST.AUG.ENABLED", True])
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (3, 96, 128), generator=g, dtype=torch.uint8).cuda()
    return model, cfg, {"image": img, "height": 75, "width": 100}              # the loader resized 75 x 100 to 96 x 128: pre_tfm is exercised


def _composition(model, wrapper, inp, batch_size):
    """the same view batches through the default inference form, counts on the host, then the restated merge"""
    from sos_wsod_amd.tta import view_table
    views = wrapper.tta_mapper(dict(inp))
    T = model.roi_heads.box_predictor.test_topk_per_image
    V = len(views)
    b, s, c, n = np.zeros((V, T, 4), np.float32), np.zeros((V, T), np.float32), np.zeros((V, T), np.int32), np.zeros(V, np.int32)
    for i in range(0, V, batch_size):
        for j, r in enumerate(model.inference([v for v, _ in views[i:i + batch_size]], do_postprocess=False)):
            k = len(r)
            n[i + j] = k
            b[i + j, :k] = r.pred_boxes.tensor.cpu().numpy(); s[i + j, :k] = r.scores.cpu().numpy(); c[i + j, :k] = r.pred_classes.cpu().numpy()
    tab = view_table([t for _, t in views], inp["image"].shape[-2:], (inp["height"], inp["width"]), "cpu").numpy()
    return views, n, tta_merge_ref(b, s, c, n, tab, inp["height"], inp["width"], wrapper.nms_thresh, wrapper.topk, K)


def _check(res, want):
    inst = res["instances"]
    n = int(want["count"][0])
    assert tuple(inst.image_size) == (75, 100) and len(inst) == n and inst.pred_classes.dtype == torch.int64
    assert np.array_equal(inst._sw_src.cpu().numpy(), want["src"][:n])
    assert np.array_equal(inst.pred_classes.cpu().numpy(), want["classes"][:n])
    assert np.array_equal(inst.scores.cpu().numpy().view(np.uint32), want["scores"][:n].view(np.uint32))
    assert np.array_equal(inst.pred_boxes.tensor.cpu().numpy().view(np.uint32), want["boxes"][:n].view(np.uint32))


def test_wrapper_equals_the_composition_and_leaves_the_detector_as_it_was(setup):
    from sos_wsod_amd.tta import GeneralizedRCNNWithTTA
    model, cfg, inp = setup
    before = model.inference([inp])[0]["instances"]
    w = GeneralizedRCNNWithTTA(cfg, model)
    assert w.batch_size == 3
    res = w([inp])
    assert len(res) == 1 and model.roi_heads.padded_detections is False           # restored
    views, counts, want = _composition(model, w, inp, 3)
    assert [tuple(v["image"].shape[-2:]) for v, _ in views] == [(64, 85), (64, 85), (96, 128), (96, 128)]      # 4 views: batches of 3 and 1
    assert [t.flip for _, t in views] == [False, True, False, True] and all("proposals" not in v for v, _ in views)
    assert counts.sum() > 0 and int(want["count"][0]) > 0
    _check(res[0], want)
    after = model.inference([inp])[0]["instances"]                                 # default behaviour unchanged, bit for bit
    assert torch.equal(before.pred_boxes.tensor, after.pred_boxes.tensor) and torch.equal(before.scores, after.scores)
    assert torch.equal(before.pred_classes, after.pred_classes) and before.pred_classes.dtype == torch.int64


def test_batch_size_one_gives_a_result_of_the_same_form(setup):
    from sos_wsod_amd.tta import GeneralizedRCNNWithTTA
    model, cfg, inp = setup
    w = GeneralizedRCNNWithTTA(cfg, model, batch_size=1)
    res = w([inp])
    _, _, want = _composition(model, w, inp, 1)
    _check(res[0], want)
    b = res[0]["instances"].pred_boxes.tensor
    assert float(b[:, 0::2].max()) <= 100 and float(b[:, 1::2].max()) <= 75 and float(b.min()) >= 0


def test_padded_switch_restored_when_a_view_fails(setup):
    from sos_wsod_amd.tta import GeneralizedRCNNWithTTA
    model, cfg, inp = setup

    def broken(d):
        raise RuntimeError("mapper")
    w = GeneralizedRCNNWithTTA(cfg, model, tta_mapper=broken)
    with pytest.raises(RuntimeError):
        w([inp])
    assert model.roi_heads.padded_detections is False


def test_with_tta_suffixes_the_result_keys(setup):
    from sos_wsod_amd.tta import test_with_TTA as run_tta
    model, cfg, inp = setup

    class Ev:
        def reset(self):
            self.n = 0

        def process(self, inputs, outputs):
            self.n += len(outputs)

        def evaluate(self):
            return {"bbox": {"AP": float(self.n)}}
    assert run_tta(cfg, model, [[inp]], Ev()) == {"bbox_TTA": {"AP": 1.0}}
    assert not model.training and model.roi_heads.padded_detections is False

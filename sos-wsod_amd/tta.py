"""Test-time augmentation.  Stage 3 (GeneralizedRCNNWithTTA, at the end of this file): the union of the views' detections and a
second NMS, detectron2/detectron2/modeling/test_time_augmentation.py.  Stage 1 (GeneralizedRCNNWithTTAAVG): score / box averaging (SURVEY §8f row 2;
uwsod/projects/WSL/wsl/modeling/test_time_augmentation_avg.py:199-427, boxes only — the path has no mask head).

For every augmented view (resize to a TEST.AUG min size, optional horizontal flip) the detector runs WITHOUT its
post-processing and returns the per-proposal score matrix (R, K+1) and class-wise boxes (R, 4K) in the view's
coordinates; the boxes are mapped back through the inverse transforms (un-flip in the resized frame, then un-resize), both
are averaged over the views (the proposals are index aligned across views), and the averaged set goes through the usual
threshold / per-class NMS / top-k (`sw_detect_postprocess`).

The reference builds the views on the CPU (`DatasetMapperTTAAVG`: PIL resize, numpy flip, `transform_proposals`).
`DeviceTTAMapper` builds them on the device: the resize is the HIP restatement of Pillow's 8-bit bilinear resampling
(`resize.resize_bilinear_u8`, bit-identical pixels, the flipped view from the same launch) and the proposal boxes go through
the same affine maps (fvcore's ResizeTransform / HFlipTransform `apply_box`, third-party, restated in `ViewTransform`).
"""
from typing import List, Tuple

import torch

from .resize import resize_bilinear_u8
from .structures import Boxes, Instances


class ViewTransform:
    """[crop: shift by -(x0, y0) into a window of size orig_hw (fvcore CropTransform.apply_coords),] resize (orig h,w -> new h,w),
    then an optional horizontal flip in the resized frame; every step in the boxes' own dtype, as numpy does it"""

    def __init__(self, orig_hw: Tuple[int, int], new_hw: Tuple[int, int], flip: bool, crop_xy=None):
        self.orig_hw, self.new_hw, self.flip = tuple(orig_hw), tuple(new_hw), bool(flip)
        self.crop_xy = None if crop_xy is None else (int(crop_xy[0]), int(crop_xy[1]))

    def apply_box(self, boxes: torch.Tensor) -> torch.Tensor:
        sx, sy = self.new_hw[1] / self.orig_hw[1], self.new_hw[0] / self.orig_hw[0]
        if self.crop_xy is not None:
            x0, y0 = self.crop_xy
            boxes = _offset_xyxy(boxes, -float(x0), -float(y0))
        b = _scale_xyxy(boxes, sx, sy)
        if self.flip:                                        # HFlipTransform.apply_box: x -> W - x, corners re-sorted
            w = float(self.new_hw[1])
            b = torch.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], 1)
        return b

    def inverse_box(self, boxes: torch.Tensor) -> torch.Tensor:
        assert self.crop_xy is None, "the test-time views are not cropped"
        b = boxes
        if self.flip:
            w = float(self.new_hw[1])
            b = torch.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], 1)
        sx, sy = self.orig_hw[1] / self.new_hw[1], self.orig_hw[0] / self.new_hw[0]
        return _scale_xyxy(b, sx, sy)


def _scale_xyxy(b: torch.Tensor, sx: float, sy: float) -> torch.Tensor:
    """b * [sx, sy, sx, sy] without building that 4-vector on the device: `b.new_tensor([...])` is a pageable host-to-device copy that
    waits for the stream — 24 of them were 13.8 of the 20 ms of a 12-view TTA call (tools/diag/infer_host_profile.py).  The scalar
    form multiplies by the same float32 values: identical bits."""
    out = b.clone()
    out[:, 0::2].mul_(sx)
    out[:, 1::2].mul_(sy)
    return out


def _offset_xyxy(b: torch.Tensor, dx: float, dy: float) -> torch.Tensor:
    out = b.clone()
    out[:, 0::2].add_(dx)
    out[:, 1::2].add_(dy)
    return out


class DeviceTTAMapper:
    """dataset dict -> list of (augmented dict, ViewTransform) for TEST.AUG.{MIN_SIZES, MAX_SIZE, FLIP}.  The views are made from the
    tensor in the dict (the loader's already resized image); "height" / "width" stay the dataset's.  Without "proposals" in the dict
    (Stage 3) the views carry none."""

    def __init__(self, min_sizes=(480, 576, 688, 864, 1000, 1200), max_size=4000, flip=True, proposal_topk=None, min_box_size=0):
        self.min_sizes, self.max_size, self.flip = tuple(min_sizes), max_size, flip
        self.proposal_topk, self.min_box_size = proposal_topk, min_box_size

    @staticmethod
    def _shortest_edge(h, w, size, max_size):                # ResizeShortestEdge.get_output_shape
        scale = size * 1.0 / min(h, w)
        nh, nw = (size, scale * w) if h < w else (scale * h, size)
        if max(nh, nw) > max_size:
            s = max_size * 1.0 / max(nh, nw)
            nh, nw = nh * s, nw * s
        return int(nh + 0.5), int(nw + 0.5)

    def __call__(self, d):
        img = d["image"]                                     # (3, h, w) uint8
        h, w = img.shape[-2:]
        prop = d.get("proposals")
        out = []
        for size in self.min_sizes:
            nh, nw = self._shortest_edge(h, w, size, self.max_size)
            r, r_flip = resize_bilinear_u8(img, (nh, nw), with_flip=True)
            for flip in ((False, True) if self.flip else (False,)):
                t = ViewTransform((h, w), (nh, nw), flip)
                if prop is None:                             # DatasetMapperTTA (test_time_augmentation.py:28-98): the detector proposes itself
                    out.append(({"image": r_flip if flip else r, "height": d.get("height", h), "width": d.get("width", w)}, t))
                    continue
                # transform_proposals (test_time_augmentation_avg.py:29-71): map, clip to the view, drop empty boxes, top-k.
                # (The reference filters per view and later stacks the views' (R, 4K) outputs: views that drop different
                # proposals fail there; here too the merge requires equal counts.)
                b = t.apply_box(prop.proposal_boxes.tensor.float())
                b = torch.stack([b[:, 0].clamp(0, nw), b[:, 1].clamp(0, nh), b[:, 2].clamp(0, nw), b[:, 3].clamp(0, nh)], 1)
                keep = ((b[:, 2] - b[:, 0]) > self.min_box_size) & ((b[:, 3] - b[:, 1]) > self.min_box_size)
                logits = prop.objectness_logits
                if not bool(keep.all()):
                    b, logits = b[keep], logits[keep]
                p = Instances((nh, nw))
                p.proposal_boxes = Boxes(b[:self.proposal_topk])
                p.objectness_logits = logits[:self.proposal_topk]
                view = {"image": r_flip if flip else r, "proposals": p, "height": d.get("height", h),
                        "width": d.get("width", w)}
                out.append((view, t))
        return out


class GeneralizedRCNNWithTTAAVG(torch.nn.Module):
    """same call interface as the model's inference forward; `tta_mapper(dict) -> [(view dict, ViewTransform)]`"""

    def __init__(self, model, tta_mapper=None, batch_views=True):
        super().__init__()
        if isinstance(model, torch.nn.parallel.DistributedDataParallel):
            model = model.module
        self.model = model
        self.tta_mapper = tta_mapper if tta_mapper is not None else DeviceTTAMapper()
        self.batch_views = bool(batch_views)

    @torch.no_grad()
    def __call__(self, batched_inputs: List[dict]):
        return [self._inference_one_image(x) for x in batched_inputs]

    def _inference_one_image(self, inp):
        from . import ops
        assert not self.model.training
        h, w = inp["image"].shape[-2:]
        orig = (inp.get("height", h), inp.get("width", w))
        views = self.tta_mapper(dict(inp, height=orig[0], width=orig[1]))
        heads = self.model.roi_heads
        K = heads.num_classes
        sum_scores = sum_boxes = None
        heads.test_scores_only = True             # per-view NMS / top-k (and their host sync) would be thrown away
        try:
            # consecutive views of one size (a scale and its flip) run as one batch: the batch-1 launches of a 375 x 500 image's
            # views fill half the chip (12 views: 26.6 -> see tools/infer_bench.py); the per-view results enter the sums in the
            # mapper's order either way
            per_view = []
            i = 0
            while i < len(views):
                j = i + 1
                while (self.batch_views and j < len(views) and j - i < 2
                       and views[j][0]["image"].shape == views[i][0]["image"].shape):
                    j += 1
                if j - i > 1 and hasattr(self.model, "view_scores"):
                    per_view += self.model.view_scores([v for v, _ in views[i:j]])
                else:
                    for v, _ in views[i:j]:
                        _, sc, bx = self.model.inference([v], do_postprocess=False)       # (1, R, K+1), (1, R, 4K), view coordinates
                        per_view.append((sc[0], bx[0]))
                i = j
            for (view, tfm), (scores, boxes) in zip(views, per_view):
                R = boxes.shape[0]
                back = tfm.inverse_box(boxes.reshape(R * K, 4)).reshape(R, 4 * K)
                if (tfm.orig_hw != orig):                        # the mapper resized from the tensor's size, not the dataset's
                    sx, sy = orig[1] / tfm.orig_hw[1], orig[0] / tfm.orig_hw[0]
                    back = _scale_xyxy(back.reshape(R * K, 4), sx, sy).reshape(R, 4 * K)
                sum_scores = scores.clone() if sum_scores is None else sum_scores + scores
                sum_boxes = back if sum_boxes is None else sum_boxes + back
        finally:
            heads.test_scores_only = False
        n = float(len(views))
        all_scores, all_boxes = (sum_scores / n).contiguous(), (sum_boxes / n).contiguous()
        self.last_avg = (all_scores, all_boxes)                    # tests: the view-averaged matrices that enter the merge
        cnt, dboxes, dscores, dclasses, _ = ops.detect_postprocess(all_scores, all_boxes, int(orig[0]), int(orig[1]),
                                                                   heads.test_score_thresh, heads.test_nms_thresh,
                                                                   heads.test_topk_per_image)
        n_det = int(cnt.item())
        res = Instances((int(orig[0]), int(orig[1])))
        res.pred_boxes = Boxes(dboxes[:n_det])
        res.scores = dscores[:n_det]
        res.pred_classes = dclasses[:n_det].to(torch.int64)
        return {"instances": res}


# ------------------------------------------------------------------------------------------------ Stage 3: union of the views' detections
def view_table(tfms, loader_hw, orig_hw, device):
    """ops.tta_merge's per-view table (V, 6) f32: flip, view width, the ratios view -> loader image (ViewTransform.inverse_box) and loader
    image -> dataset image (the inverse of DatasetMapperTTA's `pre_tfm`; 1 when the shapes are equal) as the float32 values the tensor
    forms multiply by"""
    rows = []
    for t in tfms:
        assert t.crop_xy is None and tuple(t.orig_hw) == tuple(loader_hw)
        rows.append([float(t.flip), float(t.new_hw[1]), t.orig_hw[1] / t.new_hw[1], t.orig_hw[0] / t.new_hw[0],
                     orig_hw[1] / loader_hw[1] if tuple(orig_hw) != tuple(loader_hw) else 1.0,
                     orig_hw[0] / loader_hw[0] if tuple(orig_hw) != tuple(loader_hw) else 1.0])
    return torch.tensor(rows, dtype=torch.float32).reshape(len(rows), 6).to(device)


def _cfg_get(node, key, default):
    return node.get(key, default) if hasattr(node, "get") else getattr(node, key, default)


class GeneralizedRCNNWithTTA(torch.nn.Module):
    """detectron2/detectron2/modeling/test_time_augmentation.py:101-259, boxes only (unbias/train_net_test_tta.py with
    unbias/configs/code_release/voc07_tta_test.yaml): every view (TEST.AUG.MIN_SIZES x flip, in the mapper's order, batches of
    `batch_size` — a batch pads its views to a common size, so the batching is part of the result) goes through
    `model.inference(do_postprocess=False)`; the union of the views' post-NMS detections, mapped back to the dataset image, goes through
    a second per-class NMS at score > 1e-8 and the top TEST.DETECTIONS_PER_IMAGE are kept.

    The ROI heads run with `padded_detections` set to a frcnn.PaddedDetections block: every view leaves its topk padded rows and its
    DEVICE count in the block, ONE ops.tta_merge launch merges it, and the wrapper itself reads the device once per image (the final
    count; the RPN's one read of its proposal counts per view batch is the detector's own).
    `tta_mapper(dict) -> [(view dict, ViewTransform)]`."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=3):
        super().__init__()
        if isinstance(model, torch.nn.parallel.DistributedDataParallel):
            model = model.module
        M, T = cfg.MODEL, cfg.TEST
        if _cfg_get(M, "KEYPOINT_ON", False):
            raise ValueError("GeneralizedRCNNWithTTA: MODEL.KEYPOINT_ON is not supported (the reference refuses it too)")
        if _cfg_get(M, "MASK_ON", False):
            raise ValueError("GeneralizedRCNNWithTTA: MODEL.MASK_ON is not supported (this path has no mask head)")
        if _cfg_get(M, "LOAD_PROPOSALS", False):
            raise ValueError("GeneralizedRCNNWithTTA: MODEL.LOAD_PROPOSALS is not supported (the reference refuses it too; the Stage-1 "
                             "variant for precomputed proposals is GeneralizedRCNNWithTTAAVG)")
        if not (hasattr(model, "inference") and hasattr(getattr(model, "roi_heads", None), "padded_detections")):
            raise TypeError(f"GeneralizedRCNNWithTTA needs a detector whose ROI heads have the `padded_detections` form, got {type(model).__name__}")
        A = _cfg_get(T, "AUG", {})
        self.model = model
        self.num_classes = int(M.ROI_HEADS.NUM_CLASSES)
        self.nms_thresh = float(_cfg_get(M.ROI_HEADS, "NMS_THRESH_TEST", 0.5))
        self.topk = int(_cfg_get(T, "DETECTIONS_PER_IMAGE", 100))
        if tta_mapper is None:
            tta_mapper = DeviceTTAMapper(tuple(_cfg_get(A, "MIN_SIZES", (400, 500, 600, 700, 800, 900, 1000, 1100, 1200))),
                                         int(_cfg_get(A, "MAX_SIZE", 4000)), bool(_cfg_get(A, "FLIP", True)))
        self.tta_mapper = tta_mapper
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("GeneralizedRCNNWithTTA: batch_size >= 1")
        self._tabs = {}                                         # (views' geometry, dataset (h, w)) -> device view table
        self.train(model.training)                              # a fresh Module is in training mode: evaluation.inference_on_dataset restores
        #                                                         the mode it found, which must be the detector's, not the wrapper's default

    @torch.no_grad()
    def __call__(self, batched_inputs: List[dict]):
        return [self._inference_one_image(x) for x in batched_inputs]

    def _view_table(self, tfms, loader_hw, orig, device):
        key = (tuple((t.new_hw, t.flip) for t in tfms), tuple(loader_hw), tuple(orig), str(device))
        tab = self._tabs.get(key)
        if tab is None:
            if len(self._tabs) >= 256:
                self._tabs.clear()
            tab = self._tabs[key] = view_table(tfms, loader_hw, orig, device)        # (a host-to-device copy: once per geometry)
        return tab

    def merge_inputs(self, inp):
        """-> (frcnn.PaddedDetections block of the views' detections, view table, dataset (h, w)): what the one merge launch reads"""
        from .frcnn import PaddedDetections
        assert not self.model.training
        img = inp["image"].to(self.model.device)
        h, w = (int(v) for v in img.shape[-2:])
        orig = (int(inp.get("height", h)), int(inp.get("width", w)))
        views = self.tta_mapper({"image": img, "height": orig[0], "width": orig[1]})
        heads = self.model.roi_heads
        T = heads.box_predictor.test_topk_per_image
        block = PaddedDetections(len(views), T, img.device)
        old = heads.padded_detections
        heads.padded_detections = block
        try:
            for i in range(0, len(views), self.batch_size):
                self.model.inference([v for v, _ in views[i:i + self.batch_size]], do_postprocess=False)
        finally:
            heads.padded_detections = old
        assert block.filled == len(views)
        return block, self._view_table([t for _, t in views], (h, w), orig, img.device), orig

    def _inference_one_image(self, inp):
        from . import ops
        block, tab, orig = self.merge_inputs(inp)
        cnt, boxes, scores, classes, src = ops.tta_merge(block.boxes, block.scores, block.classes, block.counts, tab, orig[0], orig[1],
                                                          self.nms_thresh, self.topk, self.num_classes)
        n = ops.tta_merge_count(cnt)                            # the one device -> host read of this image
        res = Instances(orig)
        res.pred_boxes = Boxes(boxes[:n])
        res.scores = scores[:n]
        res.pred_classes = classes[:n].to(torch.int64)
        res._sw_src = src[:n]
        return {"instances": res}


def test_with_TTA(cfg, model, data_loader, evaluator):
    """unbias/train_net_test_tta.py:101-115 (Trainer.test_with_TTA) for one loader / evaluator pair: evaluation.inference_on_dataset over
    the TTA wrapper, the result keys suffixed with "_TTA" """
    from .evaluation import inference_on_dataset
    res = inference_on_dataset(GeneralizedRCNNWithTTA(cfg, model), data_loader, evaluator)
    return {k + "_TTA": v for k, v in res.items()}


test_with_TTA.__test__ = False                                  # (the reference's name; not a pytest test)

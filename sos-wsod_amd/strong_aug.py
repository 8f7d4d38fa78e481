"""Stage-3 strong augmentation: the recipe side (unbias/ubteacher/data/detection_utils.py:9-46, `build_strong_augmentation`).

The reference composes torchvision transforms over a PIL image: RandomApply(ColorJitter(0.4, 0.4, 0.4, 0.1), p=0.8),
RandomGrayscale(p=0.2), RandomApply(GaussianBlur(sigma ~ U[0.1, 2.0]), p=0.5), then three RandomErasing(value="random") between
ToTensor and ToPILImage.  Here the random decisions are drawn on the host into a `Recipe` (plain data), and the pixels are
computed by `ops.strong_augment_u8` / `ops.strong_augment_multi_u8` (sw_strong_aug_u8: HIP kernels, bit-identical to Pillow).
There is no CPU pixel path.

Draws come from a generator keyed by (seed, dataset index, visit counter), as `split.py` keys its draws: a recipe depends on
neither the worker count nor the batch neighbours.  (The reference's draws are unseeded.)  The distributions and the decision
structure are torchvision's: the order of the four jitter ops is a uniform permutation, brightness / contrast / saturation
factors are uniform in [1 - v, 1 + v], hue in [-h, h]; an erasing tries up to 10 times for a rectangle of area fraction
U(scale) and log-uniform aspect with `h < H and w < W`, top-left uniform over the valid positions, and erases nothing when all
ten fail.

Rules chosen where the reference leaves one open: the hue shift is `int(hue * 255)` truncated toward zero modulo 256 (numpy's
uint8 cast of a negative float is not defined alike across versions); the erased bytes come from a counter-based generator in the
kernel (reproducible per (seed, key, erasing, channel, y, x)), not from torch's `normal_` stream.
Quirk kept: the augmentation reads the three planes as R, G, B whatever INPUT.FORMAT says.
"""
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

JITTER_OPS = ("brightness", "contrast", "saturation", "hue")            # torchvision ColorJitter's fn_idx 0..3
ERASINGS = ((0.7, (0.05, 0.2), (0.3, 3.3)), (0.5, (0.02, 0.2), (0.1, 6.0)), (0.3, (0.02, 0.2), (0.05, 8.0)))   # (p, scale, ratio)


@dataclass(frozen=True)
class Recipe:
    """One image's strong augmentation.  order: () = jitter off, else distinct JITTER_OPS applied left to right (the reference draws a permutation of all four);
    blur_sigma None = no blur; rects: up to three (top, left, h, w) or None, one per erasing in turn; seed / key select the
    erased bytes."""
    order: Tuple[str, ...] = ()
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0
    hue: float = 0.0
    grayscale: bool = False
    blur_sigma: Optional[float] = None
    rects: Tuple[Optional[Tuple[int, int, int, int]], ...] = field(default=(None, None, None))
    seed: int = 0
    key: int = 0


def erase_rect(rng, H, W, scale, ratio):
    """torchvision RandomErasing.get_params -> (top, left, h, w) or None after 10 failed attempts"""
    area = H * W
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        erase_area = area * rng.uniform(scale[0], scale[1])
        aspect = math.exp(rng.uniform(lo, hi))
        h = int(round(math.sqrt(erase_area * aspect)))
        w = int(round(math.sqrt(erase_area / aspect)))
        if not (h < H and w < W):
            continue
        if h <= 0 or w <= 0:                                 # nothing to erase (images of a few pixels only)
            continue
        top = int(rng.integers(0, H - h + 1))
        left = int(rng.integers(0, W - w + 1))
        return top, left, h, w
    return None


class StrongAugmentation:
    """`draw(index, visit, hw) -> Recipe` with the reference's training recipe; `__call__(img, index, visit)` applies it on the
    device.  is_train=False is the reference's empty Compose: the recipe that changes nothing."""

    def __init__(self, seed: int = 0, is_train: bool = True, p_jitter=0.8, jitter=(0.4, 0.4, 0.4, 0.1), p_gray=0.2, p_blur=0.5,
                 sigma=(0.1, 2.0), erasings=ERASINGS):
        self.seed, self.is_train = int(seed), bool(is_train)
        self.p_jitter, self.jitter, self.p_gray, self.p_blur, self.sigma = p_jitter, tuple(jitter), p_gray, p_blur, tuple(sigma)
        self.erasings = tuple(erasings)

    def rng(self, index: int, visit: int = 0):
        return np.random.default_rng([self.seed & 0xFFFFFFFF, int(index), int(visit)])

    def draw(self, index: int, visit: int, hw) -> Recipe:
        key = ((int(index) & 0xFFFFFFFF) << 32) | (int(visit) & 0xFFFFFFFF)
        if not self.is_train:
            return Recipe(seed=self.seed, key=key)
        H, W = int(hw[0]), int(hw[1])
        rng = self.rng(index, visit)
        kw = {}
        if rng.random() < self.p_jitter:
            kw["order"] = tuple(JITTER_OPS[i] for i in rng.permutation(4))
            b, c, s, h = self.jitter
            kw["brightness"] = float(rng.uniform(max(0.0, 1 - b), 1 + b))
            kw["contrast"] = float(rng.uniform(max(0.0, 1 - c), 1 + c))
            kw["saturation"] = float(rng.uniform(max(0.0, 1 - s), 1 + s))
            kw["hue"] = float(rng.uniform(-h, h))
        if rng.random() < self.p_gray:
            kw["grayscale"] = True
        if rng.random() < self.p_blur:
            kw["blur_sigma"] = float(rng.uniform(self.sigma[0], self.sigma[1]))
        rects = []
        for p, scale, ratio in self.erasings:
            rects.append(erase_rect(rng, H, W, scale, ratio) if rng.random() < p else None)
        return Recipe(rects=tuple(rects), seed=self.seed, key=key, **kw)

    def __call__(self, img, index: int, visit: int = 0, out=None):
        from . import ops
        return ops.strong_augment_u8(img, self.draw(index, visit, img.shape[-2:]), out=out)


# ================================================================================================ the two-crop mapper
def _cfg_get(node, name, default=None):
    if node is None:
        return default
    if hasattr(node, "get"):
        return node.get(name, default)
    return getattr(node, name, default)


class DeviceTwoCropMapper:
    """`mapper(dataset_dict) -> (dict_strong, dict_weak)`: the reference's DatasetMapperTwoCropSeparate
    (unbias/ubteacher/data/dataset_mapper.py:18-157) on the device.

    Weak view: optional INPUT.CROP window, ResizeShortestEdge(min_sizes, max_size, sample_style) through
    `resize.resize_bilinear_u8` (Pillow-exact), RandomFlip(horizontal, p = 0.5; the mirrored image comes from the resize launch).
    Annotations go through the same transforms (`tta.ViewTransform`, float64 like the reference's numpy path), are clipped to the
    view, crowd objects are skipped and empty boxes filtered (filter_empty_instances, threshold 1e-5); `gt_classes` kept.
    Strong view: `StrongAugmentation` applied to the weak view's pixels, always read as R, G, B planes (the reference's
    `Image.fromarray(..., "RGB")` ignores INPUT.FORMAT; the quirk is kept) and returned in the same channel order as the weak view.
    Both dicts share ONE `instances` object and the image size.  is_train=False: the single resized dict without annotations.

    dataset_dict: "image" (3, h, w) uint8 device tensor in INPUT.FORMAT order (decoding stays with the caller), optional
    "annotations" (bbox, bbox_mode 0 = XYXY_ABS / 1 = XYWH_ABS, category_id, iscrowd).  Draws are keyed by (seed, index, visit):
    index = the argument, else dataset_dict["index"] / ["image_id"].  Masks, keypoints, semantic segmentation and precomputed
    proposals are refused.  resize_pixels=False: box / label side only (host logic tests; no pixels are produced)."""

    def __init__(self, min_sizes=(800,), max_size=1333, sample_style="choice", crop=None, flip_prob=0.5, seed=0, is_train=True,
                 img_format="BGR", resize_pixels=True, strong=None):
        assert sample_style in ("choice", "range")
        self.min_sizes, self.max_size, self.sample_style = tuple(min_sizes), int(max_size), sample_style
        self.crop = None if crop is None else (str(crop[0]), tuple(crop[1]))
        self.flip_prob, self.seed, self.is_train = float(flip_prob), int(seed), bool(is_train)
        self.img_format, self.resize_pixels = img_format, resize_pixels
        self.strong = strong if strong is not None else StrongAugmentation(seed, is_train)

    @classmethod
    def from_config(cls, cfg, is_train=True, seed=0, resize_pixels=True):
        if _cfg_get(cfg.MODEL, "MASK_ON", False) or _cfg_get(cfg.MODEL, "KEYPOINT_ON", False):
            raise ValueError("DeviceTwoCropMapper: MODEL.MASK_ON / MODEL.KEYPOINT_ON are not supported (no SoS-WSOD Stage-3 config uses them)")
        if _cfg_get(cfg.MODEL, "LOAD_PROPOSALS", False):
            raise ValueError("DeviceTwoCropMapper: MODEL.LOAD_PROPOSALS (precomputed proposals) is not supported in Stage 3")
        inp = cfg.INPUT
        crop_cfg = _cfg_get(inp, "CROP", None)
        crop = None
        if is_train and crop_cfg and _cfg_get(crop_cfg, "ENABLED", False):
            crop = (_cfg_get(crop_cfg, "TYPE", "relative_range"), _cfg_get(crop_cfg, "SIZE", [0.9, 0.9]))
        if is_train:
            sizes, mx, style = inp.MIN_SIZE_TRAIN, inp.MAX_SIZE_TRAIN, _cfg_get(inp, "MIN_SIZE_TRAIN_SAMPLING", "choice")
        else:
            sizes, mx, style = _cfg_get(inp, "MIN_SIZE_TEST", 800), _cfg_get(inp, "MAX_SIZE_TEST", 1333), "choice"
        sizes = (sizes,) if isinstance(sizes, int) else tuple(sizes)
        flip = 0.5 if is_train and _cfg_get(inp, "RANDOM_FLIP", "horizontal") == "horizontal" else 0.0
        if is_train and _cfg_get(inp, "RANDOM_FLIP", "horizontal") not in ("horizontal", "none"):
            raise ValueError("DeviceTwoCropMapper: INPUT.RANDOM_FLIP must be 'horizontal' or 'none'")
        return cls(min_sizes=sizes, max_size=mx, sample_style=style, crop=crop, flip_prob=flip, seed=seed, is_train=is_train,
                   img_format=_cfg_get(inp, "FORMAT", "BGR"), resize_pixels=resize_pixels)

    # ---- draws: a RandomState keyed by (seed, index, visit), in the reference's order (crop, scale, flip)
    def draw_geometry(self, index, visit, hw):
        """-> {"crop": (y0, x0, h, w) | None, "hw": output size, "flip": bool}"""
        from .mapper import crop_size_rule
        from .tta import DeviceTTAMapper
        h, w = int(hw[0]), int(hw[1])
        rng = np.random.RandomState([self.seed & 0xFFFFFFFF, int(index) & 0xFFFFFFFF, int(visit) & 0xFFFFFFFF, 0x2C])
        crop = None
        if self.crop is not None:
            ch, cw = crop_size_rule(self.crop[0], self.crop[1], h, w, rng)
            assert h >= ch and w >= cw, "Shape computation in RandomCrop has bugs."
            y0 = int(rng.randint(h - ch + 1))
            x0 = int(rng.randint(w - cw + 1))
            crop = (y0, x0, int(ch), int(cw))
            h, w = int(ch), int(cw)
        if self.sample_style == "range":
            size = int(rng.randint(self.min_sizes[0], self.min_sizes[1] + 1))
        else:
            size = int(rng.choice(self.min_sizes))
        new_hw = DeviceTTAMapper._shortest_edge(h, w, size, self.max_size)
        flip = bool(rng.uniform() < self.flip_prob) if self.flip_prob > 0 else False
        return {"crop": crop, "hw": new_hw, "flip": flip}

    @staticmethod
    def _index_of(d, index):
        if index is None:
            index = d.get("index", d.get("image_id"))
        if not isinstance(index, (int, np.integer)):
            raise ValueError("DeviceTwoCropMapper needs an integer dataset index (argument, or dataset_dict['index'] / ['image_id'])")
        return int(index)

    def map_weak(self, d, index=None, visit=0, draws=None):
        """-> (dict_weak, Recipe): everything but the strong pixels (the batch helper augments a whole batch in one call)"""
        import torch
        from .resize import resize_bilinear_u8
        from .structures import Boxes, Instances
        from .tta import ViewTransform
        for k in ("sem_seg_file_name", "sem_seg", "proposal_boxes", "proposal_file"):
            if k in d:
                raise ValueError(f"DeviceTwoCropMapper: dataset_dict[{k!r}] is not supported (semantic segmentation / precomputed proposals)")
        index = self._index_of(d, index)
        img = d["image"]
        dev = img.device
        h, w = int(img.shape[-2]), int(img.shape[-1])
        if "height" in d and (int(d["height"]), int(d["width"])) != (h, w):                    # check_image_size
            raise ValueError(f"mismatched image shape: the image is {h} x {w}, the dataset dict says {d['height']} x {d['width']}")
        g = draws if draws is not None else self.draw_geometry(index, visit, (h, w))
        crop, new_hw, flip = g["crop"], tuple(g["hw"]), bool(g["flip"])
        y0, x0, ch, cw = crop if crop is not None else (0, 0, h, w)
        win = img[:, y0:y0 + ch, x0:x0 + cw] if crop is not None else img
        if not self.resize_pixels:
            weak = torch.zeros(3, new_hw[0], new_hw[1], dtype=torch.uint8, device=dev)
        elif flip:
            weak = resize_bilinear_u8(win, new_hw, with_flip=True)[1]
        else:
            weak = resize_bilinear_u8(win, new_hw)
        out = {k: v for k, v in d.items() if k not in ("image", "annotations")}
        out.setdefault("height", h)
        out.setdefault("width", w)
        out["image"] = weak
        self.last_draws = dict(g, index=index, visit=visit)
        if not self.is_train:
            return out, Recipe(seed=self.strong.seed)
        if "annotations" in d:
            annos = [a for a in d["annotations"] if a.get("iscrowd", 0) == 0]
            b = np.asarray([a["bbox"] for a in annos], dtype=np.float64).reshape(-1, 4)
            mode = np.asarray([int(a.get("bbox_mode", 0)) for a in annos], dtype=np.int64)
            if ((mode != 0) & (mode != 1)).any():
                raise ValueError("DeviceTwoCropMapper: bbox_mode must be XYXY_ABS (0) or XYWH_ABS (1)")
            b[mode == 1, 2:] += b[mode == 1, :2]
            t = ViewTransform((ch, cw), new_hw, flip, crop_xy=(x0, y0) if crop is not None else None)
            b = t.apply_box(torch.from_numpy(b)).numpy()
            b = np.minimum(b.clip(min=0), [new_hw[1], new_hw[0], new_hw[1], new_hw[0]])
            b32 = b.astype(np.float32)                                                           # Boxes() holds float32
            keep = ((b32[:, 2] - b32[:, 0]) > 1e-5) & ((b32[:, 3] - b32[:, 1]) > 1e-5)             # filter_empty_instances
            cls_ids = np.asarray([int(a["category_id"]) for a in annos], dtype=np.int64)
            inst = Instances(new_hw)
            inst.gt_boxes = Boxes(torch.from_numpy(b32[keep]).to(dev))
            inst.gt_classes = torch.from_numpy(cls_ids[keep]).to(dev)
            out["instances"] = inst
        return out, self.strong.draw(index, visit, new_hw)

    def _rgb_order(self, img):
        """the strong augmentation reads plane 0 as R whatever the format: nothing to reorder (the kept quirk)"""
        return img

    def __call__(self, d, index=None, visit=0, draws=None, recipe=None):
        from . import ops
        weak, rc = self.map_weak(d, index, visit, draws)
        if not self.is_train:
            return weak
        rc = recipe if recipe is not None else rc
        self.last_recipe = rc
        strong = dict(weak)
        strong["image"] = ops.strong_augment_u8(weak["image"], rc) if self.resize_pixels else weak["image"].clone()
        return strong, weak


class TwoCropBatches:
    """Iterable of `(label_q, label_k, unlabel_q, unlabel_k)`, what `semisup.SemiSupStep.run_step` takes (q = strong, k = weak):
    the reference's AspectRatioGroupedSemiSupDatasetTwoCrop (unbias/ubteacher/data/common.py:92-176) over two streams of dataset
    indices.  Each stream fills one of two aspect-ratio buckets (w > h or not, by the dataset dict's "width" / "height"); a batch is
    yielded when a labelled and an unlabelled bucket are both full; as in the reference, while one side's bucket is full its
    stream's items are dropped until the other side fills.  The strong views of a whole batch (both streams) come from ONE
    `ops.strong_augment_multi_u8` call.

    image_loader(dict) -> (3, height, width) uint8 device tensor (decoding stays with the caller, as in split.score_images).
    label_order / unlabel_order: iterables of indices into the two lists; default: endless permutations seeded by `seed`.
    A (stream, index) pair's visit counter keys its draws: the same image gets a new view each time it comes round."""

    def __init__(self, mapper, label_dicts, unlabel_dicts, image_loader, batch_size_label, batch_size_unlabel, seed=0,
                 label_order=None, unlabel_order=None):
        self.mapper, self.image_loader = mapper, image_loader
        self.dicts = (list(label_dicts), list(unlabel_dicts))
        self.bs = (int(batch_size_label), int(batch_size_unlabel))
        self.seed = int(seed)
        self.orders = (label_order, unlabel_order)
        self.visits = ({}, {})

    def _endless(self, stream):
        rng = np.random.default_rng([self.seed & 0xFFFFFFFF, stream])
        n = len(self.dicts[stream])
        while True:
            yield from (int(i) for i in rng.permutation(n))

    def _mapped(self, stream, i):
        d = dict(self.dicts[stream][i])
        d["image"] = self.image_loader(d)
        visit = self.visits[stream].get(i, 0)
        self.visits[stream][i] = visit + 1
        # the two lists index their own datasets: the stream number goes into the key through the visit word's top bit
        return self.mapper.map_weak(d, index=d.get("index", i) if isinstance(d.get("index", i), int) else i, visit=visit | (stream << 31))

    def __iter__(self):
        from . import ops
        buckets = ([[], []], [[], []])                     # [stream][aspect group] -> list of (weak dict, recipe)
        cur = [[], []]                                     # the bucket each stream touched last (the reference's loop variables)
        orders = [o if o is not None else self._endless(s) for s, o in enumerate(self.orders)]
        for il, iu in zip(*orders):
            for s, i in ((0, il), (1, iu)):
                if len(cur[s]) != self.bs[s]:
                    d = self.dicts[s][i]
                    cur[s] = buckets[s][0 if d["width"] > d["height"] else 1]
                    cur[s].append(self._mapped(s, i))
            if len(cur[0]) == self.bs[0] and len(cur[1]) == self.bs[1]:
                pairs = cur[0] + cur[1]
                if self.mapper.resize_pixels:
                    strong = ops.strong_augment_multi_u8([w["image"] for w, _ in pairs], [rc for _, rc in pairs])
                else:
                    strong = [w["image"].clone() for w, _ in pairs]
                q = [dict(w, image=s_img) for (w, _), s_img in zip(pairs, strong)]
                k = [w for w, _ in pairs]
                nl = self.bs[0]
                yield q[:nl], k[:nl], q[nl:], k[nl:]
                del cur[0][:], cur[1][:]

"""Stage 2 -> 3: the loss-ranked data split (unbias/split_single.py, split_multi.py, generate_base_split.py and the Stage-3 loader's
divide_label_unlabel, unbias/ubteacher/data/build.py:33-56).

The Stage-2 pseudo-FSOD detector scores every training image by its summed training loss; the k lowest-loss images become the
labelled set of Stage 3, written to a "data seed" JSON file whose key is the SUP_PERCENT the Stage-3 config names.

    python -m sos_wsod_amd.split base --length N --save-path F
    python -m sos_wsod_amd.split loss --config voc_split.yaml --ckpt model.pth --save-path F --k 2000 --pgt PGT.json --voc-root VOC2007
    python -m torch.distributed.run --nproc_per_node G -m sos_wsod_amd.split loss ...      (the chunks are dealt to the ranks)

Scoring (score_images) is the reference's one-image training forward, batched: images of one padded input shape share a forward
and ops.det_loss_per_image (sw_det_loss_per_image) gives every image its losses as if it were alone.  Each image's augmentation
draw (the ResizeShortestEdge size, the flip) and its RPN / ROI label-sampler seeds come from a generator keyed by (seed, dataset
index): its score depends on the weights, the image, its index and the seed only — not on the batch size, its neighbours or the
number of ranks.  (The reference's draws are unseeded: its split is one random sample, this one a reproducible one.)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

XYXY_ABS, XYWH_ABS = 0, 1
# INPUT.MIN_SIZE_TRAIN / MAX_SIZE_TRAIN when neither the caller nor the config names them (detectron2/config/defaults.py)
MIN_SIZE_TRAIN, MAX_SIZE_TRAIN = (640, 672, 704, 736, 768, 800), 1333


# ================================================================================================ the split files
def loss_split(losses, k):
    """split_single.py:77-116 -> (the data-seed JSON object {str(percent): {"1": the k lowest-loss dataset indices}}, percent).
    Order: ascending loss, NaN last (torch.sort's rule); equal losses keep index order (the reference's unstable sort left ties
    undefined: this is the rule chosen here).  percent is the 7-decimal bisection of the reference; its key is str(percent), the
    text to paste into DATALOADER.SUP_PERCENT.  Where the reference would loop forever (its `begin = middle` typo, reached whenever
    int(length * middle) < k) or k exceeds the dataset, ValueError."""
    v = np.asarray(losses, dtype=np.float32).reshape(-1)
    length = int(v.shape[0])
    k = int(k)
    if k < 0 or k > length:
        raise ValueError(f"k = {k} is outside [0, {length}] (the dataset has {length} images)")
    nan = np.isnan(v)
    order = np.lexsort((np.arange(length), np.where(nan, 0.0, v), nan))       # last key first: NaN flag, loss, index
    l1 = [int(i) for i in order]
    percent = split_percent(length, k)
    return {str(percent): {"1": l1[:k]}}, percent


def split_percent(length, k):
    """split_single.py:94-109: the 7-decimal bisection for the percent whose int(percent / 100 * length) is k (ValueError where
    the reference loops forever)"""
    low, high = k / length, (k + 1) / length
    while True:
        middle = round((low + high) / 2, 7)
        val = int(length * middle)
        if val == k:
            percent = middle * 100
            break
        if val > k:
            if middle == high:
                raise ValueError(f"the percent bisection for k = {k} of {length} images makes no progress")
            high = middle
        else:
            raise ValueError(f"the percent bisection for k = {k} of {length} images reaches int({length} * {middle}) = {val} < k: "
                             "the reference's search loops forever here (split_single.py:108 `begin = middle`)")
    return percent


def base_split(length):
    """generate_base_split.py: the data seed of "every image but the last" (Stage 2's pseudo-FSOD training set): the (0, 100)
    bisection for length - 1 images -> ({str(percent): {"1": [0 .. length - 2]}}, percent).  A bisection that stops making
    progress raises ValueError (the reference would loop forever)."""
    length = int(length)
    if length < 1:
        raise ValueError(f"length = {length}: at least one image is needed")
    target = length - 1
    low, high = 0, 100
    while True:
        middle = round((low + high) / 2, 7)
        val = int(middle / 100 * length)
        if val == target:
            percent = middle
            break
        if middle == low or middle == high:
            raise ValueError(f"the percent bisection for {target} of {length} images makes no progress")
        if val < target:
            low = middle
        else:
            high = middle
    return {str(percent): {"1": list(range(target))}}, percent


def write_split(split_dict, path):
    """json.dump with its default separators, no trailing newline: the bytes the reference writes"""
    with open(path, "w") as f:
        json.dump(split_dict, f)


def divide_label_unlabel(dataset_dicts, sup_percent, random_data_seed, random_data_seed_path):
    """unbias/ubteacher/data/build.py:33-56: (labelled dicts, unlabelled dicts) by the data-seed file's entry
    [str(sup_percent)][str(random_data_seed)], with the reference's count check."""
    num_all = len(dataset_dicts)
    num_label = int(sup_percent / 100.0 * num_all)
    with open(random_data_seed_path) as f:
        seeds = json.load(f)
    labeled_idx = np.array(seeds[str(sup_percent)][str(random_data_seed)])
    assert labeled_idx.shape[0] == num_label, "Number of READ_DATA is mismatched."
    labeled_idx = set(labeled_idx.tolist())
    label_dicts, unlabel_dicts = [], []
    for i in range(num_all):
        (label_dicts if i in labeled_idx else unlabel_dicts).append(dataset_dicts[i])
    return label_dicts, unlabel_dicts


def data_seed_keys(cfg):
    """(SUP_PERCENT, RANDOM_DATA_SEED, RANDOM_DATA_SEED_PATH) of a config's DATALOADER (ubteacher/config.py defaults)"""
    d = cfg.get("DATALOADER", {}) if hasattr(cfg, "get") else {}
    return float(d.get("SUP_PERCENT", 100.0)), int(d.get("RANDOM_DATA_SEED", 0)), d.get("RANDOM_DATA_SEED_PATH", "dataseed/COCO_supervision.txt")


def load_student_state(path):
    """split_single.py:44-49: the student's weights of a Stage-3 checkpoint, "modelStudent." (13 characters) cut off"""
    state = torch.load(path, map_location="cpu", weights_only=False)["model"]
    return {key[13:]: v for key, v in state.items() if "Student" in key}


# ================================================================================================ scoring
class _KeyedSeeds:
    """the label samplers' seeds of one batch, in the order the detector draws them: the RPN's (positives, negatives) per image,
    then the ROI heads' (foreground, background) per image"""

    def __init__(self, seeds):
        self.seeds, self.k = list(seeds), 0

    def next_seed(self):
        s = self.seeds[self.k]
        self.k += 1
        return s


def _draws(seed, index, n_sizes):
    """the per-image draws, from a generator keyed by (seed, dataset index): size choice, flip, 4 sampler seeds"""
    rng = np.random.default_rng([int(seed) & 0xFFFFFFFF, int(index)])
    size_i = int(rng.integers(n_sizes))
    flip = bool(rng.random() < 0.5)
    seeds = [int(x) for x in rng.integers(0, 2 ** 63, size=4, dtype=np.int64)]
    return size_i, flip, seeds


def filter_empty(dataset_dicts):
    """DATALOADER.FILTER_EMPTY_ANNOTATIONS (default True): images without annotations are dropped before anything is indexed —
    the index space is then the one divide_label_unlabel sees"""
    return [d for d in dataset_dicts if len(d.get("annotations", ())) > 0]


def _gt_boxes(d, h, w, nh, nw, flip):
    """the train mapper's annotation transform (detection_utils.py: transform_instance_annotations, annotations_to_instances,
    filter_empty_instances): resize, flip, clip to the image, boxes of no extent dropped -> (boxes (n, 4) f32, classes (n,) i64)"""
    boxes, classes = [], []
    for a in d.get("annotations", ()):
        if a.get("iscrowd", 0):
            continue
        b = [float(v) for v in a["bbox"]]
        mode = int(a.get("bbox_mode", XYXY_ABS))
        if mode == XYWH_ABS:
            b = [b[0], b[1], b[0] + b[2], b[1] + b[3]]
        elif mode != XYXY_ABS:
            raise ValueError(f"bbox_mode {mode} is not supported (XYXY_ABS, XYWH_ABS)")
        boxes.append(b); classes.append(int(a["category_id"]))
    bx = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    sx, sy = np.float32(nw / w), np.float32(nh / h)
    bx = bx * np.array([sx, sy, sx, sy], dtype=np.float32)
    if flip:
        bx = np.stack([nw - bx[:, 2], bx[:, 1], nw - bx[:, 0], bx[:, 3]], 1).astype(np.float32)
    bx = np.minimum(np.maximum(bx, 0), np.array([nw, nh, nw, nh], dtype=np.float32))
    keep = ((bx[:, 2] - bx[:, 0]) > 1e-5) & ((bx[:, 3] - bx[:, 1]) > 1e-5)
    return bx[keep], np.asarray(classes, dtype=np.int64)[keep]


def plan(dataset_dicts, *, min_sizes, max_size, images_per_batch, seed, size_divisibility=32):
    """The batch plan: every image's (index, output size, flip, seeds); images bucketed by padded input shape (buckets in shape
    order), each bucket cut into chunks of images_per_batch in index order -> list of chunks, each a list of such entries."""
    from .tta import DeviceTTAMapper
    buckets = {}
    for i, d in enumerate(dataset_dicts):
        h, w = int(d["height"]), int(d["width"])
        si, flip, seeds = _draws(seed, i, len(min_sizes))
        nh, nw = DeviceTTAMapper._shortest_edge(h, w, int(min_sizes[si]), int(max_size))
        pad = (-(-nh // size_divisibility) * size_divisibility, -(-nw // size_divisibility) * size_divisibility)
        buckets.setdefault(pad, []).append(dict(index=i, hw=(h, w), out=(nh, nw), flip=flip, seeds=seeds))
    chunks = []
    for pad in sorted(buckets):
        b = buckets[pad]
        chunks += [b[j:j + images_per_batch] for j in range(0, len(b), images_per_batch)]
    return chunks


def score_images(model, dataset_dicts, image_loader, *, images_per_batch=8, seed=0, min_sizes=MIN_SIZE_TRAIN, max_size=MAX_SIZE_TRAIN,
                 all_losses=False):
    """One f32 loss per dataset index: loss_cls + loss_box_reg + loss_rpn_cls + loss_rpn_loc of the training-mode forward without
    gradient (split_single.py:66-75), each image as if alone in its batch.  dataset_dicts: the detectron2 dicts ("height",
    "width", "annotations" with "bbox" / "bbox_mode" / "category_id"), empty ones already dropped (filter_empty);
    image_loader(dict) -> (3, height, width) uint8 tensor in the model's channel order (BGR for detectron2's recipes).
    min_sizes / max_size: the config's INPUT.MIN_SIZE_TRAIN / MAX_SIZE_TRAIN (default: detectron2's).  all_losses: return the
    (n, 5) array of loss_cls, loss_box_reg, loss_rpn_cls, loss_rpn_loc and their sum instead of the sums alone.
    Under torch.distributed the plan's chunks go round-robin to the ranks and every rank returns the whole array.
    Batch-size independence is exact for the plan (draws, seeds, sampling) and approximate for the numbers: the backbone's
    reduction splits depend on the batch, so a score moves by up to ~3e-4 relative at 800 x 1067."""
    import torch.distributed as dist
    from .structures import Boxes, Instances
    from .resize import resize_bilinear_u8
    min_sizes, max_size = tuple(min_sizes), int(max_size)
    if images_per_batch < 1:
        raise ValueError("images_per_batch must be >= 1")
    dev = model.device
    chunks = plan(dataset_dicts, min_sizes=min_sizes, max_size=max_size, images_per_batch=images_per_batch, seed=seed,
                  size_divisibility=model.backbone.size_divisibility)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    rpn, roi = model.proposal_generator, model.roi_heads
    saved = (rpn.sampler, roi.sampler, model.training)
    got = {}
    from contextlib import nullcontext
    from .events import EventStorage, has_event_storage
    try:
        model.train()
        with torch.no_grad(), (nullcontext() if has_event_storage() else EventStorage(0)):
            for chunk in chunks[rank::world]:
                batch = []
                for e in chunk:
                    d = dataset_dicts[e["index"]]
                    img = image_loader(d)
                    if not torch.is_tensor(img):
                        img = torch.from_numpy(np.ascontiguousarray(img))
                    img = img.to(dev)
                    if tuple(img.shape[1:]) != e["hw"]:
                        raise ValueError(f"image {e['index']}: loaded {tuple(img.shape)}, the dict says {e['hw']}")
                    r = resize_bilinear_u8(img, e["out"], with_flip=e["flip"])
                    im = r[1] if e["flip"] else r
                    nh, nw = e["out"]
                    b, c = _gt_boxes(d, e["hw"][0], e["hw"][1], nh, nw, e["flip"])
                    inst = Instances((nh, nw))
                    inst.gt_boxes = Boxes(torch.from_numpy(b).to(dev)); inst.gt_classes = torch.from_numpy(c).to(dev)
                    batch.append({"image": im, "instances": inst, "height": e["hw"][0], "width": e["hw"][1]})
                keys = _KeyedSeeds([s for e in chunk for s in e["seeds"][:2]] + [s for e in chunk for s in e["seeds"][2:]])
                rpn.sampler = roi.sampler = keys
                out = model.image_losses(batch).cpu().numpy()
                for e, v in zip(chunk, out):
                    got[e["index"]] = v
    finally:
        rpn.sampler, roi.sampler = saved[0], saved[1]
        model.train(saved[2])
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, got)
        got = {k: v for p in parts for k, v in p.items()}
    if len(got) != len(dataset_dicts):
        raise RuntimeError(f"scored {len(got)} of {len(dataset_dicts)} images")
    res = np.stack([got[i] for i in range(len(dataset_dicts))]).astype(np.float32) if got else np.zeros((0, 5), np.float32)
    return res if all_losses else np.ascontiguousarray(res[:, 4])


# ================================================================================================ command line
def _voc_dicts(pgt_files, voc_root):
    """dataset dicts of VOC pseudo-label files (pseudo_labels.load_voc_pseudo_labels), images under voc_root/JPEGImages, sizes read
    from the JPEG headers.  The dataset index order is each file's key order, files in the order given: the order in which
    pseudo_labels writes the split's images (its ImageSets/Main list), and so the order divide_label_unlabel sees when Stage 3 loads
    the same files.  A file whose keys were reordered would label the wrong images: it is the caller's to keep them in split order."""
    from PIL import Image
    from .pseudo_labels import load_voc_pseudo_labels
    dicts = []
    for path in pgt_files:
        with open(path) as f:
            pgt = json.load(f)
        images = []
        for key in pgt:
            if key == "multi_label":
                continue
            fn = os.path.join(voc_root, "JPEGImages", f"{int(key):06d}.jpg")
            with Image.open(fn) as im:
                w, h = im.size
            images.append({"image_id": f"{int(key):06d}", "file_name": fn, "height": h, "width": w})
        dicts += load_voc_pseudo_labels(pgt, images)
    return dicts


def _pillow_bgr(d):
    from PIL import Image
    with Image.open(d["file_name"]) as im:
        a = np.asarray(im.convert("RGB"))
    return torch.from_numpy(np.ascontiguousarray(a[:, :, ::-1].transpose(2, 0, 1)))


def parse_args(argv=None):
    p = argparse.ArgumentParser("python -m sos_wsod_amd.split", description="Stage 2 -> 3: the data-seed files of the split.")
    sub = p.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("base", help="generate_base_split.py: every image but the last")
    b.add_argument("--length", type=int, help="number of training images")
    b.add_argument("--pgt", nargs="+", help="or: count the images with annotations in these VOC pseudo-label files")
    b.add_argument("--save-path", required=True)
    s = sub.add_parser("loss", help="split_single.py / split_multi.py: the k lowest-loss images")
    s.add_argument("--config", default="./configs/split/voc_split.yaml")
    s.add_argument("--ckpt", default="./output/voc_baseline/model_0007999.pth")
    s.add_argument("--save-path", default="./dataseed/VOC07_oicr_plus_split.txt")
    s.add_argument("--k", default=2000, type=int)
    s.add_argument("--pgt", nargs="+", help="VOC pseudo-label files of the training splits, in DATASETS.TRAIN order")
    s.add_argument("--voc-root", default="datasets/VOC2007")
    s.add_argument("--images-per-batch", type=int, default=8)
    s.add_argument("--seed", type=int, default=0)
    s.add_argument("--decode", choices=("pillow", "device"), default="pillow",
                   help="pillow: decode on the host, one thread; device: image_io.JpegLoader (Huffman decoding on the host, the "
                        "pixels on the GPU, equal to Pillow's; unlike pillow it also applies the EXIF orientation, as the "
                        "reference's read_image does)")
    return p.parse_args(argv)


def main(argv=None, *, scorer=None, dataset_dicts=None):
    """scorer(model, dicts, image_loader, images_per_batch=, seed=, min_sizes=, max_size=) and dataset_dicts replace the GPU
    scoring and the VOC reading (tests)"""
    args = parse_args(argv)
    if args.cmd == "base":
        if args.length is None and not args.pgt:
            raise SystemExit("base: --length or --pgt is needed")
        if args.length is not None:
            length = args.length
        else:
            length = 0
            for path in args.pgt:
                with open(path) as f:
                    length += sum(1 for k, v in json.load(f).items() if k != "multi_label" and len(v) > 0)
        split_dict, percent = base_split(length)
        write_split(split_dict, args.save_path)
        print(f"The finded percent is: {percent}")
        return split_dict
    from .config import get_cfg
    print("loading config file")
    cfg = get_cfg()
    cfg.merge_from_file(args.config)
    inp = cfg.get("INPUT", {})
    min_sizes, max_size = tuple(inp.get("MIN_SIZE_TRAIN", MIN_SIZE_TRAIN)), int(inp.get("MAX_SIZE_TRAIN", MAX_SIZE_TRAIN))
    if dataset_dicts is None:
        if not args.pgt:
            raise SystemExit("loss: --pgt is needed (the training splits' pseudo-label files)")
        dataset_dicts = _voc_dicts(args.pgt, args.voc_root)
    dicts = filter_empty(dataset_dicts)
    if scorer is None:
        import torch.distributed as dist
        from .frcnn import TwoStagePseudoLabGeneralizedRCNN
        if "LOCAL_RANK" in os.environ and not dist.is_initialized():
            torch.cuda.set_device(int(os.environ["LOCAL_RANK"]) % torch.cuda.device_count())    # (ranks may share a device)
            dist.init_process_group("gloo")
        print("loading state_dict")
        model = TwoStagePseudoLabGeneralizedRCNN(cfg).cuda()
        print(model.load_state_dict(load_student_state(args.ckpt), strict=True))
        scorer, target = score_images, model
    else:
        target = None
    print("loss calculating")
    if args.decode == "device":
        from .image_io import JpegLoader
        loader = JpegLoader("BGR")
    else:
        loader = _pillow_bgr
    losses = scorer(target, dicts, loader, images_per_batch=args.images_per_batch, seed=args.seed, min_sizes=min_sizes,
                    max_size=max_size)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
        return None
    split_dict, percent = loss_split(losses, args.k)
    print(f"The finded percent is: {percent}")
    write_split(split_dict, args.save_path)
    return split_dict


if __name__ == "__main__":
    main(sys.argv[1:])

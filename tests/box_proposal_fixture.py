"""Box-proposal AR fixtures (tests/golden/box_proposal_*.npz, made by tests/golden/make_box_proposal_golden.py from the reference's
`_evaluate_box_proposals`): the seeded generator of the inputs, shared by that script and the tests (the `.npz` files hold the
reference's results and a SHA-256 of the generated inputs, not the inputs), and the loaders.

A case is (dataset, predictions, settings): `dataset` the annotation file's dict, `predictions` a list of {"image_id", "boxes" f32
[n, 4] xyxy, "logits" f32 [n]} in the order the evaluator would hold them, `settings` the (area name, limit) pairs evaluated."""
import hashlib
import os

import numpy as np

CASES = ("hand", "random", "coco")
AREA_NAMES = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")
EVALUATOR_SETTINGS = tuple((a, l) for l in (100, 1000) for a in ("all", "small", "medium", "large"))      # coco_evaluation.py:285-288
EVALUATOR_KEYS = tuple("AR{}@{:d}".format({"all": "", "small": "s", "medium": "m", "large": "l"}[a], l) for a, l in EVALUATOR_SETTINGS)


def key(area, limit):
    return f"{area}/{'none' if limit is None else limit}"


def _pred(image_id, boxes, logits):
    return {"image_id": image_id, "boxes": np.asarray(boxes, dtype=np.float32).reshape(-1, 4),
            "logits": np.asarray(logits, dtype=np.float32).reshape(-1)}


def _distinct_logits(rng, n):
    """n different float32 values in random order (no ties: the order among equal logits is torch's own)"""
    return (rng.permutation(n).astype(np.float32) / np.float32(8.0) - np.float32(n / 16.0)).astype(np.float32)


def hand():
    ds = {"images": [], "categories": [{"id": 1, "name": "thing"}], "annotations": []}
    preds = []

    def image(i):
        ds["images"].append({"id": i, "height": 480, "width": 640, "file_name": f"{i:012d}.jpg"})
        return i

    def ann(i, box, area=None, crowd=0):
        ds["annotations"].append({"id": len(ds["annotations"]) + 1, "image_id": i, "category_id": 1, "bbox": list(box),
                                  "area": box[2] * box[3] if area is None else area, "iscrowd": crowd})

    # 1: one proposal best for two identical boxes: the first box takes it, the second gets the runner-up
    i = image(1)
    ann(i, [10.0, 10.0, 50.0, 50.0])
    ann(i, [10.0, 10.0, 50.0, 50.0])
    preds.append(_pred(i, [[10, 10, 60, 60], [10, 10, 60, 55], [300, 300, 320, 320]], [3.0, 2.0, 1.0]))
    # 2: identical proposals: the first index wins; the second box then gets the twin
    i = image(2)
    ann(i, [100.0, 100.0, 40.0, 40.0])
    ann(i, [100.0, 100.0, 40.0, 30.0])
    preds.append(_pred(i, [[100, 100, 140, 130], [100, 100, 140, 130], [0, 0, 5, 5]], [0.5, 0.25, 0.125]))
    # 3: all-disjoint boxes: zeros, and the pairs are still used up in index order
    i = image(3)
    for k in range(3):
        ann(i, [20.0 + 100 * k, 20.0, 30.0, 30.0])
    preds.append(_pred(i, [[500, 400, 520, 420], [530, 400, 550, 420], [560, 400, 580, 420], [590, 400, 610, 420]],
                       [4.0, 3.0, 2.0, 1.0]))
    # 4: IoU exactly 0.5
    i = image(4)
    ann(i, [0.0, 0.0, 1.0, 1.0])
    preds.append(_pred(i, [[0, 0, 2, 1]], [1.0]))
    # 5: areas at the range borders (the annotation's own area decides, in float32)
    i = image(5)
    for k, area in enumerate((1023.9999, 1024, 1024.00001, 9216)):
        ann(i, [50.0 + 120 * k, 200.0, 40.0, 40.0], area=area)
    preds.append(_pred(i, [[50 + 120 * k, 200, 90 + 120 * k, 236 + k] for k in range(4)], [4.0, 3.0, 2.0, 1.0]))
    # 6 / 7: integer-valued and float bbox lists
    i = image(6)
    ann(i, [10, 20, 30, 40], area=1200)
    ann(i, [200, 20, 100, 100], area=10000)
    preds.append(_pred(i, [[11, 21, 40, 60], [205, 25, 300, 118]], [2.0, 1.0]))
    i = image(7)
    ann(i, [10.1, 20.2, 30.3, 40.4])
    ann(i, [200.7, 33.3, 99.9, 101.1])
    preds.append(_pred(i, [[10.4, 20.1, 40.2, 60.9], [201.3, 30.7, 299.2, 133.3]], [2.0, 1.0]))
    # 8: fewer proposals than boxes: trailing zeros
    i = image(8)
    for k in range(5):
        ann(i, [10.0 + 60 * k, 300.0, 50.0, 50.0])
    preds.append(_pred(i, [[130, 300, 180, 345], [70, 305, 120, 350]], [2.0, 1.0]))
    # 9: one proposal, one box; listed twice below
    i = image(9)
    ann(i, [400.0, 10.0, 64.0, 64.0])
    preds.append(_pred(i, [[400, 10, 464, 70]], [0.0]))
    # 10 / 11: as many proposals as limit 2, and one more: the third in rank is the best one
    for i, n in ((image(10), 2), (image(11), 3)):
        ann(i, [300.0, 300.0, 80.0, 80.0])
        ann(i, [100.0, 300.0, 80.0, 80.0])
        boxes = [[300, 300, 380, 360], [100, 300, 180, 340], [300, 300, 380, 380]][:n]
        preds.append(_pred(i, boxes, [3.0, 2.0, 1.0][:n]))
    # 12: ground truth and no proposals: not counted.  13: crowd boxes only.  999: unknown to the annotations
    i = image(12)
    ann(i, [10.0, 10.0, 100.0, 100.0])
    preds.append(_pred(i, np.zeros((0, 4)), np.zeros(0)))
    i = image(13)
    ann(i, [10.0, 10.0, 100.0, 100.0], crowd=1)
    ann(i, [200.0, 10.0, 100.0, 100.0], crowd=1)
    preds.append(_pred(i, [[10, 10, 110, 110]], [1.0]))
    preds.append(_pred(999, [[10, 10, 110, 110]], [1.0]))
    # 15: inverted proposals (x2 < x1, y2 < y1) beside a plain one; a crowd box among plain ones; proposals out of rank order
    i = image(15)
    ann(i, [50.0, 50.0, 100.0, 100.0])
    ann(i, [45.0, 45.0, 110.0, 110.0], crowd=1)
    ann(i, [300.0, 50.0, 60.0, 200.0])
    preds.append(_pred(i, [[150, 150, 50, 50], [150, 50, 50, 150], [60, 60, 150, 150], [300, 60, 350, 250], [50, 150, 150, 50]],
                       [0.5, 4.0, 1.0, 3.0, 2.0]))
    # 16: two boxes tie on the best proposal (IoU 0.8 each); the loser's runner-up differs: 0.3 for the second box, 0.625 for the first
    i = image(16)
    ann(i, [0.0, 0.0, 100.0, 80.0])
    ann(i, [0.0, 20.0, 100.0, 80.0])
    preds.append(_pred(i, [[0, 0, 100, 100], [0, 0, 100, 50]], [2.0, 1.0]))
    # 17: two proposals tie on the first box (IoU 0.8 each); what is left for the second box differs: 5/11 or 3/13
    i = image(17)
    ann(i, [0.0, 0.0, 100.0, 100.0])
    ann(i, [0.0, 50.0, 100.0, 80.0])
    preds.append(_pred(i, [[0, 0, 100, 80], [0, 20, 100, 100]], [2.0, 1.0]))
    preds.append(dict(preds[8]))                                   # a prediction listed twice is evaluated twice
    assert preds[8]["image_id"] == 9
    assert all(a["area"] < 512 ** 2 for a in ds["annotations"])    # nothing in 512-inf: num_pos 0, NaN
    return ds, preds, tuple((a, l) for a in AREA_NAMES for l in (None, 1, 2, 100))


def _grid_split(rng, n_img):
    """boxes on a 16-pixel grid: exact ties and zero-size proposals abound"""
    ids = rng.choice(np.arange(1, 30 * n_img), n_img, replace=False).tolist()
    ds = {"images": [{"id": int(i), "height": 640, "width": 640, "file_name": f"{int(i):012d}.jpg"} for i in ids],
          "categories": [{"id": 1, "name": "thing"}], "annotations": []}
    preds = []
    for n, i in enumerate(ids):
        for _ in range(int(rng.integers(0, 13)) if n % 9 else 0):
            x, y = (int(v) * 16 for v in rng.integers(0, 30, 2))
            w, h = (int(v) * 16 for v in rng.integers(1, 40, 2))
            scale = (1, 1, 0.5, 0.25)[int(rng.integers(0, 4))]
            ds["annotations"].append({"id": len(ds["annotations"]) + 1, "image_id": int(i), "category_id": 1,
                                      "bbox": [x, y, w, h] if rng.random() < 0.5 else [float(x), float(y), float(w), float(h)],
                                      "area": w * h * scale, "iscrowd": int(rng.random() < 0.15)})
        m = 0 if n % 11 == 5 else int(rng.integers(1, 201))
        x1 = rng.integers(0, 36, m) * 16
        y1 = rng.integers(0, 36, m) * 16
        boxes = np.stack([x1, y1, x1 + rng.integers(0, 24, m) * 16, y1 + rng.integers(0, 24, m) * 16], 1) if m else np.zeros((0, 4))
        preds.append(_pred(int(i), boxes, _distinct_logits(rng, m)))
    return ds, preds


def _gaussian_split(rng, n_img, max_props, max_boxes):
    """COCO-like: up to max_boxes objects per image (skewed to few), proposals placed around them with Gaussian noise, so the
    coordinates are not representable and the division rounds"""
    ids = rng.choice(np.arange(1, 30 * n_img), n_img, replace=False).tolist()
    ds = {"images": [{"id": int(i), "height": 480, "width": 640, "file_name": f"{int(i):012d}.jpg"} for i in ids],
          "categories": [{"id": 1, "name": "thing"}], "annotations": []}
    preds = []
    for n, i in enumerate(ids):
        g = max_boxes if n == 3 else int(min(max_boxes, 1 + rng.exponential(6.0)))
        sizes = np.exp(rng.uniform(np.log(8), np.log(400), (g, 2)))
        xy = rng.uniform(0, 1, (g, 2)) * np.array([640.0, 480.0])
        gt = np.round(np.concatenate([xy, sizes], 1), 2)
        for b in gt:
            ds["annotations"].append({"id": len(ds["annotations"]) + 1, "image_id": int(i), "category_id": 1,
                                      "bbox": [float(v) for v in b], "area": round(float(b[2] * b[3] * rng.uniform(0.3, 1.0)), 2),
                                      "iscrowd": int(rng.random() < 0.03)})
        m = max_props if n == 3 else int(rng.integers(max_props // 3, max_props + 1))
        src = gt[rng.integers(0, g, m)]
        near = rng.random(m) < 0.6
        cx = np.where(near, src[:, 0] + src[:, 2] / 2 + rng.normal(0, 0.15, m) * src[:, 2], rng.uniform(0, 640, m))
        cy = np.where(near, src[:, 1] + src[:, 3] / 2 + rng.normal(0, 0.15, m) * src[:, 3], rng.uniform(0, 480, m))
        w = np.where(near, src[:, 2] * np.exp(rng.normal(0, 0.2, m)), np.exp(rng.uniform(np.log(8), np.log(400), m)))
        h = np.where(near, src[:, 3] * np.exp(rng.normal(0, 0.2, m)), np.exp(rng.uniform(np.log(8), np.log(400), m)))
        boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
        preds.append(_pred(int(i), boxes, _distinct_logits(rng, m)))
    return ds, preds


def random():
    ds, preds = _grid_split(np.random.default_rng(11), 40)
    return ds, preds, tuple((a, l) for a in AREA_NAMES for l in (1, 2, 100, None)) + tuple(s for s in EVALUATOR_SETTINGS if s[1] == 1000)


def coco():
    ds, preds = _gaussian_split(np.random.default_rng(12), 150, 1200, 90)
    return ds, preds, EVALUATOR_SETTINGS


_MAKERS = {"hand": hand, "random": random, "coco": coco}
_cache = {}


def case(name):
    """(dataset, predictions, settings) of a case; built once per process — treat it as read-only"""
    if name not in _cache:
        _cache[name] = _MAKERS[name]()
    return _cache[name]


def inputs_sha256(ds, preds):
    h = hashlib.sha256()
    for a in ds["annotations"]:
        h.update(repr((a["id"], a["image_id"], [float(v) for v in a["bbox"]], float(a["area"]), int(a["iscrowd"]),
                       all(isinstance(v, int) for v in a["bbox"]))).encode())
    for p in preds:
        h.update(repr(p["image_id"]).encode())
        h.update(np.ascontiguousarray(p["boxes"]).tobytes())
        h.update(np.ascontiguousarray(p["logits"]).tobytes())
    return h.hexdigest()


def load(golden_dir, name):
    """the reference's results of a case: {key(area, limit) + "/gt_overlaps" | "/recalls" | "/ar" | "/num_pos": array, "sha256"};
    refuses a file made from other inputs than this generator's"""
    z = dict(np.load(os.path.join(golden_dir, f"box_proposal_{name}.npz")))
    ds, preds, _ = case(name)
    assert str(z["sha256"]) == inputs_sha256(ds, preds), f"box_proposal_{name}.npz was made from other inputs"
    return z


def records(preds):
    """the predictions as the evaluator holds them: [{"image_id", "proposals": Instances(proposal_boxes, objectness_logits)}]"""
    import torch
    from sos_wsod_amd.structures import Boxes, Instances
    out = []
    for p in preds:
        inst = Instances((480, 640))
        inst.proposal_boxes = Boxes(torch.from_numpy(p["boxes"].copy()))
        inst.objectness_logits = torch.from_numpy(p["logits"].copy())
        out.append({"image_id": p["image_id"], "proposals": inst})
    return out

"""Generate tests/golden/coco_eval_{hand,random,coco}.npz by RUNNING the reference's cocoeval.cpp
(uwsod/detectron2/layers/csrc/cocoeval/cocoeval.cpp: EvaluateImages and Accumulate, what COCOeval_opt calls) on synthetic
splits — build container only:

    python tests/golden/make_coco_eval_golden.py REFERENCE_ROOT [OUT_DIR]          (default OUT_DIR: tests/golden)

cocoeval.cpp is compiled from its place in the reference tree into a temporary directory, together with a small pybind11 binding
written here (InstanceAnnotation, ImageEvaluation, EvaluateImages, Accumulate); nothing compiled is kept.  pycocotools is not
installed, so what COCOeval_opt.evaluate() does around the two calls (COCO / loadRes / _prepare / computeIoU with maskApi.c's
bbIou) comes from tests/coco_eval_fixture.py, with `params` a SimpleNamespace; summarize and _derive_coco_results are restated
there too and applied to the arrays the C++ returned.  Stored: the inputs as compact arrays, and the reference's precision,
scores and recall (for "coco", where precision and scores would be 7.7 MB each, their SHA-256 and a CRC-32 per category slice),
the twelve stats and the result dict's values.

Cases
  hand    IoU exactly 0.5 and 0.75 (>= matches); two ground truths at equal IoU (the later wins); a crowd box matched by several
          detections; the break rule (a better IoU on an ignored ground truth behind a held non-ignored match); a ground truth
          outside the area range and an unmatched detection outside it; an annotation with id 0; area different from w * h on
          either side of 32^2; 130 detections in one (image, category), against 20 objects (100 x 20 IoUs: beyond the LDS slice)
          and a pair with 70 objects (beyond 64); score ties within and across images; a category without ground truth, one
          without detections, an image without detections; no ground truth in the large range at all (APl = NaN); a detection
          of an unknown category; zero-width boxes; a category of 1,500 detections (more than one 1,024 accumulate tile).
  random  200 images, 12 categories, 8 % crowd, up to 40 detections per image.
  coco    500 images, 80 categories, up to 100 detections per image."""
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import coco_eval_fixture as F  # noqa: E402

BINDING = r"""
#include "cocoeval.h"
namespace C = detectron2::COCOeval;
PYBIND11_MODULE(ref_cocoeval, m) {
  py::class_<C::InstanceAnnotation>(m, "InstanceAnnotation").def(py::init<uint64_t, double, double, bool, bool>());
  py::class_<C::ImageEvaluation>(m, "ImageEvaluation").def(py::init<>());
  m.def("EvaluateImages", &C::EvaluateImages);
  m.def("Accumulate", &C::Accumulate);
}
"""


def build_reference(ref_root, tmp):
    import pybind11
    src = os.path.join(ref_root, "uwsod", "detectron2", "layers", "csrc", "cocoeval")
    bind = os.path.join(tmp, "binding.cpp")
    with open(bind, "w") as f:
        f.write(BINDING)
    out = os.path.join(tmp, "ref_cocoeval" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-I" + pybind11.get_include(),
                           "-I" + sysconfig.get_paths()["include"], "-I" + src, os.path.join(src, "cocoeval.cpp"), bind, "-o", out])
    spec = importlib.util.spec_from_file_location("ref_cocoeval", out)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run_reference(C, ds, res):
    """COCOeval_opt.evaluate() + accumulate() with the two C++ calls"""
    img_ids, cat_ids, gts, dts = F.prepare(ds, res)
    p = types.SimpleNamespace(imgIds=img_ids, catIds=cat_ids, iouThrs=F.IOU_THRS, recThrs=F.REC_THRS, maxDets=F.MAX_DETS,
                              areaRng=F.AREA_RNG, useCats=1)

    def cpp(instances, is_det=False):
        return [C.InstanceAnnotation(int(o["id"]), o["score"] if is_det else o.get("score", 0.0), o["area"],
                                     bool(o.get("iscrowd", 0)), bool(o.get("ignore", 0))) for o in instances]

    ious = [[F.compute_iou(gts[i, c], dts[i, c]) for c in cat_ids] for i in img_ids]
    gt_inst = [[cpp(gts[i, c]) for c in cat_ids] for i in img_ids]
    dt_inst = [[cpp(dts[i, c], True) for c in cat_ids] for i in img_ids]
    imgs = C.EvaluateImages(p.areaRng, p.maxDets[-1], p.iouThrs, ious, gt_inst, dt_inst)
    ev = C.Accumulate(p, imgs)
    counts = list(ev["counts"])
    return {"precision": np.array(ev["precision"]).reshape(counts), "scores": np.array(ev["scores"]).reshape(counts),
            "recall": np.array(ev["recall"]).reshape(counts[:1] + counts[2:]), "counts": counts}


def hand():
    cats = [(1, "edge"), (3, "twin"), (4, "crowd"), (5, "area"), (7, "many"), (8, "tile"), (9, "nogt"), (11, "nodet")]
    ds = {"images": [], "categories": [{"id": c, "name": n} for c, n in cats], "annotations": []}
    res = []
    next_id = [1]

    def image(i):
        ds["images"].append({"id": i, "height": 480, "width": 640, "file_name": f"{i:012d}.jpg"})
        return i

    def ann(i, c, box, area=None, crowd=0, id=None):
        if id is None:
            id = next_id[0]
            next_id[0] += 1
        ds["annotations"].append({"id": id, "image_id": i, "category_id": c, "bbox": [float(v) for v in box],
                                  "area": float(box[2] * box[3] if area is None else area), "iscrowd": crowd})

    def det(i, c, s, box):
        res.append({"image_id": i, "category_id": c, "bbox": [float(v) for v in box], "score": s})

    # cat 1: IoU exactly 0.5 and 0.75 against 10 x 10 boxes, and just below; image ids are not in file order
    for k, i in enumerate((40, 12, 33)):
        image(i)
        ann(i, 1, [0, 0, 10, 10])
        ann(i, 1, [100, 100, 10, 10])
        det(i, 1, 0.9, [0, 0, 10, 5])                       # 50 / 100
        det(i, 1, 0.9, [100, 100, 10, 7.5])                 # 75 / 100
        det(i, 1, 0.8 - 0.1 * k, [0, 0, 10, 4.9])
        det(i, 1, 0.8, [100, 100, 10, 7.4])
    # cat 3: two ground truths at equal IoU (the later wins), the second detection takes the first
    i = image(50)
    ann(i, 3, [20, 20, 40, 40])
    ann(i, 3, [20, 20, 40, 40])
    det(i, 3, 0.7, [20, 20, 40, 36])
    det(i, 3, 0.6, [20, 20, 40, 38])
    det(i, 3, 0.6, [20, 20, 40, 39])
    # cat 4: a crowd box matched by several detections; the break rule: detection [300, 300, 20, 20] overlaps the plain object at
    # 0.64 and lies inside the crowd box (IoU 1 with it), but the walk stops at the first ignored ground truth
    i = image(51)
    ann(i, 4, [200, 200, 80, 80], crowd=1)
    ann(i, 4, [300, 300, 25, 25])
    ann(i, 4, [290, 290, 80, 80], crowd=1)
    for k in range(4):
        det(i, 4, 0.9 - 0.05 * k, [205 + 5 * k, 205, 30, 30])
    det(i, 4, 0.95, [300, 300, 20, 20])
    det(i, 4, 0.5, [300, 300, 25, 25])
    # cat 5: area against w * h on either side of 32^2; an object outside the range; an unmatched large detection; id 0;
    # zero-width boxes
    i = image(52)
    ann(i, 5, [10, 10, 40, 40], area=1000)                  # w * h = 1600, area small
    ann(i, 5, [100, 10, 30, 30], area=1100)                 # w * h = 900, area medium
    ann(i, 5, [200, 10, 20, 20])
    ann(i, 5, [300, 10, 50, 50], id=0)
    ann(i, 5, [400, 10, 0, 30])
    det(i, 5, 0.9, [10, 10, 40, 40])
    det(i, 5, 0.8, [100, 10, 30, 30])
    det(i, 5, 0.7, [200, 10, 20, 20])
    det(i, 5, 0.9, [300, 10, 50, 50])                       # takes the id-0 object: never a true positive
    det(i, 5, 0.6, [300, 10, 50, 49])                       # the id-0 object is taken
    det(i, 5, 0.5, [400, 10, 0, 30])
    det(i, 5, 0.4, [10, 200, 200, 200])                     # unmatched, large
    det(i, 5, 0.4, [10, 10, 0, 40])
    det(i, 5, 0.3, [500, 500, 10, 10], )
    res.append({"image_id": i, "category_id": 99, "bbox": [10.0, 10.0, 40.0, 40.0], "score": 0.99})   # unknown category
    # cat 7: 130 detections against 20 objects in one image; 70 objects in another
    rng = np.random.default_rng(7)
    i = image(60)
    for k in range(20):
        ann(i, 7, [10 + 30 * k, 10, 25, 25 + k % 3])
    for k in range(130):
        g = int(rng.integers(0, 20))
        det(i, 7, round(float(rng.integers(0, 50)) / 50, 3),
            [10 + 30 * g + int(rng.integers(-3, 4)), 10 + int(rng.integers(-3, 4)), 25, 25 + int(rng.integers(0, 4))])
    i = image(61)
    for k in range(70):
        ann(i, 7, [5 + 9 * k, 100 + 40 * (k % 2), 30, 30], crowd=int(k % 17 == 5))
    for k in range(25):
        g = int(rng.integers(0, 70))
        det(i, 7, round(float(rng.integers(0, 20)) / 20, 3), [5 + 9 * g + int(rng.integers(-2, 3)), 100 + 40 * (g % 2), 30, 30])
    # cat 8: 1,500 detections over 50 images, scores tied across images
    for n in range(50):
        i = image(100 + n)
        for k in range(3):
            ann(i, 8, [20 + 100 * k, 20, 60 + n % 7, 50])
        for k in range(30):
            g = int(rng.integers(0, 4))
            box = [20 + 100 * g + int(rng.integers(-8, 9)), 20 + int(rng.integers(-8, 9)), 60 + n % 7, 50] if g < 3 else \
                [int(rng.integers(0, 400)), 200, 40, 40]
            det(i, 8, round(float(rng.integers(0, 100)) / 100, 3), box)
    # cat 9: detections, no ground truth.  cat 11: ground truth, no detections.  image 70: no detections
    det(50, 9, 0.5, [10, 10, 30, 30])
    det(51, 9, 0.5, [10, 10, 30, 30])
    ann(50, 11, [10, 10, 30, 30])
    i = image(70)
    ann(i, 1, [0, 0, 10, 10])
    assert all(a["area"] <= 96 ** 2 for a in ds["annotations"] if not a["iscrowd"])      # nothing in the large range
    return ds, res


def main(ref_root, out_dir):
    with tempfile.TemporaryDirectory() as tmp:
        C = build_reference(ref_root, tmp)
        cases = {"hand": hand(), "random": F.random_split(np.random.default_rng(1), 200, 12, 40),
                 "coco": F.random_split(np.random.default_rng(2), 500, 80, 100, crowd_p=0.03, max_obj=8)}
        for case, (ds, res) in cases.items():
            ev = run_reference(C, ds, res)
            z = F.pack(ds, res, compact=case != "hand")
            assert F.dataset(z) == ds and F.results(z) == res, "the fixture does not round-trip"
            stats = F.summarize(ev)
            names = [c["name"] for c in sorted(ds["categories"], key=lambda c: c["id"])]
            z["stats"] = stats
            z["result_values"] = np.asarray(list(F.derive(ev, stats, names).values()), dtype=np.float64)
            z["recall"] = ev["recall"]
            if case == "coco":
                for k in ("precision", "scores"):
                    z[k + "_sha256"], z[k + "_crc"] = F.digest(ev[k])
            else:
                z["precision"], z["scores"] = ev["precision"], ev["scores"]
            path = os.path.join(out_dir, f"coco_eval_{case}.npz")
            np.savez_compressed(path, **z)
            print(path, os.path.getsize(path), "bytes,", len(res), "detections,", len(ds["annotations"]), "annotations; stats",
                  np.round(stats[:6], 4))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)

"""Generate tests/golden/voc_eval_{hand,random,noties,npos0}.npz by RUNNING the reference's VOC evaluation
(/root/reference/uwsod/detectron2/evaluation/pascal_voc_evaluation.py: parse_rec, voc_ap, voc_eval, voc_eval_corloc and
PascalVOCDetectionEvaluator.evaluate) on synthetic splits — build container only:

    python tests/golden/make_voc_eval_golden.py [OUT_DIR]          (default: tests/golden)

detectron2 is stubbed: fvcore's PathManager is the builtin open, MetadataCatalog returns the synthetic split's metadata, comm is
one rank, DatasetEvaluator is a plain base class.  In the loaded module's namespace np.argsort is replaced by a stable argsort
(the one deliberate deviation: ties in line order); the "noties" case is also run with the module unpatched and must agree.
Each case's devkit tree is written by tests/voc_eval_fixture.write_devkit; per class the detection file holds the lines the
evaluator writes ("\\n".join(lines)).  Stored: the inputs as compact arrays, per class and threshold the reference's AP of both
metrics and its CorLoc times 100, and evaluate()'s dict with year 2007 and 2012.

Cases
  hand    hand-made: score ties, several detections on one object, matches to difficult objects, images whose objects of the
          class are all difficult (with later detections), IoU exactly 0.5 and 0.75, recall exactly 0.3 / 0.6 / 0.7 (npos 10),
          a class without detections, a class whose only objects are difficult and which has no detections, zero-area / inverted /
          NaN / inf boxes, zero-area objects, objects of an unlisted class, a repeated image-set line, a class of 200 true
          positives (> 128 recall change points) among 1,700 detections (> one 1,024-detection tile).
  random  300 images, 20 classes, 1-6 objects per image (12 % difficult), up to 100 detections per image, scores at 3 decimals.
  noties  like random, with every score of a class distinct; also checked against the unpatched reference.
  npos0   AP only (voc_eval; voc_eval_corloc divides by zero there): a class with detections whose objects are all difficult,
          a class with detections and no objects, and an ordinary class."""
import importlib.util
import json
import os
import sys
import tempfile
import types
from collections import defaultdict

import numpy as np

REF = "/root/reference/uwsod/detectron2/evaluation/pascal_voc_evaluation.py"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import voc_eval_fixture as F  # noqa: E402

META = {}


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install():
    _mod("fvcore")
    _mod("fvcore.common")
    _mod("fvcore.common.file_io", PathManager=types.SimpleNamespace(open=open))
    _mod("detectron2")
    _mod("detectron2.data", MetadataCatalog=types.SimpleNamespace(get=lambda name: META[name]))
    _mod("detectron2.utils")
    comm = _mod("detectron2.utils.comm", gather=lambda x, dst=0: [x], is_main_process=lambda: True)
    sys.modules["detectron2.utils"].comm = comm
    _mod("detectron2.evaluation")
    _mod("detectron2.evaluation.evaluator", DatasetEvaluator=type("DatasetEvaluator", (), {}))
    spec = importlib.util.spec_from_file_location("detectron2.evaluation.pascal_voc_evaluation", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _StableNp(types.ModuleType):
    """numpy, except argsort is stable"""

    def __getattr__(self, k):
        return getattr(np, k)

    @staticmethod
    def argsort(a, *args, **kw):
        kw.pop("kind", None)
        return np.argsort(a, *args, kind="stable", **kw)


def put(z, cls, img, score, box, names, objs):
    """objs: per distinct image, in names' first-appearance order: list of (class or -1, box, difficult, truncated, pose)"""
    z["names"] = np.asarray(names, dtype=np.int32)
    z["obj_off"] = np.cumsum([0] + [len(o) for o in objs]).astype(np.int32)
    flat = [o for os_ in objs for o in os_]
    z["obj_cls"] = np.asarray([o[0] for o in flat], dtype=np.int16)
    z["obj_box"] = np.asarray([o[1] for o in flat], dtype=np.int32).reshape(-1, 4)
    z["obj_diff"] = np.asarray([o[2] for o in flat], dtype=np.uint8)
    z["obj_trunc"] = np.asarray([o[3] for o in flat], dtype=np.uint8)
    z["obj_pose"] = np.asarray([o[4] for o in flat], dtype=np.uint8)
    z["det_cls"] = np.asarray(cls, dtype=np.int16)
    z["det_img"] = np.asarray(img, dtype=np.int16)
    return z


def compact(z, score, box):
    z["det_score_milli"] = np.asarray([round(s * 1000) for s in score], dtype=np.int16)
    z["det_box_deci"] = np.asarray([round(v * 10) for v in np.asarray(box).reshape(-1)], dtype=np.int32).reshape(-1, 4)
    return z


# ---- cases ------------------------------------------------------------------------------------------------------------------

def hand():
    names, objs = [], []
    cls, img, score, box = [], [], [], []

    def image(o):
        names.append(len(names) + 1)
        objs.append([(c, b, d, 0, 0) for c, b, d in o])
        return len(names) - 1

    def det(c, i, s, b):
        cls.append(c)
        img.append(i)
        score.append(s)
        box.append([float(v) for v in b])

    sq = [10, 10, 109, 109]                      # 100 x 100 with the +1 terms
    # class 0: ties and several detections on one object
    for k in range(6):
        i = image([(0, sq, 0), (F.CLASS_NAMES.index("person"), [5, 5, 50, 60], 0)])
        det(0, i, 0.9, [11.0, 11.0, 109.0, 109.0])
        det(0, i, 0.9, [10.0, 10.0, 100.0, 100.0])
        det(0, i, 0.9 if k % 2 else 0.8, [20.0, 20.0, 109.0, 109.0])
        det(0, i, 0.5, [300.0, 300.0, 350.0, 350.0])
        det(14, i, 0.7, [5.0, 5.0, 50.0, 60.0])
    # class 1: difficult matches; images whose class-1 objects are all difficult, with later detections
    for k in range(5):
        i = image([(1, sq, 1), (1, [200, 200, 299, 299], 0 if k < 3 else 1), (-1, [1, 1, 30, 30], 0)])
        det(1, i, 0.95, [11.0, 11.0, 109.0, 109.0])             # difficult: neither TP nor FP
        det(1, i, 0.6, [201.0, 201.0, 299.0, 299.0])
        det(1, i, 0.6, [201.0, 201.0, 290.0, 299.0])
        det(1, i, 0.3, [1.0, 1.0, 30.0, 30.0])
    # class 2: IoU exactly 0.5 and 0.75 against [1, 1, 10, 10] (area 100)
    for k in range(4):
        i = image([(2, [1, 1, 10, 10], 0), (2, [101, 101, 110, 110], 0)])
        det(2, i, 0.8, [1.0, 1.0, 10.0, 5.0])                    # 50 / 100
        det(2, i, 0.8, [101.0, 101.0, 110.0, 107.5])             # 75 / 100
        det(2, i, 0.7, [1.0, 1.0, 10.0, 5.1])
        det(2, i, 0.7, [101.0, 101.0, 110.0, 107.6])
    # class 3: npos 10, true positives reaching recall 3/10, 6/10, 7/10 between false positives
    ims = [image([(3, [20 + k, 20, 80 + k, 90], 0)]) for k in range(10)]
    s = 0.99
    for k, i in enumerate(ims):
        if k in (3, 6, 7):
            det(3, ims[0], round(s, 3), [400.0, 400.0, 450.0, 450.0])
            s -= 0.01
        det(3, i, round(s, 3), [20.0 + k, 20.0, 80.0 + k, 90.0])
        s -= 0.01
    # class 4: objects, no detections.  class 8: difficult objects only, no detections
    image([(4, [30, 30, 60, 60], 0), (8, [1, 1, 40, 40], 1)])
    # class 5: degenerate and non-finite boxes; zero-area objects
    i = image([(5, [50, 50, 49, 80], 0), (5, [10, 10, 60, 60], 0), (5, [100, 100, 100, 100], 0)])
    det(5, i, 0.9, [10.0, 10.0, 9.0, 60.0])                      # zero width
    det(5, i, 0.9, [60.0, 60.0, 10.0, 10.0])                     # inverted
    det(5, i, 0.8, [float("nan"), 10.0, 60.0, 60.0])
    det(5, i, 0.8, [10.0, 10.0, float("inf"), 60.0])
    det(5, i, 0.7, [50.0, 50.0, 49.0, 80.0])                     # the zero-area object itself: 0 / 0
    det(5, i, 0.6, [10.0, 10.0, 60.0, 60.0])
    det(5, i, 0.5, [100.0, 100.0, 100.0, 100.0])
    det(5, i, float("nan"), [10.0, 10.0, 60.0, 60.0])
    # class 6: 200 true positives among 1,700 detections
    rng = np.random.default_rng(5)
    big = [image([(6, [10, 10, 100 + k % 50, 120], 0)]) for k in range(200)]
    for k, i in enumerate(big):
        det(6, i, round(0.999 - 0.004 * (k // 2), 3), [10.0, 10.0, 100.0 + k % 50, 120.0])
    for k in range(1500):
        i = big[int(rng.integers(0, 200))]
        det(6, i, round(float(rng.integers(0, 1000)) / 1000, 3), [200.0, 200.0, 260.0 + k % 7, 270.0])
    # a repeated image-set line
    names.append(names[ims[2]])
    z = put({}, cls, img, score, box, names, objs)
    z["det_score"] = np.asarray(score, dtype=np.float64)
    z["det_box"] = np.asarray(box, dtype=np.float64).reshape(-1, 4)
    return z


def random_case(seed, n_img=300, distinct=False, max_det=100):
    rng = np.random.default_rng(seed)
    names = sorted(rng.choice(np.arange(1, 10000), n_img, replace=False).tolist())
    objs = []
    cls, img, score, box = [], [], [], []
    used = defaultdict(set)
    for i in range(n_img):
        o = []
        for _ in range(int(rng.integers(1, 7))):
            x1, y1 = int(rng.integers(1, 400)), int(rng.integers(1, 300))
            o.append((int(rng.integers(0, 20)), [x1, y1, x1 + int(rng.integers(5, 100)), y1 + int(rng.integers(5, 75))],
                      int(rng.random() < 0.12), int(rng.random() < 0.3), int(rng.integers(0, len(F.POSES)))))
        objs.append(o)
        for _ in range(int(rng.integers(0, max_det + 1))):
            if rng.random() < 0.6:
                g = o[int(rng.integers(0, len(o)))]
                c = g[0]
                b = [g[1][q] + float(rng.integers(-80, 81)) / 10 for q in range(4)]
            else:
                c = int(rng.integers(0, 20))
                x1, y1 = float(rng.integers(0, 4000)) / 10, float(rng.integers(0, 3000)) / 10
                b = [x1, y1, x1 + float(rng.integers(20, 1500)) / 10, y1 + float(rng.integers(20, 1000)) / 10]
            if distinct:
                free = [v for v in range(1000) if v not in used[c]]
                if not free:
                    continue
                v = free[int(rng.integers(0, len(free)))]
                used[c].add(v)
            else:
                v = int(rng.integers(0, 1000))
            cls.append(c)
            img.append(i)
            score.append(v / 1000)
            box.append([round(q * 10) / 10 for q in b])
    z = put({}, cls, img, score, box, names, objs)
    return compact(z, score, box)


def npos0():
    names, objs = [1, 2, 3, 4], []
    objs.append([(0, [10, 10, 50, 50], 1), (2, [10, 10, 50, 50], 0)])
    objs.append([(0, [60, 60, 90, 90], 1)])
    objs.append([(2, [5, 5, 40, 40], 0)])
    objs.append([])
    objs = [[(c, b, d, 0, 0) for c, b, d in o] for o in objs]
    cls = [0, 0, 0, 1, 1, 2, 2, 2]
    img = [0, 1, 3, 2, 3, 0, 2, 3]
    score = [0.9, 0.8, 0.8, 0.5, 0.4, 0.9, 0.9, 0.1]
    box = [[10.0, 10.0, 50.0, 50.0], [60.0, 60.0, 90.0, 90.0], [1.0, 1.0, 5.0, 5.0], [5.0, 5.0, 40.0, 40.0],
           [1.0, 1.0, 2.0, 2.0], [10.0, 10.0, 50.0, 50.0], [5.0, 5.0, 40.0, 40.0], [5.0, 5.0, 40.0, 40.0]]
    z = put({}, cls, img, score, box, names, objs)
    z["det_score"] = np.asarray(score, dtype=np.float64)
    z["det_box"] = np.asarray(box, dtype=np.float64).reshape(-1, 4)
    return z


# ---- running the reference --------------------------------------------------------------------------------------------------

def run_reference(pve, z, corloc=True, with_dicts=True):
    K = len(F.CLASS_NAMES)
    lines = F.lines(z)
    out = {"ap_07": np.full((K, 10), np.nan), "ap_area": np.full((K, 10), np.nan), "corloc": np.full((K, 10), np.nan)}
    with tempfile.TemporaryDirectory() as tmp:
        root = F.write_devkit(z, os.path.join(tmp, "VOC2007"))
        pve.parse_rec.cache_clear()
        anno = os.path.join(root, "Annotations", "{}.xml")
        imageset = os.path.join(root, "ImageSets", "Main", F.SPLIT + ".txt")
        det_tpl = os.path.join(tmp, "det_{}.txt")
        for k, name in enumerate(F.CLASS_NAMES):
            with open(det_tpl.format(name), "w") as f:
                f.write("\n".join(lines[k] or [""]))
            for t, th in enumerate(range(50, 100, 5)):
                for metric, use07 in (("ap_07", True), ("ap_area", False)):
                    with np.errstate(all="ignore"):
                        _, _, ap = pve.voc_eval(det_tpl, anno, imageset, name, ovthresh=th / 100.0, use_07_metric=use07)
                    out[metric][k, t] = ap * 100
                if corloc:
                    out["corloc"][k, t] = pve.voc_eval_corloc(det_tpl, anno, imageset, name, ovthresh=th / 100.0) * 100
        parsed = {n: pve.parse_rec(anno.format(n)) for n in F.names(z)}
        assert parsed == F.recs(z), "the devkit tree does not round-trip through parse_rec"
        out["parse_rec_json"] = np.asarray(json.dumps(parsed))
        if with_dicts:
            os.makedirs(os.path.join(tmp, "results", "VOC2007", "Main"), exist_ok=True)      # so evaluate() need not mkdir
            for year in (2007, 2012):
                META["voc_eval_fixture"] = types.SimpleNamespace(dirname=root, split=F.SPLIT, thing_classes=list(F.CLASS_NAMES),
                                                                 year=year)
                ev = pve.PascalVOCDetectionEvaluator("voc_eval_fixture")
                ev._predictions = defaultdict(list, {k: list(v) for k, v in lines.items() if v})
                r = ev.evaluate()
                out[f"dict_{year}"] = np.array([r[a][b] for a, b in F.DICT_KEYS], dtype=np.float64)
    return out


def main(out_dir):
    pve = install()
    stable = _StableNp("numpy_stable_argsort")
    plain_np = pve.np
    cases = {"hand": (hand(), True), "random": (random_case(1), True), "noties": (random_case(2, n_img=120, distinct=True), True),
             "npos0": (npos0(), False)}
    for case, (z, full) in cases.items():
        pve.np = stable
        res = run_reference(pve, z, corloc=full, with_dicts=full)
        if case == "noties":
            pve.np = plain_np
            unpatched = run_reference(pve, z)
            for k in ("ap_07", "ap_area", "corloc", "dict_2007", "dict_2012"):
                assert np.array_equal(res[k], unpatched[k], equal_nan=True), k
        pve.np = plain_np
        z.update(res)
        path = os.path.join(out_dir, f"voc_eval_{case}.npz")
        np.savez_compressed(path, **z)
        print(path, os.path.getsize(path), "bytes,", len(z["det_cls"]), "detections")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)

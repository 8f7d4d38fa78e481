"""Generate tests/golden/proposal_{hand,handcoco,random,eb,ss}.npz by RUNNING the reference's proposal tools
(/root/reference/uwsod/projects/WSL/tools/proposal_recall.py and proposal_convert.py, loaded by path) on synthetic splits — build
container only:

    python tests/golden/make_proposal_golden.py [OUT_DIR]          (default: tests/golden)

`detectron2.data.catalog.DatasetCatalog.get` is stubbed to return the synthetic records; cv2, tqdm, six and wsl.data.datasets
(imported by the converter, not used by what runs here) are empty stubs.  Per budget the module's `max_num_box` and `sys.argv`
are set as its `__main__` loop sets them and the function's stdout is captured: the per-box `print(ovmax, jmax)` lines are the
only ones made of one float and one integer.  The `.mat` files are written with scipy.io.savemat from the arrays the fixture keeps
(tests/proposal_fixture.py writes the same files for the tests).

Cases (every compared image has distinct scores: the reference's argsort is not stable)
  hand      voc_2007_test, uint16 boxes, one .mat per image.  Images of 1, 3, 4, 5 and 2500 proposals (fewer than the smallest
            budget, equal to it, one more, more than the kernel stages in LDS at once, more than the largest budget); an image without
            annotations between two that have some; an image of 70 ground-truth boxes and 70 proposals; duplicated proposals
            (argmax takes the first); a proposal equal to a ground-truth box (IoU exactly 1.0 counts at threshold 1.0); file
            coordinates of 0, which `- 1` wraps to 65535 in uint16: as xmin (the box's width then wraps too) and as xmax.
  handcoco  coco_2014_val-style name (files named by file_name, XYWH ground truth), float64 boxes; a proposal of negative width
            whose area cancels the ground truth's, so that uni == 0 and the overlap is NaN from its rank on.
  random    48 images, float64 boxes with fractional coordinates, 0-4 objects, 1-400 proposals.
  eb        the EdgeBoxes layout: one file with `boxes` and `boxScores` cells.
  ss        the Selective Search layout: one file with `boxes` cells, no scores; `np.random.seed(seed)` before the budget loop."""
import contextlib
import importlib.util
import io
import os
import pickle
import re
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference/uwsod/projects/WSL/tools"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import proposal_fixture as F  # noqa: E402

DATASETS = {}


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def install():
    _mod("detectron2")
    _mod("detectron2.data")
    _mod("detectron2.data.catalog", DatasetCatalog=types.SimpleNamespace(get=lambda name: DATASETS[name]))
    _mod("cv2")
    _mod("tqdm", tqdm=lambda it, *a, **k: it)
    _mod("six")
    _mod("six.moves", cPickle=pickle)
    _mod("wsl")
    _mod("wsl.data")
    _mod("wsl.data.datasets")
    return _load("ref_proposal_recall", f"{REF}/proposal_recall.py"), _load("ref_proposal_convert", f"{REF}/proposal_convert.py")


PAIR_RE = re.compile(r"^(-?(?:\d+\.\d*(?:e[-+]?\d+)?|\d+e[-+]?\d+|nan|inf)) (\d+)$")


def run_recall(rec, z, path, seed=None):
    """the module's __main__ loop for one case -> recall [10, 11], ovmax [10, G], jmax [10, G]"""
    mode = str(z["mode"])
    fn = {"mcg": rec.recall_mcg, "ss": rec.recall_ss, "eb": rec.recall_eb}[mode]
    rows, ov, jm = [], [], []
    if seed is not None:
        np.random.seed(seed)
    for num in F.BUDGETS:
        rec.max_num_box = num
        sys.argv = ["proposal_recall.py", F.name_of(z), path, mode]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
            rows.append(fn())
        pairs = [m.groups() for m in map(PAIR_RE.match, buf.getvalue().splitlines()) if m]
        assert len(pairs) == int(z["gt_off"][-1]), (len(pairs), int(z["gt_off"][-1]))
        ov.append([float(a) for a, _ in pairs])
        jm.append([int(b) for _, b in pairs])
    return np.array(rows, dtype=np.float64), np.array(ov, dtype=np.float64), np.array(jm, dtype=np.int64)


def run_convert(conv, z, path, tmp):
    mode = str(z["mode"])
    out = os.path.join(tmp, "out.pkl")
    sys.argv = ["proposal_convert.py", F.name_of(z), path, out]
    with contextlib.redirect_stdout(io.StringIO()):
        (conv.convert_ss_box if mode == "ss" else conv.convert_mcg_box)()
    with open(out, "rb") as f:
        p = pickle.load(f)
    assert all(b.dtype == np.int16 for b in p["boxes"]) and all(s.dtype == np.float32 for s in p["scores"])
    return {"conv_box": np.concatenate(p["boxes"]).reshape(-1, 4), "conv_score": np.concatenate([s.reshape(-1) for s in p["scores"]]),
            "conv_id": np.array(p["indexes"])}


# ---------------------------------------------------------------------------------------------------------------------- inputs
def to_file(xyxy):
    """0-based xyxy rows -> the file's 1-based (y1, x1, y2, x2)"""
    a = np.asarray(xyxy)
    return a[:, (1, 0, 3, 2)] + 1


def near(rng, gt, n, spread):
    """n integer xyxy boxes scattered around the ground-truth box gt"""
    b = np.asarray(gt, dtype=np.int64)[None, :] + rng.integers(-spread, spread + 1, (n, 4))
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
    return np.maximum(b, 1)


def anywhere(rng, n, size=400):
    xy = rng.integers(1, size, (n, 2))
    return np.concatenate([xy, xy + rng.integers(2, size // 2, (n, 2))], 1)


def scores_for(rng, n):
    return rng.permutation(n).astype(np.float64) / max(n, 1) + 0.001          # distinct


def pack(name, mode, ids, files, gts, props, scores, dtype, seed=None):
    z = {"dataset_name": np.array(name), "mode": np.array(mode), "image_id": np.array(ids), "file_name": np.array(files),
         "gt_off": np.cumsum([0] + [len(g) for g in gts]).astype(np.int64),
         "gt_box": np.array([b for g in gts for b in g], dtype=np.float64).reshape(-1, 4),
         "prop_off": np.cumsum([0] + [len(p) for p in props]).astype(np.int64),
         "prop_box": np.concatenate(props).astype(dtype)}
    if scores is not None:
        z["prop_score"] = np.concatenate(scores).astype(np.float64)
    if seed is not None:
        z["seed"] = np.array(seed)
    return z


def hand_inputs():
    rng = np.random.default_rng(11)
    gts, props = [], []

    def add(gt, p):
        gts.append([[float(v) for v in g] for g in gt])
        props.append(to_file(p))

    g = [30, 40, 130, 160]
    add([g], near(rng, g, 1, 12))                                      # 1 proposal: fewer than the smallest budget
    add([g, [200, 50, 260, 120]], near(rng, g, 3, 25))                 # 3
    add([g], near(rng, g, 4, 25))                                      # 4: equal to the smallest budget
    add([g, [5, 5, 60, 70]], near(rng, g, 5, 25))                      # 5: one more
    big = [[60, 80, 200, 260], [300, 120, 380, 300], [10, 10, 50, 40], [150, 150, 400, 330]]
    add(big, np.concatenate([anywhere(rng, 2300)] + [near(rng, b, 50, 30) for b in big]))          # 2500
    add([], anywhere(rng, 9))                                          # no annotations, between two images that have some
    many = [list(b) for b in anywhere(rng, 70, 300)]
    add(many, np.concatenate([near(rng, b, 1, 10) for b in many]))     # 70 ground-truth boxes, 70 proposals
    dup = near(rng, g, 6, 20)
    add([g, [100, 100, 180, 190]], np.concatenate([dup, dup, [[100, 100, 180, 190]], near(rng, g, 7, 40)]))   # duplicates; IoU 1.0
    wrap = near(rng, g, 12, 30)
    p = to_file(wrap)
    p[2, 1] = 0                                                        # file x1 = 0: xmin wraps to 65535, and the width with it
    p[5, 3] = 0                                                        # file x2 = 0: xmax wraps to 65535, a very wide box
    p[7, 0] = 0                                                        # file y1 = 0
    gts.append([[float(v) for v in g], [300.0, 300.0, 350.0, 360.0]])
    props.append(p)
    scores = [scores_for(rng, len(p)) for p in props]
    scores[4] = np.sort(scores[4])                                     # the 200 boxes near the objects rank first, shuffled
    scores[4][-200:] = scores[4][-200:][rng.permutation(200)]
    scores[7][:6] = 0.9 + np.arange(6) / 100                           # the first copies of the duplicates lead the ranking,
    scores[7][6:12] = 0.8 + np.arange(6) / 100                         # the second copies follow: equal overlaps, distinct scores
    ids = [f"{i + 1:06d}" for i in range(len(props))]
    files = [f"JPEGImages/{i}.jpg" for i in ids]
    return pack("voc_2007_test", "mcg", ids, files, gts, props, scores, np.uint16)


def handcoco_inputs():
    rng = np.random.default_rng(12)
    gts, props = [], []
    # uni == 0: ground truth XYWH (10, 10, 9, 9) = xyxy (10, 10, 19, 19), area 100; the proposal (50, 10, 39, 19) has width -10 and
    # height 10: area -100, no intersection
    p = near(rng, [10, 10, 19, 19], 20, 6).astype(np.float64)
    p[5] = [50.0, 10.0, 39.0, 19.0]
    gts.append([[10.0, 10.0, 9.0, 9.0]])
    props.append(to_file(p))
    for _ in range(5):
        g = anywhere(rng, int(rng.integers(1, 4)), 300)
        gts.append([[float(b[0]), float(b[1]), float(b[2] - b[0]) + 0.5, float(b[3] - b[1]) + 0.25] for b in g])
        props.append(to_file(np.concatenate([near(rng, b, 15, 25) for b in g] + [anywhere(rng, 20)]).astype(np.float64)
                             + rng.integers(0, 4, (15 * len(g) + 20, 1)) / 4))
    scores = [scores_for(rng, len(p)) for p in props]
    scores[0] = 1.0 - np.arange(20) / 100                              # file order is rank order: the NaN sits at rank 5
    ids = [int(v) for v in rng.choice(np.arange(1, 600000), len(props), replace=False)]
    files = [f"val2014/COCO_val2014_{i:012d}.jpg" for i in ids]
    return pack("coco_2014_val", "mcg", ids, files, gts, props, scores, np.float64)


def random_inputs(name, mode, n_img, seed, max_props, integer=False):
    rng = np.random.default_rng(seed)
    gts, props = [], []
    for k in range(n_img):
        g = anywhere(rng, int(rng.integers(0, 5)) if k else 2, 350)
        n = int(rng.integers(1, max_props + 1))
        parts = [near(rng, b, max(n // (2 * len(g)), 1), int(rng.integers(5, 60))) for b in g] + [anywhere(rng, n)]
        p = np.concatenate(parts)[rng.permutation(sum(len(q) for q in parts))][:n].astype(np.float64)
        if not integer:
            p = p + rng.integers(0, 8, p.shape) / 8
            p[:, 2:] = np.maximum(p[:, 2:], p[:, :2])
        gts.append([[float(v) for v in b] for b in g])
        props.append(to_file(p))
    scores = None if mode == "ss" else [scores_for(rng, len(p)) for p in props]
    ids = [f"{i + 1:06d}" for i in range(n_img)]
    files = [f"JPEGImages/{i}.jpg" for i in ids]
    return pack(name, mode, ids, files, gts, props, scores, np.float64, seed=seed if mode == "ss" else None)


def main(out_dir=HERE):
    rec, conv = install()
    cases = {"hand": hand_inputs(), "handcoco": handcoco_inputs(), "random": random_inputs("voc_2007_trainval", "mcg", 48, 21, 400),
             "eb": random_inputs("voc_2007_val", "eb", 20, 22, 300, integer=True),
             "ss": random_inputs("voc_2012_val", "ss", 24, 23, 300, integer=True)}
    for case, z in cases.items():
        DATASETS[F.name_of(z)] = F.records(z)
        with tempfile.TemporaryDirectory() as tmp:
            path = F.write_mats(z, os.path.join(tmp, "mat"))
            z["recall"], z["ovmax"], z["jmax"] = run_recall(rec, z, path, seed=int(z["seed"]) if "seed" in z else None)
            if str(z["mode"]) != "eb":                                  # the reference converts MCG and Selective Search files only
                z.update(run_convert(conv, z, path, tmp))
        r = z["recall"]
        assert ((r > 0) & (r < 1)).any() and (r.max(0) != r.min(0)).any(), case          # a wrong cut must show
        if "prop_score" in z:
            for s in F.per_image(z, "prop_score"):
                assert len(np.unique(s)) == len(s), case
        np.savez_compressed(os.path.join(out_dir, f"proposal_{case}.npz"), **z)
        print(case, "G", int(z["gt_off"][-1]), "P", int(z["prop_off"][-1]), "recall@0.5", r[:, 0].round(3).tolist(),
              "nan", int(np.isnan(z["ovmax"]).sum()), os.path.getsize(os.path.join(out_dir, f"proposal_{case}.npz")))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)

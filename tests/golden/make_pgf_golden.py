"""Generate tests/golden/pgf_voc.npz and pgf_coco.npz by RUNNING the reference's Stage-2 tools (/root/reference/tools/pgf.py,
add_multi_label.py) and its Stage-3 pseudo-label loader (/root/reference/detectron2/detectron2/data/datasets/pascal_voc.py,
load_voc_instances_wsl) on synthetic splits — build container only:

    python tests/golden/make_pgf_golden.py [OUT_DIR]          (default: tests/golden)

detectron2 is stubbed: `get_detection_dataset_dicts` returns the synthetic ground-truth dicts below, BoxMode.XYXY_ABS is 0,
PathManager is the builtin open; tqdm is the identity.  Each reference function runs in a temporary directory laid out as it
expects; its stdout is captured for the four counts per split.  A fixture holds the inputs as arrays (tests/pgf_fixture.py turns
them back into the records the reference read) and, per case and split, the SHA-256 of each file the reference wrote and its counts.

Cases
  voc_a   VOC 2007, t_con 0.85, t_keep 0.2, use_diff off.  train: hand-made images — several classes per image, classes absent
          from the ground truth, an image id absent from it, an image that ends empty, a low-score first-of-class detection,
          duplicate / zero-area / nested boxes, difficult classes, pairs whose contain ratio lies within 1e-9 of t_con on either
          side where f32 arithmetic decides the other way, one image of 300 detections (more than the kernel's LDS stage);
          val: random images.  Also add_voc07 and load_voc_instances_wsl on the outputs, and on the
          unfiltered pseudo-label file (pgf_fixture.voc_unfiltered_pgt), which the CPU tests rebuild without a GPU.
  voc_b   the same detections, use_diff on, t_con 0.7, t_keep 0.3.
  coco_a  COCO, use_diff on: 80 classes through id2cat, a repeated image id, an image absent from the ground truth, one image of
          300 instances."""
import contextlib
import importlib.util
import io
import json
import os
import random
import re
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pgf_fixture as F  # noqa: E402

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
    get = lambda names: json.loads(json.dumps(DATASETS[names[0]]))      # noqa: E731  a fresh copy per call
    _mod("detectron2")
    _mod("detectron2.data", get_detection_dataset_dicts=get, build_detection_test_loader=None, DatasetCatalog=None,
         MetadataCatalog=None)
    _mod("detectron2.config", get_cfg=None)
    _mod("detectron2.structures", BoxMode=types.SimpleNamespace(XYXY_ABS=0))
    _mod("detectron2.utils")
    _mod("detectron2.utils.file_io", PathManager=types.SimpleNamespace(open=open, get_local_path=lambda p: p))
    _mod("tqdm", tqdm=lambda it, *a, **k: it)
    np.str = str                                   # removed from numpy; pascal_voc.py's np.loadtxt(dtype=np.str) needs it
    pgf = _load("ref_pgf", f"{REF}/tools/pgf.py")
    aml = _load("ref_add_multi_label", f"{REF}/tools/add_multi_label.py")
    voc = _load("ref_pascal_voc", f"{REF}/detectron2/detectron2/data/datasets/pascal_voc.py")
    return pgf, aml, voc


COUNT_RE = re.compile(r"^(train|val) split length (before multi-class filter|after multi-class filter|in middle of pgf|after pgf): (\d+)$")
COUNT_ORDER = ("before multi-class filter", "after multi-class filter", "in middle of pgf", "after pgf")


def counts_of(stdout):
    got = {"train": {}, "val": {}}
    for line in stdout.splitlines():
        m = COUNT_RE.match(line)
        if m:
            got[m.group(1)][m.group(2)] = int(m.group(3))
    return {s: [got[s][k] for k in COUNT_ORDER] for s in got}


# ---------------------------------------------------------------------------------------------------------------------- inputs
def r1(v):
    return float(f"{v:.1f}")                      # the writer's %.1f


def rand_box(rng, grid=False):
    x1, y1 = rng.uniform(0, 400), rng.uniform(0, 300)
    x2, y2 = x1 + rng.uniform(1, 200), y1 + rng.uniform(1, 200)
    if grid:
        return [float(round(x1 / 8) * 8 + 1), float(round(y1 / 8) * 8 + 1), float(round(x2 / 8) * 8), float(round(y2 / 8) * 8)]
    return [r1(x1 + 1), r1(y1 + 1), r1(x2), r1(y2)]


def contain64(a, b):
    a, b = list(a), list(b)
    a[2] += a[0]; a[3] += a[1]; b[2] += b[0]; b[3] += b[1]
    c = [max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])]
    return max(0, c[2] - c[0]) * max(0, c[3] - c[1]) / (max(0, a[2] - a[0]) * max(0, a[3] - a[1]) + 1e-6)


def contain32(a, b):
    f = np.float32
    a, b = [f(v) for v in a], [f(v) for v in b]
    a[2] += a[0]; a[3] += a[1]; b[2] += b[0]; b[3] += b[1]
    c = [max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])]
    z = f(0)
    return f(max(z, c[2] - c[0]) * max(z, c[3] - c[1])) / f(max(z, a[2] - a[0]) * max(z, a[3] - a[1]) + f(1e-6))


def near_threshold_pair(rng, t_con, above):
    """(a, b): contain_cal(a, b) within 1e-9 of t_con — at or above it when `above` — and f32 arithmetic on the other side"""
    for _ in range(200000):
        a = [r1(rng.uniform(0, 200)), r1(rng.uniform(0, 200)), r1(rng.uniform(20, 200)), r1(rng.uniform(20, 200))]
        wb = t_con * (a[2] * a[3] + 1e-6) / a[3]
        wb = float(np.nextafter(wb, np.inf if above else -np.inf)) if rng.random() < 0.5 else wb
        b = [a[0], a[1] - 1000.0, wb, a[3] + 2000.0]
        r = contain64(a, b)
        if (0 <= r - t_con <= 1e-9) if above else (0 < t_con - r <= 1e-9):
            if (contain32(a, b) >= np.float32(t_con)) != above:
                return a, b
    raise RuntimeError("no near-threshold pair found")


def voc_rec(img, c, score, box):
    return {"image_id": img, "category_id": c + 1, "score": score, "bbox": box}


def voc_gt(img, classes):
    return {"image_id": img, "annotations": [{"category_id": c} for c in classes]}


def voc_inputs():
    rng = random.Random(2024)
    recs, gt = [], []
    # 1: several classes; class 5 absent from the ground truth; low-score first of class 0; duplicates and nesting
    gt.append(voc_gt(1, [0, 2, 0]))
    recs += [voc_rec(1, 0, 0.05, [11.0, 21.0, 60.0, 80.0]), voc_rec(1, 0, 0.1, [200.0, 200.0, 50.0, 40.0]),
             voc_rec(1, 0, 0.9, [100.0, 100.0, 200.0, 150.0]), voc_rec(1, 0, 0.8, [120.0, 110.0, 50.0, 30.0]),
             voc_rec(1, 2, 0.7, [30.0, 40.0, 90.0, 95.0]), voc_rec(1, 2, 0.6, [30.0, 40.0, 90.0, 95.0]),
             voc_rec(1, 5, 0.95, [1.0, 1.0, 300.0, 300.0])]
    # 2: not in the ground truth: skipped
    recs += [voc_rec(2, 0, 0.9, [1.0, 1.0, 50.0, 50.0])]
    # 3: nothing survives the class filter
    gt.append(voc_gt(3, [7]))
    recs += [voc_rec(3, 3, 0.9, [5.0, 5.0, 60.0, 60.0]), voc_rec(3, 11, 0.8, [7.0, 7.0, 30.0, 30.0])]
    # 4: difficult classes 4 and 8 with nested boxes; class 1 nested too
    gt.append(voc_gt(4, [4, 8, 1]))
    recs += [voc_rec(4, 4, 0.9, [10.0, 10.0, 300.0, 300.0]), voc_rec(4, 4, 0.5, [20.0, 20.0, 40.0, 40.0]),
             voc_rec(4, 8, 0.3, [50.0, 50.0, 100.0, 100.0]), voc_rec(4, 8, 0.25, [50.0, 50.0, 100.0, 100.0]),
             voc_rec(4, 1, 0.6, [0.0, 0.0, 400.0, 400.0]), voc_rec(4, 1, 0.65, [10.0, 10.0, 20.0, 20.0])]
    # 5: zero-area and negative-extent boxes
    gt.append(voc_gt(5, [6, 12]))
    recs += [voc_rec(5, 12, 0.9, [10.0, 10.0, 0.0, 50.0]), voc_rec(5, 12, 0.8, [10.0, 10.0, 0.0, 50.0]),
             voc_rec(5, 12, 0.7, [5.0, 5.0, 100.0, 0.0]), voc_rec(5, 12, 0.6, [0.0, 0.0, 200.0, 200.0]),
             voc_rec(5, 6, 0.5, [30.0, 30.0, -5.0, 20.0]), voc_rec(5, 6, 0.45, [20.0, 20.0, 40.0, 40.0])]
    # 6: pairs within 1e-9 of t_con = 0.85, each side, one class per pair
    gt.append(voc_gt(6, [10, 13, 17, 19]))
    for k, c in enumerate((10, 13, 17, 19)):
        a, b = near_threshold_pair(rng, 0.85, above=bool(k % 2))
        recs += [voc_rec(6, c, 0.9, b), voc_rec(6, c, 0.8, a)]
    # 7: random boxes of several classes, some low scores
    gt.append(voc_gt(7, [3, 9, 14]))
    for _ in range(25):
        recs.append(voc_rec(7, rng.choice([3, 9, 14, 18]), round(rng.random(), 3), rand_box(rng)))
    # 8: more detections than the kernel's LDS stage (256), on a coarse grid: many duplicates and nested boxes
    gt.append(voc_gt(8, [11, 14, 15]))
    for _ in range(300):
        recs.append(voc_rec(8, rng.choice([11, 14, 15, 2]), round(rng.random(), 3), rand_box(rng, grid=True)))
    train = sorted(recs, key=lambda r: r["category_id"])                     # the writer's class-major order (stable)
    gt_train = gt

    recs, gt_val = [], []
    for img in range(100, 140):
        cls = rng.sample(range(20), rng.randint(1, 3))
        if img % 9 != 0:
            gt_val.append(voc_gt(img, cls + [cls[0]]))
        for _ in range(rng.randint(1, 30)):
            c = rng.choice(cls) if rng.random() < 0.8 else rng.randrange(20)
            recs.append(voc_rec(img, c, round(rng.random(), 3), rand_box(rng, grid=rng.random() < 0.5)))
    gt_val.append(voc_gt(999, [1]))                                       # ground truth without detections
    val = sorted(recs, key=lambda r: r["category_id"])
    return {"train": train, "val": val}, {"train": gt_train, "val": gt_val}


def coco_inputs():
    rng = random.Random(7)
    dets, gts, bases = {}, {}, {}
    for split, seed_imgs in (("train", range(1, 31)), ("val", range(500, 520))):
        d, g = [], []
        for img in seed_imgs:
            cls = rng.sample(range(80), rng.randint(1, 3))
            if img % 11 != 0:
                g.append({"image_id": img, "annotations": [{"category_id": c} for c in cls]})
            n = 300 if img == 5 else rng.randint(0, 40)
            inst = []
            for _ in range(n):
                c = rng.choice(cls) if rng.random() < 0.7 else rng.randrange(80)
                x, y = round(rng.uniform(0, 500), 2), round(rng.uniform(0, 400), 2)
                w, h = (round(rng.uniform(0, 200), 2), round(rng.uniform(0, 200), 2)) if img != 5 else \
                    (float(rng.randrange(1, 8) * 16), float(rng.randrange(1, 8) * 16))
                if img == 5:
                    x, y = float(rng.randrange(0, 8) * 16), float(rng.randrange(0, 8) * 16)
                inst.append({"image_id": img, "category_id": c, "bbox": [x, y, w, h], "score": round(rng.random(), 4)})
            d.append({"image_id": img, "instances": inst})
        d.append({"image_id": d[3]["image_id"], "instances": d[4]["instances"][:5]})     # repeated image id: the last wins
        dets[split], gts[split] = d, g
        bases[split] = {"info": {"description": f"synthetic {split}"}, "images": [{"id": x["image_id"]} for x in g],
                        "annotations": [{"id": 0}], "categories": [{"id": v} for v in range(1, 91)]}
    return dets, gts, bases


# ---------------------------------------------------------------------------------------------------------------------- runs
def run_voc(pgf, det, gt, t_con, t_keep, use_diff):
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(f"{tmp}/uwsod"); os.makedirs(f"{tmp}/det"); os.makedirs(f"{tmp}/out")
        for s in ("train", "val"):
            DATASETS[f"voc_2007_{s}"] = gt[s]
            with open(f"{tmp}/det/oicr_plus_voc_2007_{s}.json", "w") as f:
                json.dump(det[s], f)
        cwd = os.getcwd()
        os.chdir(tmp)
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                pgf.pgf_voc(f"{tmp}/det", f"{tmp}/out", "oicr_plus_", t_con, t_keep, use_diff, "2007")
        finally:
            os.chdir(cwd)
        out = {s: open(f"{tmp}/out/oicr_plus_voc_2007_{s}.json").read() for s in ("train", "val")}
    return out, counts_of(buf.getvalue())


def run_add_multi_label(aml, outs, gt):
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(f"{tmp}/unbias")
        for s in ("train", "val"):
            DATASETS[f"voc_2007_{s}"] = gt[s]
            with open(f"{tmp}/pgt_{s}.json", "w") as f:
                f.write(outs[s])
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                aml.add_voc07(f"{tmp}/pgt_{{}}.json")
        finally:
            os.chdir(cwd)
        return {s: open(f"{tmp}/pgt_{s}.json").read() for s in ("train", "val")}


def run_voc_loader(voc, pgts):
    """load_voc_instances_wsl over every image of each split's pseudo-label file, with a VOC-style tree in a temp dir"""
    images, dicts = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            os.makedirs("VOC2007/ImageSets/Main"); os.makedirs("VOC2007/Annotations"); os.makedirs("VOC2007/pseudo_labels")
            for s in ("train", "val"):
                ids = [int(k) for k in json.loads(pgts[s]) if k != "multi_label"]
                with open(f"VOC2007/ImageSets/Main/{s}.txt", "w") as f:
                    f.write("".join(f"{i:06d}\n" for i in ids))
                with open(f"VOC2007/pseudo_labels/oicr_plus_voc_2007_{s}.json", "w") as f:
                    f.write(pgts[s])
                hw = [(300 + k, 400 + 2 * k) for k in range(len(ids))]
                for i, (h, w) in zip(ids, hw):
                    with open(f"VOC2007/Annotations/{i:06d}.xml", "w") as f:
                        f.write(f"<annotation><size><width>{w}</width><height>{h}</height></size></annotation>")
                images[s] = {"id": ids, "h": [h for h, _ in hw], "w": [w for _, w in hw]}
                dicts[s] = voc.load_voc_instances_wsl("VOC2007", s, voc.CLASS_NAMES)
        finally:
            os.chdir(cwd)
    return images, dicts


def run_coco(pgf, det, gt, base, t_con, t_keep):
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(f"{tmp}/uwsod"); os.makedirs(f"{tmp}/det"); os.makedirs(f"{tmp}/out"); os.makedirs(f"{tmp}/coco/annotations")
        names = {"train": ("coco_2014_train", "instances_train2014.json", "coco_2014_train"),
                 "val": ("coco_2014_valminusminival", "instances_valminusminival2014.json", "coco_2014_valminusminival2014")}
        for s, (name, base_file, _) in names.items():
            DATASETS[name] = gt[s]
            with open(f"{tmp}/det/oicr_plus_{name}.json", "w") as f:
                json.dump(det[s], f)
            with open(f"{tmp}/coco/annotations/{base_file}", "w") as f:
                json.dump(base[s], f)
        cwd = os.getcwd()
        os.chdir(tmp)
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                pgf.pgf_coco(f"{tmp}/det", f"{tmp}/out", "oicr_plus_", t_con, t_keep, True, f"{tmp}/coco")
        finally:
            os.chdir(cwd)
        out = {s: open(f"{tmp}/out/oicr_plus_{names[s][2]}.json").read() for s in names}
    return out, counts_of(buf.getvalue())


def det_arrays(recs, s):
    return {f"{s}_det_image": np.array([r["image_id"] for r in recs], dtype=np.int64),
            f"{s}_det_cat": np.array([r["category_id"] for r in recs], dtype=np.int64),
            f"{s}_det_score": np.array([r["score"] for r in recs], dtype=np.float64).reshape(-1),
            f"{s}_det_bbox": np.array([r["bbox"] for r in recs], dtype=np.float64).reshape(-1, 4)}


def gt_arrays(gt, s):
    cls = [[a["category_id"] for a in d["annotations"]] for d in gt]
    return {f"{s}_gt_image": np.array([d["image_id"] for d in gt], dtype=np.int64),
            f"{s}_gt_off": np.cumsum([0] + [len(c) for c in cls]).astype(np.int64),
            f"{s}_gt_cls": np.array([c for cs in cls for c in cs], dtype=np.int64)}


def voc_fixture(pgf, aml, voc):
    det, gt = voc_inputs()
    z = {}
    for s in F.SPLITS:
        z.update(det_arrays(det[s], s)); z.update(gt_arrays(gt[s], s))
    det = {s: F.voc_records(z, s) for s in F.SPLITS}          # what the tests rebuild is what the reference reads
    gt = {s: F.gt_dicts(z, s, voc=True) for s in F.SPLITS}
    for case, prm in (("voc_a", (0.85, 0.2, False)), ("voc_b", (0.7, 0.3, True))):
        z[f"{case}_params"] = np.array(prm, dtype=np.float64)
        out, counts = run_voc(pgf, json.loads(json.dumps(det)), gt, *prm)
        for s in F.SPLITS:
            z[f"{case}_{s}_sha256"] = np.array(F.sha256(out[s]))
            z[f"{case}_{s}_counts"] = np.array(counts[s], dtype=np.int64)
        if case == "voc_a":
            filtered = out
    # add_voc07 + the Stage-3 loader on voc_a's output, and on the unfiltered file (which a test rebuilds without the GPU)
    for tag, pgts in (("voc_a", filtered), ("unfiltered", {s: json.dumps(F.voc_unfiltered_pgt(z, s)) for s in F.SPLITS})):
        ml = run_add_multi_label(aml, pgts, gt)
        images, dicts = run_voc_loader(voc, ml)
        for s in F.SPLITS:
            z[f"{tag}_{s}_multi_label_sha256"] = np.array(F.sha256(ml[s]))
            z[f"{tag}_{s}_dicts_sha256"] = np.array(F.sha256(json.dumps(dicts[s])))
            for k, v in images[s].items():             # both files list the same images: every one with a detection
                assert f"{s}_img_{k}" not in z or z[f"{s}_img_{k}"].tolist() == v
                z[f"{s}_img_{k}"] = np.array(v, dtype=np.int64)
    return z


def coco_fixture(pgf):
    det, gt, base = coco_inputs()
    z = {}
    for s in F.SPLITS:
        z.update(det_arrays([i for e in det[s] for i in e["instances"]], s)); z.update(gt_arrays(gt[s], s))
        z[f"{s}_entry_image"] = np.array([e["image_id"] for e in det[s]], dtype=np.int64)
        z[f"{s}_entry_off"] = np.cumsum([0] + [len(e["instances"]) for e in det[s]]).astype(np.int64)
        z[f"{s}_base"] = np.array(json.dumps(base[s]))
    det = {s: F.coco_records(z, s) for s in F.SPLITS}
    gt = {s: F.gt_dicts(z, s, voc=False) for s in F.SPLITS}
    z["coco_a_params"] = np.array((0.85, 0.2, True), dtype=np.float64)
    out, counts = run_coco(pgf, det, gt, base, 0.85, 0.2)
    for s in F.SPLITS:
        z[f"coco_a_{s}_sha256"] = np.array(F.sha256(out[s]))
        z[f"coco_a_{s}_counts"] = np.array(counts[s], dtype=np.int64)
    return z


def main(out_dir=HERE):
    pgf, aml, voc = install()
    for name, z in (("voc", voc_fixture(pgf, aml, voc)), ("coco", coco_fixture(pgf))):
        np.savez_compressed(os.path.join(out_dir, f"pgf_{name}.npz"), **z)
        print(name, {k: v.tolist() for k, v in z.items() if k.endswith("_counts")})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)

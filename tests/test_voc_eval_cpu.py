"""CPU: the host side of the VOC evaluation (sos_wsod_amd.evaluation): the annotation reader against the reference's parse_rec
output stored in tests/golden/voc_eval_hand.npz, the fixtures' arrays through lines / records / the devkit tree and back, the
errors raised before any GPU work, the CLI's argument errors and the rank-order gather on a gloo world of two."""
import json
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import voc_eval_fixture as F


def _gt(z, tmp_path):
    from sos_wsod_amd import evaluation as E
    return E.GroundTruth.load(F.write_devkit(z, tmp_path / "VOC2007"), F.SPLIT, F.CLASS_NAMES)


def test_xml_reader_equals_reference_parse_rec(golden_dir, tmp_path):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "hand")
    root = F.write_devkit(z, tmp_path / "VOC2007")
    want = json.loads(str(z["parse_rec_json"]))
    got = {n: E.parse_rec(os.path.join(root, "Annotations", n + ".xml")) for n in F.names(z)}
    assert got == want


@pytest.mark.parametrize("case", F.CASES)
def test_fixture_arrays_round_trip(golden_dir, tmp_path, case):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, case)
    gt = _gt(z, tmp_path)
    assert gt.names == F.names(z) and gt.images == list(dict.fromkeys(F.names(z)))
    cls, img, score, box = F.detections(z)
    for dets in (E.Detections.from_lines(F.lines(z), gt), E.Detections.from_records(F.records(z), gt)):
        for k, (i, s, b) in enumerate(dets.per_class):
            sel = cls == k
            assert np.array_equal(i, img[sel]) and np.array_equal(s, score[sel], equal_nan=True)
            assert np.array_equal(b, box[sel], equal_nan=True)
    # the ground-truth layout: per (image, class) the objects of that class in annotation order
    recs = F.recs(z)
    K = len(F.CLASS_NAMES)
    for i, n in enumerate(gt.images):
        for k in range(K):
            rows = range(gt.gt_off[i * K + k], gt.gt_off[i * K + k + 1])
            objs = [o for o in recs[n] if o["name"] == F.CLASS_NAMES[k]]
            assert [list(gt.gt_box[r]) for r in rows] == [[float(v) for v in o["bbox"]] for o in objs]
            assert [int(gt.gt_diff[r]) for r in rows] == [o["difficult"] for o in objs]
    # npos counts the image-set lines, a repeated line included
    npos = np.zeros(K, dtype=np.int64)
    for n in gt.names:
        for o in recs[n]:
            if o["name"] in F.CLASS_NAMES and not o["difficult"]:
                npos[F.CLASS_NAMES.index(o["name"])] += 1
    assert np.array_equal(gt.npos, npos)


def _no_gpu(monkeypatch):
    from sos_wsod_amd import ops

    def fail(*a, **k):
        raise AssertionError("reached the GPU")
    monkeypatch.setattr(ops, "voc_eval", fail)


def test_value_errors_before_gpu_work(golden_dir, tmp_path, monkeypatch):
    from sos_wsod_amd import evaluation as E
    _no_gpu(monkeypatch)
    z = F.load(golden_dir, "npos0")
    gt = _gt(z, tmp_path)
    dets = E.Detections.from_lines(F.lines(z), gt)
    with pytest.raises(ValueError, match="CorLoc is undefined"):
        E.voc_eval_arrays(gt, dets)
    lines = F.lines(z)
    lines[2].append("999999 0.500 1.0 1.0 5.0 5.0")
    with pytest.raises(ValueError, match="not in the split"):
        E.Detections.from_lines(lines, gt)
    recs = F.records(z) + [{"image_id": 999999, "category_id": 3, "score": 0.5, "bbox": [1.0, 1.0, 5.0, 5.0]}]
    with pytest.raises(ValueError, match="not in the split"):
        E.Detections.from_records(recs, gt)
    with pytest.raises(ValueError, match="category_id"):
        E.Detections.from_records([{"image_id": 1, "category_id": 21, "score": 0.5, "bbox": [1.0, 1.0, 5.0, 5.0]}], gt)
    with pytest.raises(ValueError, match="6 fields"):
        E.Detections.from_lines({0: ["000001 0.5 1.0 1.0"]}, gt)
    with pytest.raises(ValueError, match="2012_test|voc_2012_test"):
        E.PascalVOCDetectionEvaluator(str(tmp_path), "test", 2012)
    with pytest.raises(ValueError, match="year"):
        E.PascalVOCDetectionEvaluator(str(tmp_path), "test", 2010)
    with pytest.raises(ValueError, match="classes"):
        E.voc_eval_arrays(E.GroundTruth([], {}, [f"c{k}" for k in range(257)]), E.Detections([([], [], [])] * 257))


def test_cli_argument_errors(golden_dir, tmp_path, capsys):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "hand")
    root = F.write_devkit(z, tmp_path / "VOC2007")
    det = tmp_path / "dets.json"
    det.write_text(json.dumps(F.records(z)))
    bad = [[],
           ["--voc-root", root, "--split", F.SPLIT],                                          # no --detections
           ["--voc-root", root, "--split", F.SPLIT, "--detections", str(tmp_path / "none.json")],
           ["--voc-root", root, "--split", "trainval", "--detections", str(det)],              # no image set
           ["--voc-root", root, "--split", "test", "--year", "2012", "--detections", str(det)],
           ["--voc-root", root, "--split", F.SPLIT, "--year", "2010", "--detections", str(det)]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            E.parse_args(argv)
        assert e.value.code == 2, argv
    args = E.parse_args(["--voc-root", root, "--split", F.SPLIT, "--detections", str(det)])
    assert (args.year, args.out) == (2007, None)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import evaluation as E
    lines = {0: [f"r{rank}a", f"r{rank}b"], 2: [f"r{rank}c"]} if rank == 0 else {1: [f"r{rank}d"], 2: [f"r{rank}e"]}
    got = E.gather_lines(lines, 3)
    with open(f"{out}.{rank}", "w") as f:
        json.dump(got, f)
    dist.barrier()
    dist.destroy_process_group()


def test_gather_lines_rank_order_gloo_world2(tmp_path):
    out = str(tmp_path / "g")
    mp.spawn(_gather_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    with open(out + ".0") as f:
        r0 = json.load(f)
    with open(out + ".1") as f:
        r1 = json.load(f)
    assert r0 == {"0": ["r0a", "r0b"], "1": ["r1d"], "2": ["r0c", "r1e"]}
    assert r1 is None

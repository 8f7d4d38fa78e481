"""GPU: the PGF threshold sweep (ops.pgf_sweep / sos_wsod_amd.pgf_sweep) against the NumPy forms of tests/pgf_sweep_ref.py, against
ops.pgf_keep cell by cell, and on the reference-made fixtures tests/golden/pgf_{voc,coco}.npz.  Every comparison is integer
equality."""
import numpy as np
import pytest

import pgf_fixture as F
import pgf_sweep_ref as R

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = -0x0123456789ABCDEF
TABLES = ("kept", "tp", "ign", "npos")


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_inputs(case):
    gt_mask, diff_mask = R.masks(case)
    return {"det_off": _up(case["off"]), "boxes": _up(case["boxes"]), "scores": _up(case["scores"]),
            "classes": _up(case["classes"]), "gt_mask": _up(gt_mask.view(np.int32)), "diff_mask": _up(diff_mask.view(np.int32)),
            "gt_off": _up(case["gt_off"]), "gt_box": _up(case["gt_box"]), "gt_cls": _up(case["gt_cls"]),
            "gt_ign": _up(case["gt_ign"])}


def _sweep(case, d, out=None, guard=0, **over):
    from sos_wsod_amd import ops
    a = dict(K=case["K"], use_diff=case["use_diff"], t_keep=case["t_keep"], t_con=case["t_con"], iou=case["iou"],
             xywh=case["xywh"], plus_one=case["plus_one"], boxes=d["boxes"])
    a.update(over)
    return ops.pgf_sweep(d["det_off"], a["boxes"], d["scores"], d["classes"], a["K"], d["gt_mask"], d["diff_mask"], a["use_diff"],
                         a["t_keep"], a["t_con"], a["iou"], d["gt_off"], d["gt_box"], d["gt_cls"], d["gt_ign"], a["xywh"],
                         a["plus_one"], guard=guard, out=out)


def _guarded(case):
    import torch
    from sos_wsod_amd import ops
    layout, total = ops.pgf_sweep_layout(len(case["t_keep"]), len(case["t_con"]), len(case["iou"]), case["K"], GUARD)
    return torch.full((total,), SENTINEL, dtype=torch.int64, device="cuda"), layout, total


def _bands_untouched(host, layout, total):
    inside = np.zeros(total, dtype=bool)
    for at, shape in layout.values():
        inside[at:at + int(np.prod(shape))] = True
    assert (~inside).sum() == 5 * GUARD
    return bool((host[~inside] == SENTINEL).all())


@pytest.mark.parametrize("name", list(R.CASES))
def test_tables_equal_reference_guard_bands_and_repeat(name):
    """every table equals the NumPy form; the words around each table keep their sentinel; a second launch gives the same bits"""
    from sos_wsod_amd import ops
    case = R.make_case(name)
    d = _device_inputs(case)
    out, layout, total = _guarded(case)
    host = _sweep(case, d, out, GUARD).cpu().numpy()
    assert _bands_untouched(host, layout, total)
    got = ops.pgf_sweep_unpack(host, len(case["t_keep"]), len(case["t_con"]), len(case["iou"]), case["K"], GUARD)
    for key in TABLES:
        bad = np.argwhere(got[key] != case["expected"][key])
        assert bad.size == 0, f"{name} {key}: {len(bad)} entries differ, first at {bad[:3].tolist()}"
    again = _sweep(case, d).cpu().numpy()                   # fresh, unguarded memory
    plain = ops.pgf_sweep_unpack(again, len(case["t_keep"]), len(case["t_con"]), len(case["iou"]), case["K"])
    for key in TABLES:
        assert np.array_equal(plain[key], got[key]), (name, key)


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_cell_is_pgf_keep_plus_the_matching_rule(name):
    """composition: ops.pgf_keep's flags at (t_keep[a], t_con[b]), matched by voc_eval's sequential loop, are the sweep's cell"""
    from sos_wsod_amd import ops
    case = R.make_case(name)
    d = _device_inputs(case)
    nk, nc, nt, K = len(case["t_keep"]), len(case["t_con"]), len(case["iou"]), case["K"]
    got = ops.pgf_sweep_unpack(_sweep(case, d).cpu().numpy(), nk, nc, nt, K)
    done = {}
    for a, tk in enumerate(case["t_keep"]):
        for b, tc in enumerate(case["t_con"]):
            if (tk, tc) not in done:                        # a repeated pair of grid values is the same launch
                packed = ops.pgf_keep(d["det_off"], d["boxes"], d["scores"], d["classes"], K, d["gt_mask"], d["diff_mask"], tk, tc,
                                      case["use_diff"]).cpu().numpy()
                done[(tk, tc)] = R.match_cell(case, packed[32:].astype(bool)) + (int(packed[:32].view(np.int64)[3]),)
            kept, tp, ign, after = done[(tk, tc)]
            assert got["kept"][a, b].sum() == after
            assert np.array_equal(got["kept"][a, b], kept), (name, a, b)
            assert np.array_equal(got["tp"][:, a, b], tp), (name, a, b)
            assert np.array_equal(got["ign"][:, a, b], ign), (name, a, b)


@pytest.mark.parametrize("what", ["nk_33", "nc_0", "nt_11", "nan_t_con", "inf_t_keep", "nan_iou", "K_257", "K_0", "boxes_misaligned"])
def test_refused_launch_writes_nothing(what):
    import torch
    from sos_wsod_amd._lib import HipKernelError
    case = R.make_case("grid_1x1")
    d = _device_inputs(case)
    over = {"nk_33": {"t_keep": [0.2] * 33}, "nc_0": {"t_con": []}, "nt_11": {"iou": [0.5] * 11},
            "nan_t_con": {"t_con": [0.85, float("nan")]}, "inf_t_keep": {"t_keep": [float("inf")]},
            "nan_iou": {"iou": [float("nan")]}}.get(what, {})
    sizes = {k: max(len(over.get(k, case[k])), 1) for k in ("t_keep", "t_con", "iou")}
    K = case["K"]
    if what == "boxes_misaligned":
        flat = torch.zeros(case["boxes"].size + 1, dtype=torch.float64, device="cuda")
        flat[1:] = d["boxes"].reshape(-1)
        over = {"boxes": flat[1:].view(-1, 4)}
        assert over["boxes"].data_ptr() % 16 == 8
    from sos_wsod_amd import ops
    total = ops.pgf_sweep_layout(sizes["t_keep"], sizes["t_con"], sizes["iou"], K, GUARD)[1]
    out = torch.full((total,), SENTINEL, dtype=torch.int64, device="cuda")
    if what in ("K_257", "K_0"):
        # the wrapper's own shape checks stand in front of the entry point: call it directly
        from sos_wsod_amd._lib import lib
        import ctypes
        p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
        one = (ctypes.c_double * 1)(0.5)
        ws = torch.empty(max(len(case["scores"]), 1) * ops.PGF_SWEEP_WS_WORDS, dtype=torch.int32, device="cuda")
        tab = ctypes.c_void_p(out.data_ptr() + 8 * GUARD)
        rc = lib.sw_pgf_sweep(len(case["off"]) - 1, len(case["scores"]), p(d["det_off"]), p(d["boxes"]), p(d["scores"]),
                              p(d["classes"]), 257 if what == "K_257" else 0, p(d["gt_mask"]), p(d["diff_mask"]), 0, 1, one, 1, one, 1,
                              one, p(d["gt_off"]), p(d["gt_box"]), p(d["gt_cls"]), p(d["gt_ign"]), 0, 1, p(ws), tab, tab, tab, tab,
                              None)
        assert rc == -6
    else:
        with pytest.raises(HipKernelError) as e:
            _sweep(case, d, out, GUARD, **over)
        assert ("code -4" if what == "boxes_misaligned" else "code -7") in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def _seeded_dicts(z, s, voc, seed):
    """the fixture's ground-truth dicts (classes only) with boxes and ignore flags drawn from a seed; about half the boxes are a
    detection's own box, so that matches occur"""
    rng = np.random.default_rng(seed)
    dicts = F.gt_dicts(z, s, voc)
    bbox, cat, img = z[f"{s}_det_bbox"], z[f"{s}_det_cat"] - (1 if voc else 0), z[f"{s}_det_image"]
    for d in dicts:
        for a in d["annotations"]:
            rows = np.nonzero((img == int(d["image_id"])) & (cat == a["category_id"]))[0]
            if len(rows) and rng.random() < 0.6:
                b = bbox[rng.choice(rows)].tolist()
                b = [b[0] - 1.0, b[1] - 1.0, b[2], b[3]] if voc else b       # VOC dicts hold 0-based x1 / y1
            else:
                x, y = rng.uniform(0, 200, 2).round(1).tolist()
                w, h = rng.uniform(10, 200, 2).round(1).tolist()
                b = [x, y, x + w, y + h] if voc else [x, y, w, h]
            a["bbox"], a["bbox_mode"] = b, 0 if voc else 1
            a["difficult" if voc else "iscrowd"] = int(rng.random() < 0.15)
    return dicts


def _case_of(S, P, groups, anns, grid, use_diff, diff, key, xywh, shift):
    """the module's own host packing as a reference case"""
    class_dict = {i: P._unique(a["category_id"] for a in anns[i]) for i in groups}
    g = P.pack_groups(groups, class_dict, diff)
    gt_off, gt_box, gt_cls, gt_ign = S.pack_ground_truth(g["ids"], anns, g["universe"], key, shift)
    dense = {int(c): k for k, c in enumerate(g["universe"])}
    return {"off": g["off"], "boxes": g["boxes"], "scores": g["scores"], "classes": g["classes"], "K": g["K"],
            "gt_sets": [{dense[c] for c in class_dict[i]} for i in g["ids"]], "gt_off": gt_off, "gt_box": gt_box, "gt_cls": gt_cls,
            "gt_ign": gt_ign, "diff": tuple(dense[c] for c in diff if c in dense), "use_diff": use_diff, "xywh": xywh,
            "plus_one": not xywh, "t_keep": grid[0], "t_con": grid[1], "iou": list(S.IOU_THRESHOLDS)}


@pytest.mark.parametrize("case", list(F.CASES))
def test_fixture_cells_sum_to_the_reference_counts(golden_dir, case, monkeypatch):
    """on the reference-made fixtures: the cell at the fixture's own thresholds keeps as many detections as the reference's run
    counted after its containment stage; the whole result equals the NumPy form on the module's own packing; one copy per split;
    score() is that cell; the inputs are left as they were"""
    import copy
    import torch
    from sos_wsod_amd import pgf_sweep as S
    from sos_wsod_amd import pseudo_labels as P
    voc = F.CASES[case] == "voc"
    z = F.load(golden_dir, F.CASES[case])
    t_con, t_keep, use_diff = F.params(z, case)
    grid = ([0.5, t_keep, 0.0], [t_con, 0.6])
    copies = []
    orig = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        if self.is_cuda:
            copies.append(self.numel())
        return orig(self, *a, **k)

    for n, s in enumerate(F.SPLITS):
        dicts = _seeded_dicts(z, s, voc, 100 + n)
        dets = F.voc_records(z, s) if voc else F.coco_records(z, s)
        before = copy.deepcopy((dets, dicts))
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "cpu", counting_cpu)
            del copies[:]
            if voc:
                res = S.sweep_voc(dets, dicts, grid[0], grid[1], use_diff=use_diff)
            else:
                res = S.sweep_coco(dets, dicts, grid[0], grid[1], use_diff=use_diff)
            assert len(copies) == 1
        assert (dets, dicts) == before
        assert int(res.kept[1, 0].sum()) == int(z[f"{case}_{s}_counts"][3]), (case, s)
        groups, anns = (S.voc_groups if voc else S.coco_groups)(dets, dicts)
        ref = _case_of(S, P, groups, anns, grid, use_diff, P.VOC_DIFF_CLASSES if voc else (), "difficult" if voc else "iscrowd",
                       not voc, (1.0, 1.0, 0.0, 0.0) if voc else (0.0,) * 4)
        want = R.decomposed_tables(ref)
        for key in TABLES:
            assert np.array_equal(getattr(res, key), want[key]), (case, s, key)
        assert res.tp.sum() > 0 and res.npos.sum() > 0
        one = S.score(dets, dicts, "voc" if voc else "coco", t_con, t_keep, use_diff=use_diff)
        assert np.array_equal(one.kept[0, 0], res.kept[1, 0]) and np.array_equal(one.tp[:, 0, 0], res.tp[:, 1, 0])
        assert np.array_equal(one.ign[:, 0, 0], res.ign[:, 1, 0]) and np.array_equal(one.npos, res.npos)


def test_cli_prints_the_table_and_writes_json(golden_dir, tmp_path, capsys):
    import json
    from sos_wsod_amd import pgf_sweep as S
    z = F.load(golden_dir, "voc")
    (tmp_path / "det").mkdir()
    gt = {}
    for n, s in enumerate(F.SPLITS):
        (tmp_path / "det" / f"oicr_plus_voc_2007_{s}.json").write_text(json.dumps(F.voc_records(z, s)))
        gt[f"voc_2007_{s}"] = _seeded_dicts(z, s, True, 100 + n)
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    out = S.main(["--det-path", str(tmp_path / "det"), "--gt-dicts", str(tmp_path / "gt.json"), "--t-keep", "0.1:0.3:0.1",
                  "--t-con", "0.85,0.7", "--out", str(tmp_path / "table.json")])
    text = capsys.readouterr().out
    assert 't_keep ["0.1", "0.2", "0.3"]' in text and 't_con ["0.85", "0.7"]' in text
    assert "voc_2007_train: F1 at IoU 0.5" in text and "voc_2007_val best" in text
    saved = json.loads((tmp_path / "table.json").read_text())
    for s in F.SPLITS:
        name = f"voc_2007_{s}"
        assert int(np.sum(saved[name]["kept"][1][0])) == int(z[f"voc_a_{s}_counts"][3])
        back = S.SweepResult.from_json(saved[name])
        assert back.best() == saved[name]["best"] == out[name]["best"]

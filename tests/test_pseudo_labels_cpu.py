"""CPU: the Stage-2 pseudo-label fixtures (tests/golden/pgf_{voc,coco}.npz) are what their generator makes from the reference, the host-only
parts of sos_wsod_amd.pseudo_labels (add_multi_label, load_voc_pseudo_labels) match them, and the CLI parses as documented."""
import json
import os
import subprocess
import sys

import pytest

import pgf_fixture as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REFERENCE_TOOLS = "/root/reference/tools/pgf.py"


@pytest.mark.skipif(not os.path.exists(REFERENCE_TOOLS), reason="the reference tree is only present where fixtures are made")
def test_generator_reproduces_fixtures(golden_dir, tmp_path):
    subprocess.check_call([sys.executable, os.path.join(golden_dir, "make_pgf_golden.py"), str(tmp_path)], stdout=subprocess.DEVNULL)
    for name in ("voc", "coco"):
        committed, fresh = F.load(golden_dir, name), F.load(str(tmp_path), name)
        assert sorted(committed) == sorted(fresh), name
        for k, v in committed.items():                     # same dtype, shape and bits (an .npz file itself carries timestamps)
            assert v.dtype == fresh[k].dtype and v.shape == fresh[k].shape and v.tobytes() == fresh[k].tobytes(), (name, k)


def test_add_multi_label_matches_reference(golden_dir):
    from sos_wsod_amd import pseudo_labels as P
    z = F.load(golden_dir, "voc")
    for s in F.SPLITS:
        pgt = P.add_multi_label(F.voc_unfiltered_pgt(z, s), F.gt_dicts(z, s, voc=True))
        assert F.sha256(json.dumps(pgt)) == str(z[f"unfiltered_{s}_multi_label_sha256"]), s


def test_add_multi_label_coco_keys_are_image_ids(golden_dir):
    from sos_wsod_amd import pseudo_labels as P
    gt = F.gt_dicts(F.load(golden_dir, "coco"), "train", voc=False)
    pgt = P.add_multi_label({}, gt, coco=True)
    assert list(pgt["multi_label"]) == [d["image_id"] for d in gt]
    assert all(len(set(v)) == len(v) for v in pgt["multi_label"].values())


def test_load_voc_pseudo_labels_matches_reference_loader(golden_dir, tmp_path):
    from sos_wsod_amd import pseudo_labels as P
    z = F.load(golden_dir, "voc")
    for s in F.SPLITS:
        text = json.dumps(P.add_multi_label(F.voc_unfiltered_pgt(z, s), F.gt_dicts(z, s, voc=True)))
        pgt = json.loads(text)
        assert F.sha256(json.dumps(P.load_voc_pseudo_labels(pgt, F.voc_images(z, s)))) == str(z[f"unfiltered_{s}_dicts_sha256"]), s
        assert "multi_label" in pgt                                    # the caller's dict is left as it was
        path = tmp_path / f"{s}.json"
        path.write_text(text)
        assert F.sha256(json.dumps(P.load_voc_pseudo_labels(str(path), F.voc_images(z, s)))) == str(z[f"unfiltered_{s}_dicts_sha256"])
    d = P.load_voc_pseudo_labels(json.loads(json.dumps(F.voc_unfiltered_pgt(z, "train"))), F.voc_images(z, "train")[:1])[0]
    assert "multi_label" not in d and all(isinstance(v, int) for a in d["annotations"] for v in a["bbox"])


def test_cli_parses_floats_and_defaults():
    from sos_wsod_amd import pseudo_labels as P
    a = P.parse_args(["--gt-dicts", "gt.json", "--t-con", "0.9", "--t-keep", "0.25"])
    assert a.t_con == 0.9 and a.t_keep == 0.25 and isinstance(a.t_con, float) and isinstance(a.t_keep, float)
    a = P.parse_args(["--gt-dicts", "gt.json"])
    assert (a.t_con, a.t_keep, a.use_diff, a.dataset, a.prefix) == (0.85, 0.2, False, "voc2007", "oicr_plus_")
    a = P.parse_args(["--gt-dicts", "gt.json", "--dataset", "coco", "--use-diff", "--coco-path", "c"])
    assert a.use_diff and a.coco_path == "c"


def test_cli_rejects_coco_without_use_diff():
    from sos_wsod_amd import pseudo_labels as P
    with pytest.raises(SystemExit):
        P.parse_args(["--gt-dicts", "gt.json", "--dataset", "coco"])
    with pytest.raises(ValueError):
        P.pgf_coco([], [], use_diff=False)


def test_module_entry_point_runs_through_the_import_shim():
    r = subprocess.run([sys.executable, "-m", "sos_wsod_amd.pseudo_labels", "--dataset", "coco", "--gt-dicts", "x.json"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--use-diff" in r.stderr, r.stderr

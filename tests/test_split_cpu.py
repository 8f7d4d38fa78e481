"""CPU: the Stage 2 -> 3 split files (sos_wsod_amd.split) against the bytes the reference's split_single.py / generate_base_split.py
wrote and divide_label_unlabel returned (tests/golden/make_split_golden.py -> split_files.npz), the chosen tie / NaN order, the two
bisection bugs as ValueError, the checkpoint prefix rule, the detector's loss-config keys and the CLI with a fake scorer."""
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_files.npz")


@pytest.fixture(scope="module")
def S():
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import split
    return split


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def _cases(g):
    return sorted(k[5:] for k in g.files if k.startswith("file_"))


def test_loss_split_writes_the_reference_bytes(S, g, tmp_path):
    assert len(_cases(g)) >= 5
    for c in _cases(g):
        obj, percent = S.loss_split(g[f"loss_{c}"], int(g[f"k_{c}"]))
        out = tmp_path / f"{c}.txt"
        S.write_split(obj, str(out))
        assert out.read_bytes() == g[f"file_{c}"].tobytes(), c
        assert f"The finded percent is: {percent}" == str(g[f"pct_{c}"]), c


def test_base_split_writes_the_reference_bytes(S, g, tmp_path):
    for key in [k for k in g.files if k.startswith("base_")]:
        n = int(key[5:])
        obj, _ = S.base_split(n)
        out = tmp_path / key
        S.write_split(obj, str(out))
        assert out.read_bytes() == g[key].tobytes(), key


def test_divide_label_unlabel_matches_the_reference(S, g, tmp_path):
    p = tmp_path / "seed.txt"
    p.write_bytes(g["file_voc07"].tobytes())
    dicts = [{"i": i} for i in range(5011)]
    lab, unl = S.divide_label_unlabel(dicts, float(g["divide_pct"]), 1, str(p))
    assert [d["i"] for d in lab] == g["divide_label"].tolist()
    assert [d["i"] for d in unl] == g["divide_unlabel"].tolist()
    with pytest.raises(AssertionError, match="mismatched"):
        S.divide_label_unlabel(dicts[:-3], float(g["divide_pct"]), 1, str(p))


def test_ties_keep_index_order_and_nan_sorts_last(S):
    v = np.array([0.5, np.nan, 0.25, 0.5, 0.25, np.nan, 0.1, 0.5], dtype=np.float32)
    obj, _ = S.loss_split(v, 8)
    assert list(obj.values())[0]["1"] == [6, 2, 4, 0, 3, 7, 1, 5]
    obj, _ = S.loss_split(v, 3)
    assert list(obj.values())[0]["1"] == [6, 2, 4]


def test_bisection_bugs_raise_instead_of_looping(S):
    # int(length * middle) < k at the first middle: the reference's `begin = middle` never moves the bound (needs a length
    # above ~10^7, where the 7-decimal rounding of the middle exceeds half an image)
    n = 30_000_000
    k = next(k for k in range(1, 1000) if int(n * round((k / n + (k + 1) / n) / 2, 7)) < k)
    with pytest.raises(ValueError, match="loops forever"):
        S.split_percent(n, k)
    with pytest.raises(ValueError, match="outside"):
        S.loss_split(np.zeros(5, np.float32), 6)
    with pytest.raises(ValueError):
        S.base_split(0)


def test_load_student_state_prefix_rule(S, tmp_path):
    ck = {"model": {"modelStudent.backbone.w": torch.ones(2), "modelTeacher.backbone.w": torch.zeros(2),
                    "modelStudent.roi_heads.b": torch.full((1,), 3.0)}, "iteration": 7}
    p = tmp_path / "m.pth"
    torch.save(ck, str(p))
    sd = S.load_student_state(str(p))
    assert sorted(sd) == ["backbone.w", "roi_heads.b"] and float(sd["roi_heads.b"]) == 3.0


def test_data_seed_keys(S):
    from sos_wsod_amd.config import CfgNode
    cfg = CfgNode({"DATALOADER": {"SUP_PERCENT": 39.92217, "RANDOM_DATA_SEED": 1, "RANDOM_DATA_SEED_PATH": "x.txt"}})
    assert S.data_seed_keys(cfg) == (39.92217, 1, "x.txt")


def test_plan_is_independent_of_batch_size(S):
    rng = np.random.default_rng(0)
    dicts = [{"height": int(rng.integers(200, 500)), "width": int(rng.integers(200, 500)), "annotations": [{}]} for _ in range(40)]
    kw = dict(min_sizes=(96, 128, 160), max_size=300, seed=5)
    per = {}
    for ipb in (1, 3, 8):
        chunks = S.plan(dicts, images_per_batch=ipb, **kw)
        assert all(len(c) <= ipb for c in chunks)
        flat = {e["index"]: (e["out"], e["flip"], tuple(e["seeds"])) for c in chunks for e in c}
        assert sorted(flat) == list(range(40))
        per[ipb] = flat
        for c in chunks:                                          # one padded shape per chunk, index order inside
            assert len({(-(-e["out"][0] // 32), -(-e["out"][1] // 32)) for e in c}) == 1
            assert [e["index"] for e in c] == sorted(e["index"] for e in c)
    assert per[1] == per[3] == per[8]


def test_loss_config_keys_are_read_or_refused():
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd.config import CfgNode
    from sos_wsod_amd.frcnn import _loss_kwargs
    M = CfgNode({"RPN": {"BBOX_REG_LOSS_TYPE": "smooth_l1_mean", "POSITIVE_FRACTION": 1.0},
                 "ROI_HEADS": {"LOSS": "CrossEntropy"}, "ROI_BOX_HEAD": {"BBOX_REG_LOSS_TYPE": "smooth_l1_mean"}})
    assert _loss_kwargs(M) == ({"box_loss_type": "smooth_l1_mean"}, {"loss": "CrossEntropy", "box_loss_type": "smooth_l1_mean"})
    assert _loss_kwargs(CfgNode({})) == ({"box_loss_type": "smooth_l1"}, {"loss": "FocalLoss", "box_loss_type": "smooth_l1"})
    for bad in ({"ROI_HEADS": {"LOSS": "Softmax"}}, {"RPN": {"BBOX_REG_LOSS_TYPE": "giou"}}, {"ROI_BOX_HEAD": {"BBOX_REG_LOSS_TYPE": "diou"}}):
        with pytest.raises(AssertionError, match="not implemented"):
            _loss_kwargs(CfgNode(bad))


def test_cli_end_to_end_with_a_fake_scorer(S, tmp_path, capsys):
    cfg = tmp_path / "c.yaml"
    cfg.write_text("INPUT:\n  MIN_SIZE_TRAIN: (96, 128)\n  MAX_SIZE_TRAIN: 300\n")
    dicts = [{"height": 100 + i, "width": 120, "annotations": [{"bbox": [1, 1, 50, 50], "category_id": 0}] if i != 4 else []}
             for i in range(12)]
    seen = {}

    def scorer(model, ds, loader, *, images_per_batch, seed, min_sizes, max_size):
        seen.update(n=len(ds), ipb=images_per_batch, seed=seed, min_sizes=min_sizes, max_size=max_size)
        return np.array([(7 * i) % 11 for i in range(len(ds))], dtype=np.float32)

    out = tmp_path / "split.txt"
    S.main(["loss", "--config", str(cfg), "--save-path", str(out), "--k", "4", "--images-per-batch", "2", "--seed", "3"],
           scorer=scorer, dataset_dicts=dicts)
    assert seen == dict(n=11, ipb=2, seed=3, min_sizes=(96, 128), max_size=300)            # the empty image is dropped first
    obj = json.loads(out.read_text())
    (pct, entry), = obj.items()
    assert entry["1"] == [0, 8, 5, 2]
    assert f"The finded percent is: {pct}" in capsys.readouterr().out
    lab, unl = S.divide_label_unlabel(S.filter_empty(dicts), float(pct), 1, str(out))
    assert len(lab) == 4 and len(unl) == 7
    base = tmp_path / "base.txt"
    S.main(["base", "--length", "11", "--save-path", str(base)])
    (bp, be), = json.loads(base.read_text()).items()
    lab, unl = S.divide_label_unlabel(S.filter_empty(dicts), float(bp), 1, str(base))
    assert len(lab) == 10 and len(unl) == 1

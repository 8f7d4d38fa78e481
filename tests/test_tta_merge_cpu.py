"""CPU: the Stage-3 test-time-augmentation merge.  tests/golden/tta_merge.npz was written by the reference's own `_merge_detections` ->
`fast_rcnn_inference_single_image` (tests/golden/make_tta_merge_golden.py); the NumPy restatement of sw_tta_merge (tta_merge_ref.py)
must reproduce every case exactly, which pins both.  The wrapper, the helper and the TEST.AUG keys exist and read the reference's two
YAML shapes; the three refusals raise."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tta_merge_ref import F, _iou, inverse_box, tta_merge_ref  # noqa: E402

CASES = ["c1", "c2", "c3", "c4", "c5", "c6", "c7", "c8"]


def load_case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "tta_merge.npz"))
    return {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}


def _ordinary_boxes(rng, n):
    """the box recipe of test_gpu_tta_merge.test_one_class_at_the_row_limit: heavy overlap inside a 500 x 375 image"""
    x0, y0 = rng.uniform(0, 400, n), rng.uniform(0, 300, n)
    return np.stack([x0, y0, x0 + rng.uniform(40, 120, n), y0 + rng.uniform(40, 120, n)], -1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """Inputs that no golden case holds, with the restatement's result for them: (case, want).  Built once; nobody writes to either.
    "negative_nms": nms -1.0, where the kernel takes the plain `iou > thresh` (every IoU that is a number is above it, 0 / 0 is not):
        class 0 five zero-area boxes, class 1 seventy ordinary ones (two chunks of the wave-per-class resolver), class 2 fifteen.
    "chunk_edges": classes of 63, 64, 65 and 129 candidates at nms 0.5 (chunks of 63; 64; 64 + 1; 64 + 64 + 1).  3 * 107 rows are
        321 = 63 + 64 + 65 + 129 already, so the view that is short takes T to 108: counts 108, 108, 105, the rows beyond a count NaN.
    Rows go to the views in a fixed shuffle, every other view flipped."""
    rng = np.random.RandomState({"negative_nms": 11, "chunk_edges": 0}[name])
    if name == "negative_nms":
        sizes, T, counts, nms = (5, 70, 15), 30, (30, 30, 30), -1.0
    else:
        sizes, T, counts, nms = (63, 64, 65, 129), 108, (108, 108, 105), 0.5
    V, K, n = 3, len(sizes), sum(sizes)
    assert n == sum(counts)
    cls = rng.permutation(np.repeat(np.arange(K, dtype=np.int32), sizes))
    b = _ordinary_boxes(rng, n)
    if name == "negative_nms":
        b[cls == 0, 2:] = b[cls == 0, :2]                                        # x1 == x0, y1 == y0
    s = rng.permutation(np.linspace(0.01, 0.99, n)).astype(np.float32)
    boxes, scores, classes = np.full((V, T, 4), np.nan, np.float32), np.ones((V, T), np.float32), np.zeros((V, T), np.int32)
    at = 0
    for v, m in enumerate(counts):
        boxes[v, :m], scores[v, :m], classes[v, :m] = b[at:at + m], s[at:at + m], cls[at:at + m]
        at += m
    tab = np.tile(np.array([[0, 500, 1, 1, 1, 1]], np.float32), (V, 1)); tab[1::2, 0] = 1
    c = dict(boxes=boxes, scores=scores, classes=classes, counts=np.array(counts, np.int32), view_tab=tab, hw=np.array([375, 500]),
             nms=nms, topk=400, K=K)
    return c, run_ref(c)


def class_ranks(c, k):
    """union indices of class k's candidates in the resolver's order (score descending, union index ascending) and their class-offset
    boxes as the restatement forms them; every row below its view's count is a candidate in the edge cases"""
    T = c["scores"].shape[1]
    rows = [(v, s) for v in range(len(c["counts"])) for s in range(int(c["counts"][v]))]
    clip = [tuple(min(max(x, F(0)), F(c["hw"][1 - (j & 1)])) for j, x in enumerate(inverse_box(c["boxes"][v, s], c["view_tab"][v])))
            for v, s in rows]
    off = F(F(k) * F(max(max(b) for b in clip) + F(1)))
    mine = sorted((i for i, (v, s) in enumerate(rows) if c["classes"][v, s] == k), key=lambda i: (-float(c["scores"][rows[i]]), i))
    return [rows[i][0] * T + rows[i][1] for i in mine], [tuple(F(x + off) for x in clip[i]) for i in mine]


def run_ref(c, **over):
    a = dict(c, **over)
    return tta_merge_ref(a["boxes"], a["scores"], a["classes"], a["counts"], a["view_tab"], int(a["hw"][0]), int(a["hw"][1]),
                         float(a["nms"]), int(a["topk"]), int(a["K"]))


def assert_equals_fixture(got, c):
    n = len(c["exp_scores"])
    assert int(got["count"][0]) == n
    assert np.array_equal(got["src"][:n], c["exp_src"])
    assert np.array_equal(got["classes"][:n], c["exp_classes"])
    assert np.array_equal(got["scores"][:n].view(np.uint32), c["exp_scores"].view(np.uint32))
    assert np.array_equal(got["boxes"][:n].view(np.uint32), c["exp_boxes"].view(np.uint32))
    for k in ("boxes", "scores", "classes", "src"):
        assert not got[k][n:].any(), k


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_merge(golden_dir, name):
    c = load_case(golden_dir, name)
    assert_equals_fixture(run_ref(c), c)


def test_fixture_covers_what_it_claims(golden_dir):
    c = load_case(golden_dir, "c3")
    assert c["scores"].shape == (16, 100) and int(c["K"]) == 20 and tuple(c["hw"]) == (375, 500)
    assert sorted(c["counts"])[:2] == [0, 0] and c["counts"].max() == 100 and c["counts"].sum() > 1024
    assert len(c["exp_scores"]) == 100 == int(c["topk"])
    assert run_ref(c, topk=2048)["count"][0] > 100                                # the cut at top-k is exercised
    assert len(set(load_case(golden_dir, "c4")["exp_classes"].tolist())) <= 10 and int(load_case(golden_dir, "c4")["K"]) == 80


def test_rows_beyond_the_count_never_matter_and_a_bad_count_poisons(golden_dir):
    c = load_case(golden_dir, "c3")
    b, s = c["boxes"].copy(), c["scores"].copy()
    for v, n in enumerate(c["counts"]):
        b[v, n:] = np.nan; s[v, n:] = 1.0
    assert_equals_fixture(run_ref(c, boxes=b, scores=s), c)
    bad = c["counts"].copy(); bad[5] = 101
    got = run_ref(c, counts=bad)
    assert got["count"][0] == -1 and not got["scores"].any()


def test_negative_threshold_case_keeps_every_empty_box_and_one_ordinary_box_per_class():
    c, want = edge_case("negative_nms")
    assert float(c["nms"]) == -1.0 and len(c["counts"]) == 3 and int(c["K"]) == 3
    live = c["classes"][np.arange(30)[None, :] < c["counts"][:, None]]
    assert np.bincount(live).tolist() == [5, 70, 15]
    zb = c["boxes"][c["classes"] == 0]
    assert np.array_equal(zb[:, 0], zb[:, 2]) and np.array_equal(zb[:, 1], zb[:, 3])
    n = int(want["count"][0])
    assert np.bincount(want["classes"][:n], minlength=3).tolist() == [5, 1, 1]     # 0 / 0 is never above; any other IoU is above -1
    for k in (1, 2):                                                               # the one survivor is the class's best score
        assert want["scores"][:n][want["classes"][:n] == k][0] == c["scores"][c["classes"] == k].max()


def test_chunk_edge_case_crosses_every_chunk_boundary():
    c, want = edge_case("chunk_edges")
    assert c["counts"].tolist() == [108, 108, 105] and np.isnan(c["boxes"][2, 105:]).all()
    n = int(want["count"][0])
    assert n < int(c["topk"])                                                      # no cut: every survivor is in the result
    surv = set(want["src"][:n].tolist())
    ranks = {k: class_ranks(c, k) for k in range(4)}
    assert [len(ranks[k][0]) for k in range(4)] == [63, 64, 65, 129]
    idx, ob = ranks[3]
    kept = [r for r, i in enumerate(idx) if i in surv]
    assert any(r >= 64 for r in kept)                                              # a candidate past the first chunk survives
    assert any(idx[r] not in surv and any(q < 64 and _iou(ob[q], ob[r]) > F(0.5) for q in kept) for r in range(64, 129))   # one falls to a first-chunk box
    assert 128 in kept                                                             # the chunk of one is reached, alive
    assert ranks[2][0][64] in surv                                                 # and so is the 65-class's


def _reference_yaml_shapes():
    """unbias/configs/code_release/voc07_tta_test.yaml and the detectron2 defaults it inherits, restated as dicts"""
    voc = {"MODEL": {"MASK_ON": False, "ROI_HEADS": {"NUM_CLASSES": 20}},
           "TEST": {"EVAL_PERIOD": 1000, "AUG": {"ENABLED": True, "MIN_SIZES": "(480, 576, 672, 768, 864, 960, 1056, 1152)",
                                                 "MAX_SIZE": 4000, "FLIP": True}},
           "INPUT": {"MIN_SIZE_TEST": 688, "MAX_SIZE_TEST": 4000}}
    plain = {"MODEL": {"ROI_HEADS": {"NUM_CLASSES": 80}}, "TEST": {"AUG": {"ENABLED": True}}}
    return voc, plain


class _Heads:
    padded_detections = False


class _Model:
    training = False
    roi_heads = _Heads()

    def inference(self, *a, **k):
        raise AssertionError("not called")


def test_wrapper_helper_and_config_keys_read_the_reference_shapes():
    from sos_wsod_amd import tta
    from sos_wsod_amd.config import CfgNode, get_cfg
    assert callable(tta.test_with_TTA) and tta.test_with_TTA.__test__ is False
    voc, plain = _reference_yaml_shapes()
    cfg = get_cfg()
    assert cfg.TEST.AUG.MIN_SIZES == (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)        # detectron2/config/defaults.py:592-595
    assert (cfg.TEST.AUG.MAX_SIZE, cfg.TEST.AUG.FLIP, cfg.TEST.AUG.ENABLED, cfg.MODEL.KEYPOINT_ON) == (4000, True, False, False)
    cfg._merge(CfgNode(voc))
    w = tta.GeneralizedRCNNWithTTA(cfg, _Model())
    assert w.tta_mapper.min_sizes == (480, 576, 672, 768, 864, 960, 1056, 1152) and w.tta_mapper.max_size == 4000 and w.tta_mapper.flip
    assert (w.num_classes, w.nms_thresh, w.topk, w.batch_size) == (20, 0.5, 100, 3)
    cfg = get_cfg()
    cfg._merge(CfgNode(plain))
    w = tta.GeneralizedRCNNWithTTA(cfg, _Model(), batch_size=1)
    assert len(w.tta_mapper.min_sizes) == 9 and w.num_classes == 80 and w.batch_size == 1


@pytest.mark.parametrize("key", ["KEYPOINT_ON", "MASK_ON", "LOAD_PROPOSALS"])
def test_wrapper_refuses_what_it_does_not_implement(key):
    from sos_wsod_amd import tta
    from sos_wsod_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL[key] = True
    with pytest.raises(ValueError, match=key):
        tta.GeneralizedRCNNWithTTA(cfg, _Model())


def test_mapper_without_proposals_gives_the_same_views_and_transforms():
    """geometry only (the resize kernel needs a GPU): the no-proposal form is checked on the device in test_gpu_stage3_tta.py"""
    from sos_wsod_amd.tta import DeviceTTAMapper, ViewTransform, view_table
    assert DeviceTTAMapper._shortest_edge(688, 917, 480, 4000) == (480, 640)
    t = [ViewTransform((96, 128), (64, 85), False), ViewTransform((96, 128), (64, 85), True)]
    tab = view_table(t, (96, 128), (75, 100), "cpu").numpy()
    assert tab.shape == (2, 6) and tab[:, 0].tolist() == [0.0, 1.0] and tab[0, 1] == 85
    assert tab[0, 2] == np.float32(128 / 85) and tab[0, 3] == np.float32(96 / 64) and tab[0, 4] == np.float32(100 / 128) and tab[0, 5] == np.float32(75 / 96)
    assert view_table(t, (96, 128), (96, 128), "cpu")[:, 4:].tolist() == [[1.0, 1.0], [1.0, 1.0]]

"""GPU: sw_tta_merge (ops.tta_merge) against tests/golden/tta_merge.npz — the reference's own merged detections — bit for bit, and the
entry's conventions: nothing beyond a count matters, zero tail, `out`, the poisoned count, the limits, run-to-run identical bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_tta_merge_cpu import CASES, edge_case, load_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


def run(ops, c, out=None, **over):
    a = dict(c, **over)
    dev = "cuda:0"
    return ops.tta_merge(torch.from_numpy(a["boxes"]).to(dev), torch.from_numpy(a["scores"]).to(dev), torch.from_numpy(a["classes"]).to(dev),
                         torch.from_numpy(a["counts"]).to(dev), torch.from_numpy(a["view_tab"]).to(dev), int(a["hw"][0]), int(a["hw"][1]),
                         float(a["nms"]), int(a["topk"]), int(a["K"]), out=out)


def assert_equals_fixture(ops, got, c):
    cnt, boxes, scores, classes, src = got
    n = len(c["exp_scores"])
    assert ops.tta_merge_count(cnt) == n
    assert np.array_equal(src.cpu().numpy()[:n], c["exp_src"])
    assert np.array_equal(classes.cpu().numpy()[:n], c["exp_classes"])
    assert np.array_equal(scores.cpu().numpy()[:n].view(np.uint32), c["exp_scores"].view(np.uint32))
    assert np.array_equal(boxes.cpu().numpy()[:n].view(np.uint32), c["exp_boxes"].view(np.uint32))
    for t in (boxes, scores, classes, src):                                                    # rows beyond the count are zero
        assert not t[n:].any()


@pytest.mark.parametrize("name", CASES)
def test_tta_merge_equals_the_reference(ops, golden_dir, name):
    c = load_case(golden_dir, name)
    assert_equals_fixture(ops, run(ops, c), c)


def test_rows_beyond_the_count_never_matter(ops, golden_dir):
    c = load_case(golden_dir, "c3")
    b, s = c["boxes"].copy(), c["scores"].copy()
    for v, n in enumerate(c["counts"]):
        b[v, n:] = np.nan; s[v, n:] = 1.0
    assert_equals_fixture(ops, run(ops, c, boxes=b, scores=s), c)


def test_preallocated_out_keeps_its_tail_and_two_launches_agree(ops, golden_dir):
    c = load_case(golden_dir, "c4")
    n, topk = len(c["exp_scores"]), int(c["topk"])
    assert 0 < n < topk
    first = run(ops, c)
    dev = "cuda:0"
    out = (torch.full((1,), 77, dtype=torch.int32, device=dev), torch.full((topk, 4), -5.0, device=dev), torch.full((topk,), -5.0, device=dev),
           torch.full((topk,), 77, dtype=torch.int32, device=dev), torch.full((topk,), 77, dtype=torch.int32, device=dev))
    got = run(ops, c, out=out)
    assert all(g is o for g, o in zip(got, out)) and int(got[0].item()) == n
    for g, f, sentinel in zip(got[1:], first[1:], (-5.0, -5.0, 77, 77)):
        assert torch.equal(g[:n], f[:n]) and bool((g[n:] == sentinel).all())                   # only the first count rows are written
    c3 = load_case(golden_dir, "c3")
    a, b = run(ops, c3), run(ops, c3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_bad_count_and_limits_raise(ops, golden_dir):
    c = load_case(golden_dir, "c4")
    bad = c["counts"].copy(); bad[2] = c["scores"].shape[1] + 1
    got = run(ops, c, counts=bad)
    with pytest.raises(ValueError):
        ops.tta_merge_count(got[0])
    assert not got[2].any()                                                                    # nothing else written
    bad[2] = -1
    with pytest.raises(ValueError):
        ops.tta_merge_count(run(ops, c, counts=bad)[0])
    dev = "cuda:0"
    V, T = 1, 2049
    args = (torch.zeros(V, T, 4, device=dev), torch.zeros(V, T, device=dev), torch.zeros(V, T, dtype=torch.int32, device=dev),
            torch.zeros(V, dtype=torch.int32, device=dev), torch.ones(V, 6, device=dev))
    with pytest.raises(ValueError):
        ops.tta_merge(*args, 100, 100, 0.5, 100, 20)
    ok = tuple(t[:, :2048].contiguous() if t.dim() > 1 and t.shape[1] == T else t for t in args)
    with pytest.raises(ValueError):
        ops.tta_merge(*ok, 100, 100, 0.5, 100, 1025)
    assert ops.tta_merge_count(ops.tta_merge(*ok, 100, 100, 0.5, 100, 1024)[0]) == 0           # at both limits, every count 0


@pytest.mark.parametrize("name", ["negative_nms", "chunk_edges"])
def test_edge_case_equals_the_restatement(ops, name):
    """negative_nms: the plain `iou > thresh` of a threshold below zero, empty boxes included; chunk_edges: classes of 63, 64, 65 and 129
    candidates through the wave-per-class resolver (test_tta_merge_cpu asserts what each case reaches).  Count, source rows, classes, score
    bits and box bits, every element"""
    c, want = edge_case(name)
    cnt, boxes, scores, classes, src = run(ops, c)
    assert ops.tta_merge_count(cnt) == int(want["count"][0])
    assert np.array_equal(src.cpu().numpy(), want["src"])
    assert np.array_equal(classes.cpu().numpy(), want["classes"])
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), want["scores"].view(np.uint32))
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), want["boxes"].view(np.uint32))


def test_one_class_at_the_row_limit(ops):
    """V * T = 2048 rows of ONE class (one wave resolves 32 chunks), heavy overlap, against the NumPy restatement"""
    from tta_merge_ref import tta_merge_ref
    rng = np.random.RandomState(3)
    V, T = 16, 128
    x0, y0 = rng.uniform(0, 400, (V, T)), rng.uniform(0, 300, (V, T))
    b = np.stack([x0, y0, x0 + rng.uniform(40, 120, (V, T)), y0 + rng.uniform(40, 120, (V, T))], -1).astype(np.float32)
    s = rng.permutation(np.linspace(0.01, 0.99, V * T)).reshape(V, T).astype(np.float32)
    tab = np.tile(np.array([[0, 500, 1, 1, 1, 1]], np.float32), (V, 1)); tab[1::2, 0] = 1
    c = dict(boxes=b, scores=s, classes=np.zeros((V, T), np.int32), counts=np.full(V, T, np.int32), view_tab=tab, hw=np.array([375, 500]),
             nms=0.5, topk=300, K=1)
    want = tta_merge_ref(b, s, c["classes"], c["counts"], tab, 375, 500, 0.5, 300, 1)
    cnt, boxes, scores, classes, src = run(ops, c)
    n = int(want["count"][0])
    assert ops.tta_merge_count(cnt) == n and 60 < n
    assert np.array_equal(src.cpu().numpy(), want["src"]) and np.array_equal(boxes.cpu().numpy().view(np.uint32), want["boxes"].view(np.uint32))
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), want["scores"].view(np.uint32))

"""GPU: sw_detect_postprocess against tests/detect_ref.py (the reference's clip / filter / batched_nms / top-k tail in float32 NumPy, pinned
by test_detect_ref_cpu.py) — count, rows, classes, score bits and box bits, no tolerance and no excluded element (+0.0 and -0.0 are one
score).  Every case runs twice, each run compared with the reference on its own: ops.detect_postprocess (the full workspace: classes of
256 candidates or more take the mask form, C = det_mask_kernel + det_resolve_kernel) and a direct call with
sw_detect_workspace_bytes(0, K, topk) bytes (det_class_nms_kernel alone: A, its chunked LDS form, or B, its one-box-at-a-time loop).
Before each run the form every class takes is worked out from the reference's candidate counts and asserted, so no case can drift to
another form unnoticed.  det_maxcoord_kernel and det_merge_kernel run in every call; the class_offset and topk_tie_cut cases are the
ones that depend on them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as D  # noqa: E402
import test_detect_ref_cpu as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope="module")
def lib():
    from sos_wsod_amd._lib import lib
    return lib


def workspace_bytes(lib, c, full):
    """the two workspace sizes, and that detect_ref's restatement of them (which `route` rests on) is the entry's"""
    R, K = c["scores"].shape[0], c["scores"].shape[1] - 1
    base, both = int(lib.sw_detect_workspace_bytes(0, K, c["topk"])), int(lib.sw_detect_workspace_bytes(R, K, c["topk"]))
    assert base == D.base_bytes(K, c["topk"]) and both - base == D.mask_bytes(R, K)
    return both if full else base


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                               # a copy: the shared inputs are read-only


def direct(lib, c, nbytes, scores=None, boxes=None, out=None, ws=None):
    R, K = c["scores"].shape[0], c["scores"].shape[1] - 1
    topk = c["topk"]
    scores = dev(c["scores"]) if scores is None else scores
    boxes = dev(c["boxes"]) if boxes is None else boxes
    if out is None:
        out = (torch.zeros(1, device=DEV, dtype=torch.int32), torch.zeros(max(topk, 1), 4, device=DEV), torch.zeros(max(topk, 1), device=DEV),
               torch.zeros(max(topk, 1), device=DEV, dtype=torch.int32), torch.zeros(max(topk, 1), device=DEV, dtype=torch.int32))
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8) if ws is None else ws
    rc = lib.sw_detect_postprocess(R, K, scores.data_ptr(), boxes.data_ptr(), c["H"], c["W"], c["thr"], c["nms"], topk, *(o.data_ptr() for o in out),
                                   ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def to_host(got):
    cnt, boxes, scores, classes, rows = (g.cpu().numpy() for g in got)
    return int(cnt[0]), boxes, scores, classes, rows


def assert_same(got, ref, what):
    n = got[0]
    assert n == ref.count, (what, "count", n, ref.count)
    for name, g, r in (("rows", got[4], ref.rows), ("classes", got[3], ref.classes)):
        bad = np.nonzero(g[:n] != r[:n])[0]
        assert not len(bad), (what, name, "first difference at", int(bad[0]), int(g[bad[0]]), int(r[bad[0]]))
    assert D.same(got, ref), (what, "score or box bits")


def run_both(ops, lib, c, ref, reached=None):
    """the case through the full workspace and through the per-class one, each against the reference; -> the two host results"""
    assert C.check_conditions(c, ref)
    results = []
    scores, boxes = dev(c["scores"]), dev(c["boxes"])
    for full in (True, False):
        nbytes = workspace_bytes(lib, c, full)
        f = C.forms(c, ref, full)                                              # from the reference's nv[c], R and the workspace size
        if "forms" in c:
            assert f == c["forms"][1 if full else 0]
        assert "C" not in f or (full and nbytes > D.base_bytes(len(f), c["topk"]))
        if reached is not None:
            reached.update(f)
        if full:
            got = ops.detect_postprocess(scores, boxes, c["H"], c["W"], c["thr"], c["nms"], c["topk"])
        else:
            rc, got = direct(lib, c, nbytes, scores, boxes)
            assert rc == 0
        got = to_host(got)
        assert_same(got, ref, "forms " + f)
        results.append(got)
    return results


EDGE_CASES = [n for n in C.CASES]


@pytest.mark.parametrize("name", EDGE_CASES)
def test_equals_the_reference(ops, lib, name):
    """every constructed case of test_detect_ref_cpu.CASES: the A -> B boundaries at R 64 / 256 / 257 with classes of 0, 1, 63, 64, 65,
    128, 129 candidates; the mask boundary (255 | 256, 257, 320, 321) and R = 255; a class past the resolver's 4096-row LDS window; more
    than 4096 mask tiles; the row limit R = 16384 (NB = 256); the top-k cuts; IoU exactly at the threshold; the class offset's float32
    rounding; nms_thresh < 0; negative / -inf / at-threshold / signed-zero scores; clipped, empty and duplicate boxes"""
    c, ref = C.case(name)
    full, per = run_both(ops, lib, c, ref)
    assert D.same(full, per)


def test_limits(lib):
    c, _ = C.case("boundary_R64")
    K = c["scores"].shape[1] - 1
    sent = lambda: (torch.full((1,), 77, device=DEV, dtype=torch.int32), torch.full((8, 4), -5.0, device=DEV), torch.full((8,), -5.0, device=DEV),  # noqa: E731
                    torch.full((8,), 77, device=DEV, dtype=torch.int32), torch.full((8,), 77, device=DEV, dtype=torch.int32))
    untouched = lambda out: all(bool((o == v).all()) for o, v in zip(out, (77, -5.0, -5.0, 77, 77)))  # noqa: E731
    # R = 16385, K * topk = 16385 and topk = 0: refused before anything is launched or written
    big = dict(scores=np.zeros((16385, 2), np.float32), boxes=np.zeros((16385, 4), np.float32), H=10, W=10, thr=0.5, nms=0.5, topk=8)
    for bad in (big, dict(big, scores=big["scores"][:16], boxes=big["boxes"][:16], topk=16385), dict(c, topk=0),
                dict(scores=np.zeros((16, 6), np.float32), boxes=np.zeros((16, 20), np.float32), H=10, W=10, thr=0.5, nms=0.5, topk=3277)):
        out = sent()
        rc, _ = direct(lib, bad, 1 << 20, out=out)
        assert rc == -6 and untouched(out)
    ok = dict(big, scores=big["scores"][:16384], boxes=big["boxes"][:16384], topk=16384)      # the limits themselves are accepted
    rc, out = direct(lib, ok, int(lib.sw_detect_workspace_bytes(16384, 1, 16384)))
    assert rc == 0 and int(out[0].item()) == 0                                                 # (no score above 0.5)
    # R = 0: count 0, nothing else written
    out = sent()
    rc, _ = direct(lib, dict(c, scores=c["scores"][:0], boxes=c["boxes"][:0], topk=8), int(lib.sw_detect_workspace_bytes(0, K, 8)), out=out)
    assert rc == 0 and int(out[0].item()) == 0
    out[0].fill_(77)
    assert untouched(out)


@pytest.mark.parametrize("full", [True, False])
def test_footprint(lib, full):
    """outputs and workspace carved out of larger sentinel-filled buffers: only the first `count` rows of each output change, no byte outside
    the declared workspace changes, two runs give the same bits"""
    c, ref = C.case("mask_R400")
    assert C.forms(c, ref, full) == c["forms"][1 if full else 0]
    topk, n, nbytes = c["topk"], ref.count, workspace_bytes(lib, c, full)
    assert 0 < n < topk
    PAD = 64                                                                   # elements around each output
    WPAD = 4096                                                                # bytes around the workspace (keeps its 256-byte alignment)
    runs = []
    for _ in range(2):
        bufs = (torch.full((2 * PAD + 1,), 77, device=DEV, dtype=torch.int32), torch.full((2 * PAD + topk, 4), -5.0, device=DEV),
                torch.full((2 * PAD + topk,), -5.0, device=DEV), torch.full((2 * PAD + topk,), 77, device=DEV, dtype=torch.int32),
                torch.full((2 * PAD + topk,), 77, device=DEV, dtype=torch.int32))
        out = tuple(b[PAD:b.shape[0] - PAD] for b in bufs)
        wbuf = torch.full((nbytes + 2 * WPAD,), 0xA5, device=DEV, dtype=torch.uint8)
        rc, _ = direct(lib, c, nbytes, out=out, ws=wbuf[WPAD:WPAD + nbytes])
        assert rc == 0
        got = to_host(out)
        assert_same(got, ref, "footprint")
        for b, o, v in zip(bufs[1:], out[1:], (-5.0, -5.0, 77, 77)):
            assert bool((b[:PAD] == v).all()) and bool((b[b.shape[0] - PAD:] == v).all()) and bool((o[n:] == v).all())
        assert bool((bufs[0][:PAD] == 77).all()) and bool((bufs[0][PAD + 1:] == 77).all())
        assert bool((wbuf[:WPAD] == 0xA5).all()) and bool((wbuf[WPAD + nbytes:] == 0xA5).all())
        runs.append(tuple(o.clone() for o in out))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_seeded_fuzz(ops, lib):
    """40 seeded shapes: R in 1..700, K in {1, 3, 20, 80}, scores sometimes in steps of 1/50, thresholds, box sizes and top-k vary; each
    of the three forms is reached in five iterations or more (test_detect_ref_cpu.test_fuzz_seed_reaches_every_form chose the seed)"""
    reached = {"A": 0, "B": 0, "C": 0}
    for i in range(C.FUZZ_N):
        c = C.fuzz_case(i)
        seen = set()
        run_both(ops, lib, c, C.ref_of(c), seen)
        for f in seen:
            reached[f] += 1
    assert min(reached.values()) >= 5, reached

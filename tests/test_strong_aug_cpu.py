"""CPU: the numpy restatement of the Stage-3 strong augmentation (tests/strong_aug_ref.py) equals Pillow, the committed fixtures
equal the restatement, the recipe draws follow the reference's distributions, and the two-crop mapper's box / label side."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import strong_aug_ref as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "strong_aug.npz")
FACTORS = (0.6, 0.75, 0.83, 1.0, 1.17, 1.25, 1.4)
SIZES = ((61, 83, 1), (5, 83, 2), (83, 5, 5), (97, 131, 3))


def _pil():
    pytest.importorskip("PIL")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_strong_aug_golden as M
    return M


@pytest.mark.parametrize("op", ["brightness", "contrast", "saturation"])
def test_blends_equal_pillow(op):
    M = _pil()
    for h, w, tag in SIZES:
        src = R.make_image(h, w, tag)
        for f in FACTORS:
            assert np.array_equal(getattr(R, op)(src, f), M.pil_recipe(src, {"order": [op], op: f})), (op, h, w, f)


def test_l_conversion_equals_pillow():
    M = _pil()
    from PIL import Image
    src = np.ascontiguousarray(R.all_colours()[::7, ::5])
    assert np.array_equal(R.lum(src), np.array(Image.fromarray(src, "RGB").convert("L")))
    assert np.array_equal(R.grayscale(src), M.pil_recipe(src, {"grayscale": True}))


def test_hsv_round_trip_equals_pillow_over_all_colours():
    _pil()
    from PIL import Image
    src = R.all_colours()
    assert int((R.rgb2hsv(src) != np.array(Image.fromarray(src, "RGB").convert("HSV"))).sum()) == 0
    assert int((R.hsv2rgb(src) != np.array(Image.fromarray(src, "HSV").convert("RGB"))).sum()) == 0


@pytest.mark.parametrize("f", [-0.1, -0.05, -0.004, 0.0, 0.004, 0.037, 0.1])
def test_hue_shift_equals_pillow(f):
    M = _pil()
    from PIL import Image
    src = np.ascontiguousarray(R.all_colours()[::3, ::5])
    assert np.array_equal(R.hue(src, f), np.array(M.pil_hue(Image.fromarray(src, "RGB"), f)))


# sigma = 2.4495 and 2.45 sit on either side of the l = 1 -> 2 boundary (12 sigma^2 / 3 + 1 = 25); 2.45, 3.0 and 3.4 give r = 2, the
# largest radius the kernels accept
@pytest.mark.parametrize("sigma", [0.1, 0.3, 0.45, 0.9, 1.0, 1.37, 1.73, 2.0, 2.4495, 2.45, 3.0, 3.4])
def test_gaussian_blur_equals_pillow(sigma):
    M = _pil()
    for h, w, tag in SIZES:
        src = R.make_image(h, w, tag)
        assert np.array_equal(R.gaussian_blur(src, sigma), M.pil_recipe(src, {"blur_sigma": sigma})), (sigma, h, w)


def test_blur_weights_match_the_library():
    import ctypes
    import sos_wsod_amd._lib as L
    r, ww, fw = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
    for sigma in (0.1, 0.45, 0.9, 1.37, 2.0, 2.4495, 2.45, 3.0):
        assert L.lib.sw_gaussian_blur_weights(sigma, ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw)) == 0
        assert (r.value, ww.value, fw.value) == R.blur_weights(sigma), sigma
    assert L.lib.sw_gaussian_blur_weights(0.0, ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw)) == -1
    assert L.lib.sw_gaussian_blur_weights(8.0, ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw)) == -6


def test_fixtures_equal_the_restatement():
    cases, version = R.load_cases(GOLDEN)
    assert version and len(cases) >= 80
    key, src = None, None
    for c in cases:
        h, w = c["hw"]
        if key != (h, w, c["tag"]):
            key, src = (h, w, c["tag"]), R.all_colours() if c["tag"] < 0 else R.make_image(h, w, c["tag"])
        got = R.apply_recipe(src, c["recipe"])
        if "out" in c:
            assert np.array_equal(got, c["out"]), c["name"]
        else:
            sha, rows = R.digest(got)
            assert np.array_equal(rows, c["rows"]) and sha == c["sha"], c["name"]


def test_fixture_generator_reproduces_the_fixture_with_this_pillow():
    M = _pil()
    cases, _ = R.load_cases(GOLDEN)
    for c in cases:
        if "out" in c:
            assert np.array_equal(M.pil_recipe(R.make_image(*c["hw"], c["tag"]), c["recipe"]), c["out"]), c["name"]


# ------------------------------------------------------------------------------------------------ erased bytes
def test_splitmix64_published_vector():
    assert int(R.splitmix64(0)) == 0xE220A8397B1DCDAF                     # the first output of the published generator seeded 0
    assert int(R.splitmix64(np.array([0, 0], np.uint64))[1]) == 0xE220A8397B1DCDAF


def test_erase_band_holds_a_float32_evaluation_and_few_bytes_are_undecided():
    """4e6 hashed counters: the formula evaluated in float32 by numpy (another libm than the device's, the same error class)
    lands inside the band of the float64 value everywhere, so its byte is one of (lo, hi); at most 0.2 % of the counters are
    undecided (a condition: the GPU tests allow the same share)"""
    seed, key, e, c, h, w = 2 ** 63 + 5, 12345, 1, 2, 2000, 2000
    v, band = R.erase_values(seed, key, e, c, h, w)
    lo, hi = R.erase_bytes(seed, key, e, c, h, w)
    u1, arg = R.erase_uniforms(seed, key, e, c, h, w)
    assert u1.dtype == np.float32 and arg.dtype == np.float32 and float(u1.min()) > 0 and float(u1.max()) <= 1
    v32 = np.float32(255) * (np.sqrt(np.float32(-2) * np.log(u1)) * np.cos(arg))
    assert v32.dtype == np.float32
    err = np.abs(v32.astype(np.float64) - v)
    b32 = (np.trunc(v32).astype(np.int64) & 255).astype(np.uint8)
    b64 = (np.trunc(v).astype(np.int64) & 255).astype(np.uint8)
    undecided = float((lo != hi).mean())
    print(f"erase band: {v.size} counters, {int((b32 != b64).sum())} float32/float64 byte disagreements, largest relative error "
          f"{float((err / np.maximum(1.0, np.abs(v))).max()):.3g} of {2.0 ** -20:.3g} allowed, undecided share {undecided:.3g}")
    assert v.size == 4 * 10 ** 6 and (err <= band).all()
    assert ((b32 == lo) | (b32 == hi)).all()
    assert ((b64 == lo) | (b64 == hi)).all()
    assert undecided <= 0.002
    assert abs(float(v.mean())) < 1.0 and abs(float(v.std()) - 255.0) < 1.0      # 255 n, n ~ N(0, 1): 4 sigma of the mean is 0.51


def test_apply_erasings_order_and_mask():
    img = np.full((20, 30, 3), 128, np.uint8)
    rects = ((2, 3, 10, 12), (5, 6, 10, 12), None)
    out, decided, alt = R.apply_erasings(img, rects, 7, 9)
    lo0, _ = R.erase_bytes(7, 9, 0, 1, 10, 12)
    lo1, _ = R.erase_bytes(7, 9, 1, 1, 10, 12)
    assert np.array_equal(out[5:15, 6:18, 1], lo1)                             # the later erasing wins where they overlap
    assert np.array_equal(out[2:5, 3:15, 1], lo0[:3]) and np.array_equal(out[5:12, 3:6, 1], lo0[3:, :3])
    m = R.rect_mask((20, 30), rects)
    assert (out[~m] == 128).all() and decided[~m].all() and np.array_equal(alt[decided], out[decided])
    assert not np.array_equal(R.erase_bytes(7, 9, 0, 0, 10, 12)[0], R.erase_bytes(7, 9, 0, 0, 12, 10)[0].T)   # (dy, dx) is ordered


@pytest.mark.parametrize("op", ["contrast", "saturation"])
def test_blend_inputs_are_sensitive_to_a_fused_multiply_add(op):
    """the (x, d, f) triples of tests/test_gpu_strong_aug_edges.py's blend cases: for each op at least one triple gives another byte
    when d + f * (x - d) is evaluated as one fused multiply-add, so a build with contraction on cannot pass the GPU test"""
    differing = {}
    if op == "contrast":
        for d in R.CONTRAST_DEGENERATES:
            src = R.contrast_ramp_image(d)
            for f in R.BLEND_FACTORS:
                differing[(d, f)] = int((R.blend(np.uint8(d), src, f) != R.blend_fused(np.uint8(d), src, f)).sum())
    else:
        src = R.saturation_pairs_image()
        L = R.lum(src)[..., None]
        for f in R.BLEND_FACTORS:
            differing[f] = int((R.blend(L, src, f) != R.blend_fused(L, src, f)).sum())
    print(op, "bytes that a fused multiply-add changes:", differing)
    assert sum(differing.values()) >= 1, differing


# ------------------------------------------------------------------------------------------------ recipe draws
def test_recipe_draws_are_keyed():
    from sos_wsod_amd.strong_aug import StrongAugmentation
    a, b = StrongAugmentation(7), StrongAugmentation(7)
    assert a.draw(5, 2, (800, 1216)) == b.draw(5, 2, (800, 1216))
    assert a.draw(5, 2, (800, 1216)) != a.draw(6, 2, (800, 1216))
    assert a.draw(5, 2, (800, 1216)) != a.draw(5, 3, (800, 1216))
    assert a.draw(5, 2, (800, 1216)) != StrongAugmentation(8).draw(5, 2, (800, 1216))
    off = StrongAugmentation(7, is_train=False).draw(5, 2, (800, 1216))
    assert off.order == () and not off.grayscale and off.blur_sigma is None and off.rects == (None, None, None)


def _attempt_failure_rate(H, W, scale, ratio, n=200000):
    """P(one attempt of RandomErasing.get_params is rejected), by a seeded Monte-Carlo run of the rule itself"""
    rng = np.random.default_rng(12345)
    area = H * W * rng.uniform(scale[0], scale[1], n)
    ar = np.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1]), n))
    h, w = np.rint(np.sqrt(area * ar)), np.rint(np.sqrt(area / ar))
    return float(np.mean(~((h < H) & (w < W))))


def test_recipe_draw_statistics():
    from sos_wsod_amd.strong_aug import ERASINGS, JITTER_OPS, StrongAugmentation
    H, W, N = 800, 1216, 20000
    aug = StrongAugmentation(3)
    rs = [aug.draw(i, 0, (H, W)) for i in range(N)]

    def within(count, p, what):
        assert abs(count / N - p) <= 4 * math.sqrt(p * (1 - p) / N), (what, count / N, p)
    within(sum(bool(r.order) for r in rs), 0.8, "jitter")
    within(sum(r.grayscale for r in rs), 0.2, "grayscale")
    within(sum(r.blur_sigma is not None for r in rs), 0.5, "blur")
    for e, (p, scale, ratio) in enumerate(ERASINGS):
        fail = _attempt_failure_rate(H, W, scale, ratio) ** 10            # all ten attempts rejected
        within(sum(r.rects[e] is not None for r in rs), p * (1 - fail), f"erasing {e}")
        for r in rs:
            if r.rects[e] is None:
                continue
            t, l, h, w = r.rects[e]
            assert 0 < h < H and 0 < w < W and 0 <= t and 0 <= l and t + h <= H and l + w <= W
            # h, w are rounded square roots: each is off by at most 0.5 from the real-valued side
            lo_a, hi_a = (h - 0.5) * (w - 0.5) / (H * W), (h + 0.5) * (w + 0.5) / (H * W)
            assert hi_a >= scale[0] and lo_a <= scale[1], (r.rects[e], scale)
            assert (h + 0.5) / (w - 0.5) >= ratio[0] and (h - 0.5) / (w + 0.5) <= ratio[1], (r.rects[e], ratio)
    orders = {r.order for r in rs if r.order}
    assert len(orders) == 24 and all(sorted(o) == sorted(JITTER_OPS) for o in orders)
    for r in rs:
        if r.order:
            assert 0.6 <= r.brightness <= 1.4 and 0.6 <= r.contrast <= 1.4 and 0.6 <= r.saturation <= 1.4 and -0.1 <= r.hue <= 0.1
        if r.blur_sigma is not None:
            assert 0.1 <= r.blur_sigma <= 2.0


# ------------------------------------------------------------------------------------------------ mapper: box / label side
def _dict(h=100, w=150, index=3):
    return {"image": torch.zeros(3, h, w, dtype=torch.uint8), "index": index, "height": h, "width": w, "file_name": "x.jpg",
            "annotations": [{"bbox": [10, 10, 50, 60], "category_id": 2},
                            {"bbox": [0, 0, 5, 5], "category_id": 1, "iscrowd": 1},
                            {"bbox": [60, 20, 30, 40], "bbox_mode": 1, "category_id": 7},
                            {"bbox": [160, 5, 400, 50], "category_id": 4},                    # empty after the clip
                            {"bbox": [20, 30, 20, 80], "category_id": 5}]}                    # zero width


def test_mapper_boxes_and_labels():
    from sos_wsod_amd.strong_aug import DeviceTwoCropMapper
    m = DeviceTwoCropMapper(min_sizes=(200,), max_size=1000, resize_pixels=False, seed=1)
    d = _dict()
    plain = m(d, draws={"crop": None, "hw": (200, 300), "flip": False})
    flipped = m(d, draws={"crop": None, "hw": (200, 300), "flip": True})
    for strong, weak in (plain, flipped):
        assert strong["instances"] is weak["instances"]
        assert strong["image"].shape == weak["image"].shape == (3, 200, 300)
        assert weak["instances"].image_size == (200, 300)
        assert weak["instances"].gt_classes.tolist() == [2, 7]                               # crowd, clipped-empty and zero-width gone
        assert weak["height"] == 100 and weak["width"] == 150 and weak["file_name"] == "x.jpg" and "annotations" not in weak
    b, bf = plain[1]["instances"].gt_boxes.tensor, flipped[1]["instances"].gt_boxes.tensor
    assert b.dtype == torch.float32 and b.tolist() == [[20, 20, 100, 120], [120, 40, 180, 120]]
    assert bf.tolist() == [[200, 20, 280, 120], [120, 40, 180, 120]]                           # x -> 300 - x, corners re-sorted
    cropped = m(d, draws={"crop": (10, 20, 80, 100), "hw": (160, 200), "flip": False})[1]["instances"]
    assert cropped.gt_boxes.tensor.tolist() == [[0, 0, 60, 100], [80, 20, 140, 100]] and cropped.gt_classes.tolist() == [2, 7]


def test_mapper_draws_are_keyed_and_flip_half_the_time():
    from sos_wsod_amd.strong_aug import DeviceTwoCropMapper
    m = DeviceTwoCropMapper(min_sizes=(64, 80, 96), max_size=130, crop=("relative_range", (0.3, 0.3)), resize_pixels=False, seed=5)
    g = [m.draw_geometry(i, 0, (100, 150)) for i in range(2000)]
    assert g[7] == m.draw_geometry(7, 0, (100, 150)) and g[7] != m.draw_geometry(7, 1, (100, 150))
    flips = sum(x["flip"] for x in g)
    assert abs(flips / 2000 - 0.5) <= 4 * math.sqrt(0.25 / 2000)
    assert all(max(x["hw"]) <= 130 and min(x["hw"]) <= 96 for x in g)
    for x in g:
        y0, x0, ch, cw = x["crop"]
        assert 30 <= ch <= 100 and 45 <= cw <= 150 and 0 <= y0 <= 100 - ch and 0 <= x0 <= 150 - cw
    test = DeviceTwoCropMapper(min_sizes=(64,), max_size=130, resize_pixels=False, is_train=False)
    out = test(_dict())
    assert isinstance(out, dict) and "instances" not in out and "annotations" not in out and out["image"].shape == (3, 64, 96)


def test_mapper_refuses_what_it_does_not_support():
    from types import SimpleNamespace as NS
    from sos_wsod_amd.config import get_cfg
    from sos_wsod_amd.strong_aug import DeviceTwoCropMapper
    cfg = get_cfg()
    m = DeviceTwoCropMapper.from_config(cfg, is_train=True, resize_pixels=False)
    assert m.min_sizes == tuple(cfg.INPUT.MIN_SIZE_TRAIN) and m.max_size == cfg.INPUT.MAX_SIZE_TRAIN and m.flip_prob == 0.5
    for key in ("MASK_ON", "KEYPOINT_ON", "LOAD_PROPOSALS"):
        bad = NS(MODEL=NS(**{key: True}), INPUT=cfg.INPUT)
        with pytest.raises(ValueError):
            DeviceTwoCropMapper.from_config(bad, is_train=True)
    with pytest.raises(ValueError):
        m(dict(_dict(), sem_seg_file_name="s.png"))
    with pytest.raises(ValueError):
        m(dict(_dict(), proposal_boxes=[[0, 0, 1, 1]]))
    with pytest.raises(ValueError):
        m({k: v for k, v in _dict().items() if k != "index"})
    with pytest.raises(ValueError):
        m(dict(_dict(), height=99))
    with pytest.raises(RuntimeError):                                   # no CPU pixel path
        DeviceTwoCropMapper(min_sizes=(64,), max_size=130)(_dict())


def test_batches_mirror_the_two_stream_grouping():
    from sos_wsod_amd.strong_aug import DeviceTwoCropMapper, TwoCropBatches
    m = DeviceTwoCropMapper(min_sizes=(64,), max_size=130, resize_pixels=False, seed=2)
    dicts = [{"height": 100, "width": 150 if i % 3 else 80, "annotations": [{"bbox": [5, 5, 60, 70], "category_id": i}]} for i in range(9)]
    loader = lambda d: torch.zeros(3, d["height"], d["width"], dtype=torch.uint8)
    it = iter(TwoCropBatches(m, dicts, dicts, loader, 2, 3, seed=4))
    for _ in range(4):
        lq, lk, uq, uk = next(it)
        assert (len(lq), len(lk), len(uq), len(uk)) == (2, 2, 3, 3)
        for q, k in zip(lq + uq, lk + uk):
            assert q["instances"] is k["instances"] and q["image"].shape == k["image"].shape and q["image"] is not k["image"]
        for group in (lk, uk):                                          # one aspect-ratio group per stream and batch
            assert len({d["width"] > d["height"] for d in group}) == 1
    a = next(iter(TwoCropBatches(m, dicts, dicts, loader, 2, 3, seed=4)))
    b = next(iter(TwoCropBatches(m, dicts, dicts, loader, 2, 3, seed=4)))
    assert [d["instances"].gt_classes.tolist() for d in a[1] + a[3]] == [d["instances"].gt_classes.tolist() for d in b[1] + b[3]]

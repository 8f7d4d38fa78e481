"""GPU: sw_strong_aug_u8 / sw_strong_aug_multi_u8 against the Pillow-made fixtures (tests/golden/strong_aug.npz, written by
tests/golden/make_strong_aug_golden.py): every pixel outside the erased rectangles equals Pillow's, bit for bit; the erased
rectangles' geometry, reproducibility and distribution; batched == per image; the two-crop mapper end to end."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import strong_aug_ref as R  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "strong_aug.npz")


def _recipe(rc, seed=11, key=5):
    from sos_wsod_amd.strong_aug import Recipe
    kw = {k: rc[k] for k in ("brightness", "contrast", "saturation", "hue", "blur_sigma") if k in rc}
    rects = tuple(None if r is None else tuple(r) for r in rc.get("rects", ())) + (None,) * (3 - len(rc.get("rects", ())))
    return Recipe(order=tuple(rc.get("order", ())), grayscale=bool(rc.get("grayscale", False)), rects=rects, seed=seed, key=key, **kw)


def _dev(img_hwc):
    return torch.from_numpy(np.ascontiguousarray(img_hwc.transpose(2, 0, 1))).cuda()


def _host(t):
    return np.ascontiguousarray(t.cpu().numpy().transpose(1, 2, 0))


def _src(c):
    return R.all_colours() if c["tag"] < 0 else R.make_image(c["hw"][0], c["hw"][1], c["tag"])


def test_every_fixture_case_equals_pillow_outside_the_rectangles():
    """each step alone and whole recipes (7 orders with contrast first / in the middle / last, jitter off, grayscale + blur,
    overlapping rectangles, nothing on) at 61 x 83, 5 x 83, 97 x 131 and 800 x 1216; the hue path over all 2^24 colours.
    No tolerance, no excluded pixel."""
    import sos_wsod_amd.ops as ops
    cases, _ = R.load_cases(GOLDEN)
    assert len({tuple(c["hw"]) for c in cases}) >= 4 and any(c["hw"] == [800, 1216] for c in cases)
    assert len({tuple(c["recipe"]["order"]) for c in cases if len(c["recipe"].get("order", ())) == 4}) >= 6
    key, src, dev = None, None, None
    for c in cases:
        if key != (tuple(c["hw"]), c["tag"]):
            key, src = (tuple(c["hw"]), c["tag"]), _src(c)
            dev = _dev(src)
        got = _host(ops.strong_augment_u8(dev, _recipe(c["recipe"])))
        if c["name"].endswith("/nothing"):
            assert np.array_equal(got, src), c["name"]
        rects = c["recipe"].get("rects")
        if "out" in c:
            want = c["out"]
        elif rects:
            # a larger image with rectangles: the fixture keeps the digest of Pillow's un-erased result; the pixels outside the
            # rectangles are compared with the restatement, after checking that the restatement has that digest
            want = R.apply_recipe(src, c["recipe"])
            assert R.digest(want)[0] == c["sha"], c["name"]
        else:
            sha, rows = R.digest(got)
            wrong = np.nonzero(rows != c["rows"])[0]
            assert wrong.size == 0 and sha == c["sha"], (c["name"], f"{wrong.size} rows differ, first {wrong[:5].tolist()}")
            continue
        bad = (got != want).any(-1) & ~R.rect_mask(tuple(c["hw"]), rects)
        assert not bad.any(), (c["name"], int(bad.sum()), np.argwhere(bad)[:5].tolist())


def test_erasing_geometry_reproducibility_and_seed():
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd.strong_aug import Recipe
    H, W = 203, 317
    grey = torch.full((3, H, W), 128, dtype=torch.uint8, device="cuda")
    rects = ((10, 12, 80, 130), (60, 100, 90, 101), (5, 200, 150, 33))                  # overlapping
    rc = Recipe(rects=rects, seed=3, key=9)
    a, b = ops.strong_augment_u8(grey, rc), ops.strong_augment_u8(grey, rc)
    assert torch.equal(a, b)
    mask = torch.from_numpy(R.rect_mask((H, W), rects)).cuda()
    changed = a != grey
    assert not (changed & ~mask).any()                                                # a subset of the rectangles
    assert float(changed[:, mask].float().mean()) >= 0.99
    for other in (Recipe(rects=rects, seed=4, key=9), Recipe(rects=rects, seed=3, key=10)):
        c = ops.strong_augment_u8(grey, other)
        assert not ((c != grey) & ~mask).any()
        assert float((a != c)[:, mask].float().mean()) >= 0.99
    # a sample depends on its erasing, channel and offset inside the rectangle only: the same rectangle moved keeps its bytes
    one = ops.strong_augment_u8(grey, Recipe(rects=((10, 12, 80, 130), None, None), seed=3, key=9))
    moved = ops.strong_augment_u8(grey, Recipe(rects=((33, 47, 80, 130), None, None), seed=3, key=9))
    assert torch.equal(one[:, 10:90, 12:142], moved[:, 33:113, 47:177])
    # the batched call: same bytes for the same key
    multi = ops.strong_augment_multi_u8([grey, grey], [rc, Recipe(rects=rects, seed=4, key=9)])
    assert torch.equal(multi[0], a)


def test_erased_bytes_follow_the_wrapped_truncated_normal():
    """chi-square over 16 bins of 16 byte values against wrap(trunc(255 n)), n ~ N(0, 1), at p > 1e-4 (15 degrees of freedom:
    statistic < 44.26); 3 x 700 x 1000 = 2.1e6 samples, fixed seed"""
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd.strong_aug import Recipe
    H, W = 720, 1040
    grey = torch.full((3, H, W), 128, dtype=torch.uint8, device="cuda")
    out = ops.strong_augment_u8(grey, Recipe(rects=((10, 20, 700, 1000), None, None), seed=2024, key=1))
    samples = out[:, 10:710, 20:1020].reshape(-1).cpu().numpy()
    n = samples.size
    assert n >= 10 ** 6
    # trunc(255 n) = k: k >= 1 is n in [k/255, (k+1)/255), k <= -1 is n in ((k-1)/255, k/255], k = 0 is (-1/255, 1/255)
    cdf = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))
    p = np.zeros(256)
    for k in range(-2600, 2601):
        if k > 0:
            pk = cdf((k + 1) / 255.0) - cdf(k / 255.0)
        elif k < 0:
            pk = cdf(k / 255.0) - cdf((k - 1) / 255.0)
        else:
            pk = cdf(1 / 255.0) - cdf(-1 / 255.0)
        p[k % 256] += pk
    assert abs(p.sum() - 1.0) < 1e-9
    expect = p.reshape(16, 16).sum(1) * n
    counts = np.bincount(samples, minlength=256).reshape(16, 16).sum(1)
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"erased bytes: chi-square {chi2:.2f} over 16 bins, {n} samples")
    assert chi2 < 44.26, chi2


def test_batched_equals_per_image():
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd.strong_aug import Recipe, StrongAugmentation
    sizes = ((61, 83), (200, 304), (97, 131), (333, 517), (5, 83), (128, 2100))
    imgs = [_dev(R.make_image(h, w, 20 + i)) for i, (h, w) in enumerate(sizes)]
    aug = StrongAugmentation(5)
    recipes = [Recipe(order=("hue", "contrast", "brightness", "saturation"), brightness=1.2, contrast=0.7, saturation=1.3, hue=0.05,
                      blur_sigma=2.0, rects=((3, 4, 30, 40), (20, 30, 25, 20), None), seed=1, key=1),
               Recipe(order=("saturation", "brightness", "hue", "contrast"), brightness=0.8, contrast=1.4, saturation=0.6, hue=-0.1,
                      grayscale=True, rects=((100, 100, 50, 120), None, (0, 0, 199, 10)), seed=1, key=2),
               Recipe(blur_sigma=0.3, seed=1, key=3),
               aug.draw(3, 0, sizes[3]),
               Recipe(order=("contrast",), contrast=1.3, blur_sigma=1.1, seed=1, key=4),
               Recipe(order=("brightness", "contrast", "saturation", "hue"), brightness=1.4, contrast=0.6, saturation=1.4, hue=0.1,
                      blur_sigma=1.5, rects=((1, 1000, 100, 1050), None, None), seed=1, key=5)]
    single = [ops.strong_augment_u8(im, rc) for im, rc in zip(imgs, recipes)]
    multi = ops.strong_augment_multi_u8(imgs, recipes)
    for i, (a, b) in enumerate(zip(single, multi)):
        assert torch.equal(a, b), (i, sizes[i])
    for i, (im, rc, got) in enumerate(zip(imgs, recipes, single)):         # and both equal the restatement outside the rectangles
        d = {"order": rc.order, "brightness": rc.brightness, "contrast": rc.contrast, "saturation": rc.saturation, "hue": rc.hue,
             "grayscale": rc.grayscale, "blur_sigma": rc.blur_sigma}
        want = R.apply_recipe(_host(im), d)
        bad = (_host(got) != want).any(-1) & ~R.rect_mask(sizes[i], rc.rects)
        assert not bad.any(), (i, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    with pytest.raises(RuntimeError):
        ops.strong_augment_u8(imgs[0].cpu(), recipes[0])


def test_two_crop_mapper_on_the_device():
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd.resize import resize_bilinear_u8
    from sos_wsod_amd.strong_aug import DeviceTwoCropMapper
    m = DeviceTwoCropMapper(min_sizes=(96, 128), max_size=200, crop=("relative_range", (0.6, 0.6)), seed=3)
    img = _dev(R.make_image(150, 203, 31))
    d = {"image": img, "index": 4, "height": 150, "width": 203, "annotations": [{"bbox": [20, 30, 120, 140], "category_id": 3}]}
    seen = set()
    for visit in range(8):
        strong, weak = m(d, visit=visit)
        g = m.last_draws
        y0, x0, ch, cw = g["crop"]
        r, rf = resize_bilinear_u8(img[:, y0:y0 + ch, x0:x0 + cw], g["hw"], with_flip=True)
        assert torch.equal(weak["image"], rf if g["flip"] else r)
        assert torch.equal(strong["image"], ops.strong_augment_u8(weak["image"], m.last_recipe))
        assert strong["image"].shape == weak["image"].shape == (3,) + tuple(g["hw"]) and strong["instances"] is weak["instances"]
        assert weak["instances"].image_size == tuple(g["hw"]) and weak["instances"].gt_boxes.tensor.is_cuda
        seen.add(g["flip"])
    assert seen == {True, False}
    assert torch.equal(m(d, visit=2)[0]["image"], m(d, visit=2)[0]["image"])


def test_batches_feed_the_semi_supervised_step():
    """TwoCropBatches -> SemiSupStep.run_step on the small detector of tests/test_gpu_stage3.py: finite losses in burn-in and past it"""
    from oracle import frcnn_oracle as FO                                  # parameters and images of the small detector only
    from sos_wsod_amd.frcnn import TwoStagePseudoLabGeneralizedRCNN
    from sos_wsod_amd.semisup import SemiSupStep
    from sos_wsod_amd.strong_aug import DeviceTwoCropMapper, TwoCropBatches
    K = 20
    P = FO.make_params(K, tag="s3s", head_scale=14.0)

    def model():
        mm = TwoStagePseudoLabGeneralizedRCNN(num_classes=K, compute_dtype=torch.float32).cuda()
        sd = mm.state_dict()
        with torch.no_grad():
            for k, v in P.items():
                sd[k].copy_(torch.from_numpy(v))
        return mm.train()
    student, teacher = model(), model()
    opt = torch.optim.SGD([p for p in student.parameters() if p.requires_grad], lr=1e-5, momentum=0.9)
    step = SemiSupStep(student, teacher, opt, burn_up_step=1, ema_keep_rate=0.9996, bbox_threshold=0.7, unsup_loss_weight=2.0)
    sizes = [(120, 160), (128, 150), (110, 170), (140, 180)]
    dicts = []
    for i, (h, w) in enumerate(sizes):
        b, c = FO.make_gt(h, w, 2, K, f"tc{i}")
        dicts.append({"height": h, "width": w, "tag": f"tc{i}",
                      "annotations": [{"bbox": [float(v) for v in bb], "category_id": int(cc)} for bb, cc in zip(b, c)]})
    loader = lambda d: torch.from_numpy(FO.make_image(d["height"], d["width"], d["tag"])).cuda()
    mapper = DeviceTwoCropMapper(min_sizes=(96, 112), max_size=160, seed=1)
    it = iter(TwoCropBatches(mapper, dicts, dicts, loader, 2, 2, seed=1))
    for i in range(2):
        data = next(it)
        assert [len(x) for x in data] == [2, 2, 2, 2]
        for q, k in zip(data[0] + data[2], data[1] + data[3]):
            assert q["image"].is_cuda and q["image"].dtype == torch.uint8 and q["image"].shape == k["image"].shape
        record, loss_dict = step.run_step(data)
        torch.cuda.synchronize()
        vals = {k: float(v) for k, v in loss_dict.items()}
        assert vals and all(math.isfinite(v) for v in vals.values()), vals
        assert ("loss_cls_pseudo" in vals) == (i == 1), (i, sorted(vals))

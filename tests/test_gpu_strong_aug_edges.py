"""GPU: the five kernels of csrc/augment.hip at their tile, word, alignment and erasing edges, against tests/strong_aug_ref.py
(proven equal to Pillow by tests/test_strong_aug_cpu.py).  Every comparison is exact (array_equal).  The one exception is an
erased byte whose float64 value lies within the float32 error band of a truncation step (strong_aug_ref.erase_bytes: "undecided"):
it may be either neighbour, and the share of such bytes is capped at 0.2 %.

The edges in the code: aug_blur_h_kernel's tile of BH_TW = 1024 columns behind BH_PAD = 12; aug_blur_v_kernel's tile of
BV_TW = 256 x BV_TH = 64 behind BLUR_HALO = 9 rows; the 4-pixel word of load4 / store4 and its `aligned4(...) && (n & 3) == 0`
switch; blur radius 2, which uses the halo of 9 in full."""
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

SEEDS = (0, 1, 2 ** 63 + 5, 2 ** 64 - 1)                                  # seeds and keys: both halves of the 64 bits in use
UNDECIDED_CAP = 0.002
ORDER = ("brightness", "contrast", "hue", "saturation")                  # contrast in the middle: aug_lsum_kernel recomputes brightness
JITTER = dict(order=ORDER, brightness=1.2, contrast=0.7, saturation=1.3, hue=0.05)


def _ops():
    import sos_wsod_amd.ops as ops
    return ops


def _recipe(**kw):
    from sos_wsod_amd.strong_aug import Recipe
    rects = tuple(kw.pop("rects", ()))
    return Recipe(rects=rects + (None,) * (3 - len(rects)), **kw)


def _as_dict(rc):
    return {"order": rc.order, "brightness": rc.brightness, "contrast": rc.contrast, "saturation": rc.saturation, "hue": rc.hue,
            "grayscale": rc.grayscale, "blur_sigma": rc.blur_sigma}


def _dev(img_hwc):
    return torch.from_numpy(np.ascontiguousarray(img_hwc.transpose(2, 0, 1))).cuda()


def _host(t):
    return np.ascontiguousarray(t.cpu().numpy().transpose(1, 2, 0))


def _rects(H, W):
    """the rectangles of the erasing tests, for an image of at least 67 x 90"""
    return {"tall": (5, 7, 33, 20),                                      # not square: a dy / dx swap changes its bytes
            "over": (15, 12, 25, 40),                                    # overlaps `tall`
            "corner": (H - 20, W - 30, 20, 30),                          # touches the bottom-right corner
            "dot": (3, 3, 1, 1),
            "whole": (0, 0, H, W),
            "lastcol": (8, W - 13, 11, 13)}                              # ends at the last column


def _rect_sets(H, W, lastcol=False):
    r = _rects(H, W)
    sets = [(r["tall"], r["over"], r["corner"]), (r["whole"], r["dot"], r["tall"])]
    return sets + [(r["lastcol"], None, r["dot"])] if lastcol else sets


def _check_erased(got, base, rc, what):
    """got == base outside the recipe's rectangles, == the restated bytes inside (either neighbour where undecided)
    -> (undecided bytes, erased bytes)"""
    want, decided, alt = R.apply_erasings(base, rc.rects, rc.seed, rc.key)
    wrong = decided & (got != want)
    assert not wrong.any(), (what, "decided bytes differ", int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
    stray = ~decided & (got != want) & (got != alt)
    assert not stray.any(), (what, "an undecided byte is neither neighbour", int(stray.sum()), np.argwhere(stray)[:5].tolist())
    return int((~decided).sum()), 3 * int(R.rect_mask(got.shape[:2], rc.rects).sum())


# ------------------------------------------------------------------------------------------------ a. erased bytes, point path
def test_erased_bytes_equal_the_restatement_on_the_point_path():
    """aug_point_kernel's bytes against strong_aug_ref.apply_erasings on a grey 70 x 90 image: a non-square rectangle, one
    overlapping it, one in the bottom-right corner, a 1 x 1 and a whole-image rectangle, for every pairing of the seeds and keys
    0, 1, 2^63 + 5 and 2^64 - 1, single and batched.  Decided bytes are equal, undecided ones are one of the two neighbours.
    Seen on an MI355X: 152 undecided bytes of 394320 erased ones, a share of 3.9e-4 against the cap of 2e-3 (numpy's float32
    evaluation of the formula gives 3.9e-4 over 4e6 counters in tests/test_strong_aug_cpu.py)."""
    ops = _ops()
    H, W = 70, 90
    grey_h = np.full((H, W, 3), 128, np.uint8)
    grey = _dev(grey_h)
    undecided = erased = 0
    recipes, singles = [], []
    for seed in SEEDS:
        for key in SEEDS:
            for rects in _rect_sets(H, W):
                rc = _recipe(rects=rects, seed=seed, key=key)
                got = ops.strong_augment_u8(grey, rc)
                u, n = _check_erased(_host(got), grey_h, rc, (seed, key, rects))
                undecided, erased = undecided + u, erased + n
                recipes.append(rc)
                singles.append(got)
    print(f"erased bytes, point path: {undecided} undecided of {erased} ({undecided / erased:.3g})")
    assert erased >= 3 * 10 ** 5 and undecided <= UNDECIDED_CAP * erased
    multi = ops.strong_augment_multi_u8([grey] * len(recipes), recipes)           # the record array's hand-over of seed and key
    for rc, a, b in zip(recipes, singles, multi):
        assert torch.equal(a, b), (rc.seed, rc.key, rc.rects)


def test_channels_and_erasings_draw_different_bytes():
    """one geometry in each of the three erasing slots, three channels each: nine different byte fields (independent near-uniform
    bytes agree at about 1 position in 256), each equal to the restatement for its (erasing, channel)"""
    ops = _ops()
    H, W = 70, 90
    grey_h = np.full((H, W, 3), 128, np.uint8)
    grey = _dev(grey_h)
    t, l, h, w = rect = _rects(H, W)["tall"]
    fields = {}
    for e in range(3):
        rc = _recipe(rects=tuple(rect if k == e else None for k in range(3)), seed=2 ** 63 + 5, key=1)
        got = _host(ops.strong_augment_u8(grey, rc))
        _check_erased(got, grey_h, rc, ("slot", e))
        for c in range(3):
            fields[(e, c)] = got[t:t + h, l:l + w, c]
    keys = sorted(fields)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert float((fields[a] != fields[b]).mean()) >= 0.9, (a, b)


# ------------------------------------------------------------------------------------------------ b. blur path erases the same bytes
@pytest.mark.parametrize("hw", [(67, 259), (130, 1030)])
def test_blur_path_erases_the_same_bytes_as_the_point_path(hw):
    """aug_blur_v_kernel writes the erased bytes with its own coordinates (gy, x + b): inside the rectangles its output is
    byte-identical to aug_point_kernel's for the same recipe without blur; outside, each equals the restatement.  W % 4 != 0 with
    a rectangle ending at the last column; single and batched."""
    ops = _ops()
    H, W = hw
    assert W % 4 != 0
    src_h = R.make_image(H, W, 41)
    src = _dev(src_h)
    jittered = R.apply_recipe(src_h, JITTER)
    imgs, recipes, singles = [], [], []
    for si, rects in enumerate(_rect_sets(H, W, lastcol=True)):
        mask = R.rect_mask(hw, rects)
        plain = _recipe(rects=rects, seed=2 ** 63 + 5, key=2 ** 64 - 1 - si, **JITTER)
        point = ops.strong_augment_u8(src, plain)
        point_h = _host(point)
        _check_erased(point_h, jittered, plain, (hw, si, "point"))
        imgs.append(src), recipes.append(plain), singles.append(point)
        for sigma in (1.73, 3.0):                                                   # r = 1 and r = 2
            blurred = _recipe(rects=rects, seed=plain.seed, key=plain.key, blur_sigma=sigma, **JITTER)
            got = ops.strong_augment_u8(src, blurred)
            got_h = _host(got)
            assert np.array_equal(got_h[mask], point_h[mask]), (hw, si, sigma, int((got_h[mask] != point_h[mask]).sum()))
            want = R.gaussian_blur(jittered, sigma)
            bad = (got_h != want).any(-1) & ~mask
            assert not bad.any(), (hw, si, sigma, int(bad.sum()), np.argwhere(bad)[:5].tolist())
            imgs.append(src), recipes.append(blurred), singles.append(got)
    multi = ops.strong_augment_multi_u8(imgs, recipes)
    for i, (a, b) in enumerate(zip(singles, multi)):
        assert torch.equal(a, b), (hw, i, recipes[i].blur_sigma)


# ------------------------------------------------------------------------------------------------ c. tile and word edges
EDGE_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (130, 3),                   # below a word, one row, one column
              (63, 255), (64, 256), (65, 257), (73, 260), (74, 256),              # aug_blur_v_kernel's 64 x 256 tile and its halo of 9
              (9, 1023), (9, 1024), (10, 1025), (9, 1036), (9, 1037), (5, 2049)]  # aug_blur_h_kernel's 1024 tile and its pad of 12
# r = 0 (outer weight small), 0 (outer weight as large as the inner: the pass reaches one sample out), 1, 2 (outer weight nearly
# nothing: the first sigma of that radius), 2 (outer weight as large as the inner: reaches 3 samples per pass, 9 in all)
EDGE_SIGMAS = (0.3, 1.37, 1.73, 2.45, 3.4)


@pytest.mark.parametrize("hw", EDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_and_word_edges(hw):
    """the full recipe (four jitter ops with contrast in the middle, blur, one rectangle where the image has room) at every blur
    radius, and its no-blur twin, at sizes on either side of every tile, halo and word edge"""
    ops = _ops()
    H, W = hw
    assert [R.blur_weights(s)[0] for s in EDGE_SIGMAS] == [0, 0, 1, 2, 2]
    src_h = R.make_image(H, W, 50 + (H * 31 + W) % 17)
    src = _dev(src_h)
    rects = ((H // 4, W // 3, H // 2, W // 2),) if H >= 4 and W >= 4 else ()
    jittered = R.apply_recipe(src_h, JITTER)
    for sigma in (None,) + EDGE_SIGMAS:
        rc = _recipe(rects=rects, seed=1, key=2 ** 63 + 5, blur_sigma=sigma, **JITTER)
        want = jittered if sigma is None else R.gaussian_blur(jittered, sigma)
        _check_erased(_host(ops.strong_augment_u8(src, rc)), want, rc, (hw, sigma))


def test_blur_radius_three_is_refused_and_writes_nothing():
    ops = _ops()
    assert R.blur_weights(3.5)[0] == 3 and R.blur_weights(3.4)[0] == 2
    src = _dev(R.make_image(20, 40, 3))
    out = torch.full_like(src, 0x5A)
    with pytest.raises(RuntimeError):
        ops.strong_augment_u8(src, _recipe(blur_sigma=3.5), out=out)
    outs = [torch.full_like(src, 0x5A), torch.full_like(src, 0x5A)]
    with pytest.raises(RuntimeError):
        ops.strong_augment_multi_u8([src, src], [_recipe(blur_sigma=1.0), _recipe(blur_sigma=3.5)], outs=outs)
    torch.cuda.synchronize()
    for o in [out] + outs:
        assert bool((o == 0x5A).all())
    assert torch.equal(ops.strong_augment_u8(src, _recipe(blur_sigma=3.4), out=out), _dev(R.gaussian_blur(_host(src), 3.4)))


# ------------------------------------------------------------------------------------------------ d. unaligned bases, stray writes
CANARY = 64


def _carve(n_bytes, offset, fill):
    """a uint8 buffer of CANARY + offset + n_bytes + CANARY + 8 bytes filled with a pattern; -> (buffer, first byte of the carved part)"""
    buf = torch.empty(CANARY + offset + n_bytes + CANARY + 8, dtype=torch.uint8, device="cuda")
    buf.copy_(torch.from_numpy(((np.arange(buf.numel()) * 37 + fill) % 251).astype(np.uint8)))
    assert buf.data_ptr() % 4 == 0
    return buf, CANARY + offset


@pytest.mark.parametrize("hw", [(64, 256), (12, 1028), (3, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_unaligned_bases_and_stray_writes(hw):
    """img and out as contiguous views at byte offsets 0..3 of larger buffers, chosen independently: all four pixel kernels take
    the byte-wise branch of load4 / store4 although H * W is a multiple of 4 (the first two sizes); the bytes around `out` stay"""
    ops = _ops()
    H, W = hw
    n = 3 * H * W
    src_h = R.make_image(H, W, 61)
    planar = torch.from_numpy(np.ascontiguousarray(src_h.transpose(2, 0, 1))).reshape(-1).cuda()
    recipes = [_recipe(seed=1, key=2, **JITTER), _recipe(seed=1, key=2, blur_sigma=3.0, **JITTER)]
    wants = [torch.from_numpy(np.ascontiguousarray(R.apply_recipe(src_h, _as_dict(rc)).transpose(2, 0, 1))).cuda() for rc in recipes]
    for oi in range(4):
        ibuf, i0 = _carve(n, oi, 11)
        ibuf[i0:i0 + n] = planar
        img = ibuf[i0:i0 + n].view(3, H, W)
        assert img.is_contiguous() and img.data_ptr() % 4 == oi
        for oo in range(4):
            for rc, want in zip(recipes, wants):
                obuf, o0 = _carve(n, oo, 99)
                before = obuf.clone()
                out = obuf[o0:o0 + n].view(3, H, W)
                assert out.data_ptr() % 4 == oo
                ret = ops.strong_augment_u8(img, rc, out=out)
                assert ret.data_ptr() == out.data_ptr()
                assert torch.equal(out, want), (hw, oi, oo, rc.blur_sigma, int((out != want).sum()))
                assert torch.equal(obuf[:o0], before[:o0]) and torch.equal(obuf[o0 + n:], before[o0 + n:]), (hw, oi, oo, rc.blur_sigma)
        assert torch.equal(img.reshape(-1), planar)                                          # the input is only read


# ------------------------------------------------------------------------------------------------ e. contrast tie, blend arithmetic
TIE_HW = (37, 54)                                                        # 1998 pixels: even, no multiple of 4, two blocks of aug_lsum_kernel


def _tie_image(k, below, brightness=None):
    """a grey image whose mean L, after `brightness` if given, is exactly k + 1/2 (below: one pixel less, k + 1/2 - 1 / count):
    half the pixels at k, half at k + 1, interleaved"""
    H, W = TIE_HW
    lo, hi = k, k + 1
    if brightness is not None:                                           # source values that brightness maps onto k and k + 1
        image_of = R.brightness(np.arange(256, dtype=np.uint8), brightness)
        lo, hi = int(np.nonzero(image_of == k)[0][0]), int(np.nonzero(image_of == k + 1)[0][0])
    flat = np.full(H * W, lo, np.uint8)
    flat[1::2] = hi
    if below:
        flat[H * W - 1] = lo
    img = np.repeat(flat.reshape(H, W, 1), 3, -1)
    seen = img if brightness is None else R.brightness(img, brightness)
    total = int(R.lum(seen).astype(np.int64).sum())
    assert 2 * total == (2 * k + 1) * H * W - (2 if below else 0)         # sum / count == k + 1/2 (- 1 / count) exactly
    return img


def test_contrast_mean_rounds_a_tie_up_and_one_count_below_it_down():
    """int(sum / count + 0.5) on the device: a mean of exactly k + 1/2 gives the degenerate k + 1, one count less gives k, for
    k = 0, 127, 254; with contrast first and with brightness in front of it (aug_lsum_kernel recomputes it); single and batched"""
    ops = _ops()
    imgs, recipes, wants = [], [], []
    for k, bright in ((0, 0.75), (127, 0.75), (254, 1.3)):
        for order, b in ((("contrast", "saturation"), None), (("brightness", "contrast"), bright)):
            pair = []
            for below in (False, True):
                img = _tie_image(k, below, b)
                rc = _recipe(order=order, brightness=b or 1.0, contrast=0.0, saturation=1.2, seed=1, key=1)
                seen = img if b is None else R.brightness(img, b)
                assert R.contrast_mean(seen) == (k if below else k + 1), (k, order, below)
                want = R.apply_recipe(img, _as_dict(rc))                  # contrast factor 0: every pixel becomes the degenerate
                assert (want == (k if below else k + 1)).all()
                pair.append(want)
                imgs.append(_dev(img)), recipes.append(rc), wants.append(want)
            assert not np.array_equal(pair[0], pair[1])
    multi = ops.strong_augment_multi_u8(imgs, recipes)
    for i, (im, rc, want) in enumerate(zip(imgs, recipes, wants)):
        got = _host(ops.strong_augment_u8(im, rc))
        assert np.array_equal(got, want), (i, rc.order, int(got[0, 0, 0]), int(want[0, 0, 0]))
        assert np.array_equal(_host(multi[i]), want), (i, rc.order, "batched")
        rb = _recipe(order=rc.order, brightness=rc.brightness, contrast=0.0, saturation=1.2, blur_sigma=1.0)
        got = _host(ops.strong_augment_u8(im, rb))                        # aug_blur_h_kernel reads the same sum
        assert np.array_equal(got, R.gaussian_blur(want, 1.0)), (i, rc.order, "blur", int(got[0, 0, 0]), int(want[0, 0, 0]))


@pytest.mark.parametrize("d", R.CONTRAST_DEGENERATES)
def test_contrast_blend_is_two_roundings(d):
    """every x in 0..255 blended with the degenerate d at the factors that tests/test_strong_aug_cpu.py proves sensitive to a
    fused multiply-add: `d + f * (x - d)` must round the product and the sum separately, as Pillow does"""
    ops = _ops()
    src_h = R.contrast_ramp_image(d)
    src = _dev(src_h)
    for f in R.BLEND_FACTORS:
        got = _host(ops.strong_augment_u8(src, _recipe(order=("contrast",), contrast=f)))
        want = R.contrast(src_h, f)
        assert np.array_equal(got, want), (d, f, np.argwhere(got != want)[:5].tolist())


def test_saturation_blend_is_two_roundings():
    ops = _ops()
    src_h = R.saturation_pairs_image()
    src = _dev(src_h)
    for f in R.BLEND_FACTORS:
        got = _host(ops.strong_augment_u8(src, _recipe(order=("saturation",), saturation=f)))
        want = R.saturation(src_h, f)
        assert np.array_equal(got, want), (f, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())


# ------------------------------------------------------------------------------------------------ f. batch shape edges
def test_batch_of_unlike_images_and_stages():
    """one batched call whose union of stages (contrast sum, point, blur) is on for images that use none or one of them: a 1 x 1
    image, a recipe that changes nothing, contrast only, blur only across both blur tiles, and blur + contrast + erasing"""
    ops = _ops()
    sizes = ((1, 1), (33, 47), (41, 300), (65, 1025), (10, 2049))
    recipes = [_recipe(order=("hue", "brightness"), brightness=1.3, hue=-0.1),
               _recipe(seed=5, key=6),
               _recipe(order=("contrast",), contrast=1.4),
               _recipe(blur_sigma=3.4),
               _recipe(order=("saturation", "contrast"), contrast=0.6, saturation=1.4, blur_sigma=2.45,
                       rects=((2, 1000, 6, 100), None, (0, 2040, 10, 9)), seed=2 ** 64 - 1, key=2 ** 63 + 5)]
    hosts = [R.make_image(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    imgs = [_dev(x) for x in hosts]
    multi = ops.strong_augment_multi_u8(imgs, recipes)
    for i, (im, x, rc) in enumerate(zip(imgs, hosts, recipes)):
        assert torch.equal(multi[i], ops.strong_augment_u8(im, rc)), (i, sizes[i])
        _check_erased(_host(multi[i]), R.apply_recipe(x, _as_dict(rc)), rc, (i, sizes[i]))
    assert torch.equal(multi[1], imgs[1])                                                     # nothing on: the input comes back
    for im, rc in zip(imgs, recipes):                                                         # n = 1 through the batched entry
        assert torch.equal(ops.strong_augment_multi_u8([im], [rc])[0], ops.strong_augment_u8(im, rc))

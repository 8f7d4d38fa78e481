"""numpy restatement of Pillow's arithmetic behind the Stage-3 strong augmentation (the CHECKER of sw_strong_aug_u8, not the product).
Images are HWC uint8 arrays here, as Pillow hands them out.  tests/test_strong_aug_cpu.py proves each function equal to Pillow."""
import hashlib
import json
import zlib

import numpy as np

f32, f64 = np.float32, np.float64


def make_image(h, w, tag=0):
    """deterministic test image from integer arithmetic only (the same bytes on every machine): the left part hashed noise, the
    right part smooth ramps with saturated and grey stripes"""
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    out = np.zeros((h, w, 3), np.uint8)
    for c in range(3):
        z = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ np.uint64((c + 1) * 83492791 + tag * 2654435761)
        z = (z ^ (z >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
        z = (z ^ (z >> np.uint64(12))) * np.uint64(0x297A2D39) & np.uint64(0xFFFFFFFF)
        noise = ((z ^ (z >> np.uint64(15))) & np.uint64(255)).astype(np.uint8)
        ramp = ((x * np.uint64(3 + c) + y * np.uint64(5 - c) + np.uint64(40 * c + 7 * tag)) % np.uint64(256)).astype(np.uint8)
        out[..., c] = np.where(x < np.uint64(w // 2), noise, ramp)
    stripe = (y % np.uint64(11)) == np.uint64(3)
    out[stripe & (x >= np.uint64(w // 2))] = out[stripe & (x >= np.uint64(w // 2))][:, :1]          # grey rows: r = g = b
    return out


def lum(img):
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """Image.blend(degenerate, image, f) on uint8 arrays (deg broadcastable)"""
    d = np.asarray(deg).astype(f32)
    t = d + f32(f) * (img.astype(f32) - d)
    return np.clip(t, f32(0), f32(255)).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros((), np.uint8), img, f)


def contrast_mean(img):
    L = lum(img)
    return int(int(L.astype(np.int64).sum()) / L.size + 0.5)


def contrast(img, f):
    return blend(np.uint8(contrast_mean(img)), img, f)


def saturation(img, f):
    return blend(lum(img)[..., None], img, f)


def grayscale(img):
    return np.repeat(lum(img)[..., None], 3, -1)


def rgb2hsv(rgb):
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    with np.errstate(all="ignore"):
        cr = (mx - mn).astype(f32)
        s = cr / mx.astype(f32)
        rc, gc, bc = (mx - r).astype(f32) / cr, (mx - g).astype(f32) / cr, (mx - b).astype(f32) / cr
        h = np.where(r == mx, (bc - gc).astype(f64), np.where(g == mx, 2.0 + rc.astype(f64) - bc, 4.0 + gc.astype(f64) - rc)).astype(f32)
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        uh = np.clip((h.astype(f64) * 255.0).astype(np.int32), 0, 255)
        us = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    z = mx == mn
    return np.stack([np.where(z, 0, uh), np.where(z, 0, us), mx], -1).astype(np.uint8)


def hsv2rgb(hsv):
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    hf = h.astype(f64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int32)
    f = (hf - i.astype(f64)).astype(f32).astype(f64)
    fs = (s.astype(f64) / 255.0).astype(f32).astype(f64)
    vf = v.astype(f64)
    rnd = lambda t: np.clip(np.floor(t + 0.5), 0, 255).astype(np.uint8)           # C round() of a non-negative double
    p, q, t = rnd(vf * (1.0 - fs)), rnd(vf * (1.0 - fs * f)), rnd(vf * (1.0 - fs * (1.0 - f)))
    i6 = i % 6
    out = np.stack([np.choose(i6, [v, q, p, p, t, v]), np.choose(i6, [t, v, v, q, p, p]), np.choose(i6, [p, p, t, v, v, q])], -1)
    z = s == 0
    out[z] = np.stack([v, v, v], -1)[z]
    return out


def hue_shift_of(factor):
    return int(factor * 255) % 256


def hue(img, factor):
    hsv = rgb2hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift_of(factor)) & 255
    return hsv2rgb(hsv)


def blur_weights(sigma):
    """Pillow's _gaussian_blur_radius for three passes (float32 variables; sqrt and floor in double), then ImagingLineBoxBlur8's
    integer weights: -> (r, ww, fw)"""
    s = f32(sigma)
    s2 = f32(s * s / f32(3))
    L = f32(np.sqrt(12.0 * float(s2) + 1.0))
    l = f32(np.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    a = f32(a / f32(f32(6) * f32(s2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    R = f32(l + a)
    r = int(R)
    ww = int(np.uint32(f32(1 << 24) / (R * f32(2) + f32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def _box_pass(x, r, ww, fw):
    """one box pass along the last axis, edges replicated"""
    n = x.shape[-1]
    idx = np.arange(n)
    at = lambda k: x[..., np.clip(idx + k, 0, n - 1)].astype(np.uint64)
    s = sum(at(k) for k in range(-r, r + 1))
    return ((np.uint64(ww) * s + np.uint64(fw) * (at(-r - 1) + at(r + 1)) + np.uint64(1 << 23)) >> np.uint64(24)).astype(np.uint8)


def gaussian_blur(img, sigma):
    r, ww, fw = blur_weights(sigma)
    x = np.moveaxis(img, -1, 0)                                  # (3, H, W)
    for _ in range(3):
        x = _box_pass(x, r, ww, fw)
    x = np.swapaxes(x, 1, 2)
    for _ in range(3):
        x = _box_pass(x, r, ww, fw)
    return np.ascontiguousarray(np.moveaxis(np.swapaxes(x, 1, 2), 0, -1))


_JITTER = {"brightness": brightness, "contrast": contrast, "saturation": saturation, "hue": hue}


def apply_recipe(img, recipe):
    """the whole recipe without the erasings (recipe: dict with the fields of strong_aug.Recipe)"""
    for op in recipe.get("order", ()):
        img = _JITTER[op](img, recipe[op])
    if recipe.get("grayscale"):
        img = grayscale(img)
    if recipe.get("blur_sigma") is not None:
        img = gaussian_blur(img, recipe["blur_sigma"])
    return img


def rect_mask(hw, rects):
    m = np.zeros(hw, bool)
    for rc in rects or ():
        if rc is not None and rc[2] > 0:
            t, l, h, w = rc
            m[t:t + h, l:l + w] = True
    return m


# ------------------------------------------------------------------------------------------------ erased bytes
_U64 = np.uint64


def splitmix64(x):
    """one splitmix64 output of state x (uint64 scalar or array, arithmetic modulo 2^64)"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, _U64) + _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
        return x ^ (x >> _U64(31))


def erase_uniforms(seed, key, e, c, h, w):
    """-> (u1, arg) float32 (h, w): the kernel's hash chain over (seed, key, e * 4 + c, dy << 32 | dx), the first uniform in (0, 1]
    and the cosine argument float32(2 pi) * u2.  The 24-bit integers, `+ 1` and the scaling by 2^-24 are exact in float32; the
    product with 2 pi is one correctly rounded float32 operation: both are the same bits on every IEEE machine."""
    dy, dx = np.meshgrid(np.arange(h, dtype=_U64), np.arange(w, dtype=_U64), indexing="ij")
    s = splitmix64(_U64(int(seed) & 0xFFFFFFFFFFFFFFFF))
    s = splitmix64(s ^ _U64(int(key) & 0xFFFFFFFFFFFFFFFF))
    s = splitmix64(s ^ _U64(e * 4 + c))
    s = splitmix64(s ^ ((dy << _U64(32)) | dx))
    u1 = ((s >> _U64(40)).astype(f32) + f32(1)) * f32(1.0 / 16777216.0)
    u2 = ((s >> _U64(16)) & _U64(0xFFFFFF)).astype(f32) * f32(1.0 / 16777216.0)
    return u1, f32(6.283185307179586) * u2


def erase_values(seed, key, e, c, h, w):
    """-> (v, band) float64 (h, w): v = 255 n at every offset (dy, dx) of erasing e, channel c, where the kernel computes
    `255.0f * (sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2))` in float32; band bounds |kernel's float - v|.

    u1 and the cosine argument are taken in float32 exactly as the kernel has them (erase_uniforms); log, sqrt and cos are then
    evaluated in float64, whose own error (2^-52) does not count.  The kernel's float32 chain adds, relative to its result:
    logf <= 1 ulp, so sqrt(-2 log u1) <= 1/2 ulp from it (the factor -2 is exact) + 1/2 ulp of the correctly rounded sqrtf
    = 1 ulp; cosf <= 2 ulp; the product of the two and the product with 255 correctly rounded, 1/2 ulp each: 4 ulp in all, and an
    ulp is at most 2^-23 of the value it belongs to, so the relative error of 255 n is at most 2^-21.  The two library
    figures (1 ulp, 2 ulp) are the vendor's documented bounds, not this project's measurements, so the band is doubled:
    band = 2^-20 * max(1, |v|)  (below |v| = 1 the truncation is 0 either way and the floor of 2^-20 only keeps the band from
    vanishing at v = 0)."""
    u1, arg = erase_uniforms(seed, key, e, c, h, w)
    v = 255.0 * (np.sqrt(-2.0 * np.log(u1.astype(f64))) * np.cos(arg.astype(f64)))
    return v, 2.0 ** -20 * np.maximum(1.0, np.abs(v))


def erase_bytes(seed, key, e, c, h, w):
    """-> (lo, hi) uint8 (h, w): trunc(v - band) & 255 and trunc(v + band) & 255 (truncation toward zero, wrapped modulo 256: torch's
    CPU float -> uint8).  A sample is decided where they agree; elsewhere the kernel may give either."""
    v, band = erase_values(seed, key, e, c, h, w)
    wrap = lambda t: (np.trunc(t).astype(np.int64) & 255).astype(np.uint8)
    return wrap(v - band), wrap(v + band)


def apply_erasings(img, rects, seed, key):
    """the three erasings in turn on an HWC uint8 image (a later rectangle overwrites an earlier one)
    -> (out, decided, alt): decided (H, W, 3) bool; where it is False the byte may also be alt"""
    out, alt = img.copy(), img.copy()
    decided = np.ones(img.shape, bool)
    for e, rc in enumerate(rects or ()):
        if rc is None or rc[2] <= 0:
            continue
        t, l, h, w = rc
        for c in range(3):
            lo, hi = erase_bytes(seed, key, e, c, h, w)
            out[t:t + h, l:l + w, c], alt[t:t + h, l:l + w, c], decided[t:t + h, l:l + w, c] = lo, hi, lo == hi
    return out, decided, alt


# ------------------------------------------------------------------------------------------------ blend inputs
BLEND_FACTORS = (0.0, 0.1, 1.0 / 3.0, 0.6, 0.72, 1.0, 1.31, 1.4, 2.0)
CONTRAST_DEGENERATES = (0, 1, 127, 128, 254, 255)


def contrast_ramp_image(d, rows=300):
    """(rows, 256, 3) grey image: row 0 the ramp 0..255, every other row the constant d, which puts int(mean(L) + 0.5) at d
    (the ramp moves the mean by less than 0.43): contrast then blends every x in 0..255 with the degenerate d"""
    img = np.full((rows, 256, 3), d, np.uint8)
    img[0] = np.arange(256, dtype=np.uint8)[:, None]
    assert contrast_mean(img) == d
    return img


def saturation_pairs_image():
    """a subsample of all 2^24 colours: 586 x 820 pixels whose (lum, channel value) pairs are what saturation blends"""
    return np.ascontiguousarray(all_colours()[::7, ::5])


def blend_fused(deg, img, f):
    """`blend` as a build with floating-point contraction would compute it: d + f * (x - d) as ONE fused multiply-add, i.e. the exact
    f * (x - d) + d rounded once to float32 (f a float32, x - d an integer below 2^8: product and sum are exact in float64)"""
    d = np.asarray(deg).astype(f64)
    t = (f64(f32(f)) * (img.astype(f64) - d) + d).astype(f32)
    return np.clip(t, f32(0), f32(255)).astype(np.uint8)


def digest(img):
    """(sha256 hex of the bytes, crc32 per row) of an HWC uint8 image: what the fixtures keep of images too large to commit"""
    img = np.ascontiguousarray(img)
    return hashlib.sha256(img.tobytes()).hexdigest(), np.array([zlib.crc32(row.tobytes()) for row in img], np.uint32)


def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def load_cases(path):
    """-> list of dicts {name, hw, tag, recipe, and either "out" (pixels) or "sha" + "rows"}"""
    g = np.load(path, allow_pickle=False)
    cases = json.loads(str(g["cases"]))
    for c in cases:
        n = c["name"]
        if n + "/out" in g:
            c["out"] = g[n + "/out"]
        else:
            c["sha"], c["rows"] = str(g[n + "/sha"]), g[n + "/rows"]
    return cases, str(g["pil_version"])

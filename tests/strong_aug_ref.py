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

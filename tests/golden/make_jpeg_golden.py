"""Generate tests/golden/jpeg_*.npz from Pillow itself: synthetic images encoded with Pillow and decoded again with Pillow, the
call chain behind the reference's detection_utils.read_image (detectron2/data/detection_utils.py:119-185): Image.open, the EXIF
orientation, convert("RGB").  Data only; no dataset is needed.

    python tests/golden/make_jpeg_golden.py

Every file holds, per case, `<case>/jpeg` (the JPEG bytes as uint8) and `<case>/rgb` (Pillow's (H, W, 3) pixels after
ImageOps.exif_transpose and convert("RGB")).  jpeg_uncovered.npz holds the files the package's own decoder leaves to Pillow.
"""
import io
import os

import numpy as np
from PIL import Image, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
# partial MCUs, a chroma plane one sample wide, odd downsampled sizes; 3..6: both sides of libjpeg's "downsampled width > 2" rule
SIZES = [(1, 1), (3, 3), (4, 4), (5, 6), (7, 5), (8, 8), (9, 9), (15, 17), (16, 16), (17, 15), (33, 31), (64, 48)]
SAMPLINGS = {"444": 0, "422": 1, "420": 2}


def lowpass(rng, h, w, c=3, amp=1.0):
    """smooth colour blobs plus fine noise: chroma that varies from sample to sample, so the upsampling filter matters"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w, c))
    for k in range(c):
        for _ in range(4):
            fy, fx, ph = rng.uniform(0.05, 0.9), rng.uniform(0.05, 0.9), rng.uniform(0, 6.28)
            out[:, :, k] += np.sin(yy * fy + xx * fx + ph) * 45
        out[:, :, k] += 128 + rng.uniform(-30, 30)
    out += rng.normal(0, 12 * amp, out.shape)
    return np.clip(out, 0, 255).astype(np.uint8)


def pillow_pixels(data):
    im = Image.open(io.BytesIO(data))
    im = ImageOps.exif_transpose(im)
    return np.asarray(im.convert("RGB"))


def encode(arr, **kw):
    mode = "L" if arr.ndim == 2 else {3: "RGB", 4: "CMYK"}[arr.shape[2]]
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def exif_bytes(orientation):
    ex = Image.Exif()
    ex[274] = orientation
    return ex.tobytes()


def main():
    rng = np.random.RandomState(20)
    groups = {"sizes": {}, "content": {}, "streams": {}, "exif": {}, "uncovered": {}}

    for w, h in SIZES:
        img = lowpass(rng, h, w)
        for name, sub in SAMPLINGS.items():
            groups["sizes"][f"{name}_{w}x{h}"] = encode(img, quality=88, subsampling=sub)
        groups["sizes"][f"gray_{w}x{h}"] = encode(img[:, :, 0], quality=88)

    h, w = 48, 64
    noise = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    binary = np.repeat((rng.randint(0, 2, (h, w, 1)) * 255).astype(np.uint8), 3, 2)
    binary[:, :, 2] = 255 - binary[:, :, 2]
    yy, xx = np.mgrid[0:h, 0:w]
    grad = np.stack([xx * 4, yy * 5, (xx + yy) * 2], -1).clip(0, 255).astype(np.uint8)
    stripes = np.repeat((((xx % 2) * 255).astype(np.uint8))[:, :, None], 3, 2)
    stripes_rows = np.repeat((((yy % 2) * 255).astype(np.uint8))[:, :, None], 3, 2)
    flat = np.empty((h, w, 3), np.uint8)
    flat[:] = (200, 40, 90)
    for name, sub in SAMPLINGS.items():
        groups["content"][f"noise_q100_{name}"] = encode(noise, quality=100, subsampling=sub)       # 16-bit codes, ZRL, every coefficient alive
        groups["content"][f"clip_q50_{name}"] = encode(binary, quality=50, subsampling=sub)         # IDCT well beyond [0, 255] on both sides
        groups["content"][f"flat_{name}"] = encode(flat, quality=90, subsampling=sub)               # DC only
        groups["content"][f"grad_q30_{name}"] = encode(grad, quality=30, subsampling=sub)
        groups["content"][f"grad_q75_{name}"] = encode(grad, quality=75, subsampling=sub)
        groups["content"][f"stripes_{name}"] = encode(stripes, quality=95, subsampling=sub)
        groups["content"][f"stripes_rows_{name}"] = encode(stripes_rows, quality=95, subsampling=sub)
    groups["content"]["noise_q100_gray"] = encode(noise[:, :, 1], quality=100)
    groups["content"]["flat_gray"] = encode(flat[:, :, 0], quality=90)

    img = lowpass(rng, 31, 45)
    qt = [[min(255, 3 + (i * 7) % 50) for i in range(64)], [min(255, 9 + (i * 11) % 70) for i in range(64)]]
    for name, sub in SAMPLINGS.items():
        groups["streams"][f"optimize_{name}"] = encode(img, quality=92, subsampling=sub, optimize=True)
        groups["streams"][f"restart1_{name}"] = encode(img, quality=92, subsampling=sub, restart_marker_blocks=1)
        groups["streams"][f"restart3_{name}"] = encode(img, quality=92, subsampling=sub, restart_marker_blocks=3)
        groups["streams"][f"qtables_{name}"] = encode(img, subsampling=sub, qtables=qt)
        groups["streams"][f"com_exif_{name}"] = encode(img, quality=80, subsampling=sub, comment=b"a comment segment",
                                                       exif=exif_bytes(1))
    groups["streams"]["restart3_gray"] = encode(img[:, :, 0], quality=92, restart_marker_blocks=3)
    groups["streams"]["optimize_gray"] = encode(img[:, :, 0], quality=92, optimize=True)

    img = lowpass(rng, 9, 17)
    for o in range(1, 9):
        groups["exif"][f"orient{o}"] = encode(img, quality=90, subsampling=2, exif=exif_bytes(o))

    img = lowpass(rng, 24, 40)
    groups["uncovered"]["progressive"] = encode(img, quality=85, progressive=True)
    groups["uncovered"]["cmyk"] = encode(np.concatenate([img, img[:, :, :1]], 2), quality=85)
    try:                                                    # 4:4:0 (luma 1x2): only if this Pillow writes it
        data = encode(img, quality=85, subsampling="4:4:0")
        groups["uncovered"]["440"] = data
    except Exception as e:                                  # noqa: BLE001
        print("4:4:0 not written:", e)

    for g, cases in groups.items():
        out = {}
        for name, data in cases.items():
            out[name + "/jpeg"] = np.frombuffer(data, np.uint8)
            out[name + "/rgb"] = pillow_pixels(data)
        path = os.path.join(HERE, f"jpeg_{g}.npz")
        np.savez_compressed(path, **out)
        print(g, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

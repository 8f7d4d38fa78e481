"""GPU: the JPEG reader (image_io.read_image / read_images / JpegLoader over sw_jpeg_decode_batch) against Pillow's own pixels,
the fixtures of tests/golden/make_jpeg_golden.py (images of at most 64 x 48: partial MCUs, chroma planes one sample wide, odd
downsampled sizes, both sides of libjpeg's "filter only if the downsampled width exceeds 2" rule).  Every pixel equal, in RGB and
BGR, one at a time and as one mixed batch that must not fall back; the files the decoder does not cover equal through Pillow;
nothing written outside the outputs and the declared workspace; the loader feeds TwoCropBatches."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as J  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def fixtures():
    return J.load_fixtures(GOLDEN)


def _hwc(t):
    return np.ascontiguousarray(t.cpu().numpy().transpose(1, 2, 0))


def _mismatches(got, want):
    return [(k, g.shape, w.shape, int((g != w).sum()) if g.shape == w.shape else -1, np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else None)
            for k, g, w in zip(got[0], got[1], want) if g.shape != w.shape or (g != w).any()]


def test_read_image_equals_pillow_in_rgb_and_bgr(fixtures):
    from sos_wsod_amd import read_image
    names = sorted(fixtures)
    rgb, bgr = [], []
    for k in names:
        t, path = read_image(fixtures[k][0], format="RGB", return_path=True)
        assert path == "device" and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous(), k
        rgb.append(_hwc(t))
        bgr.append(_hwc(read_image(fixtures[k][0].tobytes())))                  # bytes, and BGR is the default
    want = [fixtures[k][1] for k in names]
    assert not _mismatches((names, rgb), want)
    assert not _mismatches((names, bgr), [w[:, :, ::-1] for w in want])


def test_one_mixed_batch_equals_pillow_without_fallback(fixtures):
    from sos_wsod_amd import read_images
    names = sorted(fixtures)
    for fmt in ("RGB", "BGR"):
        outs, paths = read_images([fixtures[k][0] for k in names], format=fmt, return_paths=True)
        assert paths == ["device"] * len(names)                                 # a condition: Pillow cannot hide a kernel failure
        want = [fixtures[k][1] if fmt == "RGB" else fixtures[k][1][:, :, ::-1] for k in names]
        assert not _mismatches((names, [_hwc(t) for t in outs]), want)
    again = read_images([fixtures[k][0] for k in names], format="BGR", threads=3)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))                  # run to run, and whatever the host threads


def test_component_planes_equal_the_restatement(fixtures):
    """the first kernel alone: the workspace holds each component's padded plane, dequantised, transformed and limited as the
    restatement does it (DC-only blocks included: the flat files)"""
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd.image_io import decode_batch
    names = ["content/clip_q50_420", "content/noise_q100_422", "content/flat_444", "sizes/420_17x15", "sizes/gray_9x9"]
    datas = [fixtures[k][0] for k in names]
    infos = [ops.jpeg_probe(d)[1] for d in datas]
    ws = torch.zeros(sum(f.coef_bytes // 2 for f in infos), dtype=torch.uint8, device="cuda")
    decode_batch(datas, infos, workspace=ws)
    got, off = ws.cpu().numpy(), 0
    for k, d in zip(names, datas):
        p = J.parse(d.tobytes())
        coef, q = J.entropy_decode(p, d.tobytes())
        for c, plane in enumerate(J.planes(p, coef, q)):
            assert np.array_equal(got[off:off + plane.size].reshape(plane.shape), plane), (k, c)
            off += plane.size
    assert off == got.size


def test_not_covered_files_come_back_through_pillow():
    from sos_wsod_amd import read_image, read_images
    un = J.load_fixtures(GOLDEN, ("uncovered",))
    names = sorted(un)
    outs, paths = read_images([un[k][0] for k in names], format="RGB", return_paths=True)
    assert paths == ["pillow"] * len(names) and len(names) >= 2
    assert not _mismatches((names, [_hwc(t) for t in outs]), [un[k][1] for k in names])
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(un[names[0]][1]).save(buf, "PNG")                           # not a JPEG at all
    t, path = read_image(buf.getvalue(), format="BGR", return_path=True)
    assert path == "pillow" and np.array_equal(_hwc(t), un[names[0]][1][:, :, ::-1])


def test_orientations(fixtures):
    from sos_wsod_amd import read_image
    for o in range(1, 9):
        jp, want = fixtures[f"exif/orient{o}"]
        t = read_image(jp, format="RGB")
        assert tuple(t.shape) == (3,) + want.shape[:2] == ((3, 17, 9) if o >= 5 else (3, 9, 17)), o
        assert np.array_equal(_hwc(t), want), o


def test_malformed_stream_raises_with_the_reason(fixtures):
    from sos_wsod_amd import read_image, read_images
    jp = fixtures["sizes/420_16x16"][0]
    with pytest.raises(ValueError, match="entropy-coded data ends early"):
        read_image(jp[:len(jp) - 40])
    with pytest.raises(ValueError, match="marker segments end early"):
        read_images([fixtures["sizes/444_8x8"][0], jp[:100]])
    with pytest.raises(ValueError):
        read_image(jp, format="L")


def test_nothing_is_written_outside_outputs_and_workspace(fixtures):
    """outputs and workspace carved out of larger sentinel-filled buffers: every byte outside the 3 * H * W of each output and
    outside the declared workspace bytes keeps the sentinel; odd widths take the byte-store path, multiples of 4 the word stores"""
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd._lib import JpegInfo
    from sos_wsod_amd.image_io import decode_batch
    names = ["sizes/420_17x15", "sizes/422_33x31", "sizes/444_7x5", "sizes/gray_9x9", "sizes/420_1x1", "sizes/420_64x48",
             "sizes/422_16x16", "sizes/gray_8x8", "sizes/420_5x6"]
    datas = [fixtures[k][0] for k in names]
    infos = [ops.jpeg_probe(d)[1] for d in datas]
    need = ops.jpeg_workspace_bytes((JpegInfo * len(infos))(*infos))
    assert need == sum(f.coef_bytes // 2 for f in infos)
    S, PAD = 0xA5, 256
    big_ws = torch.full((need + 3 * PAD,), S, dtype=torch.uint8, device="cuda")
    lead = (-big_ws.data_ptr()) % 256 + PAD
    ws = big_ws[lead:lead + need]
    sizes = [3 * f.height * f.width for f in infos]
    starts = np.concatenate([[0], np.cumsum([PAD + (s + 3) // 4 * 4 for s in sizes])]) + PAD
    big_out = torch.full((int(starts[-1]) + PAD,), S, dtype=torch.uint8, device="cuda")
    outs = [big_out[int(a):int(a) + s].view(3, f.height, f.width) for a, s, f in zip(starts, sizes, infos)]
    decode_batch(datas, infos, format="RGB", outs=outs, workspace=ws)
    torch.cuda.synchronize()
    for k, t in zip(names, outs):
        assert np.array_equal(_hwc(t), fixtures[k][1]), k
    mask = np.ones(big_out.numel(), bool)
    for a, s in zip(starts, sizes):
        mask[int(a):int(a) + s] = False
    assert (big_out.cpu().numpy()[mask] == S).all()
    host_ws = big_ws.cpu().numpy()
    assert (host_ws[:lead] == S).all() and (host_ws[lead + need:] == S).all()
    with pytest.raises(ValueError):
        decode_batch(datas, infos, workspace=ws[:need - 1])
    with pytest.raises(ValueError):
        decode_batch(datas, infos, workspace=big_ws[lead + 1:lead + 1 + need])


def test_loader_feeds_two_crop_batches(fixtures, tmp_path):
    from sos_wsod_amd import JpegLoader
    from sos_wsod_amd.strong_aug import DeviceTwoCropMapper, TwoCropBatches
    dicts = []
    for i, k in enumerate(("sizes/420_64x48", "sizes/422_33x31")):
        jp, rgb = fixtures[k]
        fn = tmp_path / f"{i}.jpg"
        fn.write_bytes(jp.tobytes())
        dicts.append({"file_name": str(fn), "index": i, "height": rgb.shape[0], "width": rgb.shape[1],
                      "annotations": [{"bbox": [2, 2, 20, 20], "category_id": 1}]})
    loader = JpegLoader("BGR")
    for d, k in zip(dicts, ("sizes/420_64x48", "sizes/422_33x31")):
        assert np.array_equal(_hwc(loader(d)), fixtures[k][1][:, :, ::-1])
    m = DeviceTwoCropMapper(min_sizes=(48,), max_size=96, seed=3)
    lq, lk, uq, uk = next(iter(TwoCropBatches(m, dicts, dicts, loader, 1, 1, seed=1, label_order=[0, 1, 0, 1], unlabel_order=[0, 1, 0, 1])))
    for q, k in zip(lq + uq, lk + uk):
        assert q["image"].is_cuda and q["image"].dtype == torch.uint8 and q["image"].shape == k["image"].shape
        assert min(k["image"].shape[1:]) == 48 and q["instances"] is k["instances"]

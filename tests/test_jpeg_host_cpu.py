"""CPU: the host half of the JPEG reader (sw_jpeg_probe, sw_jpeg_entropy_decode in csrc/jpeg.hip; plain C++ inside the library,
which loads on a machine without a GPU) against tests/jpeg_ref.py: the probe's fields, the coefficients and tables, the codes for
files it does not cover, and that no truncation or marker damage makes it read or write out of bounds."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_ref as J

SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return J.load_fixtures(golden_dir)


def _decode(ops, data, info, extra=64):
    """-> (code, coefficients, tables, the sentinel words behind each buffer)"""
    n = info.coef_bytes // 2
    coef = np.full(n + extra, SENTINEL, np.int16)
    qt = np.full(256 + extra, SENTINEL, np.uint16)
    rc = ops.jpeg_entropy_decode(data, info, coef.ctypes.data, qt.ctypes.data)
    return rc, coef[:n], qt[:256], (coef[n:], qt[256:])


def test_probe_fields(fixtures):
    import sos_wsod_amd.ops as ops
    for name, (jp, rgb) in fixtures.items():
        p = J.parse(jp.tobytes())
        rc, f = ops.jpeg_probe(jp)
        assert rc == 1, (name, rc)
        nc = p["ncomp"]
        assert (f.width, f.height, f.ncomp, f.restart_interval, f.orientation) == \
            (p["width"], p["height"], nc, p["restart"], p["orientation"]), name
        assert (f.mcus_x, f.mcus_y) == (p["mcus_x"], p["mcus_y"]), name
        assert list(f.hsamp)[:nc] == p["hs"] and list(f.vsamp)[:nc] == p["vs"] and list(f.qtable)[:nc] == p["tq"], name
        assert list(f.blocks_w)[:nc] == p["blocks_w"] and list(f.blocks_h)[:nc] == p["blocks_h"], name
        assert f.coef_bytes == p["coef_bytes"], name
        shape = (f.width, f.height) if f.orientation >= 5 else (f.height, f.width)
        assert rgb.shape[:2] == shape, name


def test_coefficients_and_tables_equal_the_restatement(fixtures):
    import sos_wsod_amd.ops as ops
    for name, (jp, _) in fixtures.items():
        p = J.parse(jp.tobytes())
        want, q = J.entropy_decode(p, jp.tobytes())
        rc, f = ops.jpeg_probe(jp)
        rc, coef, qt, guards = _decode(ops, jp, f)
        assert rc == 0, (name, rc)
        assert np.array_equal(coef, np.concatenate([w.reshape(-1) for w in want])), name
        assert np.array_equal(qt.reshape(4, 64), q), name
        assert all((g == SENTINEL).all() for g in guards), name


def test_threads_share_nothing(fixtures):
    """re-entrant: sixteen threads decoding different files at once give what one thread gives"""
    import sos_wsod_amd.ops as ops
    items = [jp for _, (jp, _) in sorted(fixtures.items())][:32]

    def one(jp):
        rc, f = ops.jpeg_probe(jp)
        rc, coef, qt, _ = _decode(ops, jp, f)
        return rc, coef.copy(), qt.copy()

    serial = [one(jp) for jp in items]
    with ThreadPoolExecutor(16) as pool:
        for _ in range(3):
            for a, b in zip(serial, pool.map(one, items)):
                assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_not_covered_and_not_jpeg(golden_dir):
    import sos_wsod_amd.ops as ops
    for name, (jp, _) in J.load_fixtures(golden_dir, ("uncovered",)).items():
        assert ops.jpeg_probe(jp)[0] == 0, name
    for junk in (b"\x89PNG\r\n\x1a\n" + b"\0" * 64, b"", b"\xff", b"\xff\xd8", b"GIF89a" + b"\1" * 40):
        rc, _ = ops.jpeg_probe(np.frombuffer(junk, np.uint8))
        assert rc < 0, junk
        assert ops.jpeg_error(rc) not in ("", "unknown code")
    assert ops.jpeg_probe(np.frombuffer(b"\x89PNG\r\n\x1a\n" + b"\0" * 64, np.uint8))[0] == -2


def _variants_of_adobe_and_ids(jp):
    """the same 3-component stream with (a) an Adobe APP14 marker, transform 0, in front of the tables, (b) the JFIF segment
    dropped and the component ids spelled R, G, B, (c) luma sampling factors the decoder does not cover (4:4:0 and 4:1:1, which
    Pillow does not write) and one it does"""
    b = bytes(jp)
    assert b[2:4] == b"\xff\xe0"
    L = (b[4] << 8) | b[5]
    rest = b[4 + L:]
    adobe = lambda t: b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t])
    yield "adobe0", b[:4 + L] + adobe(0) + rest, 0
    yield "adobe1", b[:4 + L] + adobe(1) + rest, 1
    r = bytearray(b[:2] + rest)
    sof = r.index(b"\xff\xc0")
    sos = r.index(b"\xff\xda")
    for c, ch in enumerate(b"RGB"):
        r[sof + 10 + 3 * c] = ch
        r[sos + 5 + 2 * c] = ch
    yield "rgb_ids", bytes(r), 0
    for name, samp in (("luma_1x2", 0x12), ("luma_4x1", 0x41), ("luma_2x2_again", 0x22)):     # the SOF's luma sampling byte alone
        r = bytearray(b)
        r[r.index(b"\xff\xc0") + 11] = samp
        yield name, bytes(r), 1 if samp == 0x22 else 0


def test_colour_space_markers(fixtures):
    import sos_wsod_amd.ops as ops
    for name, data, want in _variants_of_adobe_and_ids(fixtures["sizes/444_16x16"][0]):
        assert ops.jpeg_probe(np.frombuffer(data, np.uint8))[0] == want, name
        assert (J.parse(data)["status"] == 1) == (want == 1), name


def test_truncation_and_marker_damage_stay_in_bounds(fixtures):
    """one 16 x 16 4:2:0 file: every truncation length, and every single-byte change in the marker segments, returns a code (a
    negative one or a decode) and leaves the words behind the buffers alone.  The input array ends exactly at the truncation, so
    a read past `n` would land in another allocation."""
    import sos_wsod_amd.ops as ops
    jp = fixtures["sizes/420_16x16"][0]
    whole = jp.tobytes()
    rc, full = ops.jpeg_probe(jp)
    assert rc == 1
    scan = J.parse(whole)["scan"]
    want = _decode(ops, jp, full)[1]
    seen = set()
    for n in range(len(whole)):
        data = np.frombuffer(whole[:n], np.uint8).copy()
        rc, f = ops.jpeg_probe(data)
        assert rc in (1, 0) or rc < 0
        assert rc < 0 or n >= scan
        seen.add(rc)
        if rc == 1:
            rc2, coef, qt, guards = _decode(ops, data, f)
            assert rc2 <= 0, (n, rc2)
            if rc2 == 0:                                                        # only EOI or padding is gone: the same decode
                assert n >= len(whole) - 3 and np.array_equal(coef, want), n
            assert all((g == SENTINEL).all() for g in guards), n
            seen.add(rc2)
    assert {-2, -3, -6} <= seen
    rng = np.random.RandomState(3)
    for pos in range(2, scan):
        for val in {whole[pos] ^ 0xFF, whole[pos] ^ 0x01, int(rng.randint(256))} - {whole[pos]}:
            data = np.frombuffer(whole, np.uint8).copy()
            data[pos] = val
            rc, f = ops.jpeg_probe(data)
            assert isinstance(rc, int)
            if rc == 1:
                assert f.coef_bytes == 128 * sum(f.blocks_w[c] * f.blocks_h[c] for c in range(f.ncomp)) and f.coef_bytes <= 128 * 3 * 8192 ** 2
                if f.coef_bytes <= 1 << 24:                                     # a damaged size field may ask for gigabytes: probe only
                    rc2, coef, qt, guards = _decode(ops, data, f)
                    assert all((g == SENTINEL).all() for g in guards), (pos, val)
    # the info must describe the stream it is used with
    other = ops.jpeg_probe(fixtures["sizes/444_16x16"][0])[1]
    assert _decode(ops, jp, other)[0] == -9


def test_orientation_on_tensors_equals_image_transpose(fixtures):
    """image_io.apply_orientation (exact torch flips / transposes) on Pillow's unrotated pixels gives Pillow's rotated ones"""
    import torch
    from sos_wsod_amd.image_io import apply_orientation
    base = fixtures["exif/orient1"][1]
    for o in range(1, 9):
        jp, rgb = fixtures[f"exif/orient{o}"]
        plain = J.decode_rgb(jp.tobytes())[0]
        assert np.array_equal(plain, base)
        got = apply_orientation(torch.from_numpy(np.ascontiguousarray(plain.transpose(2, 0, 1))), o)
        assert got.is_contiguous() and np.array_equal(got.numpy().transpose(1, 2, 0), rgb), o


def test_formats_other_than_rgb_and_bgr_raise():
    from sos_wsod_amd.image_io import JpegLoader, read_image
    with pytest.raises(ValueError):
        read_image(b"", format="L")
    with pytest.raises(ValueError):
        JpegLoader(format="YUV-BT.601")


def test_split_cli_picks_the_loader(tmp_path):
    """`python -m sos_wsod_amd.split loss --decode device` hands the scorer a JpegLoader in BGR; the default stays _pillow_bgr"""
    import sos_wsod_amd.split as S
    from sos_wsod_amd.image_io import JpegLoader
    cfg = tmp_path / "c.yaml"
    cfg.write_text("INPUT:\n  MIN_SIZE_TRAIN: (96,)\n  MAX_SIZE_TRAIN: 300\n")
    dicts = [{"height": 100, "width": 120, "annotations": [{"bbox": [1, 1, 50, 50], "category_id": 0}]} for _ in range(6)]
    seen = []

    def scorer(model, ds, loader, **kw):
        seen.append(loader)
        return np.arange(len(ds), dtype=np.float32)

    common = ["loss", "--config", str(cfg), "--save-path", str(tmp_path / "s.txt"), "--k", "2"]
    S.main(common, scorer=scorer, dataset_dicts=dicts)
    S.main(common + ["--decode", "device"], scorer=scorer, dataset_dicts=dicts)
    assert seen[0] is S._pillow_bgr
    assert isinstance(seen[1], JpegLoader) and seen[1].format == "BGR"
    with pytest.raises(SystemExit):
        S.parse_args(["loss", "--decode", "opencv"])

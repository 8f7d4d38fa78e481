"""CPU: tests/jpeg_ref.py, the NumPy restatement of the baseline JPEG decode chain, against Pillow's own pixels (the fixtures of
tests/golden/make_jpeg_golden.py).  The chain is integer arithmetic throughout, so the bar is zero mismatches: this test settles
the IDCT constants, the range limit, the upsampling edge rules (libjpeg filters only when the downsampled width exceeds 2) and the
colour rule that the host code and the kernels are then held to."""
import numpy as np
import pytest

import jpeg_ref as J


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return J.load_fixtures(golden_dir)


def test_fixture_set_is_the_one_the_generator_writes(fixtures):
    sizes = [(1, 1), (3, 3), (4, 4), (5, 6), (7, 5), (8, 8), (9, 9), (15, 17), (16, 16), (17, 15), (33, 31), (64, 48)]
    for s in ("444", "422", "420", "gray"):
        for w, h in sizes:
            jp, rgb = fixtures[f"sizes/{s}_{w}x{h}"]
            assert rgb.shape == (h, w, 3)
    assert sum(k.startswith("exif/") for k in fixtures) == 8
    assert max(v[1].shape[0] for v in fixtures.values()) <= 48 and max(v[1].shape[1] for v in fixtures.values()) <= 64


def test_every_covered_fixture_equals_pillow(fixtures):
    bad = []
    for name, (jp, rgb) in fixtures.items():
        got = J.decode_rgb(jp.tobytes())
        assert got is not None, f"{name}: not covered"
        px = J.apply_orientation(got[0], got[1])
        if px.shape != rgb.shape or (px != rgb).any():
            bad.append((name, px.shape, int((px != rgb).sum()) if px.shape == rgb.shape else -1))
    assert not bad, bad


def test_fixtures_reach_the_hard_paths(fixtures):
    """the binary-noise files leave [0, 255] on both sides before the range limit, the uniform-noise ones hold 16-bit codes; the
    samplings are the ones the names say; restart intervals and orientations are read"""
    jp = fixtures["content/clip_q50_444"][0].tobytes()
    p = J.parse(jp)
    coef, q = J.entropy_decode(p, jp)
    x = (coef[0].astype(np.int64) * q[p["tq"][0]].astype(np.int64)).reshape(-1, 8, 8)
    ws = J._idct_1d(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)
    v = J._idct_1d(ws, 18)
    assert v.min() < -128 - 16 and v.max() > 127 + 16                      # clipped by a margin, not by one rounding step
    jp = fixtures["content/noise_q100_444"][0].tobytes()
    p = J.parse(jp)
    assert max(ln for tab in p["huff"].values() for ln in range(16) if tab[0][ln]) + 1 >= 11
    for s, want in (("444", (1, 1)), ("422", (2, 1)), ("420", (2, 2))):
        p = J.parse(fixtures[f"sizes/{s}_17x15"][0].tobytes())
        assert (p["hs"][0], p["vs"][0]) == want and p["ncomp"] == 3
    assert J.parse(fixtures["sizes/gray_17x15"][0].tobytes())["ncomp"] == 1
    assert J.parse(fixtures["streams/restart1_420"][0].tobytes())["restart"] == 1
    assert J.parse(fixtures["streams/restart3_422"][0].tobytes())["restart"] == 3
    assert [J.parse(fixtures[f"exif/orient{o}"][0].tobytes())["orientation"] for o in range(1, 9)] == list(range(1, 9))
    flat = J.parse(fixtures["content/flat_420"][0].tobytes())
    c, _ = J.entropy_decode(flat, fixtures["content/flat_420"][0].tobytes())
    assert all(not a[:, :, 1:].any() for a in c)                                   # DC only


def test_not_covered_files_are_left_alone(golden_dir):
    un = J.load_fixtures(golden_dir, ("uncovered",))
    assert {"uncovered/progressive", "uncovered/cmyk"} <= set(un)
    for name, (jp, _) in un.items():
        assert J.parse(jp.tobytes())["status"] == 0, name
    with pytest.raises(J.MalformedJpeg):
        J.parse(b"\x89PNG\r\n\x1a\n" + b"\0" * 32)

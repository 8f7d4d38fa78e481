"""tests/roipool_ref.py against the CPU oracle, and the constructed cases of tests/test_gpu_roipool_bwd.py against the property each
one is named for.  No GPU."""
import numpy as np
import pytest

import roipool_ref as RR
from oracle import oicr_oracle as O


def _edge_rois(H, W, nimg):
    boxes = [[0, 0, 1e4, 1e4], [-50, -50, -10, -10], [100, 100, 90, 90], [8 * W - 1, 8 * H - 1, 8 * W + 40, 8 * H + 40],
             [3.9, 3.9, 4.1, 4.1], [-8, -8, 8 * W, 8 * H], [12, 20, 12, 20], [4, 4, 11.9, 12.1], [-3.99, -4.0, 20, 28]]
    return RR._rois_from_boxes(np.arange(len(boxes)) % nimg, boxes)


@pytest.mark.parametrize("P", [(7, 7), (1, 1), (1, 3), (3, 2), (14, 14)])
def test_forward_restatement_equals_the_oracle(P):
    nimg, C, H, W, R = 2, 5, 23, 31, 60
    rng = np.random.default_rng(1)
    feat = rng.standard_normal((nimg, C, H, W)).astype(np.float32)
    feat[0, 0, 3:9, 4:12] = 0.5                                    # ties: the first pixel in row-major order wins
    feat[1, 1, 5, 5] = np.nan                                      # never wins
    feat[1, 2, :, :] = -np.inf                                     # cannot beat -FLT_MAX: -FLT_MAX / -1
    x1 = rng.uniform(-20, 8 * W, R); y1 = rng.uniform(-20, 8 * H, R)
    boxes = np.stack([x1, y1, x1 + rng.uniform(0, 200, R), y1 + rng.uniform(0, 160, R)], 1)
    rois = np.concatenate([RR._rois_from_boxes(np.arange(R) % nimg, boxes), _edge_rois(H, W, nimg)])
    out, arg = RR.roi_pool_fwd(feat, rois, 1.0 / 8, *P)
    ref_out, ref_arg = O.roi_pool_fwd(feat, rois, 1.0 / 8, *P)
    assert np.array_equal(arg, ref_arg)
    assert np.array_equal(out, ref_out)
    assert (arg == -1).any() and (arg >= 0).any()


@pytest.mark.parametrize("name", sorted(RR.OVERSHOOT_MAPS))
def test_forward_restatement_equals_the_oracle_on_overshooting_rois(name):
    case = RR.overshoot_case(name, "f32", 32)
    nimg, H, W, C = case.shape
    _, ref_arg = O.roi_pool_fwd(RR.row_ramp(nimg, C, H, W), case.rois, case.scale, 7, 7)
    assert np.array_equal(case.argmax.reshape(ref_arg.shape), ref_arg)


def test_backward_restatement_equals_the_oracle_within_float32_summation_error():
    nimg, C, H, W, R = 2, 6, 12, 15, 300
    rng = np.random.default_rng(2)
    feat = rng.standard_normal((nimg, C, H, W)).astype(np.float32)
    x1 = rng.uniform(-20, 8 * W, R); y1 = rng.uniform(-20, 8 * H, R)
    boxes = np.stack([x1, y1, x1 + rng.uniform(0, 100, R), y1 + rng.uniform(0, 100, R)], 1)
    rois = np.concatenate([RR._rois_from_boxes(np.arange(R) % nimg, boxes), _edge_rois(H, W, nimg)])
    _, arg = RR.roi_pool_fwd(feat, rois, 1.0 / 8)
    g = rng.standard_normal(arg.shape).astype(np.float32)
    oracle = O.roi_pool_bwd(g, arg, rois, feat.shape).transpose(0, 2, 3, 1)                  # NCHW -> NHWC
    br = RR.roi_pool_bwd_ref(g.reshape(len(rois), C, 49), arg.reshape(len(rois), C, 49), rois, (nimg, H, W, C))
    assert br.n.sum() == (arg >= 0).sum() and br.n.max() > 8
    # the oracle adds n float32 terms one after the other: each addition is off by at most 2^-24 of a partial sum <= S
    assert np.all(np.abs(oracle - br.ref) <= br.S * br.n * 2.0 ** -24)
    assert np.all(br.tmax <= br.S) and np.all(br.tmax * br.n >= br.S * (1 - 1e-12))
    # row scale and ReLU mask
    rs = rng.random(len(rois)).astype(np.float32)
    relu = rng.standard_normal((nimg, H, W, C)).astype(np.float32)
    relu[0, 0, 0, 0] = np.nan; relu[0, 0, 1, 0] = -0.0
    b2 = RR.roi_pool_bwd_ref(g.reshape(len(rois), C, 49), arg.reshape(len(rois), C, 49), rois, (nimg, H, W, C), rs, 1.0, relu)
    scaled = g * (rs + np.float32(1.0))[:, None, None, None]
    o2 = O.roi_pool_bwd(scaled, arg, rois, feat.shape).transpose(0, 2, 3, 1) * (relu > 0)
    assert np.all(np.abs(o2 - b2.ref) <= b2.S * (b2.n + 1) * 2.0 ** -24)
    assert b2.ref[0, 0, 0, 0] == 0 and b2.ref[0, 0, 1, 0] == 0


def test_overshoot_heights():
    h7 = RR.overshoot_heights(7)
    assert h7 and h7 == RR.overshoot_heights(14)
    assert {57, 114, 121} <= set(h7)
    for h in h7:                                                   # the statement itself, in plain float32
        b = np.float32(h) / np.float32(7)
        assert np.ceil(np.float32(7) * b) > h


def test_half_ulp_and_bf16_rounding():
    assert RR.half_ulp(1.0, "bf16") == 2.0 ** -8 and RR.half_ulp(1.99, "bf16") == 2.0 ** -8 and RR.half_ulp(2.0, "bf16") == 2.0 ** -7
    assert RR.half_ulp(1.0, "f32") == 2.0 ** -24 and RR.half_ulp(0.0, "f32") == 2.0 ** -150 and RR.half_ulp(0.0, "bf16") == 2.0 ** -134
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3], np.float32)
    assert np.array_equal(RR.round_bf16(x)[:3], np.array([1.0, 1.0, 1.0 + 2.0 ** -6], np.float32))      # ties to even
    assert RR.fx_frac(1 - 2.0 ** -8, 1.0, 13) == 13 and RR.fx_frac(1.0, 1.0, 13) == 12 and RR.fx_frac(0.0, 1.0, 13) == 0


def test_plan_mirror_on_the_training_shapes():
    p = RR.bwd_plan("bf16", 16, 2, 63, 63, 512, 7, 7, 4000, 512 * 49 + 64, True, True)
    assert (p.path, p.accmode, p.CB, p.nsplit) == ("fx", 2, 4, 1) and p.bits(2000) == (13, 14)
    assert RR.bwd_plan("bf16", 16, 2, 150, 200, 512, 7, 7, 4000, 0, True, True).nsplit == 7
    assert RR.bwd_plan("bf16", 16, 2, 99, 165, 512, 7, 7, 4000, 0, True, True).nsplit == 4
    assert RR.bwd_plan("f32", 32, 2, 63, 63, 512, 7, 7, 4000, 0, True, True).accmode == 0
    assert RR.bwd_plan("bf16", 16, 1, 4, 4, 4, 16, 16, 16384, 0, True, True).accmode == 0        # 2^22 terms: 64-bit words
    assert RR.bwd_plan("bf16", 16, 1, 4, 4, 4, 16, 16, 16383, 0, True, True).accmode == 2
    assert RR.bwd_plan("bf16", 32, 1, 240, 320, 4, 7, 7, 8, 0, True, True).nsplit == 16
    assert RR.bwd_plan("bf16", 32, 1, 240, 321, 4, 7, 7, 8, 0, True, True).path == "refused"
    assert RR.bwd_plan("bf16", 16, 2, 63, 63, 512, 7, 7, 4000, 512 * 49 - 1, True, True).path == "refused"


# ---------------------------------------------------------------------------------------------- the constructed cases
def _assert_plan(case):
    p = case.plan()
    assert (p.path, p.CB) == (case.path, case.CB), (case.name, p)
    if case.path == "fx":
        assert (p.nsplit, p.accmode) == (case.nsplit, case.accmode), (case.name, p)


@pytest.mark.parametrize("name", sorted(RR.OVERSHOOT_MAPS))
def test_overshoot_cases_put_gradient_in_the_row_after_the_roi_inside_the_later_range(name):
    H, W, rs, re, cols = RR.OVERSHOOT_MAPS[name]
    case = RR.overshoot_case(name, "bf16", 16)
    _assert_plan(case)
    assert re - rs + 1 in RR.overshoot_heights(7)
    p0 = RR.pixel_ranges(case.plan(), H, W)[1][0]
    assert p0 // W == re + 1                                       # the second range starts in the row after the ROIs' end row
    for r in range(len(cols)):                                     # the ROI's own rounded rows, as the parent's filter read them
        s, e, _ = RR.roi_extent(case.rois[r, 2], case.rois[r, 4], case.scale)
        assert (int(s), int(e)) == (rs, re)
    only = RR.roi_pool_bwd_ref(case.dout[:len(cols)], case.argmax[:len(cols)], case.rois[:len(cols)], case.shape)
    row = only.ref.reshape(H * W, 4)[max(p0, (re + 1) * W):(re + 2) * W]
    assert np.count_nonzero(row) >= 4                              # lost by a filter that stops at row re
    assert not only.n.reshape(H, W, 4)[re + 2:].any()


@pytest.mark.parametrize("nsplit", sorted(RR.RANGE_MAPS))
def test_range_cases_touch_both_sides_of_every_boundary(nsplit):
    case = RR.range_edge_case(nsplit, "bf16")
    _assert_plan(case)
    _, H, W, C = case.shape
    n = case.reference().n.reshape(2, H * W, C).sum(axis=(0, 2))
    for p0, p1 in RR.pixel_ranges(case.plan(), H, W):
        assert p1 > p0 and n[p0] and n[p1 - 1] and (p0 == 0 or n[p0 - 1])
    assert n[H * W - 1]


def test_pooled_cases_take_both_slab_widths_and_keep_channels_apart():
    for PH, PW in RR.POOLED:
        for dtype, C in (("bf16", 4), ("f32", 4), ("bf16", 1024)):
            case = RR.pooled_case(PH, PW, dtype, C)
            _assert_plan(case)
            assert (case.argmax >= 0).any()
            d = case.dout
            assert all(not np.array_equal(d[:, c], d[:, c + 1]) for c in range(C - 1))
    _assert_plan(RR.pooled_case(7, 7, "bf16", 1024, has_absmax=False))
    _assert_plan(RR.pooled_case(1, 1, "f32", 4, has_absmax=False))


@pytest.mark.parametrize("R", RR.CHUNK_R)
def test_chunk_cases_leave_one_image_without_rois(R):
    case = RR.chunk_case(R, True)
    _assert_plan(case)
    n = case.n_img()
    assert n[2] == 0 and n.sum() == R
    if R > 100:
        assert n[0] > n[1] > n[3] > 0
    assert not case.reference().ref[2].any()


def test_pile_cases_sit_on_the_accumulator_edges():
    for R, bits in ((1023, 16), (1024, 17), (1025, 17)):
        for absmax in (1 - 2.0 ** -8, 1.0):
            case = RR.pile_case(8, R, absmax)
            _assert_plan(case)
            assert (64 * R).bit_length() == bits and case.plan().bits(R) == (30 - bits, 31 - bits)
            br = case.reference()
            assert br.n.max() == 64 * R and np.count_nonzero(br.n) == 4 and br.ref.max() == 64 * R * absmax
            # the hi word at its fullest: every term below 2^term_bits, their sum below 2^30
            tb = 30 - bits
            assert 64 * R * absmax * 2.0 ** RR.fx_frac(absmax, 1.0, tb) < 2.0 ** 30
            assert 4 * R * 2.0 ** tb < 2.0 ** 30 < 64 * R * 2.0 ** (30 - (4 * R).bit_length())     # 4 bins per ROI would not fit
    assert RR.pile_case(8, 1024, 1 - 2.0 ** -24, "f32").plan().accmode == 0


def test_remaining_cases_take_their_plans():
    _assert_plan(RR.lognormal_case())
    for dtype in ("bf16", "f32"):
        for kind in ("negative", "decades", "zero"):
            case = RR.scale_case(kind, dtype)
            _assert_plan(case)
            mul = RR.row_multiplier(case.row_scale, case.add, case.R)
            if kind == "negative":
                assert (mul < 0).all()
            elif kind == "decades":
                assert np.abs(mul).max() / np.abs(mul).min() > 1e25
            else:
                assert not mul.any()
            m = case.relu_ref
            assert np.isnan(m).any() and (np.signbit(m) & (m == 0)).any() and (m < 0).any() and (m > 0).any()
        for kind in RR.POISONS:
            for amax in (True, False):
                case = RR.poison_case(kind, dtype, amax)
                _assert_plan(case)
                ref = case.reference().ref
                assert case.rois[3, 0] == 0 and not np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
                assert np.isnan(ref[0]).any() == kind.endswith("nan")
        for kind in RR.FALLBACKS:
            _assert_plan(RR.fallback_case(kind, dtype))
        _assert_plan(RR.gap_case(dtype, 16, "fx"))
        _assert_plan(RR.gap_case(dtype, 32, "float"))
    assert RR.gap_case("bf16", 16, "fx").pad % 4 == 0 and RR.gap_case("bf16", 16, "float").pad % 4 != 0

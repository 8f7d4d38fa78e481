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


# ================================================================================================ the forward's mirror and cases
def _plan(H, W, ws, C=512, R=4000, nimg=2, P=7, dtype="bf16", bits=16):
    return RR.fwd_plan(dtype, bits, nimg, H, W, C, P, P, R, 0, True, ws)


@pytest.mark.parametrize("H,W,with_ws,without_ws", [
    (63, 63, ("sparse_whole", 8, 1), ("sparse_whole", 8, 1)),        # "maps that fit LDS whole at 8 channels per lane ... stay with" the sparse kernel
    (76, 114, ("tasks", 4, 1), ("sparse_band", 4, 1)),
    (99, 165, ("tasks", 4, 3), ("sparse_band", 4, 3)),               # "99x165 -> 3 bands"
    (125, 167, ("tasks", 4, 4), ("sparse_band", 4, 4)),
    (150, 200, ("tasks", 4, 7), ("sparse_band", 4, 7)),
])
def test_fwd_plan_on_the_maps_roipool_hip_names(H, W, with_ws, without_ws):
    """C = 512, two images, 7 x 7, 4000 ROIs: the forms (and channels per lane, bands) the comments of roipool.hip give these maps"""
    for ws, want in (("auto", with_ws), (None, without_ws)):
        p = _plan(H, W, ws)
        assert (p.form, p.CB, p.n_bands) == want, (ws, p)
        assert p.lds <= RR.LDS_CU - 1024
        assert p.rows * W <= 10 * 1024 or p.form == "sparse_whole"
    # the slab widths the plane form's comment names: 8 channels per lane on 76x114 and 86x115, 2 on 125x167 and 150x200 (bf16, 4-byte pixels)
    for (h, w), cb in (((76, 114), 8), ((86, 115), 8)):
        assert RR.fwd_plan("bf16", 16, 2, h, w, 512, 9, 7, 4000, 0, True, None).CB == cb
    assert RR.fwd_plan("f32", 16, 2, 150, 200, 512, 7, 7, 4000, 0, True, None).CB == 1
    assert RR.fwd_plan("f32", 16, 2, 125, 167, 512, 7, 7, 4000, 0, True, None).CB == 1


def test_fwd_workspace_bytes_mirror_the_entry():
    """seg, geo and histogram regions rounded to 256 bytes, then nimg * R * PH records of 32 bytes"""
    assert RR.fwd_workspace_bytes(2, 4000, 7, 7) == 5632 + 192000 + 86016 + 2 * 4000 * 7 * 32
    assert RR.fwd_workspace_bytes(0, 10, 7, 7) == 0 and RR.fwd_workspace_bytes(2, 0, 7, 7) == 0


def test_band_geometry_rules():
    assert RR.band_geometry(76, 7, 80, RR.TASK_BANDS) == (76, 76, 1)                 # whole if it fits
    assert RR.band_geometry(76, 7, 80, RR.PLANE_BANDS) == (68, 80, 2)                # the plane form never takes that way out
    assert RR.band_geometry(99, 7, 57, RR.TASK_BANDS) == (33, 57, 3)                 # equal bands: 41 own rows evened out to 33
    assert RR.band_geometry(99, 7, 57, RR.SPARSE_BANDS) == (41, 57, 3)
    assert RR.band_geometry(99, 7, 16 + 7, RR.SPARSE_BANDS) is None and RR.band_geometry(99, 7, 16 + 8, RR.SPARSE_BANDS) == (8, 24, 13)
    assert RR.band_geometry(99, 7, 16 + 3, RR.TASK_BANDS) is None and RR.band_geometry(99, 7, 16 + 4, RR.TASK_BANDS) == (4, 20, 25)
    for H, S, n in ((110, 55, 2), (99, 33, 3)):
        assert RR.band_owner(H, S, n) == n - 1 and RR.band_owner(H - 1, S, n) == n - 1 and RR.band_owner(S - 1, S, n) == 0
    assert RR.band_y0(2, 33, 57, 99, True) == 42 and RR.band_y0(2, 33, 57, 99, False) == 66


def test_threshold_straddles_flip_the_plan():
    """the cases of one straddle sit on both sides of ONE inequality: neighbours differ in form, channels per lane or refusal code, and
    each lands where it aims (monotone: no third form in between)"""
    for what, cases in RR.threshold_pairs():
        plans = [RR.check_fwd_plan(c) for c in cases]
        keys = [(p.form, p.CB, p.code, c.shape[3] // p.CB if p.CB else 0) for p, c in zip(plans, cases)]       # (C 6 / 2 and 3 / 1 differ in slabs only)
        for (ca, a), (cb, b) in zip(zip(cases, keys), zip(cases[1:], keys[1:])):
            if cb.pad > 0:
                assert a == b, what                                                  # a wider pitch changes nothing
            else:
                assert a != b, what
    # the edges the issue names by shape are the exact ones
    assert 96 * 100 * 16 == 120 * 160 * 8 == 160 * 240 * 4 == RR.PLANE_BUDGET
    assert min(97 * 99 * 16, 113 * 170 * 8, 161 * 239 * 4) > RR.PLANE_BUDGET


def test_declined_band_geometries_go_to_the_next_form():
    by = {c.name.split("/")[1]: c for c in RR.fwd_cases("thresholds")}
    c = by["declined_tasks"]
    assert RR._task_bands(c.shape[1], c.shape[2], c.PH) is None and c.workspace == "auto" and c.form in ("sparse_band", "plane")
    c = by["declined_sparse"]
    assert RR._sparse_bands(c.shape[1], c.shape[2], c.PH, c.R) is None and c.form in ("plane_band", "plane")
    c = by["declined_plane_band"]
    assert RR.plane_band_geometry(c.shape[1], c.shape[2], c.PH, c.PW) is None and c.form in ("plane", "gather")
    c = by["bands17"]
    assert RR._task_bands(c.shape[1], c.shape[2], c.PH)[2] > RR.TK_MAXB and c.form != "tasks"
    # ROI tables larger than a CU's LDS: the band form declines whatever the map, one pooled row earlier it still has a (useless) budget
    c = by["declined_plane_band_tables"]
    assert RR.LDS_CU - 1024 - RR.plane_lds_bytes(0, c.shape[2], 16, RR.PLANE_CHUNK, c.PH - 1, c.PW, True) > 0
    assert RR.plane_band_geometry(c.shape[1], c.shape[2], c.PH, c.PW) is None and c.shape[1] * c.shape[2] * 16 > RR.PLANE_BUDGET


def test_inequalities_the_entry_cannot_make_false():
    """what the mirror's comments claim unreachable, over every shape the entry admits to those lines"""
    worst_tb = RR.sparse_lds_bytes(0, 16384, RR.SP_CH, 8, 8, True)
    assert worst_tb + 255 * 16 * 8 <= RR.SPARSE_LDS_MAX
    assert RR.SPARSE_LDS_MAX // 32 < 5 * RR.SP_NT and RR.TASKS_LDS_ALL // 32 < 5 * 1024      # the LDS bound binds before H * W <= 5 * 1024


@pytest.mark.parametrize("group", sorted(RR.GROUPS))
def test_every_forward_case_lands_on_the_form_it_names(group):
    cases = RR.fwd_cases(group)
    forms = set()
    for c in cases:
        p = RR.check_fwd_plan(c)
        forms.add(p.form)
        nimg = c.shape[0]
        img = c.rois[:, 0].astype(np.int64)
        assert c.R == 0 or (0 <= img.min() and img.max() < nimg)                             # no batch index outside [0, nimg)
        if c.layout == "grouped_gap":
            assert 1 not in set(img.tolist()) and np.all(np.diff(img) >= 0)
        if c.layout == "grouped":
            assert np.all(np.diff(img) >= 0) and len(set(img.tolist())) == nimg
    if group in ("forms", "values", "untouched", "chunks", "classes"):
        assert set(RR.FORMS) <= forms, (group, forms)


def test_chunk_cases_have_their_property():
    by = {c.name.split("/")[1]: c for c in RR.fwd_cases("chunks")}
    for fid in ("sparse_whole", "sparse_band", "tasks", "tasks_bands"):
        c = by[f"{fid}_one_class"]
        lv, hc, _, _ = RR.np_roi_classes(c.rois, RR.SCALE, c.PH, c.PW)
        per_image = np.bincount(c.rois[:, 0].astype(np.int64))
        assert len(set(zip(lv.tolist(), hc.tolist()))) == 1 and per_image.min() > RR.SP_CH    # one class, more than one chunk of it per image
    # grouped: the plane form's first chunk of 256 holds no ROI of the last image
    c = by["plane_bf16_cb4_grouped"]
    assert not (c.rois[:RR.PLANE_CHUNK, 0] == c.shape[0] - 1).any()
    # one workgroup per (slab, image): R = 1024 is the last single round of for_my_rois, 1025 the first of two, 2177 the first of three
    rounds = {}
    for name, c in by.items():
        if "_rounds_R" in name:
            p = c.plan()
            assert p.nz == 1 and p.n_chunks == -(-c.R // 128)
            rounds[name] = RR.sparse_rounds(p)
    assert rounds == {"sparse_whole_rounds_R1023": 1, "sparse_whole_rounds_R1024": 1, "sparse_whole_rounds_R1025": 2,
                      "sparse_whole_rounds_R2177": 3, "sparse_band_rounds_R1025": 2}
    # plane forms with fewer workgroups than chunks: a first chunk without a ROI of the workgroup's image before one with (grouped), a
    # second chunk worked on after a first (interleaved); whole plane with and without keys, and row bands
    walked = set()
    for name, c in by.items():
        if "_walk_" in name:
            p = c.plan()
            walks = RR.plane_walks(c, p)
            assert p.nz < p.n_chunks and c.R >= 3 * RR.PLANE_CHUNK
            if c.layout == "interleaved":
                assert all(len(w) < 2 or (w[0] > 0 and w[1] > 0) for w in walks.values()) and any(len(w) > 1 for w in walks.values())
            else:
                assert any(w[0] == 0 and any(w[1:]) for w in walks.values()), name
            if c.layout == "grouped_gap":
                assert all(not any(w) for (img, _), w in walks.items() if img == 1)
            walked.add((p.form, p.key, c.layout))
    assert walked == {(f, k, l) for f, k in (("plane", False), ("plane", True), ("plane_band", True)) for l in ("interleaved", "grouped", "grouped_gap")}


@pytest.mark.parametrize("index", range(len(RR.fwd_cases("classes"))), ids=[c.name for c in RR.fwd_cases("classes")])
def test_class_cases_hold_every_class_and_placement(index):
    c = RR.fwd_cases("classes")[index]
    nimg, H, W, C = c.shape
    plan = c.plan()
    lv, hc, wc, narrow = RR.np_roi_classes(c.rois, RR.SCALE, c.PH, c.PW)
    assert set(lv.tolist()) == set(range(RR.SP_NLEV)) and set(hc.tolist()) == set(range(RR.SP_NHC)) == set(wc.tolist())
    assert set(RR.LEVEL_WIDTHS) <= set(narrow.tolist())
    sw, _, ew = RR.roi_extent(c.rois[:, 1], c.rois[:, 3], RR.SCALE)
    sh, _, eh = RR.roi_extent(c.rois[:, 2], c.rois[:, 4], RR.SCALE)
    for P, e in ((c.PH, eh), (c.PW, ew)):                                                     # one below, on and above every class boundary
        assert set(RR.class_extents(P)) <= set(e.tolist())
        b = e.astype(np.float32) / np.float32(P)
        for bound in RR.SIZE_BOUNDS:
            assert (b == bound).any() and (b < bound).any() and (b > bound).any()
    assert (sh + eh <= 0).any() and (sh >= H).any() and (sw + ew <= 0).any() and (sw >= W).any()      # wholly outside, four sides
    assert ((sh < 0) & (sh + eh > 0)).any() and ((sh < H) & (sh + eh > H)).any() and ((sw < 0) & (sw + ew > 0)).any() and ((sw < W) & (sw + ew > W)).any()
    assert (c.rois[:, 3] < c.rois[:, 1]).any() and (c.rois[:, 4] < c.rois[:, 2]).any() and (ew == 1).any() and (eh == 1).any()
    over = set(RR.overshoot_heights(c.PH))                                                        # (none for a pooled height of 4: h / 4 is exact)
    assert not over or any(int(h) in over and int(s + h) == H for s, h in zip(sh, eh))          # overshoot ending on the map's last row
    if plan.n_bands > 1:
        S = plan.S
        for d in (-1, 0, 1):
            assert (sh == S + d).any()
        assert not over or any(int(h) in over and int(s + h) == S for s, h in zip(sh, eh))      # ... and on a band's last owned row
        assert ((sh <= 0) & (sh + eh >= H)).any()                                               # spanning every band
    # the level cap: a window on the map wider than twice the widest span
    _, arg = RR.roi_pool_fwd(np.zeros((nimg, 1, H, W), np.float32), c.rois[:40], RR.SCALE, c.PH, c.PW)
    ref_arg = O.roi_pool_fwd(np.zeros((nimg, 1, H, W), np.float32), c.rois[:40], RR.SCALE, c.PH, c.PW)[1]
    assert np.array_equal(arg, ref_arg)
    if W > 2 * 32 + 1 and c.PW == 7:
        ws, we = RR.bin_edges(int(sw[narrow >= 65][0]), int(ew[narrow >= 65][0]), c.PW, W)
        assert (we - ws).max() > 2 * 32


@pytest.mark.parametrize("index", range(len(RR.fwd_cases("values"))), ids=[c.name for c in RR.fwd_cases("values")])
def test_value_cases_tie_where_they_claim(index):
    c = RR.fwd_cases("values")[index]
    nimg, H, W, C = c.shape
    feat = c.feat()
    no_nan = np.where(np.isnan(feat), np.float32(1), feat)
    assert C >= 8 and np.array_equal(RR.round_to(no_nan, c.dtype), no_nan)                       # exact in the type
    kinds = {k: i for i, k in enumerate(RR.VALUE_CHANNELS)}
    assert np.isneginf(feat[0, kinds["-inf"]]).all() and np.isposinf(feat[0, kinds["+inf"]]).all()
    z = feat[0, kinds["signed_zero"]]
    assert np.signbit(z).any() and not np.signbit(z).all() and not z.any()
    for k in ("nan_rows", "neg_nan_cols"):
        assert np.isnan(feat[0, kinds[k]]).any()
    assert np.signbit(feat[0, kinds["neg_nan_cols"]][np.isnan(feat[0, kinds["neg_nan_cols"]])]).all()
    assert not np.signbit(feat[0, kinds["nan_rows"]][np.isnan(feat[0, kinds["nan_rows"]])]).any()
    # the NumPy restatement agrees with the oracle on this map, and the pairs tie: windows that hold BOTH maxima of a row, 2^L apart, exist
    # for every L the map is wide enough for, and name the first
    ch = kinds["pow2_pairs"]
    out, arg = RR.roi_pool_fwd(feat[:, ch:ch + 1], c.rois, RR.SCALE, c.PH, c.PW)
    ref_out, ref_arg = O.roi_pool_fwd(feat[:, ch:ch + 1], c.rois, RR.SCALE, c.PH, c.PW)
    assert np.array_equal(arg, ref_arg) and np.array_equal(out, ref_out)
    sw, _, ew = RR.roi_extent(c.rois[:, 1], c.rois[:, 3], RR.SCALE)
    sh, _, eh = RR.roi_extent(c.rois[:, 2], c.rois[:, 4], RR.SCALE)
    seen = set()
    for r in range(c.R - len(RR.pow2_boxes(H, W, c.PH, c.PW)), c.R):
        hs, he = RR.bin_edges(int(sh[r]), int(eh[r]), c.PH, H)
        ws, we = RR.bin_edges(int(sw[r]), int(ew[r]), c.PW, W)
        for ph in range(c.PH):
            for pw in range(c.PW):
                win = feat[0, ch, hs[ph]:he[ph], ws[pw]:we[pw]]
                if win.size and he[ph] - hs[ph] == 1 and (win == 5.0).sum() == 2:
                    x = np.flatnonzero(win[0] == 5.0)
                    seen.add(int(x[1] - x[0]))
                    assert arg[r, 0, ph, pw] == hs[ph] * W + ws[pw] + x[0]
    assert {1 << L for L in range(6) if (2 << L) + 1 < W} <= seen, seen

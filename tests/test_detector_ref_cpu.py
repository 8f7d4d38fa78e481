"""CPU: the float64 restatements of tests/detector_ref.py against torch (conv2d, max_pool2d, interpolate, avg_pool2d x 4) and the C
ROIAlign oracle on the case inputs, the edges the case tables of tests/test_gpu_detector_kernels.py are named for (sampling grids and
both backward forms, scalar / vector path by C % V, partial stem tiles, ld > 5A), and the tolerance table detector_ref.E32
(recomputed here; `python tests/test_detector_ref_cpu.py` prints a fresh table)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import frcnn_oracle as FO  # noqa: E402
import detector_ref as D  # noqa: E402

# a wrong restatement is off by O(1); float32 against float64 of these formulas stays far below this at every case used
PIN = 1e-5


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


@pytest.fixture(scope="module")
def fresh():
    return D.fresh_table()


# ------------------------------------------------------------------------------------------------ restatements
def test_preprocess_ref_against_the_oracle_preprocess():
    img = D.preprocess_inputs(37, 50)
    ref, _ = FO.preprocess([img])
    o = D.preprocess_ref(img, 64, 64, FO.PIXEL_MEAN, FO.PIXEL_STD)
    assert D.same_bits(o[:37, :50, :3].transpose(2, 0, 1), ref[0, :, :37, :50].numpy())
    assert not o[37:].any() and not o[:, 50:].any() and not o[..., 3].any()
    t = torch.from_numpy(img).float()
    want = (t - torch.tensor(D.OTHER_MEAN).view(3, 1, 1)) / torch.tensor(D.OTHER_STD).view(3, 1, 1)
    assert D.same_bits(D.preprocess_ref(img, 37, 50, D.OTHER_MEAN, D.OTHER_STD)[..., :3].transpose(2, 0, 1), want.numpy())
    cases = D.PREPROCESS_CASES
    assert any(h < H and w < W for h, w, H, W, _, _ in cases) and any(h == H and w == W for h, w, H, W, _, _ in cases)
    assert any(h == 1 and w == 1 for h, w, _, _, _, _ in cases) and any(s != D.DEFAULT_STD for *_, s in cases)


@pytest.mark.parametrize("c", D.STEM_CASES)
def test_stem_ref_against_torch_conv2d(c):
    x, w, sc, sh = D.stem_inputs(*c, "f32")
    ref = D.stem_ref(x, w, sc, sh)
    t = F.relu(F.conv2d(_nchw(x[..., :3]).double(), torch.from_numpy(w).double(), None, stride=2, padding=3)
               * torch.from_numpy(sc).double().view(1, -1, 1, 1) + torch.from_numpy(sh).double().view(1, -1, 1, 1))
    assert ref.shape == (c[0], *D.stem_out_hw(c[1], c[2]), 64)
    assert D.rel_err(ref, _nhwc(t)) <= 1e-12
    assert 0.2 < float((ref == 0).mean()) < 0.8                  # the ReLU cuts: scales of both signs
    assert (sc < 0).any() and (sc > 0).any() and np.isnan(x[..., 3]).all()


def test_stem_cases_reach_full_partial_and_sub_filter_tiles():
    T = D.STEM_TILE
    out = [D.stem_out_hw(H, W) for H, W in D.STEM_HW]
    assert D.stem_out_hw(16, 16) == (T, T)                                              # exactly one tile
    assert any(oh % T and ow % T and oh > T and ow > T for oh, ow in out)              # partial tiles behind full ones, both axes
    assert any(H < 7 for H, W in D.STEM_HW)                                             # an image smaller than the filter
    assert any(((oh + T - 1) // T) * ((ow + T - 1) // T) > 1 for oh, ow in out) and {N for N, _, _ in D.STEM_CASES} == {1, 3}
    assert any(oh % T == 1 for oh, _ in out)                                            # a tile that holds a single row


@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("c", D.POOL_CASES)
def test_maxpool_ref_is_torch_max_pool2d_bit_for_bit(c, dtype):
    H, W, C = c
    for regime in D.POOL_REGIMES:
        x = D.pool_inputs(2, H, W, C, dtype, regime)
        want = _nhwc(F.max_pool2d(_nchw(x), kernel_size=3, stride=2, padding=1))
        got = D.maxpool_ref(x)
        assert D.same_bits(got, want), (c, dtype, regime)
        if regime == "negative":
            assert (got < 0).all()
        if regime == "special" and H * W > 1:
            assert np.isnan(got).any() or H * W <= 4
    if (H, W) == (35, 48):
        sp = D.maxpool_ref(D.pool_inputs(2, H, W, C, dtype, "special"))
        assert np.isnan(sp).any() and np.isneginf(sp).any() and (sp == 0).any()


def test_pool_and_copy_cases_reach_both_paths():
    for dtype in D.DTYPES:
        assert {D.takes_vector_path(C, dtype) for C in D.POOL_C} == {True, False}
        assert {D.takes_vector_path(C, dtype) for C in D.FPN_C} == {True, False}
        assert {D.takes_copy16_path(C, dtype) for C in D.SUB_C} == {True, False}
    assert D.takes_vector_path(12, "f32") and not D.takes_vector_path(12, "bf16")        # 12: vector for f32, scalar for bf16
    assert not D.takes_vector_path(64, "f32", misaligned=True) and not D.takes_copy16_path(16, "bf16", misaligned=True)
    assert any(H % 2 and W % 2 for H, W in D.SUB_HW) and (1, 1) in D.SUB_HW and (1, 1) in D.POOL_HW and (1, 1) in D.FPN_HW
    # more than one 256-thread block on both paths
    assert max(H * W * C for H, W, C in D.POOL_CASES) // 4 // 8 > 256 and max(4 * h * w * C for h, w, C in D.FPN_CASES) // 8 > 256


@pytest.mark.parametrize("c", D.FPN_CASES)
def test_fpn_join_refs_against_torch(c):
    h, w, C = c
    for N in D.FPN_N:
        top = D.dense_inputs(43, (N, h, w, C), "f32"); lat = D.dense_inputs(44, (N, 2 * h, 2 * w, C), "f32")
        want = lat + _nhwc(F.interpolate(_nchw(top), scale_factor=2.0, mode="nearest"))
        assert D.same_bits(D.upsample_add_ref(lat, top, "f32"), want)
        g = D.dense_inputs(45, (N, 2 * h, 2 * w, C), "f32")
        want = _nhwc(F.avg_pool2d(_nchw(g).double(), 2) * 4)
        assert D.rel_err(D.downsample_sum_ref(g), want) <= 1e-14
        assert D.rel_err(D.downsample_sum_f32(g), want) <= 1e-6
        # the adjoint pair in float64
        up = np.repeat(np.repeat(top.astype(np.float64), 2, 1), 2, 2)
        assert abs(float((up * g).sum()) - float((top * D.downsample_sum_ref(g)).sum())) <= 1e-9 * float(np.abs(up * g).sum())


def test_subsample_scatter_and_add_relu_refs_against_torch():
    for H, W, C in D.SUB_CASES:
        x = D.dense_inputs(41, (2, H, W, C), "f32")
        s = D.subsample_ref(x)
        assert np.array_equal(s, _nhwc(F.max_pool2d(_nchw(x), kernel_size=1, stride=2)))
        back = D.scatter_ref(s, H, W)
        assert back.shape == x.shape and np.array_equal(D.subsample_ref(back), s) and np.count_nonzero(back) == np.count_nonzero(s) == s.size
    for n in D.ADD_N:
        for dtype in D.DTYPES:
            a, b = D.add_inputs(n, dtype)
            ta, tb = (torch.from_numpy(v).to(D.torch_dtype(dtype)) for v in (a, b))
            for relu in (0, 1):
                want = (ta.float() + tb.float())
                want = (F.relu(want) if relu else want).to(D.torch_dtype(dtype)).float().numpy()
                got = D.add_relu_ref(a, b, relu, dtype)
                assert D.same_bits(got, want), (n, dtype, relu)
                if dtype == "f32":                               # torch's own float32 join
                    assert D.same_bits(got, (F.relu(ta + tb) if relu else ta + tb).numpy())
            if n >= 255:
                r = D.add_relu_ref(a, b, 1, dtype)
                assert np.isnan(r[3]) and np.isnan(r[7]) and np.isnan(r[n - 1]) and np.signbit(r[11]) and r[11] == 0 and r[19] == 0
                assert not np.signbit(r[13]) and not np.signbit(r[17])


# ------------------------------------------------------------------------------------------------ ROIAlign
def test_roi_set_reaches_every_grid_and_both_backward_forms():
    rois = D.roi_set()
    assert len(rois) == 60
    g = D.roi_geometry(rois, 7, 7, 0)
    assert set(D.ROI_GRIDS) <= set(g["grid_h"].tolist()) and set(D.ROI_GRIDS) <= set(g["grid_w"].tolist())
    pairs = set(zip(g["grid_h"].tolist(), g["grid_w"].tolist()))
    assert set(D.ROI_GRID_PAIRS) <= pairs
    # the geometry restated here is the recomputation the issue names: ceil(roi / pooled) in float32
    f = np.float32
    rh = (rois[:, 4] * f(0.25) - f(0.5)) - (rois[:, 2] * f(0.25) - f(0.5))
    assert np.array_equal(g["grid_h"], np.ceil(rh / f(7)).astype(np.int64))
    forms = [D.roi_bwd_form(g, i) for i in range(len(rois))]
    assert "axis" in forms and "sample" in forms
    by_form = {}
    for i, fm in enumerate(forms):
        by_form.setdefault(fm, set()).add((int(g["grid_h"][i]), int(g["grid_w"][i])))
    assert {(7, 7), (8, 8)} <= by_form["axis"] and {(8, 9), (9, 8), (9, 9), (12, 1)} <= by_form["sample"]
    # bin exactly equal to the grid, at 8 (register form, sample spacing exactly 1) and at 9 (first grid of the other form)
    eq = [(int(g["grid_h"][i]), forms[i]) for i in range(len(rois)) if g["bin_h"][i] == g["grid_h"][i] and g["bin_w"][i] == g["grid_w"][i]
          and g["grid_h"][i] > 0]
    assert (8, "axis") in eq and (9, "sample") in eq and (1, "axis") in eq
    x1, y1, x2, y2 = (rois[:, k] * 0.25 for k in (1, 2, 3, 4))
    W, H = D.ROI_W, D.ROI_H
    big = (g["grid_h"] == 8) | (g["grid_w"] == 8)
    assert (big & (x1 < -1) & (x2 > 0)).any() and (big & (x1 < W) & (x2 > W)).any()            # grid 8 across the left / right border
    assert (big & (y1 < -1) & (y2 > 0)).any() and (big & (y1 < H) & (y2 > H)).any()            # ... the top / bottom border
    assert ((x1 > W + 1) | (x2 < -2) | (y1 > H + 1) | (y2 < -2)).sum() >= 3                    # wholly outside
    assert ((x2 == x1) & (y2 == y1)).any()                                                     # zero area
    assert set(rois[:, 0].astype(int).tolist()) == set(range(D.ROI_N))
    # the other configurations: 14 x 14 halves the grids (register form only), 7 x 3 widens them, a fixed ratio of 2
    g14 = D.roi_geometry(rois, 14, 14, 0)
    assert {D.roi_bwd_form(g14, i) for i in range(len(rois))} == {"axis"} and int(g14["grid_h"].max()) == 6
    g73 = D.roi_geometry(rois, 7, 3, 0)
    assert int(g73["grid_w"].max()) > 20 and {D.roi_bwd_form(g73, i) for i in range(len(rois))} == {"axis", "sample"}
    g2 = D.roi_geometry(rois, 7, 7, 2)
    assert {D.roi_bwd_form(g2, i) for i in range(len(rois))} == {"axis", "sample"}              # bin > grid = 2: spacing above 1
    sel = D.roi_sel_shuffled()
    assert len(set(sel.tolist())) == len(sel) == 40 and not np.array_equal(sel, np.sort(sel))


@pytest.mark.parametrize("cfg", D.ROI_CONFIGS)
@pytest.mark.parametrize("C", D.ROI_C)
def test_roi_align_refs_against_the_c_oracle(C, cfg):
    """forward and backward, on the inputs of the GPU tests, within float32 rounding of the oracle's serial float32 loops"""
    PH, PW, sr = cfg
    rois = D.roi_set()
    for dtype in D.DTYPES:
        feat = D.roi_feat(C, dtype)
        o = FO.roi_align_fwd(feat.transpose(0, 3, 1, 2), rois, D.ROI_SCALE, PH, PW, sr)
        ref = D.roi_fwd_expected(C, cfg, dtype)
        assert ref.shape == o.shape and D.rel_err(o, ref) <= PIN
        g = D.roi_geometry(rois, PH, PW, sr)
        gone = (g["grid_h"] <= 0) | (g["grid_w"] <= 0)
        assert not ref[gone].any() and not o[gone].any()
        outside = [25, 26, 27]
        assert not ref[outside].any()
        gout = D.roi_gout(C, PH, PW, dtype)
        b = FO.roi_align_bwd(gout, rois, D.ROI_SCALE, (D.ROI_N, C, D.ROI_H, D.ROI_W), sr).transpose(0, 2, 3, 1)
        assert D.rel_err(b, D.roi_bwd_expected(C, cfg, dtype)) <= PIN
    # adjoint pair in float64: <fwd(feat), gout> == <feat, bwd(gout)>
    feat, gout = D.roi_feat(C, "f32").astype(np.float64), D.roi_gout(C, PH, PW, "f32").astype(np.float64)
    lhs = float((D.roi_fwd_expected(C, cfg, "f32") * gout).sum()); rhs = float((feat * D.roi_bwd_expected(C, cfg, "f32")).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), 1.0)


# ------------------------------------------------------------------------------------------------ RPN layout, column scaling
@pytest.mark.parametrize("c", D.RPN_CASES)
def test_rpn_layout_restatement(c):
    """the index restatement against the reshapes the reference applies to per-level NCHW head outputs (rpn.py:457-470: permute to
    (N, Hi*Wi*A) / (N, Hi*Wi*A, 4), concatenate the levels), and that unpack_bwd is its exact transpose"""
    N, A, hw, ld = c
    y, dl, dd, gl, gd = D.rpn_inputs(N, A, hw, ld)
    logits, deltas = D.rpn_unpack_ref(y, N, A, hw)
    lv_l, lv_d, r0 = [], [], 0
    for h in hw:
        blk = y[r0:r0 + N * h].reshape(N, h, ld); r0 += N * h                # pixels of this level, image-major
        lv_l.append(blk[:, :, :A].reshape(N, h * A)); lv_d.append(blk[:, :, A:5 * A].reshape(N, h * A, 4))
    assert np.array_equal(logits, np.concatenate(lv_l, 1)) and np.array_equal(deltas, np.concatenate(lv_d, 1))
    assert not np.isnan(logits).any() and not np.isnan(deltas).any()
    dy = D.rpn_unpack_bwd_ref(dl, dd, None, None, N, A, hw, ld)
    l2, d2 = D.rpn_unpack_ref(dy, N, A, hw)
    assert np.array_equal(l2, dl) and np.array_equal(d2, dd) and not dy[:, 5 * A:].any()
    assert int((dy != 0).sum()) == dl.size + dd.size
    only = D.rpn_unpack_bwd_ref(dl, None, gl, gd, N, A, hw, ld)
    assert not only[:, A:].any() and np.array_equal(D.rpn_unpack_ref(only, N, A, hw)[0], dl * gl)


def test_rpn_and_scale_cases_reach_their_edges():
    assert any(ld == 5 * A for _, A, _, ld in D.RPN_CASES) and any(ld > 5 * A for _, A, _, ld in D.RPN_CASES)
    assert any(len(hw) == 1 for _, _, hw, _ in D.RPN_CASES) and max(len(hw) for _, _, hw, _ in D.RPN_CASES) == 5
    assert any(D.rpn_rows(N, hw) * ld > 256 for N, _, hw, ld in D.RPN_CASES)
    assert any(s == 0 for _, _, s, _ in D.SCALE_BLOCK_CASES) and any(s == N for _, N, s, _ in D.SCALE_BLOCK_CASES)
    assert any(p > N for _, N, _, p in D.SCALE_BLOCK_CASES) and any(M * p > 4096 for M, _, _, p in D.SCALE_BLOCK_CASES)
    src, g0, g1 = D.scale_blocks_inputs(37, 15, 3, 16)
    want = torch.from_numpy(np.nan_to_num(src)) * torch.cat([torch.full((3,), float(g0)), torch.full((12,), float(g1)), torch.zeros(1)])
    assert D.same_bits(D.scale_blocks_ref(src, 15, 3, g0, g1), want.numpy())


# ------------------------------------------------------------------------------------------------ tolerance table
def test_float32_forms_stay_within_the_pin(fresh):
    for key, e in fresh.items():
        assert e <= PIN, (key, e)


def test_tolerance_table_is_current(fresh):
    """detector_ref.E32 against a fresh computation: the same keys, and every bar max(2e-5, 8 * e32) within a factor 2 of the fresh
    one (below the 2e-5 floor an e32 is rounding noise of this host's float32 kernels and decides nothing)"""
    assert set(fresh) == set(D.E32), (set(fresh) ^ set(D.E32))
    for key, e in fresh.items():
        a, b = max(D.BAR_FLOOR, D.BAR_FACTOR * e), D.bar(*key)
        assert a <= 2 * b and b <= 2 * a, (key, e, D.E32[key])
    assert D.bf16_half_ulp(1.0) == 2.0 ** -8 and D.bf16_half_ulp(1.99) == 2.0 ** -8 and D.bf16_half_ulp(150.0) == 0.5


if __name__ == "__main__":
    for key, e in sorted(D.fresh_table().items()):
        print(f"    {key!r}: {e:.2e},")

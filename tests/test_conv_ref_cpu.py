"""tests/conv_ref.py on the CPU: the float64 references against torch.nn.functional.conv2d and autograd, the restated dispatch on the
edges it has to tell apart, every case table reaching the edge it is named for, and the integer operands inside their exact range and
exercising every position.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as C


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("dil", (1, 2))
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 5), (1, 1, 1, 7, 2), (1, 2, 9, 5, 11)])
def test_references_equal_conv2d_and_autograd_in_float64(shape, dil):
    n, H, W, Cin, Cout = shape
    r = np.random.default_rng([1, *shape, dil])
    x, w, b = r.normal(size=(n, H, W, Cin)), r.normal(size=(Cout, Cin, 3, 3)), r.normal(size=Cout)
    dy = r.normal(size=(n, H, W, Cout))
    xt = _nchw(x).requires_grad_(True); wt = torch.from_numpy(w).requires_grad_(True)
    y = F.conv2d(xt, wt, torch.from_numpy(b), padding=dil, dilation=dil)
    gx, gw = torch.autograd.grad(y, (xt, wt), _nchw(dy))
    np.testing.assert_allclose(C.conv3x3(x, w, b, dil), y.detach().permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(C.conv_dgrad(dy, w, dil), gx.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(C.wgrad(x, dy, dil), gw.numpy(), rtol=0, atol=1e-12)
    mask = C.mask_ref((9,), n * H * W, Cin)
    want = gx.permute(0, 2, 3, 1).numpy() * 0.5 * np.isin(mask, [1.0]).reshape(n, H, W, Cin)        # of the five values only 1 is > 0
    np.testing.assert_allclose(C.conv_dgrad(dy, w, dil, mask, 0.5), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("hw", [(2, 2), (5, 4), (7, 9)])
def test_pool_reference_equals_max_pool2d(hw):
    y = np.random.default_rng([2, *hw]).normal(size=(2, hw[0], hw[1], 3))
    want = F.max_pool2d(_nchw(C.relu(y)), 2, 2).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(C.maxpool2x2s2(C.relu(y)), want) and want.shape[1:3] == C.pool_out_hw(*hw)


def test_fold_reference_and_the_float32_expectation():
    s = C.fold_slabs((1,), 3, 8, 2)
    old = C.old_gradient((1,), (2, 8, 3, 3)); sc = C.general_scale((1,), 2)
    want = s.astype(np.float64).sum(0).transpose(0, 2, 1).reshape(2, 8, 3, 3)
    assert np.array_equal(C.fold(s), want)
    assert np.array_equal(C.fold(s, sc, old), want * sc.astype(np.float64).reshape(2, 1, 1, 1) + old)
    got = C.scaled_f32(want, sc, old)
    assert got.dtype == np.float32 and np.abs(got - C.fold(s, sc, old)).max() <= 2.0 ** -20
    assert np.array_equal(C.scaled_f32(want, C.pow2_scale((1,), 2), old), C.fold(s, C.pow2_scale((1,), 2), old))       # exact
    # the slab layout [co][tap][ci] of a weight gradient folds to OIHW
    x, dy = C.wgrad_operands((1, 3, 4, 8, 2, 1))
    dw = C.wgrad(x, dy, 1)
    assert np.array_equal(C.fold(dw.reshape(2, 8, 9).transpose(0, 2, 1)[None]), dw)


def test_bar_formula():
    ref, S = np.array([2.0, 0.0]), np.array([8.0, 4.0])
    a = C.allowed(ref, S, 576, "bf16")
    assert a[0] == 2.0 ** -8 * 2.0 + 2 * 578 * 2.0 ** -24 * 8.0 and a[1] == 2 * 578 * 2.0 ** -24 * 4.0
    assert C.allowed(ref, S, 576, "f32")[0] == 2.0 ** -23 * 2.0 + 2 * 578 * 2.0 ** -24 * 8.0
    assert C.worst(ref + 0.5 * a, ref, S, 576, "bf16") == pytest.approx(0.5) and C.worst(ref, ref, S, 576, "bf16") == 0.0
    assert C.worst(np.array([np.nan, 0.0]), ref, S, 576, "bf16") == np.inf


# ------------------------------------------------------------------------------------------------ the direct kernel's tables
def test_direct_tables_reach_every_form_at_both_dilations():
    for form, cases in C.DIRECT_FAMILIES.items():
        assert {C.conv_direct_form(*c[:5]) for c in cases} == {form}
        assert {c[5] for c in cases} == {1, 2}
        assert {c[5] for c in C.DIRECT_GAUSS if C.conv_direct_form(*c[:5]) == form} == {1, 2}
        assert sum(C.conv_direct_form(*c[:5]) == form for c in C.X3_CASES) == 1
    assert all(c in C.DIRECT_CASES and c[3] % 6 == 0 for c in C.X3_CASES)
    assert {C.conv_direct_form(*c) for c in C.FIRST_CASES_SHAPES} == {"first"}
    assert all(C.conv_direct_form(2, 19, 23, ci, co) is None for ci, co in C.IGEMM_BF16_CH)


def test_direct_tables_reach_the_edge_forms():
    cen = {c: C.direct_census(*c[:5]) for c in C.DIRECT_CASES}
    for form, cases in C.DIRECT_FAMILIES.items():
        assert any(cen[c]["left_wgs"] for c in cases) and any(cen[c]["empty_waves"] for c in cases), form
        assert any(cen[c]["mod8"] for c in cases), form
        assert any(0 < cen[c]["left_wgs"] < cen[c]["total"] for c in cases), form                  # LEFT next to FULL tile columns
    assert {cen[c]["chunks"] for c in C.DIRECT_KGROUP} >= {1, 2, 3}                                # per K group (odd and even)
    assert {cen[c]["chunks"] for c in C.DIRECT_TILE32} >= {3, 5, 7} and {cen[c]["chunks"] for c in C.DIRECT_FOURWAVE64} >= {2, 3, 4}
    assert any(cen[c]["cout_tail"] == 8 and cen[c]["tn"] == 32 for c in C.DIRECT_TILE32)
    assert any(cen[c]["cout_tail"] == 8 and cen[c]["tn"] == 64 for c in C.DIRECT_KGROUP + C.DIRECT_FOURWAVE64)
    assert any(c[4] == 8 for c in C.DIRECT_KGROUP) and any(c[4] == 8 for c in C.DIRECT_TILE32)
    big = cen[(1, 50, 200, 64, 520, 1)]
    assert big["total"] == 441 and big["idle"] == 7 and big["left_wgs"] and big["cout_tail"] == 8
    assert big["empty_waves"] == 3 * big["tiles_x"] * big["n_co_blocks"]                           # the bottom tile row: rows 48, 49
    assert cen[(1, 50, 215, 96, 456, 2)]["chunks"] == 3 and 215 % 32 > 16                          # a ragged FULL column
    assert all(cen[c]["total"] > 384 for c in C.DIRECT_FOURWAVE64) and any(c[0] == 3 for c in C.DIRECT_FOURWAVE64)    # the image index
    assert all(cen[c]["total"] <= 384 or cen[c]["form"] == "fourwave64" for c in C.DIRECT_CASES)
    one = C.direct_census(1, 9, 16, 128, 64)
    assert (one["left_wgs"], one["empty_waves"], one["total"]) == (2, 6, 2)                        # 16 columns; rows 8 of the second tile row only


def test_pool_cases_lie_on_both_sides_of_384():
    n, H, W, Cin, Cout = C.POOL_COVERED
    assert C.pool_fused_covered(*C.POOL_COVERED) and H % 2 and W % 2
    assert (-(-W // 32)) * (-(-H // 8)) * n * (Cout // 64) == 392
    assert not any(C.pool_fused_covered(*c) for c in C.POOL_REFUSED)
    assert C.POOL_REFUSED[0][4] % 64 == 0 and C.POOL_REFUSED[1][4] % 64 == 8


def test_multi_lists_and_their_range_tables():
    p8 = [c[:5] for c in C.MULTI_8]
    assert C.multi_covered(p8) and len(p8) == 8
    assert C.multi_first(p8) == [0, 24, 40, 48, 56, 64, 72, 80, 88]
    totals = [C._census(*p, "multi", 1, 64)["total"] for p in p8]
    assert any(t % 8 for t in totals) and any(t % 8 == 0 for t in totals)
    assert {p[3] for p in p8} == {64, 96, 128, 256} and {p[4] for p in p8} == {8, 64, 72, 256}
    assert {c[5] for c in C.MULTI_8} == {"relu", "mask", "plain"}
    assert [p[:3] for p in p8] == [(2, 40, 56), (2, 20, 28), (2, 10, 14), (2, 5, 7), (1, 1, 1), (1, 8, 32), (1, 9, 33), (3, 7, 17)]
    assert C.multi_covered([c[:5] for c in C.MULTI_SHARED]) and C.conv_direct_form(*C.MULTI_SHARED[0][:5]) == "fourwave64"
    assert not C.multi_covered([c[:5] for c in C.MULTI_CIN32]) and any(c[3] == 32 for c in C.MULTI_CIN32)
    assert len(C.MULTI_9) == 9 and not C.multi_covered([c[:5] for c in C.MULTI_9])
    ops_ = C.multi_operands("shared_weight")
    assert np.array_equal(ops_[0]["w"], ops_[1]["w"])
    ops8 = C.multi_operands("eight")
    assert not np.array_equal(ops8[2]["w"][:, :64], ops8[7]["w"][:, :64])                          # distinct weights


def test_first_layer_cases_reach_segment_and_grid_edges():
    cnt = {c: C.first_layer_counts(*c) for c in C.FIRST_CASES}
    assert any(c[2] < 16 for c in C.FIRST_CASES) and any(c[1] == 1 for c in C.FIRST_CASES)
    assert {c[2] for c in C.FIRST_CASES} >= {64, 65} and {v["segs"] for v in cnt.values()} >= {1, 2, 3}
    assert any(v["last_width"] == 1 for v in cnt.values()) and any(v["last_width"] == 64 for v in cnt.values())
    big = cnt[(1, 16500, 5)]
    assert big["nseg"] == 16500 > 4 * 4096 and big["blocks"] == 4096 and big["turns"] == 2
    assert all(v["turns"] == 1 for c, v in cnt.items() if c != (1, 16500, 5))
    assert any(v["nseg"] % 4 for v in cnt.values())                                                # a block with idle waves
    for c in C.FIRST_CASES:
        assert (C.first_operands(c)["x"] != 0).all()


def test_igemm_fallback_cases():
    assert C.IGEMM_BF16_CH == [(8, 32), (16, 24), (32, 64), (48, 40), (72, 64), (64, 12)]
    assert all(C.igemm_refusal("bf16", ci) is None for ci, _ in C.IGEMM_BF16_CH)
    assert all(C.igemm_refusal("f32", ci) is None for ci in C.IGEMM_F32_CIN)
    assert C.igemm_refusal("bf16", C.IGEMM_REFUSED_BF16[3]) == 5
    assert {ci % 64 == 0 for ci, _ in C.IGEMM_BF16_CH} == {True, False} and {ci % 32 == 0 for ci in C.IGEMM_F32_CIN} == {True, False}
    assert any(co % 8 for _, co in C.IGEMM_BF16_CH) and any(co % 4 == 0 and co % 8 for co in C.IGEMM_F32_COUT)


# ------------------------------------------------------------------------------------------------ weight gradients
def test_weight_gradient_cases_reach_their_edges():
    assert C.gather_admits(33, 1) and not C.gather_admits(32, 1)
    assert any(c[:3] == (1, 33, 1) for c in C.WGRAD_CASES) and C.WGRAD_REFUSED[:3] == (1, 32, 1)
    assert all(C.gather_admits(c[1], c[2]) for c in C.WGRAD_CASES)
    n, H, W = 1, 5, 13
    over = [c for c in C.WGRAD_CASES if c[6] > -(-c[0] * c[1] * c[2] // 64)]
    assert over and all(C.nslab("bf16", *c[:3], c[6]) == -(-c[0] * c[1] * c[2] // 64) for c in over)
    assert C.nslab("bf16", 2, 19, 23, 3) == 3 and C.nslab("f32", 1, 5, 13, 40) == 3 and C.nslab("bf16", 1, 5, 13, 40) == 2
    assert {c[7] for c in C.WGRAD_CASES} == {None, "pow2", "general"} and {c[8] for c in C.WGRAD_CASES} == {True, False}
    assert {c[5] for c in C.WGRAD_CASES} == {1, 2}
    for c in C.GROUPED_DIRECT:
        assert C.wgrad_direct_taken("bf16", [c]), c
    assert C.wgrad_direct_taken("bf16", C.GROUPED_DIRECT) and C.wgrad_direct_taken("bf16", [C.GROUPED_GAUSS])
    assert C.wgrad_direct_steps(1, 8, 1) == 8 and C.GROUPED_DIRECT[0][6] == 1                       # the eight-step minimum
    assert {c[5] for c in C.GROUPED_DIRECT} == {1, 2} and any(c[2] % 32 == 1 for c in C.GROUPED_DIRECT)
    for dtype, c in C.GROUPED_IGEMM:
        assert not C.wgrad_direct_taken(dtype, [c]) and C.gather_admits(c[1], c[2]), c
    why = [(d, c[1] < 8, c[4] % 64 != 0, -(-C.wgrad_direct_steps(*c[:3]) // C.nslab(d, *c[:3], c[6])) < 8) for d, c in C.GROUPED_IGEMM]
    assert why == [("bf16", True, False, False), ("bf16", False, True, False), ("f32", False, False, False), ("bf16", False, False, True)]


def test_small_weight_gradient_cases():
    assert C.SMALL_MAPS == [(1, 1), (1, 5), (2, 2), (4, 4), (7, 3)] and C.SMALL_N == (1, 2)
    n, H, W, Cin, Cout = C.SMALL_LARGE
    assert (Cout, Cin) == (1024, 1028) and Cout * Cin > C.SMALL_GRID and n * H * W <= 4096
    assert (C.SMALL_CIN * 2) % 16 and (C.SMALL_COUT * 2) % 16


def test_fold_cases_reach_every_loop_and_parts_edge():
    assert {c[0] for c in C.FOLD_CASES} >= {1, 7, 8, 9, 16, 17}
    assert {c[0] < C.FOLD_UNROLL for c in C.FOLD_CASES} == {True, False} and any(c[0] % C.FOLD_UNROLL == 0 for c in C.FOLD_CASES)
    assert {c[1] for c in C.FOLD_CASES} >= {4, 8, 36, 64, 72, 256, 1820} and {c[2] for c in C.FOLD_CASES} >= {1, 8, 64, 1024}
    assert all(C.fold_accepts(c[1]) for c in C.FOLD_CASES) and not C.fold_accepts(C.FOLD_REFUSED_CIN) and C.FOLD_REFUSED_CIN % 4 == 0
    assert C.fold_accepts(1820) and 36 * 1820 == 65520
    pr = {C.fold_parts(c[1], c[2]) for c in C.FOLD_CASES}
    assert {p for p, _ in pr} == {1, 2, 4, 8}
    assert {why for _, why in pr} == {"cout", "divide", "size"} and {why for p, why in pr if p > 1} == {"cout", "divide", "size"}
    assert C.fold_parts(64, 8) == (2, "size") and C.fold_parts(72, 8) == (2, "divide") and C.fold_parts(256, 256) == (4, "cout")
    assert {c[3] for c in C.FOLD_CASES} == {None, "pow2", "general"} and {c[4] for c in C.FOLD_CASES} == {True, False}
    assert len(C.FOLD_MULTI) == 35 > C.FOLD_MAX
    lds = [36 * ci // C.fold_parts(ci, co)[0] for ci, co, _ in C.FOLD_MULTI]
    assert len(set(lds[:C.FOLD_MAX])) > 2 and len(set(lds[C.FOLD_MAX:])) > 1                        # each launch mixes LDS sizes
    assert all(C.fold_accepts(ci) for ci, _, _ in C.FOLD_MULTI)


def test_weight_prep_cases():
    assert any(pad > ci for _, ci, pad in C.PREP_CASES) and any(pad == ci for _, ci, pad in C.PREP_CASES)


# ------------------------------------------------------------------------------------------------ the integer operands
def _exact_range(refs_bf16, abs_sum):
    for r in refs_bf16:
        assert np.abs(r).max() <= 256, np.abs(r).max()
    assert abs_sum.max() < 2 ** 24
    for r in refs_bf16:
        assert np.array_equal(2 * r, np.round(2 * r))                                               # integers (halves behind ref_scale = 0.5)


def _positions(x, w, mask=None):
    assert w.any(axis=0).all(), "a (ci, tap) without a non-zero weight"
    assert x.reshape(-1, x.shape[-1]).any(axis=1).all(), "an input pixel that is zero in every channel"
    if mask is not None:
        bits = set(np.unique(mask.view(np.int32)).tolist()) - {np.float32(np.nan).view(np.int32).item()}
        assert np.isnan(mask).any() and bits == {np.float32(v).view(np.int32).item() for v in (-1.0, -0.0, 0.0, 1.0)}


@pytest.mark.parametrize("case", C.DIRECT_CASES, ids=C.case_id)
def test_direct_integer_cases_are_exact_and_exercise_every_position(case):
    o = C.direct_int_operands(case)
    r = C.direct_int_refs(case)
    S = C.conv3x3(np.abs(o["x"]), np.abs(o["w"]), np.abs(o["bias"]), case[5])
    Sd = C.conv3x3(np.abs(o["x"]), np.abs(C.dgrad_weights(o["wd"])), None, case[5])
    _exact_range([r["fwd"], r["plain"], r["dgrad"]], np.maximum(S, Sd))
    _positions(o["x"], o["w"], o["mask"]); _positions(o["x"], C.dgrad_weights(o["wd"]))
    assert set(np.unique(o["x"])) == {-2, -1, 0, 1, 2} and set(np.unique(o["w"])) <= {-1, 0, 1} and np.abs(o["bias"]).max() <= 3
    if r["fwd"].size > 64:
        assert (r["fwd"] == 0).any() and (r["fwd"] > 0).any()                                       # the ReLU cuts


def test_six_product_operands_are_exact():
    for case in C.X3_CASES:
        o = C.x3_operands(case)
        xb = torch.from_numpy(o["x"]).to(torch.bfloat16).float().numpy()
        assert (xb != o["x"]).any(), "no operand needs a second bf16 piece"
        assert np.array_equal(torch.from_numpy(o["x"] - xb).to(torch.bfloat16).float().numpy(), o["x"] - xb)       # two pieces suffice
        y = C.conv3x3(o["x"], o["w"], o["bias"], case[5])
        assert np.array_equal(y * 512, np.round(y * 512)) and np.abs(y).max() < 2 ** 15
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
        _positions(o["x"], o["w"], o["mask"])
        wb = torch.from_numpy(o["w2"]).to(torch.bfloat16).float().numpy()
        assert (wb != o["w2"]).any() and np.array_equal(torch.from_numpy(o["w2"] - wb).to(torch.bfloat16).float().numpy(), o["w2"] - wb)
        y2 = C.conv3x3(o["x_int"], o["w2"], None, case[5])
        assert np.array_equal(y2 * 512, np.round(y2 * 512)) and np.abs(y2).max() < 2 ** 15
        _positions(o["x_int"], o["w2"])


def test_other_integer_cases_are_exact_and_exercise_every_position():
    n, H, W, Cin, Cout = C.POOL_COVERED
    o = C.direct_int_operands(C.POOL_COVERED + (1,))
    _positions(o["x"], o["w"])
    for name in C.MULTI_LISTS:
        for o in C.multi_operands(name):
            if o["x"].size < 10 ** 6:
                _exact_range([C.multi_ref(o)], C.conv3x3(np.abs(o["x"]), np.abs(o["w"]), np.abs(o["bias"]), 1))
            _positions(o["x"], o["w"], o["mask"])
    for c in C.FIRST_CASES[:-1]:
        o = C.first_operands(c)
        _exact_range([C.conv3x3(o["x"], o["w"], o["bias"], 1)], C.conv3x3(np.abs(o["x"]), np.abs(o["w"]), np.abs(o["bias"]), 1))
        _positions(o["x"], o["w"])
    for (ci, co) in C.IGEMM_BF16_CH:
        for m in C.IGEMM_MAPS:
            o = C.igemm_operands(*m, ci, co)
            _exact_range([C.igemm_ref(o, v, 2 if v == "dil2" else 1) for v in C.IGEMM_VARIANTS],
                         C.conv3x3(np.abs(o["x"]), np.abs(o["w"]), np.abs(o["bias"]), 1))
            _positions(o["x"], o["w"], o["mask"])
            half = C.igemm_ref(o, "ref_scale", 1)
            assert np.array_equal(torch.from_numpy(half).to(torch.bfloat16).double().numpy(), half)  # halves of integers <= 256
    o = C.igemm_operands(*C.IGEMM_DIRECT_SHAPE)
    _exact_range([C.igemm_ref(o, v, 1) for v in ("pitched_mask", "ref_scale")], C.conv3x3(np.abs(o["x"]), np.abs(o["w"]), None, 1))
    _positions(o["x"], o["w"], o["mask"])
    for c in C.WGRAD_CASES + [d + (None, False) for d in C.GROUPED_DIRECT] + [d + (None, False) for _, d in C.GROUPED_IGEMM]:
        x, dy = C.wgrad_operands(c)
        assert C.wgrad(np.abs(x), np.abs(dy), c[5]).max() < 2 ** 24
        assert x.reshape(-1, x.shape[-1]).any(axis=1).all() and dy.reshape(-1, dy.shape[-1]).any(axis=1).all()
    for (ns, ci, co, sk, acc) in C.FOLD_CASES:
        assert np.abs(C.fold_slabs((ns, ci, co), ns, ci, co)).sum(0).max() < 2 ** 24

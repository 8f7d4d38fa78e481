"""CPU: the restatements of tests/elementwise_ref.py against torch (max_pool2d forward and backward with NaN, +-inf, +-0 and ties,
F.relu's backward, .to(bfloat16), torch.optim.SGD in float64, permute expressions, oracle.semisup_oracle.update_teacher), and the
case tables of tests/test_gpu_elementwise_kernels.py against the dispatch predicates of csrc/elementwise.hip restated here: every
table must reach both outcomes of the predicate it is named for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as E


# ------------------------------------------------------------------------------------------------ 2x2 max pool
@pytest.mark.parametrize("regime", E.POOL_REGIMES)
@pytest.mark.parametrize("stride", E.POOL_STRIDES)
@pytest.mark.parametrize("hw", E.POOL_HW, ids=[f"{h}x{w}" for h, w in E.POOL_HW])
def test_maxpool_restatement_is_max_pool2d_forward_indices_and_backward(hw, stride, regime):
    H, W = hw
    for dtype in E.DTYPES:
        x = E.pool_inputs(H, W, 12, dtype, regime)
        xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        yt, idx = F.max_pool2d(xt, 2, stride, return_indices=True)
        got, am = E.maxpool_fwd_ref(x, stride)
        assert E.same_bits(got, yt.detach().permute(0, 2, 3, 1).numpy())
        OH, OW = E.pool_out_hw(H, W, stride)
        oy, ox = np.arange(OH)[None, :, None, None], np.arange(OW)[None, None, :, None]
        flat = (oy * stride + (am >> 1)) * W + ox * stride + (am & 1)
        assert np.array_equal(flat, idx.permute(0, 2, 3, 1).numpy()), "the selected element is the one torch's indices name"
        dout = E.pool_dout(H, W, 12, stride, dtype)
        yt.backward(torch.from_numpy(dout).permute(0, 3, 1, 2))
        want = xt.grad.permute(0, 2, 3, 1).numpy()                 # float32 sums of up to four terms in output order
        assert E.same_bits(E.maxpool_bwd_ref(x, dout, stride, 0, "f32"), want)
        if regime != "nan":                                        # the masked form: the gradient of max_pool2d(relu(x)) where x > 0
            masked = E.maxpool_bwd_ref(x, dout, stride, 1, "f32")
            assert E.same_bits(masked, np.where(x > 0, want, np.float32(0)))
        if stride == 2 and (H % 2 or W % 2):
            assert not E.maxpool_bwd_ref(x, dout, stride, 0, dtype)[:, 2 * OH:].any() and not E.maxpool_bwd_ref(x, dout, stride, 0, dtype)[:, :, 2 * OW:].any()


def test_pool_inputs_hold_the_windows_they_are_named_for():
    for (H, W) in E.POOL_HW:
        for stride in E.POOL_STRIDES:
            w = E._pool_windows(E.pool_inputs(H, W, 12, "f32", "nan"), stride)          # (4, N, OH, OW, C)
            assert (w < 0).all(0).any(), "an all-negative window"
            assert (w[:, 1, :, :, 1] == 0.5).all(), "ties"
            z = w[:, 1, :, :, 2]
            assert ((z[0] == 0) & ~np.signbit(z[0]) & np.signbit(z[1])).any(), "+0 in front of -0"
            if z.shape[1] * z.shape[2] > 1:
                assert ((z[0] == 0) & np.signbit(z[0]) & ((z[1:] == 0) & ~np.signbit(z[1:])).any(0)).any(), "-0 in front of +0"
            assert np.isposinf(w).any() and np.isneginf(w).any() and np.isneginf(w).all(0).any(), "+-inf and an all -inf window"
            top = w[:, 0, 0, 0, :]                                                       # the top-left window of image 0
            for pos in range(4):
                assert np.isnan(top[pos, pos]) and np.isnan(top[:, pos]).sum() == 1
            assert np.isnan(top[[0, 3], 4]).all() and np.isnan(w[[1, 2], 1, 0, 0, 0]).all(), "two NaN in one window"
    assert not np.isnan(E.pool_inputs(5, 4, 8, "bf16", "inf")).any() and np.isfinite(E.pool_inputs(5, 4, 8, "bf16", "finite")).all()
    x = E.pool_inputs(4, 7, 8, "f32", "finite")
    assert (x < 0).any() and (x > 0).any(), "signed, not post-ReLU"


def test_pool_cases_reach_every_kernel():
    fwd = {(d, E.pool_fwd_form(C, d, mis)) for (_, _, _, C, mis) in E.POOL_CASES for d in E.DTYPES}
    bwd = {(d, E.pool_bwd_form(C, d, s, mis)) for (_, _, s, C, mis) in E.POOL_CASES for d in E.DTYPES}
    assert fwd == {(d, f) for d in E.DTYPES for f in ("vector", "scalar")}
    assert bwd == {(d, f) for d in E.DTYPES for f in ("window", "vector", "scalar")}
    for d in E.DTYPES:                                             # C % vn: both outcomes; the scalar form also with C % vn == 0
        assert {C % E.VEC[d] == 0 for (_, _, _, C, _) in E.POOL_CASES} == {True, False}
        assert any(mis and C % E.VEC[d] == 0 for (_, _, _, C, mis) in E.POOL_CASES)
    assert any(s == 2 and (H % 2 or W % 2) for (H, W, s, _, _) in E.POOL_CASES), "an odd last row / column at stride 2"
    assert min(E.POOL_C) >= 5, "pool_inputs uses channels 0..4"


# ------------------------------------------------------------------------------------------------ relu_bwd
def test_relu_bwd_rule_against_torch_and_cases():
    for dtype in E.DTYPES:
        for n in E.RELU_N:
            ref, g = E.relu_inputs(n, dtype)
            want = E.relu_bwd_ref(ref, g)
            x = torch.from_numpy(ref).requires_grad_(True)
            F.relu(x).backward(torch.from_numpy(g))
            t = x.grad.numpy()
            nan_ref = np.isnan(ref)
            # torch's threshold_backward is `x <= 0 ? 0 : g`: a NaN reference lets g through; the kernels' documented rule gives 0
            assert E.same_bits(want[~nan_ref].view(np.float32), t[~nan_ref])           # a NaN g passes (its payload is torch's)
            assert (want[nan_ref] == 0).all()
        ref, g = E.relu_inputs(4104, dtype)
        for s in E.RELU_SPECIALS:
            assert (E.bits(ref) == E.bits(np.float32(s))).any() or (np.isnan(s) and np.isnan(ref).any())
        assert np.isnan(g[np.asarray(ref) > 0]).any(), "a NaN gradient passes where ref > 0"
        assert {E.relu_bwd_form(n, dtype, m) for n in E.RELU_N for m in (False, True)} == {"vector", "scalar"}
        assert {n % E.VEC[dtype] == 0 for n in E.RELU_N} == {True, False}
    assert E.relu_inputs(1, "bf16")[0][0] == E.F32_MIN_NORMAL


# ------------------------------------------------------------------------------------------------ casts
def test_round_to_is_torch_bf16_cast_on_the_value_set():
    v = E.cast_values()
    assert len(v) == E.N_CAST_VALUES and not E.is_subnormal(v[:E.N_CAST_NORMAL]).any() and E.is_subnormal(v[E.N_CAST_NORMAL:]).all()
    b = E.round_to(v, "bf16")
    assert np.array_equal(b[:5], np.array([1.0, 1.015625, -1.0, -1.015625, np.inf], np.float32)), "ties to even both ways; overflow to inf"
    assert E.same_bits(b[5:10], v[5:10]) and np.signbit(b[6]) and not np.signbit(b[5])
    assert E.same_bits(b, torch.from_numpy(v).to(torch.bfloat16).float().numpy())
    # the last subnormal lies halfway between two bf16 subnormals (a 1 in bit 15, zeros below)
    assert (E.bits(v[12]) & 0xFFFF) == 0x8000


def test_convert_cases_reach_both_forms():
    forms = {}
    for (r, c, ls, ld, ms, md) in E.CONVERT_CASES:
        assert ls >= c and ld >= c
        forms.setdefault(E.convert_2d_form(c, ls, ld, ms, md), []).append((c % 4 == 0, ls % 4 == 0, ld % 4 == 0, ms == 0, md == 0))
    assert set(forms) == {"vec4", "scalar"}
    for k in range(5):                                             # each term of the predicate alone sends a case to the scalar form
        assert any(not t[k] and all(t[:k] + t[k + 1:]) for t in forms["scalar"]), k
    assert {(r, c) for (r, c, *_) in E.CONVERT_CASES} == {(3, 5), (3, 8), (64, 4)}
    for (rows, cols, add) in E.CONVERT_T_CASES:
        assert rows % 64 == 0 and cols % 64 == 0
    assert {frozenset(E.convert_t_row_forms(r, r + a, "bf16")) for (r, _, a) in E.CONVERT_T_CASES} == {frozenset({"vector"}), frozenset({"vector", "scalar"})}
    it = E.grid_items()
    assert all(E.GRID_CAP < v <= E.GRID_CAP + 1024 for v in it.values()), it
    p = E.GRID_POOL
    assert E.pool_fwd_form(p["C"], p["dtype"], False) == "vector" and E.relu_bwd_form(E.GRID_RELU_N, "f32", False) == "vector"
    assert E.convert_2d_form(E.GRID_CONVERT[1], E.GRID_CONVERT[1], E.GRID_CONVERT[1], 0, 0) == "vec4"


def test_layout_restatements_are_permute_expressions():
    for shape in E.WEIGHT_PREP_SHAPES:
        w = E.weight_matrix(1, shape + (3, 3))
        wt = torch.from_numpy(w)
        Cout, Cin = shape
        assert E.same_bits(E.weight_prep_ref(w, 0), wt.permute(0, 2, 3, 1).reshape(Cout, 9, Cin).numpy())
        assert E.same_bits(E.weight_prep_ref(w, 1), wt.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9, Cout).numpy())
        for pad in E.WEIGHT_PREP_PADS[shape]:
            got = E.weight_prep_ref(w, 0, pad)
            assert pad >= Cin and got.shape == (Cout, 9, pad) and not got[:, :, Cin:].any()
            if Cout * Cin < 100:
                assert E.same_bits(got, E.weight_prep_loops(w, 0, pad))
        if Cout * Cin < 100:
            assert E.same_bits(E.weight_prep_ref(w, 1), E.weight_prep_loops(w, 1))
        assert {pad == Cin for pad in E.WEIGHT_PREP_PADS[shape]} == {True, False}
    x = E.weight_matrix(2, E.NCHW_SHAPE)
    for cpad in E.NCHW_CPADS:
        got = E.nchw_to_nhwc_ref(x, cpad)
        assert E.same_bits(got[..., :3], torch.from_numpy(x).permute(0, 2, 3, 1).numpy()) and not got[..., 3:].any()
    bx = [np.arange(12, dtype=np.float32).reshape(3, 4) + 100 * v for v in range(4)]
    ob = [np.arange(3, dtype=np.float32) + 10 * v for v in range(4)]
    boxes, obj, rois = E.pack_views_ref(bx, ob)
    t = torch.from_numpy(np.stack(bx))
    want = torch.cat([torch.tensor([0., 1.]).view(1, 2, 1, 1).expand(2, 2, 3, 1), t.view(2, 2, 3, 4)], 3).reshape(2, 6, 5)
    assert np.array_equal(rois, want.numpy()) and np.array_equal(boxes, t.numpy()) and np.array_equal(obj, np.stack(ob))


def test_scale_cols_and_split_restatements():
    for (M, N, ld_in, ld_out) in E.SCALE_COLS_CASES:
        assert ld_in >= N and ld_out >= N
        src, cs = E.scale_cols_inputs(M, N, ld_in)
        p = E.scale_cols_ref(src, cs, N)
        want = (torch.from_numpy(src[:, :N].copy()) * torch.from_numpy(cs)).to(torch.bfloat16).float().numpy()
        assert E.same_bits(E.round_to(p, "bf16"), want)
        assert np.isnan(src[:, N:]).all() and E.is_subnormal(src[:, :N]).sum() == 3 and E.is_subnormal(p).any(), "subnormal inputs and products"
    assert any(li > N for (_, N, li, _) in E.SCALE_COLS_CASES) and any(lo > N for (_, N, _, lo) in E.SCALE_COLS_CASES)
    for (rows, cols) in E.SPLIT_SHAPES:
        a = E.cast_matrix(3, rows, cols, cols)
        assert E.is_subnormal(a).sum() == 3
        a1, a2, a3 = E.split_pieces_ref(a)
        for q in (a1, a2, a3):
            assert E.same_bits(q, E.round_to(q, "bf16"))
        fin = np.isfinite(a) & (np.abs(a) >= 2.0 ** -100) & (np.abs(a) < 1e38)
        assert fin.sum() >= a.size - E.N_CAST_VALUES               # the finite normal inputs
        with np.errstate(invalid="ignore"):
            s = a1.astype(np.float64) + a2.astype(np.float64) + a3.astype(np.float64)
        assert np.array_equal(s[fin], a.astype(np.float64)[fin]), "three bf16 pieces hold all 24 bits"
        assert (a3[fin] != 0).any()
        for side in (0, 1):
            L = E.split_layout_ref(a, side, 0)
            assert L.shape == (rows, 6 * cols)
            names = [(a1, a2, a3)[k] for k in E.SPLIT_PATTERNS[side]]
            for p_, q in enumerate(names):
                assert E.same_bits(L[:, p_ * cols:(p_ + 1) * cols], q)
            assert E.same_bits(E.split_layout_ref(a, side, 1).reshape(6, rows, cols), np.stack(names))
    # the six products of the two patterns are a1b1, a1b2, a2b1, a1b3, a2b2, a3b1: every pair with index sum <= 4 once
    pairs = sorted(zip(E.SPLIT_PATTERNS[0], E.SPLIT_PATTERNS[1]))
    assert pairs == sorted((i, j) for i in range(3) for j in range(3) if i + j <= 2)


# ------------------------------------------------------------------------------------------------ optimizer
def test_sgd_reference_is_torch_sgd_in_float64():
    r = np.random.default_rng(5)
    w = r.normal(size=300).astype(np.float32); buf = r.normal(size=300).astype(np.float32)
    lr, wd, mom, gs = 0.03, 5e-4, 0.9, 0.5
    f = lambda v: float(np.float32(v))
    p = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.SGD([p], lr=f(lr), momentum=f(mom), weight_decay=f(wd))
    wc, bc = w.astype(np.float64), None
    for step in range(3):
        g = r.normal(size=300).astype(np.float32)
        p.grad = torch.from_numpy(g.astype(np.float64) * f(gs))
        opt.step()
        wc, bc, S = E.sgd_ref(wc, g, bc, lr, wd, mom, gs, first=(step == 0))
        np.testing.assert_allclose(wc, p.detach().numpy(), rtol=1e-14, atol=1e-16)
        np.testing.assert_allclose(bc, opt.state[p]["momentum_buffer"].numpy(), rtol=1e-14, atol=1e-16)
        assert (S >= np.abs(bc) - 1e-12).all()


def test_sgd_bound_covers_float32_arithmetic_with_and_without_fma():
    r = np.random.default_rng(6)
    n = 200000
    worst = 0.0
    for first in (True, False):
        for (lr, wd) in ((0.01, 5e-4), (0.03, 0.0), (0.006, 6e-4)):
            draw = lambda: (r.normal(size=n) * np.exp(r.normal(0, 1.5, n))).astype(np.float32)
            w, g, buf = draw(), draw(), draw()
            pr, br, S = E.sgd_ref(w, g, buf, lr, wd, 0.9, 0.5, first)
            ab, ap = E.sgd_bounds(w, S, lr)
            for fma in (False, True):
                p32, b32 = E.sgd_f32(w, g, buf, lr, wd, 0.9, 0.5, first, fma)
                worst = max(worst, float(np.max(np.abs(b32 - br) / ab)), float(np.max(np.abs(p32 - pr) / ap)))
    assert 0.2 < worst <= 1.0, worst


def test_sgd_entries_reach_every_form_and_branch():
    es = E.sgd_entries()
    assert len(es) > E.SGD_MAX_TENSORS and len(es) <= 2 * E.SGD_MAX_TENSORS, "two launches"
    assert es[E.SGD_MAX_TENSORS - 1]["kind"] == 3, "a kind-3 entry (its own launch) at the boundary between the two batches"
    assert sum(int(np.prod(e["shape"])) == 0 for e in es) == 1
    assert {E.sgd_form(e) for e in es} == {"tile64", "conv_tile", "vector", "scalar"}
    el = [e for e in es if e["kind"] == 0 and e["shape"] != (0,)]
    assert {(e["shape"][0], e["mis"] % 4 == 0) for e in el} == {(n, a) for n in E.SGD_ELEMENT_N for a in (True, False)}
    assert {n % E.SGD_CHUNK for n in E.SGD_ELEMENT_N} >= {0, 1, E.SGD_CHUNK - 1} and any(n % 4 and n > E.SGD_CHUNK for n in E.SGD_ELEMENT_N)
    k1 = [e for e in es if e["kind"] == 1]
    assert {e["d0"] % 4 == 0 for e in k1} == {True, False} and any(e.get("f32") for e in k1)
    forms = [E.stage_row_forms(e, "bf16") for e in k1 if e["d0"] == 72 and not e.get("f32")]
    assert {"8B"} in forms and {"8B", "scalar"} in forms, "rows that start on 8 bytes, and a pitch whose odd rows do not"
    k2 = [e for e in es if e["kind"] == 2]
    assert any(E.sgd_form(e) != "conv_tile" for e in k2)
    tiled = [e for e in k2 if E.sgd_form(e) == "conv_tile"]
    assert {e["d1"] // 32 for e in tiled} >= {1, 2, 3}, "cib = 1 and more than one input-channel tile"
    assert any(e["d0"] // 32 > 1 and e["d1"] // 32 > 1 for e in tiled), "blk / cib and blk % cib both vary"
    assert any(e["d2"] > e["d1"] and e["s0"] for e in tiled), "a padded d2 pitch"
    assert {(e["s0"], e["s1"]) for e in tiled} == {(True, False), (False, True), (True, True)}
    k3 = [e for e in es if e["kind"] == 3]
    assert all(e["shape"][0] % 64 == 0 and e["d0"] % 64 == 0 for e in k3)
    assert {frozenset(E.convert_t_row_forms(e["shape"][0], e["ld1"], "bf16")) for e in k3} == {frozenset({"vector"}), frozenset({"vector", "scalar"})}
    assert {frozenset(E.stage_row_forms(e, "bf16")) for e in k3} == {frozenset({"8B"}), frozenset({"8B", "scalar"})}
    for i in range(len(es)):
        (lr, wd), (lr2, wd2) = E.sgd_hyper(i)
        assert np.float32(lr) != np.float32(lr2) and np.float32(wd) != np.float32(wd2)


def test_stage_kind2_ref_layouts():
    p = E.weight_matrix(4, (32, 64, 3, 3))
    s0, s1 = E.stage_kind2_ref(p, 72)
    assert s0.shape == (32, 9, 72) and np.isnan(s0[:, :, 64:]).all() and s1.shape == (64, 9, 32)
    assert s0[3, 5, 7] == p[3, 7, 1, 2] and s1[7, 8 - 5, 3] == p[3, 7, 1, 2]


# ------------------------------------------------------------------------------------------------ EMA
def test_ema_restatement_is_the_oracle_update_teacher():
    from oracle import semisup_oracle as SO
    te, st = E.ema_inputs()
    assert len(te) == E.EMA_COUNT > 48 and {t.size for t in te} == set(E.EMA_SIZES)
    assert np.isinf(te[E.EMA_INF_AT[0]][E.EMA_INF_AT[1]])
    for keep in E.EMA_KEEPS:
        ref = E.ema_ref(te, st, keep)
        with np.errstate(invalid="ignore"):
            o = SO.update_teacher({str(i): t for i, t in enumerate(te)}, {str(i): s for i, s in enumerate(st)}, keep)
            tt = [torch.from_numpy(s) * (1 - keep) + torch.from_numpy(t) * keep for t, s in zip(te, st)]
        for i in range(E.EMA_COUNT):
            assert E.same_bits(ref[i], o[str(i)]) and E.same_bits(ref[i], tt[i].numpy())
    assert np.isnan(E.ema_ref(te, st, 0.0)[E.EMA_INF_AT[0]][E.EMA_INF_AT[1]]), "inf * 0"
    assert E.same_bits(E.ema_ref(te, st, 1.0)[1], te[1]) and E.same_bits(E.ema_ref(te, st, 0.0)[1], st[1])


# ------------------------------------------------------------------------------------------------ scalars
def test_weighted_sum_order_matters_and_dropout_restatement():
    for n in E.WS_N:
        v, w = E.weighted_sum_inputs(n)
        ref = E.weighted_sum_ref(v, w)
        t = torch.zeros((), dtype=torch.float32)
        for i in range(n):                                         # Python's sum() over the weighted losses
            t = torch.tensor(v[i]) * float(w[i]) if i == 0 else t + torch.tensor(v[i]) * float(w[i])
        assert E.bits(ref[n]) == E.bits(t.numpy())
        if n >= 3:
            p = ref[:n]
            assert np.float32(np.float32(p[0] + p[2]) + np.float32(p[1:2].sum() + p[3:].sum())) != ref[n], "another order gives another sum"
            assert abs(float(ref[n]) - float(np.sum(p.astype(np.float64)))) > 0.5
    assert max(E.WS_N) == E.WS_MAX
    # splitmix64: the numpy uint64 form against Python integers
    for seed in E.DROPOUT_SEEDS:
        for off in (0, 5, 2 ** 64 - 2):
            s = E.splitmix64_int(seed)
            z = [E.splitmix64_int((s + off + i) & E._M64) for i in range(8)]
            for p in E.DROPOUT_P:
                want = [1 if np.float32(zz >> 40) * np.float32(2.0 ** -24) >= np.float32(p) else 0 for zz in z]
                assert list(E.dropout_ref(8, seed, off, p)) == want
    assert any(s >= 2 ** 63 for s in E.DROPOUT_SEEDS)
    assert E.dropout_ref(5000, 7, 0, 0.0).all() and not E.dropout_ref(5000, 7, 0, 1.0).any()
    assert abs(float(E.dropout_ref(70001, 7, 0, 0.3).mean()) - 0.7) < 0.01
    assert np.array_equal(E.dropout_ref(990, 7, 10, 0.3), E.dropout_ref(1000, 7, 0, 0.3)[10:])
    assert any(s < 2 ** 32 <= s + i for s, i in E.COUNTER_CASES) and any(s + i >= 2 ** 64 for s, i in E.COUNTER_CASES)
    assert {R % 256 == 0 for R in E.PACK_R} == {False} and max(E.PACK_R) * 4 > 1024, "more than one block, a ragged last one"


# ------------------------------------------------------------------------------------------------ NaN cases
def test_nan_cases_name_the_form_they_reach():
    want = {"first_layer": "first", "kgroup_bf16": "kgroup", "kgroup_f32": "kgroup", "fourwave_bf16": "fourwave32", "fourwave_f32": "fourwave32"}
    for k, (n, H, W, cin, cout, _) in E.NAN_CONV_CASES.items():
        assert E.conv_direct_form(n, H, W, cin, cout) == want[k]
    assert {c[5] for c in E.NAN_CONV_CASES.values()} == {"bf16", "f32"}
    n, H, W, cin, cout = E.NAN_POOL_CASE
    assert E.pool_fused_covered(n, H, W, cin, cout) and E.conv_direct_form(n, H, W, cin, cout) == "fourwave64"
    assert not E.pool_fused_covered(1, 48, 224, 64, 512)
    # the GEMM cases against the restated dispatch of sw_gemm / launch_auto
    want = {"pp256": "pp256", "256x64": "register", "fold": "fold"}
    for (site, M, N, K, idt, _, sk) in E.NAN_GEMM_CASES:
        assert E.gemm_relu_site(M, N, K, idt, sk) == want[site], site
        assert K % 8 == 0
    sites = {c[0]: c for c in E.NAN_GEMM_CASES}
    _, M, N, K, idt, _, sk = sites["pp256"]
    assert N > 128 and -(-M // 256) * -(-N // 256) >= 200 and K >= 1024 and K % 64 == 0 and idt == "bf16" and sk == 1
    assert sites["256x64"][2] <= 64 and sites["256x64"][6] == 1
    assert sites["fold"][6] > 1 and sites["fold"][2] % 4 == 0
    assert E.gemm_relu_site(3841, 3583, 1048, "bf16", 1) == "register" and E.gemm_relu_site(1025, 3583, 1024, "bf16", 1) == "register"

"""GPU: every form of the 3x3 convolution family against the float64 references of tests/conv_ref.py: the direct forward / data-gradient
kernel (two K groups, 32-channel tiles, four waves on 64-channel tiles; LEFT and EMPTY edge forms, odd chunk counts, 8-channel tails,
work lists that are no multiple of 8), its multi-problem launch, the first-layer kernel, the fused conv + ReLU + pool form
(csrc/conv_direct.hip), the implicit-GEMM fallback, the weight-gradient slabs and folds (csrc/gemm.hip), the direct weight-gradient
kernel (csrc/conv_wgrad_direct.hip) and the small-map weight gradient (csrc/proposals.hip).

Integer operands: every element equals the float64 reference cast to the output type (conv_ref's docstring: all sums are exact in
float32, whatever their order).  Gaussian operands: every element within its own bar u_out |ref| + 2 (K + 2) 2^-24 S, which comes from
the reference alone; max(err / allowed) is printed per case.  Every output lives in a buffer filled with a NaN whose payload no kernel
writes, with slack in front and behind: what the contract says is written is written, everything else (the slack, the whole output of
a refused launch) still holds the sentinel.  No element is masked and no case skipped; tests/test_conv_ref_cpu.py asserts that the
case tables reach the edges they are named for."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as C  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


_F32_SENTINEL, _BF16_SENTINEL = 0x7FA5A5A5, 0x7FA5


def _sent(n, dtype):
    if dtype == F32:
        return torch.full((n,), _F32_SENTINEL, device="cuda", dtype=torch.int32).view(F32)
    return torch.full((n,), _BF16_SENTINEL, device="cuda", dtype=torch.int16).view(BF16)


def _untouched(t):
    """bool tensor: the element still holds the sentinel bits"""
    if t.dtype == F32:
        return t.view(torch.int32) == _F32_SENTINEL
    return t.view(torch.int16) == _BF16_SENTINEL


class _Out:
    """an output of `shape` inside a sentinel-filled buffer: SLACK elements (a multiple of 16 bytes) in front and behind"""

    def __init__(self, shape, dtype, init=None):
        self.n = int(np.prod(shape))
        self.buf = _sent(self.n + 2 * C.SLACK, dtype)
        self.t = self.buf[C.SLACK:C.SLACK + self.n].view(*shape)
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))

    def _slack_intact(self):
        return bool(_untouched(self.buf[:C.SLACK]).all() and _untouched(self.buf[C.SLACK + self.n:]).all())

    def host(self):
        """CPU tensor of the output, after checking that nothing around it was written and all of it was"""
        torch.cuda.synchronize()
        assert self._slack_intact(), "written outside the output"
        assert not bool(_untouched(self.t).any()), "an element of the output was not written"
        return self.t.cpu()

    def assert_intact(self):
        torch.cuda.synchronize()
        assert bool(_untouched(self.buf).all()), "a refused launch wrote to its output"


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dtype).cuda()


def _wk(ops, w_oihw, mode, dtype, cin_pad=None):
    """the kernel layout of OIHW master weights, through sw_conv_weight_prep as the product does"""
    Cout, Cin = w_oihw.shape[:2]
    wk = torch.empty((Cout, 9, Cin if cin_pad is None else cin_pad) if mode == 0 else (Cin, 9, Cout), device="cuda", dtype=dtype)
    ops.conv_weight_prep(_dev(w_oihw, F32), wk, mode, cin_pad)
    return wk


def _assert_equal(got, ref, what=""):
    """every element of the CPU tensor `got` equals the float64 reference cast to its type"""
    want = torch.from_numpy(np.ascontiguousarray(ref)).to(got.dtype).view(got.shape)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: "
                             f"got {float(got[idx])}, want {float(want[idx])}")


def _assert_within(name, got, ref, S, K, out):
    w = C.worst(got.double().numpy().reshape(ref.shape), ref, S, K, out)
    print(f"GAUSS {name}: max(err / allowed) = {w:.4f}")
    assert w <= 1.0, f"{name}: an element is {w:.3g} x its bar"


def _ep(ops, dtype, bias=None, relu=False, mask=None, ref_scale=1.0):
    return ops.make_epilogue(bias=bias, relu=relu, relu_ref=mask, ref_scale=ref_scale, out_dtype=dtype)


# ------------------------------------------------------------------------------------------------ direct kernel, integer operands
@pytest.mark.parametrize("case", C.DIRECT_CASES, ids=C.case_id)
def test_direct_forms_bit_exact_with_integer_operands(ops, case):
    """forward (bias + ReLU, bf16), plain (f32), data-gradient form with a bf16 mask (bf16) and with an f32 mask (f32)"""
    n, H, W, Cin, Cout, dil = case
    o, r = C.direct_int_operands(case), C.direct_int_refs(case)
    x, bias = _dev(o["x"], BF16), _dev(o["bias"], F32)
    wk, wkd = _wk(ops, o["w"], 0, BF16), _wk(ops, o["wd"], 1, BF16)
    assert wkd.shape == (Cout, 9, Cin)
    out = _Out((n, H, W, Cout), BF16)
    ops.conv3x3(x, wk, out.t, dil, _ep(ops, BF16, bias, True))
    _assert_equal(out.host(), r["fwd"], "forward")
    out = _Out((n, H, W, Cout), F32)
    ops.conv3x3(x, wk, out.t, dil, _ep(ops, F32))
    _assert_equal(out.host(), r["plain"], "plain f32")
    out = _Out((n, H, W, Cout), BF16)
    ops.conv3x3(x, wkd, out.t, dil, _ep(ops, BF16, mask=_dev(o["mask"], BF16)))
    _assert_equal(out.host(), r["dgrad"], "dgrad bf16")
    out = _Out((n, H, W, Cout), F32)
    ops.conv3x3(x, wkd, out.t, dil, _ep(ops, F32, mask=_dev(o["mask"], F32)))
    _assert_equal(out.host(), r["dgrad"], "dgrad f32")


@pytest.mark.parametrize("case", C.X3_CASES, ids=C.case_id)
def test_direct_six_product_form_bit_exact(ops, case):
    """the bf16x3 convolution of f32 operands (three bf16 pieces each, K-concatenated: Cin = 6 x the layer's) on an input, then on
    weights, that need two pieces, with sums that stay exact in f32"""
    n, H, W, Cin6, Cout, dil = case
    cin = Cin6 // 6
    o = C.x3_operands(case)
    x, bias = _dev(o["x"], F32), _dev(o["bias"], F32)
    wk = _wk(ops, o["w"], 0, F32)
    wk3 = ops.split_bf16x3(wk.view(Cout * 9, cin), 1, out=torch.empty(Cout * 9, Cin6, device="cuda", dtype=BF16)).view(Cout, 9, Cin6)
    x3 = ops.split_bf16x3(x.view(n * H * W, cin), 0, out=torch.empty(n * H * W, Cin6, device="cuda", dtype=BF16)).view(n, H, W, Cin6)
    y = C.conv3x3(o["x"], o["w"], None, dil)
    out = _Out((n, H, W, Cout), F32)
    ops.conv3x3(x3, wk3, out.t, dil, _ep(ops, F32, bias, True))
    _assert_equal(out.host(), C.relu(y + o["bias"].astype(np.float64)), "forward")
    out = _Out((n, H, W, Cout), F32)
    ops.conv3x3(x3, wk3, out.t, dil, _ep(ops, F32, mask=_dev(o["mask"], F32)))
    _assert_equal(out.host(), y * C.relu_mask(o["mask"]).reshape(y.shape), "masked")
    # the weights in two pieces, the input in one
    wk = _wk(ops, o["w2"], 0, F32)
    wk3 = ops.split_bf16x3(wk.view(Cout * 9, cin), 1, out=torch.empty(Cout * 9, Cin6, device="cuda", dtype=BF16)).view(Cout, 9, Cin6)
    x = _dev(o["x_int"], F32)
    x3 = ops.split_bf16x3(x.view(n * H * W, cin), 0, out=torch.empty(n * H * W, Cin6, device="cuda", dtype=BF16)).view(n, H, W, Cin6)
    out = _Out((n, H, W, Cout), F32)
    ops.conv3x3(x3, wk3, out.t, dil, _ep(ops, F32))
    _assert_equal(out.host(), C.conv3x3(o["x_int"], o["w2"], None, dil), "two-piece weights")


@pytest.mark.parametrize("case", C.DIRECT_GAUSS, ids=C.case_id)
def test_direct_forms_within_the_per_element_bar(ops, case):
    n, H, W, Cin, Cout, dil = case
    o = C.direct_gauss_operands(case)
    x, bias = _dev(o["x"], BF16), _dev(o["bias"], F32)
    wk, wkd = _wk(ops, o["w"], 0, BF16), _wk(ops, o["wd"], 1, BF16)
    plain = C.conv3x3(o["x"], o["w"], None, dil)
    S = C.conv3x3(np.abs(o["x"]), np.abs(o["w"]), np.abs(o["bias"]), dil)
    K, name = 9 * Cin, f"direct[{C.conv_direct_form(*case[:5])}] {C.case_id(case)}"
    out = _Out((n, H, W, Cout), BF16)
    ops.conv3x3(x, wk, out.t, dil, _ep(ops, BF16, bias, True))
    _assert_within(name + " fwd bf16", out.host(), C.relu(plain + o["bias"].astype(np.float64)), S, K, "bf16")
    out = _Out((n, H, W, Cout), F32)
    ops.conv3x3(x, wk, out.t, dil, _ep(ops, F32))
    _assert_within(name + " plain f32", out.host(), plain, S, K, "f32")
    Sd = C.conv3x3(np.abs(o["x"]), np.abs(C.dgrad_weights(o["wd"])), None, dil)
    out = _Out((n, H, W, Cout), BF16)
    ops.conv3x3(x, wkd, out.t, dil, _ep(ops, BF16, mask=_dev(o["mask"], BF16)))
    _assert_within(name + " dgrad bf16", out.host(), C.conv_dgrad(o["x"], o["wd"], dil, o["mask"]), Sd, K, "bf16")


# ------------------------------------------------------------------------------------------------ fused conv + ReLU + pool
def test_fused_pool_equals_the_pooled_float64_reference(ops):
    n, H, W, Cin, Cout = C.POOL_COVERED
    o = C.direct_int_operands(C.POOL_COVERED + (1,))
    OH, OW = C.pool_out_hw(H, W)
    out = _Out((n, OH, OW, Cout), BF16)
    assert ops.conv3x3_relu_pool2(_dev(o["x"], BF16), _wk(ops, o["w"], 0, BF16), _dev(o["bias"], F32), out.t) is True
    ref = C.maxpool2x2s2(C.relu(C.conv3x3(o["x"], o["w"], o["bias"], 1)))
    assert ref.shape == (n, OH, OW, Cout) and np.abs(ref).max() <= 256
    _assert_equal(out.host(), ref, "pooled")


@pytest.mark.parametrize("case", C.POOL_REFUSED, ids=C.case_id)
def test_fused_pool_refuses_and_leaves_the_output_alone(ops, case):
    n, H, W, Cin, Cout = case
    OH, OW = C.pool_out_hw(H, W)
    out = _Out((n, OH, OW, Cout), BF16)
    x = _dev(C.int_map(case, (n, H, W, Cin)), BF16)
    wk = torch.zeros(Cout, 9, Cin, device="cuda", dtype=BF16)
    assert ops.conv3x3_relu_pool2(x, wk, torch.zeros(Cout, device="cuda"), out.t) is False
    out.assert_intact()


# ------------------------------------------------------------------------------------------------ sw_conv3x3_multi
@pytest.mark.parametrize("name", list(C.MULTI_LISTS))
def test_multi_launch_against_float64_and_the_single_launches(ops, name, monkeypatch):
    table = C.MULTI_LISTS[name]
    operands = C.multi_operands(name)
    probs, outs, weights = [], [], {}
    for (n, H, W, Cin, Cout, epi), o in zip(table, operands):
        wkey = o["w"].tobytes() if name == "shared_weight" else len(probs)
        if wkey not in weights:
            weights[wkey] = (_wk(ops, o["w"], 0, BF16), _dev(o["bias"], F32))
        wk, bias = weights[wkey]
        ep = _ep(ops, BF16, bias, True) if epi == "relu" else _ep(ops, BF16, mask=_dev(o["mask"], BF16) if epi == "mask" else None)
        outs.append(_Out((n, H, W, Cout), BF16))
        probs.append((_dev(o["x"], BF16), wk, outs[-1].t, ep))
    assert len(weights) == (1 if name == "shared_weight" else len(table))
    single, calls = ops.conv3x3, []
    monkeypatch.setattr(ops, "conv3x3", lambda *a, **k: (calls.append(1), single(*a, **k))[1])
    ops.conv3x3_multi(probs)
    monkeypatch.setattr(ops, "conv3x3", single)
    # a covered list is one launch of the multi kernel; the others run every problem alone
    assert len(calls) == (0 if C.multi_covered([c[:5] for c in table]) else len(table))
    for i, ((n, H, W, Cin, Cout, epi), o) in enumerate(zip(table, operands)):
        got = outs[i].host()
        _assert_equal(got, C.multi_ref(o), f"problem {i}")
        if C.conv_direct_form(n, H, W, Cin, Cout) == "fourwave64":              # alone it takes the same form: the same bits
            alone = _Out((n, H, W, Cout), BF16)
            ops.conv3x3(probs[i][0], probs[i][1], alone.t, 1, probs[i][3])
            assert torch.equal(alone.host(), got)


# ------------------------------------------------------------------------------------------------ first layer
@pytest.mark.parametrize("epi", ("bias_relu", "plain"))
@pytest.mark.parametrize("case", C.FIRST_CASES, ids=C.case_id)
def test_first_layer_kernel_bit_exact(ops, case, epi):
    n, H, W = case
    o = C.first_operands(case)
    wk = _wk(ops, o["w"], 0, BF16)
    out = _Out((n, H, W, 64), BF16)
    if epi == "plain":
        ops.conv3x3(_dev(o["x"], BF16), wk, out.t, 1, _ep(ops, BF16))
        ref = C.conv3x3(o["x"], o["w"], None, 1)
    else:
        ops.conv3x3(_dev(o["x"], BF16), wk, out.t, 1, _ep(ops, BF16, _dev(o["bias"], F32), True))
        ref = C.relu(C.conv3x3(o["x"], o["w"], o["bias"], 1))
    _assert_equal(out.host(), ref)


# ------------------------------------------------------------------------------------------------ implicit-GEMM fallback
@pytest.mark.parametrize("hw", C.IGEMM_MAPS, ids=C.case_id)
@pytest.mark.parametrize("ch", C.IGEMM_BF16_CH, ids=C.case_id)
def test_igemm_fallback_bf16_bit_exact(ops, ch, hw):
    """what the direct kernel refuses: Cin 8 .. 72, Cout % 8 != 0, a pitched mask, ref_scale != 1; both dilations"""
    (Cin, Cout), (n, H, W) = ch, hw
    assert C.igemm_refusal("bf16", Cin) is None
    o = C.igemm_operands(n, H, W, Cin, Cout)
    x, wk = _dev(o["x"], BF16), _wk(ops, o["w"], 0, BF16)
    pitched = torch.full((n * H * W, Cout + C.REF_PITCH_ADD), float("nan"), device="cuda", dtype=BF16)
    pitched[:, :Cout] = _dev(o["mask"], BF16)
    eps = {"relu": _ep(ops, BF16, _dev(o["bias"], F32), True), "pitched_mask": _ep(ops, BF16, mask=pitched[:, :Cout]),
           "ref_scale": _ep(ops, BF16, mask=_dev(o["mask"], BF16), ref_scale=0.5), "dil2": _ep(ops, BF16)}
    assert eps["pitched_mask"].ld_ref == Cout + C.REF_PITCH_ADD
    for v in C.IGEMM_VARIANTS:
        dil = 2 if v == "dil2" else 1
        out = _Out((n, H, W, Cout), BF16)
        ops.conv3x3(x, wk, out.t, dil, eps[v])
        _assert_equal(out.host(), C.igemm_ref(o, v, dil), v)


def test_igemm_fallback_takes_a_direct_shape_with_a_pitched_mask_or_a_mask_scale(ops):
    """a shape the direct kernel covers, refused there for its epilogue: a mask with a row pitch above Cout, ref_scale = 0.5"""
    n, H, W, Cin, Cout = C.IGEMM_DIRECT_SHAPE
    assert C.conv_direct_form(n, H, W, Cin, Cout) == "kgroup"
    o = C.igemm_operands(n, H, W, Cin, Cout)
    x, wk = _dev(o["x"], BF16), _wk(ops, o["w"], 0, BF16)
    pitched = torch.full((n * H * W, Cout + C.REF_PITCH_ADD), float("nan"), device="cuda", dtype=BF16)
    pitched[:, :Cout] = _dev(o["mask"], BF16)
    for v, ep in (("pitched_mask", _ep(ops, BF16, mask=pitched[:, :Cout])), ("ref_scale", _ep(ops, BF16, mask=_dev(o["mask"], BF16), ref_scale=0.5))):
        out = _Out((n, H, W, Cout), BF16)
        ops.conv3x3(x, wk, out.t, 1, ep)
        _assert_equal(out.host(), C.igemm_ref(o, v, 1), v)


def test_igemm_refuses_a_ragged_input_row_and_leaves_the_output_alone(ops):
    n, H, W, Cin, Cout = C.IGEMM_REFUSED_BF16
    out = _Out((n, H, W, Cout), BF16)
    x = _dev(C.int_map((1,), (n, H, W, Cin)), BF16)
    with pytest.raises(Exception, match=f"code -{C.igemm_refusal('bf16', Cin)}"):
        ops.conv3x3(x, torch.zeros(Cout, 9, Cin, device="cuda", dtype=BF16), out.t, 1, _ep(ops, BF16))
    out.assert_intact()


@pytest.mark.parametrize("Cin", C.IGEMM_F32_CIN)
def test_igemm_fallback_f32_bit_exact(ops, Cin):
    n, H, W = C.IGEMM_F32_MAP
    assert C.igemm_refusal("f32", Cin) is None
    for Cout in C.IGEMM_F32_COUT:
        o = C.igemm_operands(n, H, W, Cin, Cout)
        x, wk = _dev(o["x"], F32), _wk(ops, o["w"], 0, F32)
        out = _Out((n, H, W, Cout), F32)
        ops.conv3x3(x, wk, out.t, 1, _ep(ops, F32, _dev(o["bias"], F32), True))
        _assert_equal(out.host(), C.igemm_ref(o, "relu", 1), f"Cout {Cout} dil 1")
        out = _Out((n, H, W, Cout), F32)
        ops.conv3x3(x, wk, out.t, 2, _ep(ops, F32, mask=_dev(o["mask"], F32)))
        _assert_equal(out.host(), C.igemm_ref(o, "pitched_mask", 2), f"Cout {Cout} dil 2")


def test_first_layer_and_fallback_within_the_per_element_bar(ops):
    for name, dtype, (n, H, W, Cin, Cout), dil in (("first", "bf16", (2, 19, 130, 8, 64), 1), ("igemm bf16", "bf16", (2, 19, 23, 72, 64), 1),
                                                   ("igemm bf16", "bf16", (2, 19, 23, 48, 40), 2), ("igemm f32", "f32", (2, 7, 19, 36, 20), 1)):
        key = (n, H, W, Cin, Cout, dil)
        td = C.torch_dtype(dtype)
        x, w = C.gauss(key, (n, H, W, Cin), 0.7, dtype), C.gauss(key + (0,), (Cout, Cin, 3, 3), 0.05, dtype)
        bias = C.gauss(key, (Cout,), 0.1, "f32")
        out = _Out((n, H, W, Cout), td)
        ops.conv3x3(_dev(x, td), _wk(ops, w, 0, td), out.t, dil, _ep(ops, td, _dev(bias, F32), True))
        S = C.conv3x3(np.abs(x), np.abs(w), np.abs(bias), dil)
        _assert_within(f"{name} {C.case_id(key)}", out.host(), C.relu(C.conv3x3(x, w, bias, dil)), S, 9 * Cin, dtype)


# ------------------------------------------------------------------------------------------------ weight gradients
def _scale_old(case, sk, acc):
    Cin, Cout = case[3], case[4]
    scale = C.scale_of(sk, case[:6], Cout)
    old = C.old_gradient(case[:6], (Cout, Cin, 3, 3)) if acc else None
    return scale, old, (None if scale is None else _dev(scale, F32))


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
@pytest.mark.parametrize("case", C.WGRAD_CASES, ids=C.case_id)
def test_wgrad_bit_exact(ops, case, dtype):
    n, H, W, Cin, Cout, dil, ns, sk, acc = case
    td = C.torch_dtype(dtype)
    x, dy = C.wgrad_operands(case)
    scale, old, scale_d = _scale_old(case, sk, acc)
    exact = C.wgrad(x, dy, dil)
    nsl = C.nslab(dtype, n, H, W, ns)
    xd, dyd = _dev(x, td), _dev(dy, td)
    assert ops.conv3x3_wgrad_nslab(xd, Cout, ns) == nsl
    dw, ws = _Out((Cout, Cin, 3, 3), F32, init=old), _Out((nsl, Cout, 9, Cin), F32)
    ops.conv3x3_wgrad(xd, dyd, dw.t, dil, splitk=ns, workspace=ws.t.view(-1), cout_scale=scale_d, accumulate=acc)
    _assert_equal(dw.host(), C.scaled_f32(exact, scale, old), "dW")
    assert np.array_equal(C.fold(ws.host().numpy()), exact)                    # every slab written, nothing behind the last one


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
def test_wgrad_refuses_a_map_below_the_gather_guard(ops, dtype):
    n, H, W, Cin, Cout, dil = C.WGRAD_REFUSED
    td = C.torch_dtype(dtype)
    x, dy = C.wgrad_operands(C.WGRAD_REFUSED)
    dw, ws = _Out((Cout, Cin, 3, 3), F32), _Out((1, Cout, 9, Cin), F32)
    with pytest.raises(Exception, match="code -6"):
        ops.conv3x3_wgrad(_dev(x, td), _dev(dy, td), dw.t, dil, splitk=1, workspace=ws.t.view(-1))
    dw.assert_intact(); ws.assert_intact()
    slabs = _Out((1, Cout, 9, Cin), F32)
    with pytest.raises(Exception, match="code -6"):
        ops.conv3x3_wgrad_grouped([(_dev(x, td), _dev(dy, td), slabs.t, dil, 1)])
    slabs.assert_intact()


def _grouped(ops, dtype, cases, gaussian=False):
    td = C.torch_dtype(dtype)
    probs, keep = [], []
    for c in cases:
        n, H, W, Cin, Cout, dil, ns = c
        x, dy = C.wgrad_operands(c, gaussian, dtype)
        nsl = C.nslab(dtype, n, H, W, ns)
        xd, dyd = _dev(x, td), _dev(dy, td)
        assert ops.conv3x3_wgrad_nslab(xd, Cout, ns) == nsl
        slabs = _Out((nsl, Cout, 9, Cin), F32)
        probs.append((xd, dyd, slabs.t, dil, ns)); keep.append((x, dy, slabs, nsl))
    ops.conv3x3_wgrad_grouped(probs)
    return keep


def _check_grouped(ops, cases, keep):
    for c, (x, dy, slabs, nsl) in zip(cases, keep):
        n, H, W, Cin, Cout, dil, ns = c
        exact = C.wgrad(x, dy, dil)
        assert np.array_equal(C.fold(slabs.host().numpy()), exact), c         # the slabs themselves: all written, their sum exact
        dw = _Out((Cout, Cin, 3, 3), F32)
        ops.conv3x3_wgrad_fold(slabs.t, nsl, dw.t)
        _assert_equal(dw.host(), exact, str(c))


@pytest.mark.parametrize("cases", [[c] for c in C.GROUPED_DIRECT] + [C.GROUPED_DIRECT], ids=lambda cs: "+".join(C.case_id(c) for c in cs))
def test_grouped_direct_weight_gradient_kernel_bit_exact(ops, cases):
    assert C.wgrad_direct_taken("bf16", cases)
    _check_grouped(ops, cases, _grouped(ops, "bf16", cases))


@pytest.mark.parametrize("dtype,case", C.GROUPED_IGEMM, ids=lambda v: v if isinstance(v, str) else C.case_id(v))
def test_grouped_implicit_gemm_weight_gradient_bit_exact(ops, dtype, case):
    assert not C.wgrad_direct_taken(dtype, [case])
    _check_grouped(ops, [case], _grouped(ops, dtype, [case]))


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
@pytest.mark.parametrize("n", C.SMALL_N)
@pytest.mark.parametrize("hw", C.SMALL_MAPS, ids=C.case_id)
def test_wgrad_small_bit_exact(ops, hw, n, dtype):
    (H, W), Cin, Cout = hw, C.SMALL_CIN, C.SMALL_COUT
    td = C.torch_dtype(dtype)
    case = (n, H, W, Cin, Cout, 1)
    x, dy = C.wgrad_operands(case)
    exact = C.wgrad(x, dy, 1)
    for sk, acc in ((None, False), ("pow2", False), (None, True), ("general", True)):
        scale, old, scale_d = _scale_old(case, sk, acc)
        dw = _Out((Cout, Cin, 3, 3), F32, init=old)
        ops.conv3x3_wgrad_small(_dev(x, td), _dev(dy, td), dw.t, cout_scale=scale_d, accumulate=acc)
        _assert_equal(dw.host(), C.scaled_f32(exact, scale, old), f"scale {sk} accumulate {acc}")


def test_wgrad_small_second_grid_stride_turn(ops):
    n, H, W, Cin, Cout = C.SMALL_LARGE
    case = (n, H, W, Cin, Cout, 1)
    x, dy = C.wgrad_operands(case)
    scale, old, scale_d = _scale_old(case, "pow2", True)
    dw = _Out((Cout, Cin, 3, 3), F32, init=old)
    ops.conv3x3_wgrad_small(_dev(x, BF16), _dev(dy, BF16), dw.t, cout_scale=scale_d, accumulate=True)
    _assert_equal(dw.host(), C.scaled_f32(C.wgrad(x, dy, 1), scale, old))


@pytest.mark.parametrize("case", C.FOLD_CASES, ids=C.case_id)
def test_fold_bit_exact(ops, case):
    ns, Cin, Cout, sk, acc = case
    slabs = C.fold_slabs(case[:3], ns, Cin, Cout)
    key = (ns, Cin, Cout, 0, 0, 0)
    scale, old, scale_d = _scale_old((0, 0, 0, Cin, Cout, ns), sk, acc)
    dw = _Out((Cout, Cin, 3, 3), F32, init=old)
    ops.conv3x3_wgrad_fold(_dev(slabs, F32), ns, dw.t, cout_scale=scale_d, accumulate=acc)
    _assert_equal(dw.host(), C.scaled_f32(C.fold(slabs), scale, old), str(key))


def test_fold_refuses_more_input_channels_than_its_lds_holds(ops):
    Cin = C.FOLD_REFUSED_CIN
    dw = _Out((1, Cin, 3, 3), F32)
    with pytest.raises(Exception, match="code -5"):
        ops.conv3x3_wgrad_fold(torch.zeros(1, 9 * Cin, device="cuda"), 1, dw.t)
    dw.assert_intact()
    with pytest.raises(Exception, match="code -5"):
        ops.conv3x3_wgrad_fold_multi([(torch.zeros(1, 9 * Cin, device="cuda"), 1, dw.t)])
    dw.assert_intact()


def test_fold_multi_more_folds_than_one_launch_holds(ops):
    folds, want = [], []
    for i, (Cin, Cout, ns) in enumerate(C.FOLD_MULTI):
        slabs = C.fold_slabs((i,), ns, Cin, Cout)
        dw = _Out((Cout, Cin, 3, 3), F32)
        folds.append((_dev(slabs, F32), ns, dw.t)); want.append((dw, C.fold(slabs)))
    ops.conv3x3_wgrad_fold_multi(folds)
    for i, (dw, ref) in enumerate(want):
        _assert_equal(dw.host(), ref, f"fold {i} {C.FOLD_MULTI[i]}")


def test_weight_gradients_within_the_per_element_bar(ops):
    for dtype in ("bf16", "f32"):
        n, H, W, Cin, Cout, dil, ns = c = C.WGRAD_GAUSS
        td = C.torch_dtype(dtype)
        x, dy = C.wgrad_operands(c, True, dtype)
        scale = C.general_scale(c, Cout)
        ref = C.fold(C.wgrad(x, dy, dil).reshape(Cout, Cin, 9).transpose(0, 2, 1)[None], scale)
        S = C.wgrad(np.abs(x), np.abs(dy), dil) * np.abs(scale).astype(np.float64).reshape(Cout, 1, 1, 1)
        dw = _Out((Cout, Cin, 3, 3), F32)
        ops.conv3x3_wgrad(_dev(x, td), _dev(dy, td), dw.t, dil, splitk=ns, cout_scale=_dev(scale, F32))
        _assert_within(f"wgrad {dtype} {C.case_id(c)}", dw.host(), ref, S, n * H * W, "f32")
    n, H, W, Cin, Cout, dil, ns = c = C.GROUPED_GAUSS
    (x, dy, slabs, nsl), = _grouped(ops, "bf16", [c], True)
    dw = _Out((Cout, Cin, 3, 3), F32)
    ops.conv3x3_wgrad_fold(slabs.t, nsl, dw.t)
    slabs.host()
    _assert_within(f"wgrad direct {C.case_id(c)}", dw.host(), C.wgrad(x, dy, dil), C.wgrad(np.abs(x), np.abs(dy), dil), n * H * W, "f32")
    for dtype in ("bf16", "f32"):
        c = (2, 7, 3, C.SMALL_CIN, C.SMALL_COUT, 1)
        x, dy = C.wgrad_operands(c, True, dtype)
        dw = _Out((C.SMALL_COUT, C.SMALL_CIN, 3, 3), F32)
        ops.conv3x3_wgrad_small(_dev(x, C.torch_dtype(dtype)), _dev(dy, C.torch_dtype(dtype)), dw.t)
        _assert_within(f"wgrad small {dtype} {C.case_id(c)}", dw.host(), C.wgrad(x, dy, 1), C.wgrad(np.abs(x), np.abs(dy), 1), 2 * 7 * 3, "f32")
    ns, Cin, Cout = 17, 64, 8
    slabs = C.gauss((ns, Cin, Cout), (ns, Cout, 9, Cin), 1.0, "f32")
    scale = C.general_scale((ns,), Cout)
    dw = _Out((Cout, Cin, 3, 3), F32)
    ops.conv3x3_wgrad_fold(_dev(slabs, F32), ns, dw.t, cout_scale=_dev(scale, F32))
    S = C.fold(np.abs(slabs), np.abs(scale))
    _assert_within(f"fold {ns} slabs", dw.host(), C.fold(slabs, scale), S, ns, "f32")


# ------------------------------------------------------------------------------------------------ sw_conv_weight_prep
@pytest.mark.parametrize("dtype", ("bf16", "f32"))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("case", C.PREP_CASES, ids=C.case_id)
def test_weight_prep_is_the_permuted_tensor_with_zero_padding(ops, case, mode, dtype):
    Cout, Cin, pad = case
    td = C.torch_dtype(dtype)
    w = C.gauss(case, (Cout, Cin, 3, 3), 1.0, dtype)
    out = _Out((Cout, 9, pad) if mode == 0 else (Cin, 9, Cout), td)
    ops.conv_weight_prep(_dev(w, F32), out.t, mode, pad if mode == 0 else None)
    want = C.weight_prep_ref(w, mode, pad)
    got = out.host()
    _assert_equal(got, want)
    if mode == 0 and pad > Cin:
        assert not got[:, :, Cin:].float().any()

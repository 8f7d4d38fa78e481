"""GPU: the pooling, layout, optimizer and scalar kernels of csrc/elementwise.hip against the restatements of tests/elementwise_ref.py
at their edges: f32 and bf16, the scalar twins of the vector kernels (C % V != 0, a view one element into a buffer), signed inputs
with ties, +-0, +-inf and NaN through the 2x2 pool and its three backward kernels, the cast value set (ties to even both ways,
overflow, subnormals) through every conversion, row pitches on both sides, the unaligned-row branches of the staged stores, every
form of the fused SGD (element, 32x32x9 conv tiles with several input-channel tiles and a padded pitch, 64x64 tiles) on a first and a
later step with host and device hyper-parameters, more than one launch of the multi-tensor kernels, the grid-stride second pass, and
a NaN through every forward ReLU / max site of conv_direct.hip and gemm.hip.  Every output starts as a NaN with a payload no kernel
writes and has slack behind its end: what the contract says is written must equal the reference (bit for bit, or within the bound
of elementwise_ref.sgd_bounds), everything else must still hold the sentinel.  tests/test_elementwise_ref_cpu.py pins the
restatements to torch and asserts that the case tables reach the edges they are named for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import elementwise_ref as E  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope="module")
def kernel_error():
    from sos_wsod_amd._lib import HipKernelError
    return HipKernelError


_F32_SENTINEL, _BF16_SENTINEL = 0x7FA5A5A5, 0x7FA5


def _tdt(d):
    return E.torch_dtype(d) if isinstance(d, str) else d


def _sent(n, dtype=torch.float32):
    if dtype == torch.float32:
        return torch.full((n,), _F32_SENTINEL, device="cuda", dtype=torch.int32).view(torch.float32)
    return torch.full((n,), _BF16_SENTINEL, device="cuda", dtype=torch.int16).view(torch.bfloat16)


def _untouched(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32) == _F32_SENTINEL
    return t.view(torch.int16) == _BF16_SENTINEL


class _Out:
    """a (rows, cols) output of row pitch ld (or any shape, contiguous, with ld=None) inside a sentinel-filled buffer: `mis` elements
    in front (1 = off every vector alignment), SLACK behind"""

    def __init__(self, shape, dtype, mis=0, ld=None):
        dtype = _tdt(dtype)
        self.mis = mis
        if ld is None:
            self.n = int(np.prod(shape))
            self.buf = _sent(mis + self.n + E.SLACK, dtype)
            self.block = self.buf[mis:mis + self.n]
            self.t = self.block.view(*shape)
            self.pad = None
        else:
            rows, cols = shape
            self.n = rows * ld
            self.buf = _sent(mis + self.n + E.SLACK, dtype)
            self.block = self.buf[mis:mis + self.n].view(rows, ld)
            self.t = self.block[:, :cols]
            self.pad = self.block[:, cols:]

    def assert_untouched(self):
        torch.cuda.synchronize()
        assert bool(_untouched(self.buf).all()), "an output that must not be written was written"

    def host(self):
        """float32 numpy of the output, after checking that nothing around it was written and all of it was"""
        torch.cuda.synchronize()
        assert bool(_untouched(self.buf[:self.mis]).all() and _untouched(self.buf[self.mis + self.n:]).all()), "written outside the output"
        if self.pad is not None:
            assert bool(_untouched(self.pad).all()), "written into the row padding"
        assert not bool(_untouched(self.t).any()), "an element of the output was not written"
        return self.t.float().cpu().numpy()


def _dev(x, dtype="f32", mis=0):
    """float32 numpy (values of `dtype`) -> device tensor of `dtype`; mis: a view that many elements into a larger buffer"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(_tdt(dtype))
    if not mis:
        return t.cuda()
    buf = torch.full((t.numel() + mis,), float("nan"), dtype=t.dtype, device="cuda")
    buf[mis:] = t.reshape(-1).cuda()
    return buf[mis:].view(*t.shape)


def _pitched(m, cols, mis=0):
    """float32 numpy (rows, ld) -> device float32 view (rows, cols) of row pitch ld, `mis` elements into a buffer"""
    return _dev(m, "f32", mis)[:, :cols]


def _cast_want(x_host, x_dev, dtype):
    """the expected cast of float32 values: the host's round-to-nearest-even; for float32 subnormals the device's own
    tensor.to(bfloat16) (the denormal mode is a property of the build)"""
    want = E.round_to(x_host, dtype)
    sub = E.is_subnormal(x_host)
    if dtype == "bf16" and sub.any():
        dev = x_dev.to(torch.bfloat16).float().cpu().numpy()
        want = np.where(sub, dev, want)
    return want


# ------------------------------------------------------------------------------------------------ 2x2 max pool
_POOL_IDS = [f"{c[0]}x{c[1]}-s{c[2]}-C{c[3]}{'-mis' if c[4] else ''}" for c in E.POOL_CASES]


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("c", E.POOL_CASES, ids=_POOL_IDS)
def test_maxpool2x2_fwd_is_max_pool2d_bit_for_bit(ops, c, dtype):
    H, W, stride, C, mis = c
    for regime in E.POOL_REGIMES:
        x = E.pool_inputs(H, W, C, dtype, regime)
        want, _ = E.maxpool_fwd_ref(x, stride)
        for mi, mo in (((1, 0), (0, 1)) if mis else ((0, 0),)):
            out = _Out(want.shape, dtype, mo)
            ops.maxpool_fwd(_dev(x, dtype, mi), out.t, stride)
            assert E.same_bits(out.host(), want), (c, dtype, regime, mi, mo)


@pytest.mark.parametrize("relu_mask", [0, 1])
@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("c", E.POOL_CASES, ids=_POOL_IDS)
def test_maxpool2x2_bwd_routes_to_torchs_index_bit_for_bit(ops, c, dtype, relu_mask):
    """the gradient goes to the element torch's indices name (the last NaN in scan order, else the first maximum); the stride-1 sum
    is the float32 sum in window order, rounded once; the odd last row / column gets zeros; NaN inputs only without the mask"""
    H, W, stride, C, mis = c
    OH, OW = E.pool_out_hw(H, W, stride)
    for regime in (E.POOL_REGIMES[:2] if relu_mask else E.POOL_REGIMES):
        x = E.pool_inputs(H, W, C, dtype, regime)
        dout = E.pool_dout(H, W, C, stride, dtype)
        want = E.maxpool_bwd_ref(x, dout, stride, relu_mask, dtype)
        for mx, md, mo in (((1, 0, 0), (0, 1, 0), (0, 0, 1)) if mis else ((0, 0, 0),)):
            out = _Out(want.shape, dtype, mo)
            ops.maxpool_bwd(_dev(x, dtype, mx), _dev(dout, dtype, md), out.t, stride, relu_mask)
            got = out.host()
            assert E.same_bits(got, want), (c, dtype, regime, relu_mask, mx, md, mo)
            if stride == 2:
                assert not got[:, 2 * OH:].any() and not got[:, :, 2 * OW:].any()


# ------------------------------------------------------------------------------------------------ relu_bwd
@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("n", E.RELU_N)
def test_relu_bwd_rule_and_bits(ops, n, dtype):
    """out = ref > 0 ? g : 0 (a NaN ref gives 0); g passes with its bits; aligned and misaligned, in place and with a separate out"""
    ref, g = E.relu_inputs(n, dtype)
    for mis in (0, 1):
        r_d, g_d = _dev(ref, dtype, mis), _dev(g, dtype, mis)
        want = E.relu_bwd_ref(ref, g_d.float().cpu().numpy())      # the bits g has on the device (a host cast picks its own NaN payload)
        keep = g_d.clone()
        out = _Out((n,), dtype, mis)
        assert ops.relu_bwd(r_d, g_d, out=out.t) is out.t
        got = out.host()
        assert np.array_equal(E.bits(got), want), (n, dtype, mis)
        assert torch.equal(g_d.view(torch.int16 if dtype == "bf16" else torch.int32), keep.view(torch.int16 if dtype == "bf16" else torch.int32))
        assert ops.relu_bwd(r_d, g_d) is g_d
        torch.cuda.synchronize()
        assert np.array_equal(E.bits(g_d.float().cpu().numpy()), want), (n, dtype, mis, "in place")


# ------------------------------------------------------------------------------------------------ conversions
@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("shape", E.CONVERT_SHAPES, ids=[f"{r}x{c}" for r, c in E.CONVERT_SHAPES])
def test_convert_2d_casts_bit_for_bit_on_both_forms(ops, shape, dtype):
    seen = set()
    for (rows, cols, ld_src, ld_dst, ms, md) in E.CONVERT_CASES:
        if (rows, cols) != shape:
            continue
        m = E.cast_matrix(1, rows, cols, ld_src)
        src = _pitched(m, cols, ms)
        out = _Out((rows, cols), dtype, md, ld=ld_dst)
        ops.convert_2d(src, out.t, rows, cols)
        want = _cast_want(m[:, :cols], src, dtype)
        assert E.same_bits(out.host(), want), (rows, cols, ld_src, ld_dst, ms, md, dtype)
        seen.add(E.convert_2d_form(cols, ld_src, ld_dst, ms, md))
        assert (src.data_ptr() % 16 == 0) == (ms == 0) and (out.t.data_ptr() % (4 * E.ESIZE[dtype]) == 0) == (md == 0)
    assert seen == ({"vec4", "scalar"} if shape[1] % 4 == 0 else {"scalar"})


@pytest.mark.parametrize("dtype", E.DTYPES)
def test_convert_flat_casts_bit_for_bit(ops, dtype):
    for shape in E.CONVERT_FLAT_SHAPES:
        cols = shape[-1]
        m = E.cast_matrix(2, int(np.prod(shape)) // cols, cols, cols).reshape(shape)
        src = _dev(m)
        got = ops.convert_flat(src, _tdt(dtype))
        torch.cuda.synchronize()
        assert got.shape == src.shape and got.dtype == _tdt(dtype)
        assert E.same_bits(got.float().cpu().numpy(), _cast_want(m, src, dtype)), (shape, dtype)
    if dtype == "bf16":                                            # the build's denormal mode, for the record
        sub = E.cast_values()[E.N_CAST_NORMAL:]
        dev = _dev(sub).to(torch.bfloat16).float().cpu().numpy()
        print("float32 subnormals", sub, "-> bf16 on the device", dev, "; host round-to-nearest-even", E.round_to(sub, "bf16"))


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("c", E.CONVERT_T_CASES, ids=[f"{c[0]}x{c[1]}+{c[2]}" for c in E.CONVERT_T_CASES])
def test_convert_2d_t_transposes_and_casts_bit_for_bit(ops, c, dtype, kernel_error):
    rows, cols, add = c
    m = E.cast_matrix(3, rows, cols, cols + 4)
    src = _pitched(m, cols)
    out = _Out((cols, rows), dtype, 0, ld=rows + add)
    ops.convert_2d_t(src, out.t, rows, cols)
    want = _cast_want(m[:, :cols], src, dtype).T
    assert E.same_bits(out.host(), want)
    bad = _Out((65, 64), dtype, 0, ld=64 + 8)
    with pytest.raises(kernel_error, match="-5"):
        ops.convert_2d_t(_pitched(E.cast_matrix(3, 64, 65, 68), 65), bad.t, 64, 65)
    bad.assert_untouched()


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("shape", E.WEIGHT_PREP_SHAPES, ids=[f"{a}x{b}" for a, b in E.WEIGHT_PREP_SHAPES])
def test_conv_weight_prep_layouts_bit_for_bit(ops, shape, dtype, kernel_error):
    Cout, Cin = shape
    w = E.weight_matrix(1, (Cout, Cin, 3, 3))
    wd = _dev(w)
    for pad in E.WEIGHT_PREP_PADS[shape]:
        out = _Out((Cout, 9, pad), dtype)
        ops.conv_weight_prep(wd, out.t, 0, pad)
        got = out.host()                                           # (the tail behind the block stays sentinel)
        want = E.weight_prep_ref(w, 0, pad)
        want[:, :, :Cin] = _cast_want(want[:, :, :Cin], torch.from_numpy(want[:, :, :Cin].copy()).cuda(), dtype)
        assert E.same_bits(got, want) and not got[:, :, Cin:].any(), (shape, pad, dtype)
    out = _Out((Cin, 9, Cout), dtype)
    ops.conv_weight_prep(wd, out.t, 1)
    want = E.weight_prep_ref(w, 1)
    assert E.same_bits(out.host(), _cast_want(want, torch.from_numpy(want).cuda(), dtype))
    bad = _Out((Cin + 1, 9, Cout), dtype)
    with pytest.raises(kernel_error, match="-3"):
        ops.conv_weight_prep(wd, bad.t, 1, Cin + 1)
    bad.assert_untouched()


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("cpad", E.NCHW_CPADS)
def test_nchw_to_nhwc_bit_for_bit(ops, cpad, dtype):
    x = E.weight_matrix(2, E.NCHW_SHAPE)
    N, C, H, W = E.NCHW_SHAPE
    out = _Out((N, H, W, cpad), dtype)
    xd = _dev(x)
    ops.nchw_to_nhwc(xd, out.t)
    want = E.nchw_to_nhwc_ref(x, cpad)
    want[..., :C] = _cast_want(want[..., :C], xd.permute(0, 2, 3, 1), dtype)
    got = out.host()
    assert E.same_bits(got, want) and not got[..., C:].any()


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("c", E.SCALE_COLS_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}" for c in E.SCALE_COLS_CASES])
def test_scale_cols_one_product_one_rounding(ops, c, dtype):
    M, N, ld_in, ld_out = c
    src, cs = E.scale_cols_inputs(M, N, ld_in)
    out = _Out((M, N), dtype, 0, ld=ld_out)
    src_d, cs_d = _pitched(src, N), _dev(cs)
    ops.scale_cols(src_d, cs_d, out.t, M, N)
    prod = E.scale_cols_ref(src, cs, N)
    want = E.round_to(prod, dtype)
    sub = E.is_subnormal(src[:, :N]) | E.is_subnormal(prod)        # there: the device's own product and cast (the build's denormal mode)
    assert E.is_subnormal(src[:, :N]).any() and E.is_subnormal(prod).any()
    dev = (src_d * cs_d).to(_tdt(dtype)).float().cpu().numpy()
    print("scale_cols", c, dtype, "subnormal elements: device", dev[sub], "host", want[sub])
    assert E.same_bits(out.host(), np.where(sub, dev, want))


@pytest.mark.parametrize("c", E.SPLIT_CASES, ids=[f"{c[0]}x{c[1]}-side{c[2]}-{'rows' if c[3] else 'cols'}" for c in E.SPLIT_CASES])
def test_split_bf16x3_pieces_and_block_patterns(ops, c, kernel_error):
    rows, cols, side, along_rows = c
    m = E.cast_matrix(4, rows, cols, cols + 4)
    a = m[:, :cols]
    src_d = _pitched(m, cols)
    # the pieces of the float32 subnormals: the device's own torch expression (the build's denormal mode), as for every cast
    sub = E.is_subnormal(a)
    assert sub.sum() == 3
    b1 = src_d.to(torch.bfloat16).float(); r1 = src_d - b1
    b2 = r1.to(torch.bfloat16).float(); r2 = r1 - b2
    dev_pieces = [t.cpu().numpy() for t in (b1, b2, r2.to(torch.bfloat16).float())]
    pieces = [np.where(sub, d, h) for d, h in zip(dev_pieces, E.split_pieces_ref(a))]
    print("split_bf16x3 pieces of the subnormals: device", [d[sub] for d in dev_pieces], "host", [h[sub] for h in E.split_pieces_ref(a)])
    shape = (6 * rows, cols) if along_rows else (rows, 6 * cols)
    out = _Out(shape, "bf16", 0, ld=shape[1] + 4)
    assert ops.split_bf16x3(src_d, side, along_rows=bool(along_rows), out=out.t) is out.t
    got = out.host()
    assert E.same_bits(got, np.concatenate([pieces[k] for k in E.SPLIT_PATTERNS[side]], axis=0 if along_rows else 1))
    blocks = got.reshape(6, rows, cols) if along_rows else got.reshape(rows, 6, cols).transpose(1, 0, 2)
    for p, k in enumerate(E.SPLIT_PATTERNS[side]):
        assert E.same_bits(blocks[p], pieces[k]), (c, p)
    by_piece = {k: blocks[p].astype(np.float64) for p, k in enumerate(E.SPLIT_PATTERNS[side])}
    fin = np.isfinite(a) & (np.abs(a) < 1e38) & ~sub               # the finite normal inputs
    assert np.array_equal((by_piece[0] + by_piece[1] + by_piece[2])[fin], a.astype(np.float64)[fin])
    bad = _Out((3, 36), "bf16", 0, ld=40)
    with pytest.raises(kernel_error, match="-5"):
        ops.split_bf16x3(_pitched(E.cast_matrix(4, 3, 6, 8), 6), side, out=bad.t)
    bad.assert_untouched()


# ------------------------------------------------------------------------------------------------ optimizer
_MOM, _GSCALE = 0.9, 0.5


def _sgd_check(what, got_p, got_b, w, g, buf, lr, wd, first, ratios, form):
    pr, br, S = E.sgd_ref(w, g, buf, lr, wd, _MOM, _GSCALE, first)
    ab, ap = E.sgd_bounds(w, S, lr)
    assert not np.isnan(got_p).any() and not np.isnan(got_b).any(), f"{what}: NaN after the step"
    eb = np.abs(got_b.astype(np.float64) - br); ep = np.abs(got_p.astype(np.float64) - pr)
    if eb.size:
        rb = float(np.max(np.where(eb == 0, 0.0, eb / np.maximum(ab, 1e-300)))); rp = float(np.max(np.where(ep == 0, 0.0, ep / np.maximum(ap, 1e-300))))
        ratios[form] = max(ratios.get(form, 0.0), rb, rp)
    assert (eb <= ab).all(), f"{what}: momentum buffer off by {float((eb - ab).max()):.3g} beyond 4u S"
    assert (ep <= ap).all(), f"{what}: parameter off by {float((ep - ap).max()):.3g} beyond u (6 lr S + 2|w|)"


@pytest.mark.parametrize("hyper", ["host", "device"])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("sdt", E.DTYPES)
def test_sgd_multi_against_float64_and_staged_copies(ops, sdt, first, hyper):
    """one list of 28 entries (two launches of the multi-tensor kernel, two of the 64x64 tile kernel): parameter and momentum buffer
    against float64 from the pre-step state within sgd_bounds, every staged copy bit for bit the cast of the updated parameter in
    its declared layout, row padding and slack untouched; a first step ignores a NaN-poisoned buffer; `hyper` on the device
    overrides the host fields"""
    es = E.sgd_entries()
    state, entries, stages = [], [], []
    for i, e in enumerate(es):
        w, g, buf = E.sgd_state(i, e, 0 if first else 1)
        if first:
            buf = np.full_like(buf, np.nan)
        pd, gd, bd = _dev(w, "f32", e["mis"]), _dev(g, "f32", e["mis"]), _dev(buf, "f32", e["mis"])
        (lr, wd), (lr2, wd2) = E.sgd_hyper(i)
        hy = torch.tensor([lr2, wd2], dtype=torch.float32, device="cuda") if hyper == "device" else None
        d = "f32" if e.get("f32") else sdt
        s0 = s1 = None
        if e["kind"] == 1:
            s0 = _Out((e["shape"][0], e["d0"]), d, 0, ld=e["ld0"])
        elif e["kind"] == 2:
            s0 = _Out((e["d0"] * 9, e["d1"]), d, 0, ld=e["d2"]) if e["s0"] else None
            s1 = _Out((e["d1"] * 9, e["d0"]), d, 0, ld=e["d0"]) if e["s1"] else None
        elif e["kind"] == 3:
            s0 = _Out((e["shape"][0], e["d0"]), d, 0, ld=e["ld0"])
            s1 = _Out((e["d0"], e["shape"][0]), d, 0, ld=e["ld1"])
        st = None
        if e["kind"]:
            st = dict(kind=e["kind"], dtype=_tdt(d), stage0=None if s0 is None else s0.t, stage1=None if s1 is None else s1.t,
                      d0=e["d0"], d1=e.get("d1", 0), d2=e.get("d2", 0), ld0=e.get("ld0", 0), ld1=e.get("ld1", 0))
        entries.append(dict(param=pd, grad=gd, buf=bd, lr=lr, weight_decay=wd, first=first, staging=st, hyper=hy))
        state.append((w, g, buf, (lr2, wd2) if hyper == "device" else (lr, wd), pd, gd, bd, d))
        stages.append((s0, s1))
    ops.sgd_multi(entries, _MOM, _GSCALE)
    torch.cuda.synchronize()
    ratios = {}
    for i, e in enumerate(es):
        w, g, buf, (lr, wd), pd, gd, bd, d = state[i]
        p_new, b_new = pd.cpu().numpy(), bd.cpu().numpy()
        assert E.same_bits(gd.cpu().numpy(), g), "the gradient is read only"
        _sgd_check(e["name"], p_new, b_new, w, g, buf, lr, wd, first, ratios, E.sgd_form(e))
        s0, s1 = stages[i]
        cast = E.round_to(p_new, d)
        if e["kind"] in (1, 3):
            assert E.same_bits(s0.host(), cast.reshape(-1, e["d0"])), (e["name"], "row-major copy")
        if e["kind"] == 3:
            assert E.same_bits(s1.host(), cast.T), (e["name"], "transposed copy")
        if e["kind"] == 2:
            r0, r1 = E.stage_kind2_ref(cast, e["d2"])
            if s0 is not None:
                assert E.same_bits(s0.host(), r0[:, :, :e["d1"]].reshape(e["d0"] * 9, e["d1"])), (e["name"], "forward layout")
            if s1 is not None:
                assert E.same_bits(s1.host(), r1.reshape(e["d1"] * 9, e["d0"])), (e["name"], "data-gradient layout")
    print("sgd_multi", sdt, "first" if first else "later", hyper, "max error / bound per form:", {k: round(v, 3) for k, v in sorted(ratios.items())})
    assert set(ratios) == {"tile64", "conv_tile", "vector", "scalar"}


def _sgd_seam_entries(all_live):
    """25 entries (SW_SGD_MAX_TENSORS + 1): the empty one and the kind-3 one (its own launch) sit inside the first launch's range, the
    conv tile form, an unaligned parameter and 4097 elements (a second chunk of one element) on both sides of the seam.  sw_sgd_multi
    cuts its launches by input index, so those two leave the first launch 22 tensors; all_live puts element tensors in their places:
    24 tensors, every slot of the table and block_start[24] in use"""
    k1 = dict(name="k1-72/76", shape=(11, 72), mis=0, kind=1, d0=72, ld0=76)
    k2t = dict(name="k2-32x32", shape=(32, 32, 3, 3), mis=0, kind=2, d0=32, d1=32, d2=32, s0=True, s1=True)
    k2 = dict(name="k2-40x24", shape=(40, 24, 3, 3), mis=0, kind=2, d0=40, d1=24, d2=24, s0=True, s1=True)
    k3 = dict(name="k3-64x128", shape=(64, 128), mis=0, kind=3, d0=128, ld0=128 + 8, ld1=64 + 8)
    el = [dict(name=f"el{n}+{4 * m}B", shape=(n,), mis=m, kind=0) for n in (1, 4095, 4096, 4097) for m in (0, 3)]
    es = el[:5] + [dict(name="zero", shape=(0,), mis=0, kind=0)] + el[5:] + [k2t, k3, k1, k2] + el + [k2t, k1, el[6], el[7]]
    if all_live:
        es[5], es[10] = el[2], el[3]
    assert len(es) == E.SGD_MAX_TENSORS + 1 and es[24]["shape"] == (4097,) and es[24]["mis"] == 3
    assert sum(e["kind"] != 3 and e["shape"] != (0,) for e in es[:24]) == (24 if all_live else 22)
    return es


def _sgd_entry(i, e, sdt, first):
    """entry i on fresh device copies -> (ops.sgd_multi entry, its tensors and staged outputs)"""
    w, g, buf = E.sgd_state(i, e, 0 if first else 1)
    pd, gd, bd = _dev(w, "f32", e["mis"]), _dev(g, "f32", e["mis"]), _dev(buf, "f32", e["mis"])
    (lr, wd), _ = E.sgd_hyper(i)
    s0 = s1 = st = None
    if e["kind"] == 1:
        s0 = _Out((e["shape"][0], e["d0"]), sdt, 0, ld=e["ld0"])
    elif e["kind"] == 2:
        s0 = _Out((e["d0"] * 9, e["d1"]), sdt, 0, ld=e["d2"])
        s1 = _Out((e["d1"] * 9, e["d0"]), sdt, 0, ld=e["d0"])
    elif e["kind"] == 3:
        s0 = _Out((e["shape"][0], e["d0"]), sdt, 0, ld=e["ld0"])
        s1 = _Out((e["d0"], e["shape"][0]), sdt, 0, ld=e["ld1"])
    if e["kind"]:
        st = dict(kind=e["kind"], dtype=_tdt(sdt), stage0=s0.t, stage1=None if s1 is None else s1.t,
                  d0=e["d0"], d1=e.get("d1", 0), d2=e.get("d2", 0), ld0=e.get("ld0", 0), ld1=e.get("ld1", 0))
    return dict(param=pd, grad=gd, buf=bd, lr=lr, weight_decay=wd, first=first, staging=st), (pd, bd, s0, s1)


@pytest.mark.parametrize("all_live", [False, True], ids=["skips", "full_table"])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("sdt", E.DTYPES)
def test_sgd_multi_across_the_launch_seam_equals_each_entry_alone(ops, sdt, first, all_live):
    """25 entries in one call: parameter, momentum buffer and every staged copy bit for bit what the same entry gives as a call of
    its own, and parameter and buffer within sgd_bounds of float64"""
    es = _sgd_seam_entries(all_live)
    made = [_sgd_entry(i, e, sdt, first) for i, e in enumerate(es)]
    ops.sgd_multi([m[0] for m in made], _MOM, _GSCALE)
    torch.cuda.synchronize()
    ratios = {}
    for i, e in enumerate(es):
        entry, alone = _sgd_entry(i, e, sdt, first)
        ops.sgd_multi([entry], _MOM, _GSCALE)
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(made[i][1], alone)):
            if a is not None:
                a, b = (a.cpu().numpy(), b.cpu().numpy()) if k < 2 else (a.host(), b.host())
                assert E.same_bits(a, b), (e["name"], i, ("param", "buf", "stage0", "stage1")[k])
        w, g, buf = E.sgd_state(i, e, 0 if first else 1)
        _sgd_check(e["name"], made[i][1][0].cpu().numpy(), made[i][1][1].cpu().numpy(), w, g, buf, entry["lr"], entry["weight_decay"],
                   first, ratios, E.sgd_form(e))
    assert set(ratios) == {"conv_tile", "vector", "scalar"} | (set() if all_live else {"tile64"})


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_sgd_momentum_step_against_float64(ops, first):
    ratios = {}
    for i, n in enumerate(E.SGD_ELEMENT_N):
        for mis in (0, 3):
            w, g, buf = E.sgd_state(100 + i, dict(shape=(n,)), 0 if first else 1)
            if first:
                buf = np.full_like(buf, np.nan)
            pd, gd, bd = _dev(w, "f32", mis), _dev(g, "f32", mis), _dev(buf, "f32", mis)
            (lr, wd), _ = E.sgd_hyper(i + 1)
            ops.sgd_momentum_step(pd, gd, bd, lr, _MOM, wd, first, _GSCALE)
            torch.cuda.synchronize()
            _sgd_check(f"n{n}+{mis}", pd.cpu().numpy(), bd.cpu().numpy(), w, g, buf, lr, wd, first, ratios, "single")
    print("sgd_momentum_step", "first" if first else "later", "max error / bound:", round(ratios["single"], 3))


# ------------------------------------------------------------------------------------------------ EMA
@pytest.mark.parametrize("keep", E.EMA_KEEPS)
def test_ema_multi_two_launches_bit_for_bit(ops, keep):
    te, st = E.ema_inputs()
    want = E.ema_ref(te, st, keep)
    outs = [_Out((t.size,), "f32") for t in te]
    for o, t in zip(outs, te):
        if t.size:
            o.t.copy_(torch.from_numpy(t))
    sd = [torch.from_numpy(s).cuda() for s in st]
    ops.ema_multi([o.t for o in outs], sd, keep)
    for i, (o, s) in enumerate(zip(outs, sd)):
        assert E.same_bits(o.host(), want[i]), (i, keep)
        assert E.same_bits(s.cpu().numpy(), st[i])
    if keep == 0.0:
        assert np.isnan(outs[E.EMA_INF_AT[0]].host()[E.EMA_INF_AT[1]])


# ------------------------------------------------------------------------------------------------ scalars and packing
def test_weighted_sum_and_scale_scalars(ops, kernel_error):
    for n in E.WS_N:
        v, w = E.weighted_sum_inputs(n)
        pool = _dev(v)
        vals = [pool[i:i + 1] for i in range(n)]
        out = _Out((n + 1,), "f32")
        ops.weighted_sum(vals, list(w), out.t)
        assert E.same_bits(out.host(), E.weighted_sum_ref(v, w)), n
        g = torch.tensor([1.7], device="cuda")
        out = _Out((n,), "f32")
        ops.scale_scalars(g, list(w), out.t)
        assert E.same_bits(out.host(), (np.float32(1.7) * w).astype(np.float32)), n
    for n in (E.WS_MAX + 1, 0):
        pool = torch.ones(max(n, 1), device="cuda")
        out = _Out((n + 1,), "f32")
        with pytest.raises(kernel_error, match="-5"):
            ops.weighted_sum([pool[i:i + 1] for i in range(n)], [1.0] * n, out.t)
        out.assert_untouched()
        out = _Out((max(n, 1),), "f32")
        with pytest.raises(kernel_error, match="-5"):
            ops.scale_scalars(pool[:1], [1.0] * n, out.t)
        out.assert_untouched()


def test_counter_add_crosses_2_32_and_wraps_2_64(ops):
    for start, inc in E.COUNTER_CASES:
        signed = lambda v: v - (1 << 64) if v >= (1 << 63) else v
        buf = torch.tensor([7, signed(start), 7], dtype=torch.int64, device="cuda")
        ops.counter_add(buf[1:2], inc)
        torch.cuda.synchronize()
        assert buf.tolist() == [7, signed((start + inc) % (1 << 64)), 7], (start, inc)


@pytest.mark.parametrize("seed", E.DROPOUT_SEEDS, ids=["seed-small", "seed-2^63+"])
@pytest.mark.parametrize("n", E.DROPOUT_N)
def test_dropout_mask_is_the_splitmix64_stream(ops, n, seed):
    for p in E.DROPOUT_P:
        for off in (0, 777):
            buf = torch.full((n + E.SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
            ops.dropout_mask(buf[:n], seed, off, p)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert (got[n:] == 0xA5).all()
            assert np.array_equal(got[:n], E.dropout_ref(n, seed, off, p)), (n, seed, p, off)
            if p == 0.0:
                assert got[:n].all()
            if p == 1.0:
                assert not got[:n].any()
    k = 13
    a = torch.empty(n, dtype=torch.uint8, device="cuda"); b = torch.empty(n - k, dtype=torch.uint8, device="cuda")
    ops.dropout_mask(a, seed, 0, 0.3); ops.dropout_mask(b, seed, k, 0.3)
    assert torch.equal(a[k:], b) and 0.6 < float(a.float().mean()) < 0.8


@pytest.mark.parametrize("R", E.PACK_R)
def test_pack_views_layout(ops, R):
    r = np.random.default_rng(R)
    bx = [r.normal(50.0, 20.0, (R, 4)).astype(np.float32) for _ in range(4)]
    ob = [r.normal(0.0, 1.0, R).astype(np.float32) for _ in range(4)]
    boxes, obj, rois = _Out((4, R, 4), "f32"), _Out((4, R), "f32"), _Out((2, 2 * R, 5), "f32")
    ops.pack_views([_dev(b) for b in bx], [_dev(o) for o in ob], boxes.t, obj.t, rois.t)
    wb, wo, wr = E.pack_views_ref(bx, ob)
    assert E.same_bits(boxes.host(), wb) and E.same_bits(obj.host(), wo) and E.same_bits(rois.host(), wr)
    assert set(np.unique(rois.host()[:, :, 0])) == {0.0, 1.0}


# ------------------------------------------------------------------------------------------------ grid-stride second pass
def test_grid_stride_second_pass_pool_forward(ops):
    p = E.GRID_POOL
    r = np.random.default_rng(1)
    x = E.round_to(r.normal(0.0, 1.0, (p["N"], p["H"], p["W"], p["C"])), p["dtype"])
    want, _ = E.maxpool_fwd_ref(x, p["stride"])
    out = _Out(want.shape, p["dtype"])
    ops.maxpool_fwd(_dev(x, p["dtype"]), out.t, p["stride"])
    assert E.same_bits(out.host(), want)


def test_grid_stride_second_pass_relu_bwd(ops):
    n = E.GRID_RELU_N
    r = np.random.default_rng(2)
    ref = r.normal(0.0, 1.0, n).astype(np.float32); g = r.normal(0.0, 1.0, n).astype(np.float32)
    out = _Out((n,), "f32")
    ops.relu_bwd(_dev(ref), _dev(g), out=out.t)
    assert np.array_equal(E.bits(out.host()), E.relu_bwd_ref(ref, g))


def test_grid_stride_second_pass_convert_2d(ops):
    rows, cols = E.GRID_CONVERT
    m = np.random.default_rng(3).normal(0.0, 1.0, (rows, cols)).astype(np.float32)
    out = _Out((rows, cols), "bf16", 0, ld=cols + 8)
    ops.convert_2d(_dev(m), out.t, rows, cols)
    assert E.same_bits(out.host(), E.round_to(m, "bf16"))


# ------------------------------------------------------------------------------------------------ NaN through the forward ReLU / max sites
_BAR = {"bf16": 1e-2, "f32": 3e-5}        # bf16 output rounding / f32 accumulation: the bars of tests/test_gpu_kernels.py


def _assert_nan_like_reference(got, ref, out_dtype, what):
    """isnan(out) == isnan(ref), and the usual bar elsewhere"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    assert nan.any() and not nan.all(), what
    assert np.array_equal(np.isnan(got), nan), f"{what}: {int((np.isnan(got) != nan).sum())} elements differ in NaN-ness from relu(float64)"
    err = E.rel_err(got[~nan], ref[~nan])
    assert err < _BAR[out_dtype], (what, err)


def _poison(kind, x, at, w_zero, b):
    """put the NaN where `kind` says: x[at] = NaN; x[at] = +inf against the weights w_zero (a view), set to zero; b[5] = NaN"""
    if kind == "nan_input":
        x[at] = float("nan")
    elif kind == "inf_times_zero":
        x[at] = float("inf")
        w_zero.zero_()
    else:
        b[5] = float("nan")


@pytest.mark.parametrize("kind", E.NAN_KINDS)
@pytest.mark.parametrize("key", list(E.NAN_CONV_CASES))
def test_conv3x3_relu_epilogues_keep_nan(ops, key, kind):
    """a NaN input, +inf against a zero weight and a NaN bias through bias + ReLU of each epilogue of the direct convolution: NaN
    exactly where float64 relu(conv2d) of the same operands has it (fmaxf(NaN, 0) = 0 would hide a diverged activation)"""
    n, H, W, cin, cout, od = E.NAN_CONV_CASES[key]
    real = 3 if key == "first_layer" else cin
    g = torch.Generator().manual_seed(H * 100 + W + cin)
    x = torch.zeros(n, H, W, cin); x[..., :real] = torch.randn(n, H, W, real, generator=g) * 0.7
    w = torch.zeros(cout, cin, 3, 3); w[:, :real] = torch.randn(cout, real, 3, 3, generator=g) * 0.05
    b = torch.randn(cout, generator=g) * 0.1
    x, w = x.bfloat16(), w.bfloat16()
    _poison(kind, x, (0, H // 2, W // 2, 1), w[:, 1], b)
    with np.errstate(invalid="ignore"):
        ref = F.relu(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1).numpy()
    wk = torch.empty(cout, 9, cin, device="cuda", dtype=torch.bfloat16)
    ops.conv_weight_prep(w.float().cuda(), wk, 0, cin)
    out = _Out((n, H, W, cout), od)
    ops.conv3x3(x.cuda(), wk, out.t, 1, ops.make_epilogue(bias=b.cuda(), relu=True, out_dtype=_tdt(od)))
    _assert_nan_like_reference(out.host(), ref, od, (key, kind))


@pytest.mark.parametrize("kind", E.NAN_KINDS)
def test_conv3x3_relu_pool2_keeps_nan_and_equals_the_unfused_pair(ops, kind):
    n, H, W, cin, cout = E.NAN_POOL_CASE
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    x = (torch.randn(n, H, W, cin, device="cuda", generator=g) * 0.7).to(torch.bfloat16)
    w = (torch.randn(cout, cin, 3, 3, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(cout, device="cuda", generator=g) * 0.1
    _poison(kind, x, (0, 21, 101, 1), w[:, 1], b)
    ref = F.max_pool2d(F.relu(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)), 2, 2).permute(0, 2, 3, 1).cpu().numpy()
    wk = torch.empty(cout, 9, cin, device="cuda", dtype=torch.bfloat16)
    ops.conv_weight_prep(w.float(), wk, 0, cin)
    full = torch.empty(n, H, W, cout, device="cuda", dtype=torch.bfloat16)
    ops.conv3x3(x, wk, full, 1, ops.make_epilogue(bias=b, relu=True, out_dtype=torch.bfloat16))
    oh, ow = E.pool_out_hw(H, W, 2)
    pair = _Out((n, oh, ow, cout), "bf16")
    ops.maxpool_fwd(full, pair.t, 2)
    fused = _Out((n, oh, ow, cout), "bf16")
    assert ops.conv3x3_relu_pool2(x, wk, b, fused.t)
    got = fused.host()
    _assert_nan_like_reference(got, ref, "bf16", ("relu_pool2", kind))
    assert torch.equal(fused.t.view(torch.int16), pair.t.view(torch.int16)), "the fused launch equals conv + pool bit for bit, NaN included"
    pair.host()


@pytest.mark.parametrize("kind", E.NAN_KINDS)
@pytest.mark.parametrize("c", E.NAN_GEMM_CASES, ids=[c[0] for c in E.NAN_GEMM_CASES])
def test_gemm_relu_epilogues_keep_nan(ops, c, kind):
    site, M, N, K, idt, odt, sk = c
    g = torch.Generator(device="cuda"); g.manual_seed(M + N + K)
    a = torch.randn(M, K, device="cuda", generator=g).to(_tdt(idt))
    bm = torch.randn(N, K, device="cuda", generator=g).to(_tdt(idt))
    bias = torch.randn(N, device="cuda", generator=g)
    _poison(kind, a, (M // 2, 11), bm[:, 11], bias)
    ref = F.relu(a.double() @ bm.double().t() + bias.double()).cpu().numpy()
    ldc = ((N + 15) // 8) * 8
    out = _Out((M, N), odt, 0, ld=ldc)
    ops.gemm(a, bm, out.t, M, N, K, ep=ops.make_epilogue(bias=bias, relu=True, out_dtype=_tdt(odt)), splitk=sk)
    _assert_nan_like_reference(out.host(), ref, odt, (site, kind))

"""GPU: the dense kernels of the Stage-3 detector (csrc/detector.hip, the RPN layout kernels and sw_scale_col_blocks of
csrc/proposals.hip) against the restatements of tests/detector_ref.py at their edges: f32 and bf16, the scalar twins of the vector
kernels (C % V != 0, a view one element into a buffer), partial and single stem tiles, -inf / NaN / signed zeros through the
selections, both forms of the ROIAlign backward (per-axis registers up to grid 8, sample by sample from 9, the mixed case),
PH != PW, a fixed sampling ratio, row pitches, shuffled and device-counted row lists, every RPN level geometry.  Every output buffer
starts as a NaN with a payload no kernel writes and has slack behind its end: what the contract says is written must be finite
(where the inputs are) and exact or within the bar of detector_ref.E32 (taken from the float32 error of the reference formula, never
from the kernel); everything else must still hold the sentinel.  No element is masked and no case skipped;
tests/test_detector_ref_cpu.py asserts that the case tables reach the edges they are named for."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detector_ref as D  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


_F32_SENTINEL, _BF16_SENTINEL = 0x7FA5A5A5, 0x7FA5


def _sent(n, dtype=torch.float32):
    if dtype == torch.float32:
        return torch.full((n,), _F32_SENTINEL, device="cuda", dtype=torch.int32).view(torch.float32)
    return torch.full((n,), _BF16_SENTINEL, device="cuda", dtype=torch.int16).view(torch.bfloat16)


def _untouched(t):
    """bool tensor: the element still holds the sentinel bits"""
    if t.dtype == torch.float32:
        return t.view(torch.int32) == _F32_SENTINEL
    return t.view(torch.int16) == _BF16_SENTINEL


class _Out:
    """an output of `shape` inside a sentinel-filled buffer: `mis` elements in front (1 = not 16-byte aligned), SLACK behind"""

    def __init__(self, shape, dtype, mis=0):
        self.n = int(np.prod(shape)); self.mis = mis
        self.buf = _sent(mis + self.n + D.SLACK, D.torch_dtype(dtype) if isinstance(dtype, str) else dtype)
        self.t = self.buf[mis:mis + self.n].view(*shape)

    def host(self):
        """float32 numpy of the output, after checking that nothing around it was written and all of it was"""
        torch.cuda.synchronize()
        assert bool(_untouched(self.buf[:self.mis]).all() and _untouched(self.buf[self.mis + self.n:]).all()), "written outside the output"
        assert not bool(_untouched(self.t).any()), "an element of the output was not written"
        return self.t.float().cpu().numpy()


def _dev(x, dtype="f32", mis=0):
    """float32 numpy (values of `dtype`) -> device tensor of `dtype`; mis = 1: a view one element into a larger buffer"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(D.torch_dtype(dtype))
    if not mis:
        return t.cuda()
    buf = torch.full((t.numel() + mis,), float("nan"), dtype=t.dtype, device="cuda")
    buf[mis:] = t.reshape(-1).cuda()
    return buf[mis:].view(*t.shape)


def _close(kind, dtype, got, ref, what, out_bf16):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{what}: {kind} holds non-finite values"
    d = float(np.max(np.abs(got - ref))) if got.size else 0.0
    a = D.allowed(kind, dtype, ref, out_bf16)
    m = float(np.max(np.abs(ref))) if got.size else 0.0
    print(f"{what} {kind}[{dtype}]: err {d / m if m else d:.3g} of max|ref|, bar {a / m if m else a:.3g}")
    assert d <= a, f"{what}: {kind} off by {d:.3g} (allowed {a:.3g}, max|ref| {m:.3g})"


_VARIANTS = (("aligned", 0, 0), ("in+1", 1, 0), ("out+1", 0, 1), ("both+1", 1, 1))


# ------------------------------------------------------------------------------------------------ preprocess_pad
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("c", D.PREPROCESS_CASES, ids=[f"{c[0]}x{c[1]}-in-{c[2]}x{c[3]}-std{c[5][0]:g}" for c in D.PREPROCESS_CASES])
def test_preprocess_pad_bit_exact(ops, c, dtype):
    h, w, H, W, mean, std = c
    img = D.preprocess_inputs(h, w)
    want = D.round_to(D.preprocess_ref(img, H, W, mean, std), dtype)
    out = _Out((H, W, 4), dtype)
    ops.preprocess_pad(torch.from_numpy(img).cuda(), out.t, mean, std)
    got = out.host()
    assert D.same_bits(got, want)
    assert not got[h:].any() and not got[:, w:].any() and not got[..., 3].any()            # padding and channel 3: exactly 0


# ------------------------------------------------------------------------------------------------ stem_conv7x7
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("c", D.STEM_CASES, ids=[f"N{c[0]}-{c[1]}x{c[2]}" for c in D.STEM_CASES])
def test_stem_conv7x7_against_float64(ops, c, dtype):
    N, H, W = c
    x, w, sc, sh = D.stem_inputs(N, H, W, dtype)
    ref = D.stem_ref(x, w, sc, sh)
    out = _Out(ref.shape, dtype)
    ops.stem_conv7x7(_dev(x, dtype), _dev(w), _dev(sc), _dev(sh), out.t)                    # channel 3 of x holds NaN: never read
    got = out.host()
    _close("stem", dtype, got, ref, f"N{N}-{H}x{W}", dtype == "bf16")
    assert 0.2 < float((got == 0).mean()) < 0.8                                              # the ReLU cut


def test_stem_conv7x7_propagates_nan_like_relu_of_conv2d(ops):
    N, H, W = 1, 17, 15
    x, w, sc, sh = D.stem_inputs(N, H, W, "f32")
    x = x.copy(); x[0, 8, 7, 1] = np.nan
    with np.errstate(invalid="ignore"):
        ref = D.stem_ref(x, w, sc, sh)
    out = _Out(ref.shape, "f32")
    ops.stem_conv7x7(_dev(x), _dev(w), _dev(sc), _dev(sh), out.t)
    got = out.host()
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "a NaN pixel must reach every output whose window holds it, and no other"


# ------------------------------------------------------------------------------------------------ maxpool3x3s2
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("c", D.POOL_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in D.POOL_CASES])
def test_maxpool3x3s2_bit_exact_against_max_pool2d(ops, c, dtype):
    """every regime (ordinary, all negative, -inf / NaN / signed zeros) on the path the shape takes, and the scalar twin through a
    misaligned input or output; detector_ref.maxpool_ref is F.max_pool2d bit for bit (test_detector_ref_cpu.py)"""
    H, W, C = c
    N = 2
    for regime in D.POOL_REGIMES:
        x = D.pool_inputs(N, H, W, C, dtype, regime)
        want = D.maxpool_ref(x)
        for name, mi, mo in (_VARIANTS if D.takes_vector_path(C, dtype) else _VARIANTS[:1]):
            out = _Out(want.shape, dtype, mo)
            ops.maxpool3x3s2(_dev(x, dtype, mi), out.t)
            assert D.same_bits(out.host(), want), (c, dtype, regime, name)


# ------------------------------------------------------------------------------------------------ subsample2x / scatter2x
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("c", D.SUB_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in D.SUB_CASES])
def test_subsample2x_and_scatter2x_bit_exact(ops, c, dtype):
    H, W, C = c
    for N in (1, 2):
        x = D.dense_inputs(41, (N, H, W, C), dtype)
        x[0, 0, 0, 0] = np.nan; x[-1, -1, -1, -1] = -0.0                                    # copies: bits, not values
        want = D.subsample_ref(x)
        back = D.scatter_ref(want, H, W)
        for name, mi, mo in (_VARIANTS if D.takes_copy16_path(C, dtype) else _VARIANTS[:1]):
            out = _Out(want.shape, dtype, mo)
            ops.subsample2x(_dev(x, dtype, mi), out.t)
            assert D.same_bits(out.host(), want), (c, dtype, N, name)
            out = _Out(x.shape, dtype, mo)                                                   # every element of the sentinel-filled map
            ops.scatter2x(_dev(want, dtype, mi), out.t)
            got = out.host()
            assert D.same_bits(got, back), (c, dtype, N, name)
            assert not np.signbit(got[:, 1::2]).any() and not np.signbit(got[:, :, 1::2]).any()


# ------------------------------------------------------------------------------------------------ add_relu
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n", D.ADD_N)
def test_add_relu_bit_exact_with_nan_and_signed_zero(ops, n, relu, dtype):
    a, b = D.add_inputs(n, dtype)
    want = D.add_relu_ref(a, b, relu, dtype)
    out = _Out((n,), dtype)
    ops.add_relu(_dev(a, dtype), _dev(b, dtype), out.t, relu=bool(relu))
    got = out.host()
    assert D.same_bits(got, want)
    if n >= 255:
        assert np.isnan(got[3]) and np.isnan(got[7]) and np.isnan(got[n - 1]), "NaN in a or b gives NaN"
        assert np.signbit(got[11]) and got[11] == 0                                          # (-0) + (-0) = -0, kept by torch's relu


# ------------------------------------------------------------------------------------------------ upsample2x_add / downsample2x_sum
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("c", D.FPN_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in D.FPN_CASES])
def test_upsample2x_add_bit_exact(ops, c, dtype):
    h, w, C = c
    for N in D.FPN_N:
        top = D.dense_inputs(43, (N, h, w, C), dtype); lat = D.dense_inputs(44, (N, 2 * h, 2 * w, C), dtype)
        want = D.upsample_add_ref(lat, top, dtype)
        for name, mi, mo in (_VARIANTS if D.takes_vector_path(C, dtype) else _VARIANTS[:1]):
            out = _Out(want.shape, dtype, mo)
            ops.upsample2x_add(_dev(lat, dtype, mi), _dev(top, dtype), out.t)
            assert D.same_bits(out.host(), want), (c, dtype, N, name)
        if D.takes_vector_path(C, dtype):                                                    # only `top` misaligned
            out = _Out(want.shape, dtype)
            ops.upsample2x_add(_dev(lat, dtype), _dev(top, dtype, 1), out.t)
            assert D.same_bits(out.host(), want), (c, dtype, N, "top+1")


@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("c", D.FPN_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in D.FPN_CASES])
def test_downsample2x_sum_exact_order_and_against_float64(ops, c, dtype):
    h, w, C = c
    for N in D.FPN_N:
        g = D.dense_inputs(45, (N, 2 * h, 2 * w, C), dtype)
        want = D.round_to(D.downsample_sum_f32(g), dtype)                                    # (a + b) + (c + d) in float32, one rounding
        ref = D.downsample_sum_ref(g)
        for name, mi, mo in (_VARIANTS if D.takes_vector_path(C, dtype) else _VARIANTS[:1]):
            out = _Out(want.shape, dtype, mo)
            ops.downsample2x_sum(_dev(g, dtype, mi), out.t)
            got = out.host()
            assert D.same_bits(got, want), (c, dtype, N, name)
            _close("downsample", dtype, got, ref, f"N{N}-{h}x{w}x{C}-{name}", dtype == "bf16")
        if dtype == "f32":
            # adjoint identity in float64: <upsample(top), g> = <top, downsample(g)>.  The upsampling onto a zero lateral is exact; each
            # downsampled sum carries at most 3 * 2^-24 of the sum of its four magnitudes ((a + b) + (c + d): three roundings).
            top = D.dense_inputs(43, (N, h, w, C), dtype)
            up = _Out(g.shape, dtype); ops.upsample2x_add(_dev(np.zeros_like(g)), _dev(top), up.t)
            down = _Out(top.shape, dtype); ops.downsample2x_sum(_dev(g), down.t)
            lhs = float((up.host().astype(np.float64) * g).sum()); rhs = float((top.astype(np.float64) * down.host()).sum())
            slack = 3 * 2.0 ** -24 * float((np.abs(top).astype(np.float64) * D.downsample_sum_ref(np.abs(g))).sum())
            assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)


# ------------------------------------------------------------------------------------------------ ROIAlign
def _roi_dev():
    rois = D.roi_set()
    return torch.from_numpy(rois).cuda(), len(rois)


@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("cfg", D.ROI_CONFIGS, ids=[f"{a}x{b}-sr{s}" for a, b, s in D.ROI_CONFIGS])
@pytest.mark.parametrize("C", D.ROI_C)
def test_roi_align_fwd_against_float64(ops, C, cfg, dtype):
    PH, PW, sr = cfg
    rois, R = _roi_dev()
    ref = D.roi_fwd_expected(C, cfg, dtype).reshape(R, -1)
    n = C * PH * PW
    feat = _dev(D.roi_feat(C, dtype), dtype)
    out = _Out((R, n), dtype)
    ops.roi_align_fwd(feat, rois, torch.arange(R, dtype=torch.int32, device="cuda"), out.t, D.ROI_SCALE, PH, PW, sr)
    got = out.host()
    _close("roi_fwd", dtype, got, ref, f"C{C}-{PH}x{PW}-sr{sr}", dtype == "bf16")
    assert not got[ref.any(1) == 0].any(), "a ROI outside the map or without area pools exact zeros"


@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("mode", ["pitch", "shuffled", "device-count"])
def test_roi_align_fwd_row_pitch_row_list_and_device_count(ops, mode, dtype):
    """out with a row pitch of C*PH*PW + 5; `sel` shuffled with gaps; n_sel_dev = half of len(sel): only the listed rows are written,
    the pitch padding and every other row keep the sentinel"""
    C, cfg = 3, (7, 7, 0)
    PH, PW, sr = cfg
    rois, R = _roi_dev()
    ref = D.roi_fwd_expected(C, cfg, dtype).reshape(R, -1)
    n = C * PH * PW
    pitch = n + 5
    sel = np.arange(R, dtype=np.int32) if mode == "pitch" else D.roi_sel_shuffled()
    n_dev = len(sel) // 2 if mode == "device-count" else None
    listed = sel[:n_dev] if n_dev is not None else sel
    buf = _sent((R + 1) * pitch + D.SLACK, D.torch_dtype(dtype))
    out = buf[:(R + 1) * pitch].view(R + 1, pitch)
    ops.roi_align_fwd(_dev(D.roi_feat(C, dtype), dtype), rois, torch.from_numpy(sel).cuda(), out[:R, :n], D.ROI_SCALE, PH, PW, sr,
                      n_sel_dev=None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert out[:R, :n].stride(0) == pitch
    rows = torch.from_numpy(np.sort(listed).astype(np.int64)).cuda()
    assert not bool(_untouched(out[rows][:, :n]).any())
    _close("roi_fwd", dtype, out[rows][:, :n].float().cpu().numpy(), ref[np.sort(listed)], f"{mode}", dtype == "bf16")
    rest = torch.ones(R + 1, dtype=torch.bool, device="cuda"); rest[rows] = False
    assert int(rest.sum()) == R + 1 - len(listed)
    assert bool(_untouched(out[rest]).all()), "a row that is not listed was written"
    assert bool(_untouched(out[:, n:]).all()), "the pitch padding was written"
    assert bool(_untouched(buf[(R + 1) * pitch:]).all())


def _gout_dev(C, PH, PW, dtype):
    """the output gradient with a row pitch of C*PH*PW + 5 whose padding holds NaN (never read) -> (view (R, n), contiguous copy)"""
    g = D.roi_gout(C, PH, PW, dtype)
    R = g.shape[0]; n = C * PH * PW
    buf = torch.full((R, n + 5), float("nan"), dtype=D.torch_dtype(dtype), device="cuda")
    buf[:, :n] = _dev(g.reshape(R, n), dtype)
    return buf[:, :n], buf[:, :n].contiguous()


@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("cfg", D.ROI_CONFIGS, ids=[f"{a}x{b}-sr{s}" for a, b, s in D.ROI_CONFIGS])
@pytest.mark.parametrize("C", D.ROI_C)
def test_roi_align_bwd_both_forms_against_float64(ops, C, cfg, dtype):
    """the f32-atomic and the fixed-point backward on the ROI set that holds grids 1 .. 12 (register form up to 8, sample by sample
    from 9, mixed): each within the bar of float64, the fixed-point form bit-equal over two runs and within the bar of the atomic one"""
    PH, PW, sr = cfg
    rois, R = _roi_dev()
    ref = D.roi_bwd_expected(C, cfg, dtype)
    shape = (D.ROI_N, D.ROI_H, D.ROI_W, C)
    gv, gc = _gout_dev(C, PH, PW, dtype)
    sel = torch.arange(R, dtype=torch.int32, device="cuda")
    what = f"C{C}-{PH}x{PW}-sr{sr}"
    d = torch.zeros(int(np.prod(shape)) + D.SLACK, device="cuda")
    ops.roi_align_bwd(gv, rois, sel, d[:-D.SLACK].view(*shape), D.ROI_SCALE, PH, PW, sr)
    torch.cuda.synchronize()
    assert not bool(d[-D.SLACK:].any())
    atomic = d[:-D.SLACK].view(*shape).cpu().numpy()
    _close("roi_bwd", dtype, atomic, ref, what + "-atomic", False)
    amax = ops.absmax(gc)
    assert float(amax) == float(np.abs(D.roi_gout(C, PH, PW, dtype)).max())

    def fx():
        acc = torch.zeros(int(np.prod(shape)) + D.SLACK, device="cuda", dtype=torch.int64)
        ops.roi_align_bwd_fx(gv, rois, sel, acc[:-D.SLACK].view(*shape), D.ROI_SCALE, amax, PH, PW, sr)
        out = _Out(shape, "f32")
        ops.fx_to_float(acc[:-D.SLACK].view(*shape), amax, out.t)
        got = out.host()
        assert not bool(acc[-D.SLACK:].any())
        return got
    a, b = fx(), fx()
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the fixed-point form must be bit-equal over two runs"
    _close("roi_bwd", dtype, a, ref, what + "-fixed-point", False)
    _close("roi_bwd", dtype, a, atomic.astype(np.float64), what + "-fixed-point-vs-atomic", False)
    out16 = _Out(shape, "bf16")
    acc = torch.zeros(shape, device="cuda", dtype=torch.int64)
    ops.roi_align_bwd_fx(gv, rois, sel, acc, D.ROI_SCALE, amax, PH, PW, sr)
    ops.fx_to_float(acc, amax, out16.t)
    _close("roi_bwd", dtype, out16.host(), ref, what + "-fixed-point-bf16-map", True)


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_roi_align_bwd_shuffled_row_list_with_device_count(ops, dtype):
    C, cfg = 3, (7, 7, 0)
    PH, PW, sr = cfg
    rois, R = _roi_dev()
    sel = D.roi_sel_shuffled(); n_dev = len(sel) // 2
    listed = sel[:n_dev].astype(np.int64)
    shape = (D.ROI_N, D.ROI_H, D.ROI_W, C)
    ref = D.roi_align_bwd_ref(D.roi_gout(C, PH, PW, dtype)[listed], D.roi_set()[listed], PH, PW, sr, shape)
    gv, gc = _gout_dev(C, PH, PW, dtype)
    sel_d = torch.from_numpy(sel).cuda(); cnt = torch.tensor([n_dev], dtype=torch.int32, device="cuda")
    d = torch.zeros(shape, device="cuda")
    ops.roi_align_bwd(gv, rois, sel_d, d, D.ROI_SCALE, PH, PW, sr, n_sel_dev=cnt)
    _close("roi_bwd", dtype, d.cpu().numpy(), ref, "listed-atomic", False)
    amax = ops.absmax(gc)                                       # an upper bound of the listed rows' gradients
    acc = torch.zeros(shape, device="cuda", dtype=torch.int64)
    ops.roi_align_bwd_fx(gv, rois, sel_d, acc, D.ROI_SCALE, amax, PH, PW, sr, n_sel_dev=cnt)
    out = _Out(shape, "f32")
    ops.fx_to_float(acc, amax, out.t)
    _close("roi_bwd", dtype, out.host(), ref, "listed-fixed-point", False)


# ------------------------------------------------------------------------------------------------ rpn_unpack / rpn_unpack_bwd
def _hw_arg(hw):
    return (ctypes.c_int * len(hw))(*[int(v) for v in hw])


def _unpack(ops, y, N, A, hw, ld):
    """sw_rpn_unpack into sentinel-filled outputs (ops.rpn_unpack allocates its own)"""
    At = A * int(sum(hw))
    lo, do = _Out((N, At), "f32"), _Out((N, At, 4), "f32")
    ops.check(ops.lib.sw_rpn_unpack(N, len(hw), A, _hw_arg(hw), ops._p(y), ld, ops._p(lo.t), ops._p(do.t), ops._stream()), "sw_rpn_unpack")
    return lo.host(), do.host()


_RPN_IDS = [f"N{c[0]}-A{c[1]}-L{len(c[2])}-ld{c[3]}" for c in D.RPN_CASES]


@pytest.mark.parametrize("c", D.RPN_CASES, ids=_RPN_IDS)
def test_rpn_unpack_bit_exact_against_the_layout(ops, c):
    N, A, hw, ld = c
    y = D.rpn_inputs(N, A, hw, ld)[0]                            # NaN in the padding columns: never read
    wl, wd = D.rpn_unpack_ref(y, N, A, hw)
    gl, gd = _unpack(ops, _dev(y), N, A, hw, ld)
    assert D.same_bits(gl, wl) and D.same_bits(gd, wd)
    l2, d2 = ops.rpn_unpack(_dev(y), N, A, hw)                   # the wrapper the detector calls
    assert D.same_bits(l2.cpu().numpy(), wl) and D.same_bits(d2.cpu().numpy(), wd)


@pytest.mark.parametrize("scalars", [True, False], ids=["device-scalars", "no-scalars"])
@pytest.mark.parametrize("which", ["both", "dlogits", "ddeltas"])
@pytest.mark.parametrize("c", D.RPN_CASES, ids=_RPN_IDS)
def test_rpn_unpack_bwd_bit_exact_and_round_trip(ops, c, which, scalars):
    N, A, hw, ld = c
    _, dl, dd, gl, gd = D.rpn_inputs(N, A, hw, ld)
    if not scalars:
        gl = gd = None
    dl_in, dd_in = (dl if which != "ddeltas" else None), (dd if which != "dlogits" else None)
    want = D.rpn_unpack_bwd_ref(dl_in, dd_in, gl, gd, N, A, hw, ld)
    rows = D.rpn_rows(N, hw)
    out = _Out((rows, ld), "f32")                                # every element of the sentinel-filled dy is overwritten
    t = [None if v is None else _dev(v) for v in (dl_in, dd_in)]
    s = [None if v is None else _dev(np.array([v], np.float32)) for v in (gl, gd)]
    ops.check(ops.lib.sw_rpn_unpack_bwd(N, len(hw), A, _hw_arg(hw), ops._p(t[0]), ops._p(t[1]), ops._p(s[0]), ops._p(s[1]), ops._p(out.t),
                                        ld, ops._stream()), "sw_rpn_unpack_bwd")
    got = out.host()
    assert D.same_bits(got, want)
    assert not got[:, 5 * A:].any() and not np.signbit(got[:, 5 * A:]).any(), "padding columns must be exactly 0"
    _close("rpn_scale", "f32", got, D.rpn_unpack_bwd_ref(dl_in, dd_in, gl, gd, N, A, hw, ld, np.float64), "rpn_unpack_bwd", False)
    if which == "both":
        dy = ops.rpn_unpack_bwd(t[0], t[1], N, A, hw, rows, ld, "cuda", g_logits=s[0], g_deltas=s[1])     # the detector's wrapper
        assert D.same_bits(dy.cpu().numpy(), want)
        l2, d2 = _unpack(ops, dy, N, A, hw, ld)                  # round trip: (dl * g, dd * g) bit for bit
        one = np.float32(1.0)
        assert D.same_bits(l2, dl * (one if gl is None else gl)) and D.same_bits(d2, dd * (one if gd is None else gd))


# ------------------------------------------------------------------------------------------------ scale_col_blocks
@pytest.mark.parametrize("c", D.SCALE_BLOCK_CASES, ids=[f"M{c[0]}-N{c[1]}-split{c[2]}-pitch{c[3]}" for c in D.SCALE_BLOCK_CASES])
def test_scale_col_blocks_bit_exact(ops, c):
    M, N, split, pitch = c
    src, g0, g1 = D.scale_blocks_inputs(M, N, split, pitch)       # NaN in the padding columns: never read
    want = D.scale_blocks_ref(np.nan_to_num(src), N, split, g0, g1)
    out = _Out((M, pitch), "f32")
    ops.scale_col_blocks(_dev(src)[:, :N], out.t[:, :N], split, _dev(np.array([g0], np.float32)), _dev(np.array([g1], np.float32)))
    got = out.host()
    assert D.same_bits(got, want)
    assert not got[:, N:].any() and not np.signbit(got[:, N:]).any(), "padding columns must be exactly 0"
    _close("scale_col_blocks", "f32", got, D.scale_blocks_ref(np.nan_to_num(src), N, split, g0, g1, np.float64), "scale_col_blocks", False)

"""GPU: sw_im2col3x3 / sw_col2im3x3 (csrc/conv_col.hip) bit for bit against tests/conv_col_ref.py: f32 and bf16, both strides, one
pixel, odd maps, channel counts that are no multiple of 64, more than one block, a row pitch of 9 C and of 9 C + 8; NaN (with a
payload), +-inf and -0 through im2col; the ReLU mask off and on in col2im, two runs bit-identical.  Every output sits inside a
sentinel-filled buffer: the guard in front, behind, and the pad columns of every row must still hold the sentinel, and no element the
contract says is written may.  The refusals return their codes without a launch."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_col_ref as R  # noqa: E402

CASES = [(1, 1, 1, 8, 1), (1, 1, 1, 8, 2), (1, 2, 3, 8, 2), (3, 5, 4, 24, 2), (1, 8, 8, 64, 2), (2, 9, 13, 136, 2), (2, 7, 7, 16, 1),
         (2, 6, 10, 264, 1)]
GUARD = 64                                     # elements in front of and behind every output (a multiple of 16 bytes: the view stays aligned)
SENT = {"f32": 0x7FA5A5A5, "bf16": 0x7FA5}     # NaNs with a payload no kernel writes
_ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


def _np_bits(dtype):
    return np.uint32 if dtype == "f32" else np.uint16


def _tdtype(dtype):
    return torch.float32 if dtype == "f32" else torch.bfloat16


def _to_dev(bits, dtype):
    """numpy words (uint32 f32 bits / uint16 bf16 bits) -> device tensor of the dtype with those bits"""
    return torch.from_numpy(bits.view(np.int32 if dtype == "f32" else np.int16).copy()).cuda().view(_tdtype(dtype))


def _bits_of(t, dtype):
    torch.cuda.synchronize()
    return t.contiguous().view(torch.int32 if dtype == "f32" else torch.int16).cpu().numpy().view(_np_bits(dtype))


def _guarded(rows, ld, dtype):
    """-> (flat sentinel buffer, its (rows, ld) view behind GUARD elements)"""
    n = GUARD + rows * ld + GUARD
    buf = torch.from_numpy(np.full(n, SENT[dtype], _np_bits(dtype)).view(np.int32 if dtype == "f32" else np.int16)).cuda().view(_tdtype(dtype))
    return buf, buf[GUARD:GUARD + rows * ld].view(rows, ld)


def _values(shape, dtype, seed):
    """random words of the dtype (normal values, as float32 numbers and as bits)"""
    v = np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
    if dtype == "bf16":
        bits = R.round_bf16(v)
        return R.bf16_to_f32(bits).reshape(shape), bits.reshape(shape)
    return v, v.view(np.uint32).reshape(shape)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_im2col_bits(ops, case, dtype, pad):
    n, H, W, C, s = case
    _, bits = _values((n, H, W, C), dtype, 11)
    special = [0x7FC12345, 0x7F800000, 0xFF800000, 0x80000000] if dtype == "f32" else [0x7FC1, 0x7F80, 0xFF80, 0x8000]
    flat = bits.reshape(-1)
    flat[:4] = special                                                               # (C >= 8: the first pixel holds all four,
    flat[-4:] = special                                                              # and the last one)
    x = _to_dev(bits, dtype)
    Ho, Wo = R.out_hw(H, W, s)
    rows, ld = n * Ho * Wo, 9 * C + pad
    buf, col = _guarded(rows, ld, dtype)
    ops.im2col3x3(x, col[:, :9 * C] if pad else col, s)
    want = np.full(GUARD + rows * ld + GUARD, SENT[dtype], _np_bits(dtype))
    want[GUARD:GUARD + rows * ld].reshape(rows, ld)[:, :9 * C] = R.im2col3x3(bits, s)
    got = _bits_of(buf, dtype)
    assert np.array_equal(got, want), f"{int((got != want).sum())} words differ (first at {int(np.argmax(got != want))})"
    assert set(special) <= set(got.tolist())                                         # the special values arrived as they were


@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_col2im_bits(ops, case, dtype, pad, mask):
    n, H, W, C, s = case
    Ho, Wo = R.out_hw(H, W, s)
    rows, ld = n * Ho * Wo, 9 * C + pad
    dv, dbits = _values((rows, ld), dtype, 12)
    dcol = _to_dev(dbits, dtype)
    ref_v = ref_t = None
    if mask:
        ref_v, rbits = _values((n, H, W, C), dtype, 13)
        ref_v = ref_v.copy(); rbits = rbits.copy()
        ref_v.reshape(-1)[::5] = 0.0; rbits.reshape(-1)[::5] = 0                     # exact zeros: masked (ref <= 0)
        rbits.reshape(-1)[3::11] = 0x80000000 if dtype == "f32" else 0x8000           # -0 likewise
        ref_v.reshape(-1)[3::11] = -0.0
        ref_t = _to_dev(rbits, dtype)
    want_v = R.col2im3x3(dv, n, H, W, C, s, relu_ref=ref_v)
    want = want_v.view(np.uint32) if dtype == "f32" else R.round_bf16(want_v)
    outs = []
    for _ in range(2):
        buf, dx = _guarded(n * H * W, C, dtype)
        ops.col2im3x3(dcol[:, :9 * C] if pad else dcol, dx.view(n, H, W, C), s, relu_ref=ref_t)
        outs.append(_bits_of(buf, dtype))
    full = np.full(GUARD + n * H * W * C + GUARD, SENT[dtype], _np_bits(dtype))
    full[GUARD:GUARD + n * H * W * C] = want.reshape(-1)
    assert np.array_equal(outs[0], full), f"{int((outs[0] != full).sum())} words differ (first at {int(np.argmax(outs[0] != full))})"
    assert np.array_equal(outs[0], outs[1])


def test_refusals_return_their_codes(ops):
    from sos_wsod_amd._lib import lib
    x = torch.zeros(1, 4, 4, 16, device="cuda")
    col = torch.zeros(16, 152, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731

    def im(dtype=0, n=1, H=4, W=4, C=16, s=1, ld=144, a=p(x), b=p(col)):
        return lib.sw_im2col3x3(dtype, n, H, W, C, s, a, b, ld, None)

    def co(dtype=0, n=1, H=4, W=4, C=16, s=1, ld=144, a=p(col), r=None, b=p(x)):
        return lib.sw_col2im3x3(dtype, n, H, W, C, s, a, ld, r, b, None)
    for f in (im, co):
        assert f(dtype=7) == -1
        assert f(s=3) == -3 and f(s=0) == -3
        assert f(C=12) == -5 and f(C=0) == -5
        assert f(ld=136) == -5 and f(ld=148) == -5                                   # below 9 C; no multiple of 8
        assert f(H=0) == -5
        assert f(a=p(col, 4)) == -4 and f(b=p(x, 8)) == -4
        assert f(n=1, H=2048, W=2048, C=64, ld=576) == -6                            # 2^22 rows x 576 columns: 2^31 elements and more
        assert f(n=0) == 0
    assert co(r=p(x, 4)) == -4
    torch.cuda.synchronize()
    assert float(col.abs().sum()) == 0.0 and float(x.abs().sum()) == 0.0             # nothing was launched

"""CPU: tests/conv_col_ref.py (the restatements the GPU tests hold sw_im2col3x3 / sw_col2im3x3 to) against F.unfold and its adjoint
F.fold on small-integer data, where every float32 sum is exact in any order: exact equality.  The case table is the one of
tests/test_gpu_conv_col_kernels.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_col_ref as R

CASES = [(1, 1, 1, 8, 1), (1, 1, 1, 8, 2), (1, 2, 3, 8, 2), (3, 5, 4, 24, 2), (1, 8, 8, 64, 2), (2, 9, 13, 136, 2), (2, 7, 7, 16, 1),
         (2, 6, 10, 264, 1)]


def _ints(shape, seed):
    return np.random.RandomState(seed).randint(-8, 9, size=shape).astype(np.float32)


def _tap_major(cols_nchw9, n, C):
    """F.unfold's (n, C * 9, L) with rows c * 9 + tap -> (n * L, 9 * C) with columns tap * C + c"""
    L = cols_nchw9.shape[2]
    return cols_nchw9.reshape(n, C, 9, L).permute(0, 3, 2, 1).reshape(n * L, 9 * C)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_im2col_restatement_is_unfold(case):
    n, H, W, C, s = case
    x = _ints((n, H, W, C), 1)
    want = _tap_major(F.unfold(torch.from_numpy(x).permute(0, 3, 1, 2), 3, padding=1, stride=s), n, C).numpy()
    got = R.im2col3x3(x, s)
    Ho, Wo = R.out_hw(H, W, s)
    assert got.shape == (n * Ho * Wo, 9 * C) == want.shape
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_col2im_restatement_is_fold(case):
    n, H, W, C, s = case
    Ho, Wo = R.out_hw(H, W, s)
    d = _ints((n * Ho * Wo, 9 * C + 8), 2)                                           # 8 columns of padding: ignored
    cols = torch.from_numpy(d[:, :9 * C].copy()).reshape(n, Ho * Wo, 9, C).permute(0, 3, 2, 1).reshape(n, C * 9, Ho * Wo)
    want = F.fold(cols, (H, W), 3, padding=1, stride=s).permute(0, 2, 3, 1).numpy()
    got = R.col2im3x3(d, n, H, W, C, s)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    ref = _ints((n, H, W, C), 3)
    ref[0, 0, 0, 0] = np.nan                                                         # not > 0: masked, like sw_relu_bwd
    masked = R.col2im3x3(d, n, H, W, C, s, relu_ref=ref)
    assert np.array_equal(masked, np.where(ref > 0, want, 0.0).astype(np.float32))


def test_the_adjoint_pair_is_adjoint():
    """<im2col(x), d> == <x, col2im(d)> exactly on integers, both strides"""
    for n, H, W, C, s in CASES:
        x = _ints((n, H, W, C), 4)
        Ho, Wo = R.out_hw(H, W, s)
        d = _ints((n * Ho * Wo, 9 * C), 5)
        assert float((R.im2col3x3(x, s).astype(np.float64) * d).sum()) == float((x.astype(np.float64) * R.col2im3x3(d, n, H, W, C, s)).sum())


def test_bits_pass_through_and_bf16_rounding():
    x = np.zeros((1, 2, 2, 8), np.uint16)
    x[0, 0, 0, :4] = [0x7FC1, 0x7F80, 0xFF80, 0x8000]                                # NaN with a payload, +inf, -inf, -0 as bf16 words
    col = R.im2col3x3(x, 1)
    assert col.dtype == np.uint16 and sorted(set(col.reshape(-1).tolist())) == [0, 0x7F80, 0x7FC1, 0x8000, 0xFF80]
    v = np.array([1.0, 1.00390625, 1.01171875, -3.0e-3, 65504.0], np.float32)        # 1 + 2^-8: a tie -> even; 1 + 3 * 2^-8: a tie -> up
    assert np.array_equal(R.round_bf16(v), torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.bf16_to_f32(R.round_bf16(v))[:3], np.array([1.0, 1.0, 1.015625], np.float32))

"""NumPy restatements of csrc/conv_col.hip (sw_im2col3x3 / sw_col2im3x3): the column matrix of a 3x3 convolution with padding 1 and
stride 1 or 2 on NHWC maps, columns in [tap][c] order, and its adjoint in the kernel's gather form (f32 sums in ascending tap order,
ReLU mask of the layer's input, one rounding).  tests/test_conv_col_ref_cpu.py pins both against F.unfold / F.fold."""
import numpy as np


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _tap_ranges(H, W, stride, ky, kx):
    """the output pixels whose tap (ky, kx) lies inside the map: (oy list, ox list, iy list, ix list)"""
    Ho, Wo = out_hw(H, W, stride)
    oy = np.array([o for o in range(Ho) if 0 <= stride * o + ky - 1 < H], dtype=np.int64)
    ox = np.array([o for o in range(Wo) if 0 <= stride * o + kx - 1 < W], dtype=np.int64)
    return oy, ox, stride * oy + ky - 1, stride * ox + kx - 1


def im2col3x3(x, stride):
    """x (n, H, W, C), any dtype (bf16 as uint16 words: values are copied as bits) -> (n * Ho * Wo, 9 C)"""
    n, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, stride)
    col = np.zeros((n, Ho, Wo, 9, C), dtype=x.dtype)
    for tap in range(9):
        oy, ox, iy, ix = _tap_ranges(H, W, stride, tap // 3, tap % 3)
        if len(oy) and len(ox):
            col[:, oy[:, None], ox[None, :], tap] = x[:, iy[:, None], ix[None, :]]
    return col.reshape(n * Ho * Wo, 9 * C)


def col2im3x3(dcol, n, H, W, C, stride, relu_ref=None):
    """dcol (n * Ho * Wo, >= 9 C) float32 values (columns beyond 9 C ignored) -> dx (n, H, W, C) float32, NOT yet rounded to the
    storage dtype (round_bf16 for bf16).  relu_ref (n, H, W, C) float32 values or None: dx = 0 where relu_ref is not > 0."""
    Ho, Wo = out_hw(H, W, stride)
    d = np.ascontiguousarray(dcol[:, :9 * C], dtype=np.float32).reshape(n, Ho, Wo, 9, C)
    acc = np.zeros((n, H, W, C), dtype=np.float32)
    for tap in range(9):                                            # every input pixel receives at most one cell per tap
        oy, ox, iy, ix = _tap_ranges(H, W, stride, tap // 3, tap % 3)
        if len(oy) and len(ox):
            acc[:, iy[:, None], ix[None, :]] = acc[:, iy[:, None], ix[None, :]] + d[:, oy[:, None], ox[None, :], tap]
    if relu_ref is not None:
        acc = np.where(np.asarray(relu_ref, dtype=np.float32) > 0, acc, np.float32(0.0)).astype(np.float32)
    return acc


def bf16_to_f32(bits_u16):
    return (np.asarray(bits_u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x_f32):
    """float32 -> bf16 words, round to nearest even (finite values)"""
    b = np.ascontiguousarray(x_f32, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> 16) & np.uint32(1))) >> 16).astype(np.uint16)

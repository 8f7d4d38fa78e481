// 3x3 convolutions (padding 1, stride 1 or 2) as a GEMM over an explicit column matrix: the two data-movement kernels around
// sw_gemm.  Used where the direct / implicit-GEMM kernels (stride 1 on whole maps) do not apply: the stride-2 conv2 of a
// torchvision-style bottleneck (detectron2/modeling/backbone/resnet.py, the `stride_in_1x1 = False` branch) and the 3x3
// convolutions of FastRCNNConvFCHead on (R, 7, 7, C) ROI maps (detectron2/modeling/roi_heads/box_head.py).
//   col[(n * Ho + oy) * Wo + ox][(3 * ky + kx) * C + c] = in[n][stride * oy + ky - 1][stride * ox + kx - 1][c]   (0 outside)
// which is the [tap][ci] order of the staged [co][tap][ci] weight: that tensor is the (Cout, 9 C) B operand of sw_gemm as it is.
// Both kernels move 16-byte pieces (8 channels per lane), index in 64 bits and write every element they own exactly once.
#include "common.h"
#include "soswsod_hip.h"

namespace {

inline int col_grid_for(long n) {
  long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 1048576 ? 1048576 : g));
}

// V = 16-byte pieces per 8 channels: 1 (bf16) or 2 (f32).  One lane: 8 channels of one (output pixel, tap) cell.
template <int V>
__global__ void im2col3x3_kernel(long total, int H, int W, int C8, int Ho, int Wo, int stride, const u32x4* __restrict__ in,
                                 u32x4* __restrict__ col, long ldv) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % C8);
    long r = i / C8;
    const int tap = (int)(r % 9);
    r /= 9;                                                        // output pixel (n * Ho + oy) * Wo + ox
    const int ox = (int)(r % Wo);
    const long t = r / Wo;
    const int oy = (int)(t % Ho);
    const long n = t / Ho;
    const int iy = stride * oy + tap / 3 - 1, ix = stride * ox + tap % 3 - 1;
    const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
    u32x4* dst = col + r * ldv + ((long)tap * C8 + c8) * V;
    if (inside) {
      const u32x4* src = in + (((n * H + iy) * W + ix) * C8 + c8) * V;
#pragma unroll
      for (int v = 0; v < V; ++v) dst[v] = src[v];
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) dst[v] = u32x4{0u, 0u, 0u, 0u};
    }
  }
}

template <int V>
__device__ __forceinline__ void add8(float* acc, const u32x4* p) {
  if (V == 1) {
    const u32x4 q = p[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[2 * k] += __uint_as_float(q[k] << 16);
      acc[2 * k + 1] += __uint_as_float(q[k] & 0xFFFF0000u);
    }
  } else {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const u32x4 q = p[v];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[4 * v + k] += __uint_as_float(q[k]);
    }
  }
}

// the adjoint, gathered: one lane owns 8 channels of one INPUT pixel and adds, in ascending tap order in f32, the cells of dcol
// that im2col filled from it (stride 1: at most 9, stride 2: at most 4); ReLU mask of the layer's input, one rounding, one store
template <int V>
__global__ void col2im3x3_kernel(long total, int H, int W, int C8, int Ho, int Wo, int stride, const u32x4* __restrict__ dcol,
                                 long ldv, const u32x4* __restrict__ relu_ref, u32x4* __restrict__ dx) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % C8);
    long r = i / C8;                                               // input pixel (n * H + iy) * W + ix
    const int ix = (int)(r % W);
    const long t = r / W;
    const int iy = (int)(t % H);
    const long n = t / H;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ny = iy + 1 - tap / 3, nx = ix + 1 - tap % 3;      // = stride * (oy, ox)
      if (ny < 0 || nx < 0 || (stride == 2 && ((ny | nx) & 1))) continue;
      const int oy = ny / stride, ox = nx / stride;
      if (oy >= Ho || ox >= Wo) continue;
      add8<V>(acc, dcol + ((n * Ho + oy) * Wo + ox) * ldv + ((long)tap * C8 + c8) * V);
    }
    if (relu_ref != nullptr) {
      const u32x4* rp = relu_ref + i * V;
      if (V == 1) {
        const u32x4 q = rp[0];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(__uint_as_float(q[k] << 16) > 0.f)) acc[2 * k] = 0.f;
          if (!(__uint_as_float(q[k] & 0xFFFF0000u) > 0.f)) acc[2 * k + 1] = 0.f;
        }
      } else {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const u32x4 q = rp[v];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (!(__uint_as_float(q[k]) > 0.f)) acc[4 * v + k] = 0.f;
        }
      }
    }
    u32x4* dst = dx + i * V;
    if (V == 1) {
      u32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = (unsigned)f32_to_bf16_bits(acc[2 * k]) | ((unsigned)f32_to_bf16_bits(acc[2 * k + 1]) << 16);
      dst[0] = o;
    } else {
#pragma unroll
      for (int v = 0; v < 2; ++v)
        dst[v] = u32x4{__float_as_uint(acc[4 * v]), __float_as_uint(acc[4 * v + 1]), __float_as_uint(acc[4 * v + 2]),
                       __float_as_uint(acc[4 * v + 3])};
    }
  }
}

// 0: run, 1: nothing to do, < 0: refused.  rows = output pixels
int col_args(int dtype, int nimg, int H, int W, int C, int stride, long ldcol, long* rows, int* Ho, int* Wo) {
  if (dtype != SW_F32 && dtype != SW_BF16) return -1;
  if (stride != 1 && stride != 2) return -3;
  if (nimg < 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8) != 0 || ldcol < 9L * C || (ldcol % 8) != 0) return -5;
  *Ho = (H - 1) / stride + 1;
  *Wo = (W - 1) / stride + 1;
  *rows = (long)nimg * *Ho * *Wo;
  if (ldcol >= 2147483648L || *rows >= 2147483648L || *rows * ldcol >= 2147483648L) return -6;
  return nimg == 0 ? 1 : 0;
}

}  // namespace

extern "C" int sw_im2col3x3(int dtype, int nimg, int H, int W, int C, int stride, const void* in, void* col, long ldcol,
                            hipStream_t stream) {
  SW_ENTER();
  long rows;
  int Ho, Wo;
  const int rc = col_args(dtype, nimg, H, W, C, stride, ldcol, &rows, &Ho, &Wo);
  if (rc) return rc < 0 ? rc : 0;
  if (in == nullptr || col == nullptr || (((uintptr_t)in | (uintptr_t)col) & 15)) return -4;
  const int C8 = C / 8;
  const long total = rows * 9 * C8;
  if (dtype == SW_BF16)
    hipLaunchKernelGGL(im2col3x3_kernel<1>, dim3(col_grid_for(total)), dim3(256), 0, stream, total, H, W, C8, Ho, Wo, stride,
                       (const u32x4*)in, (u32x4*)col, ldcol / 8);
  else
    hipLaunchKernelGGL(im2col3x3_kernel<2>, dim3(col_grid_for(total)), dim3(256), 0, stream, total, H, W, C8, Ho, Wo, stride,
                       (const u32x4*)in, (u32x4*)col, ldcol / 4);
  SW_CHECK_LAUNCH();
  return 0;
}

extern "C" int sw_col2im3x3(int dtype, int nimg, int H, int W, int C, int stride, const void* dcol, long ldcol,
                            const void* relu_ref, void* dx, hipStream_t stream) {
  SW_ENTER();
  long rows;
  int Ho, Wo;
  const int rc = col_args(dtype, nimg, H, W, C, stride, ldcol, &rows, &Ho, &Wo);
  if (rc) return rc < 0 ? rc : 0;
  if (dcol == nullptr || dx == nullptr || (((uintptr_t)dcol | (uintptr_t)dx | (uintptr_t)relu_ref) & 15)) return -4;
  const int C8 = C / 8;
  const long total = (long)nimg * H * W * C8;
  if (dtype == SW_BF16)
    hipLaunchKernelGGL(col2im3x3_kernel<1>, dim3(col_grid_for(total)), dim3(256), 0, stream, total, H, W, C8, Ho, Wo, stride,
                       (const u32x4*)dcol, ldcol / 8, (const u32x4*)relu_ref, (u32x4*)dx);
  else
    hipLaunchKernelGGL(col2im3x3_kernel<2>, dim3(col_grid_for(total)), dim3(256), 0, stream, total, H, W, C8, Ho, Wo, stride,
                       (const u32x4*)dcol, ldcol / 4, (const u32x4*)relu_ref, (u32x4*)dx);
  SW_CHECK_LAUNCH();
  return 0;
}

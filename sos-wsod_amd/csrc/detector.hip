// Kernels of the Stage-3 detector (the ResNet-50-FPN Faster R-CNN of the Unbiased-Teacher step) that the
// Stage-1 path did not need.  Dense work stays on the MFMA kernels of gemm.hip / conv_direct.hip (1x1 convolutions = sw_gemm on
// NHWC pixels, 3x3 = sw_conv3x3_igemm, fc = sw_gemm); here: the frozen stem (7x7 stride-2 convolution with the FrozenBN affine +
// ReLU, 3x3 stride-2 max pooling), the stride-2 pixel subsampling in front of a 1x1 stride-2 convolution and its scatter
// backward, residual add + ReLU, FPN's nearest 2x upsample + add and its backward, ROIAlign (aligned, adaptive sampling grid)
// forward / backward over FPN levels, anchor-delta decoding, and the RPN's objectness / localisation losses with their unit
// gradients.  All NHWC, wave64, HBM-bound elementwise / gather work: coalesced channel-contiguous accesses, no MFMA.
#include <float.h>
#include <math.h>
#include "common.h"
#include "soswsod_hip.h"

namespace {

constexpr long GRID_CAP = 1048576;                             // these kernels' grid-stride loops start up to 2^20 workgroups

// ------------------------------------------------------------------------------------------- input: normalise + pad
// img u8 [3][h][w] -> out [H][W][4] = (img - mean) / std inside the image, 0 in the padding and in channel 3
// (detectron2/modeling/meta_arch/rcnn.py:220-228 + structures/image_list.py:60-124)
template <typename T>
__global__ void preprocess_pad_kernel(int h, int w, int H, int W, const uint8_t* __restrict__ img, float m0, float m1, float m2,
                                      float s0, float s1, float s2, T* __restrict__ out) {
  const long n = (long)H * W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (y < h && x < w) {
      const long p = (long)y * w + x, hw = (long)h * w;
      v0 = ((float)img[p] - m0) / s0; v1 = ((float)img[hw + p] - m1) / s1; v2 = ((float)img[2 * hw + p] - m2) / s2;
    }
    T* o = out + i * 4;
    Elem<T>::store(o, v0); Elem<T>::store(o + 1, v1); Elem<T>::store(o + 2, v2); Elem<T>::store(o + 3, 0.f);
  }
}

// ------------------------------------------------------------------------------------------- stem: conv 7x7 s2 p3 + affine + ReLU
// in [N][H][W][4], w f32 [64][3][7][7] (OIHW), scale / bias f32 [64] (the FrozenBN fold), out [N][OH][OW][64], OH = (H + 6 - 7) / 2 + 1.
// Workgroup = an 8x8 tile of output pixels x 64 channels; thread = (pixel, 16-channel group): the 21x21x3 input patch and the
// 147x64 weights sit in LDS, the weight reads of a wave are broadcasts.  Frozen layer (FREEZE_AT 2): forward only.
template <typename T>
__global__ __launch_bounds__(256) void stem_conv7_kernel(int N, int H, int W, int OH, int OW, const T* __restrict__ in,
                                                         const float* __restrict__ w, const float* __restrict__ scale,
                                                         const float* __restrict__ bias, T* __restrict__ out) {
  __shared__ float s_w[147 * 64];
  __shared__ float s_in[21 * 21 * 3];
  const int tiles_x = (OW + 7) / 8, tiles_y = (OH + 7) / 8;
  const int t = blockIdx.x;
  const int n = t / (tiles_x * tiles_y), ty = (t / tiles_x) % tiles_y, tx = t % tiles_x;
  for (int i = threadIdx.x; i < 147 * 64; i += 256) {
    const int k = i >> 6, co = i & 63;                       // k = (ci * 7 + ky) * 7 + kx
    s_w[i] = w[co * 147 + k];
  }
  const int iy0 = ty * 16 - 3, ix0 = tx * 16 - 3;
  for (int i = threadIdx.x; i < 21 * 21; i += 256) {
    const int py = i / 21, px = i - py * 21, y = iy0 + py, x = ix0 + px;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const T* p = in + (((long)n * H + y) * W + x) * 4;
      v0 = Elem<T>::load(p); v1 = Elem<T>::load(p + 1); v2 = Elem<T>::load(p + 2);
    }
    s_in[i * 3] = v0; s_in[i * 3 + 1] = v1; s_in[i * 3 + 2] = v2;
  }
  __syncthreads();
  const int p = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int oy = p >> 3, ox = p & 7;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
  for (int ci = 0; ci < 3; ++ci)
    for (int ky = 0; ky < 7; ++ky)
      for (int kx = 0; kx < 7; ++kx) {
        const float v = s_in[((oy * 2 + ky) * 21 + ox * 2 + kx) * 3 + ci];
        const float* wr = s_w + ((ci * 7 + ky) * 7 + kx) * 64 + g * 16;
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = fmaf(v, wr[c], acc[c]);
      }
  const int Y = ty * 8 + oy, X = tx * 8 + ox;
  if (Y < OH && X < OW) {
    T* o = out + (((long)n * OH + Y) * OW + X) * 64 + g * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c) Elem<T>::store(o + c, relu_keep_nan(fmaf(acc[c], scale[g * 16 + c], bias[g * 16 + c])));
  }
}

// The pooling / FPN kernels below are templates over <T, V>: a thread carries V channels of a pixel, V = 1 with scalar accesses (any
// C, any alignment) or V = 16 / sizeof(T) with 16-byte pieces (C a multiple of V, 16-byte aligned tensors: vec16_ok).
// 3x3 max pooling, stride 2, padding 1 (resnet.py:358): out [N][OH][OW][C], OH = (H + 2 - 3) / 2 + 1
template <typename T, int V>
__global__ void maxpool3x3s2_kernel(int N, int H, int W, int C, int OH, int OW, const T* __restrict__ in, T* __restrict__ out) {
  const int cp = C / V;
  const long n = (long)N * OH * OW * cp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const Nhwc o = nhwc_split(i, OH, OW, cp);
    float m[V];
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
      const int y = o.y * 2 - 1 + ky;
      if (y < 0 || y >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int x = o.x * 2 - 1 + kx;
        if (x < 0 || x >= W) continue;
        float v[V];
        elems_load<T, V>(in + (((long)o.b * H + y) * W + x) * C + o.c * V, v);
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = max_keep_nan(m[k], v[k]);
      }
    }
    elems_store<T, V>(out + i * V, m);                   // (i * V: the flat index of channel o.c * V of this pixel, C = cp * V)
  }
}

// ------------------------------------------------------------------------------------------- stride-2 subsample / scatter
// (T = u32x4 with C counted in pieces: the 16-byte form of these two copies)
// out[n][y][x][:] = in[n][2y][2x][:]  (the pixels a 1x1 stride-2 convolution reads; also FPN's p6 = max_pool(k 1, s 2) of p5)
template <typename T>
__global__ void subsample2_kernel(int N, int H, int W, int C, int OH, int OW, const T* __restrict__ in, T* __restrict__ out) {
  const long n = (long)N * OH * OW * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const Nhwc o = nhwc_split(i, OH, OW, C);
    out[i] = in[(((long)o.b * H + o.y * 2) * W + o.x * 2) * C + o.c];
  }
}
// backward: out [N][H][W][C] = g at the even pixels, 0 elsewhere (fully written)
template <typename T>
__global__ void scatter2_kernel(int N, int H, int W, int C, int OH, int OW, const T* __restrict__ g, T* __restrict__ out) {
  const long n = (long)N * H * W * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const Nhwc p = nhwc_split(i, H, W, C);
    T v = {};
    if (!(p.y & 1) && !(p.x & 1)) v = g[(((long)p.b * OH + (p.y >> 1)) * OW + (p.x >> 1)) * C + p.c];
    out[i] = v;
  }
}

// ------------------------------------------------------------------------------------------- residual add + ReLU, FPN top-down
template <typename T>
__global__ void add_relu_kernel(long n, const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, int relu) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = Elem<T>::load(a + i) + Elem<T>::load(b + i);
    if (relu) v = relu_keep_nan(v);
    Elem<T>::store(out + i, v);
  }
}
// out [N][2h][2w][C] = lateral + nearest-neighbour 2x upsampling of top [N][h][w][C]  (fpn.py:142-144)
template <typename T, int V>
__global__ void upsample2_add_kernel(int N, int h, int w, int C, const T* __restrict__ lateral, const T* __restrict__ top,
                                     T* __restrict__ out) {
  const int cp = C / V;
  const long n = (long)N * 2 * h * 2 * w * cp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const Nhwc p = nhwc_split(i, 2 * h, 2 * w, cp);
    float a[V], t[V];
    elems_load<T, V>(lateral + i * V, a);
    elems_load<T, V>(top + (((long)p.b * h + (p.y >> 1)) * w + (p.x >> 1)) * C + p.c * V, t);
#pragma unroll
    for (int k = 0; k < V; ++k) a[k] += t[k];
    elems_store<T, V>(out + i * V, a);
  }
}
// backward of the upsampling: out [N][h][w][C] = sum of the 2x2 block of g [N][2h][2w][C], (a + b) + (c + d) per element in f32
template <typename T, int V>
__global__ void downsample2_sum_kernel(int N, int h, int w, int C, const T* __restrict__ g, T* __restrict__ out) {
  const int cp = C / V;
  const long n = (long)N * h * w * cp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const Nhwc o = nhwc_split(i, h, w, cp);
    const T* p = g + (((long)o.b * 2 * h + 2 * o.y) * 2 * w + 2 * o.x) * C + o.c * V;
    float q0[V], q1[V], q2[V], q3[V];
    elems_load<T, V>(p, q0); elems_load<T, V>(p + C, q1);
    elems_load<T, V>(p + (long)2 * w * C, q2); elems_load<T, V>(p + (long)2 * w * C + C, q3);
#pragma unroll
    for (int k = 0; k < V; ++k) q0[k] = (q0[k] + q1[k]) + (q2[k] + q3[k]);
    elems_store<T, V>(out + i * V, q0);
  }
}

// ------------------------------------------------------------------------------------------- ROIAlign (aligned = true)
// The arithmetic of uwsod/detectron2/layers/csrc/ROIAlign/ROIAlign_cpu.cpp:20-218 (= torchvision.ops.roi_align, which
// detectron2/layers/roi_align.py:56-64 calls): offset 0.5, ROI size not clamped, sampling grid ceil(roi / pooled) when
// sampling_ratio == 0, samples outside [-1, size] contribute 0, average over the grid.  Compiled with -ffp-contract=off.
struct AlignGeom { float start_h, start_w, bin_h, bin_w, count; int grid_h, grid_w, batch; };
__device__ __forceinline__ AlignGeom align_geom(const float* roi, float scale, int PH, int PW, int sampling_ratio) {
  AlignGeom g;
  g.batch = (int)roi[0];
  g.start_w = __fsub_rn(__fmul_rn(roi[1], scale), 0.5f);
  g.start_h = __fsub_rn(__fmul_rn(roi[2], scale), 0.5f);
  const float end_w = __fsub_rn(__fmul_rn(roi[3], scale), 0.5f), end_h = __fsub_rn(__fmul_rn(roi[4], scale), 0.5f);
  const float rw = __fsub_rn(end_w, g.start_w), rh = __fsub_rn(end_h, g.start_h);
  g.bin_h = __fdiv_rn(rh, (float)PH);
  g.bin_w = __fdiv_rn(rw, (float)PW);
  g.grid_h = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(__fdiv_rn(rh, (float)PH));
  g.grid_w = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(__fdiv_rn(rw, (float)PW));
  const int c = g.grid_h * g.grid_w;
  g.count = (float)(c > 1 ? c : 1);
  return g;
}
__device__ __forceinline__ bool align_corners(int H, int W, float y, float x, int* yl, int* xl, int* yh, int* xh, float* wgt) {
  if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return false;
  if (y <= 0) y = 0;
  if (x <= 0) x = 0;
  int y_low = (int)y, x_low = (int)x, y_high, x_high;
  if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else y_high = y_low + 1;
  if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else x_high = x_low + 1;
  const float ly = __fsub_rn(y, (float)y_low), lx = __fsub_rn(x, (float)x_low);
  const float hy = __fsub_rn(1.0f, ly), hx = __fsub_rn(1.0f, lx);
  wgt[0] = __fmul_rn(hy, hx); wgt[1] = __fmul_rn(hy, lx); wgt[2] = __fmul_rn(ly, hx); wgt[3] = __fmul_rn(ly, lx);
  *yl = y_low; *xl = x_low; *yh = y_high; *xh = x_high;
  return true;
}
__device__ __forceinline__ float align_coord(float start, int p, float bin, int i, int grid) {
  // start + p * bin + (i + .5f) * bin / grid, left to right as the reference writes it
  return __fadd_rn(__fadd_rn(start, __fmul_rn((float)p, bin)), __fdiv_rn(__fmul_rn((float)i + .5f, bin), (float)grid));
}

// thread = (listed ROI, bin, channel): consecutive threads = consecutive channels -> coalesced NHWC reads.  Only the ROIs listed in
// `sel` (n_sel row indices into rois / out) are computed: the FPN pooler calls once per level with that level's ROIs.
// `o` = where the bin's element sits in out / gout [R][C][PH][PW] (the reference's flatten order: fc1.weight needs no permutation),
// row pitch ld.
struct AlignBin { int ph, pw, c; long o; AlignGeom g; };
__device__ __forceinline__ long align_bins(int n_sel, const int* n_sel_dev, int PH, int PW, int C) {
  return (long)(n_sel_dev ? min(n_sel_dev[0], n_sel) : n_sel) * PH * PW * C;     // device count: no host round trip for the level lists
}
__device__ __forceinline__ AlignBin align_bin(long i, int C, int PH, int PW, float scale, int sampling_ratio, const float* rois,
                                              const int* sel, long ld) {
  const Nhwc p = nhwc_split(i, PH, PW, C);                   // (listed ROI, ph, pw, c)
  const int row = sel[p.b];
  return {p.y, p.x, p.c, (long)row * ld + ((long)p.c * PH + p.y) * PW + p.x, align_geom(rois + (long)row * 5, scale, PH, PW, sampling_ratio)};
}
template <typename T>
__global__ void roi_align_fwd_kernel(int H, int W, int C, int PH, int PW, float scale, int sampling_ratio,
                                     const T* __restrict__ feat, const float* __restrict__ rois, const int* __restrict__ sel,
                                     int n_sel, const int* __restrict__ n_sel_dev, T* __restrict__ out, long ld) {
  const long n = align_bins(n_sel, n_sel_dev, PH, PW, C);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const AlignBin b = align_bin(i, C, PH, PW, scale, sampling_ratio, rois, sel, ld);
    const AlignGeom& g = b.g;
    const T* f = feat + (long)g.batch * H * W * C + b.c;
    float v = 0.f;
    for (int iy = 0; iy < g.grid_h; ++iy) {
      const float y = align_coord(g.start_h, b.ph, g.bin_h, iy, g.grid_h);
      for (int ix = 0; ix < g.grid_w; ++ix) {
        const float x = align_coord(g.start_w, b.pw, g.bin_w, ix, g.grid_w);
        int yl, xl, yh, xh; float wg[4];
        if (!align_corners(H, W, y, x, &yl, &xl, &yh, &xh, wg)) continue;
        // ((w1 v1 + w2 v2) + w3 v3) + w4 v4 added to the running sum, as ROIAlign_cpu.cpp:204-206 evaluates it
        const float t = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(wg[0], Elem<T>::load(f + ((long)yl * W + xl) * C)),
                                                      __fmul_rn(wg[1], Elem<T>::load(f + ((long)yl * W + xh) * C))),
                                            __fmul_rn(wg[2], Elem<T>::load(f + ((long)yh * W + xl) * C))),
                                  __fmul_rn(wg[3], Elem<T>::load(f + ((long)yh * W + xh) * C)));
        v = __fadd_rn(v, t);
      }
    }
    Elem<T>::store(out + b.o, __fdiv_rn(v, g.count));
  }
}
// backward: dfeat f32 [N][H][W][C] (caller zero-fills) += w * g / count by f32 atomics (ROIAlign_cpu.cpp:286-400).
// The bilinear weight of a sample factors into a row part and a column part, and validity / border clamping act per axis, so the
// contributions of a bin's grid_h x grid_w samples to pixel (Y, X) sum to (sum_iy wy_iy(Y)) * (sum_ix wx_ix(X)) * g / count: with the
// per-axis sums in registers a bin issues (rows touched) x (columns touched) <= (grid_h + 1)(grid_w + 1) atomics instead of
// 4 * grid_h * grid_w (grid 4 x 4: 25 for 64).  Sample spacing is bin / ceil(bin) <= 1 pixel, so the touched rows are consecutive.
// Grids above AXIS_MAX - 1 per axis (a ROI far too large for its level) take the sample-by-sample form.
constexpr int AXIS_MAX = 9;
struct AxisW { float w[AXIS_MAX]; int base; };
__device__ __forceinline__ AxisW align_axis_weights(float start, int p, float bin, int grid, int size) {
  AxisW a;
#pragma unroll
  for (int s = 0; s < AXIS_MAX; ++s) a.w[s] = 0.f;
  a.base = -1;
  for (int i = 0; i < grid; ++i) {
    float y = align_coord(start, p, bin, i, grid);
    if (y < -1.0f || y > (float)size) continue;
    if (y <= 0) y = 0;
    int lo = (int)y, hi;
    if (lo >= size - 1) { hi = lo = size - 1; y = (float)lo; } else hi = lo + 1;
    const float l = __fsub_rn(y, (float)lo), h = __fsub_rn(1.0f, l);
    if (a.base < 0) a.base = lo;
    const int k0 = lo - a.base, k1 = hi - a.base;
#pragma unroll
    for (int s = 0; s < AXIS_MAX; ++s) {                     // (static register indices: a dynamic one would put the array in scratch)
      if (s == k0) a.w[s] += h;
      if (s == k1) a.w[s] += l;
    }
  }
  return a;
}
// One kernel for both accumulators: Acc::init(arg) prepares the launch (false: nothing to add), Acc::add(p, v) adds contribution v into *p.
struct AccF32 {                                              // f32 atomics, arrival order: the last bits differ between runs
  typedef float type;
  struct Arg {};
  __device__ __forceinline__ bool init(Arg) { return true; }
  __device__ __forceinline__ void add(float* p, float v) const { atomicAdd(p, v); }
};
// Deterministic backward (round 6).  The f32 atomics above add in arrival order: two runs of one iteration differ in the last bits of
// the feature gradients, the student drifts, pseudo boxes jitter, position-keyed anchor sampling flips (tests had to allow 6e-2 on the
// pseudo RPN losses).  Here the SAME contributions are accumulated as 64-bit fixed-point integers — integer addition commutes, so the sum
// does not depend on the order: contribution v (|v| <= max|gout| = am: a bin hands out exactly its gradient, weights sum to count) is
// added as llrint(v * 2^(40 - e)) with am = f * 2^e, f in [0.5, 1) (frexpf): |v * 2^(40 - e)| < 2^40; a pixel collects at most
// R * PH * PW * 2^40 < 2^63 for R < 170 000 ROIs; resolution 2^-40 of 2^e <= 2 am against f32's 2^-24.  The scale is a power of two
// applied by ldexpf: exact, no intermediate overflows for any finite am > 0 (2^40 / am overflowed below am ~ 3e-27), and a gradient
// scaled by 2^k yields the same integers.  acc [N][H][W][C] int64, zero-filled by the caller; fx_to_float_kernel turns it into the map
// (NaN / Inf in gout: absmax reports it, the whole map comes out NaN — the f32 form poisoned the pixels the ROI touched).
constexpr int FX_BITS = 40;
struct AccFx {
  typedef unsigned long long type;
  typedef const float* Arg;                                  // absmax: max |gout|, one float in device memory
  int sh;                                                    // v * 2^sh, |v| <= am < 2^e
  __device__ __forceinline__ bool init(Arg absmax) {
    const float am = absmax[0];
    if (!(am > 0.f) || !__builtin_isfinite(am)) return false;          // zero gradient: nothing to add; NaN / Inf: the conversion reports it
    int e;
    (void)frexpf(am, &e);
    sh = FX_BITS - e;
    return true;
  }
  __device__ __forceinline__ void add(unsigned long long* p, float v) const { atomicAdd(p, (unsigned long long)__float2ll_rn(ldexpf(v, sh))); }
};
template <typename T, typename Acc>
__global__ void roi_align_bwd_kernel(int H, int W, int C, int PH, int PW, float scale, int sampling_ratio,
                                     const T* __restrict__ gout, long ld, const float* __restrict__ rois,
                                     const int* __restrict__ sel, int n_sel, const int* __restrict__ n_sel_dev,
                                     typename Acc::Arg arg, typename Acc::type* __restrict__ dfeat) {
  Acc acc;
  if (!acc.init(arg)) return;
  const long n = align_bins(n_sel, n_sel_dev, PH, PW, C);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const AlignBin b = align_bin(i, C, PH, PW, scale, sampling_ratio, rois, sel, ld);
    const AlignGeom& g = b.g;
    const float go = Elem<T>::load(gout + b.o);
    typename Acc::type* d = dfeat + (long)g.batch * H * W * C + b.c;
    if (g.grid_h < AXIS_MAX && g.grid_w < AXIS_MAX && g.bin_h <= (float)g.grid_h && g.bin_w <= (float)g.grid_w) {     // (sample spacing <= 1)
      const AxisW ay = align_axis_weights(g.start_h, b.ph, g.bin_h, g.grid_h, H);
      const AxisW ax = align_axis_weights(g.start_w, b.pw, g.bin_w, g.grid_w, W);
      if (ay.base < 0 || ax.base < 0) continue;
      const float gs = __fdiv_rn(go, g.count);
#pragma unroll
      for (int ry = 0; ry < AXIS_MAX; ++ry) {
        if (ay.w[ry] == 0.f) continue;
        const float gy = __fmul_rn(gs, ay.w[ry]);
        typename Acc::type* drow = d + (long)(ay.base + ry) * W * C;
#pragma unroll
        for (int rx = 0; rx < AXIS_MAX; ++rx)
          if (ax.w[rx] != 0.f) acc.add(drow + (long)(ax.base + rx) * C, __fmul_rn(gy, ax.w[rx]));
      }
      continue;
    }
    for (int iy = 0; iy < g.grid_h; ++iy) {
      const float y = align_coord(g.start_h, b.ph, g.bin_h, iy, g.grid_h);
      for (int ix = 0; ix < g.grid_w; ++ix) {
        const float x = align_coord(g.start_w, b.pw, g.bin_w, ix, g.grid_w);
        int yl, xl, yh, xh; float wg[4];
        if (!align_corners(H, W, y, x, &yl, &xl, &yh, &xh, wg)) continue;
        acc.add(d + ((long)yl * W + xl) * C, __fdiv_rn(__fmul_rn(go, wg[0]), g.count));
        acc.add(d + ((long)yl * W + xh) * C, __fdiv_rn(__fmul_rn(go, wg[1]), g.count));
        acc.add(d + ((long)yh * W + xl) * C, __fdiv_rn(__fmul_rn(go, wg[2]), g.count));
        acc.add(d + ((long)yh * W + xh) * C, __fdiv_rn(__fmul_rn(go, wg[3]), g.count));
      }
    }
  }
}
template <typename T>
__global__ void fx_to_float_kernel(long n, const long long* __restrict__ acc, const float* __restrict__ absmax, T* __restrict__ out) {
  const float am = absmax[0];
  const bool bad = !__builtin_isfinite(am);                           // NaN or Inf somewhere in the gradient
  int e = 0;
  if (!bad) (void)frexpf(am, &e);
  const double inv = ldexp(1.0, e - FX_BITS);                         // the exact inverse of AccFx's 2^(40 - e)            
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    Elem<T>::store(out + i, bad ? __uint_as_float(0x7FC00000u) : (float)((double)acc[i] * inv));
}

// ------------------------------------------------------------------------------------------- RPN losses
// RPN losses (detectron2/modeling/proposal_generator/rpn.py:362-420, box_regression.py:229-260): over all N * A anchors,
//   objectness: sum over label >= 0 of BCE-with-logits(x, label);   localisation: sum over label == 1 of |delta - get_deltas(anchor, gt)|
// both x inv_norm (1 / (batch_size_per_image * N)).  One partial pair per workgroup into `partial` (ordered fold by the second
// kernel: deterministic), and the unit gradients dlogit = (sigmoid(x) - y) inv_norm, ddelta = sign(delta - target) inv_norm
// (0 where the anchor does not take part).
__global__ __launch_bounds__(256) void rpn_loss_kernel(long n, long n_anchors, const float* __restrict__ logits,
                                                       const float* __restrict__ deltas, const signed char* __restrict__ labels,
                                                       const float* __restrict__ anchors, const float* __restrict__ gt_boxes,
                                                       float wx, float wy, float ww, float wh, float inv_norm,
                                                       float* __restrict__ partial, float* __restrict__ dlogits,
                                                       float* __restrict__ ddeltas) {
  __shared__ float red[32];
  float s_obj = 0.f, s_loc = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int lab = labels[i];
    const float x = logits[i];
    float dl = 0.f;
    if (lab >= 0) {
      const float y = (float)lab;
      s_obj += bce_with_logits(x, y);
      dl = (1.f / (1.f + expf(-x)) - y) * inv_norm;
    }
    if (dlogits) dlogits[i] = dl;
    float dd[4] = {0.f, 0.f, 0.f, 0.f};
    if (lab == 1) {
      float t[4];
      box_deltas(anchors + (i % n_anchors) * 4, gt_boxes + i * 4, wx, wy, ww, wh, t);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float e = deltas[i * 4 + k] - t[k];
        s_loc += fabsf(e);
        dd[k] = (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) * inv_norm;
      }
    }
    if (ddeltas) { ddeltas[i * 4] = dd[0]; ddeltas[i * 4 + 1] = dd[1]; ddeltas[i * 4 + 2] = dd[2]; ddeltas[i * 4 + 3] = dd[3]; }
  }
  s_obj = block_reduce_sum(s_obj, red);
  __syncthreads();
  s_loc = block_reduce_sum(s_loc, red);
  if (threadIdx.x == 0) { partial[blockIdx.x * 2] = s_obj; partial[blockIdx.x * 2 + 1] = s_loc; }
}
__global__ void rpn_loss_fold_kernel(int nblocks, const float* __restrict__ partial, float inv_norm, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int i = 0; i < nblocks; ++i) { a += partial[2 * i]; b += partial[2 * i + 1]; }
    out[0] = a * inv_norm; out[1] = b * inv_norm;
  }
}
constexpr int RPN_LOSS_BLOCKS = 256;

// ---------------------------------------------------------------- every weight of a detector staged by ONE launch
// entry kinds: 0 linear (rows, cols) f32 -> compute dtype rows of pitch cols; 1 conv3x3 OIHW -> [co][tap][ci]; 2 conv3x3 OIHW ->
// [ci][8 - tap][co] (data-gradient layout); 3 f32 copy (bias pieces of packed heads).  With FrozenBN buffers the folded weight
// w * scale[co] is staged (scale = bn_weight * rsqrt(bn_var + eps), layers/batch_norm.py:52-60; rsqrt spelled 1 / sqrt with the
// _rn intrinsics: within one ulp of the reference's CPU result, tests/test_gpu_stage3.py) and scale / shift are written.
constexpr int STAGE_CHUNK = 4096;
// block geometry per kind (sw_stage_blocks must agree):
//   0 / 3: STAGE_CHUNK consecutive elements, 4 per thread and step (16-byte loads when a row is a multiple of 4 elements);
//   1: one output channel x a range of <= STAGE_CI1 input channels: the [ci][tap] run is read as it lies (contiguous), turned in LDS,
//      and written as 9 runs over ci (the first version gathered 4 bytes every 36: 9x the read transactions);
//   2: 64 output channels x 7 input channels: 63-float runs read per output channel, written as (ci, tap) rows of 64 channels.
constexpr int STAGE_CI1 = 448, STAGE_CO2 = 64, STAGE_CI2 = 7;
__host__ __device__ inline int stage_ci_chunk(int cols) { return cols <= STAGE_CI1 ? cols : 256; }
template <typename T>
__global__ __launch_bounds__(256) void stage_weights_multi_kernel(int n, const sw_stage_desc* __restrict__ descs, float eps) {
  __shared__ float s_t[STAGE_CO2 * (STAGE_CI2 * 9 + 2) > STAGE_CI1 * 9 ? STAGE_CO2 * (STAGE_CI2 * 9 + 2) : STAGE_CI1 * 9];
  int lo = 0, hi = n - 1;                                     // the last entry whose block_start <= blockIdx.x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block_start <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const sw_stage_desc d = descs[lo];
  const int rows = d.rows, cols = d.cols;
  const bool bn = d.bn_weight != nullptr;
  const int blk = (int)blockIdx.x - d.block_start;
  if (bn && blk == 0 && d.scale)
    for (int r = threadIdx.x; r < rows; r += 256) {
      const float sc = __fmul_rn(d.bn_weight[r], __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(d.bn_var[r], eps))));
      d.scale[r] = sc;
      if (d.shift) d.shift[r] = __fsub_rn(d.bn_bias[r], __fmul_rn(d.bn_mean[r], sc));
    }
  auto scale_of = [&](int co) { return __fmul_rn(d.bn_weight[co], __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(d.bn_var[co], eps)))); };
  if (d.kind == 0 || d.kind == 3) {
    const long total = (long)rows * cols;
    const long base = (long)blk * STAGE_CHUNK;
    const bool vec = (cols % 4) == 0 && ((((uintptr_t)d.w) & 15) == 0) && ((((uintptr_t)d.dst) & 15) == 0);
    if (vec) {
      for (long i = base + threadIdx.x * 4; i < base + STAGE_CHUNK && i < total; i += 1024) {
        f32x4 v = *(const f32x4*)(d.w + i);
        if (bn) { const float sc = scale_of((int)(i / cols));
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = __fmul_rn(v[t], sc); }
        if (d.kind == 3) *(f32x4*)((float*)d.dst + i) = v;
        else if (sizeof(T) == 4) *(f32x4*)((float*)d.dst + i) = v;
        else {
          unsigned int* o = (unsigned int*)((unsigned short*)d.dst + i);
          o[0] = pack_bf16x2(v[0], v[1]);
          o[1] = pack_bf16x2(v[2], v[3]);
        }
      }
    } else {
      for (long i = base + threadIdx.x; i < base + STAGE_CHUNK && i < total; i += 256) {
        float v = d.w[i];
        if (bn) v = __fmul_rn(v, scale_of((int)(i / cols)));
        if (d.kind == 3) ((float*)d.dst)[i] = v;
        else Elem<T>::store((T*)d.dst + i, v);
      }
    }
  } else if (d.kind == 1) {                                   // OIHW [co][ci][tap] -> [co][tap][ci]
    const int cic = stage_ci_chunk(cols), nch = (cols + cic - 1) / cic;
    const int co = blk / nch, ci0 = (blk - co * nch) * cic;
    const int CI = min(cic, cols - ci0);
    const float* src = d.w + ((long)co * cols + ci0) * 9;
    for (int e = threadIdx.x; e < CI * 9; e += 256) s_t[e] = src[e];
    __syncthreads();
    const float sc = bn ? scale_of(co) : 1.f;
    T* dst = (T*)d.dst + (long)co * 9 * cols + ci0;
    for (int e = threadIdx.x; e < CI * 9; e += 256) {
      const int tap = e / CI, ci = e - tap * CI;
      const float v = s_t[ci * 9 + tap];
      Elem<T>::store(dst + (long)tap * cols + ci, bn ? __fmul_rn(v, sc) : v);
    }
  } else {                                                    // OIHW -> [ci][8 - tap][co]
    constexpr int PITCH = STAGE_CI2 * 9 + 2;                  // 65: the write phase walks co at a fixed (ci, tap)
    const int nci = (cols + STAGE_CI2 - 1) / STAGE_CI2;
    const int cob = blk / nci, ci0 = (blk - cob * nci) * STAGE_CI2, co0 = cob * STAGE_CO2;
    const int CI = min(STAGE_CI2, cols - ci0), CO = min(STAGE_CO2, rows - co0);
    const int run = CI * 9;
    for (int e = threadIdx.x; e < CO * run; e += 256) {
      const int col = e / run, k = e - col * run;
      s_t[col * PITCH + k] = d.w[((long)(co0 + col) * cols + ci0) * 9 + k];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < run * CO; e += 256) {
      const int col = e % CO, k = e / CO;                     // k = ci_l * 9 + tapf
      const int cil = k / 9, tapf = k - cil * 9;
      float v = s_t[col * PITCH + cil * 9 + (8 - tapf)];
      if (bn) v = __fmul_rn(v, scale_of(co0 + col));
      Elem<T>::store((T*)d.dst + ((long)(ci0 + cil) * 9 + tapf) * rows + co0 + col, v);
    }
  }
}

// ---------------------------------------------------------------- per-image detector losses (Stage-3 split scoring)
// Each image's four training losses as if it were alone in its batch (unbias/split_single.py:66-75 runs one image per forward).
// Grid (DETLOSS_CHUNK-anchor chunks + DETLOSS_ROWS-row chunks, images): column c < chunks sums one chunk of that image's anchors
// (BCE over label >= 0, |delta - get_deltas(anchor, gt)|_1 and the count over label == 1); the columns after them each run up to
// DETLOSS_ROWS of the image's sampled ROI rows (one wave per row: focal / CE term, class-specific L1 box term, foreground count), as
// many columns as max_rows (the sampler's batch_size_per_image) needs, so an image's 512 rows spread over 8 workgroups instead of
// queuing behind one.  Partials go to [image][column][4]; det_loss_fold_kernel adds them in column order (deterministic) and
// applies the per-image normalisers.
constexpr int DETLOSS_CHUNK = 4096;
constexpr int DETLOSS_ROWS = 64;
__global__ __launch_bounds__(256) void det_loss_partial_kernel(
    long A, int chunks, const float* __restrict__ logits, const float* __restrict__ deltas, const signed char* __restrict__ labels,
    const float* __restrict__ anchors, const float* __restrict__ matched, float rx, float ry, float rw, float rh,
    const float* __restrict__ roi_logits, long ld, int K, const int* __restrict__ roi_cls, const float* __restrict__ roi_boxes,
    const float* __restrict__ roi_gt, const int* __restrict__ roi_counts, long roi_rows, long max_rows, float bx, float by,
    float bw, float bh, float gamma, float* __restrict__ partial) {
  __shared__ float red[32];
  const int img = blockIdx.y, c = blockIdx.x;
  float* out = partial + ((long)img * gridDim.x + c) * 4;
  if (c < chunks) {
    const long lo = (long)c * DETLOSS_CHUNK, hi = lo + DETLOSS_CHUNK < A ? lo + DETLOSS_CHUNK : A;
    const long base = (long)img * A;
    float s_obj = 0.f, s_loc = 0.f, s_fg = 0.f;
    for (long a = lo + threadIdx.x; a < hi; a += blockDim.x) {
      const long i = base + a;
      const int lab = labels[i];
      if (lab >= 0) s_obj += bce_with_logits(logits[i], (float)lab);
      if (lab == 1) {
        float t[4];
        box_deltas(anchors + a * 4, matched + i * 4, rx, ry, rw, rh, t);
#pragma unroll
        for (int k = 0; k < 4; ++k) s_loc += fabsf(deltas[i * 4 + k] - t[k]);
        s_fg += 1.f;
      }
    }
    s_obj = block_reduce_sum(s_obj, red);
    __syncthreads();
    s_loc = block_reduce_sum(s_loc, red);
    __syncthreads();
    s_fg = block_reduce_sum(s_fg, red);
    if (threadIdx.x == 0) { out[0] = s_obj; out[1] = s_loc; out[2] = s_fg; out[3] = 0.f; }
    return;
  }
  // ROI rows of this image: packed back to back, image i's rows start at sum(roi_counts[0..i)); this column takes rows
  // [r0, r1) of them
  long off = 0;
  for (int j = 0; j < img; ++j) off += roi_counts[j];
  const long n = roi_counts[img];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const float nan = __uint_as_float(0x7FC00000u);
  if (n < 0 || n > max_rows || off < 0 || off + n > roi_rows) {          // inconsistent counts: no read out of bounds, no number
    if (threadIdx.x == 0) { out[0] = nan; out[1] = nan; out[2] = nan; out[3] = nan; }
    return;
  }
  const long r0 = (long)(c - chunks) * DETLOSS_ROWS, r1 = r0 + DETLOSS_ROWS < n ? r0 + DETLOSS_ROWS : n;
  const int C = K + 1;
  float s_ce = 0.f, s_box = 0.f, s_fg = 0.f;                             // lane 0 of each wave
  for (long r = off + r0 + w; r < off + r1; r += nw) {
    const float* x = roi_logits + r * ld;
    const int t = roi_cls[r];
    if ((unsigned)t >= (unsigned)C) { s_ce = nan; continue; }            // (focal_loss_kernel's rule for a class outside [0, C))
    const float ce = row_cross_entropy(x, C, lane).ce(x[t]);
    s_ce += powf(fmaxf(1.f - expf(-ce), 0.f), gamma) * ce;              // gamma 0: the plain cross-entropy term
    if (t < K) {
      float tg[4];
      box_deltas(roi_boxes + r * 4, roi_gt + r * 4, bx, by, bw, bh, tg);
      const float* pd = x + C + 4 * t;
#pragma unroll
      for (int k = 0; k < 4; ++k) s_box += fabsf(pd[k] - tg[k]);
      s_fg += 1.f;
    }
  }
  __syncthreads();
  if (lane == 0) { red[w] = s_ce; red[8 + w] = s_box; red[16 + w] = s_fg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f, f = 0.f;
    for (int k = 0; k < nw; ++k) { a += red[k]; b += red[8 + k]; f += red[16 + k]; }   // wave order: deterministic
    out[0] = a; out[1] = b; out[2] = f; out[3] = (float)(r1 > r0 ? r1 - r0 : 0);
  }
}

// out [image][5] = loss_cls, loss_box_reg, loss_rpn_cls, loss_rpn_loc, their sum (f32, left to right: split_single.py:74)
//   loss_rpn_cls = BCE sum / B_rpn;  loss_rpn_loc = L1 sum / B_rpn (smooth_l1) or L1 sum / (4 fg anchors) / B_rpn (smooth_l1_mean,
//   rpn.py:405-425 with box_regression.py:261-268);  loss_cls = CE sum / rows, 0 without rows (layers/wrappers.py:26-33);
//   loss_box_reg = L1 sum / max(rows, 1) (smooth_l1) or L1 sum / (4 fg rows) (smooth_l1_mean, fast_rcnn.py:534-564).  The mean of
//   an empty foreground set is 0 / 0 = NaN, as torch's mean of an empty tensor.
__global__ void det_loss_fold_kernel(int n_img, int chunks, int rchunks, const float* __restrict__ partial, float rpn_bs,
                                     int rpn_mean, int roi_mean, float* __restrict__ out) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= n_img) return;
  const float* p = partial + (long)img * (chunks + rchunks) * 4;
  float so = 0.f, sl = 0.f, sf = 0.f;
  for (int c = 0; c < chunks; ++c) { so += p[c * 4]; sl += p[c * 4 + 1]; sf += p[c * 4 + 2]; }
  float ce = 0.f, box = 0.f, fg = 0.f, rows = 0.f;             // (NaN when the image's counts were inconsistent: stays NaN)
  for (int c = chunks; c < chunks + rchunks; ++c) { ce += p[c * 4]; box += p[c * 4 + 1]; fg += p[c * 4 + 2]; rows += p[c * 4 + 3]; }
  const float l_cls = rows == 0.f ? 0.f : ce / rows;
  const float l_box = roi_mean ? box / (4.f * fg) : box / fmaxf(rows, 1.f);
  const float l_rpn_cls = so / rpn_bs;
  const float l_rpn_loc = rpn_mean ? (sl / (4.f * sf)) / rpn_bs : sl / rpn_bs;
  float* o = out + (long)img * 5;
  o[0] = l_cls; o[1] = l_box; o[2] = l_rpn_cls; o[3] = l_rpn_loc;
  o[4] = ((l_cls + l_box) + l_rpn_cls) + l_rpn_loc;
}

}  // namespace

// every launch below: 256 threads, a grid-stride loop over n items
#define LAUNCH_N(kernel, n, ...) hipLaunchKernelGGL((kernel), dim3(grid_for((n), GRID_CAP)), dim3(256), 0, stream, __VA_ARGS__)

extern "C" int sw_preprocess_pad(int dtype, int h, int w, int H, int W, const uint8_t* img_chw, const float* mean3,
                                 const float* std3, void* out_nhwc4, hipStream_t stream) {
  SW_ENTER();
  if (h > H || w > W || H <= 0 || W <= 0) return -5;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    LAUNCH_N(preprocess_pad_kernel<T>, (long)H * W, h, w, H, W, img_chw, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
             (T*)out_nhwc4);
  });
}

extern "C" int sw_stem_conv7x7(int dtype, int N, int H, int W, const void* in_nhwc4, const float* w_oihw, const float* scale,
                               const float* bias, void* out_nhwc64, hipStream_t stream) {
  SW_ENTER();
  const int OH = (H + 6 - 7) / 2 + 1, OW = (W + 6 - 7) / 2 + 1;
  if (N <= 0 || OH <= 0 || OW <= 0) return 0;
  const long tiles = (long)N * ((OH + 7) / 8) * ((OW + 7) / 8);
  if (tiles > 2147483647L) return -6;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    hipLaunchKernelGGL(stem_conv7_kernel<T>, dim3((unsigned)tiles), dim3(256), 0, stream, N, H, W, OH, OW, (const T*)in_nhwc4, w_oihw,
                       scale, bias, (T*)out_nhwc64);
  });
}

extern "C" int sw_maxpool3x3s2(int dtype, int N, int H, int W, int C, const void* in, void* out, hipStream_t stream) {
  SW_ENTER();
  const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
  const long n = (long)N * OH * OW * C;
  if (n <= 0) return 0;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    constexpr int V = 16 / (int)sizeof(T);
    if (vec16_ok<T>(C, in, out)) LAUNCH_N((maxpool3x3s2_kernel<T, V>), n / V, N, H, W, C, OH, OW, (const T*)in, (T*)out);
    else LAUNCH_N((maxpool3x3s2_kernel<T, 1>), n, N, H, W, C, OH, OW, (const T*)in, (T*)out);
  });
}

extern "C" int sw_subsample2x(int dtype, int N, int H, int W, int C, const void* in, void* out, hipStream_t stream) {
  SW_ENTER();
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const long n = (long)N * OH * OW * C;
  if (n <= 0) return 0;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    constexpr int V = 16 / (int)sizeof(T);
    if (vec16_ok<T>(C, in, out))                              // a copy: 16-byte pieces of a pixel's channel run when they exist
      LAUNCH_N(subsample2_kernel<u32x4>, n / V, N, H, W, C / V, OH, OW, (const u32x4*)in, (u32x4*)out);
    else LAUNCH_N(subsample2_kernel<T>, n, N, H, W, C, OH, OW, (const T*)in, (T*)out);
  });
}

extern "C" int sw_scatter2x(int dtype, int N, int H, int W, int C, const void* g, void* out, hipStream_t stream) {
  SW_ENTER();
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const long n = (long)N * H * W * C;
  if (n <= 0) return 0;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    constexpr int V = 16 / (int)sizeof(T);
    if (vec16_ok<T>(C, g, out)) LAUNCH_N(scatter2_kernel<u32x4>, n / V, N, H, W, C / V, OH, OW, (const u32x4*)g, (u32x4*)out);
    else LAUNCH_N(scatter2_kernel<T>, n, N, H, W, C, OH, OW, (const T*)g, (T*)out);
  });
}

extern "C" int sw_add_relu(int dtype, long n, const void* a, const void* b, void* out, int relu, hipStream_t stream) {
  SW_ENTER();
  if (n <= 0) return 0;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    LAUNCH_N(add_relu_kernel<T>, n, n, (const T*)a, (const T*)b, (T*)out, relu);
  });
}

extern "C" int sw_upsample2x_add(int dtype, int N, int h, int w, int C, const void* lateral, const void* top, void* out,
                                 hipStream_t stream) {
  SW_ENTER();
  const long n = (long)N * 4 * h * w * C;
  if (n <= 0) return 0;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    constexpr int V = 16 / (int)sizeof(T);
    if (vec16_ok<T>(C, lateral, top, out))
      LAUNCH_N((upsample2_add_kernel<T, V>), n / V, N, h, w, C, (const T*)lateral, (const T*)top, (T*)out);
    else LAUNCH_N((upsample2_add_kernel<T, 1>), n, N, h, w, C, (const T*)lateral, (const T*)top, (T*)out);
  });
}

extern "C" int sw_downsample2x_sum(int dtype, int N, int h, int w, int C, const void* g, void* out, hipStream_t stream) {
  SW_ENTER();
  const long n = (long)N * h * w * C;
  if (n <= 0) return 0;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    constexpr int V = 16 / (int)sizeof(T);
    if (vec16_ok<T>(C, g, out)) LAUNCH_N((downsample2_sum_kernel<T, V>), n / V, N, h, w, C, (const T*)g, (T*)out);
    else LAUNCH_N((downsample2_sum_kernel<T, 1>), n, N, h, w, C, (const T*)g, (T*)out);
  });
}

extern "C" int sw_roi_align_fwd(int dtype, int H, int W, int C, int PH, int PW, float spatial_scale, int sampling_ratio,
                                const void* feat, const float* rois, const int32_t* sel, int n_sel, const int32_t* n_sel_dev, void* out, long ld_out,
                                hipStream_t stream) {
  SW_ENTER();
  if (n_sel <= 0) return 0;
  if (ld_out < (long)C * PH * PW) return -5;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    LAUNCH_N(roi_align_fwd_kernel<T>, (long)n_sel * PH * PW * C, H, W, C, PH, PW, spatial_scale, sampling_ratio, (const T*)feat, rois, sel,
             n_sel, n_sel_dev, (T*)out, ld_out);
  });
}

extern "C" int sw_roi_align_bwd(int dtype, int H, int W, int C, int PH, int PW, float spatial_scale, int sampling_ratio,
                                const void* gout, long ld, const float* rois, const int32_t* sel, int n_sel, const int32_t* n_sel_dev, float* dfeat_f32,
                                hipStream_t stream) {
  SW_ENTER();
  if (n_sel <= 0) return 0;
  if (ld < (long)C * PH * PW) return -5;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    LAUNCH_N((roi_align_bwd_kernel<T, AccF32>), (long)n_sel * PH * PW * C, H, W, C, PH, PW, spatial_scale, sampling_ratio, (const T*)gout,
             ld, rois, sel, n_sel, n_sel_dev, AccF32::Arg{}, dfeat_f32);
  });
}

extern "C" int sw_roi_align_bwd_fx(int dtype, int H, int W, int C, int PH, int PW, float spatial_scale, int sampling_ratio,
                                   const void* gout, long ld, const float* rois, const int32_t* sel, int n_sel, const int32_t* n_sel_dev,
                                   const float* gout_absmax, long long* acc_i64, hipStream_t stream) {
  SW_ENTER();
  if (n_sel <= 0) return 0;
  if (ld < (long)C * PH * PW || !gout_absmax || !acc_i64) return -5;
  return dispatch_elem(dtype, [&](auto elem) {
    using T = decltype(elem);
    LAUNCH_N((roi_align_bwd_kernel<T, AccFx>), (long)n_sel * PH * PW * C, H, W, C, PH, PW, spatial_scale, sampling_ratio, (const T*)gout,
             ld, rois, sel, n_sel, n_sel_dev, gout_absmax, (unsigned long long*)acc_i64);
  });
}

extern "C" int sw_fx_to_float(int out_dtype, long n, const long long* acc_i64, const float* absmax, void* out, hipStream_t stream) {
  SW_ENTER();
  if (n <= 0) return 0;
  if (!acc_i64 || !absmax || !out) return -5;
  return dispatch_elem(out_dtype, [&](auto elem) {
    using T = decltype(elem);
    LAUNCH_N(fx_to_float_kernel<T>, n, n, acc_i64, absmax, (T*)out);
  });
}

extern "C" long sw_rpn_loss_workspace_floats(void) { return 2L * RPN_LOSS_BLOCKS; }

extern "C" int sw_rpn_loss(long n, long n_anchors, const float* logits, const float* deltas, const int8_t* labels,
                           const float* anchors, const float* matched_gt_boxes, const float* weights4, float inv_norm,
                           float* losses2, float* dlogits, float* ddeltas, float* workspace, hipStream_t stream) {
  SW_ENTER();
  if (n <= 0 || n_anchors <= 0) return -5;
  int blocks = grid_for(n, GRID_CAP);
  if (blocks > RPN_LOSS_BLOCKS) blocks = RPN_LOSS_BLOCKS;
  hipLaunchKernelGGL(rpn_loss_kernel, dim3(blocks), dim3(256), 0, stream, n, n_anchors, logits, deltas, (const signed char*)labels,
                     anchors, matched_gt_boxes, weights4[0], weights4[1], weights4[2], weights4[3], inv_norm, workspace, dlogits,
                     ddeltas);
  hipLaunchKernelGGL(rpn_loss_fold_kernel, dim3(1), dim3(64), 0, stream, blocks, (const float*)workspace, inv_norm, losses2);
  SW_CHECK_LAUNCH();
  return 0;
}

extern "C" long sw_det_loss_workspace_floats(int n_img, long n_anchors, long max_rows) {
  if (n_img <= 0 || n_anchors <= 0 || max_rows < 0) return 0;
  const long rchunks = max_rows > 0 ? (max_rows + DETLOSS_ROWS - 1) / DETLOSS_ROWS : 1;
  return (long)n_img * ((n_anchors + DETLOSS_CHUNK - 1) / DETLOSS_CHUNK + rchunks) * 4;
}

extern "C" int sw_det_loss_per_image(int n_img, long n_anchors, const float* rpn_logits, const float* rpn_deltas,
                                     const int8_t* rpn_labels, const float* anchors, const float* rpn_matched,
                                     const float* rpn_weights4, int rpn_batch_size, int rpn_loss_type, const float* roi_logits,
                                     long ld, int K, const int32_t* roi_classes, const float* roi_boxes, const float* roi_gt_boxes,
                                     const int32_t* roi_counts, long roi_rows, long max_rows, const float* roi_weights4, float gamma,
                                     int roi_loss_type, float* out, float* workspace, hipStream_t stream) {
  SW_ENTER();
  if (n_img <= 0) return 0;
  if (n_img > 65535 || n_anchors <= 0 || K <= 0 || ld < 5L * K + 1 || rpn_batch_size <= 0 || roi_rows < 0 || max_rows < 0) return -5;
  if ((unsigned)rpn_loss_type > 1u || (unsigned)roi_loss_type > 1u || !roi_counts) return -5;
  if (roi_rows > 0 && (!roi_logits || !roi_classes || !roi_boxes || !roi_gt_boxes)) return -5;
  const long chunks = (n_anchors + DETLOSS_CHUNK - 1) / DETLOSS_CHUNK;
  const long rchunks = max_rows > 0 ? (max_rows + DETLOSS_ROWS - 1) / DETLOSS_ROWS : 1;
  if (chunks + rchunks > 2147483647L) return -5;
  hipLaunchKernelGGL(det_loss_partial_kernel, dim3((unsigned)(chunks + rchunks), (unsigned)n_img), dim3(256), 0, stream, n_anchors,
                     (int)chunks, rpn_logits, rpn_deltas, (const signed char*)rpn_labels, anchors, rpn_matched, rpn_weights4[0],
                     rpn_weights4[1], rpn_weights4[2], rpn_weights4[3], roi_logits, ld, K, roi_classes, roi_boxes, roi_gt_boxes,
                     roi_counts, roi_rows, max_rows, roi_weights4[0], roi_weights4[1], roi_weights4[2], roi_weights4[3], gamma,
                     workspace);
  hipLaunchKernelGGL(det_loss_fold_kernel, dim3((n_img + 63) / 64), dim3(64), 0, stream, n_img, (int)chunks, (int)rchunks,
                     (const float*)workspace, (float)rpn_batch_size, rpn_loss_type, roi_loss_type, out);
  SW_CHECK_LAUNCH();
  return 0;
}

extern "C" int sw_stage_blocks(int kind, int rows, int cols) {
  if (kind == 1) { const int cic = stage_ci_chunk(cols); return rows * ((cols + cic - 1) / cic); }
  if (kind == 2) return ((rows + STAGE_CO2 - 1) / STAGE_CO2) * ((cols + STAGE_CI2 - 1) / STAGE_CI2);
  const long total = (long)rows * cols;
  return (int)((total + STAGE_CHUNK - 1) / STAGE_CHUNK);
}

extern "C" int sw_stage_weights_multi(int dtype, int n, const sw_stage_desc* descs_dev, int total_blocks, float eps,
                                      hipStream_t stream) {
  SW_ENTER();
  if (n <= 0 || total_blocks <= 0) return 0;
  return dispatch_elem(dtype, [&](auto elem) {
    hipLaunchKernelGGL(stage_weights_multi_kernel<decltype(elem)>, dim3(total_blocks), dim3(256), 0, stream, n, descs_dev, eps);
  });
}

// Stage-3 strong augmentation on planar (3, H, W) uint8 images (the reference's build_strong_augmentation,
// unbias/ubteacher/data/detection_utils.py:9-46: torchvision ColorJitter / RandomGrayscale, a Pillow GaussianBlur, three
// RandomErasing).  Every pixel operation restates Pillow's arithmetic bit for bit (tests/strong_aug_ref.py is the checker,
// tests/golden/strong_aug.npz the Pillow-made fixture).
//
// One recipe = up to four colour-jitter blends in a drawn order, grayscale, Gaussian blur, up to three erased rectangles.
// The launch sequence (a batch = blockIdx.y):
//   1. lsum    (only with contrast)  sum of L over the image as it is when contrast is reached — the one whole-image dependence
//   2a. point  (no blur)             in -> jitter ops, grayscale, erasing -> out
//   2b. blur_h (blur)                in -> jitter ops, grayscale -> three box passes along x in LDS -> tmp
//       blur_v                       tmp -> three box passes along y in LDS -> erasing -> out
// The point-wise ops never make a round trip of their own: they are recomputed where the image is read (the ops in front of
// contrast twice: once for the sum, once for the pixels).  With everything on the image is read 3 times and written twice.
#include "common.h"
#include "soswsod_hip.h"

namespace {

struct AugArgs { const sw_aug_item* items; sw_aug_item one; };            // items == nullptr: the single image `one`
__device__ __forceinline__ const sw_aug_item& aug_item(const AugArgs& a, int i) { return a.items ? a.items[i] : a.one; }

// ---- Pillow's point arithmetic
__device__ __forceinline__ int lum(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }   // convert("L")

// Image.blend(degenerate, image, f): float32 `d + f * (x - d)`, clipped to [0, 255], truncated
__device__ __forceinline__ int blend(float d, float f, int x) {
  const float t = d + f * ((float)x - d);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// convert("HSV"), H += shift (mod 256), convert("RGB"): Pillow's rgb2hsv_row / hsv2rgb, float and double widths as in its C
__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = maxc;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double a = (double)h / 6.0 + 1.0;                 // in [5/6, 2): fmod(a, 1.0) == a - floor(a), exact
    h = (float)(a - floor(a));
    uh = min(max((int)((double)h * 255.0), 0), 255);
    us = min(max((int)((double)s * 255.0), 0), 255);
  }
  uh = (uh + shift) & 255;
  if (us == 0) { r = g = b = uv; return; }
  const double hf = (double)(float)uh * 6.0 / 255.0;
  const int i = (int)floor(hf);
  const float f = (float)(hf - (double)(float)i);
  const float fs = (float)((double)(float)us / 255.0);
  const double v = (double)(float)uv;
  const int p = min(max((int)round(v * (1.0 - (double)fs)), 0), 255);
  const int q = min(max((int)round(v * (1.0 - (double)fs * (double)f)), 0), 255);
  const int t = min(max((int)round(v * (1.0 - (double)fs * (1.0 - (double)f))), 0), 255);
  switch (i % 6) {
    case 0: r = uv; g = t; b = p; break;
    case 1: r = q; g = uv; b = p; break;
    case 2: r = p; g = uv; b = t; break;
    case 3: r = p; g = q; b = uv; break;
    case 4: r = t; g = p; b = uv; break;
    default: r = uv; g = p; b = q; break;
  }
}

// jitter slots [from, to) of the recipe's order; cdeg = contrast's degenerate value int(mean(L) + 0.5)
__device__ __forceinline__ void jitter_ops(int& r, int& g, int& b, const sw_aug_recipe& R, int from, int to, float cdeg) {
  for (int s = from; s < to; ++s) {
    const int op = R.order[s];
    if (op == SW_AUG_BRIGHTNESS) {
      const float f = R.factor[0];
      r = blend(0.f, f, r); g = blend(0.f, f, g); b = blend(0.f, f, b);
    } else if (op == SW_AUG_CONTRAST) {
      const float f = R.factor[1];
      r = blend(cdeg, f, r); g = blend(cdeg, f, g); b = blend(cdeg, f, b);
    } else if (op == SW_AUG_SATURATION) {
      const float f = R.factor[2], d = (float)lum(r, g, b);
      r = blend(d, f, r); g = blend(d, f, g); b = blend(d, f, b);
    } else if (op == SW_AUG_HUE) {
      hue_shift(r, g, b, R.hue_shift);
    }
  }
}

__device__ __forceinline__ int contrast_slot(const sw_aug_recipe& R) {
  for (int s = 0; s < 4; ++s) if (R.order[s] == SW_AUG_CONTRAST) return s;
  return -1;
}
__device__ __forceinline__ bool any_point_op(const sw_aug_recipe& R) {
  return R.grayscale || R.order[0] >= 0 || R.order[1] >= 0 || R.order[2] >= 0 || R.order[3] >= 0;
}
// ImageStat.Stat(L).mean[0] = sum / count in double; ImageEnhance.Contrast takes int(mean + 0.5)
__device__ __forceinline__ float contrast_degenerate(const sw_aug_item& it) {
  return (float)(int)((double)(*it.lsum) / (double)((long)it.H * it.W) + 0.5);
}
__device__ __forceinline__ void point_ops(int& r, int& g, int& b, const sw_aug_recipe& R, float cdeg) {
  jitter_ops(r, g, b, R, 0, 4, cdeg);
  if (R.grayscale) r = g = b = lum(r, g, b);
}

// ---- erasing: byte(255 * n), n ~ N(0, 1) from a counter-based generator: four rounds of splitmix64 over
// (seed, image key, erasing index * 4 + channel, (y - top) << 32 | (x - left)), two 24-bit uniforms, Box-Muller; the float is
// truncated toward zero and wrapped modulo 256 (torch's CPU .byte()).  A sample depends on nothing but its coordinates.
__device__ __forceinline__ int erase_byte(const sw_aug_recipe& R, int e, int c, int dy, int dx) {
  uint64_t h = sw_splitmix64(R.seed);
  h = sw_splitmix64(h ^ R.key);
  h = sw_splitmix64(h ^ (uint64_t)(e * 4 + c));
  h = sw_splitmix64(h ^ (((uint64_t)(uint32_t)dy << 32) | (uint64_t)(uint32_t)dx));
  const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777216.0f);          // (0, 1]
  const float u2 = (float)(uint32_t)((h >> 16) & 0xFFFFFFu) * (1.0f / 16777216.0f);     // [0, 1)
  const float n = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
  return ((int)(255.0f * n)) & 255;
}
__device__ __forceinline__ bool any_rect(const sw_aug_recipe& R) { return R.rect[0][2] > 0 || R.rect[1][2] > 0 || R.rect[2][2] > 0; }
// the erasings run one after the other: a later rectangle overwrites an earlier one
__device__ __forceinline__ int erased(const sw_aug_recipe& R, int c, int y, int x, int v) {
#pragma unroll
  for (int e = 2; e >= 0; --e) {
    const int top = R.rect[e][0], left = R.rect[e][1], h = R.rect[e][2], w = R.rect[e][3];
    if (h > 0 && y >= top && y < top + h && x >= left && x < left + w) return erase_byte(R, e, c, y - top, x - left);
  }
  return v;
}

// ---- up to four bytes of a line as one word: a 4-byte access when the line allows it
__device__ __forceinline__ uint32_t load4(const uint8_t* p, long i, long n, bool aligned) {
  if (aligned && i + 4 <= n) return *(const uint32_t*)(p + i);
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k) if (i + k < n) v |= (uint32_t)p[i + k] << (8 * k);
  return v;
}
__device__ __forceinline__ void store4(uint8_t* p, long i, long n, bool aligned, uint32_t v) {
  if (aligned && i + 4 <= n) { *(uint32_t*)(p + i) = v; return; }
  for (int k = 0; k < 4; ++k) if (i + k < n) p[i + k] = (uint8_t)(v >> (8 * k));
}
__device__ __forceinline__ bool aligned4(const void* p, long ld) { return ((((uintptr_t)p) | (uintptr_t)ld) & 3) == 0; }

__global__ void aug_zero_sums_kernel(AugArgs a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const sw_aug_item& it = aug_item(a, i); if (it.lsum) *it.lsum = 0ull; }
}

// 1. integer sum of L over the image after the jitter ops in front of contrast (integer addition: any order is exact)
__global__ __launch_bounds__(256) void aug_lsum_kernel(AugArgs a) {
  const sw_aug_item& it = aug_item(a, blockIdx.y);
  const sw_aug_recipe& R = it.recipe;
  const int cs = contrast_slot(R);
  if (cs < 0) return;
  const long n = (long)it.H * it.W, nw = (n + 3) >> 2;
  const bool al = aligned4(it.in, n);
  unsigned int acc = 0;                                      // <= 255 * 4 per word, < 2^22 words per thread
  for (long w = blockIdx.x * (long)blockDim.x + threadIdx.x; w < nw; w += (long)gridDim.x * blockDim.x) {
    const uint32_t wr = load4(it.in, 4 * w, n, al), wg = load4(it.in + n, 4 * w, n, al), wb = load4(it.in + 2 * n, 4 * w, n, al);
    const int m = (int)min(4L, n - 4 * w);
    for (int k = 0; k < m; ++k) {
      int r = (wr >> (8 * k)) & 255, g = (wg >> (8 * k)) & 255, b = (wb >> (8 * k)) & 255;
      jitter_ops(r, g, b, R, 0, cs, 0.f);
      acc += (unsigned int)lum(r, g, b);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += (unsigned int)__shfl_xor((int)acc, o, 64);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd((unsigned long long*)it.lsum, (unsigned long long)acc);
}

// 2a. images without blur: point ops + erasing, four pixels per thread
__global__ __launch_bounds__(256) void aug_point_kernel(AugArgs a) {
  const sw_aug_item& it = aug_item(a, blockIdx.y);
  const sw_aug_recipe& R = it.recipe;
  if (R.blur_r >= 0) return;
  const long n = (long)it.H * it.W, nw = (n + 3) >> 2;
  const long w = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (w >= nw) return;
  const bool al = aligned4(it.in, n) && aligned4(it.out, n);
  const bool ops = any_point_op(R), rects = any_rect(R);
  const float cdeg = contrast_slot(R) >= 0 ? contrast_degenerate(it) : 0.f;
  const uint32_t wr = load4(it.in, 4 * w, n, al), wg = load4(it.in + n, 4 * w, n, al), wb = load4(it.in + 2 * n, 4 * w, n, al);
  uint32_t o0 = 0, o1 = 0, o2 = 0;
  int y = (int)((4 * w) / it.W), x = (int)((4 * w) % it.W);
  for (int k = 0; k < 4; ++k) {
    int r = (wr >> (8 * k)) & 255, g = (wg >> (8 * k)) & 255, b = (wb >> (8 * k)) & 255;
    if (ops) point_ops(r, g, b, R, cdeg);
    if (rects) { r = erased(R, 0, y, x, r); g = erased(R, 1, y, x, g); b = erased(R, 2, y, x, b); }
    o0 |= (uint32_t)r << (8 * k); o1 |= (uint32_t)g << (8 * k); o2 |= (uint32_t)b << (8 * k);
    if (++x == it.W) { x = 0; ++y; }
  }
  store4(it.out, 4 * w, n, al, o0); store4(it.out + n, 4 * w, n, al, o1); store4(it.out + 2 * n, 4 * w, n, al, o2);
}

// ---- Pillow's box blur: one output of one pass, ImagingLineBoxBlur8's integer arithmetic on a line with replicated edges.
// `at(k)` returns the sample at line position k already clamped.
constexpr int BLUR_HALO = 9;                                 // three passes reach 3 * (r + 1) samples; r <= 2
template <typename At>
__device__ __forceinline__ uint32_t box_sample(int i, int r, uint32_t ww, uint32_t fw, At at) {
  uint32_t s = 0;
  for (int k = -r; k <= r; ++k) s += at(i + k);
  return (ww * s + fw * (at(i - r - 1) + at(i + r + 1)) + (1u << 23)) >> 24;
}

// 2b. point ops, then the three passes along x.  One workgroup = BH_TW outputs of one row, all three channels; the passes run on
// the whole LDS line (reads clamped to the image line and to the buffer), so what the buffer's ends lack creeps inward by
// r + 1 per pass and stops short of the BH_TW outputs behind a halo of BH_PAD >= BLUR_HALO.
constexpr int BH_TW = 1024, BH_PAD = 12, BH_BW = BH_TW + 2 * BH_PAD;
__global__ __launch_bounds__(256) void aug_blur_h_kernel(AugArgs a, int tiles_x) {
  const sw_aug_item& it = aug_item(a, blockIdx.y);
  const sw_aug_recipe& R = it.recipe;
  if (R.blur_r < 0) return;
  const int y = blockIdx.x / tiles_x, x0 = (blockIdx.x % tiles_x) * BH_TW, W = it.W;
  if (y >= it.H || x0 >= W) return;
  __shared__ __attribute__((aligned(16))) uint8_t buf[2][3][BH_BW];
  const long n = (long)it.H * W;
  const uint8_t* row = it.in + (long)y * W;
  const bool al = aligned4(it.in, W) && (n & 3) == 0;
  const bool ops = any_point_op(R);
  const float cdeg = contrast_slot(R) >= 0 ? contrast_degenerate(it) : 0.f;
  const int g0 = x0 - BH_PAD;                                // image x of buffer position 0 (a multiple of 4)
  for (int j = threadIdx.x; j < BH_BW / 4; j += blockDim.x) {
    const int gx = g0 + 4 * j;
    if (gx + 4 <= 0 || gx >= W) continue;                    // never read: the passes clamp to the line
    uint32_t wr = 0, wg = 0, wb = 0;
    if (gx >= 0) { wr = load4(row, gx, W, al); wg = load4(row + n, gx, W, al); wb = load4(row + 2 * n, gx, W, al); }
    for (int k = 0; k < 4; ++k) {
      const int x = gx + k;
      if (x < 0 || x >= W) continue;
      int r, g, b;
      if (gx >= 0) { r = (wr >> (8 * k)) & 255; g = (wg >> (8 * k)) & 255; b = (wb >> (8 * k)) & 255; }
      else { r = row[x]; g = row[n + x]; b = row[2 * n + x]; }
      if (ops) point_ops(r, g, b, R, cdeg);
      buf[0][0][4 * j + k] = (uint8_t)r; buf[0][1][4 * j + k] = (uint8_t)g; buf[0][2][4 * j + k] = (uint8_t)b;
    }
  }
  const int r = R.blur_r;
  const uint32_t ww = R.blur_ww, fw = R.blur_fw;
  for (int pass = 0; pass < 3; ++pass) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 3 * BH_BW; idx += blockDim.x) {
      const int c = idx / BH_BW, i = idx - c * BH_BW, gx = g0 + i;
      if (gx < 0 || gx >= W) continue;
      const uint8_t* src = buf[pass & 1][c];
      buf[(pass + 1) & 1][c][i] = (uint8_t)box_sample(gx, r, ww, fw, [&](int k) -> uint32_t {
        return src[min(max(min(max(k, 0), W - 1) - g0, 0), BH_BW - 1)];
      });
    }
  }
  __syncthreads();
  uint8_t* orow = it.tmp + (long)y * W;
  const bool alo = aligned4(it.tmp, W) && (n & 3) == 0;
  for (int idx = threadIdx.x; idx < 3 * (BH_TW / 4); idx += blockDim.x) {
    const int c = idx / (BH_TW / 4), j = idx - c * (BH_TW / 4), gx = x0 + 4 * j;
    if (gx >= W) continue;
    store4(orow + c * n, gx, W, alo, *(const uint32_t*)&buf[1][c][BH_PAD + 4 * j]);
  }
}

// the three passes along y, then erasing.  One workgroup = a BV_TW x BV_TH tile of one channel with BLUR_HALO rows above and below;
// a thread owns a word of four neighbouring columns.
constexpr int BV_TW = 256, BV_TH = 64, BV_ROWS = BV_TH + 2 * BLUR_HALO;
__global__ __launch_bounds__(256) void aug_blur_v_kernel(AugArgs a, int tiles_x) {
  const sw_aug_item& it = aug_item(a, blockIdx.y);
  const sw_aug_recipe& R = it.recipe;
  if (R.blur_r < 0) return;
  const int c = blockIdx.z, H = it.H, W = it.W;
  const int x0 = (blockIdx.x % tiles_x) * BV_TW, y0 = (blockIdx.x / tiles_x) * BV_TH;
  if (x0 >= W || y0 >= H) return;
  __shared__ uint32_t buf[2][BV_ROWS][BV_TW / 4];
  const long n = (long)H * W;
  const uint8_t* src = it.tmp + c * n;
  const bool al = aligned4(it.tmp, W) && (n & 3) == 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, x = x0 + 4 * lane;
  const int g0 = y0 - BLUR_HALO;
  for (int j = wave; j < BV_ROWS; j += 4) {
    const int gy = g0 + j;
    if (gy < 0 || gy >= H || x >= W) continue;
    buf[0][j][lane] = load4(src + (long)gy * W, x, W, al);
  }
  const int r = R.blur_r;
  const uint32_t ww = R.blur_ww, fw = R.blur_fw;
  for (int pass = 0; pass < 3; ++pass) {
    __syncthreads();
    if (x >= W) continue;
    for (int j = wave; j < BV_ROWS; j += 4) {
      const int gy = g0 + j;
      if (gy < 0 || gy >= H) continue;
      uint32_t o = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        o |= box_sample(gy, r, ww, fw, [&](int k) -> uint32_t {
               return (buf[pass & 1][min(max(min(max(k, 0), H - 1) - g0, 0), BV_ROWS - 1)][lane] >> (8 * b)) & 255u;
             }) << (8 * b);
      buf[(pass + 1) & 1][j][lane] = o;
    }
  }
  __syncthreads();
  if (x >= W) return;
  uint8_t* dst = it.out + c * n;
  const bool alo = aligned4(it.out, W) && (n & 3) == 0;
  const bool rects = any_rect(R);
  for (int j = BLUR_HALO + wave; j < BLUR_HALO + BV_TH; j += 4) {
    const int gy = g0 + j;
    if (gy >= H) break;
    uint32_t o = buf[1][j][lane];
    if (rects) {
      uint32_t e = 0;
      for (int b = 0; b < 4; ++b) e |= (uint32_t)erased(R, c, gy, x + b, (o >> (8 * b)) & 255) << (8 * b);
      o = e;
    }
    store4(dst + (long)gy * W, x, W, alo, o);
  }
}

int launch_strong_aug(const AugArgs& a, int n, int max_h, int max_w, int stages, hipStream_t stream) {
  if (n <= 0) return 0;
  if (max_h <= 0 || max_w <= 0 || n > 65535) return -6;
  const long px = (long)max_h * max_w;
  if (stages & SW_AUG_STAGE_CONTRAST) {
    hipLaunchKernelGGL(aug_zero_sums_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a, n);
    long blocks = ((px + 3) / 4 + 255) / 256;
    blocks = blocks > 512 ? 512 : blocks;
    hipLaunchKernelGGL(aug_lsum_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, stream, a);
  }
  if (stages & SW_AUG_STAGE_POINT) {
    const long blocks = ((px + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(aug_point_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, stream, a);
  }
  if (stages & SW_AUG_STAGE_BLUR) {
    const int th = (max_w + BH_TW - 1) / BH_TW;
    hipLaunchKernelGGL(aug_blur_h_kernel, dim3((unsigned)(th * max_h), (unsigned)n), dim3(256), 0, stream, a, th);
    const int tv = (max_w + BV_TW - 1) / BV_TW;
    hipLaunchKernelGGL(aug_blur_v_kernel, dim3((unsigned)(tv * ((max_h + BV_TH - 1) / BV_TH)), (unsigned)n, 3), dim3(256), 0,
                       stream, a, tv);
  }
  SW_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sw_gaussian_blur_weights(float sigma, int32_t* r, uint32_t* ww, uint32_t* fw) {
  if (!(sigma > 0.f) || !r || !ww || !fw) return -1;
  // Pillow's _gaussian_blur_radius (three passes): float variables, the square root and the floor taken in double
  const float s2 = sigma * sigma / 3.0f;
  const float L = (float)sqrt(12.0 * (double)s2 + 1.0);
  const float l = (float)floor(((double)L - 1.0) / 2.0);
  float a = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * s2);
  a = a / (6.0f * (s2 - (l + 1.0f) * (l + 1.0f)));
  const float R = l + a;
  const int ri = (int)R;
  if (ri < 0 || 3 * (ri + 1) > BLUR_HALO) return -6;
  const uint32_t w = (uint32_t)((float)(1 << 24) / (R * 2 + 1));
  *r = ri; *ww = w; *fw = ((1u << 24) - (uint32_t)(2 * ri + 1) * w) / 2;
  return 0;
}

extern "C" long sw_strong_aug_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return -1;
  return ((3L * H * W + 255) & ~255L) + 256;                             // the blur's intermediate image + the L sum
}

extern "C" int sw_strong_aug_u8(int H, int W, const uint8_t* in, const sw_aug_recipe* recipe, uint8_t* out, void* workspace,
                                hipStream_t stream) {
  SW_ENTER();
  if (H <= 0 || W <= 0 || !in || !out || !recipe || !workspace || in == out) return -1;
  if (((uintptr_t)workspace & 255) != 0) return -4;
  if (recipe->blur_r >= 0 && 3 * (recipe->blur_r + 1) > BLUR_HALO) return -6;
  AugArgs a = {};
  a.one.in = in; a.one.out = out; a.one.tmp = (uint8_t*)workspace;
  a.one.lsum = (uint64_t*)((char*)workspace + ((3L * H * W + 255) & ~255L));
  a.one.H = H; a.one.W = W; a.one.recipe = *recipe;
  int stages = recipe->blur_r >= 0 ? SW_AUG_STAGE_BLUR : SW_AUG_STAGE_POINT;
  for (int s = 0; s < 4; ++s) if (recipe->order[s] == SW_AUG_CONTRAST) stages |= SW_AUG_STAGE_CONTRAST;
  return launch_strong_aug(a, 1, H, W, stages, stream);
}

extern "C" int sw_strong_aug_multi_u8(int n, const sw_aug_item* items_dev, int max_h, int max_w, int stages, hipStream_t stream) {
  SW_ENTER();
  if (n < 0 || (n > 0 && !items_dev)) return -1;
  AugArgs a = {};
  a.items = items_dev;
  return launch_strong_aug(a, n, max_h, max_w, stages, stream);
}

// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the OICR+ hot path.
// wave = 64 lanes everywhere in this tree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#define SW_F32 0
#define SW_BF16 1

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
  return __uint_as_float(((unsigned int)b) << 16);
}
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
  // plain cast: hipcc emits v_cvt_pk_bf16_f32 (RNE, NaN stays NaN)
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(unsigned short, h);
}

// two floats as one word of two bf16 (a in the low half)
__device__ __forceinline__ unsigned int pack_bf16x2(float a, float b) {
  return (unsigned)f32_to_bf16_bits(a) | ((unsigned)f32_to_bf16_bits(b) << 16);
}

// flat index of an NHWC element -> (b, y, x, c)
struct Nhwc { int b, y, x, c; };
__device__ __forceinline__ Nhwc nhwc_split(long i, int H, int W, int C) {
  Nhwc p;
  p.c = (int)(i % C); long r = i / C;
  p.x = (int)(r % W); r /= W;
  p.y = (int)(r % H); p.b = (int)(r / H);
  return p;
}

// Hash dropout: element i of a tensor is kept when dropout_uniform(splitmix64(seed) + offset, i) >= p.  The keep-mask kernel and the
// GEMM epilogues draw from this one definition, the host pre-mixes the seed with the same splitmix64.
__host__ __device__ __forceinline__ uint64_t sw_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ float dropout_uniform(uint64_t base, uint64_t i) {
  return (float)(sw_splitmix64(base + i) >> 40) * (1.0f / 16777216.0f);
}

// SGD with momentum as torch.optim.SGD rounds it (the library is built without FMA contraction): the one spelling of the update
// (`first` alone decides whether m is used: callers pass what the buffer holds, written before or not; only the GEMM epilogue,
// which requests the buffer ahead of its accumulators, passes 0 on a first step instead of loading)
struct SgdWM { float w, m; };
__device__ __forceinline__ SgdWM sgd_update(float w, float g, float m, int first, float mom, float gscale, float lr, float wd) {
  const float d = g * gscale + wd * w;
  const float mn = first ? d : mom * m + d;
  return {w - lr * mn, mn};
}
// learning rate / weight decay: kernel arguments, or (hyper_dev) two floats in device memory — a captured hipGraph of the step then
// stays valid when the schedule changes them
struct SgdHyper { float lr, wd; };
__device__ __forceinline__ SgdHyper sgd_hyper(const float* hyper_dev, float lr, float wd) {
  return {hyper_dev ? hyper_dev[0] : lr, hyper_dev ? hyper_dev[1] : wd};
}

// Several problems in one launch.  `first[0..n]` are the prefix sums of the problems' block counts; a block finds its problem and
// its index inside it.  The host fills the table with BatchTable: first[n] always holds the total, add() refuses past 2^31 - 1.
template <typename T>
__device__ __forceinline__ int batch_find(const T* first, int n, T blk, T* local) {
  int i = 0;
  while (i + 1 < n && blk >= first[i + 1]) ++i;
  *local = blk - first[i];
  return i;
}
struct BatchTable {
  int* first; int n; long blocks;
  explicit BatchTable(int* f) : first(f), n(0), blocks(0) { first[0] = 0; }
  bool add(long nb) {
    if (nb < 0 || blocks + nb > 2147483647L) return false;
    blocks += nb; first[++n] = (int)blocks;
    return true;
  }
};

template <typename T> struct Elem;
template <> struct Elem<float> {
  static constexpr int kDtype = SW_F32;
  __device__ static __forceinline__ float load(const float* p) { return *p; }
  __device__ static __forceinline__ void store(float* p, float v) { *p = v; }
  __device__ static __forceinline__ void store_nt(float* p, float v) { __builtin_nontemporal_store(v, p); }     // written once, read by a later kernel
};
template <> struct Elem<unsigned short> {   // bf16 carried as raw 16-bit words
  static constexpr int kDtype = SW_BF16;
  __device__ static __forceinline__ float load(const unsigned short* p) { return bf16_bits_to_f32(*p); }
  __device__ static __forceinline__ void store(unsigned short* p, float v) { *p = f32_to_bf16_bits(v); }
  __device__ static __forceinline__ void store_nt(unsigned short* p, float v) { __builtin_nontemporal_store(f32_to_bf16_bits(v), p); }
};

// max(v, 0) and a running maximum as torch evaluates them (F.relu = clamp_min, max_pool2d's `val > max || isnan(val)`): NaN
// propagates (fmaxf returns the other operand: a diverged activation would vanish at the first join), -0 stays -0, and a maximum
// that starts at -inf can return -inf.  For every other input the result is fmaxf's.
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float max_keep_nan(float m, float v) { return (v > m || v != v) ? v : m; }

// 16 bytes of T (float: 4 elements, bf16 bits: 8, low half of a word first) <-> float[16 / sizeof(T)]
template <typename T>
__device__ __forceinline__ void piece16_load(const T* p, float* v) {
  const u32x4 q = *(const u32x4*)p;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (sizeof(T) == 2) { v[2 * k] = bf16_bits_to_f32((unsigned short)q[k]); v[2 * k + 1] = bf16_bits_to_f32((unsigned short)(q[k] >> 16)); }
    else v[k] = __uint_as_float(q[k]);
  }
}
template <typename T>
__device__ __forceinline__ void piece16_store(T* p, const float* v) {
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = sizeof(T) == 2 ? pack_bf16x2(v[2 * k], v[2 * k + 1]) : __float_as_uint(v[k]);
  *(u32x4*)p = o;
}
// V elements of a thread: one scalar access (any alignment) or one 16-byte piece
template <typename T, int V>
__device__ __forceinline__ void elems_load(const T* p, float* v) {
  if (V == 1) v[0] = Elem<T>::load(p); else piece16_load(p, v);
}
template <typename T, int V>
__device__ __forceinline__ void elems_store(T* p, const float* v) {
  if (V == 1) Elem<T>::store(p, v[0]); else piece16_store(p, v);
}

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// max of |x| carried as IEEE bits: for non-negative floats the unsigned order is the numeric order, Inf sits above every finite
// value and NaN above Inf — a NaN / Inf anywhere survives the reduction (fmaxf drops NaN)
__device__ __forceinline__ unsigned int absbits(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }
__device__ __forceinline__ unsigned int wave_reduce_max_u32(unsigned int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, o, 64));
  return v;
}

// block-wide reductions for blockDim.x a multiple of 64 and <= 1024; red must hold >= 16 floats.
__device__ __forceinline__ float block_reduce_sum(float v, float* red) {
  v = wave_reduce_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = (lane < nw) ? red[lane] : 0.f;
  r = wave_reduce_sum(r);
  return r;
}
__device__ __forceinline__ float block_reduce_max(float v, float* red) {
  v = wave_reduce_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = (lane < nw) ? red[lane] : -3.402823466e38f;
  r = wave_reduce_max(r);
  return r;
}

// ---- loss arithmetic shared by the RPN / detector losses (detector.hip) and the refinement / focal losses (heads.hip)
// get_deltas(src, tgt) with weights (wx, wy, ww, wh) (box_regression.py:59-62), boxes as x0 y0 x1 y1
__device__ __forceinline__ void box_deltas(const float* s, const float* g, float wx, float wy, float ww, float wh, float* t) {
  const float sw = s[2] - s[0], sh = s[3] - s[1], sx = s[0] + 0.5f * sw, sy = s[1] + 0.5f * sh;
  const float tw = g[2] - g[0], th = g[3] - g[1], tx = g[0] + 0.5f * tw, ty = g[1] + 0.5f * th;
  t[0] = __fdiv_rn(wx * (tx - sx), sw);
  t[1] = __fdiv_rn(wy * (ty - sy), sh);
  t[2] = ww * logf(__fdiv_rn(tw, sw));
  t[3] = wh * logf(__fdiv_rn(th, sh));
}
// max(x, 0) - x y + log(1 + exp(-|x|))   (torch's binary_cross_entropy_with_logits)
__device__ __forceinline__ float bce_with_logits(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))); }
// One wave over a row of C logits: maximum m, se = sum exp(x - m), and the logsumexp relative to c, the multiple of 64 nearest m:
// x - c is exact in float32, so a common offset of the row costs no digits (m + log(se) at logits of 3e4 keeps 2e-3 of absolute
// precision, 1e-3 of the softmax), and a row with |m| < 32 has c = 0 and is computed without offset, bit for bit.
struct RowCe {
  float m, se, c, lse;
  __device__ __forceinline__ float ce(float xt) const { return lse - (xt - c); }     // cross-entropy against the target logit xt
};
__device__ __forceinline__ RowCe row_cross_entropy(const float* x, int C, int lane) {
  RowCe r;
  r.m = -3.402823466e38f;
  for (int j = lane; j < C; j += 64) r.m = fmaxf(r.m, x[j]);
  r.m = wave_reduce_max(r.m);
  r.se = 0.f;
  for (int j = lane; j < C; j += 64) r.se += expf(x[j] - r.m);
  r.se = wave_reduce_sum(r.se);
  r.c = 64.f * rintf(r.m * 0.015625f);
  r.lse = (r.m - r.c) + logf(r.se);
  return r;
}

// LDS-DMA (buffer_load_dwordx4 ... lds: 16 bytes per lane from a buffer resource straight into LDS at m0 + 16 * lane) issued through
// inline assembly.  Through the builtin (__builtin_amdgcn_raw_ptr_buffer_load_lds) hipcc's waitcnt pass knows an LDS write is in flight, and
// in front of the next ds_read_b64_tr_b16 — the transposed-read intrinsic carries no alias information — it puts s_waitcnt vmcnt(0): a
// kernel that prefetches K-tiles and reads fragments transposed then waits for the DMA it has just issued (found in round 6: the direct
// conv weight gradient spent 52 % of its wave cycles parked there; the fc6 weight-gradient GEMM, K-strided B operand, had the same wait in
// phases 0 and 1 of every K-tile).  The kernels order DMA -> read themselves (counted vmcnt + barrier), so nothing is lost.
// (m0: written here, no other user in these kernels — no builtin LDS-DMA left beside it, no GWS, no movrel.)
typedef __attribute__((ext_vector_type(4))) int sw_i32x4;
__device__ __forceinline__ sw_i32x4 sw_make_rsrc(const void* base, unsigned bytes) {
  const unsigned long long b = (unsigned long long)base;
  return sw_i32x4{(int)(unsigned)b, (int)(unsigned)((b >> 32) & 0xFFFFu), (int)bytes, 0x00020000};
}
__device__ __forceinline__ void sw_dma16(const sw_i32x4 rsrc, const char* lds_dst, unsigned voff, unsigned soff) {
  const unsigned m = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)lds_dst;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(m), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}

// compute units of the current device (256 if the query fails), looked up once per device
inline int sw_cu_count() {
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (!n) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// hipGetLastError() is a per-thread sticky value: a recoverable error of an unrelated earlier HIP call (e.g. torch probing a
// device) would otherwise be reported by the first SW_CHECK_LAUNCH of this library.  Every entry point starts clean.
#define SW_ENTER() (void)hipGetLastError()

// ---- host side of the elementwise launches
// workgroups of `block` threads for a grid-stride loop over n elements, at most `cap`
inline int grid_for(long n, long cap = 2048, int block = 256) {
  const long g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
// f(T()) with T the element type of dtype, then the launch status; -1 for an unknown dtype
template <typename F>
inline int dispatch_elem(int dtype, F&& f) {
  if (dtype == SW_BF16) f((unsigned short)0);
  else if (dtype == SW_F32) f(0.f);
  else return -1;
  return (int)hipGetLastError();
}
// do the 16-byte forms apply: a run of C elements of T is whole 16-byte pieces and every pointer is 16-byte aligned
template <typename T, typename... P>
inline bool vec16_ok(long C, const P*... ptrs) {
  return (C * (long)sizeof(T)) % 16 == 0 && (((uintptr_t)ptrs | ...) & 15) == 0;
}
#define SW_CHECK_LAUNCH()                         \
  do {                                            \
    hipError_t e__ = hipGetLastError();           \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

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
#define SW_CHECK_LAUNCH()                         \
  do {                                            \
    hipError_t e__ = hipGetLastError();           \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

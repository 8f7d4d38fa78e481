// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the OICR+ hot path.
// wave = 64 lanes everywhere in this tree.
// In order: bf16 / NHWC / dropout / SGD / batched-launch helpers, element and 16-byte access, wave and workgroup reductions, then the
// labelled sections: index arithmetic (workgroup scan, sort keys, bitonic sort), float32 box arithmetic (area, IoU, clip, decode),
// loss arithmetic, LDS-DMA, and the host side of the launches.
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

// ---- index arithmetic shared by the kernels that select, sort, compact and match (heads.hip, proposals.hip, evaluation.hip,
// elementwise.hip)
// Inclusive scan over the workgroup's blockDim.x threads (Hillis-Steele in LDS, two barriers per step; any blockDim.x <= the
// length of buf; a kernel that is only ever launched with one block size names it as THREADS, which lets the compiler unroll the
// steps as it did for the literal bounds the sites used to spell — 0 = read blockDim.x), in thread order, or with REVERSE from the last thread to the first (a suffix scan).  op(earlier, later) need
// only be associative.  Every thread of the workgroup calls it.  Returns
//   incl   op over the threads up to and including this one,
//   prev   the incl of the thread before this one in scan order — the exclusive value, for operators without an inverse;
//          this thread's own incl at the first thread, which has none before it,
//   total  the incl of the last thread in scan order.
// It begins by writing buf and ends in a barrier after its last read: on return buf is free, and a call site needs no barrier of
// its own for it, neither before the next call on the same buf nor before any other use.  (Fields a caller leaves unread cost
// nothing: the helper is inlined and their LDS reads go.)
template <typename T> struct BlockScan { T incl, prev, total; };
template <int THREADS = 0, bool REVERSE = false, typename T, typename Op>
__device__ __forceinline__ BlockScan<T> block_scan(T v, T* buf, Op op) {
  const int n = THREADS ? THREADS : (int)blockDim.x, rank = REVERSE ? n - 1 - (int)threadIdx.x : (int)threadIdx.x;   // this thread's place in scan order
  auto at = [&](int r) -> T& { return buf[REVERSE ? n - 1 - r : r]; };                      // buf is indexed by thread
  at(rank) = v;
  __syncthreads();
  for (int off = 1; off < n; off <<= 1) {
    const bool has = rank >= off;
    const T o = at(has ? rank - off : rank);
    __syncthreads();
    if (has) {
      v = op(o, v);
      at(rank) = v;
    }
    __syncthreads();
  }
  BlockScan<T> r;
  r.incl = v;
  r.prev = at(rank > 0 ? rank - 1 : rank);
  r.total = at(n - 1);
  __syncthreads();
  return r;
}
struct ScanAdd {
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// Order-preserving map of a float onto unsigned bits (ascending unsigned order == ascending float order by bits: -NaN < -inf < ..
// < -0.0 < +0.0 < .. < +inf < +NaN) and its inverse
__device__ __forceinline__ unsigned int orderable(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_orderable(unsigned int o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
// ascending sort of this key == descending score, ascending index (the oracle's tie rule)
__device__ __forceinline__ unsigned long long make_key(float score, unsigned int idx) {
  return ((unsigned long long)(~orderable(score)) << 32) | idx;
}
// a make_key key taken apart: its index, and its score bit for bit
__device__ __forceinline__ int key_index(unsigned long long key) { return (int)(unsigned int)(key & 0xFFFFFFFFu); }
__device__ __forceinline__ float key_score(unsigned long long key) { return from_orderable(~(unsigned int)(key >> 32)); }

// Ascending bitonic sort of N 64-bit keys by one workgroup.  Requires: N a power of two, blockDim.x a multiple of 64, every thread
// of the workgroup calls it, and the keys are written and a barrier passed before the call.  It ends in a barrier: on return every
// thread may read any key.  An ascending sort of a fixed multiset of words has one result, whatever the order of the passes.
// WAVE_LOCAL (keys in LDS only): a pass whose partner distance j is < 128 stays inside one aligned block of 128 keys.  A wave owns
// such a block (lane = the pair whose lower index has bit j clear) and runs all the remaining passes of the stage on it back to
// back: the LDS serves one wave's requests in issue order, so those passes need no workgroup barrier — 2048 keys take 14
// barriers instead of 66 (the mining kernel sorts one score column per image-level class on the step's critical path).
// (Holding the block in registers and exchanging by __shfl_xor was slower — four ds_bpermute per pass — and so was giving a thread
// four independent pairs per pass: a pass costs ~0.2 us of issue + LDS round trip either way; in-kernel stamps at R = 2000, G = 2:
// column sorts 27 us, threshold + keys 2, NMS sort 7, NMS 12, labels 6.)
// nseg > 1: nseg independent arrays of N keys back to back, all sorted ascending by the same passes (the passes are latency bound,
// so several score columns sort in the time of one).
template <bool WAVE_LOCAL>
__device__ void bitonic_sort(unsigned long long* keys, int N, int nseg = 1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int T = N * nseg;
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (WAVE_LOCAL && j < 128) {
        for (int base = wave * 128; base < T; base += nwaves * 128) {
          for (int jj = j; jj > 0; jj >>= 1) {
            const int i = base + (((lane & ~(jj - 1)) << 1) | (lane & (jj - 1))), p = i | jj;
            if (p < T) {
              const unsigned long long a = keys[i], b = keys[p];
              const bool asc = ((i & (N - 1)) & k) == 0;
              if ((a > b) == asc) { keys[i] = b; keys[p] = a; }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
        }
        __syncthreads();
        break;
      }
      for (int i = threadIdx.x; i < T; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keys[i], b = keys[ixj];
          const bool asc = ((i & (N - 1)) & k) == 0;
          if ((a > b) == asc) { keys[i] = b; keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
}
// smallest power of two >= n, at least 64 (a wave): the length a list of n keys is padded to for bitonic_sort, on both sides of a launch
__host__ __device__ __forceinline__ int next_pow2(int n) { int p = 64; while (p < n) p <<= 1; return p; }

// ---- float32 box arithmetic of the index side (heads.hip, proposals.hip, proposal_ar.hip): boxes as x0 y0 x1 y1, a float4 by value
// (a caller whose pointer is not known to be 16-byte aligned builds it from four scalar loads); every operation rounds on its own,
// in the reference's order (the library is built without FMA contraction)
__device__ __forceinline__ float box_area(float4 b) { return __fmul_rn(b.z - b.x, b.w - b.y); }
// detectron2 pairwise_iou (structures/boxes.py:322-370), one pair: 0 where inter <= 0.  A NaN width or height of the intersection
// counts as 0 (fmaxf drops it), so a NaN coordinate gives 0 unless it reaches an area: then the union, and the result, is NaN.
// area_a / area_b: box_area of a and b (a caller that holds one box against many hoists its area)
__device__ __forceinline__ float pairwise_iou(float4 a, float area_a, float4 b, float area_b) {
  const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = __fmul_rn(w, h);
  return inter > 0.f ? __fdiv_rn(inter, __fadd_rn(area_a, area_b) - inter) : 0.f;
}
__device__ __forceinline__ float pairwise_iou(float4 a, float4 b) { return pairwise_iou(a, box_area(a), b, box_area(b)); }
// torchvision nms IoU: inter / (a_i + a_j - inter), inter = max(0,dx)*max(0,dy)
__device__ __forceinline__ float iou_nms(float4 a, float4 b) {
  const float w = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
  const float h = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
  const float inter = __fmul_rn(w, h);
  return __fdiv_rn(inter, __fadd_rn(box_area(a), box_area(b)) - inter);
}
// iou_nms(a, b) > thresh for thresh >= 0, without the division for disjoint boxes: inter == 0 gives 0 / union = 0 (or 0 / 0 = NaN for
// two empty boxes), never > thresh — most pairs of a 2000-candidate list are disjoint
__device__ __forceinline__ bool iou_nms_above(float4 a, float4 b, float thresh) {
  const float w = fminf(a.z, b.z) - fmaxf(a.x, b.x);
  const float h = fminf(a.w, b.w) - fmaxf(a.y, b.y);
  if (!(w > 0.f && h > 0.f)) return false;
  const float inter = __fmul_rn(w, h);
  return __fdiv_rn(inter, __fadd_rn(box_area(a), box_area(b)) - inter) > thresh;
}
// one coordinate clipped to [0, hi] (Boxes.clip); a NaN becomes 0 (fmaxf drops it)
__device__ __forceinline__ float clip(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }
// Box2BoxTransform.apply_deltas (box_regression.py:73-116) against one anchor / proposal box.  dx dy dw dh are the deltas AFTER the
// caller has divided them by the weights and clamped dw, dh at scale_clamp: the callers differ in that clamp (see there).
__device__ __forceinline__ float4 decode_box(float4 an, float dx, float dy, float dw, float dh) {
  const float w = an.z - an.x, h = an.w - an.y;
  const float cx = an.x + __fmul_rn(0.5f, w), cy = an.y + __fmul_rn(0.5f, h);
  const float px = __fadd_rn(__fmul_rn(dx, w), cx), py = __fadd_rn(__fmul_rn(dy, h), cy);
  const float pw = __fmul_rn(expf(dw), w), ph = __fmul_rn(expf(dh), h);
  return make_float4(px - __fmul_rn(0.5f, pw), py - __fmul_rn(0.5f, ph), px + __fmul_rn(0.5f, pw), py + __fmul_rn(0.5f, ph));
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

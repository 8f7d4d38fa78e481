// Box-proposal AR (reference detectron2/detectron2/evaluation/coco_evaluation.py: the per-image loop of _evaluate_box_proposals
// :482-514 with structures/boxes.py pairwise_iou :322-368): one-to-one greedy coverage of the ground-truth boxes of an image by
// its ranked proposals, for every (limit, area range) of a split in one launch, and the boxes covered at every IoU threshold.
//
// The reference builds the P x G IoU matrix and runs min(P', G') rounds of `overlaps.max(dim=0)` / `max_overlaps.max(dim=0)` over
// the whole matrix, eight times over the split.  A round takes the pair that is best under (largest IoU, smallest box index,
// smallest proposal index) among pairs whose proposal and box are both unused, so it is enough to keep, per box, its best unused
// proposal: a round is one reduction over the boxes, and only the boxes whose best proposal was the one just taken are scanned
// again.  No matrix is stored; an IoU is recomputed from the boxes whenever it is needed.
//
// Layout: a workgroup is 4 waves and owns one image at a time (the workgroups stride over the images).  The image's ranked
// proposals are staged in LDS once, as many as the largest limit asks for and at most kLdsProps; an item with a smaller limit reads
// a prefix.  The waves take the image's (limit, area range) items round-robin; a wave keeps its item's state — the valid boxes, each
// one's best unused proposal as (IoU, rank), and the used-proposal bitmask — in its own LDS slice.  An item with more than kLdsProps
// proposals or more than kLdsGt valid boxes runs the same code (run_item) with the proposals read from global memory and the state
// in the wave's slot of the caller's workspace.
//
// Who touches what: box k's (IoU, rank) is read and written by lane k & 63 only, and the used bit of proposal p lives in a word that
// only lane p & 63 reads or writes (word (p >> 11) * 64 + (p & 63), bit (p >> 6) & 31), so neither needs a fence; the valid boxes
// are written once by whichever lane found them and read by all, behind one fence.
//
// Arithmetic: the reference's float32 operations in its order (the library builds with -ffp-contract=off), the compiler's default
// correctly rounded division, no fast-math intrinsics.  The counts are integers: each lane t < n_thr counts its threshold in a
// register, the waves add them per workgroup in LDS and the workgroups add them to the table with 64-bit atomics, so the result does
// not depend on the order and two launches are bit-identical.
#include "common.h"
#include "soswsod_hip.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kLdsProps = SW_BOXAR_LDS_BOXES;
constexpr int kLdsGt = SW_BOXAR_LDS_GT;
constexpr int kMaxArea = SW_BOXAR_MAX_AREAS;
constexpr int kMaxLim = SW_BOXAR_MAX_LIMITS;
constexpr int kMaxThr = SW_BOXAR_MAX_THRESHOLDS;
constexpr int kLdsUsedWords = 64 * ((kLdsProps / 64 + 31) / 32);

struct Params {
  float area_rng[kMaxArea][2];
  int32_t limits[kMaxLim];
  float thr[kMaxThr];
  int n_area, n_lim, n_thr;
};

// a (proposal, box) pair and its IoU; j < 0: none
struct Cand {
  float v;
  int k, j;
};

// THE comparator of every scan, reduction and merge: does b replace a as the better pair?  Largest IoU, then the smallest box
// index, then the smallest proposal index
__device__ __forceinline__ bool replaces(const Cand& a, const Cand& b) {
  if (b.j < 0) return false;
  if (a.j < 0) return true;
  if (b.v != a.v) return b.v > a.v;
  if (b.k != a.k) return b.k < a.k;
  return b.j < a.j;
}

__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Cand d;
    d.v = __shfl_xor(c.v, o, 64);
    d.k = __shfl_xor(c.k, o, 64);
    d.j = __shfl_xor(c.j, o, 64);
    if (replaces(c, d)) c = d;
  }
  return c;
}

// the words of the used-proposal bitmask of n proposals (64 lanes x one word per 32 strides)
__host__ __device__ inline long long used_words(long long n) { return 64 * (((n + 63) / 64 + 31) / 32); }
__host__ __device__ inline long long slot_bytes(long long boxes, long long props) {
  return (24 * boxes + 4 * used_words(props) + 15) / 16 * 16;
}

// box k's best unused proposal among the first np (every lane returns it)
__device__ __forceinline__ Cand scan_box(const float4* prop, int np, const float4* gbox, const uint32_t* used, int k, int lane) {
  const float4 g = gbox[k];
  const float ga = box_area(g);
  Cand best = {0.f, k, -1};
  uint32_t uw = 0;
  for (int p = lane, i = 0; p < np; p += 64, ++i) {
    if ((i & 31) == 0) uw = used[(i >> 5) * 64 + lane];
    if ((uw >> (i & 31)) & 1u) continue;
    const Cand c = {pairwise_iou(prop[p], box_area(prop[p]), g, ga), k, p};     // boxes.py:322-368 in float32, g's area hoisted
    if (replaces(best, c)) best = c;
  }
  return wave_best(best);
}

// One item: the first np ranked proposals (np >= 1) against the ng_valid >= 1 boxes of the image whose area lies in [lo, hi].
// gbox / bv / bj hold ng_valid entries, used holds used_words(np) words.  Returns this lane's count for its threshold.
__device__ __forceinline__ unsigned long long run_item(const float4* prop, int np, float4* gbox, float* bv, int* bj,
                                                       uint32_t* used, const float4* ggt, const float* garea, int ng, float lo,
                                                       float hi, int ng_valid, bool counts, float my_thr, float* overlap,
                                                       int32_t* match_gt, int32_t* match_box, int lane) {
  // the valid boxes, in file order
  int base = 0;
  for (int c0 = 0; c0 < ng; c0 += 64) {
    const int g = c0 + lane;
    float a = 0.f;
    if (g < ng) a = garea[g];
    const bool valid = g < ng && a >= lo && a <= hi;
    const unsigned long long m = __ballot(valid);
    if (valid) gbox[base + __popcll(m & ((1ull << lane) - 1ull))] = ggt[g];
    base += __popcll(m);
  }
  const int nw = (int)used_words(np);
  for (int w = lane; w < nw; w += 64) used[w] = 0;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          // gbox is read by every lane
  __builtin_amdgcn_wave_barrier();

  for (int k = 0; k < ng_valid; ++k) {
    const Cand c = scan_box(prop, np, gbox, used, k, lane);
    if ((k & 63) == lane) {
      bv[k] = c.v;
      bj[k] = c.j;
    }
  }

  unsigned long long cnt = 0;
  const int rounds = np < ng_valid ? np : ng_valid;
  for (int r = 0; r < rounds; ++r) {
    Cand best = {0.f, 0, -1};
    for (int k = lane; k < ng_valid; k += 64) {
      const Cand c = {bv[k], k, bj[k]};
      if (replaces(best, c)) best = c;
    }
    best = wave_best(best);
    if (lane == 0) {
      overlap[r] = best.v;
      match_gt[r] = best.k;
      match_box[r] = best.j;
    }
    if (counts && best.v >= my_thr) ++cnt;
    if ((best.k & 63) == lane) bj[best.k] = -1;
    if ((best.j & 63) == lane) {
      const int i = best.j >> 6;
      used[(i >> 5) * 64 + lane] |= 1u << (i & 31);
    }
    if (r + 1 == rounds) break;                                   // nothing is read after the last round
    for (int c0 = 0; c0 < ng_valid; c0 += 64) {
      const int k = c0 + lane;
      unsigned long long m = __ballot(k < ng_valid && bj[k] == best.j);
      while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const Cand c = scan_box(prop, np, gbox, used, c0 + b, lane);
        if (lane == b) {
          bv[c0 + b] = c.v;
          bj[c0 + b] = c.j;
        }
      }
    }
  }
  // boxes no round reached: "_gt_overlaps = torch.zeros(len(gt_boxes))"
  for (int e = rounds + lane; e < ng_valid; e += 64) {
    overlap[e] = 0.f;
    match_gt[e] = -1;
    match_box[e] = -1;
  }
  if (counts && 0.f >= my_thr) cnt += (unsigned long long)(ng_valid - rounds);
  return cnt;
}

__global__ void __launch_bounds__(kThreads) box_proposal_ar_kernel(
    int n_img, const int64_t* __restrict__ prop_off, const float4* __restrict__ prop_box, long long n_prop,
    const int64_t* __restrict__ gt_off, const float4* __restrict__ gt_box, const float* __restrict__ gt_area, long long n_gt,
    const Params prm, const int64_t* __restrict__ item_off, long long n_out, float* overlap, int32_t* match_gt, int32_t* match_box,
    unsigned long long* cnt_yes, char* workspace, long long ws_boxes, long long ws_props, int32_t* status) {
  __shared__ float4 s_prop[kLdsProps];
  __shared__ float4 s_gbox[kWaves][kLdsGt];
  __shared__ float s_bv[kWaves][kLdsGt];
  __shared__ int s_bj[kWaves][kLdsGt];
  __shared__ uint32_t s_used[kWaves][kLdsUsedWords];
  __shared__ unsigned long long s_cnt[kMaxLim * kMaxArea * kMaxThr];
  __shared__ float s_rng[kMaxArea][2];
  __shared__ float s_thr[kMaxThr];
  __shared__ int s_lim[kMaxLim];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A = prm.n_area, L = prm.n_lim, T = prm.n_thr;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kMaxArea; ++i) {
      s_rng[i][0] = prm.area_rng[i][0];
      s_rng[i][1] = prm.area_rng[i][1];
    }
#pragma unroll
    for (int i = 0; i < kMaxLim; ++i) s_lim[i] = prm.limits[i];
#pragma unroll
    for (int i = 0; i < kMaxThr; ++i) s_thr[i] = prm.thr[i];
  }
  for (int i = threadIdx.x; i < L * A * T; i += kThreads) s_cnt[i] = 0;
  __syncthreads();
  const bool counts = lane < T;
  const float my_thr = counts ? s_thr[lane] : 0.f;

  for (int img = blockIdx.x; img < n_img; img += gridDim.x) {
    // everything up to the staging is the same for the whole workgroup: no barrier is skipped by a part of it
    const int64_t p0 = prop_off[img], p1 = prop_off[img + 1], g0 = gt_off[img], g1 = gt_off[img + 1];
    if (p0 < 0 || p1 < p0 || p1 > n_prop || g0 < 0 || g1 < g0 || g1 > n_gt || p1 - p0 > 0x7fffffffLL || g1 - g0 > 0x7fffffffLL) {
      if (threadIdx.x == 0) *status = SW_BOXAR_BAD_OFFSETS;
      continue;
    }
    const int np_all = (int)(p1 - p0), ng = (int)(g1 - g0);
    if (np_all == 0 || ng == 0) continue;                         // coco_evaluation.py:479: skipped before num_pos is counted
    int n_need = 0;
    for (int l = 0; l < L; ++l) {
      const int lim = s_lim[l];
      const int n = lim > 0 && lim < np_all ? lim : np_all;
      n_need = n > n_need ? n : n_need;
    }
    const int n_stage = n_need < kLdsProps ? n_need : kLdsProps;
    const float4* gprop = prop_box + p0;
    const float4* ggt = gt_box + g0;
    const float* garea = gt_area + g0;
    __syncthreads();                                              // the previous image has been read
    for (int i = threadIdx.x; i < n_stage; i += kThreads) s_prop[i] = gprop[i];
    __syncthreads();

    for (int it = wave; it < L * A; it += kWaves) {
      const int l = it / A, a = it - l * A;
      const float lo = s_rng[a][0], hi = s_rng[a][1];
      int ng_valid = 0;
      for (int c0 = 0; c0 < ng; c0 += 64) {
        const int g = c0 + lane;
        float ar = 0.f;
        if (g < ng) ar = garea[g];
        ng_valid += __popcll(__ballot(g < ng && ar >= lo && ar <= hi));
      }
      const int64_t item = (int64_t)it * n_img + img;
      const int64_t o0 = item_off[item], o1 = item_off[item + 1];
      if (o0 < 0 || o1 > n_out || o1 - o0 != ng_valid) {          // not the layout of this split: refused, never written
        if (lane == 0) *status = SW_BOXAR_BAD_LAYOUT;
        continue;
      }
      if (ng_valid == 0) continue;
      const int lim = s_lim[l];
      const int np = lim > 0 && lim < np_all ? lim : np_all;
      unsigned long long cnt;
      if (np <= kLdsProps && ng_valid <= kLdsGt) {
        cnt = run_item(s_prop, np, s_gbox[wave], s_bv[wave], s_bj[wave], s_used[wave], ggt, garea, ng, lo, hi, ng_valid, counts,
                       my_thr, overlap + o0, match_gt + o0, match_box + o0, lane);
      } else {
        if (workspace == nullptr || ng_valid > ws_boxes || np > ws_props) {
          if (lane == 0) *status = SW_BOXAR_WORKSPACE;
          continue;
        }
        char* slot = workspace + ((long long)blockIdx.x * kWaves + wave) * slot_bytes(ws_boxes, ws_props);
        float4* w_gbox = reinterpret_cast<float4*>(slot);
        float* w_bv = reinterpret_cast<float*>(slot + 16 * ws_boxes);
        int* w_bj = reinterpret_cast<int*>(slot + 20 * ws_boxes);
        uint32_t* w_used = reinterpret_cast<uint32_t*>(slot + 24 * ws_boxes);
        cnt = run_item(gprop, np, w_gbox, w_bv, w_bj, w_used, ggt, garea, ng, lo, hi, ng_valid, counts, my_thr, overlap + o0,
                       match_gt + o0, match_box + o0, lane);
      }
      if (counts && cnt) atomicAdd(&s_cnt[it * T + lane], cnt);
    }
  }

  __syncthreads();
  for (int i = threadIdx.x; i < L * A * T; i += kThreads)
    if (s_cnt[i]) atomicAdd(cnt_yes + i, s_cnt[i]);
}

int grid_of(int n_img) { return n_img < 8 * sw_cu_count() ? n_img : 8 * sw_cu_count(); }

}  // namespace

extern "C" long long sw_box_proposal_ar_workspace_bytes(int n_img, long long max_boxes, long long max_props) {
  if (n_img < 0 || max_boxes < 0 || max_props < 0) return -1;
  if (n_img == 0 || (max_boxes <= kLdsGt && max_props <= kLdsProps)) return 0;
  return (long long)grid_of(n_img) * kWaves * slot_bytes(max_boxes, max_props);
}

extern "C" int sw_box_proposal_ar(int n_img, const int64_t* prop_off, const float* prop_box, long long n_prop, const int64_t* gt_off,
                                  const float* gt_box, const float* gt_area, long long n_gt, int n_area, const float* area_rng,
                                  int n_lim, const int32_t* limits, int n_thr, const float* thr, const int64_t* item_off,
                                  long long n_item_off, long long n_out, float* overlap, int32_t* match_gt, int32_t* match_box,
                                  long long* cnt_yes, void* workspace, long long ws_bytes, long long ws_boxes, long long ws_props,
                                  int32_t* status, hipStream_t stream) {
  SW_ENTER();
  if (n_img < 0 || n_prop < 0 || n_gt < 0 || n_out < 0) return -5;
  if (n_area < 1 || n_area > kMaxArea || n_lim < 1 || n_lim > kMaxLim || n_thr < 1 || n_thr > kMaxThr) return -6;
  if (area_rng == nullptr || limits == nullptr || thr == nullptr || status == nullptr) return -1;
  for (int l = 0; l < n_lim; ++l)
    if (limits[l] < 0) return -6;
  if (n_item_off != (long long)n_lim * n_area * n_img + 1) return -6;
  if (((uintptr_t)prop_box & 15) != 0 || ((uintptr_t)gt_box & 15) != 0 || ((uintptr_t)cnt_yes & 7) != 0 ||
      ((uintptr_t)workspace & 15) != 0)
    return -4;
  if (ws_boxes < 0 || ws_props < 0 || ws_bytes < 0) return -5;
  if (workspace != nullptr && ws_bytes < sw_box_proposal_ar_workspace_bytes(n_img, ws_boxes, ws_props)) return -7;
  Params prm = {};
  for (int a = 0; a < n_area; ++a) {
    prm.area_rng[a][0] = area_rng[2 * a];
    prm.area_rng[a][1] = area_rng[2 * a + 1];
  }
  for (int l = 0; l < n_lim; ++l) prm.limits[l] = limits[l];
  for (int t = 0; t < n_thr; ++t) prm.thr[t] = thr[t];
  prm.n_area = n_area;
  prm.n_lim = n_lim;
  prm.n_thr = n_thr;
  hipError_t e = hipMemsetAsync(cnt_yes, 0, (size_t)n_lim * n_area * n_thr * sizeof(long long), stream);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(status, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return (int)e;
  if (n_img == 0) return 0;
  if (workspace == nullptr) ws_boxes = ws_props = 0;
  hipLaunchKernelGGL(box_proposal_ar_kernel, dim3(grid_of(n_img)), dim3(kThreads), 0, stream, n_img, prop_off,
                     reinterpret_cast<const float4*>(prop_box), n_prop, gt_off, reinterpret_cast<const float4*>(gt_box), gt_area, n_gt,
                     prm, item_off, n_out, overlap, match_gt, match_box, reinterpret_cast<unsigned long long*>(cnt_yes),
                     static_cast<char*>(workspace), ws_boxes, ws_props, status);
  SW_CHECK_LAUNCH();
  return 0;
}

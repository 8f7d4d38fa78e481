// Proposal recall (reference uwsod/projects/WSL/tools/proposal_recall.py: the overlap block :204-225 of recall_mcg, the same lines
// in recall_ss :277-297 and recall_eb :356-376): the best overlap of every ground-truth box with the first cuts[c] proposals of its
// image, for every cut at once, and the boxes recalled at every IoU threshold.
//
// The reference runs its whole loop once per budget; the budgets are nested prefixes of one ranked list, so one pass that keeps the
// best overlap per SEGMENT [cuts[c - 1], cuts[c]) and then takes a running best over the segments gives every row.
//
// Layout: a workgroup is 4 waves and owns one image at a time (the workgroups stride over the images).  The image's proposals are
// staged in LDS in chunks of kChunk boxes, each with its area; the waves take the image's ground-truth boxes round-robin; the lanes
// of a wave stride over one segment's part of the chunk and keep the best value and its first index; a wave reduction picks the
// segment's best, and lane 0 merges it with what earlier chunks left for that segment — kept in the output row itself, which the
// same lane wrote (a segment spans chunks only beyond kChunk ranks).  After the last chunk lane 0 takes the prefix over the
// segments and writes the row; lanes 0..n_thr-1 count it.  The counts are integers: they are summed per workgroup in LDS and added
// to the table with atomics, so the result does not depend on the order.
//
// Arithmetic: the reference's f64 operations in its order (the library builds with -ffp-contract=off, so no product is fused into a
// sum), IEEE division, no fast-math intrinsics.  np.max / np.argmax semantics: a NaN in the prefix wins, the first one gives the
// index; otherwise the largest value, the first of equals.  +0.0 and -0.0 are equals: ovmax is the overlap AT jmax, sign included
// (np.max itself gives either sign for a prefix that holds both, depending on how the host's vector unit folds it).
#include "common.h"
#include "soswsod_hip.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kChunk = SW_PROPOSAL_RECALL_LDS_BOXES;
constexpr int kMaxCut = SW_PROPOSAL_RECALL_MAX_CUTS;
constexpr int kMaxThr = SW_PROPOSAL_RECALL_MAX_THRESHOLDS;

// does (bv, bj) replace (av, aj) as the np.max / np.argmax of their union?  j < 0: empty
__device__ __forceinline__ bool replaces(double av, int aj, double bv, int bj) {
  if (bj < 0) return false;
  if (aj < 0) return true;
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return bn && (!an || bj < aj);
  return bv > av || (bv == av && bj < aj);
}

__global__ void __launch_bounds__(kThreads) proposal_recall_kernel(
    int n_img, const int64_t* __restrict__ prop_off, const double* __restrict__ prop_box, const int64_t* __restrict__ gt_off,
    const double* __restrict__ gt_box, int n_cut, const int32_t* __restrict__ cuts, int n_thr, const double* __restrict__ thr,
    double* ovmax, int32_t* jmax, long long* __restrict__ cnt_yes) {
  __shared__ double2 s_box[kChunk][2];          // [xmin, ymin] [xmax, ymax]
  __shared__ double s_area[kChunk];
  __shared__ double s_thr[kMaxThr];
  __shared__ int s_cut[kMaxCut];
  __shared__ unsigned long long s_cnt[kMaxCut * kMaxThr];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < n_cut) s_cut[threadIdx.x] = cuts[threadIdx.x];
  if (threadIdx.x < n_thr) s_thr[threadIdx.x] = thr[threadIdx.x];
  if (threadIdx.x < n_cut * n_thr) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int last_cut = s_cut[n_cut - 1];

  for (int img = blockIdx.x; img < n_img; img += gridDim.x) {
    const int64_t g0 = gt_off[img];
    const int ng = (int)(gt_off[img + 1] - g0);
    if (ng == 0) continue;                      // the same for the whole workgroup: no barrier is skipped by a part of it
    const int64_t p0 = prop_off[img];
    const int64_t np_all = prop_off[img + 1] - p0;
    const int n = np_all < (int64_t)last_cut ? (int)np_all : last_cut;       // ranks beyond the largest cut are never read
    const double2* gprop = reinterpret_cast<const double2*>(prop_box) + 2 * p0;
    const double2* ggt = reinterpret_cast<const double2*>(gt_box) + 2 * g0;

    for (int c0 = 0; c0 < n; c0 += kChunk) {
      const int cn = n - c0 < kChunk ? n - c0 : kChunk;
      __syncthreads();                          // the previous chunk (or image) has been read
      for (int i = threadIdx.x; i < cn; i += kThreads) {
        const double2 lo = gprop[2 * (c0 + i)], hi = gprop[2 * (c0 + i) + 1];
        s_box[i][0] = lo;
        s_box[i][1] = hi;
        s_area[i] = (hi.x - lo.x + 1.0) * (hi.y - lo.y + 1.0);
      }
      __syncthreads();

      for (int g = wave; g < ng; g += kWaves) {
        const double2 glo = ggt[2 * g], ghi = ggt[2 * g + 1];
        const double gt_area = (ghi.x - glo.x + 1.0) * (ghi.y - glo.y + 1.0);
        const int64_t row = (g0 + g) * n_cut;
        for (int s = 0; s < n_cut; ++s) {
          const int seg_lo = s ? s_cut[s - 1] : 0;
          const int lo = seg_lo > c0 ? seg_lo : c0;
          const int hi = s_cut[s] < c0 + cn ? s_cut[s] : c0 + cn;
          if (lo >= hi) continue;               // the same for the whole wave
          double bv = 0.0;
          int bj = -1;
          for (int i = lo + lane; i < hi; i += 64) {
            const double2 plo = s_box[i - c0][0], phi = s_box[i - c0][1];
            const double ixmin = plo.x > glo.x ? plo.x : glo.x;
            const double iymin = plo.y > glo.y ? plo.y : glo.y;
            const double ixmax = phi.x < ghi.x ? phi.x : ghi.x;
            const double iymax = phi.y < ghi.y ? phi.y : ghi.y;
            const double tw = ixmax - ixmin + 1.0, th = iymax - iymin + 1.0;
            const double iw = tw > 0.0 ? tw : 0.0;
            const double ih = th > 0.0 ? th : 0.0;
            const double inters = iw * ih;
            const double uni = gt_area + s_area[i - c0] - inters;
            const double ov = inters / uni;
            if (bj < 0 || (bv == bv && (ov != ov || ov > bv))) {             // i rises: an equal value never replaces
              bv = ov;
              bj = i;
            }
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (replaces(bv, bj, ov, oj)) {
              bv = ov;
              bj = oj;
            }
          }
          if (lane == 0) {
            if (seg_lo < c0) {                  // the segment began in an earlier chunk: lower indices, so they keep a tie
              const double ev = ovmax[row + s];
              const int ej = jmax[row + s];
              if (!replaces(ev, ej, bv, bj)) {
                bv = ev;
                bj = ej;
              }
            }
            ovmax[row + s] = bv;
            jmax[row + s] = bj;
          }
        }
      }
    }

    // running best over the segments; a segment that holds no proposal was never written
    for (int g = wave; g < ng; g += kWaves) {
      const int64_t row = (g0 + g) * n_cut;
      double rv = __builtin_nan("");
      int rj = -1;
      for (int s = 0; s < n_cut; ++s) {
        if (lane == 0) {
          const int seg_lo = s ? s_cut[s - 1] : 0;
          if (seg_lo < n) {
            const double sv = ovmax[row + s];
            const int sj = jmax[row + s];
            if (replaces(rv, rj, sv, sj)) {
              rv = sv;
              rj = sj;
            }
          }
          ovmax[row + s] = rv;
          jmax[row + s] = rj;
        }
        const double v = __shfl(rv, 0, 64);
        if (lane < n_thr && v >= s_thr[lane]) atomicAdd(&s_cnt[s * n_thr + lane], 1ull);
      }
    }
  }

  __syncthreads();
  if (threadIdx.x < n_cut * n_thr && s_cnt[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long*>(cnt_yes) + threadIdx.x, s_cnt[threadIdx.x]);
}

}  // namespace

extern "C" int sw_proposal_recall(int n_img, const int64_t* prop_off, const double* prop_box, const int64_t* gt_off,
                                  const double* gt_box, int n_cut, const int32_t* cuts, int n_thr, const double* thr, double* ovmax,
                                  int32_t* jmax, long long* cnt_yes, hipStream_t stream) {
  SW_ENTER();
  if (n_img < 0) return -5;
  if (n_cut < 1 || n_cut > kMaxCut || n_thr < 1 || n_thr > kMaxThr) return -6;
  if (((uintptr_t)prop_box & 15) != 0 || ((uintptr_t)gt_box & 15) != 0 || ((uintptr_t)cnt_yes & 7) != 0 ||
      ((uintptr_t)ovmax & 7) != 0)
    return -4;
  const hipError_t e = hipMemsetAsync(cnt_yes, 0, (size_t)n_cut * n_thr * sizeof(long long), stream);
  if (e != hipSuccess) return (int)e;
  if (n_img == 0) return 0;
  const int grid = n_img < 8 * sw_cu_count() ? n_img : 8 * sw_cu_count();
  hipLaunchKernelGGL(proposal_recall_kernel, dim3(grid), dim3(kThreads), 0, stream, n_img, prop_off, prop_box, gt_off, gt_box,
                     n_cut, cuts, n_thr, thr, ovmax, jmax, cnt_yes);
  SW_CHECK_LAUNCH();
  return 0;
}

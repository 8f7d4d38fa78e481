// Stage-2 pseudo-ground-truth filtering (reference tools/pgf.py: class_filter :273-292, pgf :221-271, contain_cal :209-219):
// stages 3-5 of a whole split in one launch (sw_pgf_keep), and the same filter over a grid of thresholds with each cell's kept set
// matched against the ground truth (sw_pgf_sweep, further down).
//
// Layout: a workgroup is 4 waves, a wave owns one image at a time; the workgroups stride over groups of 4 images (uniform trip
// count, so every wave meets the same barriers).  An image of at most kCap detections is staged in the wave's LDS slice (boxes,
// classes, the keep-stage survivors); a larger one reads boxes and classes from global memory and keeps its survivors in the
// caller's workspace.  The first survivor of each class comes from an LDS min-reduction over the detection index; the pair test
// runs one lane per detection i, looping over j in list order (all lanes read the same j: an LDS broadcast).
//
// Arithmetic: contain_cal's f64 operations in the reference's order (the library builds with -ffp-contract=off), Python's
// max / min / comparison semantics spelled out below.  No fast-math intrinsics: the IEEE division is required.
#include "common.h"
#include "soswsod_hip.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kCap = SW_PGF_LDS_CAP;
constexpr int kMaxK = SW_PGF_MAX_CLASSES;
constexpr int kNoIndex = 0x7FFFFFFF;

struct WaveSlice {
  double2 box[kCap][2];          // [x, y] [w, h] as given (for VOC records these are really [x1 + 1, y1 + 1] [x2, y2])
  int cls[kCap];
  int first[kMaxK];              // smallest index of a class-filter survivor of each class
  unsigned char survive[kCap];   // survived the keep stage
};

// Python's max(a, b) / min(a, b): the first argument unless the second compares strictly greater / smaller
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }

// bit c of a class mask; a class outside [0, K) is in no mask
__device__ __forceinline__ bool has_bit(const uint32_t* mask, int c, int K) {
  return (unsigned)c < (unsigned)K && ((mask[c >> 5] >> (c & 31)) & 1u);
}

// contain_cal(a, b) with the a-side terms precomputed: ax2 = a0 + a2, ay2 = a1 + a3, den = area_a + 1e-6
__device__ __forceinline__ double contain_quotient(double a0, double a1, double ax2, double ay2, double den, double2 bxy,
                                                   double2 bwh) {
  const double bx2 = bxy.x + bwh.x;
  const double by2 = bxy.y + bwh.y;
  const double c0 = py_max(a0, bxy.x);
  const double c1 = py_max(a1, bxy.y);
  const double c2 = py_min(ax2, bx2);
  const double c3 = py_min(ay2, by2);
  const double area_c = py_max(0.0, c2 - c0) * py_max(0.0, c3 - c1);
  return area_c / den;
}

// contain_cal(a, b) >= t_con
__device__ __forceinline__ bool contained(double a0, double a1, double ax2, double ay2, double den, double2 bxy, double2 bwh,
                                          double t_con) {
  return contain_quotient(a0, a1, ax2, ay2, den, bxy, bwh) >= t_con;
}

__global__ void __launch_bounds__(kThreads) pgf_keep_kernel(
    int n_img, const int64_t* __restrict__ det_off, const double* __restrict__ boxes, const double* __restrict__ scores,
    const int32_t* __restrict__ classes, int K, const uint32_t* __restrict__ gt_mask, const uint32_t* __restrict__ diff_mask,
    double t_keep, double t_con, int use_diff, uint8_t* __restrict__ keep, uint8_t* __restrict__ workspace,
    long long* __restrict__ counts) {
  __shared__ WaveSlice slices[kWaves];
  __shared__ unsigned long long red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  WaveSlice& S = slices[wave];
  const int words = (K + 31) >> 5;
  if (threadIdx.x < 4) red[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long n_in = 0, n_cls = 0, n_keep = 0, n_out = 0;

  const int n_groups = (n_img + kWaves - 1) / kWaves;
  for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int img = g * kWaves + wave;
    const int64_t base = img < n_img ? det_off[img] : 0;
    const int n = img < n_img ? (int)(det_off[img + 1] - base) : 0;
    const bool staged = n <= kCap;
    const uint32_t* gt = gt_mask + (long)(img < n_img ? img : 0) * words;
    const double2* gbox = reinterpret_cast<const double2*>(boxes) + 2 * base;
    const int32_t* gcls = classes + base;

    for (int c = lane; c < K; c += 64) S.first[c] = kNoIndex;
    if (staged) {
      for (int i = lane; i < n; i += 64) {
        S.box[i][0] = gbox[2 * i];
        S.box[i][1] = gbox[2 * i + 1];
        S.cls[i] = gcls[i];
      }
    }
    __syncthreads();

    // class filter + first survivor of each class
    for (int i = lane; i < n; i += 64) {
      const int c = staged ? S.cls[i] : gcls[i];
      if (has_bit(gt, c, K)) atomicMin(&S.first[c], i);
    }
    __syncthreads();

    // keep stage: the first survivor of a class stays whatever its score; a later one goes if score < t_keep
    for (int i = lane; i < n; i += 64) {
      const int c = staged ? S.cls[i] : gcls[i];
      const bool pass_cls = has_bit(gt, c, K);
      const bool pass_keep = pass_cls && (S.first[c] == i || !(scores[base + i] < t_keep));
      n_cls += pass_cls;
      n_keep += pass_keep;
      if (staged) S.survive[i] = pass_keep;
      else workspace[base + i] = pass_keep;
    }
    if (lane == 0) n_in += (unsigned long long)n;
    __syncthreads();

    // containment stage: i goes if another keep-stage survivor j of its class contains it (j may itself go)
    for (int i = lane; i < n; i += 64) {
      bool out = staged ? S.survive[i] : workspace[base + i];
      if (out) {
        const int c = staged ? S.cls[i] : gcls[i];
        if (use_diff || !has_bit(diff_mask, c, K)) {
          const double2 axy = staged ? S.box[i][0] : gbox[2 * i];
          const double2 awh = staged ? S.box[i][1] : gbox[2 * i + 1];
          const double ax2 = axy.x + awh.x;
          const double ay2 = axy.y + awh.y;
          const double area_a = py_max(0.0, ax2 - axy.x) * py_max(0.0, ay2 - axy.y);
          const double den = area_a + 1e-6;
          for (int j = 0; j < n && out; ++j) {
            if (j == i) continue;
            if (staged) {
              if (!S.survive[j] || S.cls[j] != c) continue;
              if (contained(axy.x, axy.y, ax2, ay2, den, S.box[j][0], S.box[j][1], t_con)) out = false;
            } else {
              if (!workspace[base + j] || gcls[j] != c) continue;
              if (contained(axy.x, axy.y, ax2, ay2, den, gbox[2 * j], gbox[2 * j + 1], t_con)) out = false;
            }
          }
        }
      }
      keep[base + i] = out;
      n_out += out;
    }
    __syncthreads();          // the next group overwrites the slices
  }

  atomicAdd(&red[0], n_in);
  atomicAdd(&red[1], n_cls);
  atomicAdd(&red[2], n_keep);
  atomicAdd(&red[3], n_out);
  __syncthreads();
  if (threadIdx.x < 4) atomicAdd(reinterpret_cast<unsigned long long*>(counts) + threadIdx.x, red[threadIdx.x]);
}

}  // namespace

extern "C" int sw_pgf_keep(int n_img, const int64_t* det_off, const double* boxes, const double* scores, const int32_t* classes,
                           int K, const uint32_t* gt_mask, const uint32_t* diff_mask, double t_keep, double t_con, int use_diff,
                           uint8_t* keep, uint8_t* workspace, long long* counts, hipStream_t stream) {
  SW_ENTER();
  if (n_img < 0) return -5;
  if (K < 1 || K > SW_PGF_MAX_CLASSES) return -6;
  if (((uintptr_t)boxes & 15) != 0 || ((uintptr_t)counts & 7) != 0) return -4;
  const hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(long long), stream);
  if (e != hipSuccess) return (int)e;
  if (n_img == 0) return 0;
  const int n_groups = (n_img + kWaves - 1) / kWaves;
  const int grid = n_groups < 4 * sw_cu_count() ? n_groups : 4 * sw_cu_count();
  hipLaunchKernelGGL(pgf_keep_kernel, dim3(grid), dim3(kThreads), 0, stream, n_img, det_off, boxes, scores, classes, K, gt_mask,
                     diff_mask, t_keep, t_con, use_diff, keep, workspace, counts);
  SW_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The threshold sweep: the kept set of every (t_keep[a], t_con[b]) cell matched against the ground truth by voc_eval's rule
// (evaluation/pascal_voc_evaluation.py:357-397), counted per cell and class.
//
// Two identities make the grid share its work (both follow from the loops of pgf :221-271):
//   * a detection survives stage 4 at t_keep[a] iff it is the first class-filter survivor of its class or !(score < t_keep[a]):
//     one bit per a, the word `msk`;
//   * detection i leaves cell (a, b) iff m_i[a] >= t_con[b], m_i[a] the largest contain_cal(i, j) over the same-class stage-4
//     survivors j != i at t_keep[a].  Each pair's quotient is computed once and offered to every a both survive at.  Only the
//     number r of grid values t_con <= m_i[a] is kept (a byte): m >= t_con[b] iff r >= pos[b], pos[b] the number of grid values
//     <= t_con[b] (the host counts them; the grid is finite).
// The matching box, ovmax and jmax of a detection depend on no cell, so they are computed once as well.
//
// Layout: a wave owns one image at a time and meets no workgroup barrier; the waves of the grid stride over the images.  The
// wave walks the image's classes; for a class it lists the members (list order), runs one lane per member for m, the rank bytes
// and the match, then one lane per cell over the members for the counts, which leave as 64-bit integer atomic adds (zero counts
// are skipped).  An image of at most kCap detections keeps boxes, classes and the per-member words in the wave's LDS slice; a
// larger one reads boxes and classes from global memory and keeps the per-member words in the caller's workspace.
namespace {

constexpr int kSweepWaves = 2;                     // 2 x 22 KiB of slices: three workgroups per CU
constexpr int kSweepThreads = 64 * kSweepWaves;
constexpr int kMaxKeep = SW_PGF_SWEEP_MAX_KEEP;
constexpr int kMaxCon = SW_PGF_SWEEP_MAX_CON;
constexpr int kMaxIou = SW_PGF_SWEEP_MAX_IOU;
constexpr int kWsWords = SW_PGF_SWEEP_WS_WORDS;
constexpr uint32_t kIgnored = 1u << 15;            // in a member's match word, above the kMaxIou threshold bits
static_assert(kMaxKeep == 32 && kMaxCon <= 255 && kMaxIou < 15, "one bit per t_keep in a word, ranks in a byte");
static_assert(kWsWords == 4 + kMaxKeep / 4, "list, msk, jm, rm and the rank bytes of a member");

struct SweepGrid {
  double t_keep[kMaxKeep], t_con[kMaxCon], iou[kMaxIou];
  int pos[kMaxCon];
  int nk, nc, nt;
};

struct SweepSlice {
  double2 box[kCap][2];
  int cls[kCap];
  int first[kMaxK];
  // per member of the class at hand, in list order
  int list[kCap];                 // its detection index
  uint32_t msk[kCap];             // bit a: a stage-4 survivor at t_keep[a]
  int jm[kCap];                   // jmax: the image's ground-truth row it matches, -1 without a candidate
  uint32_t rm[kCap];              // bit t: ovmax > iou[t]; kIgnored: object jmax is ignored
  uint32_t rank[kCap][kMaxKeep / 4];   // byte a: how many t_con are <= m[a]
};

// orders the wave's own writes (LDS, or the workspace through the same generic pointers) before its later reads
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(kSweepThreads) pgf_sweep_kernel(
    int n_img, long long N, const int64_t* __restrict__ det_off, const double* __restrict__ boxes,
    const double* __restrict__ scores, const int32_t* __restrict__ classes, int K, const uint32_t* __restrict__ gt_mask,
    const uint32_t* __restrict__ diff_mask, int use_diff, const SweepGrid grid, const int64_t* __restrict__ gt_off,
    const double* __restrict__ gt_box, const int32_t* __restrict__ gt_cls, const uint8_t* __restrict__ gt_ign, int xywh,
    int plus_one, uint32_t* __restrict__ workspace, unsigned long long* __restrict__ kept, unsigned long long* __restrict__ tp,
    unsigned long long* __restrict__ ign, unsigned long long* __restrict__ npos) {
  __shared__ SweepSlice slices[kSweepWaves];
  __shared__ SweepGrid G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  SweepSlice& S = slices[wave];
  if (threadIdx.x == 0) G = grid;
  __syncthreads();
  const int nk = G.nk, nc = G.nc, nt = G.nt;
  const int words = (K + 31) >> 5;
  const double p1 = plus_one ? 1.0 : 0.0;
  const uint32_t all_keep = nk == 32 ? 0xFFFFFFFFu : (1u << nk) - 1u;
  const long long cell_stride = (long long)nk * nc * K;         // one threshold's table

  for (int img = blockIdx.x * kSweepWaves + wave; img < n_img; img += gridDim.x * kSweepWaves) {
    const int64_t base = det_off[img];
    const int n = (int)(det_off[img + 1] - base);
    const int64_t gbase = gt_off[img];
    const int gn = (int)(gt_off[img + 1] - gbase);
    const bool staged = n <= kCap;
    const uint32_t* gt = gt_mask + (long)img * words;
    const double2* gbox = reinterpret_cast<const double2*>(boxes) + 2 * base;
    const int32_t* gcls = classes + base;
    // the per-member words: the slice, or this image's rows of the workspace
    int* list = staged ? S.list : reinterpret_cast<int*>(workspace) + base;
    uint32_t* msk = staged ? S.msk : workspace + N + base;
    int* jm = staged ? S.jm : reinterpret_cast<int*>(workspace) + 2 * N + base;
    uint32_t* rm = staged ? S.rm : workspace + 3 * N + base;
    unsigned char* rank = staged ? reinterpret_cast<unsigned char*>(S.rank)
                                 : reinterpret_cast<unsigned char*>(workspace + 4 * N) + base * kMaxKeep;

    // npos: the image's non-ignored objects
    for (int g = lane; g < gn; g += 64) {
      const int c = gt_cls[gbase + g];
      if ((unsigned)c < (unsigned)K && !gt_ign[gbase + g]) atomicAdd(&npos[c], 1ull);
    }

    for (int c = lane; c < K; c += 64) S.first[c] = kNoIndex;
    if (staged) {
      for (int i = lane; i < n; i += 64) {
        S.box[i][0] = gbox[2 * i];
        S.box[i][1] = gbox[2 * i + 1];
        S.cls[i] = gcls[i];
      }
    }
    wave_sync();
    // class filter + first survivor of each class
    for (int i = lane; i < n; i += 64) {
      const int c = staged ? S.cls[i] : gcls[i];
      if (has_bit(gt, c, K)) atomicMin(&S.first[c], i);
    }
    wave_sync();

    for (int c = 0; c < K; ++c) {
      const int first = S.first[c];
      if (first == kNoIndex) continue;           // no detection of this class passes the class filter

      // the members in list order, each with its stage-4 bits
      int nm = 0;
      for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool is = i < n && (staged ? S.cls[i] : gcls[i]) == c;
        const unsigned long long vote = __ballot(is);
        if (is) {
          const int k = nm + __popcll(vote & ((1ull << lane) - 1ull));
          uint32_t bits = all_keep;
          if (i != first) {
            const double s = scores[base + i];
            bits = 0;
            for (int a = 0; a < nk; ++a) bits |= (uint32_t)(!(s < G.t_keep[a])) << a;
          }
          list[k] = i;
          msk[k] = bits;
        }
        nm += __popcll(vote);
      }
      wave_sync();

      const bool exempt = !use_diff && has_bit(diff_mask, c, K);
      for (int k0 = 0; k0 < nm; k0 += 64) {
        const int k = k0 + lane;
        if (k < nm) {
          const int i = list[k];
          const uint32_t mi = msk[k];
          const double2 axy = staged ? S.box[i][0] : gbox[2 * i];
          const double2 awh = staged ? S.box[i][1] : gbox[2 * i + 1];
          const double ax2 = axy.x + awh.x;
          const double ay2 = axy.y + awh.y;

          // containment: the largest quotient per t_keep, then its rank among the t_con
          uint32_t rw[kMaxKeep / 4] = {};
          if (!exempt) {
            const double area_a = py_max(0.0, ax2 - axy.x) * py_max(0.0, ay2 - axy.y);
            const double den = area_a + 1e-6;
            double m[kMaxKeep];
#pragma unroll
            for (int a = 0; a < kMaxKeep; ++a) m[a] = -__builtin_inf();
            for (int kk = 0; kk < nm; ++kk) {
              const uint32_t both = msk[kk] & mi;
              if (kk == k || both == 0) continue;
              const int j = list[kk];
              const double q = contain_quotient(axy.x, axy.y, ax2, ay2, den, staged ? S.box[j][0] : gbox[2 * j],
                                                staged ? S.box[j][1] : gbox[2 * j + 1]);
#pragma unroll
              for (int a = 0; a < kMaxKeep; ++a)
                if (((both >> a) & 1u) && q > m[a]) m[a] = q;          // `v > m ? v : m`: a NaN never enters
            }
#pragma unroll
            for (int a = 0; a < kMaxKeep; ++a) {
              uint32_t r = 0;
              for (int b = 0; b < nc; ++b) r += G.t_con[b] <= m[a];
              rw[a >> 2] |= r << (8 * (a & 3));
            }
          }
#pragma unroll
          for (int w = 0; w < kMaxKeep / 4; ++w) reinterpret_cast<uint32_t*>(rank)[(long)k * (kMaxKeep / 4) + w] = rw[w];

          // voc_eval's overlaps with the image's objects of this class: numpy max / argmax (first maximum, a NaN wins)
          const double bx1 = axy.x, by1 = axy.y, bx2 = xywh ? ax2 : awh.x, by2 = xywh ? ay2 : awh.y;
          const double area_d = (bx2 - bx1 + p1) * (by2 - by1 + p1);
          double ovmax = 0.0;
          int jmax = -1;
          for (int g = 0; g < gn; ++g) {
            if (gt_cls[gbase + g] != c) continue;
            const double2 g0 = reinterpret_cast<const double2*>(gt_box)[2 * (gbase + g)];
            const double2 g1 = reinterpret_cast<const double2*>(gt_box)[2 * (gbase + g) + 1];
            const double ixmin = g0.x > bx1 ? g0.x : bx1, iymin = g0.y > by1 ? g0.y : by1;
            const double ixmax = g1.x < bx2 ? g1.x : bx2, iymax = g1.y < by2 ? g1.y : by2;
            const double iw0 = ixmax - ixmin + p1, ih0 = iymax - iymin + p1;
            const double inters = (iw0 > 0.0 ? iw0 : 0.0) * (ih0 > 0.0 ? ih0 : 0.0);
            const double uni = area_d + (g1.x - g0.x + p1) * (g1.y - g0.y + p1) - inters;
            const double ov = inters / uni;
            if (jmax < 0 || ov > ovmax || (ov != ov && ovmax == ovmax)) { ovmax = ov; jmax = g; }
          }
          uint32_t r = 0;
          if (jmax >= 0) {
            for (int t = 0; t < nt; ++t) r |= (uint32_t)(ovmax > G.iou[t]) << t;
            if (gt_ign[gbase + jmax]) r |= kIgnored;
          }
          jm[k] = jmax;
          rm[k] = r;
        }
      }
      wave_sync();

      // one lane per cell
      for (int cell = lane; cell < nk * nc; cell += 64) {
        const int a = cell / nc, b = cell - a * nc;
        const uint32_t pb = (uint32_t)G.pos[b];
        unsigned n_kept = 0, n_ign[kMaxIou] = {}, n_tp[kMaxIou] = {};
        for (int k = 0; k < nm; ++k) {
          if (!((msk[k] >> a) & 1u) || rank[(long)k * kMaxKeep + a] >= pb) continue;
          ++n_kept;
          const uint32_t r = rm[k];
          if (r & kIgnored) {
#pragma unroll
            for (int t = 0; t < kMaxIou; ++t) n_ign[t] += (r >> t) & 1u;
          }
        }
        // tp counts the claimed objects: object g is claimed at t if a kept detection with jmax == g has ovmax > iou[t]
        for (int g = 0; g < gn; ++g) {
          if (gt_cls[gbase + g] != c || gt_ign[gbase + g]) continue;
          uint32_t claim = 0;
          for (int k = 0; k < nm; ++k) {
            if (jm[k] != g) continue;
            if (((msk[k] >> a) & 1u) && rank[(long)k * kMaxKeep + a] < pb) claim |= rm[k];
          }
#pragma unroll
          for (int t = 0; t < kMaxIou; ++t) n_tp[t] += (claim >> t) & 1u;
        }
        const long long at = (long long)cell * K + c;
        if (n_kept) atomicAdd(&kept[at], (unsigned long long)n_kept);
#pragma unroll
        for (int t = 0; t < kMaxIou; ++t) {
          if (t < nt && n_ign[t]) atomicAdd(&ign[t * cell_stride + at], (unsigned long long)n_ign[t]);
          if (t < nt && n_tp[t]) atomicAdd(&tp[t * cell_stride + at], (unsigned long long)n_tp[t]);
        }
      }
      wave_sync();            // the next class overwrites the member words
    }
  }
}

}  // namespace

extern "C" int sw_pgf_sweep(int n_img, long long N, const int64_t* det_off, const double* boxes, const double* scores,
                            const int32_t* classes, int K, const uint32_t* gt_mask, const uint32_t* diff_mask, int use_diff,
                            int nk, const double* t_keep, int nc, const double* t_con, int nt, const double* iou,
                            const int64_t* gt_off, const double* gt_box, const int32_t* gt_cls, const uint8_t* gt_ign, int xywh,
                            int plus_one, uint32_t* workspace, long long* kept, long long* tp, long long* ign, long long* npos,
                            hipStream_t stream) {
  SW_ENTER();
  if (n_img < 0 || N < 0) return -5;
  if (K < 1 || K > SW_PGF_MAX_CLASSES) return -6;
  if (nk < 1 || nk > kMaxKeep || nc < 1 || nc > kMaxCon || nt < 1 || nt > kMaxIou) return -7;
  SweepGrid grid = {};
  grid.nk = nk; grid.nc = nc; grid.nt = nt;
  for (int a = 0; a < nk; ++a) grid.t_keep[a] = t_keep[a];
  for (int b = 0; b < nc; ++b) grid.t_con[b] = t_con[b];
  for (int t = 0; t < nt; ++t) grid.iou[t] = iou[t];
  for (int i = 0; i < nk + nc + nt; ++i) {
    const double v = i < nk ? t_keep[i] : i < nk + nc ? t_con[i - nk] : iou[i - nk - nc];
    if (!(v - v == 0.0)) return -7;              // NaN or infinite
  }
  for (int b = 0; b < nc; ++b)
    for (int o = 0; o < nc; ++o) grid.pos[b] += t_con[o] <= t_con[b];
  if (((uintptr_t)boxes & 15) != 0 || ((uintptr_t)gt_box & 15) != 0 || ((uintptr_t)workspace & 3) != 0 ||
      (((uintptr_t)kept | (uintptr_t)tp | (uintptr_t)ign | (uintptr_t)npos) & 7) != 0)
    return -4;
  const size_t cells = (size_t)nk * nc * K * sizeof(long long);
  hipError_t e = hipMemsetAsync(kept, 0, cells, stream);
  if (e == hipSuccess) e = hipMemsetAsync(tp, 0, nt * cells, stream);
  if (e == hipSuccess) e = hipMemsetAsync(ign, 0, nt * cells, stream);
  if (e == hipSuccess) e = hipMemsetAsync(npos, 0, K * sizeof(long long), stream);
  if (e != hipSuccess) return (int)e;
  if (n_img == 0) return 0;
  const int n_groups = (n_img + kSweepWaves - 1) / kSweepWaves;
  const int blocks = n_groups < 6 * sw_cu_count() ? n_groups : 6 * sw_cu_count();
  hipLaunchKernelGGL(pgf_sweep_kernel, dim3(blocks), dim3(kSweepThreads), 0, stream, n_img, N, det_off, boxes, scores, classes, K,
                     gt_mask, diff_mask, use_diff, grid, gt_off, gt_box, gt_cls, gt_ign, xywh, plus_one, workspace,
                     reinterpret_cast<unsigned long long*>(kept), reinterpret_cast<unsigned long long*>(tp),
                     reinterpret_cast<unsigned long long*>(ign), reinterpret_cast<unsigned long long*>(npos));
  SW_CHECK_LAUNCH();
  return 0;
}

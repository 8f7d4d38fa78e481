// VOC AP and CorLoc of a whole split (reference evaluation/pascal_voc_evaluation.py: voc_eval :295-408, voc_ap :263-292,
// voc_eval_corloc :411-505): every class at every IoU threshold in two launches.
//
// Match kernel: one lane per detection.  It takes the IoU against the ground truth of its (image, class) with numpy's f64
// operations in the reference's order, ovmax = np.max (NaN-propagating) and jmax = np.argmax (first maximum).  The sequential
// "first unclaimed match wins" rule becomes a min-reduction: at each threshold a detection that matches a non-difficult object
// takes an atomicMin of its row into that object's claim slot, and the smallest row (the best-ranked detection) holds it.  A
// detection also takes an atomicMin into its (class, image) slot when the image has a non-difficult object of the class: the
// slot's holder is the detection voc_eval_corloc looks at for that image.  Min-reductions make the result independent of
// scheduling.
//
// AP kernel: one workgroup per (class, threshold).  Pass 1 walks the class's detections forward in tiles: TP / FP flags, a
// block-wide prefix scan of the packed (TP << 32 | FP) counts, the CorLoc count.  Pass 2 walks the sentinel-extended
// precision / recall arrays of voc_ap backward: a suffix max (the precision envelope), a suffix count of the recall change points
// (their positions in the compacted term array, stored back to front), the 11-point levels (recall never decreases, so
// rec >= t is a suffix and its max precision is the envelope there).  One lane then sums the terms in np.sum's order: chunks of
// 8192 (the ufunc buffer), each a pairwise sum with eight accumulators over leaves of at most 128.
//
// COCO bbox evaluation (reference evaluation/fast_eval_api.py: COCOeval_opt over layers/csrc/cocoeval/cocoeval.cpp, with the
// pieces it inherits from pycocotools: computeIoU -> maskApi.c bbIou, _prepare, summarize) in two more launches.
//
// coco_match_kernel (cocoeval.cpp:61-140 MatchDetectionsToGroundTruth, :33-56 SortInstancesByIgnore, maskApi.c bbIou): the work
// item is an (image, category) pair that has detections, one wave per pair, four waves per workgroup striding over the pairs.  The
// wave computes the pair's IoU matrix once (at most 100 x G, f64), builds the four area ranges' stable "non-ignored first"
// partitions with ballots, and then lanes 0..39 each own one (area range, IoU threshold) greedy walk over the detections in score
// order; the set of taken ground truths of a walk is a bitmask.  The matrix, the partitions and the bitmasks live in the wave's
// LDS slice when G <= 64 and D * G <= lds_doubles, otherwise in the pair's region of the global workspace (a crowd image with
// hundreds of boxes of one class); both are reached through the same pointers.  Per detection the 40 walks' "matched" (ground
// truth id > 0, the reference's test) and "ignored" bits come out of two ballots.  Nothing depends on scheduling.
//
// coco_accum_kernel (cocoeval.cpp:222-370 BuildSortedDetectionList, ComputePrecisionRecallCurve): one workgroup per (category,
// area range, maxDet, threshold) walks the category's score-sorted detection list in tiles, keeping the detections of in-image
// rank < maxDet.  Pass 1 sums the packed (TP << 32 | FP) flags.  Pass 2 walks the tiles backward: a block-wide prefix scan gives
// the running TP / FP sums (the tile's carry is the later tile's carry minus the tile's total), a suffix max the precision
// envelope (the reference's backward loop with >).  recall = tp / npig is monotonic in the integer tp, so lower_bound over the
// recalls at level r is the position of the n_r-th true positive, n_r the smallest n with (double)n / npig >= recThrs[r] (position
// 0 for n_r = 0): the true positive whose running count is n_r writes the precision envelope and its score for that level.
#include <cmath>

#include "common.h"
#include "soswsod_hip.h"

namespace {

constexpr int kT = SW_VOC_THRESHOLDS;
constexpr int kThreads = 256;
constexpr int kItems = 4;
constexpr int kTile = kThreads * kItems;

// np.maximum / np.minimum on two scalars: NaN in either argument gives NaN
__device__ __forceinline__ double np_max(double a, double b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ double np_min(double a, double b) { return (a <= b || a != a) ? a : b; }

struct Layout {
  size_t ovmax, jmax, claim, first, cum, terms, total;
};

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

__host__ __device__ inline Layout layout(int K, int n_img, long long N, long long G) {
  Layout L;
  size_t o = 0;
  L.ovmax = o; o = align256(o + sizeof(double) * N);
  L.jmax = o; o = align256(o + sizeof(int) * N);
  L.claim = o; o = align256(o + sizeof(int) * G * kT);
  L.first = o; o = align256(o + sizeof(int) * (size_t)K * n_img);
  L.cum = o; o = align256(o + sizeof(unsigned long long) * N * kT);
  L.terms = o; o = align256(o + sizeof(double) * (N + K) * kT);
  L.total = o < 256 ? 256 : o;
  return L;
}

__global__ void __launch_bounds__(kThreads) voc_match_kernel(
    int K, int n_img, long long N, const int64_t* __restrict__ det_off, const int32_t* __restrict__ det_img,
    const double* __restrict__ det_box, const int64_t* __restrict__ gt_off, const double* __restrict__ gt_box,
    const uint8_t* __restrict__ gt_diff, const double* __restrict__ thr, double* __restrict__ ovmax_out,
    int* __restrict__ jmax_out, int* __restrict__ claim, int* __restrict__ first) {
  const long long d = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (d >= N) return;
  int lo = 0, hi = K - 1;                       // the class: the largest c with det_off[c] <= d
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (det_off[mid] <= d) lo = mid;
    else hi = mid - 1;
  }
  const int c = lo;
  const int img = det_img[d];
  const int64_t g0 = gt_off[(long long)img * K + c], g1 = gt_off[(long long)img * K + c + 1];
  const double2* bp = reinterpret_cast<const double2*>(det_box) + 2 * d;
  const double2 b01 = bp[0], b23 = bp[1];
  const double area_b = (b23.x - b01.x + 1.0) * (b23.y - b01.y + 1.0);
  double ov = -INFINITY;
  int j = -1;
  bool any_nan = false, any_plain = false;
  for (int64_t g = g0; g < g1; ++g) {
    const double2* gp = reinterpret_cast<const double2*>(gt_box) + 2 * g;
    const double2 q01 = gp[0], q23 = gp[1];
    const double ixmin = np_max(q01.x, b01.x);
    const double iymin = np_max(q01.y, b01.y);
    const double ixmax = np_min(q23.x, b23.x);
    const double iymax = np_min(q23.y, b23.y);
    const double iw = np_max(ixmax - ixmin + 1.0, 0.0);
    const double ih = np_max(iymax - iymin + 1.0, 0.0);
    const double inters = iw * ih;
    const double uni = area_b + (q23.x - q01.x + 1.0) * (q23.y - q01.y + 1.0) - inters;
    const double o = inters / uni;
    any_nan |= o != o;
    if (j < 0 || o > ov) {                      // np.argmax: the first maximum (only read when no overlap is NaN)
      ov = o;
      j = (int)g;
    }
    any_plain |= gt_diff[g] == 0;
  }
  if (any_nan) ov = NAN;                        // np.max propagates NaN; NaN > thr is false
  ovmax_out[d] = ov;
  jmax_out[d] = j;
  if (j >= 0 && gt_diff[j] == 0) {
#pragma unroll
    for (int t = 0; t < kT; ++t)
      if (ov > thr[t]) atomicMin(&claim[(long long)j * kT + t], (int)d);
  }
  if (any_plain) atomicMin(&first[(long long)c * n_img + img], (int)d);
}

struct MaxCount {
  double m;
  int n;
};

// numpy's pairwise_sum of a[s, s + n) for n <= 8192, with a(k) = rterms[last - k] (the terms are stored back to front)
__device__ double pairwise_leaf(const double* rterms, long long last, long long s, long long n) {
  if (n < 8) {
    double res = 0.0;
    for (long long i = 0; i < n; ++i) res += rterms[last - (s + i)];
    return res;
  }
  double r[8];
  for (int k = 0; k < 8; ++k) r[k] = rterms[last - (s + k)];
  long long i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int k = 0; k < 8; ++k) r[k] += rterms[last - (s + i + k)];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += rterms[last - (s + i)];
  return res;
}

__device__ double pairwise_sum(const double* rterms, long long last, long long s, long long n) {
  struct Frame {
    long long s, n;
    double left;
    int stage;
  };
  Frame st[16];                                  // n <= 8192: seven levels above the 128-leaves
  int sp = 0;
  st[0] = {s, n, 0.0, 0};
  double ret = 0.0;
  for (;;) {
    Frame& f = st[sp];
    if (f.n <= 128) {
      ret = pairwise_leaf(rterms, last, f.s, f.n);
      --sp;
    } else {
      long long n2 = f.n / 2;
      n2 -= n2 % 8;
      if (f.stage == 0) {
        f.stage = 1;
        st[sp + 1] = {f.s, n2, 0.0, 0};
        ++sp;
        continue;
      }
      if (f.stage == 1) {
        f.left = ret;
        f.stage = 2;
        st[sp + 1] = {f.s + n2, f.n - n2, 0.0, 0};
        ++sp;
        continue;
      }
      ret = f.left + ret;
      --sp;
    }
    if (sp < 0) return ret;
  }
}

__global__ void __launch_bounds__(kThreads) voc_ap_kernel(
    int K, int n_img, long long N, const int64_t* __restrict__ det_off, const int32_t* __restrict__ det_img,
    const uint8_t* __restrict__ gt_diff, const int64_t* __restrict__ npos, const int64_t* __restrict__ npos_im,
    const double* __restrict__ thr, const double* __restrict__ t11, const double* __restrict__ ovmax,
    const int* __restrict__ jmax, const int* __restrict__ claim, const int* __restrict__ first,
    unsigned long long* __restrict__ cum_all, double* __restrict__ terms_all, double* __restrict__ out) {
  __shared__ unsigned long long sbuf[kThreads];
  __shared__ MaxCount mbuf[kThreads];
  __shared__ int cbuf[kThreads];
  __shared__ double p11[11];
  const int tid = threadIdx.x;
  const int c = blockIdx.x / kT, t = blockIdx.x % kT;
  const long long base = det_off[c], nd = det_off[c + 1] - base;
  const double tau = thr[t];
  const double npos_d = (double)npos[c];
  unsigned long long* cum = cum_all + (long long)t * N + base;
  double* rterms = terms_all + (long long)t * (N + K) + base + c;
  if (tid < 11) p11[tid] = 0.0;

  // pass 1: TP / FP flags in rank order, their running sums; the CorLoc count
  unsigned long long carry = 0;
  int hits = 0;
  for (long long lo = 0; lo < nd; lo += kTile) {
    unsigned long long v[kItems], run = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const long long d = lo + tid * kItems + k;
      unsigned long long f = 0;
      if (d < nd) {
        const long long gd = base + d;
        const double ov = ovmax[gd];
        if (ov > tau) {
          const int j = jmax[gd];
          // TP when it holds the object's claim, FP when a better-ranked detection does; a difficult match counts as neither
          if (gt_diff[j] == 0) f = claim[(long long)j * kT + t] == (int)gd ? (1ull << 32) : 1ull;
          if (first[(long long)c * n_img + det_img[gd]] == (int)gd) ++hits;
        } else {
          f = 1ull;                              // no match above the threshold (NaN included): FP
        }
      }
      run += f;
      v[k] = run;
    }
    const BlockScan<unsigned long long> sc = block_scan<kThreads>(run, sbuf, ScanAdd());
    const unsigned long long before = carry + sc.incl - run;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const long long d = lo + tid * kItems + k;
      if (d < nd) cum[d] = before + v[k];
    }
    carry += sc.total;
  }
  __syncthreads();                               // cum complete and visible to the workgroup

  auto rec_of = [&](long long d) { return (double)(cum[d] >> 32) / npos_d; };
  auto prec_of = [&](long long d) {
    const double tp = (double)(cum[d] >> 32), fp = (double)(cum[d] & 0xFFFFFFFFull);
    const double s = tp + fp;
    return tp / (s >= 2.220446049250313e-16 ? s : 2.220446049250313e-16);
  };

  // pass 2: i = nd .. 0 over mrec = [0, rec, 1], mpre = [0, prec, 0]; r = nd - i runs forward through the tiles
  MaxCount mcarry = {-INFINITY, 0};
  for (long long lo = 0; lo <= nd; lo += kTile) {
    double mpre[kItems], m0[kItems], m1[kItems];
    MaxCount run = {-INFINITY, 0};
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const long long r = lo + tid * kItems + k;
      mpre[k] = -INFINITY;
      m0[k] = m1[k] = 0.0;
      if (r <= nd) {
        const long long i = nd - r;
        mpre[k] = i == nd ? 0.0 : prec_of(i);
        m0[k] = i == 0 ? 0.0 : rec_of(i - 1);
        m1[k] = i == nd ? 1.0 : rec_of(i);
        run.m = np_max(mpre[k], run.m);
        run.n += m1[k] != m0[k];
      }
    }
    const BlockScan<MaxCount> sc = block_scan<kThreads>(run, mbuf, [](MaxCount a, MaxCount b) { return MaxCount{np_max(b.m, a.m), a.n + b.n}; });
    double env = tid > 0 ? np_max(sc.prev.m, mcarry.m) : mcarry.m;            // max(mpre[i + 1 ..]) above this thread's items
    int pos = mcarry.n + sc.incl.n - run.n;                                   // change points at larger i
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const long long r = lo + tid * kItems + k;
      if (r > nd) break;
      const long long i = nd - r;
      env = np_max(mpre[k], env);                // the envelope at i + 1
      if (m1[k] != m0[k]) rterms[pos++] = (m1[k] - m0[k]) * env;
      if (i < nd) {                              // 11-point: i is the first detection with rec >= t11[q]
        for (int q = 0; q < 11; ++q)
          if (m1[k] >= t11[q] && !(i > 0 && m0[k] >= t11[q])) p11[q] = env;
      }
    }
    mcarry.m = np_max(sc.total.m, mcarry.m);
    mcarry.n += sc.total.n;
  }
  __syncthreads();

  // hits across the workgroup
  cbuf[tid] = hits;
  __syncthreads();
  if (tid == 0) {
    long long n_hit = 0;
    for (int k = 0; k < kThreads; ++k) n_hit += cbuf[k];
    const long long n_terms = mcarry.n;
    double area = 0.0;                           // np.sum: the identity, then one pairwise sum per 8192-element chunk
    for (long long s = 0; s < n_terms; s += 8192)
      area += pairwise_sum(rterms, n_terms - 1, s, n_terms - s < 8192 ? n_terms - s : 8192);
    double ap11 = 0.0;
    for (int q = 0; q < 11; ++q) ap11 = ap11 + p11[q] / 11.0;
    const double corloc = nd == 0 ? 0.0 : 1.0 * (double)n_hit / (double)npos_im[c];
    out[(0 * K + c) * kT + t] = area;
    out[(1 * K + c) * kT + t] = ap11;
    out[(2 * K + c) * kT + t] = corloc;
  }
}

}  // namespace

extern "C" long long sw_voc_eval_workspace_bytes(int K, int n_img, long long N, long long G) {
  if (K < 1 || n_img < 0 || N < 0 || G < 0) return -1;
  return (long long)layout(K, n_img, N, G).total;
}

extern "C" int sw_voc_eval(int K, int n_img, long long N, long long G, const int64_t* det_off, const int32_t* det_img,
                           const double* det_box, const int64_t* gt_off, const double* gt_box, const uint8_t* gt_diff,
                           const int64_t* npos, const int64_t* npos_im, const double* thr, const double* t11, double* out,
                           void* workspace, hipStream_t stream) {
  SW_ENTER();
  if (K < 1 || K > SW_VOC_MAX_CLASSES) return -6;
  if (n_img < 0 || N < 0 || G < 0 || N > SW_VOC_MAX_DETS || G * kT >= (1LL << 31)) return -5;
  if (((uintptr_t)det_box & 15) != 0 || ((uintptr_t)gt_box & 15) != 0 || ((uintptr_t)out & 7) != 0 ||
      ((uintptr_t)workspace & 255) != 0)
    return -4;
  const Layout L = layout(K, n_img, N, G);
  char* ws = static_cast<char*>(workspace);
  double* ovmax = reinterpret_cast<double*>(ws + L.ovmax);
  int* jmax = reinterpret_cast<int*>(ws + L.jmax);
  int* claim = reinterpret_cast<int*>(ws + L.claim);
  int* first = reinterpret_cast<int*>(ws + L.first);
  hipError_t e = hipMemsetAsync(claim, 0x7F, sizeof(int) * G * kT, stream);
  if (e == hipSuccess) e = hipMemsetAsync(first, 0x7F, sizeof(int) * (size_t)K * n_img, stream);
  if (e != hipSuccess) return (int)e;
  if (N > 0) {
    hipLaunchKernelGGL(voc_match_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, K, n_img, N,
                       det_off, det_img, det_box, gt_off, gt_box, gt_diff, thr, ovmax, jmax, claim, first);
    SW_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(voc_ap_kernel, dim3(K * kT), dim3(kThreads), 0, stream, K, n_img, N, det_off, det_img, gt_diff, npos,
                     npos_im, thr, t11, ovmax, jmax, claim, first,
                     reinterpret_cast<unsigned long long*>(ws + L.cum), reinterpret_cast<double*>(ws + L.terms), out);
  SW_CHECK_LAUNCH();
  return 0;
}

// ---- COCO bbox evaluation ----------------------------------------------------------------------------------------------------
namespace {

constexpr int kCT = SW_COCO_THRESHOLDS;
constexpr int kCR = SW_COCO_RECALLS;
constexpr int kCA = SW_COCO_AREAS;
constexpr int kCM = SW_COCO_MAXDETS;
constexpr int kWalks = kCA * kCT;                // 40 of a wave's 64 lanes own a walk
constexpr int kCWaves = 4;
constexpr int kLdsCap = SW_COCO_LDS_DOUBLES;
constexpr int kLdsG = 64;
typedef unsigned long long u64;

// 14,160 bytes: four slices are 56,640 bytes of a CU's 160 KiB, so two workgroups (eight waves) are resident per CU
struct CocoSlice {
  double iou[kLdsCap];
  u64 taken[kWalks];
  int perm[kCA * kLdsG];
  int nvalid[kCA];
};

__host__ __device__ inline bool coco_fits(long long D, long long G, int lds_doubles) { return G <= kLdsG && D * G <= lds_doubles; }
// 8-byte words of a pair's workspace region: iou [D][G] f64, taken [40][W] u64, perm [4][G] i32
__host__ __device__ inline long long coco_words(long long D, long long G) { return D * G + kWalks * ((G + 63) >> 6) + 2 * G; }

__global__ void __launch_bounds__(64 * kCWaves) coco_match_kernel(
    long long P, const int64_t* __restrict__ pair_off, const int64_t* __restrict__ pair_gt, const int64_t* __restrict__ pair_ws,
    long long ws_words, int lds_doubles, const double* __restrict__ det_box, const int64_t* __restrict__ gt_off,
    const double* __restrict__ gt_box, const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_flags,
    const double* __restrict__ area_rng, const double* __restrict__ iou_thr, u64* ws, u64* __restrict__ match, int* err) {
  __shared__ CocoSlice slices[kCWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  CocoSlice& S = slices[wave];
  const u64 below = (1ull << lane) - 1;
  const int wa = lane / kCT, wt = lane % kCT;
  const bool walker = lane < kWalks;
  const double lo_w = walker ? area_rng[2 * wa] : 0.0, hi_w = walker ? area_rng[2 * wa + 1] : 0.0;
  const double thr_w = walker ? iou_thr[wt] : 0.0;

  const long long n_groups = (P + kCWaves - 1) / kCWaves;
  for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const long long p = grp * kCWaves + wave;
    const bool live = p < P;
    const int64_t d0 = live ? pair_off[p] : 0;
    const long long D64 = live ? pair_off[p + 1] - d0 : 0;
    const int64_t g0 = live ? gt_off[pair_gt[p]] : 0;
    const long long G64 = live ? gt_off[pair_gt[p] + 1] - g0 : 0;
    // within these limits D * G and every index below fit an int (255 * (2^23 - 1) < 2^31)
    const bool sized = D64 >= 0 && D64 <= SW_COCO_MAX_PAIR_DETS && G64 >= 0 && G64 <= SW_COCO_MAX_PAIR_GT;
    int D = sized ? (int)D64 : 0;
    int G = sized ? (int)G64 : 0;
    double* iou = S.iou;
    u64* taken = S.taken;
    int* perm = S.perm;
    if (!sized) {
      if (lane == 0) atomicOr(err, 1);
    } else if (!coco_fits(D, G, lds_doubles)) {
      const long long off = pair_ws[p];
      if (off < 0 || off + coco_words(D, G) > ws_words) {      // a region outside the workspace: nothing of the pair is touched
        if (lane == 0) atomicOr(err, 1);
        D = 0;
        G = 0;
      } else {
        iou = reinterpret_cast<double*>(ws + off);
        taken = ws + off + (long long)D * G;
        perm = reinterpret_cast<int*>(taken + kWalks * ((G + 63) >> 6));
      }
    }
    const int W = (G + 63) >> 6;                 // words of a walk's "taken" bitmask

    // SortInstancesByIgnore: per area range the stable partition, non-ignored first; perm[a * G + position] = ground truth
    for (int a = 0; a < kCA; ++a) {
      const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
      int nv = 0;
      for (int b = 0; b < G; b += 64) {
        const int g = b + lane;
        const bool in = g < G;
        const bool ign = in && ((gt_flags[g0 + (in ? g : 0)] & 1) || gt_area[g0 + (in ? g : 0)] < lo || gt_area[g0 + (in ? g : 0)] > hi);
        nv += __popcll(__ballot(in && !ign));
      }
      int cv = 0, ci = 0;
      for (int b = 0; b < G; b += 64) {
        const int g = b + lane;
        const bool in = g < G;
        const bool ign = in && ((gt_flags[g0 + (in ? g : 0)] & 1) || gt_area[g0 + (in ? g : 0)] < lo || gt_area[g0 + (in ? g : 0)] > hi);
        const u64 mv = __ballot(in && !ign), mi = __ballot(in && ign);
        if (in) perm[a * G + (ign ? nv + ci + __popcll(mi & below) : cv + __popcll(mv & below))] = g;
        cv += __popcll(mv);
        ci += __popcll(mi);
      }
      if (lane == 0) S.nvalid[a] = nv;
    }
    for (int k = lane; k < kWalks * W; k += 64) taken[k] = 0;

    // bbIou (maskApi.c): rows are the detections in score order, columns the ground truth in annotation order
    const double2* dbox = reinterpret_cast<const double2*>(det_box) + 2 * d0;
    const double2* gbox = reinterpret_cast<const double2*>(gt_box) + 2 * g0;
    for (int e = lane; e < D * G; e += 64) {
      const int d = e / G, g = e - d * G;
      const double2 dxy = dbox[2 * d], dwh = dbox[2 * d + 1], gxy = gbox[2 * g], gwh = gbox[2 * g + 1];
      const double da = dwh.x * dwh.y, ga = gwh.x * gwh.y;
      double o = 0.0;
      const double w = fmin(dwh.x + dxy.x, gwh.x + gxy.x) - fmax(dxy.x, gxy.x);
      if (!(w <= 0)) {
        const double h = fmin(dwh.y + dxy.y, gwh.y + gxy.y) - fmax(dxy.y, gxy.y);
        if (!(h <= 0)) {
          const double i = w * h;
          const double u = (gt_flags[g0 + g] & 1) ? da : da + ga - i;
          o = i / u;
        }
      }
      iou[e] = o;
    }
    __syncthreads();

    // MatchDetectionsToGroundTruth: lane (a, t) walks the detections in score order
    const int nvalid = walker ? S.nvalid[wa] : 0;
    const int* wperm = perm + (walker ? wa : 0) * G;
    u64* wtaken = taken + (walker ? lane : 0) * W;
    for (int d = 0; d < D; ++d) {
      bool matched = false, ign = false;
      if (walker) {
        double best = fmin(thr_w, 1 - 1e-10);
        int m = -1;
        for (int g = 0; g < G; ++g) {
          const int gi = wperm[g];
          if (((wtaken[g >> 6] >> (g & 63)) & 1) && !(gt_flags[g0 + gi] & 1)) continue;
          if (m >= 0 && m < nvalid && g >= nvalid) break;
          const double o = iou[d * G + gi];
          if (o >= best) {
            best = o;
            m = g;
          }
        }
        if (m >= 0) {
          ign = m >= nvalid;
          matched = (gt_flags[g0 + wperm[m]] & 2) != 0;        // detection_matches holds the ground truth's id: 0 reads as unmatched
          wtaken[m >> 6] |= 1ull << (m & 63);
        }
        if (!matched) {
          const double2 dwh = dbox[2 * d + 1];
          const double area = dwh.x * dwh.y;
          ign = ign || area < lo_w || area > hi_w;
        }
      }
      const u64 mm = __ballot(matched), mi = __ballot(ign);
      if (lane == 0) {
        match[2 * (d0 + d)] = mm;
        match[2 * (d0 + d) + 1] = mi;
      }
    }
    __syncthreads();          // the next group overwrites the slices
  }
}

__global__ void __launch_bounds__(kThreads) coco_accum_kernel(
    int K, const int64_t* __restrict__ cat_off, const int32_t* __restrict__ order, const uint8_t* __restrict__ det_rank,
    const double* __restrict__ det_score, const u64* __restrict__ match, const int64_t* __restrict__ npig,
    const int32_t* __restrict__ max_dets, const double* __restrict__ rec_thr, const int* __restrict__ err,
    double* __restrict__ out) {
  __shared__ u64 sbuf[kThreads];
  __shared__ double mbuf[kThreads];
  __shared__ long long lbuf[kThreads];
  __shared__ long long nr[kCR];
  __shared__ double sprec[kCR], sscore[kCR];
  const int tid = threadIdx.x;
  const int t = blockIdx.x % kCT, m = (blockIdx.x / kCT) % kCM, a = (blockIdx.x / (kCT * kCM)) % kCA;
  const int c = blockIdx.x / (kCT * kCM * kCA);
  const u64 bit = 1ull << (a * kCT + t);
  const long long base = cat_off[c], nd = cat_off[c + 1] - base;
  const int md = max_dets[m];
  const long long np = npig[c * kCA + a];
  const long long stride = (long long)K * kCA * kCM, cell = ((long long)c * kCA + a) * kCM + m;
  double* prec_out = out + (long long)t * kCR * stride + cell;                    // [T][R][K][A][M]
  double* score_out = prec_out + (long long)kCT * kCR * stride;
  double* rec_out = out + 2ll * kCT * kCR * stride + (long long)t * stride + cell;  // [T][K][A][M]
  if (*err != 0 || np == 0) {                    // npig == 0 leaves the -1 the reference initialises with
    const double v = *err != 0 ? NAN : -1.0;
    if (tid < kCR) prec_out[tid * stride] = score_out[tid * stride] = v;
    if (tid == 0) *rec_out = v;
    return;
  }
  if (tid < kCR) {                               // n_r: the smallest n in [0, np + 1] with (double)n / np >= recThrs[r]
    const double thr = rec_thr[tid];
    long long lo = 0, hi = np + 1;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((double)mid / (double)np >= thr) hi = mid;
      else lo = mid + 1;
    }
    nr[tid] = lo;
    sprec[tid] = sscore[tid] = 0.0;
  }

  // TP / FP flag of list position j; in: the detection's in-image rank is below maxDet
  auto flag = [&](long long j, bool& in, int& idx) -> u64 {
    idx = order[base + j];
    in = det_rank[idx] < md;
    if (!in) return 0;
    if (match[2 * (long long)idx + 1] & bit) return 0;
    return (match[2 * (long long)idx] & bit) ? (1ull << 32) : 1ull;
  };

  // pass 1: the totals and the first position that is in the list
  u64 sum = 0;
  long long first = nd;
  for (long long j = tid; j < nd; j += kThreads) {
    bool in;
    int idx;
    sum += flag(j, in, idx);
    if (in && j < first) first = j;
  }
  sbuf[tid] = sum;
  lbuf[tid] = first;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      sbuf[tid] += sbuf[tid + off];
      if (lbuf[tid + off] < lbuf[tid]) lbuf[tid] = lbuf[tid + off];
    }
    __syncthreads();
  }
  const u64 total = sbuf[0];
  first = lbuf[0];
  __syncthreads();

  // pass 2: tiles from the last to the first
  u64 carry = total;                             // the sums through the end of the current tile
  double mcarry = -INFINITY;                     // max precision over the later tiles
  for (long long lo = nd > 0 ? (nd - 1) / kTile * kTile : -1; lo >= 0; lo -= kTile) {
    u64 v[kItems], run = 0;
    bool in[kItems];
    int idx[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const long long j = lo + tid * kItems + k;
      in[k] = false;
      idx[k] = 0;
      v[k] = 0;
      if (j < nd) v[k] = flag(j, in[k], idx[k]);
      run += v[k];
    }
    const BlockScan<u64> sc = block_scan<kThreads>(run, sbuf, ScanAdd());
    const u64 before = carry - sc.total;
    u64 cum = before + sc.incl - run;
    double pr[kItems], tmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      cum += v[k];
      const long long tp = (long long)(cum >> 32), n = tp + (long long)(cum & 0xFFFFFFFFull);
      pr[k] = !in[k] ? -INFINITY : n > 0 ? (double)tp / (double)n : 0.0;
      if (pr[k] > tmax) tmax = pr[k];
    }
    // suffix max over the threads: the scan from the last thread to the first; prev = the max of the threads tid + 1 .. kThreads - 1
    const BlockScan<double> sm = block_scan<kThreads, true>(tmax, mbuf, [](double later, double mine) { return later > mine ? later : mine; });
    double env = tid + 1 < kThreads ? sm.prev : -INFINITY;
    if (mcarry > env) env = mcarry;
    const double tile_max = sm.total;
#pragma unroll
    for (int k = kItems - 1; k >= 0; --k) {
      if (pr[k] > env) env = pr[k];              // the envelope at this position
      if (v[k] == (1ull << 32)) {                // the true positive that brings the count to n: every level with n_r == n reads it
        const long long n = (long long)(cum >> 32);
        int r0 = 0, r1 = kCR;
        while (r0 < r1) {
          const int mid = (r0 + r1) >> 1;
          if (nr[mid] >= n) r1 = mid;
          else r0 = mid + 1;
        }
        for (int r = r0; r < kCR && nr[r] == n; ++r) {
          sprec[r] = env;
          sscore[r] = det_score[idx[k]];
        }
      }
      cum -= v[k];
    }
    if (tile_max > mcarry) mcarry = tile_max;
    carry = before;
  }
  __syncthreads();
  if (tid < kCR) {
    double p = sprec[tid], s = sscore[tid];
    if (nr[tid] == 0 && first < nd) {            // level 0: position 0 of the list
      p = mcarry;
      s = det_score[order[base + first]];
    }
    prec_out[tid * stride] = p;
    score_out[tid * stride] = s;
  }
  if (tid == 0) *rec_out = first < nd ? (double)(long long)(total >> 32) / (double)np : 0.0;
}

}  // namespace

extern "C" long long sw_coco_eval_workspace_bytes(int D, long long G, int lds_doubles) {
  if (D < 0 || D > SW_COCO_MAX_PAIR_DETS || G < 0 || G > SW_COCO_MAX_PAIR_GT || lds_doubles < 0 || lds_doubles > kLdsCap) return -1;
  return coco_fits(D, G, lds_doubles) ? 0 : 8 * coco_words(D, G);
}

extern "C" int sw_coco_eval(int K, long long N, long long P, const int64_t* pair_off, const int64_t* pair_gt,
                            const int64_t* pair_ws, long long ws_bytes, int lds_doubles, const double* det_box,
                            const int64_t* gt_off, const double* gt_box, const double* gt_area, const uint8_t* gt_flags,
                            const double* area_rng, const double* iou_thr, const double* rec_thr, const int32_t* max_dets,
                            const int64_t* cat_off, const int32_t* order, const uint8_t* det_rank, const double* det_score,
                            const int64_t* npig, unsigned long long* match, double* out, void* workspace, hipStream_t stream) {
  SW_ENTER();
  if (K < 1 || K > SW_COCO_MAX_CLASSES) return -6;
  if (N < 0 || N > SW_COCO_MAX_DETS || P < 0 || P > N || ws_bytes < SW_COCO_WS_HEADER || (ws_bytes & 7) != 0 || lds_doubles < 0 ||
      lds_doubles > kLdsCap)
    return -5;
  if (((uintptr_t)det_box & 15) != 0 || ((uintptr_t)gt_box & 15) != 0 || ((uintptr_t)out & 7) != 0 || ((uintptr_t)match & 7) != 0 ||
      ((uintptr_t)workspace & 255) != 0)
    return -4;
  int* err = static_cast<int*>(workspace);
  const hipError_t e = hipMemsetAsync(err, 0, SW_COCO_WS_HEADER, stream);
  if (e != hipSuccess) return (int)e;
  if (P > 0) {
    const long long n_groups = (P + kCWaves - 1) / kCWaves;
    const long long cap = 8ll * sw_cu_count();
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)(n_groups < cap ? n_groups : cap)), dim3(64 * kCWaves), 0, stream, P,
                       pair_off, pair_gt, pair_ws, (ws_bytes - SW_COCO_WS_HEADER) / 8, lds_doubles, det_box, gt_off, gt_box, gt_area,
                       gt_flags, area_rng, iou_thr, reinterpret_cast<u64*>(static_cast<char*>(workspace) + SW_COCO_WS_HEADER), match,
                       err);
    SW_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(coco_accum_kernel, dim3(K * kCA * kCM * kCT), dim3(kThreads), 0, stream, K, cat_off, order, det_rank,
                     det_score, match, npig, max_dets, rec_thr, err, out);
  SW_CHECK_LAUNCH();
  return 0;
}

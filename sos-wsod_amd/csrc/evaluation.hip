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

// inclusive Hillis-Steele scan over the workgroup in thread order; buf[kThreads - 1] holds the total until the next call
template <typename T, typename Op>
__device__ T block_scan(T v, T* buf, Op op) {
  const int tid = threadIdx.x;
  buf[tid] = v;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const bool has = tid >= off;
    T o = buf[has ? tid - off : tid];
    __syncthreads();
    if (has) {
      v = op(o, v);
      buf[tid] = v;
    }
    __syncthreads();
  }
  return v;
}

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
    const unsigned long long incl = block_scan(run, sbuf, [](unsigned long long a, unsigned long long b) { return a + b; });
    const unsigned long long total = sbuf[kThreads - 1];
    const unsigned long long before = carry + incl - run;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const long long d = lo + tid * kItems + k;
      if (d < nd) cum[d] = before + v[k];
    }
    carry += total;
    __syncthreads();
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
    const MaxCount incl = block_scan(run, mbuf, [](MaxCount a, MaxCount b) { return MaxCount{np_max(b.m, a.m), a.n + b.n}; });
    const MaxCount total = mbuf[kThreads - 1];
    double env = tid > 0 ? np_max(mbuf[tid - 1].m, mcarry.m) : mcarry.m;   // max(mpre[i + 1 ..]) above this thread's items
    int pos = mcarry.n + incl.n - run.n;                                      // change points at larger i
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
    __syncthreads();                             // mbuf is read above; the next tile's scan overwrites it
    mcarry.m = np_max(total.m, mcarry.m);
    mcarry.n += total.n;
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

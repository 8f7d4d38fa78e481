// Stage-2 pseudo-ground-truth filtering (reference tools/pgf.py: class_filter :273-292, pgf :221-271, contain_cal :209-219):
// stages 3-5 of a whole split in one launch.
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

// contain_cal(a, b) >= t_con with the a-side terms precomputed: ax2 = a0 + a2, ay2 = a1 + a3, den = area_a + 1e-6
__device__ __forceinline__ bool contained(double a0, double a1, double ax2, double ay2, double den, double2 bxy, double2 bwh,
                                          double t_con) {
  const double bx2 = bxy.x + bwh.x;
  const double by2 = bxy.y + bwh.y;
  const double c0 = py_max(a0, bxy.x);
  const double c1 = py_max(a1, bxy.y);
  const double c2 = py_min(ax2, bx2);
  const double c3 = py_min(ay2, by2);
  const double area_c = py_max(0.0, c2 - c0) * py_max(0.0, c3 - c1);
  return area_c / den >= t_con;
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

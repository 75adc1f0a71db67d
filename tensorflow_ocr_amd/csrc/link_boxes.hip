// Link-geometry detections on the device: what lies between ocr_min_area_rects and ocr_eval_collect.
//
//   ocr_component_scores  labels + pixel scores -> one detection score per component: the mean pixel score over the
//                         component's pixels.  BUILD-DEFINED (the reference gives a link box no score); the matcher walks
//                         detections in descending score order, so the mean must not depend on scheduling: every pixel
//                         score becomes the integer q = rint(clamp(s, 0, 1) * 2^24) (NaN -> 0), the integers and the
//                         pixel count are summed in 64 bits with integer atomics (order-free), and
//                         mean = f32(f64(sum) / f64(count) / 2^24).
//   ocr_link_boxes        hull size, hull head and calipers of ocr_min_area_rects -> the rows ocr_eval_collect reads:
//                         the tail of cv2.minAreaRect (RotatedRect), cv2.boxPoints and np.int0 of
//                         tool/pixellink_fn.py (_rotated_rect, _box_points), operation by operation: f32 adds and
//                         multiplies, sqrt / atan2 / cos / sin and the two divisions by / multiplications with pi in
//                         double, the same casts back to f32 at the same places, truncation toward zero at the end.
//
// Compiled without FMA contraction (Makefile NOFMA): every f32 product is rounded before it is added.
#include <limits.h>
#include "common.h"

namespace {

constexpr unsigned kNoKey = 0xFFFFFFFFu;
constexpr double kPi = 3.14159265358979323846;          // math.pi
constexpr int kMaxComps = 65535, kMaxImages = 65535, kMaxSide = 32768;
constexpr int kThreads = 256;          // every kernel here is launched with workgroups of exactly kThreads lanes (4 full waves)

// grid-stride over the n*h*w pixels, whole waves together.  A wave holds 64 consecutive pixels; lanes that follow
// each other with the same (image, label) form a segment, a segmented scan adds the segment's integers (at most
// 64 * 2^24: 32 bits hold them) and its last lane issues the two atomics — one pair per wave segment, not per pixel.
// acc u64 [n * max_comps][2] = (sum of q, pixel count), zeroed by the caller.
__global__ __launch_bounds__(kThreads) void comp_score_accum_kernel(const int* __restrict__ labels,
                                                               const float* __restrict__ score, size_t hw, size_t total,
                                                               int max_comps, unsigned long long* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  const size_t step = (size_t)gridDim.x * kThreads;
  for (size_t base = (size_t)blockIdx.x * kThreads + (threadIdx.x & ~63); base < total; base += step) {      // wave-uniform
    const size_t i = base + lane;
    unsigned key = kNoKey, q = 0;
    if (i < total) {
      const int L = labels[i];
      if (L >= 1 && L <= max_comps) {
        key = (unsigned)(i / hw) * (unsigned)max_comps + (unsigned)(L - 1);      // < 65535 * 65535 + 65535
        const float s = score[i];
        const float c = s > 0.f ? fminf(s, 1.f) : 0.f;                           // NaN and negatives -> 0
        q = (unsigned)rintf(c * 16777216.f);
      }
    }
    const unsigned prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // (lane 0 is always a head)
    unsigned v = q, c = key != kNoKey ? 1u : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned tv = __shfl_up(v, o, 64), tc = __shfl_up(c, o, 64);
      if (lane - o >= start) { v += tv; c += tc; }
    }
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (tail && key != kNoKey) {
      atomicAdd(acc + 2 * (size_t)key, (unsigned long long)v);
      atomicAdd(acc + 2 * (size_t)key + 1, (unsigned long long)c);
    }
  }
}

__global__ __launch_bounds__(kThreads) void comp_score_mean_kernel(const unsigned long long* __restrict__ acc,
                                                              const int* __restrict__ ncomp, int n, int max_comps,
                                                              float* __restrict__ comp_score) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)n * max_comps) return;
  const int img = (int)(i / max_comps), c = (int)(i % max_comps);
  const int k = min(max(ncomp[img], 0), max_comps);
  float m = 0.f;
  if (c < k) {
    const unsigned long long sum = acc[2 * i], cnt = acc[2 * i + 1];
    if (cnt > 0) m = (float)((double)sum / (double)cnt / 16777216.0);        // an id without pixels scores 0
  }
  comp_score[i] = m;
}

// one thread per (image, component)
__global__ __launch_bounds__(kThreads) void link_boxes_kernel(const int* __restrict__ hull_n, const int* __restrict__ hull_head,
                                                         const float* __restrict__ calipers,
                                                         const float* __restrict__ comp_score,
                                                         const int* __restrict__ ncomp, int n, int max_comps,
                                                         float min_side, float min_area, float* __restrict__ merged,
                                                         int* __restrict__ keep_idx, int* __restrict__ n_keep,
                                                         unsigned char* __restrict__ passed, int* __restrict__ total) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)n * max_comps) return;
  const int img = (int)(i / max_comps), comp = (int)(i % max_comps);
  const int nc = ncomp[img], k = min(max(nc, 0), max_comps);
  if (comp == 0) {
    n_keep[img] = k;
    total[img] = nc;
  }
  keep_idx[i] = comp;
  float* out = merged + i * 9;
  if (comp >= k) {                               // rows at or beyond min(ncomp, max_comps): zeros, not passed
#pragma unroll
    for (int j = 0; j < 9; ++j) out[j] = 0.f;
    passed[i] = 0;
    return;
  }
  // ---- RotatedRect (cx, cy, w, h, angle in degrees): _rotated_rect
  const int nh = hull_n[i];
  float cx = 0.f, cy = 0.f, w = 0.f, h = 0.f, ang = 0.f;
  if (nh > 2) {
    const float* c = calipers + i * 6;
    const float c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5];
    cx = c0 + (c2 + c4) * 0.5f;
    cy = c1 + (c3 + c5) * 0.5f;
    w = (float)sqrt((double)c2 * (double)c2 + (double)c3 * (double)c3);
    h = (float)sqrt((double)c4 * (double)c4 + (double)c5 * (double)c5);
    ang = (float)atan2((double)c3, (double)c2);
  } else if (nh == 2) {
    const int* hd = hull_head + i * 4;
    const float x0 = (float)hd[0], y0 = (float)hd[1], x1 = (float)hd[2], y1 = (float)hd[3];
    cx = (x0 + x1) * 0.5f;
    cy = (y0 + y1) * 0.5f;
    const double dx = (double)(x1 - x0), dy = (double)(y1 - y0);
    w = (float)sqrt(dx * dx + dy * dy);
    ang = (float)atan2(dy, dx);
  } else if (nh == 1) {
    cx = (float)hull_head[i * 4];
    cy = (float)hull_head[i * 4 + 1];
  }
  ang = (float)((double)(ang * 180.f) / kPi);
  // ---- corners: _box_points (RotatedRect::points)
  const double a_ = (double)ang * kPi / 180.;
  const float b = (float)cos(a_) * 0.5f;
  const float a = (float)sin(a_) * 0.5f;
  const float p0x = cx - a * h - b * w;
  const float p0y = cy + b * h - a * w;
  const float p1x = cx + a * h - b * w;
  const float p1y = cy - b * h - a * w;
  const float p2x = 2.f * cx - p0x, p2y = 2.f * cy - p0y;
  const float p3x = 2.f * cx - p1x, p3y = 2.f * cy - p1y;
  out[0] = truncf(p0x); out[1] = truncf(p0y);    // np.int0: toward zero
  out[2] = truncf(p1x); out[3] = truncf(p1y);
  out[4] = truncf(p2x); out[5] = truncf(p2y);
  out[6] = truncf(p3x); out[7] = truncf(p3y);
  out[8] = comp_score[i];
  passed[i] = (nh > 0 && fminf(w, h) >= min_side && w * h >= min_area) ? 1 : 0;
}

unsigned grid_for(size_t items, size_t cap) {
  size_t b = (items + kThreads - 1) / kThreads;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace

extern "C" size_t ocr_component_scores_workspace(int n, int max_comps) {
  if (n <= 0 || max_comps <= 0) return 0;
  return (size_t)n * max_comps * 2 * sizeof(unsigned long long);
}

extern "C" int ocr_component_scores(const void* labels_i32, const void* pixel_score_f32, const void* ncomp_i32, int n,
                                    int h, int w, int max_comps, void* comp_score_f32, void* workspace, size_t ws_bytes,
                                    void* stream) {
  OCR_CHECK_ARG(labels_i32 && pixel_score_f32 && ncomp_i32 && comp_score_f32 && workspace);
  OCR_CHECK_ARG(n > 0 && h > 0 && w > 0 && max_comps > 0);
  OCR_CHECK_SHAPE(n <= kMaxImages && max_comps <= kMaxComps && h <= kMaxSide && w <= kMaxSide);
  const size_t need = ocr_component_scores_workspace(n, max_comps);
  if (ws_bytes < need) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* acc = static_cast<unsigned long long*>(workspace);
  if (hipMemsetAsync(acc, 0, need, st) != hipSuccess) return OCR_ERR_HIP;
  const size_t hw = (size_t)h * w, total = (size_t)n * hw;
  hipLaunchKernelGGL(comp_score_accum_kernel, dim3(grid_for(total, 4096)), dim3(kThreads), 0, st,
                     static_cast<const int*>(labels_i32), static_cast<const float*>(pixel_score_f32), hw, total,
                     max_comps, acc);
  const size_t rows = (size_t)n * max_comps;
  hipLaunchKernelGGL(comp_score_mean_kernel, dim3(grid_for(rows, (size_t)1 << 30)), dim3(kThreads), 0, st, acc,
                     static_cast<const int*>(ncomp_i32), n, max_comps, static_cast<float*>(comp_score_f32));
  return ocr_launch_status();
}

extern "C" int ocr_link_boxes(const void* hull_n_i32, const void* hull_head_i32, const void* calipers_f32,
                              const void* comp_score_f32, const void* ncomp_i32, int n, int max_comps, float min_side,
                              float min_area, void* merged_f32, void* keep_idx_i32, void* n_keep_i32, void* passed_u8,
                              void* total_i32, void* stream) {
  OCR_CHECK_ARG(hull_n_i32 && hull_head_i32 && calipers_f32 && comp_score_f32 && ncomp_i32 && merged_f32 &&
                keep_idx_i32 && n_keep_i32 && passed_u8 && total_i32);
  OCR_CHECK_ARG(n > 0 && max_comps > 0);
  OCR_CHECK_SHAPE(n <= kMaxImages && max_comps <= kMaxComps);
  const size_t rows = (size_t)n * max_comps;
  hipLaunchKernelGGL(link_boxes_kernel, dim3(grid_for(rows, (size_t)1 << 30)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const int*>(hull_n_i32),
                     static_cast<const int*>(hull_head_i32), static_cast<const float*>(calipers_f32),
                     static_cast<const float*>(comp_score_f32), static_cast<const int*>(ncomp_i32), n, max_comps,
                     min_side, min_area, static_cast<float*>(merged_f32), static_cast<int*>(keep_idx_i32),
                     static_cast<int*>(n_keep_i32), static_cast<unsigned char*>(passed_u8),
                     static_cast<int*>(total_i32));
  return ocr_launch_status();
}

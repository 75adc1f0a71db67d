// Held-out evaluation by the ICDAR-2015 Task-1 localisation protocol (polygon IoU, don't-care regions) for all images of
// a batch, the running counters of tool/metrics.py left on the device (include/ocr_eval_ic15.h states the rule).
//
//   ic15_prep_kernel   one thread per polygon: vertices clamped to 2^22, counter-clockwise by the sign of the integer
//                      shoelace sum, kind by the number of negative turns (integer cross products), a reflex vertex
//                      rotated to position 0, the area |sum| / 2 as f64 (exact)
//   ic15_pairs_kernel  one thread per live (image, gt, det) pair: area of the intersection = two Sutherland-Hodgman
//                      clips of the convex quad against the triangles (0,1,2), (0,2,3) of the other one
//   ic15_walk_kernel   one wave per image: don't-care flag of every detection, then the ground-truth-major greedy walk,
//                      64 detections per step, the first lane that satisfies the predicate (ballot) is the match
//
// f64 and integers only; compiled without FMA contraction (Makefile NOFMA).  Every inside test of an INPUT vertex is exact:
// coordinates are integers below 2^23 in magnitude, so differences, their products (< 2^47) and the difference of two
// products are exact in f64.  No atomic takes part in a decision: the record is added to with integer atomics (order-free).
#include "common.h"

namespace {

#pragma clang fp contract(off)

constexpr int kCoordLimit = 4194304;          // 2^22, ocr_eval_collect's clamp
constexpr int kMaxD = 1024;
constexpr int kMaxG = 254;
constexpr int kPairThreads = 128;
constexpr int kClipPts = 8;                   // a quad clipped by three half-planes has at most 7 vertices

enum Kind : int { kConvex = 0, kReflex = 1, kBowTie = 2, kZero = 3 };

// the workspace: inter f64 [n][max_g][max_d] | darea f64 [n][max_d] | garea f64 [n][max_g] | dpoly int32 [n][max_d][8] |
// gpoly int32 [n][max_g][8] | dkind int32 [n][max_d] | gkind int32 [n][max_g]
struct Ws {
  double* inter;
  double* darea;
  double* garea;
  int* dpoly;
  int* gpoly;
  int* dkind;
  int* gkind;
};

__host__ __device__ inline size_t ws_bytes_of(int n, int max_d, int max_g) {
  const size_t nd = (size_t)n * max_d, ng = (size_t)n * max_g;
  return (nd * max_g + nd + ng) * sizeof(double) + (nd + ng) * 9 * sizeof(int);
}

inline Ws carve(void* workspace, int n, int max_d, int max_g) {
  const size_t nd = (size_t)n * max_d, ng = (size_t)n * max_g;
  Ws w;
  w.inter = static_cast<double*>(workspace);
  w.darea = w.inter + nd * max_g;
  w.garea = w.darea + nd;
  w.dpoly = reinterpret_cast<int*>(w.garea + ng);
  w.gpoly = w.dpoly + nd * 8;
  w.dkind = w.gpoly + ng * 8;
  w.gkind = w.dkind + nd;
  return w;
}

__device__ __forceinline__ int clamp_coord(int c) { return min(max(c, -kCoordLimit), kCoordLimit); }

// grid (cdiv(max_d + max_g, 256), n): thread p < max_d is detection p, the others ground truth p - max_d
__global__ __launch_bounds__(256) void ic15_prep_kernel(const int* __restrict__ dets, const int* __restrict__ nd,
                                                        const int* __restrict__ gts, const int* __restrict__ ng, int max_d,
                                                        int max_g, double* __restrict__ darea, double* __restrict__ garea,
                                                        int* __restrict__ dpoly, int* __restrict__ gpoly,
                                                        int* __restrict__ dkind, int* __restrict__ gkind) {
  const int img = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const bool is_det = p < max_d;
  const int k = is_det ? p : p - max_d;
  if (k >= (is_det ? min(max(nd[img], 0), max_d) : min(max(ng[img], 0), max_g))) return;
  const size_t row = is_det ? (size_t)img * max_d + k : (size_t)img * max_g + k;
  const int* src = (is_det ? dets : gts) + row * 8;
  long long x[4], y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { x[i] = clamp_coord(src[2 * i]); y[i] = clamp_coord(src[2 * i + 1]); }
  long long s2 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s2 += x[i] * y[(i + 1) & 3] - x[(i + 1) & 3] * y[i];
  if (s2 < 0) {                               // clockwise: the same polygon walked the other way
    long long t = x[1]; x[1] = x[3]; x[3] = t;
    t = y[1]; y[1] = y[3]; y[3] = t;
  }
  int negative = 0, reflex = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {               // the turn at vertex i
    const int a = (i + 3) & 3, b = (i + 1) & 3;
    const long long turn = (x[i] - x[a]) * (y[b] - y[i]) - (y[i] - y[a]) * (x[b] - x[i]);
    if (turn < 0) { ++negative; reflex = i; }
  }
  const int kind = negative >= 2 ? kBowTie : s2 == 0 ? kZero : negative == 1 ? kReflex : kConvex;
  const int rot = kind == kReflex ? reflex : 0;
  int* out = (is_det ? dpoly : gpoly) + row * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int sx = 0, sy = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)               // x[(i + rot) & 3] without a runtime-indexed private array
      if (((i + rot) & 3) == j) { sx = (int)x[j]; sy = (int)y[j]; }
    out[2 * i] = sx;
    out[2 * i + 1] = sy;
  }
  (is_det ? dkind : gkind)[row] = kind;
  (is_det ? darea : garea)[row] = (double)(s2 < 0 ? -s2 : s2) * 0.5;
}

struct dpt { double x, y; };

__device__ __forceinline__ double cross3(dpt a, dpt b, dpt c) { return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x); }

__device__ __forceinline__ dpt cut(dpt s, dpt e, double ds, double de) {
  const double t = ds / (ds - de);
  dpt r;
  r.x = s.x + t * (e.x - s.x);
  r.y = s.y + t * (e.y - s.y);
  return r;
}

// area of (convex quad q) and (triangle t0 t1 t2, counter-clockwise, not degenerate): Sutherland-Hodgman, the work
// polygons in LDS (coordinate c of point i of thread t at [c][i][t], one bank column per thread; as private arrays they
// are indexed at run time and land in scratch, lanms.hip's quad_iou_lds has the measurement)
__device__ double clip_area(const dpt* q, dpt t0, dpt t1, dpt t2, double* cur, double* nxt) {
  constexpr int S = kPairThreads, Y = kClipPts * kPairThreads;
#pragma unroll
  for (int i = 0; i < 4; ++i) { cur[i * S] = q[i].x; cur[Y + i * S] = q[i].y; }
  int n = 4;
#pragma unroll
  for (int ce = 0; ce < 3; ++ce) {
    const dpt c1 = ce == 0 ? t0 : ce == 1 ? t1 : t2, c2 = ce == 0 ? t1 : ce == 1 ? t2 : t0;
    if (n > 0) {
      int m = 0;
      dpt s = {cur[(n - 1) * S], cur[Y + (n - 1) * S]};
      double ds = cross3(c1, c2, s);
      for (int i = 0; i < n; ++i) {
        const dpt e = {cur[i * S], cur[Y + i * S]};
        const double de = cross3(c1, c2, e);
        const bool sin = ds >= 0.0, ein = de >= 0.0;
        if (sin != ein && m < kClipPts) {      // (the bound never binds for a convex quad; it keeps any input in its column)
          const dpt r = cut(s, e, ds, de);
          nxt[m * S] = r.x; nxt[Y + m * S] = r.y;
          ++m;
        }
        if (ein && m < kClipPts) {
          nxt[m * S] = e.x; nxt[Y + m * S] = e.y;
          ++m;
        }
        s = e;
        ds = de;
      }
      n = m;                                  // at most one vertex more than before: 4 -> 5 -> 6 -> 7
      double* t = cur; cur = nxt; nxt = t;
    }
  }
  if (n < 3) return 0.0;
  double acc = 0.0;
  dpt u = {cur[(n - 1) * S], cur[Y + (n - 1) * S]};
  for (int i = 0; i < n; ++i) {
    const dpt v = {cur[i * S], cur[Y + i * S]};
    acc += u.x * v.y - v.x * u.y;
    u = v;
  }
  return fabs(acc) * 0.5;
}

// grid (cdiv(max_g * max_d, 128), n), one thread per pair, the detection index fastest
__global__ __launch_bounds__(kPairThreads) void ic15_pairs_kernel(const int* __restrict__ nd, const int* __restrict__ ng,
                                                                  int max_d, int max_g, const int* __restrict__ dpoly,
                                                                  const int* __restrict__ gpoly,
                                                                  const int* __restrict__ dkind,
                                                                  const int* __restrict__ gkind,
                                                                  double* __restrict__ inter,
                                                                  double* __restrict__ inter_out) {
  __shared__ double s_poly[2][2 * kClipPts * kPairThreads];      // 32 KiB
  const int img = blockIdx.y;
  const int pair = blockIdx.x * kPairThreads + threadIdx.x;
  const int gi = pair / max_d, di = pair - gi * max_d;
  if (gi >= min(max(ng[img], 0), max_g) || di >= min(max(nd[img], 0), max_d)) return;
  const size_t drow = (size_t)img * max_d + di, grow = (size_t)img * max_g + gi;
  const int dk = dkind[drow], gk = gkind[grow];
  double area = 0.0;
  // a bow-tie or an empty polygon meets nothing; one of the two has to be convex (reflex x reflex: outside the contract)
  if (dk <= kReflex && gk <= kReflex && !(dk == kReflex && gk == kReflex)) {
    int dv[8], gv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { dv[i] = dpoly[drow * 8 + i]; gv[i] = gpoly[grow * 8 + i]; }
    int dx0 = dv[0], dx1 = dv[0], dy0 = dv[1], dy1 = dv[1], gx0 = gv[0], gx1 = gv[0], gy0 = gv[1], gy1 = gv[1];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      dx0 = min(dx0, dv[2 * i]); dx1 = max(dx1, dv[2 * i]); dy0 = min(dy0, dv[2 * i + 1]); dy1 = max(dy1, dv[2 * i + 1]);
      gx0 = min(gx0, gv[2 * i]); gx1 = max(gx1, gv[2 * i]); gy0 = min(gy0, gv[2 * i + 1]); gy1 = max(gy1, gv[2 * i + 1]);
    }
    if (!(dx1 < gx0 || gx1 < dx0 || dy1 < gy0 || gy1 < dy0)) {
      // the convex one is clipped, the other one gives the two triangles
      const bool swap = dk == kReflex;
      dpt q[4], t[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        q[i].x = swap ? gv[2 * i] : dv[2 * i]; q[i].y = swap ? gv[2 * i + 1] : dv[2 * i + 1];
        t[i].x = swap ? dv[2 * i] : gv[2 * i]; t[i].y = swap ? dv[2 * i + 1] : gv[2 * i + 1];
      }
      double* cur = &s_poly[0][threadIdx.x];
      double* nxt = &s_poly[1][threadIdx.x];
      if (cross3(t[0], t[1], t[2]) > 0.0) area += clip_area(q, t[0], t[1], t[2], cur, nxt);     // exact: integers
      if (cross3(t[0], t[2], t[3]) > 0.0) area += clip_area(q, t[0], t[2], t[3], cur, nxt);
    }
  }
  const size_t at = ((size_t)img * max_g + gi) * max_d + di;
  inter[at] = area;
  if (inter_out) inter_out[at] = area;
}

// grid (n), one wave per image
__global__ __launch_bounds__(64) void ic15_walk_kernel(const int* __restrict__ nd, const int* __restrict__ ng,
                                                       const unsigned char* __restrict__ gdontcare, int max_d, int max_g,
                                                       double iou_thr, double area_prec_thr,
                                                       const double* __restrict__ inter, const double* __restrict__ darea,
                                                       const double* __restrict__ garea, const int* __restrict__ gkind,
                                                       int* __restrict__ det_match, int* __restrict__ gt_match,
                                                       unsigned long long* __restrict__ record) {
  __shared__ int s_dm[kMaxD];                 // per detection: -1 free, -2 don't-care, else the ground truth it took
  const int img = blockIdx.x, lane = threadIdx.x;
  const int n_d = min(max(nd[img], 0), max_d), n_g = min(max(ng[img], 0), max_g);
  const unsigned char* gdc = gdontcare + (size_t)img * max_g;
  const double* in = inter + (size_t)img * max_g * max_d;
  const double* da = darea + (size_t)img * max_d;
  const double* ga = garea + (size_t)img * max_g;
  const int* gk = gkind + (size_t)img * max_g;
  int* dm = det_match + (size_t)img * max_d;
  int* gm = gt_match + (size_t)img * max_g;
  // don't-care detections: more than area_prec_thr of the detection lies in one don't-care ground truth
  int care_det = 0;
  for (int d = lane; d < n_d; d += 64) {
    const double a = da[d];
    bool dc = false;
    for (int g = 0; g < n_g; ++g)
      if (gdc[g] != 0 && a > 0.0 && in[(size_t)g * max_d + d] / a > area_prec_thr) dc = true;
    s_dm[d] = dc ? -2 : -1;
    care_det += !dc;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) care_det += __shfl_xor(care_det, o, 64);
  __syncthreads();
  int care_gt = 0, matched = 0;
  for (int g = 0; g < n_g; ++g) {             // uniform over the wave
    int found = -2;
    if (gdc[g] == 0 && gk[g] != kBowTie) {
      ++care_gt;
      found = -1;
      const double a_g = ga[g];
      for (int base = 0; base < n_d; base += 64) {
        const int d = base + lane;
        bool ok = false;
        if (d < n_d && s_dm[d] == -1) {
          const double it = in[(size_t)g * max_d + d];
          const double uni = a_g + da[d] - it;
          ok = uni > 0.0 && it / uni > iou_thr;
        }
        const unsigned long long m = __ballot(ok);
        if (m != 0ull) {
          found = base + (int)__ffsll((long long)m) - 1;
          break;
        }
      }
      if (found >= 0) {
        ++matched;
        if (lane == 0) s_dm[found] = g;
        __syncthreads();                      // uniform: `found` comes from a ballot
      }
    }
    if (lane == 0) gm[g] = found;
  }
  __syncthreads();
  for (int d = lane; d < max_d; d += 64) dm[d] = d < n_d ? s_dm[d] : -1;
  for (int g = n_g + lane; g < max_g; g += 64) gm[g] = -1;
  if (lane == 0) {
    atomicAdd(record + 0, (unsigned long long)care_gt);
    atomicAdd(record + 1, (unsigned long long)matched);
    atomicAdd(record + 2, (unsigned long long)(care_det - matched));
    atomicAdd(record + 3, (unsigned long long)n_d);
  }
}

}  // namespace

extern "C" size_t ocr_eval_ic15_workspace(int n, int max_d, int max_g) {
  if (n <= 0 || max_d <= 0 || max_g <= 0) return 0;
  return ws_bytes_of(n, max_d, max_g);
}

extern "C" int ocr_eval_ic15_match_batch(const void* dets_i32, const void* nd_i32, const void* gts_i32, const void* ng_i32,
                                         const void* gdontcare_u8, int n, int max_d, int max_g, double iou_thr,
                                         double area_prec_thr, void* det_match_i32, void* gt_match_i32, void* inter_f64,
                                         void* record_i64, void* workspace, size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(dets_i32 && nd_i32 && gts_i32 && ng_i32 && gdontcare_u8 && det_match_i32 && gt_match_i32 && record_i64 &&
                workspace && n > 0 && max_d > 0 && max_g > 0);
  OCR_CHECK_SHAPE(max_d <= kMaxD && max_g <= kMaxG && n <= 65535);
  if (ws_bytes < ocr_eval_ic15_workspace(n, max_d, max_g)) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Ws w = carve(workspace, n, max_d, max_g);
  const int* nd = static_cast<const int*>(nd_i32);
  const int* ng = static_cast<const int*>(ng_i32);
  hipLaunchKernelGGL(ic15_prep_kernel, dim3(ocr_cdiv(max_d + max_g, 256), n), dim3(256), 0, st,
                     static_cast<const int*>(dets_i32), nd, static_cast<const int*>(gts_i32), ng, max_d, max_g, w.darea,
                     w.garea, w.dpoly, w.gpoly, w.dkind, w.gkind);
  hipLaunchKernelGGL(ic15_pairs_kernel, dim3(ocr_cdiv(max_g * max_d, kPairThreads), n), dim3(kPairThreads), 0, st, nd, ng,
                     max_d, max_g, w.dpoly, w.gpoly, w.dkind, w.gkind, w.inter, static_cast<double*>(inter_f64));
  hipLaunchKernelGGL(ic15_walk_kernel, dim3(n), dim3(64), 0, st, nd, ng, static_cast<const unsigned char*>(gdontcare_u8),
                     max_d, max_g, iou_thr, area_prec_thr, w.inter, w.darea, w.garea, w.gkind,
                     static_cast<int*>(det_match_i32), static_cast<int*>(gt_match_i32),
                     static_cast<unsigned long long*>(record_i64));
  return ocr_launch_status();
}

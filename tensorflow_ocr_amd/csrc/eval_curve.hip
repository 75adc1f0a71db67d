// Score-threshold sweep and average precision over the outputs of ONE matching pass (include/ocr_eval_curve.h states the
// rule): both matchers decide a detection from the detections before it only (raster rule) or leave, on a score prefix
// of the list, exactly the full-list matches inside the prefix (IC15 rule), so the precision / recall
// curve over detection scores is a count over det_score and the match arrays, no walk is repeated.
//
//   curve_kernel<Rule>   one workgroup per image: per detection a state {absent, care unmatched, care matched} read by the
//                        rule's loader; per threshold the kept detections by ballot and popcount; the order check of the
//                        scores; inclusive prefix counts of care / matched detections (shuffle scan, LDS carry) into the
//                        image's rows of the AP pool
//   ap_terms_kernel      one thread per pool slot: a matched slot counts the care and the matched slots BEFORE it by one
//                        binary search per image (each image's scores are sorted), writes f64(M) / f64(C); the 256 terms
//                        of a workgroup are summed by a fixed tree
//   ap_finish_kernel     one workgroup: the partial sums in a fixed strided order and a fixed tree, divided by G
//
// Integers and f32 compares for the curve, f64 for AP; compiled without FMA contraction (Makefile NOFMA).  No atomic takes
// part in a decision: the curve rows are added to with integer atomics, the order flag is OR-ed into (both order-free).
#include "common.h"

namespace {

#pragma clang fp contract(off)

constexpr int kMaxD = 1024;
constexpr int kMaxG = 254;
constexpr int kMaxT = 64;
constexpr int kCurveThreads = 256;
constexpr int kApThreads = 256;

enum State : int { kAbsent = 0, kCareUnmatched = 1, kCareMatched = 2 };

// the raster rule's outputs: tp / fp uint8 [n][max_d], gignored uint8 [n][max_g]
struct RasterRule {
  const unsigned char* tp;
  const unsigned char* fp;
  const unsigned char* gignored;
  __device__ __forceinline__ int det_state(size_t at) const { return tp[at] != 0 ? kCareMatched : fp[at] != 0 ? kCareUnmatched : kAbsent; }
  __device__ __forceinline__ bool gt_care(size_t at) const { return gignored[at] == 0; }
};

// the IC15 rule's outputs: det_match int32 [n][max_d], gt_match int32 [n][max_g]
struct Ic15Rule {
  const int* det_match;
  const int* gt_match;
  __device__ __forceinline__ int det_state(size_t at) const {
    const int m = det_match[at];
    return m >= 0 ? kCareMatched : m == -1 ? kCareUnmatched : kAbsent;
  }
  __device__ __forceinline__ bool gt_care(size_t at) const { return gt_match[at] != -2; }
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (n), 256 threads = 4 waves per image
template <class Rule>
__global__ __launch_bounds__(kCurveThreads) void curve_kernel(Rule rule, const float* __restrict__ det_score,
                                                              const int* __restrict__ nd, const int* __restrict__ ng,
                                                              const float* __restrict__ thresholds, int max_d, int max_g,
                                                              int T, unsigned long long* __restrict__ curve,
                                                              int* __restrict__ unsorted, float* __restrict__ pool_score,
                                                              int* __restrict__ pool_cum, int* __restrict__ pool_nd) {
  constexpr int kWaves = kCurveThreads / 64;
  __shared__ float s_thr[kMaxT];
  __shared__ int s_kept[kWaves][kMaxT][3];    // per wave and threshold: matched, care unmatched, all kept
  __shared__ int s_wave[kWaves];              // the packed chunk totals of the waves (scan carry)
  __shared__ int s_gt;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_d = min(max(nd[img], 0), max_d), n_g = min(max(ng[img], 0), max_g);
  const float* score = det_score + (size_t)img * max_d;
  if (tid < T) s_thr[tid] = thresholds[tid];
  if (wave == 0) {                            // the care ground truths of the image
    int care = 0;
    for (int g = lane; g < n_g; g += 64) care += rule.gt_care((size_t)img * max_g + g) ? 1 : 0;
    care = wave_sum(care);
    if (lane == 0) s_gt = care;
  }
  __syncthreads();
  int k_matched = 0, k_care = 0, k_all = 0;   // lane t of every wave holds the wave's counts of threshold t
  int carry = 0;                              // care (low 16 bits) and matched (high 16 bits) detections before the chunk
  bool bad = false;
  for (int base = 0; base < max_d; base += kCurveThreads) {      // uniform over the workgroup
    const int d = base + tid;
    const bool live = d < n_d;
    const float s = live ? score[d] : 0.0f;
    const int state = live ? rule.det_state((size_t)img * max_d + d) : kAbsent;
    if (live && d > 0) {                      // collect's order: non-increasing, the NaNs last
      const float p = score[d - 1];
      bad = bad || (p != p ? s == s : s > p);
    }
    for (int t = 0; t < T; ++t) {
      const bool kept = live && s >= s_thr[t];                   // a NaN on either side: not kept
      const int a = __popcll(__ballot(kept && state == kCareMatched));
      const int b = __popcll(__ballot(kept && state == kCareUnmatched));
      const int c = __popcll(__ballot(kept));
      if (lane == t) { k_matched += a; k_care += b; k_all += c; }
    }
    if (pool_cum != nullptr) {                // (uniform) inclusive prefix counts; a NaN-scored detection is absent here
      const bool in_ap = state != kAbsent && s == s;
      int v = (in_ap ? 1 : 0) | (in_ap && state == kCareMatched ? 1 << 16 : 0);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
      }
      if (lane == 63) s_wave[wave] = v;
      __syncthreads();
      int before = carry, total = carry;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int x = s_wave[w];
        if (w < wave) before += x;
        total += x;
      }
      v += before;
      if (d < max_d) {
        const size_t at = (size_t)img * max_d + d;
        pool_cum[2 * at] = v & 0xffff;
        pool_cum[2 * at + 1] = v >> 16;
        pool_score[at] = live ? s : __int_as_float(0x7fc00000);
      }
      carry = total;
      __syncthreads();                        // s_wave is written again in the next chunk
    }
  }
  if (lane < T) { s_kept[wave][lane][0] = k_matched; s_kept[wave][lane][1] = k_care; s_kept[wave][lane][2] = k_all; }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (tid < T) {
    int sum[3] = {0, 0, 0};
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
#pragma unroll
      for (int k = 0; k < 3; ++k) sum[k] += s_kept[w][tid][k];
    unsigned long long* row = curve + 4 * (size_t)tid;
    atomicAdd(row + 0, (unsigned long long)s_gt);
    atomicAdd(row + 1, (unsigned long long)sum[0]);
    atomicAdd(row + 2, (unsigned long long)sum[1]);
    atomicAdd(row + 3, (unsigned long long)sum[2]);
  }
  if (tid == 0) {
    if (any_bad) atomicOr(unsorted, 1);
    if (pool_nd != nullptr) pool_nd[img] = n_d;
  }
}

template <class Rule>
int launch_curve(Rule rule, const void* det_score_f32, const void* nd_i32, const void* ng_i32, const void* thresholds_f32,
                 int n, int max_d, int max_g, int T, void* curve_i64, void* unsorted_i32, void* pool_score_f32,
                 void* pool_cum_i32, void* pool_nd_i32, void* stream) {
  hipLaunchKernelGGL(curve_kernel<Rule>, dim3(n), dim3(kCurveThreads), 0, static_cast<hipStream_t>(stream), rule,
                     static_cast<const float*>(det_score_f32), static_cast<const int*>(nd_i32),
                     static_cast<const int*>(ng_i32), static_cast<const float*>(thresholds_f32), max_d, max_g, T,
                     static_cast<unsigned long long*>(curve_i64), static_cast<int*>(unsorted_i32),
                     static_cast<float*>(pool_score_f32), static_cast<int*>(pool_cum_i32), static_cast<int*>(pool_nd_i32));
  return ocr_launch_status();
}

// how many e < n_e have score[e] before the slot's score s: > s, or >= s for an EARLIER image (the scores are
// non-increasing with the NaNs last, so the predicate holds on a prefix)
__device__ __forceinline__ int count_before(const float* __restrict__ score, int n_e, float s, bool earlier) {
  int lo = 0, hi = n_e;                       // the answer lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float v = score[mid];
    if (earlier ? v >= s : v > s) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// grid (cdiv(n_img * max_d, 256)), one thread per slot; partial[block] = the fixed-tree sum of the block's terms
__global__ __launch_bounds__(kApThreads) void ap_terms_kernel(const float* __restrict__ pool_score,
                                                              const int* __restrict__ pool_cum,
                                                              const int* __restrict__ pool_nd, int n_img, int max_d,
                                                              double* __restrict__ partial) {
  __shared__ double s_term[kApThreads];
  const long long slot = (long long)blockIdx.x * kApThreads + threadIdx.x;
  double term = 0.0;
  if (slot < (long long)n_img * max_d) {
    const int i = (int)(slot / max_d), d = (int)(slot - (long long)i * max_d);
    const int* cum = pool_cum + 2 * (size_t)i * max_d;
    const int n_d = min(max(pool_nd[i], 0), max_d);
    if (d < n_d && cum[2 * d + 1] - (d > 0 ? cum[2 * d - 1] : 0) == 1) {       // a matched slot
      const float s = pool_score[(size_t)i * max_d + d];
      int care = cum[2 * d], matched = cum[2 * d + 1];           // the slot itself and its own image's slots before it
      for (int j = 0; j < n_img; ++j) {
        if (j == i) continue;
        const int c = count_before(pool_score + (size_t)j * max_d, min(max(pool_nd[j], 0), max_d), s, j < i);
        if (c > 0) {
          const int* cj = pool_cum + 2 * ((size_t)j * max_d + (c - 1));
          care += cj[0];
          matched += cj[1];
        }
      }
      term = (double)matched / (double)care;
    }
  }
  s_term[threadIdx.x] = term;
  __syncthreads();
#pragma unroll
  for (int o = kApThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_term[threadIdx.x] += s_term[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = s_term[0];
}

// grid (1): thread t sums partial[t], partial[t + 256], ... in that order, then the fixed tree; ap = sum / G
__global__ __launch_bounds__(kApThreads) void ap_finish_kernel(const double* __restrict__ partial, int n_partial,
                                                               const long long* __restrict__ record,
                                                               double* __restrict__ ap) {
  __shared__ double s_term[kApThreads];
  double acc = 0.0;
  for (int p = threadIdx.x; p < n_partial; p += kApThreads) acc += partial[p];
  s_term[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int o = kApThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_term[threadIdx.x] += s_term[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long g = record[0];
    ap[0] = g > 0 ? s_term[0] / (double)g : 0.0;
  }
}

inline bool pool_ok(const void* a, const void* b, const void* c) { return (a && b && c) || (!a && !b && !c); }

}  // namespace

extern "C" int ocr_eval_curve_init(void* curve_i64, int T, void* unsorted_i32, void* ap_f64, void* stream) {
  OCR_CHECK_ARG(curve_i64 && unsorted_i32);
  OCR_CHECK_SHAPE(T >= 1 && T <= kMaxT);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(curve_i64, 0, (size_t)T * 4 * sizeof(long long), st) != hipSuccess) return OCR_ERR_HIP;
  if (hipMemsetAsync(unsorted_i32, 0, sizeof(int), st) != hipSuccess) return OCR_ERR_HIP;
  if (ap_f64 && hipMemsetAsync(ap_f64, 0, sizeof(double), st) != hipSuccess) return OCR_ERR_HIP;
  return OCR_OK;
}

extern "C" int ocr_eval_curve_batch(const void* tp_u8, const void* fp_u8, const void* det_score_f32, const void* nd_i32,
                                    const void* ng_i32, const void* gignored_u8, const void* thresholds_f32, int n, int max_d,
                                    int max_g, int T, void* curve_i64, void* unsorted_i32, void* pool_score_f32,
                                    void* pool_cum_i32, void* pool_nd_i32, void* stream) {
  OCR_CHECK_ARG(tp_u8 && fp_u8 && det_score_f32 && nd_i32 && ng_i32 && gignored_u8 && thresholds_f32 && curve_i64 &&
                unsorted_i32 && pool_ok(pool_score_f32, pool_cum_i32, pool_nd_i32) && n > 0 && max_d > 0 && max_g > 0);
  OCR_CHECK_SHAPE(max_d <= kMaxD && max_g <= kMaxG && n <= 65535 && T >= 1 && T <= kMaxT);
  const RasterRule rule = {static_cast<const unsigned char*>(tp_u8), static_cast<const unsigned char*>(fp_u8),
                           static_cast<const unsigned char*>(gignored_u8)};
  return launch_curve(rule, det_score_f32, nd_i32, ng_i32, thresholds_f32, n, max_d, max_g, T, curve_i64, unsorted_i32,
                      pool_score_f32, pool_cum_i32, pool_nd_i32, stream);
}

extern "C" int ocr_eval_ic15_curve_batch(const void* det_match_i32, const void* gt_match_i32, const void* det_score_f32,
                                         const void* nd_i32, const void* ng_i32, const void* thresholds_f32, int n, int max_d,
                                         int max_g, int T, void* curve_i64, void* unsorted_i32, void* pool_score_f32,
                                         void* pool_cum_i32, void* pool_nd_i32, void* stream) {
  OCR_CHECK_ARG(det_match_i32 && gt_match_i32 && det_score_f32 && nd_i32 && ng_i32 && thresholds_f32 && curve_i64 &&
                unsorted_i32 && pool_ok(pool_score_f32, pool_cum_i32, pool_nd_i32) && n > 0 && max_d > 0 && max_g > 0);
  OCR_CHECK_SHAPE(max_d <= kMaxD && max_g <= kMaxG && n <= 65535 && T >= 1 && T <= kMaxT);
  const Ic15Rule rule = {static_cast<const int*>(det_match_i32), static_cast<const int*>(gt_match_i32)};
  return launch_curve(rule, det_score_f32, nd_i32, ng_i32, thresholds_f32, n, max_d, max_g, T, curve_i64, unsorted_i32,
                      pool_score_f32, pool_cum_i32, pool_nd_i32, stream);
}

extern "C" size_t ocr_eval_ap_workspace(int n_img, int max_d) {
  if (n_img <= 0 || max_d <= 0) return 0;
  return (((size_t)n_img * max_d + kApThreads - 1) / kApThreads) * sizeof(double);
}

extern "C" int ocr_eval_ap(const void* pool_score_f32, const void* pool_cum_i32, const void* pool_nd_i32, int n_img,
                           int max_d, const void* record_i64, void* ap_f64, void* workspace, size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(pool_score_f32 && pool_cum_i32 && pool_nd_i32 && record_i64 && ap_f64 && workspace && n_img > 0 && max_d > 0);
  OCR_CHECK_SHAPE(max_d <= kMaxD && n_img <= 65535);
  if (ws_bytes < ocr_eval_ap_workspace(n_img, max_d)) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int n_partial = (int)(((size_t)n_img * max_d + kApThreads - 1) / kApThreads);      // at most 65535 * 4
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(ap_terms_kernel, dim3(n_partial), dim3(kApThreads), 0, st, static_cast<const float*>(pool_score_f32),
                     static_cast<const int*>(pool_cum_i32), static_cast<const int*>(pool_nd_i32), n_img, max_d, partial);
  hipLaunchKernelGGL(ap_finish_kernel, dim3(1), dim3(kApThreads), 0, st, partial, n_partial,
                     static_cast<const long long*>(record_i64), static_cast<double*>(ap_f64));
  return ocr_launch_status();
}

// Held-out evaluation on the device: the detection list of a batch and the reference's detection / ground-truth
// matching (tool/bboxes.py: bboxes_matching :171-240 on np_bboxes_jaccard :246-283) for all images of a batch, with
// the running counters of tool/metrics.py left on the device.
//
//   ocr_eval_collect      LANMS output (merged rows, keep list, optional mean-score mask) -> per image the kept quads
//                         divided by the resize ratios and truncated to int32, in descending score order (stable)
//   ocr_eval_match_batch  pixel counts of every detection x ground-truth pair of every image (the raster of raster.h,
//                         as ocr_quad_iou), then one workgroup per image walks its detections in order: first-maximum
//                         argmax of the f32 Jaccard row, tp / fp / matched flags as the reference's loop body
//   ocr_eval_record_init  zeroes the int64 [4] record {ground truths not ignored, tp, fp, detections}
//
// f32 and integers only; compiled without FMA contraction (Makefile NOFMA), the division is __fdiv_rn.  No atomic
// takes part in an ordering decision: the collect pass places a row by its rank, the record is added to with integer
// atomics (order-free).
#include "raster.h"

namespace {

constexpr float kCoordLimit = 4194304.f;      // 2^22, as ocr_quad_mean_score: keeps the raster's 16.16 arithmetic in range
constexpr int kCollectThreads = 256;
constexpr int kMaxD = 1024;
constexpr int kMaxG = 254;

// does row a (score sa, keep position ja) come before row b?  Descending score, ties in keep order; NaN scores last
// (the order of np.argsort(-score, kind="stable"))
__device__ __forceinline__ bool comes_before(float sa, int ja, float sb, int jb) {
  const bool an = sa != sa, bn = sb != sb;
  if (an || bn) return (!an && bn) || (an && bn && ja < jb);
  return sa > sb || (sa == sb && ja < jb);
}

__device__ __forceinline__ int to_pixel(float c, float ratio) {
  const float q = __fdiv_rn(c, ratio);
  if (!isfinite(q)) return 0;
  return (int)fminf(fmaxf(truncf(q), -kCoordLimit), kCoordLimit);
}

// grid (n), one workgroup per image.  A row's output slot is its rank among the passing rows: chunks of the (score,
// passes) list go through LDS and every thread counts the rows in front of its own.
__global__ __launch_bounds__(kCollectThreads) void eval_collect_kernel(
    const float* __restrict__ merged, const int* __restrict__ keep_idx, const int* __restrict__ n_keep,
    const unsigned char* __restrict__ passed, const float* __restrict__ inv_ratio, int max_k, int max_d,
    int* __restrict__ dets, float* __restrict__ det_score, int* __restrict__ nd, int* __restrict__ nd_total) {
  __shared__ float s_score[kCollectThreads];
  __shared__ int s_ok[kCollectThreads];
  __shared__ int s_cnt[kCollectThreads / 64];
  const int img = blockIdx.x, tid = threadIdx.x;
  const float* mrg = merged + (size_t)img * max_k * 9;
  const int* keep = keep_idx + (size_t)img * max_k;
  const unsigned char* pass = passed ? passed + (size_t)img * max_k : nullptr;
  const int nk = min(max(n_keep[img], 0), max_k);
  const float rw = inv_ratio[2 * img], rh = inv_ratio[2 * img + 1];
  int* out = dets + (size_t)img * max_d * 8;
  float* out_s = det_score + (size_t)img * max_d;
  int n_pass = 0;
  for (int base = 0; base < nk; base += kCollectThreads) {
    const int j = base + tid;
    int row = -1;
    float sc = 0.f;
    if (j < nk && (!pass || pass[j])) {
      const int r = keep[j];
      if (r >= 0 && r < max_k) { row = r; sc = mrg[(size_t)r * 9 + 8]; }      // an index outside the list is dropped
    }
    n_pass += row >= 0;
    int rank = 0;
    for (int cb = 0; cb < nk; cb += kCollectThreads) {
      __syncthreads();
      const int c = cb + tid;
      int ok = 0;
      float cs = 0.f;
      if (c < nk && (!pass || pass[c])) {
        const int r = keep[c];
        if (r >= 0 && r < max_k) { ok = 1; cs = mrg[(size_t)r * 9 + 8]; }
      }
      s_score[tid] = cs;
      s_ok[tid] = ok;
      __syncthreads();
      const int lim = min(kCollectThreads, nk - cb);
      if (row >= 0)
        for (int k = 0; k < lim; ++k) rank += s_ok[k] && comes_before(s_score[k], cb + k, sc, j);
    }
    if (row >= 0 && rank < max_d) {
      const float* q = mrg + (size_t)row * 9;
#pragma unroll
      for (int k = 0; k < 8; ++k) out[(size_t)rank * 8 + k] = to_pixel(q[k], (k & 1) ? rh : rw);
      out_s[rank] = sc;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_pass += __shfl_xor(n_pass, o, 64);
  __syncthreads();
  if ((tid & 63) == 0) s_cnt[tid >> 6] = n_pass;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int w = 0; w < kCollectThreads / 64; ++w) t += s_cnt[w];
    nd_total[img] = t;
    nd[img] = min(t, max_d);
  }
}

// grid (max_g, max_d, n), one workgroup per pair (ocr_quad_iou's walk over the pair's bounding box); pairs at or
// beyond nd[img] / ng[img] leave at once.  counts int32 [n][max_d][max_g][2] = (inter, union).
__global__ __launch_bounds__(256) void eval_pairs_kernel(const int* __restrict__ dets, const int* __restrict__ nd,
                                                         const int* __restrict__ gts, const int* __restrict__ ng,
                                                         int max_d, int max_g, int mask_h, int mask_w,
                                                         int* __restrict__ counts) {
  __shared__ raster::Seg s_seg[2][4];
  __shared__ raster::FillEdge s_edge[2][4];
  __shared__ int s_fill[2];
  __shared__ int s_box[4];
  __shared__ int s_cnt[2][4];
  const int gi = blockIdx.x, di = blockIdx.y, img = blockIdx.z;
  if (di >= min(nd[img], max_d) || gi >= min(ng[img], max_g)) return;           // uniform over the workgroup
  const int* pv[2] = {dets + ((size_t)img * max_d + di) * 8, gts + ((size_t)img * max_g + gi) * 8};
  if (threadIdx.x < 8) {
    const int which = threadIdx.x >> 2, e = threadIdx.x & 3;
    const int* v = pv[which];
    const int e0 = (e + 3) & 3;
    raster::Seg sg;
    raster::FillEdge fe;
    raster::setup_edge(v[2 * e0], v[2 * e0 + 1], v[2 * e], v[2 * e + 1], mask_w, mask_h, sg, fe);
    s_seg[which][e] = sg;
    s_edge[which][e] = fe;
  }
  __syncthreads();
  if (threadIdx.x < 2) s_fill[threadIdx.x] = raster::fill_enabled(s_edge[threadIdx.x], 4, mask_w, mask_h) ? 1 : 0;
  if (threadIdx.x == 2) {
    int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
    for (int w = 0; w < 2; ++w)
      for (int k = 0; k < 4; ++k) {
        x0 = min(x0, pv[w][2 * k]); x1 = max(x1, pv[w][2 * k]);
        y0 = min(y0, pv[w][2 * k + 1]); y1 = max(y1, pv[w][2 * k + 1]);
      }
    s_box[0] = max(x0 - 1, 0);
    s_box[1] = max(y0 - 1, 0);
    s_box[2] = min(x1 + 1, mask_w - 1);
    s_box[3] = min(y1 + 1, mask_h - 1);
  }
  __syncthreads();
  const int bx0 = s_box[0], by0 = s_box[1], bw = s_box[2] - bx0 + 1, bh = s_box[3] - by0 + 1;
  int ci = 0, cu = 0;
  if (bw > 0 && bh > 0) {
    const long long total = (long long)bw * bh;
    for (long long i = threadIdx.x; i < total; i += 256) {
      const int y = by0 + (int)(i / bw), x = bx0 + (int)(i % bw);
      const bool a = raster::covers(s_seg[0], s_edge[0], 4, s_fill[0] != 0, x, y);
      const bool b = raster::covers(s_seg[1], s_edge[1], 4, s_fill[1] != 0, x, y);
      ci += a && b;
      cu += a || b;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ci += __shfl_xor(ci, o, 64);
    cu += __shfl_xor(cu, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_cnt[0][threadIdx.x >> 6] = ci;
    s_cnt[1][threadIdx.x >> 6] = cu;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int* c = counts + (((size_t)img * max_d + di) * max_g + gi) * 2;
    c[0] = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
    c[1] = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
  }
}

// np.argmax's order on (value, index): a NaN is the maximum, among equals the smaller index wins
__device__ __forceinline__ bool argmax_better(float va, int ia, float vb, int ib) {
  const bool an = va != va, bn = vb != vb;
  if (an) return !bn || ia < ib;
  if (bn) return false;
  return va > vb || (va == vb && ia < ib);
}

// grid (n), one wave per image: the reference's loop over the detections in their given order
__global__ __launch_bounds__(64) void eval_greedy_kernel(const int* __restrict__ counts, const int* __restrict__ nd,
                                                         const int* __restrict__ ng,
                                                         const unsigned char* __restrict__ gignored, int max_d,
                                                         int max_g, float threshold, unsigned char* __restrict__ tp,
                                                         unsigned char* __restrict__ fp,
                                                         unsigned long long* __restrict__ record) {
  __shared__ unsigned char s_match[kMaxG + 2];
  __shared__ unsigned char s_ign[kMaxG + 2];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int n_d = min(max(nd[img], 0), max_d), n_g = min(max(ng[img], 0), max_g);
  int live = 0;
  for (int k = lane; k < n_g; k += 64) {
    const unsigned char ig = gignored[(size_t)img * max_g + k] != 0;
    s_match[k] = 0;
    s_ign[k] = ig;
    live += !ig;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) live += __shfl_xor(live, o, 64);
  __syncthreads();
  unsigned char* tpi = tp + (size_t)img * max_d;
  unsigned char* fpi = fp + (size_t)img * max_d;
  int n_tp = 0, n_fp = 0;
  for (int d = 0; d < n_d; ++d) {
    int is_tp = 0, is_fp = 1;                 // no ground truth at all: a false positive (build-defined, see the header)
    if (n_g > 0) {
      const int* row = counts + ((size_t)img * max_d + d) * max_g * 2;
      float best = -INFINITY;
      int best_i = INT_MAX;
      for (int k = lane; k < n_g; k += 64) {
        const float jac = (float)((double)row[2 * k] / (double)row[2 * k + 1]);     // 0 / 0 -> NaN
        if (argmax_better(jac, k, best, best_i)) { best = jac; best_i = k; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        if (argmax_better(ov, oi, best, best_i)) { best = ov; best_i = oi; }
      }
      const bool match = best > threshold;    // NaN: false
      const bool existing = s_match[best_i] != 0, not_ignored = s_ign[best_i] == 0;
      is_tp = not_ignored && match && !existing;
      is_fp = not_ignored && (existing || !match);
      __syncthreads();                        // every lane has read the flag
      if (lane == 0 && not_ignored && match) s_match[best_i] = 1;
      __syncthreads();
    }
    if (lane == 0) { tpi[d] = (unsigned char)is_tp; fpi[d] = (unsigned char)is_fp; }
    n_tp += is_tp;
    n_fp += is_fp;
  }
  for (int d = n_d + lane; d < max_d; d += 64) { tpi[d] = 0; fpi[d] = 0; }
  if (lane == 0) {
    atomicAdd(record + 0, (unsigned long long)live);
    atomicAdd(record + 1, (unsigned long long)n_tp);
    atomicAdd(record + 2, (unsigned long long)n_fp);
    atomicAdd(record + 3, (unsigned long long)n_d);
  }
}

}  // namespace

extern "C" int ocr_eval_collect(const void* merged_f32, const void* keep_idx_i32, const void* n_keep_i32,
                                const void* passed_u8, const void* inv_ratio_f32, int n, int max_k, int max_d,
                                void* dets_i32, void* det_score_f32, void* nd_i32, void* nd_total_i32, void* stream) {
  OCR_CHECK_ARG(merged_f32 && keep_idx_i32 && n_keep_i32 && inv_ratio_f32 && dets_i32 && det_score_f32 && nd_i32 &&
                nd_total_i32 && n > 0 && max_k > 0 && max_d > 0);
  OCR_CHECK_SHAPE(max_d <= kMaxD && n <= 65535);
  hipLaunchKernelGGL(eval_collect_kernel, dim3(n), dim3(kCollectThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(merged_f32), static_cast<const int*>(keep_idx_i32),
                     static_cast<const int*>(n_keep_i32), static_cast<const unsigned char*>(passed_u8),
                     static_cast<const float*>(inv_ratio_f32), max_k, max_d, static_cast<int*>(dets_i32),
                     static_cast<float*>(det_score_f32), static_cast<int*>(nd_i32), static_cast<int*>(nd_total_i32));
  return ocr_launch_status();
}

extern "C" size_t ocr_eval_match_workspace(int n, int max_d, int max_g) {
  if (n <= 0 || max_d <= 0 || max_g <= 0) return 0;
  return (size_t)n * max_d * max_g * 2 * sizeof(int);
}

extern "C" int ocr_eval_match_batch(const void* dets_i32, const void* nd_i32, const void* gts_i32, const void* ng_i32,
                                    const void* gignored_u8, int n, int max_d, int max_g, float threshold, int mask_h,
                                    int mask_w, void* tp_u8, void* fp_u8, void* record_i64, void* workspace,
                                    size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(dets_i32 && nd_i32 && gts_i32 && ng_i32 && gignored_u8 && tp_u8 && fp_u8 && record_i64 && workspace &&
                n > 0 && max_d > 0 && max_g > 0 && mask_h > 0 && mask_w > 0);
  OCR_CHECK_SHAPE(max_d <= kMaxD && max_g <= kMaxG && n <= 65535 && mask_h <= 32768 && mask_w <= 32768);
  if (ws_bytes < ocr_eval_match_workspace(n, max_d, max_g)) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* counts = static_cast<int*>(workspace);
  hipLaunchKernelGGL(eval_pairs_kernel, dim3(max_g, max_d, n), dim3(256), 0, st, static_cast<const int*>(dets_i32),
                     static_cast<const int*>(nd_i32), static_cast<const int*>(gts_i32), static_cast<const int*>(ng_i32),
                     max_d, max_g, mask_h, mask_w, counts);
  hipLaunchKernelGGL(eval_greedy_kernel, dim3(n), dim3(64), 0, st, static_cast<const int*>(counts),
                     static_cast<const int*>(nd_i32), static_cast<const int*>(ng_i32),
                     static_cast<const unsigned char*>(gignored_u8), max_d, max_g, threshold,
                     static_cast<unsigned char*>(tp_u8), static_cast<unsigned char*>(fp_u8),
                     static_cast<unsigned long long*>(record_i64));
  return ocr_launch_status();
}

extern "C" int ocr_eval_record_init(void* record_i64, void* stream) {
  OCR_CHECK_ARG(record_i64);
  return hipMemsetAsync(record_i64, 0, 4 * sizeof(long long), static_cast<hipStream_t>(stream)) == hipSuccess
             ? OCR_OK : OCR_ERR_HIP;
}

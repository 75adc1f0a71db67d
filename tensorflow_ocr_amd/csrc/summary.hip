// Training summaries: per-variable statistics and TensorFlow-default histograms of a flat f32 buffer in one
// segmented pass, and tf.summary.image's float -> u8 rule (ocr_tensor_stats_*, ocr_summary_image_u8,
// include/ocr_hip.h).
//
// Reference: tf.summary.histogram / scalar per variable and summed gradient (train_pixellink.py:179-194), the
// image summaries of multigpu_train.py:49-65.  The reference pays for a summary with a second train step on the
// same batch (multigpu_train.py:189-194); here the gradients of the step just taken are still in the flat gradient
// buffer, so one read of the two flat buffers yields every record.  Nothing below is part of a recorded step plan.
#include <cfloat>
#include <cmath>
#include <cstddef>

#include "common.h"

namespace {

constexpr int kPos = OCR_TENSOR_STATS_POS_LIMITS;    // 775 positive limits: 774 from the recurrence, then DBL_MAX
constexpr int kNB = OCR_TENSOR_STATS_BUCKETS;        // 1551 = 2 * 775 + 1
constexpr int kChunk = OCR_TENSOR_STATS_CHUNK;       // elements per unit of work
constexpr unsigned kMagic = 0x53544154u;             // "STAT"
constexpr unsigned kStatsGrid = 2048;                // persistent workgroups: 8 per CU at 12.5 KB of LDS each

struct StatsHeader {
  int n_segments, n_chunks, chunk;
  unsigned magic;
};
struct StatsSeg {
  long long offset, size;
  int first_chunk, n_chunks;
};
// the table: StatsHeader | double limits[kPos] | StatsSeg seg[n_segments]
struct Partial {                 // one per chunk, in the caller's workspace
  double sum, sum_squares;
  float min, max;
  unsigned num, nonfinite;
};
static_assert(sizeof(StatsHeader) == 16 && sizeof(StatsSeg) == 24 && sizeof(Partial) == 32, "table layout");
static_assert(sizeof(ocr_tensor_stats_record) % 8 == 0 && offsetof(ocr_tensor_stats_record, bucket) == 32, "record layout");

__host__ __device__ inline const double* table_limits(const void* table) {
  return reinterpret_cast<const double*>(static_cast<const char*>(table) + sizeof(StatsHeader));
}
__host__ __device__ inline const StatsSeg* table_segs(const void* table) {
  return reinterpret_cast<const StatsSeg*>(static_cast<const char*>(table) + sizeof(StatsHeader) + kPos * sizeof(double));
}

__device__ __forceinline__ bool stats_nonfinite(float v) {          // exponent field all ones: inf or NaN
  return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
}

// The reductions below run in a fixed order (shuffle tree inside a wave, waves 0..3 in turn): the same bits on every call.
struct Acc {
  double sum, sq;
  float mn, mx;
  unsigned num, nf;
};
__device__ __forceinline__ Acc acc_zero() { return Acc{0.0, 0.0, FLT_MAX, -FLT_MAX, 0u, 0u}; }
__device__ __forceinline__ void acc_join(Acc& a, const Acc& b) {
  a.sum += b.sum;
  a.sq += b.sq;
  a.mn = b.mn < a.mn ? b.mn : a.mn;
  a.mx = b.mx > a.mx ? b.mx : a.mx;
  a.num += b.num;
  a.nf += b.nf;
}
__device__ __forceinline__ Acc block_join_256(Acc a, Acc* sh) {       // result valid in thread 0
  for (int o = 32; o > 0; o >>= 1) {
    Acc b;
    b.sum = __shfl_down(a.sum, o, 64);
    b.sq = __shfl_down(a.sq, o, 64);
    b.mn = __shfl_down(a.mn, o, 64);
    b.mx = __shfl_down(a.mx, o, 64);
    b.num = __shfl_down(a.num, o, 64);
    b.nf = __shfl_down(a.nf, o, 64);
    acc_join(a, b);
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sh[0];
    acc_join(a, sh[1]);
    acc_join(a, sh[2]);
    acc_join(a, sh[3]);
  }
  __syncthreads();                                                    // sh is free again
  return a;
}

// upper_bound(limits, (double)v) over the mirrored list [-pos reversed | 0 | pos], from one search of |v| in pos:
//   v >= 0 (and -0):  776 + #{pos <= v}      v < 0:  775 - #{pos < |v|}
// #{...} <= 774 for every finite float (pos[774] = DBL_MAX).
__device__ __forceinline__ int bucket_of(float v, const double* __restrict__ pos) {
  const bool neg = v < 0.f;
  const double a = fabs((double)v);
  int base = 0, len = kPos;
  while (len > 1) {
    const int half = len >> 1;
    const double p = pos[base + half - 1];
    if (neg ? p < a : p <= a) base += half;
    len -= half;
  }
  const double p = pos[base];
  base += (neg ? p < a : p <= a) ? 1 : 0;
  return neg ? kPos - base : kPos + 1 + base;
}

__device__ __forceinline__ void take(float x, float mul, Acc& a, unsigned* hist, const double* pos) {
  const float v = x * mul;                     // the product the optimiser forms, in f32
  if (stats_nonfinite(v)) {
    ++a.nf;
    return;
  }
  ++a.num;
  a.mn = v < a.mn ? v : a.mn;
  a.mx = v > a.mx ? v : a.mx;
  const double d = (double)v;
  a.sum += d;
  a.sq += d * d;
  atomicAdd(&hist[bucket_of(v, pos)], 1u);     // LDS, integer: order-independent
}

// A table that does not describe this call (other n_segments, not a table at all) or more chunks than the workspace holds:
// nothing is read or written through it; stats_final_kernel marks every record instead.
__device__ __forceinline__ bool table_ok(const StatsHeader& h, int n_segments, unsigned cap) {
  return h.magic == kMagic && h.chunk == kChunk && h.n_segments == n_segments && h.n_chunks >= n_segments &&
         (unsigned)h.n_chunks <= cap;
}

__global__ __launch_bounds__(256) void stats_chunk_kernel(const float* __restrict__ x, const void* __restrict__ table,
                                                          int n_segments, float mul_host, const float* __restrict__ mul_dev,
                                                          ocr_tensor_stats_record* __restrict__ rec,
                                                          Partial* __restrict__ partial, unsigned cap) {
  __shared__ double pos[kPos];
  __shared__ unsigned hist[kNB];
  __shared__ Acc sh[4];
  const StatsHeader h = *static_cast<const StatsHeader*>(table);
  if (!table_ok(h, n_segments, cap) || (int)blockIdx.x >= h.n_chunks) return;          // uniform
  const StatsSeg* segs = table_segs(table);
  const double* lim = table_limits(table);
  for (int i = threadIdx.x; i < kPos; i += 256) pos[i] = lim[i];
  for (int i = threadIdx.x; i < kNB; i += 256) hist[i] = 0u;
  const float mul = mul_host * (mul_dev ? *mul_dev : 1.f);
  __syncthreads();
  for (int c = blockIdx.x; c < h.n_chunks; c += gridDim.x) {
    int lo = 0, hi = n_segments - 1;                    // the last segment whose first chunk is <= c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
    }
    const StatsSeg s = segs[lo];
    const long long start = (long long)(c - s.first_chunk) * kChunk;
    long long len = s.size - start;
    if (len > kChunk) len = kChunk;
    const float* p = x + s.offset + start;
    int head = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);          // elements in front of the first 16-byte boundary
    if (head > len) head = (int)len;
    const int n4 = (int)((len - head) >> 2), tail = (int)((len - head) & 3);
    Acc a = acc_zero();
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    for (int i = threadIdx.x; i < n4; i += 256) {
      const float4 v = p4[i];
      take(v.x, mul, a, hist, pos);
      take(v.y, mul, a, hist, pos);
      take(v.z, mul, a, hist, pos);
      take(v.w, mul, a, hist, pos);
    }
    if ((int)threadIdx.x < head) take(p[threadIdx.x], mul, a, hist, pos);
    if ((int)threadIdx.x < tail) take(p[head + (n4 << 2) + threadIdx.x], mul, a, hist, pos);
    a = block_join_256(a, sh);                                          // (its barriers: every LDS add above has landed)
    if (threadIdx.x == 0) partial[c] = Partial{a.sum, a.sq, a.mn, a.mx, a.num, a.nf};
    unsigned* out = rec[lo].bucket;
    for (int i = threadIdx.x; i < kNB; i += 256) {
      const unsigned n = hist[i];
      if (n) {
        __hip_atomic_fetch_add(&out[i], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        hist[i] = 0u;
      }
    }
    __syncthreads();
  }
}

// One workgroup per segment: its chunks' partials in a fixed order (thread t takes t, t + 256, ... rising, then the tree).
__global__ __launch_bounds__(256) void stats_final_kernel(const void* __restrict__ table, int n_segments,
                                                          ocr_tensor_stats_record* __restrict__ rec,
                                                          const Partial* __restrict__ partial, unsigned cap) {
  __shared__ Acc sh[4];
  const StatsHeader h = *static_cast<const StatsHeader*>(table);
  ocr_tensor_stats_record* r = rec + blockIdx.x;
  if (!table_ok(h, n_segments, cap)) {
    if (threadIdx.x == 0) {
      r->sum = r->sum_squares = NAN;
      r->min = r->max = NAN;
      r->num = 0u;
      r->nonfinite = 0xffffffffu;
    }
    return;
  }
  const StatsSeg s = table_segs(table)[blockIdx.x];
  Acc a = acc_zero();
  for (int i = threadIdx.x; i < s.n_chunks; i += 256) {
    const Partial q = partial[s.first_chunk + i];
    acc_join(a, Acc{q.sum, q.sum_squares, q.min, q.max, q.num, q.nonfinite});
  }
  a = block_join_256(a, sh);
  if (threadIdx.x != 0) return;
  r->sum = a.sum;
  r->sum_squares = a.sq;
  r->min = a.num ? a.mn : 0.f;
  r->max = a.num ? a.mx : 0.f;
  r->num = a.num;
  r->nonfinite = a.nf;
}

// ---- image summaries ---------------------------------------------------------------------------------------------
constexpr int kImgGrid = 64;

__device__ __forceinline__ void minmax_join_256(float& mn, float& mx, float* sh) {      // result in every thread
  for (int o = 32; o > 0; o >>= 1) {
    const float a = __shfl_down(mn, o, 64), b = __shfl_down(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = mn;
    sh[4 + (threadIdx.x >> 6)] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
  mx = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
}

__global__ __launch_bounds__(256) void image_minmax_kernel(const float* __restrict__ x, int n, float* __restrict__ part) {
  __shared__ float sh[8];
  float mn = FLT_MAX, mx = -FLT_MAX;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float v = x[i];
    if (!stats_nonfinite(v)) {
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
    }
  }
  minmax_join_256(mn, mx, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = mn;
    part[kImgGrid + blockIdx.x] = mx;
  }
}

__global__ __launch_bounds__(256) void image_u8_kernel(const float* __restrict__ x, int n, const float* __restrict__ part,
                                                       unsigned char* __restrict__ out) {
  __shared__ float sh[8];
  float mn = FLT_MAX, mx = -FLT_MAX;
  if (threadIdx.x < kImgGrid) {
    mn = part[threadIdx.x];
    mx = part[kImgGrid + threadIdx.x];
  }
  minmax_join_256(mn, mx, sh);
  // tf.summary.image on a float tensor (NormalizeFloatImage): a map with a negative value is centred on 128, any
  // other is stretched over 0..255; a map whose largest magnitude is below 1e-6 (or that holds no finite value) gets scale 0
  float scale, offset;
  if (mn < 0.f) {
    const float m = fmaxf(fabsf(mn), fabsf(mx));
    scale = m < 1e-6f ? 0.f : 127.f / m;
    offset = 128.f;
  } else {
    scale = mx < 1e-6f ? 0.f : 255.f / mx;
    offset = 0.f;
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float v = x[i];
    out[i] = stats_nonfinite(v) ? (unsigned char)0 : (unsigned char)(v * scale + offset);    // in 0..255: truncation
  }
}

}  // namespace

extern "C" int ocr_tensor_stats_num_buckets(void) { return kNB; }
extern "C" int ocr_tensor_stats_chunk(void) { return kChunk; }
extern "C" size_t ocr_tensor_stats_record_bytes(void) { return sizeof(ocr_tensor_stats_record); }
extern "C" size_t ocr_tensor_stats_workspace(int64_t n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(Partial) : 0; }
extern "C" size_t ocr_tensor_stats_table_bytes(int n_segments) {
  return sizeof(StatsHeader) + kPos * sizeof(double) + (size_t)(n_segments > 0 ? n_segments : 0) * sizeof(StatsSeg);
}

extern "C" int ocr_tensor_stats_limits(double* limits_out, int n) {
  OCR_CHECK_ARG(limits_out && n == kNB);
  double pos[kPos];
  int k = 0;
  double v = 1e-12;                                   // tensorflow/core/lib/histogram/histogram.cc: InitDefaultBucketsInner
  while (v < 1e20) {
    if (k >= kPos - 1) return OCR_ERR_INVALID_ARG;    // (cannot happen: the recurrence yields 774)
    pos[k++] = v;
    v *= 1.1;
  }
  if (k != kPos - 1) return OCR_ERR_INVALID_ARG;
  pos[k] = DBL_MAX;
  for (int i = 0; i < kPos; ++i) {
    limits_out[i] = -pos[kPos - 1 - i];
    limits_out[kPos + 1 + i] = pos[i];
  }
  limits_out[kPos] = 0.0;
  return OCR_OK;
}

extern "C" int ocr_tensor_stats_table(int n_segments, const int64_t* offsets, const int64_t* sizes, void* table_host,
                                      int64_t* n_chunks_out) {
  OCR_CHECK_ARG(n_segments > 0 && offsets && sizes && table_host && n_chunks_out);
  double all[kNB];
  const int rc = ocr_tensor_stats_limits(all, kNB);
  if (rc != OCR_OK) return rc;
  double* lim = const_cast<double*>(table_limits(table_host));
  for (int i = 0; i < kPos; ++i) lim[i] = all[kPos + 1 + i];
  StatsSeg* segs = const_cast<StatsSeg*>(table_segs(table_host));
  long long total = 0;
  for (int i = 0; i < n_segments; ++i) {
    OCR_CHECK_ARG(offsets[i] >= 0 && sizes[i] > 0 && sizes[i] <= 0xffffffffll);      // counts are 32-bit
    const long long nc = (sizes[i] + kChunk - 1) / kChunk;
    segs[i] = StatsSeg{offsets[i], sizes[i], (int)total, (int)nc};
    total += nc;
    OCR_CHECK_ARG(total <= 0x7fffffffll);
  }
  *static_cast<StatsHeader*>(table_host) = StatsHeader{n_segments, (int)total, kChunk, kMagic};
  *n_chunks_out = total;
  return OCR_OK;
}

extern "C" int ocr_tensor_stats_f32(const void* x, const void* segments_dev, int n_segments, float mul_host,
                                    const void* mul_dev, void* records, void* workspace, size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(x && segments_dev && records && workspace && n_segments > 0);
  OCR_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)mul_dev & 3) == 0 && ((uintptr_t)segments_dev & 7) == 0 &&
                ((uintptr_t)records & 7) == 0 && ((uintptr_t)workspace & 7) == 0);
  // every segment owns at least one chunk: a workspace below n_segments partials cannot belong to this table
  if (ws_bytes < (size_t)n_segments * sizeof(Partial)) return OCR_ERR_WORKSPACE;
  size_t cap = ws_bytes / sizeof(Partial);
  if (cap > 0x7fffffffu) cap = 0x7fffffffu;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(records, 0, (size_t)n_segments * sizeof(ocr_tensor_stats_record), st) != hipSuccess) return OCR_ERR_HIP;
  hipLaunchKernelGGL(stats_chunk_kernel, dim3(kStatsGrid), dim3(256), 0, st, static_cast<const float*>(x), segments_dev,
                     n_segments, mul_host, static_cast<const float*>(mul_dev),
                     static_cast<ocr_tensor_stats_record*>(records), static_cast<Partial*>(workspace), (unsigned)cap);
  hipLaunchKernelGGL(stats_final_kernel, dim3((unsigned)n_segments), dim3(256), 0, st, segments_dev, n_segments,
                     static_cast<ocr_tensor_stats_record*>(records), static_cast<const Partial*>(workspace), (unsigned)cap);
  return ocr_launch_status();
}

extern "C" size_t ocr_summary_image_workspace(void) { return 2 * kImgGrid * sizeof(float); }

extern "C" int ocr_summary_image_u8(const void* x_f32, int h, int w, int c, void* out_u8, void* workspace, void* stream) {
  OCR_CHECK_ARG(x_f32 && out_u8 && workspace && h > 0 && w > 0 && (c == 1 || c == 3 || c == 4));
  OCR_CHECK_ARG(((uintptr_t)x_f32 & 3) == 0 && ((uintptr_t)workspace & 3) == 0 && (long long)h * w * c <= (1ll << 30));
  const int n = h * w * c;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(image_minmax_kernel, dim3(kImgGrid), dim3(256), 0, st, static_cast<const float*>(x_f32), n,
                     static_cast<float*>(workspace));
  int grid = (n + 255) / 256;
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(image_u8_kernel, dim3(grid), dim3(256), 0, st, static_cast<const float*>(x_f32), n,
                     static_cast<const float*>(workspace), static_cast<unsigned char*>(out_u8));
  return ocr_launch_status();
}

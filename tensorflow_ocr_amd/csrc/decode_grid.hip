// The link decode over a GRID of (pixel threshold, link threshold) pairs in one launch sequence: include/ocr_decode_grid.h
// has the contract.  Slice b = g * n + i is grid point g of image i; it reads image i's maps (never replicated) and
// writes what ocr_link_cc / ocr_component_scores (decode.hip, link_boxes.hip) write for image i at point g, bit for bit.
//
//   ocr_link_cc_grid            decode.hip's tiled union-find with the slice in gridDim.y: init (one score read decides
//                               all G slices) -> 32x32 tiles united in LDS -> tile-border edges -> root / count /
//                               assign / relabel over N = G * n slices.  Seven launches, whatever G is.
//   ocr_component_scores_grid   link_boxes.hip's exact integer mean per component, slice b reading map b mod n.
//
// The union-find helpers are cc_union.h's, the ones decode.hip uses; the thresholds travel as a table in the kernel
// arguments.  Roots are the smallest pixel index of a set and all sums are integers, so nothing here depends on
// scheduling.
#include <limits.h>
#include "common.h"
#include "cc_union.h"

namespace {

constexpr int kMaxPoints = 65;                    // 64 grid points and the base pair
constexpr int kMaxSlices = 65535;                 // slices are gridDim.y
constexpr int kMaxComps = 65535, kMaxSide = 32768;
constexpr int kThreads = 256;

// decode.hip's direction table (kDx / kDy there, in the order of the link planes); tests/test_decode_grid_host.py holds
// the two copies equal
__device__ __constant__ int kDx[8] = {-1, -1, -1, 1, 1, 1, 0, 0};
__device__ __constant__ int kDy[8] = {0, 1, -1, 0, 1, -1, -1, 1};

struct GridThresholds {
  float tp[kMaxPoints], tl[kMaxPoints];
};

struct GridP {
  int G, n, h, w, min_size;
  int ls, lo;                                     // element stride / offset inside link_score, as CcP's
};

unsigned ggrid(size_t items, size_t cap = 4096) {
  size_t b = (items + kThreads - 1) / kThreads;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// one thread per pixel of the n maps: the score is read once and decides the pixel in all G slices
__global__ __launch_bounds__(kThreads) void ccg_init_kernel(GridP p, GridThresholds t, const float* __restrict__ score,
                                                             int* __restrict__ parent, int* __restrict__ size) {
  const size_t hw = (size_t)p.h * p.w, maps = (size_t)p.n * hw;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < maps; i += (size_t)gridDim.x * kThreads) {
    const int local = (int)(i % hw);
    const float s = score[i];
    for (int g = 0; g < p.G; ++g) {
      const size_t o = (size_t)g * maps + i;      // slice g * n + img, pixel local
      parent[o] = s > t.tp[g] ? local : -1;
      size[o] = 0;
    }
  }
}

// cc_union_tile_kernel<0, BORDER> of decode.hip with blockIdx.y = slice: the link planes of image slice % n against the
// link threshold of point slice / n
template <bool BORDER>
__global__ __launch_bounds__(1024) void ccg_union_tile_kernel(GridP p, GridThresholds t, const float* __restrict__ link,
                                                              int* __restrict__ parent, int* __restrict__ tcnt) {
  __shared__ int lp[1024];
  __shared__ int lcnt[1024];
  const int hw = p.h * p.w;
  const int slice = blockIdx.y, img = slice % p.n;
  const float tl = t.tl[slice / p.n];
  const int tiles_x = (p.w + 31) >> 5;
  const int tx0 = (blockIdx.x % tiles_x) << 5, ty0 = (blockIdx.x / tiles_x) << 5;
  const int tid = threadIdx.x, lx = tid & 31, ly = tid >> 5;
  const int x = tx0 + lx, y = ty0 + ly;
  const bool inimg = x < p.w && y < p.h;
  const int local = y * p.w + x;
  int* par = parent + (size_t)slice * hw;
  const bool seg = inimg && par[local] >= 0;
  if (!BORDER) {
    lp[tid] = seg ? tid : -1;
    lcnt[tid] = 0;
    __syncthreads();
  }
  if (seg && x >= 1 && x <= p.w - 2 && y >= 1 && y <= p.h - 2) {          // links of interior pixels only
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const int dx = kDx[d], dy = kDy[d];
      const int nx = x + dx, ny = y + dy;
      const bool inside = (nx >> 5) == (x >> 5) && (ny >> 5) == (y >> 5);
      if (inside == BORDER) continue;
      if (!(link[(((size_t)d * p.n + img) * hw + local) * p.ls + p.lo] > tl)) continue;
      const int q = ny * p.w + nx;
      if (BORDER) {
        if (par[q] >= 0) uf_unite(par, local, q);
      } else if (lp[(ly + dy) * 32 + lx + dx] >= 0) {
        lds_unite(lp, tid, (ly + dy) * 32 + lx + dx);
      }
    }
  }
  if (!BORDER) {
    __syncthreads();
    if (seg) {
      const int r = lds_find(lp, tid);
      par[local] = (ty0 + (r >> 5)) * p.w + tx0 + (r & 31);
      atomicAdd(lcnt + r, 1);
    }
    __syncthreads();
    if (inimg) tcnt[(size_t)slice * hw + local] = lcnt[tid];      // pixels per tile-local set, kept at the set's root
  }
}

// ---- root / count / assign / relabel: decode.hip's numbering over N = G * n slices ----------------------------
__global__ __launch_bounds__(kThreads) void ccg_root_kernel(int N, int hw_, int* __restrict__ parent, int* __restrict__ root,
                                                             int* __restrict__ size, const int* __restrict__ tcnt) {
  const size_t hw = (size_t)hw_, total = (size_t)N * hw;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const size_t slice = i / hw;
    const int local = (int)(i % hw);
    int* par = parent + slice * hw;
    int r = -1;
    if (par[local] >= 0) {
      r = uf_find(par, local);
      const int c = tcnt[i];                      // > 0 only at the root of a tile-local set
      if (c > 0) atomicAdd(size + slice * hw + r, c);
    }
    root[i] = r;
  }
}

__device__ __forceinline__ bool ccg_is_kept_root(int min_size, const int* rt, const int* sz, int i, int hw) {
  return i < hw && rt[i] == i && sz[i] > min_size;
}

__global__ __launch_bounds__(1024) void ccg_count_kernel(int hw, int min_size, const int* __restrict__ root,
                                                         const int* __restrict__ size, int* __restrict__ blkcnt) {
  __shared__ int wsum[16];
  const int slice = blockIdx.y;
  const int i = blockIdx.x * 1024 + threadIdx.x;
  const bool flag = ccg_is_kept_root(min_size, root + (size_t)slice * hw, size + (size_t)slice * hw, i, hw);
  const int c = __popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += wsum[k];
    blkcnt[(size_t)slice * gridDim.x + blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(1024) void ccg_assign_kernel(int hw, int min_size, const int* __restrict__ root,
                                                          const int* __restrict__ size, const int* __restrict__ blkcnt,
                                                          int* __restrict__ ids, int* __restrict__ ncomp,
                                                          int* __restrict__ comps, int max_comps) {
  __shared__ int wsum[16];
  __shared__ int s_red[16];
  const int slice = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* rt = root + (size_t)slice * hw;
  const int* sz = size + (size_t)slice * hw;
  // ids given out by the blocks before this one (and, for the slice's count, by all of them)
  int before = 0, all = 0;
  for (int b = threadIdx.x; b < (int)gridDim.x; b += 1024) {
    const int c = blkcnt[(size_t)slice * gridDim.x + b];
    all += c;
    if (b < (int)blockIdx.x) before += c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_down(before, o, 64);
    all += __shfl_down(all, o, 64);
  }
  if (lane == 0) { wsum[wave] = before; s_red[wave] = all; }
  __syncthreads();
  before = 0; all = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { before += wsum[k]; all += s_red[k]; }
  __syncthreads();
  const int i = blockIdx.x * 1024 + threadIdx.x;
  const bool flag = ccg_is_kept_root(min_size, rt, sz, i, hw);
  const unsigned long long vote = __ballot(flag);
  if (lane == 0) wsum[wave] = __popcll(vote);
  __syncthreads();
  int off = before;
  for (int k = 0; k < wave; ++k) off += wsum[k];
  if (i < hw) {
    const int myid = flag ? off + __popcll(vote & ((1ull << lane) - 1ull)) + 1 : 0;       // 1-based dense id
    ids[(size_t)slice * hw + i] = myid;
    if (flag && myid <= max_comps) {
      comps[((size_t)slice * max_comps + myid - 1) * 2 + 0] = i;
      comps[((size_t)slice * max_comps + myid - 1) * 2 + 1] = sz[i];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) ncomp[slice] = all;
}

__global__ __launch_bounds__(kThreads) void ccg_relabel_kernel(size_t hw, size_t total, const int* __restrict__ root,
                                                                const int* __restrict__ ids, int* __restrict__ label) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int r = root[i];
    label[i] = r >= 0 ? ids[(i / hw) * hw + r] : 0;
  }
}

// ---- component scores: comp_score_accum_kernel / comp_score_mean_kernel of link_boxes.hip, slice b reading map b % n
constexpr unsigned kNoKey = 0xFFFFFFFFu;

__global__ __launch_bounds__(kThreads) void csg_accum_kernel(const int* __restrict__ labels, const float* __restrict__ score,
                                                              int n, size_t hw, size_t total, int max_comps,
                                                              unsigned long long* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  const size_t step = (size_t)gridDim.x * kThreads;
  for (size_t base = (size_t)blockIdx.x * kThreads + (threadIdx.x & ~63); base < total; base += step) {      // wave-uniform
    const size_t i = base + lane;
    unsigned key = kNoKey, q = 0;
    if (i < total) {
      const int L = labels[i];
      if (L >= 1 && L <= max_comps) {
        const size_t slice = i / hw;
        key = (unsigned)slice * (unsigned)max_comps + (unsigned)(L - 1);         // < 65535 * 65535 + 65535
        const float s = score[(slice % (size_t)n) * hw + i % hw];
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

__global__ __launch_bounds__(kThreads) void csg_mean_kernel(const unsigned long long* __restrict__ acc,
                                                             const int* __restrict__ ncomp, int N, int max_comps,
                                                             float* __restrict__ comp_score) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)N * max_comps) return;
  const int slice = (int)(i / max_comps), c = (int)(i % max_comps);
  const int k = min(max(ncomp[slice], 0), max_comps);
  float m = 0.f;
  if (c < k) {
    const unsigned long long sum = acc[2 * i], cnt = acc[2 * i + 1];
    if (cnt > 0) m = (float)((double)sum / (double)cnt / 16777216.0);        // an id without pixels scores 0
  }
  comp_score[i] = m;
}

}  // namespace

extern "C" size_t ocr_link_cc_grid_workspace(int G, int n, int h, int w) {
  if (G <= 0 || n <= 0 || h <= 0 || w <= 0) return 0;
  // parent, size, root, ids per slice pixel + one counter per 1024-pixel block of a slice
  const size_t N = (size_t)G * n;
  return N * h * w * sizeof(int) * 4 + N * (((size_t)h * w + 1023) / 1024) * sizeof(int);
}

extern "C" int ocr_link_cc_grid(const void* pixel_score, const void* link_score, int link_elem_stride, int link_elem_offset,
                                int n, int h, int w, int G, const float* pixel_thresh_host, const float* link_thresh_host,
                                int min_size, void* labels_i32, void* ncomp_i32, void* comps_i32, int max_comps,
                                void* workspace, size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(pixel_score && link_score && pixel_thresh_host && link_thresh_host && labels_i32 && ncomp_i32 &&
                comps_i32 && workspace);
  OCR_CHECK_ARG(G > 0 && n > 0 && h > 0 && w > 0 && max_comps > 0);
  OCR_CHECK_ARG(link_elem_stride >= 1 && link_elem_offset >= 0 && link_elem_offset < link_elem_stride);
  OCR_CHECK_SHAPE(G <= kMaxPoints && (int64_t)G * n <= kMaxSlices && h > 2 && w > 2);
  OCR_CHECK_SHAPE((int64_t)h * w <= INT32_MAX && (int64_t)G * n * ((int64_t)h * w) <= INT32_MAX);
  if (ws_bytes < ocr_link_cc_grid_workspace(G, n, h, w)) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = G * n, hw = h * w;
  const size_t total = (size_t)N * hw;
  int* parent = static_cast<int*>(workspace);
  int* size = parent + total;
  int* root = size + total;
  int* ids = root + total;
  int* blkcnt = ids + total;
  const GridP p{G, n, h, w, min_size, link_elem_stride, link_elem_offset};
  GridThresholds t{};
  for (int g = 0; g < G; ++g) {
    t.tp[g] = pixel_thresh_host[g];
    t.tl[g] = link_thresh_host[g];
  }
  const float* score = static_cast<const float*>(pixel_score);
  const float* link = static_cast<const float*>(link_score);
  hipLaunchKernelGGL(ccg_init_kernel, dim3(ggrid((size_t)n * hw)), dim3(kThreads), 0, st, p, t, score, parent, size);
  const dim3 tgrid((unsigned)(((w + 31) / 32) * ((h + 31) / 32)), (unsigned)N);
  hipLaunchKernelGGL((ccg_union_tile_kernel<false>), tgrid, dim3(1024), 0, st, p, t, link, parent, ids);
  hipLaunchKernelGGL((ccg_union_tile_kernel<true>), tgrid, dim3(1024), 0, st, p, t, link, parent, ids);
  hipLaunchKernelGGL(ccg_root_kernel, dim3(ggrid(total)), dim3(kThreads), 0, st, N, hw, parent, root, size, ids);
  const dim3 bgrid((unsigned)(((size_t)hw + 1023) / 1024), (unsigned)N);
  hipLaunchKernelGGL(ccg_count_kernel, bgrid, dim3(1024), 0, st, hw, min_size, root, size, blkcnt);
  hipLaunchKernelGGL(ccg_assign_kernel, bgrid, dim3(1024), 0, st, hw, min_size, root, size, blkcnt, ids,
                     static_cast<int*>(ncomp_i32), static_cast<int*>(comps_i32), max_comps);
  hipLaunchKernelGGL(ccg_relabel_kernel, dim3(ggrid(total)), dim3(kThreads), 0, st, (size_t)hw, total, root, ids,
                     static_cast<int*>(labels_i32));
  return ocr_launch_status();
}

extern "C" size_t ocr_component_scores_grid_workspace(int G, int n, int max_comps) {
  if (G <= 0 || n <= 0 || max_comps <= 0) return 0;
  return (size_t)G * n * max_comps * 2 * sizeof(unsigned long long);
}

extern "C" int ocr_component_scores_grid(const void* labels_i32, const void* pixel_score_f32, const void* ncomp_i32, int G,
                                         int n, int h, int w, int max_comps, void* comp_score_f32, void* workspace,
                                         size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(labels_i32 && pixel_score_f32 && ncomp_i32 && comp_score_f32 && workspace);
  OCR_CHECK_ARG(G > 0 && n > 0 && h > 0 && w > 0 && max_comps > 0);
  OCR_CHECK_SHAPE(G <= kMaxPoints && (int64_t)G * n <= kMaxSlices && max_comps <= kMaxComps && h <= kMaxSide && w <= kMaxSide);
  const size_t need = ocr_component_scores_grid_workspace(G, n, max_comps);
  if (ws_bytes < need) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* acc = static_cast<unsigned long long*>(workspace);
  if (hipMemsetAsync(acc, 0, need, st) != hipSuccess) return OCR_ERR_HIP;
  const int N = G * n;
  const size_t hw = (size_t)h * w, total = (size_t)N * hw;
  hipLaunchKernelGGL(csg_accum_kernel, dim3(ggrid(total)), dim3(kThreads), 0, st, static_cast<const int*>(labels_i32),
                     static_cast<const float*>(pixel_score_f32), n, hw, total, max_comps, acc);
  const size_t rows = (size_t)N * max_comps;
  hipLaunchKernelGGL(csg_mean_kernel, dim3(ggrid(rows, (size_t)1 << 30)), dim3(kThreads), 0, st, acc,
                     static_cast<const int*>(ncomp_i32), N, max_comps, static_cast<float*>(comp_score_f32));
  return ocr_launch_status();
}

// Multi-scale RBOX inference on the device (include/ocr_multiscale.h): the per-scale LANMS results of an image are pooled
// in original-image pixels (ocr_ms_pool_append) and fused across scales by score-ordered NMS, optionally with a
// score-weighted vote (ocr_quad_fuse).  ocr_lanms cannot do the second step: its first phase merges RASTER NEIGHBOURS,
// which a pooled list does not have, and its score is a sum of pixel scores, which grows with the scale.
//
//   append  (one wave per image): the surviving keep slots of one scale, compacted in keep order by ballot + prefix count
//   rank    (grid = quad blocks x images): stable counting sort by descending score, NaN last, ties in pool order
//   mask    (grid = row blocks x images): nms_mask_kernel of quad_nms.h, the suppression matrix ocr_lanms builds
//   sweep   (one wave per image): ocr_lanms's greedy sweep over the row masks, rows prefetched 64 ahead; it also leaves
//           the kept sorted positions and one kept bit per sorted position
//   owner   (grid = quad blocks x images): a suppressed row's owner is the FIRST kept row whose mask holds its bit — what
//           the sweep decided, read back from the same rows by one thread per quad instead of being scattered from the
//           sequential wave; it also copies the pool rows to `fused`
//   vote    (mode 1; one wave per kept quad): walks the sorted positions from the kept quad on, 64 at a time; the
//           members found pick their cyclic shift in parallel and are then summed in rank order in f64
//
// Compiled without FMA contraction (Makefile NOFMA): the division of the append and the f64 terms of the vote are
// specified operation by operation.  No atomic decides an order.
#include <limits.h>

#include "quad_nms.h"

namespace {

#pragma clang fp contract(off)

constexpr int kMaxPool = 4096;                  // 64 mask words per row: the sweep holds one word per lane

// ------------------------------------------------------------------------------------------------ append
__global__ __launch_bounds__(64) void ms_append_kernel(
    const float* __restrict__ merged, const int* __restrict__ keep_idx, const int* __restrict__ n_keep,
    const unsigned char* __restrict__ passed, const float* __restrict__ mean, const float* __restrict__ ratio,
    int scale_id, int max_k, int max_pool, float* __restrict__ pool, int* __restrict__ pool_scale,
    int* __restrict__ pool_count, int* __restrict__ pool_total, int* __restrict__ pool_nonfinite) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const float* mrg = merged + (size_t)img * max_k * 9;
  const int* keep = keep_idx + (size_t)img * max_k;
  const float* mn = mean + (size_t)img * max_k;
  const unsigned char* pass = passed ? passed + (size_t)img * max_k : nullptr;
  const int nk = min(max(n_keep[img], 0), max_k);
  const float rw = ratio[2 * img], rh = ratio[2 * img + 1];
  const int start = min(max(pool_count[img], 0), max_pool);
  float* out = pool + (size_t)img * max_pool * 9;
  int* out_scale = pool_scale + (size_t)img * max_pool;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int appended = 0, dropped = 0;                // wave-uniform
  for (int base = 0; base < nk; base += 64) {
    const int j = base + lane;
    const bool live = j < nk && (!pass || pass[j]);
    bool ok = false;
    float row[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) row[k] = 0.f;
    if (live) {
      const int r = keep[j];
      if (r >= 0 && r < max_k) {
        const float* q = mrg + (size_t)r * 9;
        ok = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          row[k] = __fdiv_rn(q[k], (k & 1) ? rh : rw);
          ok = ok && isfinite(row[k]);
        }
        row[8] = mn[j];
        ok = ok && isfinite(row[8]);
      }
    }
    const unsigned long long good = __ballot(live && ok), bad = __ballot(live && !ok);
    if (live && ok) {
      const long long pos = (long long)start + appended + __popcll(good & lt);
      if (pos < max_pool) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[pos * 9 + k] = row[k];
        out_scale[pos] = scale_id;
      }
    }
    appended += __popcll(good);
    dropped += __popcll(bad);
  }
  if (lane == 0) {
    const long long total = (long long)pool_total[img] + appended;
    pool_total[img] = (int)min(total, (long long)INT_MAX);
    pool_count[img] = (int)min(max(total, 0ll), (long long)max_pool);
    pool_nonfinite[img] += dropped;
  }
}

// ------------------------------------------------------------------------------------------------ rank
// does row a (score sa, pool index ia) come before row b?  Descending score, ties in pool order, NaN scores last: a total
// order, so the ranks are a permutation whatever the scores hold
__device__ __forceinline__ bool ranks_before(float sa, int ia, float sb, int ib) {
  const bool an = sa != sa, bn = sb != sb;
  if (an || bn) return (!an && bn) || (an && bn && ia < ib);
  return sa > sb || (sa == sb && ia < ib);
}

// grid (quad blocks, images): one thread per pooled quad counts the rows in front of its own, the scores streamed through
// LDS 2048 at a time (lanms_rank_kernel's shape).  Block 0 of an image also leaves the clamped count for the later phases.
__global__ __launch_bounds__(256) void fuse_rank_kernel(const float* __restrict__ pool, const int* __restrict__ pool_count,
                                                        int max_pool, int* __restrict__ cnt_ws, int* __restrict__ order_ws) {
  __shared__ float s_score[2048];
  const int img = blockIdx.y;
  const int m = min(max(pool_count[img], 0), max_pool);
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt_ws[img] = m;
  if ((int)blockIdx.x * 256 >= m) return;
  const float* pl = pool + (size_t)img * max_pool * 9;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float si = i < m ? pl[9 * i + 8] : 0.f;
  int r = 0;
  for (int base = 0; base < m; base += 2048) {
    const int cnt = min(2048, m - base);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += 256) s_score[t] = pl[9 * (base + t) + 8];
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < cnt; ++t) r += ranks_before(s_score[t], base + t, si, i);
  }
  if (i < m) order_ws[(size_t)img * max_pool + r] = i;
}

// ------------------------------------------------------------------------------------------------ sweep
// One wave per image: lanms_sweep64_kernel's greedy sweep (lane w owns mask word w of every row, the rows fetched 64 ahead,
// the decision chain in scalar registers).  Besides keep_idx / n_keep it leaves, for the owner and vote phases, the kept
// SORTED positions (keep_pos) and one kept bit per sorted position (kept_ws, one word per 64 rows).
__global__ __launch_bounds__(64) void fuse_sweep_kernel(const int* __restrict__ cnt_ws, int max_pool,
                                                        const int* __restrict__ order_ws,
                                                        const unsigned long long* __restrict__ mask_ws,
                                                        int* __restrict__ keep_idx, int* __restrict__ n_keep,
                                                        int* __restrict__ keep_pos_ws,
                                                        unsigned long long* __restrict__ kept_ws) {
  constexpr int D = 64;                                   // rows in flight: a group must outlast one memory round trip
  __shared__ int s_keep[kMaxPool];                        // kept SORTED positions; mapped through order[] at the end
  const int img = blockIdx.x, lane = threadIdx.x;
  const int m = cnt_ws[img];
  const int words = (max_pool + 63) / 64;                 // <= 64
  const int* order = order_ws + (size_t)img * max_pool;
  const unsigned long long* mask = mask_ws + (size_t)img * max_pool * words;
  unsigned long long removed = 0ull, rem = 0ull, kept = 0ull, cur[D], nxt[D];
#pragma unroll
  for (int j = 0; j < D; ++j) cur[j] = (j < m && lane < words) ? mask[(size_t)j * words + lane] : 0ull;
  int nk = 0;
  for (int a0 = 0; a0 < m; a0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int row = a0 + D + j;
      nxt[j] = (row < m && lane < words) ? mask[(size_t)row * words + lane] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int a = a0 + j;
      if (a < m) {
        const int owner = __builtin_amdgcn_readfirstlane(a >> 6);
        if ((a & 63) == 0) rem = lane_word(removed, owner);
        if (!((rem >> (a & 63)) & 1ull)) {
          kept |= 1ull << (a & 63);
          removed |= cur[j];
          rem |= lane_word(cur[j], owner);
        }
        if ((a & 63) == 63 || a == m - 1) {               // block done: its kept positions, all lanes at once
          if ((kept >> lane) & 1ull) s_keep[nk + __popcll(kept & ((1ull << lane) - 1ull))] = (a & ~63) + lane;
          if (lane == 0) kept_ws[(size_t)img * (kMaxPool / 64) + (a >> 6)] = kept;
          nk += __popcll(kept);
          kept = 0ull;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) cur[j] = nxt[j];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int i = lane; i < nk; i += 64) {
    keep_idx[(size_t)img * max_pool + i] = order[s_keep[i]];
    keep_pos_ws[(size_t)img * max_pool + i] = s_keep[i];
  }
  if (lane == 0) n_keep[img] = nk;
}

// ------------------------------------------------------------------------------------------------ owner
// grid (quad blocks, images), thread t: pool row t is copied to `fused` (t < m) or marked ownerless (t >= m), and the
// quad at SORTED position t finds its owner: itself when kept, else the first kept position a (ascending = rank order)
// whose mask row holds bit t — the row that claimed it in the sweep, since a row is claimed by the first kept row that
// overlaps it.  The mask holds the strict upper triangle only, so only kept positions a < t are looked at.
__global__ __launch_bounds__(256) void fuse_owner_kernel(const float* __restrict__ pool, const int* __restrict__ cnt_ws,
                                                         int max_pool, const int* __restrict__ order_ws,
                                                         const unsigned long long* __restrict__ mask_ws,
                                                         const int* __restrict__ n_keep,
                                                         const int* __restrict__ keep_pos_ws,
                                                         const unsigned long long* __restrict__ kept_ws,
                                                         float* __restrict__ fused, int* __restrict__ owner,
                                                         int* __restrict__ owner_pos_ws) {
  const int img = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= max_pool) return;
  const int m = cnt_ws[img];
  const size_t row0 = (size_t)img * max_pool;
  if (t >= m) {
    owner[row0 + t] = -1;
    return;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) fused[(row0 + t) * 9 + k] = pool[(row0 + t) * 9 + k];
  const int words = (max_pool + 63) / 64;
  const int* order = order_ws + row0;
  const int* keep_pos = keep_pos_ws + row0;
  const unsigned long long* mask = mask_ws + row0 * words;
  int own = t;
  if (!((kept_ws[(size_t)img * (kMaxPool / 64) + (t >> 6)] >> (t & 63)) & 1ull)) {
    const int nk = n_keep[img];
    for (int kk = 0; kk < nk; ++kk) {
      const int a = keep_pos[kk];
      if (a >= t) break;
      if ((mask[(size_t)a * words + (t >> 6)] >> (t & 63)) & 1ull) { own = a; break; }
    }
  }
  owner_pos_ws[row0 + t] = own;
  owner[row0 + order[t]] = order[own];
}

// ------------------------------------------------------------------------------------------------ vote
// grid (kept-quad blocks, images), one wave per kept quad k (sorted position a): the sorted positions a, a+1, ... are
// looked at 64 per step; the members found (owner position == a; k itself is the first) each pick the cyclic shift of
// their vertices nearest k's — one member per lane — and go through LDS in rank order, where every lane adds them up in
// that order in f64 (lane c < 8 owns coordinate c), so the sums have ONE order whatever the scheduling.
__global__ __launch_bounds__(256) void fuse_vote_kernel(const float* __restrict__ pool, const int* __restrict__ cnt_ws,
                                                        int max_pool, const int* __restrict__ order_ws,
                                                        const int* __restrict__ n_keep,
                                                        const int* __restrict__ keep_pos_ws,
                                                        const int* __restrict__ owner_pos_ws,
                                                        float* __restrict__ fused) {
  __shared__ float s_q[4][64][9];
  __shared__ int s_r[4][64];
  const int img = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kk = blockIdx.x * 4 + wave;
  if (kk >= n_keep[img]) return;                          // whole wave
  const int m = cnt_ws[img];
  const size_t row0 = (size_t)img * max_pool;
  const float* pl = pool + row0 * 9;
  const int* order = order_ws + row0;
  const int* owner_pos = owner_pos_ws + row0;
  const int a = keep_pos_ws[row0 + kk];
  const int k_row = order[a];
  float qk[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) qk[c] = pl[(size_t)k_row * 9 + c];
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int c = lane & 7;
  double W = 0.0, C = 0.0;
  for (int base = a; base < m; base += 64) {
    const int b = base + lane;
    const bool member = b < m && owner_pos[b] == a;
    const unsigned long long vote = __ballot(member);
    if (vote == 0ull) continue;
    if (member) {
      const float* q = pl + (size_t)order[b] * 9;
      float v[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) v[i] = q[i];
      int best_r = 0;
      double best = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double d = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const double dx = (double)v[2 * ((p + r) & 3)] - (double)qk[2 * p];
          const double dy = (double)v[2 * ((p + r) & 3) + 1] - (double)qk[2 * p + 1];
          d = d + dx * dx;
          d = d + dy * dy;
        }
        if (r == 0 || d < best) { best = d; best_r = r; }
      }
      const int pos = __popcll(vote & lt);
#pragma unroll
      for (int i = 0; i < 9; ++i) s_q[wave][pos][i] = v[i];
      s_r[wave][pos] = best_r;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int cnt = __popcll(vote);
    for (int t = 0; t < cnt; ++t) {
      const float s = s_q[wave][t][8];
      const float qc = s_q[wave][t][(c + 2 * s_r[wave][t]) & 7];
      W = W + (double)s;
      C = C + (double)s * (double)qc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (lane < 8 && W != 0.0) fused[(row0 + k_row) * 9 + lane] = (float)(C / W);
}

struct FuseWorkspace {
  size_t cnt, order, keep_pos, owner_pos, kept, mask, bytes;
};

inline FuseWorkspace fuse_layout(int n, int max_pool) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t rows = (size_t)n * max_pool, words = (size_t)(max_pool + 63) / 64;
  FuseWorkspace w;
  w.cnt = 0;
  w.order = up((size_t)n * sizeof(int));
  w.keep_pos = w.order + up(rows * sizeof(int));
  w.owner_pos = w.keep_pos + up(rows * sizeof(int));
  w.kept = w.owner_pos + up(rows * sizeof(int));
  w.mask = w.kept + up((size_t)n * (kMaxPool / 64) * sizeof(unsigned long long));
  w.bytes = w.mask + up(rows * words * sizeof(unsigned long long));
  return w;
}

}  // namespace

extern "C" int ocr_ms_pool_append(const void* merged_f32, const void* keep_idx_i32, const void* n_keep_i32,
                                  const void* passed_u8, const void* mean_f32, const void* ratio_f32, int scale_id, int n,
                                  int max_k, int max_pool, void* pool_f32, void* pool_scale_i32, void* pool_count_i32,
                                  void* pool_total_i32, void* pool_nonfinite_i32, void* stream) {
  OCR_CHECK_ARG(merged_f32 && keep_idx_i32 && n_keep_i32 && mean_f32 && ratio_f32 && pool_f32 && pool_scale_i32 &&
                pool_count_i32 && pool_total_i32 && pool_nonfinite_i32 && n > 0 && max_k > 0 && max_pool > 0 &&
                scale_id >= 0);
  OCR_CHECK_SHAPE(n <= 65535);
  hipLaunchKernelGGL(ms_append_kernel, dim3(n), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(merged_f32), static_cast<const int*>(keep_idx_i32),
                     static_cast<const int*>(n_keep_i32), static_cast<const unsigned char*>(passed_u8),
                     static_cast<const float*>(mean_f32), static_cast<const float*>(ratio_f32), scale_id, max_k, max_pool,
                     static_cast<float*>(pool_f32), static_cast<int*>(pool_scale_i32), static_cast<int*>(pool_count_i32),
                     static_cast<int*>(pool_total_i32), static_cast<int*>(pool_nonfinite_i32));
  return ocr_launch_status();
}

extern "C" size_t ocr_quad_fuse_workspace(int n, int max_pool) {
  if (n <= 0 || max_pool <= 0 || max_pool > kMaxPool) return 0;
  return fuse_layout(n, max_pool).bytes;
}

extern "C" int ocr_quad_fuse(const void* pool_f32, const void* pool_count_i32, int n, int max_pool, float iou_thresh,
                             int mode, void* fused_f32, void* keep_idx_i32, void* n_keep_i32, void* owner_i32,
                             void* workspace, size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(pool_f32 && pool_count_i32 && fused_f32 && keep_idx_i32 && n_keep_i32 && owner_i32 && workspace && n > 0 &&
                max_pool > 0 && (mode == 0 || mode == 1));
  OCR_CHECK_SHAPE(max_pool <= kMaxPool && n <= 65535);
  const FuseWorkspace w = fuse_layout(n, max_pool);
  if (ws_bytes < w.bytes) return OCR_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  int* cnt = reinterpret_cast<int*>(ws + w.cnt);
  int* order = reinterpret_cast<int*>(ws + w.order);
  int* keep_pos = reinterpret_cast<int*>(ws + w.keep_pos);
  int* owner_pos = reinterpret_cast<int*>(ws + w.owner_pos);
  unsigned long long* kept = reinterpret_cast<unsigned long long*>(ws + w.kept);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(ws + w.mask);
  const float* pool = static_cast<const float*>(pool_f32);
  float* fused = static_cast<float*>(fused_f32);
  int* n_keep = static_cast<int*>(n_keep_i32);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int words = (max_pool + 63) / 64;
  hipLaunchKernelGGL(fuse_rank_kernel, dim3(ocr_cdiv(max_pool, 256), n), dim3(256), 0, st, pool,
                     static_cast<const int*>(pool_count_i32), max_pool, cnt, order);
  hipLaunchKernelGGL(nms_mask_kernel, dim3(ocr_cdiv(max_pool * words, 256), n), dim3(256), 0, st, pool, cnt, max_pool,
                     iou_thresh, order, mask);
  hipLaunchKernelGGL(fuse_sweep_kernel, dim3(n), dim3(64), 0, st, cnt, max_pool, order, mask,
                     static_cast<int*>(keep_idx_i32), n_keep, keep_pos, kept);
  hipLaunchKernelGGL(fuse_owner_kernel, dim3(ocr_cdiv(max_pool, 256), n), dim3(256), 0, st, pool, cnt, max_pool, order, mask,
                     n_keep, keep_pos, kept, fused, static_cast<int*>(owner_i32), owner_pos);
  if (mode == 1)
    hipLaunchKernelGGL(fuse_vote_kernel, dim3(ocr_cdiv(max_pool, 4), n), dim3(256), 0, st, pool, cnt, max_pool, order, n_keep,
                       keep_pos, owner_pos, fused);
  return ocr_launch_status();
}

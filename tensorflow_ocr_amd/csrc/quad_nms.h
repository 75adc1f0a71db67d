// The pieces of score-ordered quad NMS that lanms.hip (ocr_lanms) and multiscale.hip (ocr_quad_fuse) share: the convex-quad
// clipper (quad_iou of oracle/lanms_oracle.c, operation for operation), the bounding-box early-out and the suppression
// matrix kernel.  Both sources are compiled without FMA contraction (Makefile NOFMA); the text below is what lanms.hip
// held, so ocr_lanms computes what it computed.
#pragma once
#include "common.h"

namespace {

#pragma clang fp contract(off)

struct pt { float x, y; };

__device__ float signed_area(const pt* p, int n) {
  float a = 0.f;
  for (int i = 0; i < n; ++i) {
    const pt u = p[i], v = p[(i + 1) % n];
    a += u.x * v.y - v.x * u.y;
  }
  return a * 0.5f;
}

__device__ float cross3(pt a, pt b, pt c) { return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x); }

__device__ pt intersect(pt s, pt e, pt c1, pt c2) {
  const float d1 = cross3(c1, c2, s), d2 = cross3(c1, c2, e);
  const float t = d1 / (d1 - d2);
  pt r;
  r.x = s.x + t * (e.x - s.x);
  r.y = s.y + t * (e.y - s.y);
  return r;
}

__device__ void load_ccw(const float* q, pt* out) {
  for (int i = 0; i < 4; ++i) { out[i].x = q[2 * i]; out[i].y = q[2 * i + 1]; }
  if (signed_area(out, 4) < 0.f) {
    pt t = out[1]; out[1] = out[3]; out[3] = t;
  }
}

// IoU of two convex quads by Sutherland-Hodgman clipping (quad_iou of oracle/lanms_oracle.c, operation for
// operation), one pair per thread.  The two work polygons live in LDS (point i of thread t at [i * 256 + t]:
// one bank per lane): as private arrays the compiler places them in scratch = global memory, and a clip is a
// chain of dependent indexed reads and writes (~4x slower).  A quad clipped by four half-planes has at most
// 8 vertices.
constexpr int kClipPts = 10;
__device__ float quad_iou_lds(const float* qa, const float* qb, pt* cur, pt* nxt) {
  pt a[4], b[4];
  load_ccw(qa, a);
  load_ccw(qb, b);
  const float area_a = fabsf(signed_area(a, 4)), area_b = fabsf(signed_area(b, 4));
  int n = 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) cur[i * 256] = a[i];
#pragma unroll
  for (int ce = 0; ce < 4; ++ce) {
    if (n > 0) {
      const pt c1 = b[ce], c2 = b[(ce + 1) % 4];
      int m = 0;
      for (int i = 0; i < n; ++i) {
        const pt s = cur[i * 256], e = cur[((i + 1) % n) * 256];
        const bool sin = cross3(c1, c2, s) >= 0.f, ein = cross3(c1, c2, e) >= 0.f;
        if (sin && ein) nxt[(m++) * 256] = e;
        else if (sin && !ein) nxt[(m++) * 256] = intersect(s, e, c1, c2);
        else if (!sin && ein) { nxt[(m++) * 256] = intersect(s, e, c1, c2); nxt[(m++) * 256] = e; }
      }
      n = m;
      pt* t = cur; cur = nxt; nxt = t;
    }
  }
  float inter = 0.f;
  if (n >= 3) {
    float acc = 0.f;
    for (int i = 0; i < n; ++i) {
      const pt u = cur[i * 256], v = cur[((i + 1) % n) * 256];
      acc += u.x * v.y - v.x * u.y;
    }
    inter = fabsf(acc * 0.5f);
  }
  const float uni = area_a + area_b - inter;
  return uni > 0.f ? inter / uni : 0.f;
}

// Early-out: quads whose axis-aligned bounding boxes are disjoint have an empty intersection (the
// clipper could at most leave a rounding-sized sliver), so `iou(a, b) > thr` is false for any
// thr >= 1e-3 without running the clipper.  Only that decision is consumed, so the kept indices stay
// bit-identical to the oracle; below 1e-3 the clipper always runs.
__device__ bool aabb_disjoint(const float* a, const float* b) {
  float ax0 = a[0], ax1 = a[0], ay0 = a[1], ay1 = a[1], bx0 = b[0], bx1 = b[0], by0 = b[1], by1 = b[1];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    ax0 = fminf(ax0, a[2 * i]); ax1 = fmaxf(ax1, a[2 * i]);
    ay0 = fminf(ay0, a[2 * i + 1]); ay1 = fmaxf(ay1, a[2 * i + 1]);
    bx0 = fminf(bx0, b[2 * i]); bx1 = fmaxf(bx1, b[2 * i]);
    by0 = fminf(by0, b[2 * i + 1]); by1 = fmaxf(by1, b[2 * i + 1]);
  }
  return ax1 < bx0 || bx1 < ax0 || ay1 < by0 || by1 < ay0;
}

// Suppression matrix (grid = row blocks x images): IoU > thr of every pair of the score-sorted quads
// (quad at sorted position a = merged[order[a]], m = n_merged[img] <= max_k of them), one
// 64-bit word (64 pairs) per thread; only the strict upper triangle is evaluated.  Most pairs are
// settled by the bounding-box test; the few that need the clipper would make a wave wait on one or
// two busy lanes at a time, so candidates are queued per wave in LDS ((owner lane, bit) entries) and
// clipped 64 at a time, every lane busy, the verdicts OR-ed back into the owners' words.
__global__ __launch_bounds__(256) void nms_mask_kernel(const float* __restrict__ merged,
                                                       const int* __restrict__ n_merged, int max_k, float thr,
                                                       const int* __restrict__ order_ws,
                                                       unsigned long long* __restrict__ mask_ws) {
  __shared__ unsigned short s_queue[4][128];
  __shared__ unsigned long long s_bits[4][64];
  __shared__ pt s_poly[2][kClipPts][256];
  const int img = blockIdx.y;
  const int m = n_merged[img];
  const int words = (max_k + 63) / 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int idx0 = blockIdx.x * 256 + wave * 64;          // idx of this wave's lane 0
  if (idx0 >= m * words) return;                          // whole wave out of range
  const int idx = idx0 + lane;
  const bool valid = idx < m * words;
  const float* mg = merged + (size_t)img * max_k * 9;
  const int* order = order_ws + (size_t)img * max_k;
  unsigned long long* mask = mask_ws + (size_t)img * max_k * words;
  const int a = idx / words, wd = idx % words;
  const bool boxes_decide = thr >= 1e-3f;
  float ax0 = 0.f, ax1 = 0.f, ay0 = 0.f, ay1 = 0.f;
  const bool live = valid && wd * 64 + 63 > a;
  if (live) {
    const float* qa = mg + 9 * order[a];
    ax0 = fminf(fminf(qa[0], qa[2]), fminf(qa[4], qa[6])); ax1 = fmaxf(fmaxf(qa[0], qa[2]), fmaxf(qa[4], qa[6]));
    ay0 = fminf(fminf(qa[1], qa[3]), fminf(qa[5], qa[7])); ay1 = fmaxf(fmaxf(qa[1], qa[3]), fmaxf(qa[5], qa[7]));
  }
  s_bits[wave][lane] = 0ull;
  int qn = 0;                                             // wave-uniform queue length

  auto drain = [&](int first, int count) {                // entries [first, first+count): one per lane
    if (lane < count) {
      const int e = s_queue[wave][first + lane];
      const int owner = e >> 6, bit = e & 63;
      const int oi = idx0 + owner;
      const int oa = oi / words, ob = (oi % words) * 64 + bit;
      if (quad_iou_lds(mg + 9 * order[oa], mg + 9 * order[ob], &s_poly[0][0][threadIdx.x],
                       &s_poly[1][0][threadIdx.x]) > thr)
        atomicOr(&s_bits[wave][owner], 1ull << bit);
    }
  };

  for (int bb = 0; bb < 64; ++bb) {
    const int b = wd * 64 + bb;
    bool cand = live && b > a && b < m;
    if (cand && boxes_decide) {
      const float* qb = mg + 9 * order[b];
      const float bx0 = fminf(fminf(qb[0], qb[2]), fminf(qb[4], qb[6])), bx1 = fmaxf(fmaxf(qb[0], qb[2]), fmaxf(qb[4], qb[6]));
      const float by0 = fminf(fminf(qb[1], qb[3]), fminf(qb[5], qb[7])), by1 = fmaxf(fmaxf(qb[1], qb[3]), fmaxf(qb[5], qb[7]));
      cand = !(ax1 < bx0 || bx1 < ax0 || ay1 < by0 || by1 < ay0);
    }
    const unsigned long long vote = __ballot(cand);
    if (vote == 0ull) continue;
    if (cand) s_queue[wave][qn + __popcll(vote & ((1ull << lane) - 1ull))] = (unsigned short)((lane << 6) | bb);
    qn += __popcll(vote);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (qn >= 64) {
      drain(qn - 64, 64);
      qn -= 64;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  if (qn > 0) drain(0, qn);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (valid) mask[(size_t)a * words + wd] = s_bits[wave][lane];
}

__device__ __forceinline__ unsigned long long lane_word(unsigned long long v, int src_lane) {   // uniform src_lane
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src_lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src_lane);
  return ((unsigned long long)hi << 32) | lo;
}

}  // namespace

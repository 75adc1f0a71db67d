// Score-map fusion for multi-scale and flip testing of the link (PixelLink) geometry: include/ocr_map_fuse.h has the
// rule, operation by operation.  Built with -ffp-contract=off (Makefile NOFMA): every product and sum rounds to f32.
//
//   ocr_link_map_accumulate   one forward pass's LOGITS -> softmax index 1 at up to four taps -> bilinear sample on the
//                             fusion grid -> acc = first ? w * v : acc + w * v, nine planes [9][n][hf][wf]
//
// One thread owns one cell of the fusion grid and forms all nine planes of it: consecutive lanes own consecutive x, so the
// nine planar stores (and the nine loads of an adding pass) coalesce, and a tap's 16 link logits — one 64-byte row — come
// in as four 16-byte loads.  A tap of zero weight is not loaded at all: at the identity scale a cell reads one tap.
#include "common.h"

namespace {

// decode.hip's direction table (kDx / kDy there, in the order of ocr_link_cc's link planes); tests/test_map_fuse_host.py
// holds the two copies equal
constexpr int kDx[8] = {-1, -1, -1, 1, 1, 1, 0, 0};
constexpr int kDy[8] = {0, 1, -1, 0, 1, -1, -1, 1};

struct Perm {
  int v[8];
};
// the direction a mirrored image calls d: opposite dx, same dy
constexpr Perm mirror_perm() {
  Perm p{};
  for (int d = 0; d < 8; ++d) {
    p.v[d] = -1;
    for (int e = 0; e < 8; ++e)
      if (kDx[e] == -kDx[d] && kDy[e] == kDy[d]) p.v[d] = e;
  }
  return p;
}
constexpr bool perm_is_involution(const Perm& p) {
  for (int d = 0; d < 8; ++d)
    if (p.v[d] < 0 || p.v[d] > 7 || p.v[p.v[d]] != d) return false;
  return true;
}
static_assert(perm_is_involution(mirror_perm()), "the direction table has no mirror for some direction");

// at most 4 workgroups of 4 waves per CU on 256 CUs; the cells beyond that are taken by the grid-stride loop
constexpr unsigned kMaxBlocks = 1024;

unsigned mf_grid(size_t items) {
  size_t b = (items + 255) / 256;
  if (b > kMaxBlocks) b = kMaxBlocks;
  if (b < 1) b = 1;
  return (unsigned)b;
}

struct MfP {
  int n, hs, ws, hf, wf, first;
  float weight, ry, rx;
};

// softmax_pairs_kernel's expression for index 1 (decode.hip), operation for operation
__device__ __forceinline__ float prob1(float a, float b) {
  const float mx = fmaxf(a, b);
  const float ea = expf(a - mx), eb = expf(b - mx);
  const float s = ea + eb;
  return eb / s;
}

// source coordinate of fusion-grid index i along one axis: first tap, second tap, weight of the second
__device__ __forceinline__ void axis_taps(int i, float r, int size, int& i0, int& i1, float& t) {
  const float s = ((float)i + 0.5f) * r - 0.5f;
  const float f0 = floorf(s);
  t = s - f0;
  if (f0 < 0.f) {
    i0 = 0;
    t = 0.f;
  } else if (f0 >= (float)(size - 1)) {
    i0 = size - 1;
    t = 0.f;
  } else {
    i0 = (int)f0;               // 0 <= f0 < size - 1
  }
  i1 = min(i0 + 1, size - 1);
}

// the nine probabilities of source pixel `pix`: P(text), then P(link d) read from pair (FLIP ? perm[d] : d)
template <bool FLIP>
__device__ __forceinline__ void tap_probs(const float* __restrict__ px, const float* __restrict__ lk, size_t pix,
                                          float (&p)[9]) {
  constexpr Perm perm = mirror_perm();
  const float2 a = *reinterpret_cast<const float2*>(px + pix * 2);
  const float4* row = reinterpret_cast<const float4*>(lk + pix * 16);
  float l[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = row[q];
    l[4 * q] = v.x;
    l[4 * q + 1] = v.y;
    l[4 * q + 2] = v.z;
    l[4 * q + 3] = v.w;
  }
  p[0] = prob1(a.x, a.y);
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const int s = FLIP ? perm.v[d] : d;
    p[1 + d] = prob1(l[2 * s], l[2 * s + 1]);
  }
}

// one source row sampled at (c0, c1, tx): out = (tx == 0) ? p0 : p0 * (1 - tx) + p1 * tx
template <bool FLIP>
__device__ __forceinline__ void row_probs(const float* __restrict__ px, const float* __restrict__ lk, size_t row_base,
                                          int c0, int c1, float tx, float (&out)[9]) {
  tap_probs<FLIP>(px, lk, row_base + c0, out);
  if (tx != 0.f) {
    float q[9];
    tap_probs<FLIP>(px, lk, row_base + c1, q);
    const float ux = 1.f - tx;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = out[k] * ux + q[k] * tx;
  }
}

template <bool FLIP>
__global__ __launch_bounds__(256) void map_accumulate_kernel(MfP p, const float* __restrict__ px,
                                                             const float* __restrict__ lk, float* __restrict__ acc) {
  const size_t plane = (size_t)p.n * p.hf * p.wf;                 // <= INT32_MAX (checked by the entry)
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += (size_t)gridDim.x * 256) {
    const int x = (int)(i % (size_t)p.wf);
    const size_t r = i / (size_t)p.wf;
    const int y = (int)(r % (size_t)p.hf);
    const int img = (int)(r / (size_t)p.hf);
    int y0, y1, x0, x1;
    float ty, tx;
    axis_taps(y, p.ry, p.hs, y0, y1, ty);
    axis_taps(x, p.rx, p.ws, x0, x1, tx);
    const int c0 = FLIP ? p.ws - 1 - x0 : x0;                     // all of y0, y1 in [0, hs), c0, c1 in [0, ws)
    const int c1 = FLIP ? p.ws - 1 - x1 : x1;
    const size_t img_base = (size_t)img * p.hs * p.ws;
    float v[9];
    row_probs<FLIP>(px, lk, img_base + (size_t)y0 * p.ws, c0, c1, tx, v);
    if (ty != 0.f) {
      float b[9];
      row_probs<FLIP>(px, lk, img_base + (size_t)y1 * p.ws, c0, c1, tx, b);
      const float uy = 1.f - ty;
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = v[k] * uy + b[k] * ty;
    }
    if (p.first) {
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[(size_t)k * plane + i] = p.weight * v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[(size_t)k * plane + i] = acc[(size_t)k * plane + i] + p.weight * v[k];
    }
  }
}

}  // namespace

extern "C" int ocr_link_map_accumulate(const void* pixel_logits_f32, const void* link_logits_f32, int n, int hs, int ws,
                                       int flip, float weight, int first, void* acc_f32, int hf, int wf, void* stream) {
  OCR_CHECK_ARG(pixel_logits_f32 && link_logits_f32 && acc_f32);
  OCR_CHECK_ARG(n > 0 && hs > 0 && ws > 0 && hf > 0 && wf > 0);
  OCR_CHECK_ARG(std::isfinite(weight) && weight > 0.f);
  OCR_CHECK_ARG(reinterpret_cast<uintptr_t>(pixel_logits_f32) % 8 == 0 && reinterpret_cast<uintptr_t>(link_logits_f32) % 16 == 0 &&
                reinterpret_cast<uintptr_t>(acc_f32) % 4 == 0);
  OCR_CHECK_SHAPE(n <= 65535);
  OCR_CHECK_SHAPE((int64_t)n * hf * wf <= INT32_MAX && (int64_t)n * hs * ws <= INT32_MAX);
  MfP p;
  p.n = n, p.hs = hs, p.ws = ws, p.hf = hf, p.wf = wf, p.first = first != 0;
  p.weight = weight;
  p.ry = (float)hs / (float)hf;
  p.rx = (float)ws / (float)wf;
  const unsigned grid = mf_grid((size_t)n * hf * wf);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* px = static_cast<const float*>(pixel_logits_f32);
  const float* lk = static_cast<const float*>(link_logits_f32);
  float* acc = static_cast<float*>(acc_f32);
  if (flip)
    hipLaunchKernelGGL(map_accumulate_kernel<true>, dim3(grid), dim3(256), 0, st, p, px, lk, acc);
  else
    hipLaunchKernelGGL(map_accumulate_kernel<false>, dim3(grid), dim3(256), 0, st, p, px, lk, acc);
  return ocr_launch_status();
}

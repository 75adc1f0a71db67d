// EAST RBOX geometry (Zhou et al., CVPR 2017): the head activation, the loss of eqs. 7-10 and the per-pixel decode
// of (score, four distances, angle) maps into the raster-ordered quad lists ocr_lanms takes.
//
//   head    score = sigmoid(z0), geo[k] = sigmoid(z[1+k]) * text_scale (k < 4), geo[4] = (sigmoid(z5) - 0.5) * pi/2
//           (nets/model.py:76-80 of the reference).  The angle is evaluated as tanh(z5 / 2) * pi/4 — the same function
//           without the cancellation of sigmoid - 0.5 near z5 = 0.
//   loss    BUILD-DEFINED (the reference tree has no RBOX loss; parity unpinned): dice classification term * 0.01,
//           -log IoU of the axis-aligned boxes the distances span, 1 - cos of the angle difference * 20, mean over
//           ALL pixels.  One streaming pass -> one partial row per workgroup -> f64 finalise by one workgroup: no
//           atomics, reproducible.  The backward pass is one elementwise pass over the finalised sums.
//   decode  pixels with score > thresh, per image in RASTER order (ocr_lanms needs it; the reference's NumPy
//           restore_rectangle_rbox returns the theta >= 0 rows before the theta < 0 rows): per-workgroup counts by
//           ballot + popcount, one scan per image, a write pass with the wave prefix.  No atomic counter.
//
//   mean    the post-NMS filter of EAST's eval script: per kept quad the mean of the score map over the cv2.fillPoly
//           raster of its vertices `box.astype(np.int32) // 4` (raster.h, the bit-exact closed form the label and IoU
//           kernels use).  One workgroup per quad; f64 sums added in a fixed order.
//
// Coordinate geometry: compiled without FMA contraction (Makefile NOFMA), like lanms and boxes.
#include "raster.h"

namespace {

#pragma clang fp contract(off)

constexpr float kHalfPi = 1.57079632679489661923f;
constexpr float kQuarterPi = 0.78539816339744830962f;

__device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }

// ------------------------------------------------------------------------------------------------ head
__global__ __launch_bounds__(256) void rbox_head_fwd_kernel(const float* __restrict__ z, int P, float text_scale,
                                                            float* __restrict__ score, float* __restrict__ geo) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  f32x2 v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = *reinterpret_cast<const f32x2*>(z + (size_t)p * 6 + 2 * k);
  score[p] = sigmoidf_(v[0][0]);
  float* g = geo + (size_t)p * 5;
  g[0] = sigmoidf_(v[0][1]) * text_scale;
  g[1] = sigmoidf_(v[1][0]) * text_scale;
  g[2] = sigmoidf_(v[1][1]) * text_scale;
  g[3] = sigmoidf_(v[2][0]) * text_scale;
  g[4] = tanhf(0.5f * v[2][1]) * kQuarterPi;
}

// sigma recovered from the stored outputs; d sigma / dz = sigma (1 - sigma)
__global__ __launch_bounds__(256) void rbox_head_bwd_kernel(const float* __restrict__ score,
                                                            const float* __restrict__ dscore,
                                                            const float* __restrict__ geo,
                                                            const float* __restrict__ dgeo, int P, float text_scale,
                                                            float* __restrict__ dz) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  float o[6];
  if (dscore) {
    const float s = score[p];
    o[0] = dscore[p] * (s * (1.f - s));
  } else {
    o[0] = 0.f;
  }
  if (dgeo) {
    const float* g = geo + (size_t)p * 5;
    const float* dg = dgeo + (size_t)p * 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float s = g[k] / text_scale;
      o[1 + k] = dg[k] * text_scale * (s * (1.f - s));
    }
    const float s = g[4] / kHalfPi + 0.5f;
    o[5] = dg[4] * kHalfPi * (s * (1.f - s));
  } else {
#pragma unroll
    for (int k = 1; k < 6; ++k) o[k] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) *reinterpret_cast<f32x2*>(dz + (size_t)p * 6 + 2 * k) = f32x2{o[2 * k], o[2 * k + 1]};
}

// ------------------------------------------------------------------------------------------------ loss
// partial row (8 floats, 5 used): sum y p m, sum y m, sum p m, sum L_aabb y m, sum L_theta y m
constexpr int kLossCols = 8, kLossSums = 5;

struct RboxTerms {
  float hp, wp, w, h, ai, au;   // prediction's extents, intersection extents, intersection and union areas
};

__device__ __forceinline__ RboxTerms rbox_areas(const float* g, const float* q) {
  RboxTerms t;
  const float hg = g[0] + g[2], wg = g[1] + g[3];
  t.hp = q[0] + q[2];
  t.wp = q[1] + q[3];
  t.w = fminf(g[1], q[1]) + fminf(g[3], q[3]);
  t.h = fminf(g[0], q[0]) + fminf(g[2], q[2]);
  t.ai = t.w * t.h;
  t.au = hg * wg + t.hp * t.wp - t.ai;
  return t;
}

__global__ __launch_bounds__(256) void rbox_loss_reduce_kernel(int P, const float* __restrict__ yt,
                                                               const float* __restrict__ yp,
                                                               const float* __restrict__ gt,
                                                               const float* __restrict__ gp,
                                                               const float* __restrict__ mask,
                                                               float* __restrict__ partial) {
  __shared__ float red[4][kLossSums];
  float s[kLossSums];
#pragma unroll
  for (int j = 0; j < kLossSums; ++j) s[j] = 0.f;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)P; p += (size_t)gridDim.x * 256) {
    const float m = mask[p], y = yt[p], pr = yp[p];
    const float ym = y * m;
    s[0] += y * pr * m;
    s[1] += ym;
    s[2] += pr * m;
    if (ym != 0.f) {
      float g[5], q[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) { g[k] = gt[p * 5 + k]; q[k] = gp[p * 5 + k]; }
      const RboxTerms t = rbox_areas(g, q);
      const float l_aabb = -logf((t.ai + 1.f) / (t.au + 1.f));
      const float sh = sinf(0.5f * (q[4] - g[4]));       // 1 - cos x = 2 sin^2(x / 2), without the cancellation
      s[3] += l_aabb * ym;
      s[4] += 2.f * sh * sh * ym;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kLossSums; ++j) {
    const float v = wave_sum(s[j]);
    if (lane == 0) red[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < kLossCols)
    partial[(size_t)blockIdx.x * kLossCols + threadIdx.x] =
        threadIdx.x < kLossSums ? red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x] : 0.f;
}

// sums[5], out[4] = (loss, L_cls, mean aabb term, mean theta term): loss = out[1] + out[2] + 20 out[3]
__global__ __launch_bounds__(256) void rbox_loss_finalize_kernel(const float* __restrict__ partial, int T, int P,
                                                                 float* __restrict__ sums, float* __restrict__ out) {
  __shared__ double part[32][kLossCols];
  __shared__ double tot[kLossSums];
  const int j = threadIdx.x & 7, g = threadIdx.x >> 3;       // 32 row groups x 8 columns, rows added in row order
  double a = 0.0;
  for (int t = g; t < T; t += 32) a += (double)partial[(size_t)t * kLossCols + j];
  part[g][j] = a;
  __syncthreads();
  if (threadIdx.x < kLossSums) {
    double s = 0.0;
    for (int k = 0; k < 32; ++k) s += part[k][threadIdx.x];
    tot[threadIdx.x] = s;
    sums[threadIdx.x] = (float)s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double l_cls = 0.01 * (1.0 - 2.0 * tot[0] / (tot[1] + tot[2] + 1e-5));
    const double aabb = tot[3] / (double)P, theta = tot[4] / (double)P;
    out[0] = (float)(aabb + 20.0 * theta + l_cls);
    out[1] = (float)l_cls;
    out[2] = (float)aabb;
    out[3] = (float)theta;
  }
}

// d min(g, q) / dq = 1 only where q < g STRICTLY: at a tie the truth counts as the smaller operand and the prediction
// receives nothing from the intersection
template <class Seed>
__global__ __launch_bounds__(256) void rbox_loss_bwd_kernel(int P, const float* __restrict__ yt,
                                                            const float* __restrict__ gt,
                                                            const float* __restrict__ gp,
                                                            const float* __restrict__ mask,
                                                            const float* __restrict__ sums, Seed seed,
                                                            float* __restrict__ d_cls, float* __restrict__ d_geo) {
  __shared__ float cs[3];
  if (threadIdx.x == 0) {
    const float I = sums[0], U = sums[1] + sums[2] + 1e-5f;
    const float sd = seed.get();
    // d/dp 0.01 (1 - 2 I / U) = 0.01 m (-2 y / U + 2 I / U^2)
    cs[0] = -0.02f * sd / U;
    cs[1] = 0.02f * sd * I / (U * U);
    cs[2] = sd / (float)P;
  }
  __syncthreads();
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)P; p += (size_t)gridDim.x * 256) {
    const float m = mask[p], y = yt[p];
    d_cls[p] = m * (y * cs[0] + cs[1]);
    const float c = y * m * cs[2];
    float o[5];
    if (c != 0.f) {
      float g[5], q[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) { g[k] = gt[p * 5 + k]; q[k] = gp[p * 5 + k]; }
      const RboxTerms t = rbox_areas(g, q);
      const float iu = 1.f / (t.au + 1.f), ii = 1.f / (t.ai + 1.f);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // k = 0, 2 (top, bottom) move the heights: dA_p = W_p, dA_i = w; k = 1, 3 (right, left) the widths
        const float dap = (k & 1) ? t.hp : t.wp;
        const float dai = q[k] < g[k] ? ((k & 1) ? t.h : t.w) : 0.f;
        // L = log(A_u + 1) - log(A_i + 1), A_u = A_g + A_p - A_i
        o[k] = c * ((dap - dai) * iu - dai * ii);
      }
      o[4] = c * 20.f * sinf(q[4] - g[4]);
    } else {
#pragma unroll
      for (int k = 0; k < 5; ++k) o[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) d_geo[p * 5 + k] = o[k];
  }
}

int loss_blocks(int P) {
  int b = ocr_cdiv(P, 256 * 4);
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return b;
}

template <class Seed>
int rbox_loss_bwd_launch(const void* y_true_cls, const void* y_true_geo, const void* y_pred_geo, const void* mask, int P,
                         const void* sums, Seed seed, void* d_cls, void* d_geo, void* stream) {
  OCR_CHECK_ARG(y_true_cls && y_true_geo && y_pred_geo && mask && sums && d_cls && d_geo && P > 0);
  hipLaunchKernelGGL(rbox_loss_bwd_kernel<Seed>, dim3(loss_blocks(P) * 2), dim3(256), 0, static_cast<hipStream_t>(stream), P,
                     static_cast<const float*>(y_true_cls), static_cast<const float*>(y_true_geo),
                     static_cast<const float*>(y_pred_geo), static_cast<const float*>(mask),
                     static_cast<const float*>(sums), seed, static_cast<float*>(d_cls), static_cast<float*>(d_geo));
  return ocr_launch_status();
}

// ------------------------------------------------------------------------------------------------ decode
struct DecodeP {
  int n, hw, w, blocks, max_k;      // blocks = workgroups of 256 raster positions per image
  float thresh, scale;
};

__global__ __launch_bounds__(256) void rbox_count_kernel(DecodeP d, const float* __restrict__ score,
                                                         int* __restrict__ block_count) {
  __shared__ int wc[4];
  const int img = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const bool sel = i < d.hw && score[(size_t)img * d.hw + i] > d.thresh;
  const unsigned long long b = __ballot(sel);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) block_count[img * d.blocks + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// one workgroup per image: block_count -> exclusive offsets in place, total, counts = min(total, max_k)
__global__ __launch_bounds__(256) void rbox_scan_kernel(DecodeP d, int* __restrict__ block_count,
                                                        int* __restrict__ counts, int* __restrict__ total) {
  __shared__ int ws[4];
  __shared__ int carry;
  int* bc = block_count + blockIdx.x * d.blocks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < d.blocks; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < d.blocks ? bc[i] : 0;
    int inc = v;                                        // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int off = carry;
    for (int k = 0; k < wave; ++k) off += ws[k];
    if (i < d.blocks) bc[i] = off + inc - v;
    __syncthreads();
    if (threadIdx.x == 255) carry = off + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    total[blockIdx.x] = carry;
    counts[blockIdx.x] = carry < d.max_k ? carry : d.max_k;
  }
}

__global__ __launch_bounds__(256) void rbox_write_kernel(DecodeP d, const float* __restrict__ score,
                                                         const float* __restrict__ geo,
                                                         const int* __restrict__ block_off, float* __restrict__ boxes) {
  __shared__ int wc[4];
  const int img = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float sc = i < d.hw ? score[(size_t)img * d.hw + i] : 0.f;
  const bool sel = i < d.hw && sc > d.thresh;
  const unsigned long long b = __ballot(sel);
  if (lane == 0) wc[wave] = __popcll(b);
  __syncthreads();
  if (!sel) return;
  int idx = block_off[img * d.blocks + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; ++k) idx += wc[k];
  if (idx >= d.max_k) return;
  const float* g = geo + ((size_t)img * d.hw + i) * 5;
  const float d0 = g[0], d1 = g[1], d2 = g[2], d3 = g[3], th = g[4];
  const float ox = (float)(i % d.w) * d.scale, oy = (float)(i / d.w) * d.scale;
  const float H = d0 + d2, W = d1 + d3;
  const float c = cosf(th), s = sinf(th);
  // R(q) = (qx c + qy s, -qx s + qy c); corner = origin + R(local) - R(anchor)
  float lx[4], ly[4], ax, ay;
  if (th >= 0.f) {
    lx[0] = 0.f; ly[0] = -H; lx[1] = W; ly[1] = -H; lx[2] = W; ly[2] = 0.f; lx[3] = 0.f; ly[3] = 0.f;
    ax = d3; ay = -d2;
  } else {
    lx[0] = -W; ly[0] = -H; lx[1] = 0.f; ly[1] = -H; lx[2] = 0.f; ly[2] = 0.f; lx[3] = -W; ly[3] = 0.f;
    ax = -d1; ay = -d2;
  }
  const float rax = ax * c + ay * s, ray = -ax * s + ay * c;
  float* o = boxes + ((size_t)img * d.max_k + idx) * 9;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o[2 * k] = ox + (lx[k] * c + ly[k] * s) - rax;
    o[2 * k + 1] = oy + (-lx[k] * s + ly[k] * c) - ray;
  }
  o[8] = sc;
}

// ------------------------------------------------------------------------------------------------ mean score
constexpr float kCoordLimit = 4194304.f;      // 2^22: vertices beyond it are clamped (keeps the raster's 16.16 arithmetic in range)

// grid (k), one workgroup per quad.  A quad with a non-finite coordinate has an empty raster.
__global__ __launch_bounds__(256) void quad_mean_score_kernel(const float* __restrict__ quads,
                                                              const float* __restrict__ score, int h, int w,
                                                              float inv_scale, float* __restrict__ mean) {
  __shared__ raster::Seg s_seg[4];
  __shared__ raster::FillEdge s_edge[4];
  __shared__ int s_v[8];
  __shared__ int s_box[4];
  __shared__ int s_fill, s_ok;
  __shared__ double s_sum[4];
  __shared__ int s_cnt[4];
  const float* q = quads + (size_t)blockIdx.x * 8;
  if (threadIdx.x == 0) {
    int ok = 1;
    for (int j = 0; j < 8; ++j) {
      const float c = q[j];
      ok &= isfinite(c) ? 1 : 0;
      // int32(trunc(c)) // 4 for inv_scale = 0.25: the product and its floor are exact in f32 below 2^24
      const float t = fminf(fmaxf(truncf(ok ? c : 0.f), -kCoordLimit), kCoordLimit);
      s_v[j] = (int)fminf(fmaxf(floorf(t * inv_scale), -kCoordLimit), kCoordLimit);
    }
    s_ok = ok;
  }
  __syncthreads();
  if (!s_ok) {
    if (threadIdx.x == 0) mean[blockIdx.x] = 0.f;
    return;
  }
  if (threadIdx.x < 4) {
    const int e = threadIdx.x, e0 = e == 0 ? 3 : e - 1;
    raster::Seg sg;
    raster::FillEdge fe;
    raster::setup_edge(s_v[2 * e0], s_v[2 * e0 + 1], s_v[2 * e], s_v[2 * e + 1], w, h, sg, fe);
    s_seg[e] = sg;
    s_edge[e] = fe;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s_fill = raster::fill_enabled(s_edge, 4, w, h) ? 1 : 0;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
    for (int j = 0; j < 4; ++j) {
      x0 = min(x0, s_v[2 * j]); x1 = max(x1, s_v[2 * j]);
      y0 = min(y0, s_v[2 * j + 1]); y1 = max(y1, s_v[2 * j + 1]);
    }
    s_box[0] = max(x0 - 1, 0);
    s_box[1] = max(y0 - 1, 0);
    s_box[2] = min(x1 + 1, w - 1);
    s_box[3] = min(y1 + 1, h - 1);
  }
  __syncthreads();
  const int bx0 = s_box[0], by0 = s_box[1], bw = s_box[2] - bx0 + 1, bh = s_box[3] - by0 + 1;
  double sum = 0.0;
  int cnt = 0;
  if (bw > 0 && bh > 0) {
    const long long total = (long long)bw * bh;
    for (long long i = threadIdx.x; i < total; i += 256) {
      const int y = by0 + (int)(i / bw), x = bx0 + (int)(i % bw);
      if (raster::covers(s_seg, s_edge, 4, s_fill != 0, x, y)) {
        sum += (double)score[(size_t)y * w + x];
        ++cnt;
      }
    }
  }
  sum = wave_sum_d(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = sum;
    s_cnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const double s = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    mean[blockIdx.x] = c > 0 ? (float)(s / (double)c) : 0.f;
  }
}

}  // namespace

extern "C" int ocr_rbox_head_fwd(const void* z, int P, float text_scale, void* score, void* geo, void* stream) {
  OCR_CHECK_ARG(z && score && geo && P > 0);
  hipLaunchKernelGGL(rbox_head_fwd_kernel, dim3(ocr_cdiv(P, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(z), P, text_scale, static_cast<float*>(score), static_cast<float*>(geo));
  return ocr_launch_status();
}

extern "C" int ocr_rbox_head_bwd(const void* score, const void* dscore, const void* geo, const void* dgeo, int P,
                                 float text_scale, void* dz, void* stream) {
  OCR_CHECK_ARG(score && geo && dz && P > 0);
  hipLaunchKernelGGL(rbox_head_bwd_kernel, dim3(ocr_cdiv(P, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(score), static_cast<const float*>(dscore), static_cast<const float*>(geo),
                     static_cast<const float*>(dgeo), P, text_scale, static_cast<float*>(dz));
  return ocr_launch_status();
}

extern "C" size_t ocr_rbox_loss_workspace(int P) {
  return P > 0 ? (size_t)loss_blocks(P) * kLossCols * sizeof(float) : 0;
}

extern "C" int ocr_rbox_loss_fwd(const void* y_true_cls, const void* y_pred_cls, const void* y_true_geo,
                                 const void* y_pred_geo, const void* mask, int P, void* sums, void* out,
                                 void* workspace, size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(y_true_cls && y_pred_cls && y_true_geo && y_pred_geo && mask && sums && out && workspace && P > 0);
  if (ws_bytes < ocr_rbox_loss_workspace(P)) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int T = loss_blocks(P);
  hipLaunchKernelGGL(rbox_loss_reduce_kernel, dim3(T), dim3(256), 0, st, P, static_cast<const float*>(y_true_cls),
                     static_cast<const float*>(y_pred_cls), static_cast<const float*>(y_true_geo),
                     static_cast<const float*>(y_pred_geo), static_cast<const float*>(mask),
                     static_cast<float*>(workspace));
  hipLaunchKernelGGL(rbox_loss_finalize_kernel, dim3(1), dim3(256), 0, st, static_cast<const float*>(workspace), T, P,
                     static_cast<float*>(sums), static_cast<float*>(out));
  return ocr_launch_status();
}

extern "C" int ocr_rbox_loss_bwd(const void* y_true_cls, const void* y_true_geo, const void* y_pred_geo, const void* mask,
                                 int P, const void* sums, float grad_scale, void* d_cls, void* d_geo, void* stream) {
  return rbox_loss_bwd_launch(y_true_cls, y_true_geo, y_pred_geo, mask, P, sums, SeedStatic{grad_scale}, d_cls, d_geo,
                              stream);
}

extern "C" int ocr_rbox_loss_bwd_dyn(const void* y_true_cls, const void* y_true_geo, const void* y_pred_geo,
                                     const void* mask, int P, const void* sums, float grad_scale, const float* loss_scale,
                                     void* d_cls, void* d_geo, void* stream) {
  OCR_CHECK_ARG(loss_scale != nullptr);
  return rbox_loss_bwd_launch(y_true_cls, y_true_geo, y_pred_geo, mask, P, sums, SeedDevice{grad_scale, loss_scale}, d_cls,
                              d_geo, stream);
}

extern "C" size_t ocr_rbox_decode_workspace(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0 || (long long)n * h * w > 0x7fffffffLL) return 0;
  return (size_t)n * ocr_cdiv(h * w, 256) * sizeof(int);
}

extern "C" int ocr_rbox_decode(const void* score, const void* geo, int n, int h, int w, float score_thresh, float scale,
                               int max_k, void* boxes, void* counts, void* total, void* workspace, size_t ws_bytes,
                               void* stream) {
  OCR_CHECK_ARG(score && geo && boxes && counts && total && workspace);
  OCR_CHECK_ARG(n > 0 && h > 0 && w > 0 && max_k > 0);
  OCR_CHECK_SHAPE((long long)n * h * w <= 0x7fffffffLL && n <= 65535);
  if (ws_bytes < ocr_rbox_decode_workspace(n, h, w)) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  DecodeP d{n, h * w, w, ocr_cdiv(h * w, 256), max_k, score_thresh, scale};
  int* bc = static_cast<int*>(workspace);
  hipLaunchKernelGGL(rbox_count_kernel, dim3(d.blocks, n), dim3(256), 0, st, d, static_cast<const float*>(score), bc);
  hipLaunchKernelGGL(rbox_scan_kernel, dim3(n), dim3(256), 0, st, d, bc, static_cast<int*>(counts),
                     static_cast<int*>(total));
  hipLaunchKernelGGL(rbox_write_kernel, dim3(d.blocks, n), dim3(256), 0, st, d, static_cast<const float*>(score),
                     static_cast<const float*>(geo), static_cast<const int*>(bc), static_cast<float*>(boxes));
  return ocr_launch_status();
}

extern "C" int ocr_quad_mean_score(const void* quads_f32, int k, const void* score_f32, int h, int w, float inv_scale,
                                   void* mean_f32, void* stream) {
  OCR_CHECK_SHAPE(k >= 0 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768 && inv_scale > 0.f && inv_scale <= 1.f);
  if (k == 0) return OCR_OK;
  OCR_CHECK_ARG(quads_f32 && score_f32 && mean_f32);
  hipLaunchKernelGGL(quad_mean_score_kernel, dim3(k), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(quads_f32), static_cast<const float*>(score_f32), h, w, inv_scale,
                     static_cast<float*>(mean_f32));
  return ocr_launch_status();
}

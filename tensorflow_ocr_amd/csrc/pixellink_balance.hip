// PixelLink's instance-balanced cross-entropy (Deng et al. 2018, §3.3) on the device: the per-instance weight map from
// the cover raster, and the loss that uses it.
//
// BUILD-DEFINED.  The reference tree keeps only the remains of this loss: nets/pixellink.py:138-156 `OHNM_batch` takes a
// `weight_mask` and ignores it, the weighted pixel term (:161-168) and the W-gated link weights (:191-192) are commented
// out, and what runs is the plain mean of :160 (pixel_rule 2 of loss_softmax.hip).  What is defined here is the structure
// of that `build_loss` with the paper's weights; parity with an upstream TensorFlow run is unpinned.
//
//   weight map   every live text instance of an image weighs S/N in total (S: cells owned by live instances, N: their
//                number), spread evenly over its S_j cells: w = S / (N S_j); ignored instances, instances hidden
//                completely by later ones and background weigh exactly 0
//   P            = {w > 0};  Neg = {!(label > 0)};  label > 0 with w == 0 (ignored text) is in neither
//   mining       per image k = min(neg_ratio |P|, |Neg|) hardest negatives, tie-inclusive: the radix select and the
//                det_exp score of loss_softmax.hip (loss_math.h), so thresholds compare bit for bit
//   pixel        W = w on P, 1 on mined negatives; sum(CE W) / sum(W), 0 when sum(W) == 0
//   link d       on P: Wp = w [link > 0], Wn = w [!(link > 0)]; sum(L Wp)/sum(Wp) + sum(L Wn)/sum(Wn), zero-guarded
//   total        2 pixel + sum_d link_d.  The mined mask is a constant w.r.t. the gradient.
#include "loss_math.h"

namespace {

// ---------------------------------------------------------------------------------------------- instance weight map
struct WmP {
  int P, h, w, nh, nw;
  double ifx, ify;
};

// owner (1 + polygon index, 0: none) of label cell `cell`: bits 8-15 of the cover word at the cv2.resize INTER_NEAREST
// source index, the expression of pixellink_labels_kernel (labels.hip)
__device__ __forceinline__ unsigned cell_owner(const WmP& p, const unsigned* __restrict__ cv, int cell) {
  const int ox = cell % p.nw, oy = cell / p.nw;
  const int sx = min((int)floor(ox * p.ifx), p.w - 1), sy = min((int)floor(oy * p.ify), p.h - 1);
  const unsigned owner = (cv[(size_t)sy * p.w + sx] >> 8) & 255u;
  return owner > (unsigned)p.P ? 0u : owner;          // a cover map made with another polygon count
}

// grid (blocks, n): area[img][j] = number of label cells owned by polygon j.  Integer counts only: LDS histogram per
// workgroup, one global atomic per non-empty bin.
__global__ __launch_bounds__(256) void instance_area_kernel(WmP p, const unsigned* __restrict__ cover,
                                                            int* __restrict__ area) {
  __shared__ int hist[256];
  const int img = blockIdx.y;
  const unsigned* cv = cover + (size_t)img * p.h * p.w;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int cells = p.nh * p.nw;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < cells; c += gridDim.x * 256) {
    const unsigned owner = cell_owner(p, cv, c);
    if (owner) atomicAdd(&hist[owner], 1);
  }
  __syncthreads();
  const int j = (int)threadIdx.x - 1;                   // bin t counts owner t = polygon t - 1
  if (j >= 0 && j < p.P && hist[threadIdx.x]) atomicAdd(&area[(size_t)img * p.P + j], hist[threadIdx.x]);
}

// grid (blocks, n): every workgroup forms its image's table of per-polygon weights (at most 254 entries) and writes its
// cells from it
__global__ __launch_bounds__(256) void instance_weight_kernel(WmP p, const unsigned* __restrict__ cover,
                                                              const unsigned char* __restrict__ ignore,
                                                              const int* __restrict__ area, float* __restrict__ weight) {
  __shared__ float s_w[256];
  __shared__ int s_tot[2];                              // N, S
  const int img = blockIdx.y;
  if (threadIdx.x < 2) s_tot[threadIdx.x] = 0;
  __syncthreads();
  int mine = 0;
  if ((int)threadIdx.x < p.P) {
    const int a = area[(size_t)img * p.P + threadIdx.x];
    if (a >= 1 && ignore[(size_t)img * p.P + threadIdx.x] == 0) mine = a;
  }
  if (mine) {
    atomicAdd(&s_tot[0], 1);
    atomicAdd(&s_tot[1], mine);
  }
  __syncthreads();
  // one rounding, from double: (double)S / ((double)N * (double)S_j)
  s_w[threadIdx.x] = mine ? (float)((double)s_tot[1] / ((double)s_tot[0] * (double)mine)) : 0.f;
  __syncthreads();
  const unsigned* cv = cover + (size_t)img * p.h * p.w;
  const int cells = p.nh * p.nw;
  float* out = weight + (size_t)img * cells;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < cells; c += gridDim.x * 256) {
    const unsigned owner = cell_owner(p, cv, c);
    out[c] = owner ? s_w[owner - 1] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------- the loss
struct BlP {
  int n, hw, focal;
  float neg_ratio, alpha, gamma;
};

constexpr int kLabelRule = 1;          // pos = label > 0, neg = !pos (nets/pixellink.py)

// One 1024-thread workgroup per image: ohnm_threshold_kernel (loss_softmax.hip) with the positives counted on the weight
// map.
__global__ __launch_bounds__(1024) void balanced_threshold_kernel(BlP p, const float* __restrict__ pl,
                                                                  const float* __restrict__ lab,
                                                                  const float* __restrict__ wgt,
                                                                  float* __restrict__ thr) {
  __shared__ int hist[256];
  __shared__ int s_cnt[2];
  __shared__ unsigned s_prefix;
  __shared__ int s_k;
  const int img = blockIdx.x;
  const float* l = pl + (size_t)img * p.hw * 2;
  const float* y = lab + (size_t)img * p.hw;
  const float* wt = wgt + (size_t)img * p.hw;
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  int np = 0, nn = 0;
  for (int i = threadIdx.x; i < p.hw; i += 1024) {
    np += wt[i] > 0.f ? 1 : 0;
    nn += is_neg(y[i], kLabelRule) ? 1 : 0;
  }
  atomicAdd(&s_cnt[0], np);
  atomicAdd(&s_cnt[1], nn);
  __syncthreads();
  const int n_pos = s_cnt[0], n_neg = s_cnt[1];
  // the product in double (10 * 0.7f rounds up to 7.0f in f32; 10 * (double)0.7f = 6.9999998 mines 6)
  const int k = (int)fmin((double)n_pos * (double)p.neg_ratio, (double)n_neg);
  if (n_pos == 0 || k <= 0) {
    if (threadIdx.x == 0) thr[img] = -1.f;   // nothing is selected (scores are >= 0)
    return;
  }
  if (threadIdx.x == 0) { s_prefix = 0u; s_k = k; }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix;
    const unsigned mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int i = threadIdx.x; i < p.hw; i += 1024) {
      if (!is_neg(y[i], kLabelRule)) continue;
      const unsigned u = __float_as_uint(neg_score(l[2 * i], l[2 * i + 1]));
      if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int kk = s_k, cum = 0, d = 0;
      for (; d < 256; ++d) {
        if (cum + hist[d] >= kk) break;
        cum += hist[d];
      }
      s_prefix = prefix | ((unsigned)d << shift);
      s_k = kk - cum;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) thr[img] = __uint_as_float(s_prefix);
}

// weight of the pixel CE term: w on P, 1 on a mined negative, 0 elsewhere (ignored text among them)
__device__ __forceinline__ float balanced_pixel_weight(float w, float label, float l0, float l1, float thr) {
  if (w > 0.f) return w;
  if (is_neg(label, kLabelRule) && neg_score(l0, l1) <= thr) return 1.f;
  return 0.f;
}

// sums: [0] sum CE*W  [1] sum W  then per direction i: [2+4i] sum L*Wp [3+4i] sum Wp [4+4i] sum L*Wn [5+4i] sum Wn
constexpr int NS = 34;

__global__ __launch_bounds__(256) void balanced_reduce_kernel(BlP p, const float* __restrict__ pl,
                                                              const float* __restrict__ ll,
                                                              const float* __restrict__ plab,
                                                              const float* __restrict__ llab,
                                                              const float* __restrict__ wgt,
                                                              const float* __restrict__ thr,
                                                              float* __restrict__ partial) {
  __shared__ float red[4][NS];
  float s[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) s[j] = 0.f;
  const size_t total = (size_t)p.n * p.hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int img = (int)(i / p.hw);
    const float y = plab[i], w = wgt[i], l0 = pl[2 * i], l1 = pl[2 * i + 1];
    const float W = balanced_pixel_weight(w, y, l0, l1, thr[img]);
    float p1;
    const float ce = ce2(l0, l1, is_pos(y, kLabelRule) ? 1 : 0, &p1);
    s[0] += ce * W;
    s[1] += W;
    if (w > 0.f) {                       // links count on P only
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const float a0 = ll[i * 16 + 2 * d], a1 = ll[i * 16 + 2 * d + 1];
        const bool lp = is_pos(llab[i * 8 + d], kLabelRule);
        float dummy;
        const float L = p.focal ? focal2(a0, a1, lp ? 1 : 0, p.alpha, p.gamma, &dummy) : ce2(a0, a1, lp ? 1 : 0, &dummy);
        const float wp = lp ? w : 0.f, wn = lp ? 0.f : w;
        s[2 + 4 * d] += L * wp;
        s[3 + 4 * d] += wp;
        s[4 + 4 * d] += L * wn;
        s[5 + 4 * d] += wn;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const float v = wave_sum(s[j]);
    if (lane == 0) red[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS)
    partial[(size_t)blockIdx.x * NS + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// sums[34]; loss[0] total, loss[1] pixel term (before the factor 2), loss[2..9] link terms.  Block partials are summed in
// double, as sl_finalize_kernel does.
__global__ void balanced_finalize_kernel(const float* __restrict__ partial, int T, float* __restrict__ sums,
                                         float* __restrict__ loss) {
  __shared__ double part[4][64];
  __shared__ float tot[NS];
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  double a = 0.0;
  if (j < NS)
    for (int t = g; t < T; t += 4) a += (double)partial[(size_t)t * NS + j];
  part[g][j] = a;
  __syncthreads();
  if (threadIdx.x < NS) {
    const float v = (float)(part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
    tot[threadIdx.x] = v;
    sums[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float pixel = tot[1] > 0.f ? tot[0] / tot[1] : 0.f;
    float total = 2.f * pixel;
    loss[1] = pixel;
    for (int d = 0; d < 8; ++d) {
      const float lp = tot[2 + 4 * d], wp = tot[3 + 4 * d], ln = tot[4 + 4 * d], wn = tot[5 + 4 * d];
      const float v = (wp == 0.f ? 0.f : lp / wp) + (wn == 0.f ? 0.f : ln / wn);
      loss[2 + d] = v;
      total += v;
    }
    loss[0] = total;
  }
}

template <class Seed>
__global__ __launch_bounds__(256) void balanced_bwd_kernel(BlP p, const float* __restrict__ pl,
                                                           const float* __restrict__ ll,
                                                           const float* __restrict__ plab,
                                                           const float* __restrict__ llab,
                                                           const float* __restrict__ wgt,
                                                           const float* __restrict__ thr,
                                                           const float* __restrict__ sums, Seed seed,
                                                           float* __restrict__ dpl, float* __restrict__ dll) {
  __shared__ float c_pix, c_pos[8], c_neg[8];
  const float gscale = seed.get();
  if (threadIdx.x == 0) c_pix = sums[1] > 0.f ? 2.f * gscale / sums[1] : 0.f;
  if (threadIdx.x < 8) {
    const float wp = sums[3 + 4 * threadIdx.x], wn = sums[5 + 4 * threadIdx.x];
    c_pos[threadIdx.x] = wp == 0.f ? 0.f : gscale / wp;
    c_neg[threadIdx.x] = wn == 0.f ? 0.f : gscale / wn;
  }
  __syncthreads();
  const size_t total = (size_t)p.n * p.hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int img = (int)(i / p.hw);
    const float y = plab[i], w = wgt[i], l0 = pl[2 * i], l1 = pl[2 * i + 1];
    const bool pos = is_pos(y, kLabelRule);
    const float W = balanced_pixel_weight(w, y, l0, l1, thr[img]);
    float g1 = 0.f;                       // d/dl1 ; d/dl0 = -g1.  A zero weight writes an exact zero
    if (W != 0.f) {
      float p1;
      ce2(l0, l1, pos ? 1 : 0, &p1);
      g1 = (p1 - (pos ? 1.f : 0.f)) * W * c_pix;
    }
    dpl[2 * i] = -g1;
    dpl[2 * i + 1] = g1;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      float gl = 0.f;
      if (w > 0.f) {
        const float a0 = ll[i * 16 + 2 * d], a1 = ll[i * 16 + 2 * d + 1];
        const bool lp = is_pos(llab[i * 8 + d], kLabelRule);
        float dz1;
        if (p.focal) {
          focal2(a0, a1, lp ? 1 : 0, p.alpha, p.gamma, &dz1);
        } else {
          float q1;
          ce2(a0, a1, lp ? 1 : 0, &q1);
          dz1 = q1 - (lp ? 1.f : 0.f);
        }
        gl = dz1 * (w * (lp ? c_pos[d] : c_neg[d]));
      }
      dll[i * 16 + 2 * d] = -gl;
      dll[i * 16 + 2 * d + 1] = gl;
    }
  }
}

// the pixel-term weight map as bytes: 1 on P and on the mined negatives
__global__ void balanced_selected_kernel(BlP p, const float* __restrict__ pl, const float* __restrict__ plab,
                                         const float* __restrict__ wgt, const float* __restrict__ thr,
                                         unsigned char* __restrict__ mask) {
  const size_t total = (size_t)p.n * p.hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int img = (int)(i / p.hw);
    mask[i] = balanced_pixel_weight(wgt[i], plab[i], pl[2 * i], pl[2 * i + 1], thr[img]) != 0.f;
  }
}

// four elements per thread, capped grid (the grid of loss_softmax.hip)
int bl_blocks(size_t total) {
  size_t b = (total + 256 * 4 - 1) / (256 * 4);
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return (int)b;
}

int fill(const ocr_balanced_loss_desc* d, BlP* p) {
  OCR_CHECK_ARG(d != nullptr && d->n > 0 && d->hw > 0);
  OCR_CHECK_ARG(d->focal == 0 || d->focal == 1);
  OCR_CHECK_ARG(d->neg_ratio >= 0.f);                                 // (a NaN ratio fails the comparison too)
  OCR_CHECK_SHAPE((int64_t)d->n * d->hw <= (int64_t)INT32_MAX);       // pixels are counted in int by the mining kernel
  p->n = d->n; p->hw = d->hw; p->focal = d->focal;
  p->neg_ratio = d->neg_ratio; p->alpha = d->alpha; p->gamma = d->gamma;
  return OCR_OK;
}

template <class Seed>
int balanced_bwd_launch(const ocr_balanced_loss_desc* d, const void* pixel_logits, const void* link_logits,
                        const void* pixel_labels, const void* link_labels, const void* pixel_weights,
                        const void* ohnm_threshold, const void* sums34, Seed seed, void* d_pixel_logits,
                        void* d_link_logits, void* stream) {
  BlP p;
  int rc = fill(d, &p);
  if (rc != OCR_OK) return rc;
  OCR_CHECK_ARG(pixel_logits && link_logits && pixel_labels && link_labels && pixel_weights && ohnm_threshold);
  OCR_CHECK_ARG(sums34 && d_pixel_logits && d_link_logits);
  const int T = bl_blocks((size_t)p.n * p.hw) * 2;
  hipLaunchKernelGGL(balanced_bwd_kernel<Seed>, dim3(T), dim3(256), 0, static_cast<hipStream_t>(stream), p,
                     static_cast<const float*>(pixel_logits), static_cast<const float*>(link_logits),
                     static_cast<const float*>(pixel_labels), static_cast<const float*>(link_labels),
                     static_cast<const float*>(pixel_weights), static_cast<const float*>(ohnm_threshold),
                     static_cast<const float*>(sums34), seed, static_cast<float*>(d_pixel_logits),
                     static_cast<float*>(d_link_logits));
  return ocr_launch_status();
}

}  // namespace

extern "C" int ocr_pixellink_instance_weights(const void* cover_u32, const void* ignore_u8, int n, int max_polys, int h,
                                              int w, int new_h, int new_w, void* area_i32, void* weight_f32,
                                              void* stream) {
  OCR_CHECK_ARG(cover_u32 && ignore_u8 && area_i32 && weight_f32);
  OCR_CHECK_SHAPE(n >= 1 && h >= 1 && w >= 1 && new_h >= 1 && new_w >= 1 && max_polys >= 1 && max_polys <= 254);
  OCR_CHECK_SHAPE(n <= 65535 && h <= 16384 && w <= 16384);     // the bounds of ocr_poly_cover, which makes the cover
  OCR_CHECK_SHAPE((int64_t)new_h * new_w <= (int64_t)INT32_MAX);  // cells of one image are indexed and counted in int
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(area_i32, 0, (size_t)n * max_polys * sizeof(int), st) != hipSuccess) return OCR_ERR_HIP;
  const WmP p{max_polys, h, w, new_h, new_w, 1.0 / ((double)new_w / (double)w), 1.0 / ((double)new_h / (double)h)};
  int64_t b = ((int64_t)new_h * new_w + 256 * 4 - 1) / (256 * 4);
  if (b > 256) b = 256;
  const dim3 grid((unsigned)b, (unsigned)n);
  hipLaunchKernelGGL(instance_area_kernel, grid, dim3(256), 0, st, p, static_cast<const unsigned*>(cover_u32),
                     static_cast<int*>(area_i32));
  hipLaunchKernelGGL(instance_weight_kernel, grid, dim3(256), 0, st, p, static_cast<const unsigned*>(cover_u32),
                     static_cast<const unsigned char*>(ignore_u8), static_cast<const int*>(area_i32),
                     static_cast<float*>(weight_f32));
  return ocr_launch_status();
}

extern "C" size_t ocr_balanced_loss_workspace(const ocr_balanced_loss_desc* d) {
  if (!d || d->n <= 0 || d->hw <= 0) return 0;
  return (size_t)bl_blocks((size_t)d->n * d->hw) * NS * sizeof(float);
}

extern "C" int ocr_balanced_loss_fwd(const ocr_balanced_loss_desc* d, const void* pixel_logits, const void* link_logits,
                                     const void* pixel_labels, const void* link_labels, const void* pixel_weights,
                                     void* ohnm_threshold, void* sums34, void* loss10, void* workspace, size_t ws_bytes,
                                     void* stream) {
  BlP p;
  int rc = fill(d, &p);
  if (rc != OCR_OK) return rc;
  OCR_CHECK_ARG(pixel_logits && link_logits && pixel_labels && link_labels && pixel_weights && ohnm_threshold);
  OCR_CHECK_ARG(sums34 && loss10 && workspace);
  if (ws_bytes < ocr_balanced_loss_workspace(d)) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* pl = static_cast<const float*>(pixel_logits);
  const float* plab = static_cast<const float*>(pixel_labels);
  const float* wgt = static_cast<const float*>(pixel_weights);
  hipLaunchKernelGGL(balanced_threshold_kernel, dim3(p.n), dim3(1024), 0, st, p, pl, plab, wgt,
                     static_cast<float*>(ohnm_threshold));
  const int T = bl_blocks((size_t)p.n * p.hw);
  hipLaunchKernelGGL(balanced_reduce_kernel, dim3(T), dim3(256), 0, st, p, pl, static_cast<const float*>(link_logits),
                     plab, static_cast<const float*>(link_labels), wgt, static_cast<const float*>(ohnm_threshold),
                     static_cast<float*>(workspace));
  hipLaunchKernelGGL(balanced_finalize_kernel, dim3(1), dim3(256), 0, st, static_cast<const float*>(workspace), T,
                     static_cast<float*>(sums34), static_cast<float*>(loss10));
  return ocr_launch_status();
}

extern "C" int ocr_balanced_loss_selected(const ocr_balanced_loss_desc* d, const void* pixel_logits,
                                          const void* pixel_labels, const void* pixel_weights,
                                          const void* ohnm_threshold, void* mask_u8, void* stream) {
  BlP p;
  int rc = fill(d, &p);
  if (rc != OCR_OK) return rc;
  OCR_CHECK_ARG(pixel_logits && pixel_labels && pixel_weights && ohnm_threshold && mask_u8);
  hipLaunchKernelGGL(balanced_selected_kernel, dim3(bl_blocks((size_t)p.n * p.hw)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), p, static_cast<const float*>(pixel_logits),
                     static_cast<const float*>(pixel_labels), static_cast<const float*>(pixel_weights),
                     static_cast<const float*>(ohnm_threshold), static_cast<unsigned char*>(mask_u8));
  return ocr_launch_status();
}

extern "C" int ocr_balanced_loss_bwd(const ocr_balanced_loss_desc* d, const void* pixel_logits, const void* link_logits,
                                     const void* pixel_labels, const void* link_labels, const void* pixel_weights,
                                     const void* ohnm_threshold, const void* sums34, float grad_scale,
                                     void* d_pixel_logits, void* d_link_logits, void* stream) {
  return balanced_bwd_launch(d, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights, ohnm_threshold,
                             sums34, SeedStatic{grad_scale}, d_pixel_logits, d_link_logits, stream);
}

extern "C" int ocr_balanced_loss_bwd_dyn(const ocr_balanced_loss_desc* d, const void* pixel_logits,
                                         const void* link_logits, const void* pixel_labels, const void* link_labels,
                                         const void* pixel_weights, const void* ohnm_threshold, const void* sums34,
                                         float grad_scale, const float* loss_scale, void* d_pixel_logits,
                                         void* d_link_logits, void* stream) {
  OCR_CHECK_ARG(loss_scale != nullptr);
  return balanced_bwd_launch(d, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights, ohnm_threshold,
                             sums34, SeedDevice{grad_scale, loss_scale}, d_pixel_logits, d_link_logits, stream);
}

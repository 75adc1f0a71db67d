// f16x2 INFERENCE PRECISION (Graph(precision="f16x2"); test.py --precision f16x2): the f32 forward
// graph of f32_infer.hip (f32 storage, the same element-wise f32 kernels, heads and decode) with every convolution on the
// 16-bit matrix cores at f32 accuracy.  An f32 value v is carried as two IEEE halves,
//     hi = half(v),   lo' = half((v - hi) * 2^11),
// so that x*w = xhi*whi + 2^-11 (xhi*wlo' + xlo'*whi) up to the dropped xlo*wlo term (<= 2^-22 relative): three
// v_mfma_f32_16x16x32_f16 per k-step instead of one v_mfma_f32_32x32x2_f32 per 2 channels, f32 accumulation as before.
// The 2^11 factor keeps lo' out of the half subnormals for ordinary operands (without it |w| ~ 0.015 puts wlo at 2^-18 and
// the error grows 3x .. 2000x: scripts/f16x2_emulate.py, tests/test_f16x2_host.py); the correction products have their own
// accumulators and join the main ones once, in the epilogue.
// RANGE: |x|, |w| >= 65504 cannot be carried by the hi plane.  hi (and lo') saturate to the largest finite half, so such
// an operand gives a wrong but finite result.  Mean-subtracted images (|x| <= 150), batch-normed activations and
// He-initialised weights are orders of magnitude inside the limit.  A NaN operand is NOT made finite: its hi plane carries
// the NaN, so the outputs it reaches are NaN as on the f32 route (a diverged checkpoint looks diverged).
// The operands are IEEE half in BOTH product libraries: f32 in, f32 out, so nothing here follows the 16-bit storage macro
// of common.h (a bfloat16 split would need three planes).  Forward only.  Reference call sites as for ocr_conv2d_f32_mfma:
// slim.conv2d (nets/vgg.py:14-39, nets/resnet_v1.py:97-105, nets/model_vgg_16.py:144).
#include "f32_conv_ep.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

struct SplitP {
  int n, h, w, cin, oh, ow, cout, kh, kw, stride, dil, pt, pl, flags;
  int P;                      // n * oh * ow output pixels
  int nch, nct;               // 32-channel chunks per tap, cout tiles
};

constexpr float kLoScale = 2048.f, kLoInv = 1.f / 2048.f, kHalfMax = 65504.f;

__device__ __forceinline__ void split1(float v, _Float16& hi, _Float16& lo) {
  const float c = (v != v) ? v : fminf(fmaxf(v, -kHalfMax), kHalfMax);      // NaN stays NaN (fminf / fmaxf would drop it)
  hi = (_Float16)c;
  lo = (_Float16)fminf(fmaxf((v - (float)hi) * kLoScale, -kHalfMax), kHalfMax);
}

// cout tile of the conv kernel (and of the packed weight image): 128 couts, or 64 for layers with cout <= 64
inline int split_tc(int cout) { return cout <= 64 ? 64 : 128; }

// Packed weight image, two planes (hi, then lo' at plane_elems): [tap][cout tile][32-channel chunk][kg = 4][co = TC][8]
// halves, zero where the channel or the cout does not exist.  One (tile, chunk) block is exactly the LDS image the conv
// kernel's A fragments read (k-group major, 16 bytes per cout), so staging it is a linear copy.
__global__ void pack_split_kernel(SplitP p, int TC, const float* __restrict__ w, h16x8* __restrict__ hi,
                                  h16x8* __restrict__ lo, size_t total) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    size_t u = i;
    const int co = (int)(u % TC);
    u /= TC;
    const int kg = (int)(u & 3);
    u >>= 2;
    const int ch = (int)(u % p.nch);
    u /= p.nch;
    const int ct = (int)(u % p.nct);
    const int tap = (int)(u / p.nct);
    const int o = ct * TC + co, c0 = ch * 32 + kg * 8;
    h16x8 vh, vl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = (o < p.cout && c0 + j < p.cin) ? w[((size_t)tap * p.cin + c0 + j) * p.cout + o] : 0.f;
      _Float16 a, b;
      split1(v, a, b);
      vh[j] = a;
      vl[j] = b;
    }
    hi[i] = vh;
    lo[i] = vl;
  }
}

// Implicit GEMM, M = cout (A = packed weights), N = output pixels (B = activations), K = taps x cin in 32-channel chunks.
// Workgroup = 4 waves, each wave 64 pixels x 64 couts = 4 x 4 blocks of v_mfma_f32_16x16x32_f16, two accumulator sets
// (main, corr) = 128 accumulator registers.  WN = waves along cout: 2 -> 128 pixels x 128 couts, 1 -> 256 pixels x 64 couts.
// MFMA operand map: lane l holds A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][col l & 15]; D: col = l & 15 (pixel),
// row = 4 (l >> 4) + reg (cout).  LDS images are K-GROUP MAJOR, [kg][row][8 halves]: the 16 rows of one k-group are 256
// contiguous bytes and the planes of the k-groups are a multiple of 256 bytes apart, so each 16-lane group of a
// ds_read_b128 ({0-3, 12-15, 20-27}, ...: rows 0-3, 12-15 of one k-group and 4-11 of the next) covers the 16 slots of a bank
// row once: conflict-free.  Staging item i -> (row = (i & 7) + 8 (i >> 5), kg = (i >> 3) & 3): 8 consecutive lanes write 128
// contiguous bytes (ds_write_b128 banks in 8-lane groups), and a wave's global load covers 16 pixels x 128 contiguous bytes.
// Pipeline: only the GLOBAL LOADS of the next chunk overlap the MFMAs of the current one; the split arithmetic and the LDS
// writes of every chunk run between the two barriers, serialised with the MFMAs (one LDS buffer, one wave per SIMD).
// Epilogue: main + corr * 2^-11, then the steps of f32_conv_ep.h (inference batch norm, bias, residual, ReLU, accumulate).
template <int WN>
__global__ __launch_bounds__(256) void conv_f32_split_kernel(SplitP p, const float* __restrict__ x,
                                                             const h16x8* __restrict__ wp, size_t plane_elems,
                                                             F32Ep ep, float* __restrict__ y) {
  constexpr int WM = 4 / WN, TP = 64 * WM, TC = 64 * WN;
  constexpr int XI = TP * 4 / 256, WI = TC * 4 / 256;
  __shared__ h16x8 xs[2][4][TP];
  __shared__ h16x8 ws[2][4][TC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;
  const int p0 = blockIdx.x * TP, ct = blockIdx.y, co0 = ct * TC;
  // the XI activation pieces (8 channels of one pixel) this thread stages per chunk
  const int s_kg = (tid >> 3) & 3;
  int s_img[XI], s_iy[XI], s_ix[XI];
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const int it = tid + 256 * i, px = (it & 7) + 8 * (it >> 5);
    int q = p0 + px;
    const bool ok = q < p.P;
    if (!ok) q = 0;
    const int ox = q % p.ow;
    q /= p.ow;
    s_ix[i] = ox * p.stride - p.pl;
    s_iy[i] = ok ? (q % p.oh) * p.stride - p.pt : -(1 << 28);      // never inside the image
    s_img[i] = q / p.oh;
  }
  const bool vec_c = (p.cin & 7) == 0 && ((uintptr_t)x & 15) == 0;
  const bool vec_o = (p.cout & 3) == 0 && ((uintptr_t)y & 15) == 0;
  const bool vec_r = (p.cout & 3) == 0 && ((uintptr_t)ep.residual & 15) == 0;
  f32x4 accm[4][4], accc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) accm[a][b] = accc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  float xr[XI][8];
  h16x8 wr[WI][2];
  const int nit = p.kh * p.kw * p.nch;
  int l_tap = 0, l_ch = 0;                                           // (tap, chunk) of the next global load
  auto gload = [&]() {
    const int ky = l_tap / p.kw, kx = l_tap - ky * p.kw;
    const int c = l_ch * 32 + s_kg * 8;
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int iy = s_iy[i] + ky * p.dil, ix = s_ix[i] + kx * p.dil;
      const bool in = (unsigned)iy < (unsigned)p.h && (unsigned)ix < (unsigned)p.w;
      const float* xp = x + (((size_t)s_img[i] * p.h + (in ? iy : 0)) * p.w + (in ? ix : 0)) * p.cin + c;
      if (in && vec_c && c < p.cin) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xp), b = *reinterpret_cast<const f32x4*>(xp + 4);
        xr[i][0] = a[0]; xr[i][1] = a[1]; xr[i][2] = a[2]; xr[i][3] = a[3];
        xr[i][4] = b[0]; xr[i][5] = b[1]; xr[i][6] = b[2]; xr[i][7] = b[3];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) xr[i][e] = (in && c + e < p.cin) ? xp[e] : 0.f;
      }
    }
    const size_t wb = (((size_t)l_tap * p.nct + ct) * p.nch + l_ch) * (4 * TC);
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      wr[i][0] = wp[wb + tid + 256 * i];
      wr[i][1] = wp[plane_elems + wb + tid + 256 * i];
    }
    if (++l_ch == p.nch) { l_ch = 0; ++l_tap; }
  };
  gload();
  for (int it = 0; it < nit; ++it) {
    __syncthreads();                                       // the previous chunk's fragments have been read
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int idx = tid + 256 * i, px = (idx & 7) + 8 * (idx >> 5);
      h16x8 vh, vl;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        _Float16 a, b;
        split1(xr[i][e], a, b);
        vh[e] = a;
        vl[e] = b;
      }
      xs[0][s_kg][px] = vh;
      xs[1][s_kg][px] = vl;
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      (&ws[0][0][0])[tid + 256 * i] = wr[i][0];
      (&ws[1][0][0])[tid + 256 * i] = wr[i][1];
    }
    __syncthreads();
    if (it + 1 < nit) gload();
    h16x8 ah[4], al[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      ah[cb] = ws[0][g][wn * 64 + cb * 16 + r];
      al[cb] = ws[1][g][wn * 64 + cb * 16 + r];
    }
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) {
      const h16x8 bh = xs[0][g][wm * 64 + pb * 16 + r], bl = xs[1][g][wm * 64 + pb * 16 + r];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        accm[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[cb], bh, accm[pb][cb], 0, 0, 0);
        accc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[cb], bh, accc[pb][cb], 0, 0, 0);
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        accc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[cb], bl, accc[pb][cb], 0, 0, 0);
    }
  }
  // D block (pb, cb): lane (r, g), register e: pixel = 16 pb + r, cout = 16 cb + 4 g + e
#pragma unroll
  for (int pb = 0; pb < 4; ++pb) {
    const int q = p0 + wm * 64 + pb * 16 + r;
    if (q >= p.P) continue;
    float* yp = y + (size_t)q * p.cout;
    const float* rp = ep.residual ? ep.residual + (size_t)q * p.cout : nullptr;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int co = co0 + wn * 64 + cb * 16 + 4 * g;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = accm[pb][cb][e] + accc[pb][cb][e] * kLoInv;
      f32_ep_store4(v, p.flags, ep, co, p.cout, vec_o, vec_r, yp, rp);
    }
  }
}

bool split_desc_ok(const ocr_conv_desc* d) {
  return d && d->n > 0 && d->h > 0 && d->w > 0 && d->oh > 0 && d->ow > 0 && d->cin > 0 && d->cout > 0 && d->kh > 0 &&
         d->kw > 0 && d->stride > 0 && d->dilation > 0;
}

// halves per plane of the packed weight image
size_t split_plane_elems(const ocr_conv_desc* d) {
  const int tc = split_tc(d->cout);
  return (size_t)d->kh * d->kw * ocr_cdiv(d->cout, tc) * ocr_cdiv(d->cin, 32) * 4 * tc * 8;
}

int launch_split(const ocr_conv_desc* d, int flags, const void* x, const void* w_hwio, const F32Ep& ep, void* y,
                 void* workspace, size_t workspace_bytes, void* stream) {
  OCR_CHECK_ARG(split_desc_ok(d) && x && w_hwio && y && workspace);
  OCR_CHECK_ARG(d->flip_taps == 0);                        // forward only, as ocr_conv2d_f32_mfma
  OCR_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  if (workspace_bytes < ocr_conv2d_f32_split_workspace(d)) return OCR_ERR_WORKSPACE;   // as every other workspace of the ABI
  OCR_CHECK_SHAPE((size_t)d->n * d->oh * d->ow < (1ull << 31));
  const int tc = split_tc(d->cout);
  SplitP p{d->n, d->h, d->w, d->cin, d->oh, d->ow, d->cout, d->kh, d->kw, d->stride, d->dilation, d->pad_top, d->pad_left,
           flags, d->n * d->oh * d->ow, ocr_cdiv(d->cin, 32), ocr_cdiv(d->cout, tc)};
  const size_t plane = split_plane_elems(d), vecs = plane / 8;
  h16x8* hi = static_cast<h16x8*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  size_t pb = (vecs + 255) / 256;
  if (pb > 65536) pb = 65536;
  hipLaunchKernelGGL(pack_split_kernel, dim3((unsigned)pb), dim3(256), 0, st, p, tc, static_cast<const float*>(w_hwio), hi,
                     hi + vecs, vecs);
  if (tc == 64)
    hipLaunchKernelGGL(conv_f32_split_kernel<1>, dim3(ocr_cdiv(p.P, 256), p.nct), dim3(256), 0, st, p,
                       static_cast<const float*>(x), hi, vecs, ep, static_cast<float*>(y));
  else
    hipLaunchKernelGGL(conv_f32_split_kernel<2>, dim3(ocr_cdiv(p.P, 128), p.nct), dim3(256), 0, st, p,
                       static_cast<const float*>(x), hi, vecs, ep, static_cast<float*>(y));
  return ocr_launch_status();
}

}  // namespace

// bytes of the packed-weight workspace ocr_conv2d_f32_split needs for `d` (0: invalid descriptor)
extern "C" size_t ocr_conv2d_f32_split_workspace(const ocr_conv_desc* d) {
  if (!split_desc_ok(d)) return 0;
  return split_plane_elems(d) * 2 * sizeof(_Float16);
}

// The contract of ocr_conv2d_f32_mfma (flags OCR_CONV_BIAS, OCR_CONV_RELU, OCR_CONV_ACCUM_F16; x f32 NHWC, w f32 HWIO, y f32
// NHWC) plus the workspace: the weights are split and packed into it on `stream` by every call (a load_state_dict between
// two calls can never meet stale planes), then the convolution reads them.  workspace: 16-byte aligned device memory.
// A thin caller of the kernels of ocr_conv2d_f32_split_ep: the three flags it always took, nothing else.
extern "C" int ocr_conv2d_f32_split(const ocr_conv_desc* d, const void* x, const void* w_hwio, const void* bias, void* y,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  OCR_CHECK_ARG(d);
  OCR_CHECK_ARG(!(d->flags & ~kF32PlainFlags));            // a request this entry does not serve is refused, not dropped
  OCR_CHECK_ARG(!(d->flags & OCR_CONV_BIAS) || bias);
  return launch_split(d, d->flags, x, w_hwio, F32Ep{static_cast<const float*>(bias), nullptr, nullptr, nullptr},
                      y, workspace, workspace_bytes, stream);
}

// ... with the whole epilogue of f32_conv_ep.h (OCR_CONV_AFFINE, OCR_CONV_RESIDUAL, OCR_CONV_ACCUM_IN as well): a frozen
// batch norm, the bottleneck's residual add and the ReLU inside the convolution (Graph(fold_bn=True)).
extern "C" int ocr_conv2d_f32_split_ep(const ocr_conv_desc* d, const void* x, const void* w_hwio,
                                       const ocr_conv_f32_epilogue* epilogue, void* y, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  OCR_CHECK_ARG(d);
  F32Ep ep;
  OCR_CHECK_ARG(!(d->flags & ~kF32EpFlags));
  OCR_CHECK_ARG(f32_ep_args(d->flags, epilogue, &ep));
  return launch_split(d, d->flags, x, w_hwio, ep, y, workspace, workspace_bytes, stream);
}

// The f32 epilogue of the two inference-precision convolutions (conv_f32_mfma_kernel in f32_infer.hip, conv_f32_split_kernel
// in f16x2_infer.hip): one pixel's four consecutive couts at a time, on the finished f32 accumulator.  Steps, in order:
//   OCR_CONV_ACCUM_IN   v += y_old                       (second half of a concat-free 1x1 convolution, before its batch norm)
//   OCR_CONV_AFFINE     v = v * scale[co] + shift[co]    (inference-mode batch norm: the expression of bn_relu_f32_kernel)
//   OCR_CONV_BIAS       v += bias[co]
//   OCR_CONV_RESIDUAL   v += residual[pixel][co]         (bottleneck tail, nets/resnet_v1.py:104-111)
//   OCR_CONV_RELU       v < 0 -> 0                       (a NaN stays NaN)
//   OCR_CONV_ACCUM_F16  v += y_old                       (after the ReLU: the meaning it always had)
// Every operand is loaded HERE, after the K loop (nothing of it is live while the accumulators fill the register file).  y_old
// is read by the lane that stores the same four elements, so ACCUM_IN / ACCUM_F16 work in place; `residual` must not overlap y.
#pragma once
#include "common.h"

struct F32Ep {
  const float *bias, *scale, *shift, *residual;
};

// flags an `_ep` entry point takes / the ones the plain entry points always took
constexpr int kF32EpFlags = OCR_CONV_BIAS | OCR_CONV_RELU | OCR_CONV_ACCUM_F16 | OCR_CONV_AFFINE | OCR_CONV_RESIDUAL |
                            OCR_CONV_ACCUM_IN;
constexpr int kF32PlainFlags = OCR_CONV_BIAS | OCR_CONV_RELU | OCR_CONV_ACCUM_F16;

// host: the argument contract of the `_ep` entry points; fills `out` (NULL members where the flag is clear)
static inline bool f32_ep_args(int flags, const ocr_conv_f32_epilogue* ep, F32Ep* out) {
  *out = F32Ep{nullptr, nullptr, nullptr, nullptr};
  if ((flags & OCR_CONV_ACCUM_IN) && (flags & OCR_CONV_ACCUM_F16)) return false;
  if (flags & OCR_CONV_BIAS) {
    if (!ep || !ep->bias) return false;
    out->bias = static_cast<const float*>(ep->bias);
  }
  if (flags & OCR_CONV_AFFINE) {
    if (!ep || !ep->scale || !ep->shift) return false;
    out->scale = static_cast<const float*>(ep->scale);
    out->shift = static_cast<const float*>(ep->shift);
  }
  if (flags & OCR_CONV_RESIDUAL) {
    if (!ep || !ep->residual) return false;
    out->residual = static_cast<const float*>(ep->residual);
  }
  return true;
}

// v: accumulators of couts co .. co + 3 of the pixel whose rows of y / residual are yp / rp.  vec_o: cout % 4 == 0 and y is
// 16-byte aligned; vec_r: the same for residual.  Couts >= cout are neither read nor stored.
__device__ __forceinline__ void f32_ep_store4(float (&v)[4], int flags, const F32Ep& ep, int co, int cout, bool vec_o,
                                              bool vec_r, float* yp, const float* rp) {
  const bool full = co + 3 < cout;
  float yo[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
  if (flags & (OCR_CONV_ACCUM_IN | OCR_CONV_ACCUM_F16)) {
    if (vec_o && full) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(yp + co);
      yo[0] = t[0]; yo[1] = t[1]; yo[2] = t[2]; yo[3] = t[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (co + e < cout) yo[e] = yp[co + e];
    }
  }
  if (flags & OCR_CONV_RESIDUAL) {
    if (vec_r && full) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(rp + co);
      rs[0] = t[0]; rs[1] = t[1]; rs[2] = t[2]; rs[3] = t[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (co + e < cout) rs[e] = rp[co + e];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (co + e >= cout) continue;
    float t = v[e];
    if (flags & OCR_CONV_ACCUM_IN) t += yo[e];
    if (flags & OCR_CONV_AFFINE) t = t * ep.scale[co + e] + ep.shift[co + e];
    if (flags & OCR_CONV_BIAS) t += ep.bias[co + e];
    if (flags & OCR_CONV_RESIDUAL) t += rs[e];
    if ((flags & OCR_CONV_RELU) && t < 0.f) t = 0.f;
    if (flags & OCR_CONV_ACCUM_F16) t += yo[e];
    v[e] = t;
  }
  if (vec_o && full) {
    *reinterpret_cast<f32x4*>(yp + co) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (co + e < cout) yp[co + e] = v[e];
  }
}

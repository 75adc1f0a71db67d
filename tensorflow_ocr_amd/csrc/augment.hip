// Device-side training augmentation (the flow the reference keeps disabled, datasets/icdar.py:576-615:
// random scale, crop_area, pad to a square, resize — plus the PixelLink recipe's 90-degree rotations and
// colour distortion): ONE inverse-affine warp with a colour matrix over the whole batch, one launch,
// reading the n decoded uint8 RGB images where the generator's pinned upload put them (one slab, any
// sizes, any byte offsets) and writing the f32 [n][S][S][3] batch.
//
// Everything geometric is integer so that a NumPy restatement matches bit for bit
// (tests/test_gpu_augment.py): per output pixel (dx, dy) of image b, with the record's 16.16 inverse map A,
//     X16 = A0*dx + A1*dy + A2                        (int64; Y16 from A3..A5)
//     X5  = (X16 + 1024) >> 11                        (arithmetic shift = floor; 1/32-pixel coordinates)
//     sx  = X5 >> 5, fx = X5 & 31                     (same for y)
//     v_c = sum over the 2x2 taps of w * s_c,  w = (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx*fy  (sum 1024)
//     p_c = (float)v_c * (1/1024)                     (exact)
//     out_c = min(max(((col[c][0]*p_r + col[c][1]*p_g) + col[c][2]*p_b) + col[c][3], 0), 255)
// A tap outside [0,W) x [0,H) contributes 0 and is NOT loaded (zero padding, the reference's im_padded):
// no address outside [src_off, src_off + 3*H*W) is ever formed.  The half-pixel convention
// u = M(d + 0.5) - 0.5 is folded into A2 / A5 by the host (datasets/augment.py); the kernel knows nothing
// of it.  The colour arithmetic is f32, left to right, built with -ffp-contract=off (Makefile NOFMA).
//
// blockIdx.y is the image, so the record is wave-uniform (scalar loads, SGPRs).  A thread produces four
// adjacent pixels of an output row = 48 bytes, stored as three float4 when S is a multiple of 4 (every
// row is then 16-byte aligned) and element by element otherwise.  Source loads are byte loads: image
// offsets in the slab are arbitrary and 3*H*W is often odd.  No LDS.  HBM-bound: at most 12 source bytes
// per pixel, neighbours' taps L2-resident, 12 bytes written.
#include "common.h"

namespace {

constexpr int PX = 4;            // output pixels per thread

__device__ __forceinline__ void warp_pixel(const unsigned char* __restrict__ img, int H, int W, long long X16,
                                           long long Y16, const float (&col)[3][4], float* __restrict__ o) {
  const long long X5 = (X16 + 1024) >> 11, Y5 = (Y16 + 1024) >> 11;
  const int fx = (int)(X5 & 31), fy = (int)(Y5 & 31);
  // [-2, W] keeps "both taps outside" what it was and makes the coordinate an int whatever A holds
  const long long sxl = X5 >> 5, syl = Y5 >> 5;
  const int sx = (int)(sxl < -2 ? -2 : (sxl > W ? W : sxl));
  const int sy = (int)(syl < -2 ? -2 : (syl > H ? H : syl));
  const bool x0 = sx >= 0 && sx < W, x1 = sx + 1 >= 0 && sx + 1 < W;
  const bool y0 = sy >= 0 && sy < H, y1 = sy + 1 >= 0 && sy + 1 < H;
  const int w00 = (32 - fx) * (32 - fy), w10 = fx * (32 - fy), w01 = (32 - fx) * fy, w11 = fx * fy;
  int v0 = 0, v1 = 0, v2 = 0;
  if (y0) {
    const long long row = (long long)sy * W;
    if (x0) {
      const unsigned char* s = img + (row + sx) * 3;
      v0 += w00 * s[0]; v1 += w00 * s[1]; v2 += w00 * s[2];
    }
    if (x1) {
      const unsigned char* s = img + (row + sx + 1) * 3;
      v0 += w10 * s[0]; v1 += w10 * s[1]; v2 += w10 * s[2];
    }
  }
  if (y1) {
    const long long row = (long long)(sy + 1) * W;
    if (x0) {
      const unsigned char* s = img + (row + sx) * 3;
      v0 += w01 * s[0]; v1 += w01 * s[1]; v2 += w01 * s[2];
    }
    if (x1) {
      const unsigned char* s = img + (row + sx + 1) * 3;
      v0 += w11 * s[0]; v1 += w11 * s[1]; v2 += w11 * s[2];
    }
  }
  const float pr = (float)v0 * (1.0f / 1024), pg = (float)v1 * (1.0f / 1024), pb = (float)v2 * (1.0f / 1024);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = ((col[c][0] * pr + col[c][1] * pg) + col[c][2] * pb) + col[c][3];
    o[c] = fminf(fmaxf(t, 0.f), 255.f);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void augment_u8_batch_kernel(const unsigned char* __restrict__ slab,
                                                               const ocr_augment_desc* __restrict__ desc, int S,
                                                               int quads_per_row, float* __restrict__ dst) {
  const int b = blockIdx.y;
  const ocr_augment_desc& d = desc[b];                       // wave-uniform: scalar loads
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int dy = q / quads_per_row;
  if (dy >= S) return;
  const int dx0 = (q - dy * quads_per_row) * PX;
  const int H = d.H, W = d.W;
  const unsigned char* img = slab + d.src_off;
  const long long A0 = d.A[0], A3 = d.A[3];
  long long X16 = A0 * dx0 + d.A[1] * dy + d.A[2];
  long long Y16 = A3 * dx0 + d.A[4] * dy + d.A[5];
  float col[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) col[c][k] = d.col[c][k];
  float* out = dst + (((size_t)b * S + dy) * S + dx0) * 3;
  if (VEC) {                                                 // S % 4 == 0: all four pixels exist, 48 aligned bytes
    float o[PX * 3];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      warp_pixel(img, H, W, X16, Y16, col, o + 3 * j);
      X16 += A0;
      Y16 += A3;
    }
    float4* o4 = reinterpret_cast<float4*>(out);
    o4[0] = make_float4(o[0], o[1], o[2], o[3]);
    o4[1] = make_float4(o[4], o[5], o[6], o[7]);
    o4[2] = make_float4(o[8], o[9], o[10], o[11]);
  } else {
    for (int j = 0; j < PX && dx0 + j < S; ++j) {
      float o[3];
      warp_pixel(img, H, W, X16, Y16, col, o);
      out[3 * j] = o[0];
      out[3 * j + 1] = o[1];
      out[3 * j + 2] = o[2];
      X16 += A0;
      Y16 += A3;
    }
  }
}

}  // namespace

extern "C" int ocr_augment_u8_batch(const void* slab_u8, const void* desc, int n, int S, void* dst_f32, void* stream) {
  OCR_CHECK_ARG(slab_u8 && desc && dst_f32 && n > 0 && S > 0);
  OCR_CHECK_ARG(((uintptr_t)desc & 7) == 0 && ((uintptr_t)dst_f32 & 3) == 0);
  OCR_CHECK_SHAPE(n <= 65535 && S <= 32768);                 // grid y; rows * quads within int
  const int quads_per_row = ocr_cdiv(S, PX);
  const dim3 grid((unsigned)ocr_cdiv(S * quads_per_row, 256), (unsigned)n);
  const unsigned char* slab = static_cast<const unsigned char*>(slab_u8);
  const ocr_augment_desc* dsc = static_cast<const ocr_augment_desc*>(desc);
  float* dst = static_cast<float*>(dst_f32);
  if (S % PX == 0 && ((uintptr_t)dst_f32 & 15) == 0)
    hipLaunchKernelGGL(augment_u8_batch_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), slab, dsc, S,
                       quads_per_row, dst);
  else
    hipLaunchKernelGGL(augment_u8_batch_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), slab, dsc, S,
                       quads_per_row, dst);
  return ocr_launch_status();
}

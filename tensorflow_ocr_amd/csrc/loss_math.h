// Per-element arithmetic of the softmax cross-entropy losses, shared by loss_softmax.hip (the reference's rules) and
// pixellink_balance.hip (the instance-balanced PixelLink loss): label predicates, the mining score as a fixed f32
// sequence, the 2-class CE and the focal term.  One definition, so that a threshold mined by either file orders the same
// bits.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ bool is_pos(float label, int rule) { return rule ? label > 0.f : label == 1.f; }
__device__ __forceinline__ bool is_neg(float label, int rule) { return rule ? !(label > 0.f) : label == 0.f; }

// exp(x) as a FIXED sequence of IEEE f32 operations (no FMA contraction, no library call): the
// CPU checker evaluates the same sequence in numpy float32, so the mining scores — and with them the
// k-th-smallest threshold and the mined mask, which are index work — agree bit for bit.
// Range reduction x = n ln2 + r (Cody-Waite), degree-6 Taylor in r (|r| <= 0.347: ~1 ulp), 2^n scale.
__device__ __forceinline__ float det_exp(float x) {
#pragma clang fp contract(off)
  x = fminf(fmaxf(x, -80.f), 80.f);
  const float n = rintf(x * 1.44269504f);
  float r = x - n * 0.693145751953125f;
  r = r - n * 1.42860677e-06f;
  float p = 1.3888889e-03f;
  p = p * r + 8.3333338e-03f;
  p = p * r + 4.1666668e-02f;
  p = p * r + 1.6666667e-01f;
  p = p * r + 0.5f;
  p = p * r + 1.0f;
  p = p * r + 1.0f;
  return ldexpf(p, (int)n);
}

// P(class 0) of a 2-way softmax, = exp(l0) / (exp(l0) + exp(l1))
__device__ __forceinline__ float neg_score(float l0, float l1) {
#pragma clang fp contract(off)
  return 1.f / (1.f + det_exp(l1 - l0));
}

// 2-class CE and softmax of logits (l0, l1) for class t
__device__ __forceinline__ float ce2(float l0, float l1, int t, float* p1) {
  const float m = fmaxf(l0, l1);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  const float s = e0 + e1;
  *p1 = e1 / s;
  return logf(s) + m - (t ? l1 : l0);
}

__device__ __forceinline__ float focal2(float l0, float l1, int t, float alpha, float gamma, float* dz1) {
  // L = -a_t (1-p)^g log p,  p = softmax prob of the true class; dz1 = dL/d(l1)
  const float m = fmaxf(l0, l1);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  const float s = e0 + e1;
  const float p = (t ? e1 : e0) / s;
  const float logp = (t ? l1 : l0) - m - logf(s);
  const float a = t ? alpha : 1.f - alpha;
  const float om = 1.f - p;
  const float omg = powf(fmaxf(om, 1e-30f), gamma);
  const float dzt = a * (gamma * omg * p * logp - omg * om);   // dL/dz_true
  *dz1 = t ? dzt : -dzt;
  return -a * omg * logp;
}

}  // namespace

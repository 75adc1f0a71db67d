// Parameter update and weight re-packing.
//
// The host keeps all trainable parameters of a tower in ONE flat f32 buffer
// (regularised conv weights first, then everything else) with gradients, Adam
// moments and EMA shadows in identically laid out buffers, so the whole update —
// L2 regulariser gradient, un-scaling of the f16 loss scale, Adam, exponential
// moving average — is a single streaming launch.
//
// Reference: tf.train.AdamOptimizer + exponential_decay + ExponentialMovingAverage
// (multigpu_train.py:103-107,137-142), slim.l2_regularizer (nets/model.py:103),
// MomentumOptimizer (train_pixellink.py:243).
#include "common.h"

namespace {

struct AdamP {
  float lr_t, beta1, beta2, eps, wd, inv_scale, ema_decay;
  long long n, n_reg;
};

// Dynamic loss scaling (ocr_loss_scale_state, include/ocr_hip.h): the *_dyn entry points instantiate the SAME kernel
// bodies with a parameter block that carries the state pointer.  step_guard() is where the two differ: the static
// block hands back its host factor (the instantiation the static entry points launch is what it always was), the
// dynamic one reads the skip decision and 1 / scale that ocr_grad_check_f32 left on the device.
struct AdamDynP : AdamP {
  const ocr_loss_scale_state* st;     // inv_scale holds the reducer's host factor (1 or 1 / world)
};

template <class P>
__device__ __forceinline__ bool step_guard(const P& a, float* inv_scale) {
  *inv_scale = a.inv_scale;
  return false;
}
template <class P>
__device__ __forceinline__ bool step_guard_dyn(const P& a, float* inv_scale) {
  if (a.st->skip) return true;                          // uniform: every workgroup leaves before its first store
  *inv_scale = a.inv_scale * a.st->inv_scale_used;
  return false;
}
__device__ __forceinline__ bool step_guard(const AdamDynP& a, float* inv_scale) { return step_guard_dyn(a, inv_scale); }

// Global-norm clipping (ocr_grad_clip_state, include/ocr_hip.h): a third parameter block for the same bodies.  The factor
// comes whole from the device: g_mul = base * coef already carries the host factor and, in the dynamic mode, 1 / scale,
// so one instantiation serves a numeric and a dynamic loss scale (inv_scale of the block is not read).
struct AdamClipP : AdamP {
  const ocr_grad_clip_state* cs;
};
template <class P>
__device__ __forceinline__ bool step_guard_clip(const P& a, float* inv_scale) {
  if (a.cs->skip) return true;                          // uniform, as in step_guard_dyn
  *inv_scale = a.cs->g_mul;
  return false;
}
__device__ __forceinline__ bool step_guard(const AdamClipP& a, float* inv_scale) { return step_guard_clip(a, inv_scale); }

template <class P>
__global__ void adam_kernel(P a, float* __restrict__ w, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            float* __restrict__ ema) {
  float inv_scale;
  if (step_guard(a, &inv_scale)) return;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long long)gridDim.x * 256) {
    float wi = w[i];
    float gi = g[i] * inv_scale;
    if (i < a.n_reg) gi += a.wd * wi;
    const float mi = a.beta1 * m[i] + (1.f - a.beta1) * gi;
    const float vi = a.beta2 * v[i] + (1.f - a.beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    wi -= a.lr_t * mi / (sqrtf(vi) + a.eps);
    w[i] = wi;
    if (ema) {
      const float s = ema[i];
      ema[i] = s - (1.f - a.ema_decay) * (s - wi);
    }
  }
}

struct MomP {
  float lr, momentum, wd, inv_scale, ema_decay;
  long long n, n_reg;
};

struct MomDynP : MomP {
  const ocr_loss_scale_state* st;
};
__device__ __forceinline__ bool step_guard(const MomDynP& a, float* inv_scale) { return step_guard_dyn(a, inv_scale); }
struct MomClipP : MomP {
  const ocr_grad_clip_state* cs;
};
__device__ __forceinline__ bool step_guard(const MomClipP& a, float* inv_scale) { return step_guard_clip(a, inv_scale); }

template <class P>
__global__ void momentum_kernel(P a, float* __restrict__ w, const float* __restrict__ g,
                                float* __restrict__ acc, float* __restrict__ ema) {
  float inv_scale;
  if (step_guard(a, &inv_scale)) return;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long long)gridDim.x * 256) {
    float wi = w[i];
    float gi = g[i] * inv_scale;
    if (i < a.n_reg) gi += a.wd * wi;
    const float ai = a.momentum * acc[i] + gi;
    acc[i] = ai;
    wi -= a.lr * ai;
    w[i] = wi;
    if (ema) {
      const float s = ema[i];
      ema[i] = s - (1.f - a.ema_decay) * (s - wi);
    }
  }
}

// HWIO f32 [taps][cin][cout] -> w_kc f16 [taps][cout][cin] and w_ck f16 [taps][cin][cout]
__global__ void pack_weights_kernel(const float* __restrict__ w, int taps, int cin, int cout,
                                    half_t* __restrict__ w_kc, half_t* __restrict__ w_ck) {
  __shared__ float tile[32][33];
  const int tap = blockIdx.z;
  const int ci0 = blockIdx.y * 32, co0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const float* wt = w + (size_t)tap * cin * cout;
  for (int k = ty; k < 32; k += 8) {
    const int ci = ci0 + k, co = co0 + tx;
    float v = (ci < cin && co < cout) ? wt[(size_t)ci * cout + co] : 0.f;
    tile[k][tx] = v;
    if (w_ck && ci < cin && co < cout) w_ck[((size_t)tap * cin + ci) * cout + co] = (half_t)v;
  }
  __syncthreads();
  if (w_kc) {
    for (int k = ty; k < 32; k += 8) {
      const int co = co0 + k, ci = ci0 + tx;
      if (ci < cin && co < cout) w_kc[((size_t)tap * cout + co) * cin + ci] = (half_t)tile[tx][k];
    }
  }
}

// The same re-pack for MANY layers in one launch (after the optimiser step: 14 launches of ~7 us per VGG step, 62 per
// ResNet-50 step otherwise).  items[i] = one layer; block_first[i] = first block of layer i (block_first[n] = grid):
// a block finds its layer by bisection, then its (tap, ci tile, co tile) inside it.
struct PackItem {
  const float* w;
  half_t* w_kc;
  half_t* w_ck;
  int taps, cin, cout, tiles_ci, tiles_co;
  int ld_ck;                 // row length of w_ck: cout, or 32 for the fuse heads' zero-padded [cin][32] copy
};

__global__ void pack_weights_batch_kernel(const PackItem* __restrict__ items, const int* __restrict__ block_first, int n) {
  __shared__ float tile[32][33];
  int lo = 0, hi = n;                              // block_first[lo] <= blockIdx.x < block_first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int)blockIdx.x >= block_first[mid]) lo = mid;
    else hi = mid;
  }
  const PackItem it = items[lo];
  int b = (int)blockIdx.x - block_first[lo];
  const int cot = b % it.tiles_co;
  b /= it.tiles_co;
  const int cit = b % it.tiles_ci;
  const int tap = b / it.tiles_ci;
  const int ci0 = cit * 32, co0 = cot * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float* wt = it.w + (size_t)tap * it.cin * it.cout;
  for (int k = ty; k < 32; k += 8) {
    const int ci = ci0 + k, co = co0 + tx;
    const float v = (ci < it.cin && co < it.cout) ? wt[(size_t)ci * it.cout + co] : 0.f;
    tile[k][tx] = v;
    if (it.w_ck && ci < it.cin && co < it.cout) it.w_ck[((size_t)tap * it.cin + ci) * it.ld_ck + co] = (half_t)v;
  }
  __syncthreads();
  if (it.w_kc) {
    for (int k = ty; k < 32; k += 8) {
      const int co = co0 + k, ci = ci0 + tx;
      if (ci < it.cin && co < it.cout) it.w_kc[((size_t)tap * it.cout + co) * it.cin + ci] = (half_t)tile[tx][k];
    }
  }
}

// head weights f32 [cin][cout<=32] -> w_kc32 f16 [32][cin], w_ck32 f16 [cin][32] (zero padded)
__global__ void pack_small_kernel(const float* __restrict__ w, int cin, int cout,
                                  half_t* __restrict__ w_kc32, half_t* __restrict__ w_ck32) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cin * 32) return;
  const int ci = i >> 5, co = i & 31;
  const float v = co < cout ? w[ci * cout + co] : 0.f;
  w_ck32[i] = (half_t)v;
  w_kc32[(size_t)co * cin + ci] = (half_t)v;
}

__global__ void scale_kernel(float* __restrict__ x, long long n, float s) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    x[i] *= s;
}

__global__ void fill_kernel(float* __restrict__ x, long long n, float v) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    x[i] = v;
}

// scale * sum(x^2): slim.l2_regularizer(s)(w) = s * tf.nn.l2_loss(w) = s * sum(w^2) / 2 over the
// regularised variables (the REGULARIZATION_LOSSES term of `total_loss`, multigpu_train.py:36).
// Two launches, f64 partial per block and a fixed-order final sum: bitwise reproducible.
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void sumsq_partial_kernel(const float* __restrict__ x, long long n, double* __restrict__ partial) {
  __shared__ double sh[4];
  double acc = 0.0;
  const long long n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = x4[i];
    acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float v = x[(n4 << 2) + threadIdx.x];
    acc += (double)v * v;
  }
  const double t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void sumsq_final_kernel(const double* __restrict__ partial, int g, double scale, float* __restrict__ out) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < g; i += 256) acc += partial[i];
  const double t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) out[0] = (float)(scale * t);
}

// ---- dynamic loss scaling: the device-side state machine (ocr_loss_scale_state, include/ocr_hip.h) ----------------
__global__ void loss_scale_init_kernel(ocr_loss_scale_state* st, float init_scale) {
  if (threadIdx.x == 0) {
    st->scale = init_scale;
    st->inv_scale_used = 1.f / init_scale;
  } else if (threadIdx.x >= 2 && threadIdx.x < 8) {
    reinterpret_cast<uint32_t*>(st)[threadIdx.x] = 0u;           // skip .. reserved (words 0 and 1 are thread 0's)
  }
}

struct GradCheckP {
  float growth, backoff, min_scale, max_scale;
  unsigned interval;
  long long head, n4, tail;     // elements in front of the first 16-byte boundary, float4 groups, n & 3 leftovers
};

__device__ __forceinline__ unsigned nonfinite(float v) {          // exponent field all ones: inf or NaN
  return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
}

// The transition of the loss-scale state, run by the one thread behind the last ticket (and behind its fence):
// grad_check_kernel and the fused grad_clip_kernel<true> both end in it.  Returns `found`; st->inv_scale_used then holds
// 1 / (the scale the checked gradients were produced with).  The caller owns the ticket word it drew from.
__device__ __forceinline__ unsigned loss_scale_transition(ocr_loss_scale_state* __restrict__ st, const GradCheckP& p) {
  const unsigned found = __hip_atomic_load(&st->found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  float scale = st->scale;
  unsigned good = st->good_steps;
  __hip_atomic_store(&st->inv_scale_used, 1.f / scale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (found) {
    scale = fmaxf(scale * p.backoff, p.min_scale);
    good = 0;
    __hip_atomic_store(&st->skipped_total, st->skipped_total + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (++good == p.interval) {
    scale = fminf(scale * p.growth, p.max_scale);
    good = 0;
  }
  __hip_atomic_store(&st->skip, found ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->scale, scale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->good_steps, good, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->found, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return found;
}

// One HBM-bound read of the flat gradient buffer, shaped like sumsq_partial_kernel.  A workgroup that saw a
// non-finite element ORs `found` (one agent-scope atomic) and fences before it draws its ticket; clean workgroups
// have nothing to publish and only draw.  All ticket operations are read-modify-writes on one word, so the
// workgroup that draws the last one is ordered behind every release above and, after its own fence, reads the final
// `found`.  It alone touches the rest of the state, and it puts `found` and the ticket counter back to 0: the next
// launch on the stream starts clean with no memset in front of it (ocr_loss_scale_init zeroes them once).
__global__ __launch_bounds__(256) void grad_check_kernel(const float* __restrict__ x, GradCheckP p,
                                                         ocr_loss_scale_state* __restrict__ st) {
  unsigned bad = 0;
  const float4* x4 = reinterpret_cast<const float4*>(x + p.head);
#pragma unroll 4
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.n4; i += (long long)gridDim.x * 256) {
    const float4 v = x4[i];
    bad |= nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonfinite(v.w);
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x < p.head) bad |= nonfinite(x[threadIdx.x]);
    if (threadIdx.x < p.tail) bad |= nonfinite(x[p.head + (p.n4 << 2) + threadIdx.x]);
  }
  bad = __syncthreads_or((int)bad);
  if (threadIdx.x != 0) return;
  if (bad) {
    __hip_atomic_fetch_or(&st->found, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
  }
  const unsigned t = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t != gridDim.x - 1) return;
  __threadfence();
  loss_scale_transition(st, p);
  __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- global-norm gradient clipping: the device-side rule (ocr_grad_clip_state, include/ocr_hip.h) -------------------
__global__ void grad_clip_init_kernel(ocr_grad_clip_state* cs) {
  if (threadIdx.x < 8) reinterpret_cast<uint32_t*>(cs)[threadIdx.x] = 0u;
}

struct GradClipP {
  GradCheckP c;                 // head / n4 / tail; the loss-scale constants are read by the fused form only
  float clip_norm;
  float base;                   // static form: the optimiser's host factor; fused form: grad_scale (base = grad_scale * (1 / scale))
};

// sum over one element: the product the optimiser will use, in f32; its square and the sum in f64
__device__ __forceinline__ double clip_acc(double acc, float g, float base) {
  const double a = (double)(g * base);
  return fma(a, a, acc);
}

// grad_check_kernel's streaming pass with the squared norm of g * base summed beside it (FUSED: the non-finite test
// stays, for the loss-scale transition; the static form needs none: inf and NaN survive the sum).  Every workgroup
// stores its f64 partial write-through, releases, and draws a ticket from the CLIP state; the workgroup behind the
// last ticket acquires, sums the partials (thread t takes t, t + 256, ... in rising order, then the fixed
// block_sum_256 tree: the same bits on every call), and its thread 0 performs the transition(s).  FUSED reads
// ls->scale in every thread before its workgroup draws: the scale moves only behind the last ticket.
template <bool FUSED>
__global__ __launch_bounds__(256) void grad_clip_kernel(const float* __restrict__ x, GradClipP p,
                                                        ocr_grad_clip_state* __restrict__ cs,
                                                        ocr_loss_scale_state* ls, double* partial) {
  __shared__ double sh[4];
  __shared__ unsigned last;
  float base = p.base;
  if (FUSED) base = p.base * (1.f / __hip_atomic_load(&ls->scale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  unsigned bad = 0;
  double acc = 0.0;
  const float4* x4 = reinterpret_cast<const float4*>(x + p.c.head);
#pragma unroll 4
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.c.n4; i += (long long)gridDim.x * 256) {
    const float4 v = x4[i];
    if (FUSED) bad |= nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonfinite(v.w);
    acc = clip_acc(clip_acc(clip_acc(clip_acc(acc, v.x, base), v.y, base), v.z, base), v.w, base);
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x < p.c.head) {
      const float v = x[threadIdx.x];
      if (FUSED) bad |= nonfinite(v);
      acc = clip_acc(acc, v, base);
    }
    if (threadIdx.x < p.c.tail) {
      const float v = x[p.c.head + (p.c.n4 << 2) + threadIdx.x];
      if (FUSED) bad |= nonfinite(v);
      acc = clip_acc(acc, v, base);
    }
  }
  const double t = block_sum_256(acc, sh);
  if (FUSED) bad = __syncthreads_or((int)bad);
  if (threadIdx.x == 0) {
    __hip_atomic_store(&partial[blockIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (FUSED && bad) __hip_atomic_fetch_or(&ls->found, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned k = __hip_atomic_fetch_add(&cs->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned l = k == gridDim.x - 1;
    if (l) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    last = l;
  }
  __syncthreads();                    // (also: every thread is done with sh before the second sum writes it)
  if (!last) return;
  double s = 0.0;
  for (unsigned i = threadIdx.x; i < gridDim.x; i += 256)
    s += __hip_atomic_load(&partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s = block_sum_256(s, sh);
  if (threadIdx.x != 0) return;
  unsigned found = 0;
  if (FUSED) found = loss_scale_transition(ls, p.c);           // base above IS grad_scale * the inv_scale_used it stored
  const float norm = (float)sqrt(s);                           // root in f64; above f32's range the store is inf
  const unsigned skip = found | nonfinite(norm);
  float coef = 0.f, g_mul = 0.f;
  if (!skip) {
    coef = norm > p.clip_norm ? p.clip_norm / norm : 1.f;
    g_mul = base * coef;
  }
  __hip_atomic_store(&cs->norm, norm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&cs->coef, coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&cs->g_mul, g_mul, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&cs->skip, skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (skip)
    __hip_atomic_store(&cs->nonfinite_total, cs->nonfinite_total + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else if (coef < 1.f)
    __hip_atomic_store(&cs->clipped_total, cs->clipped_total + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&cs->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- gradient accumulation: K micro-batch gradients into one optimiser step (ocr_grad_accum_state, include/ocr_hip.h) --
__global__ void grad_accum_init_kernel(ocr_grad_accum_state* st, unsigned k) {
  if (threadIdx.x < 8) reinterpret_cast<uint32_t*>(st)[threadIdx.x] = threadIdx.x == 1 ? k : 0u;
}

__global__ void grad_accum_advance_kernel(ocr_grad_accum_state* st) {
  if (threadIdx.x != 0) return;
  unsigned m = st->micro + 1u;
  if (m >= st->k) {
    m = 0u;
    st->windows_total = st->windows_total + 1u;
  }
  st->micro = m;
}

// grad_check_kernel's streaming shape with a second buffer.  The rule is uniform over the launch: every thread reads
// micro and k (one scalar load each; the block is written by grad_accum_advance_kernel only, a launch of its own behind
// every accumulate call of the step) and the loop bodies differ in which buffer is read and which is written:
//   STORE  micro == 0      acc  = grad          (acc is not read: nothing to zero between windows)
//   ADD    0 < micro < k-1 acc  = acc + grad
//   CLOSE  micro == k-1    grad = acc + grad    (k == 1: grad = grad, nothing is launched into the loops at all)
// p.head / p.n4 / p.tail come from grad's address; acc has the same address modulo 16 (checked by the entry point).
template <int RULE>
__device__ __forceinline__ void grad_accum_body(float* __restrict__ grad, float* __restrict__ acc, const GradCheckP& p) {
  float4* g4 = reinterpret_cast<float4*>(grad + p.head);
  float4* a4 = reinterpret_cast<float4*>(acc + p.head);
#pragma unroll 4
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.n4; i += (long long)gridDim.x * 256) {
    const float4 g = g4[i];
    if (RULE == 0) {
      a4[i] = g;
    } else {
      const float4 a = a4[i];
      const float4 s = make_float4(a.x + g.x, a.y + g.y, a.z + g.z, a.w + g.w);
      if (RULE == 1) a4[i] = s; else g4[i] = s;
    }
  }
  if (blockIdx.x != 0) return;
  long long j = -1;
  if (threadIdx.x < p.head) j = threadIdx.x;
  else if (threadIdx.x >= 4 && threadIdx.x - 4 < p.tail) j = p.head + (p.n4 << 2) + (threadIdx.x - 4);
  if (j < 0) return;
  if (RULE == 0) acc[j] = grad[j];
  else if (RULE == 1) acc[j] = acc[j] + grad[j];
  else grad[j] = acc[j] + grad[j];
}

__global__ __launch_bounds__(256) void grad_accum_kernel(float* __restrict__ grad, float* __restrict__ acc, GradCheckP p,
                                                         const ocr_grad_accum_state* __restrict__ st) {
  const unsigned micro = st->micro, k = st->k;
  if (k <= 1u) return;
  if (micro + 1u >= k) grad_accum_body<2>(grad, acc, p);
  else if (micro == 0u) grad_accum_body<0>(grad, acc, p);
  else grad_accum_body<1>(grad, acc, p);
}

unsigned sumsq_grid(long long n) {
  long long b = (n / 4 + 255) / 256;
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return (unsigned)b;
}

unsigned ogrid(long long n) {
  long long b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// grad_clip_kernel: at most 2048 workgroups (8 resident per CU on 256 CUs): each publishes one partial behind one
// release, so fewer, longer-lived workgroups than grad_check_kernel's 4096
unsigned clip_grid(long long n4) {
  long long b = (n4 + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (unsigned)b;
}

GradCheckP split_head_tail(const void* grad, long long n, GradCheckP p) {
  p.head = (long long)(((16 - ((uintptr_t)grad & 15)) & 15) >> 2);       // 0..3 elements up to the 16-byte boundary
  if (p.head > n) p.head = n;
  p.n4 = (n - p.head) >> 2;
  p.tail = (n - p.head) & 3;
  return p;
}

}  // namespace

extern "C" int ocr_adam_step(void* w, const void* g, void* m, void* v, void* ema, int64_t n,
                             int64_t n_regularized, float lr_t, float beta1, float beta2, float eps,
                             float weight_decay, float inv_loss_scale, float ema_decay,
                             void* stream) {
  OCR_CHECK_ARG(w && g && m && v && n > 0 && n_regularized >= 0 && n_regularized <= n);
  AdamP a{lr_t, beta1, beta2, eps, weight_decay, inv_loss_scale, ema_decay, n, n_regularized};
  hipLaunchKernelGGL(adam_kernel<AdamP>, dim3(ogrid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     static_cast<float*>(w), static_cast<const float*>(g), static_cast<float*>(m),
                     static_cast<float*>(v), static_cast<float*>(ema));
  return ocr_launch_status();
}

extern "C" int ocr_momentum_step(void* w, const void* g, void* accum, void* ema, int64_t n,
                                 int64_t n_regularized, float lr, float momentum, float weight_decay,
                                 float inv_loss_scale, float ema_decay, void* stream) {
  OCR_CHECK_ARG(w && g && accum && n > 0 && n_regularized >= 0 && n_regularized <= n);
  MomP a{lr, momentum, weight_decay, inv_loss_scale, ema_decay, n, n_regularized};
  hipLaunchKernelGGL(momentum_kernel<MomP>, dim3(ogrid(n)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, static_cast<float*>(w),
                     static_cast<const float*>(g), static_cast<float*>(accum),
                     static_cast<float*>(ema));
  return ocr_launch_status();
}

extern "C" int ocr_pack_weights_f16(const void* w_hwio_f32, int taps, int cin, int cout, void* w_kc,
                                    void* w_ck, void* stream) {
  OCR_CHECK_ARG(w_hwio_f32 && (w_kc || w_ck) && taps > 0 && cin > 0 && cout > 0);
  hipLaunchKernelGGL(pack_weights_kernel, dim3(ocr_cdiv(cout, 32), ocr_cdiv(cin, 32), taps),
                     dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(w_hwio_f32), taps, cin, cout,
                     static_cast<half_t*>(w_kc), static_cast<half_t*>(w_ck));
  return ocr_launch_status();
}

extern "C" size_t ocr_pack_weights_batch_table_bytes(int n) { return (size_t)n * sizeof(PackItem) + (size_t)(n + 1) * sizeof(int); }

extern "C" int ocr_pack_weights_batch_table(int n, const void* const* w_hwio_f32, const int* taps, const int* cin,
                                            const int* cout, void* const* w_kc, void* const* w_ck, const int* ld_ck,
                                            void* table_host, int* grid_out) {
  OCR_CHECK_ARG(n > 0 && w_hwio_f32 && taps && cin && cout && w_kc && w_ck && table_host && grid_out);
  PackItem* items = static_cast<PackItem*>(table_host);
  int* first = reinterpret_cast<int*>(items + n);
  int g = 0;
  for (int i = 0; i < n; ++i) {
    OCR_CHECK_ARG(w_hwio_f32[i] && (w_kc[i] || w_ck[i]) && taps[i] > 0 && cin[i] > 0 && cout[i] > 0);
    items[i] = PackItem{static_cast<const float*>(w_hwio_f32[i]), static_cast<half_t*>(w_kc[i]),
                        static_cast<half_t*>(w_ck[i]), taps[i], cin[i], cout[i], ocr_cdiv(cin[i], 32), ocr_cdiv(cout[i], 32),
                        (ld_ck && ld_ck[i] > 0) ? ld_ck[i] : cout[i]};
    OCR_CHECK_ARG(items[i].ld_ck >= cout[i]);
    first[i] = g;
    g += taps[i] * items[i].tiles_ci * items[i].tiles_co;
  }
  first[n] = g;
  *grid_out = g;
  return OCR_OK;
}

extern "C" int ocr_pack_weights_batch_f16(const void* table_dev, int n, int grid, void* stream) {
  OCR_CHECK_ARG(table_dev && n > 0 && grid > 0);
  const PackItem* items = static_cast<const PackItem*>(table_dev);
  hipLaunchKernelGGL(pack_weights_batch_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                     items, reinterpret_cast<const int*>(items + n), n);
  return ocr_launch_status();
}

extern "C" int ocr_pack_weights_small_f16(const void* w_f32, int cin, int cout, void* w_kc32,
                                          void* w_ck32, void* stream) {
  OCR_CHECK_ARG(w_f32 && w_kc32 && w_ck32 && cin > 0 && cout > 0 && cout <= 32);
  hipLaunchKernelGGL(pack_small_kernel, dim3(ocr_cdiv(cin * 32, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const float*>(w_f32), cin, cout,
                     static_cast<half_t*>(w_kc32), static_cast<half_t*>(w_ck32));
  return ocr_launch_status();
}

extern "C" size_t ocr_sum_squares_workspace(int64_t n) { return (size_t)sumsq_grid(n) * sizeof(double); }

extern "C" int ocr_sum_squares_f32(const void* x, int64_t n, float scale, void* out_f32, void* workspace,
                                   size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(x && out_f32 && workspace && n > 0 && ((uintptr_t)x & 15) == 0);
  const unsigned g = sumsq_grid(n);
  if (ws_bytes < (size_t)g * sizeof(double)) return OCR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(g), dim3(256), 0, st, static_cast<const float*>(x),
                     (long long)n, static_cast<double*>(workspace));
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(workspace),
                     (int)g, (double)scale, static_cast<float*>(out_f32));
  return ocr_launch_status();
}

extern "C" int ocr_scale_f32(void* x, int64_t n, float s, void* stream) {
  OCR_CHECK_ARG(x && n > 0);
  hipLaunchKernelGGL(scale_kernel, dim3(ogrid(n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<float*>(x), (long long)n, s);
  return ocr_launch_status();
}

extern "C" int ocr_fill_f32(void* x, int64_t n, float value, void* stream) {
  OCR_CHECK_ARG(x && n > 0);
  hipLaunchKernelGGL(fill_kernel, dim3(ogrid(n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<float*>(x), (long long)n, value);
  return ocr_launch_status();
}

extern "C" int ocr_loss_scale_init(void* state, float init_scale, void* stream) {
  OCR_CHECK_ARG(state && ((uintptr_t)state & 3) == 0 && init_scale > 0.f && init_scale <= 3.4028234664e38f);
  hipLaunchKernelGGL(loss_scale_init_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<ocr_loss_scale_state*>(state), init_scale);
  return ocr_launch_status();
}

extern "C" int ocr_grad_check_f32(const void* grad, int64_t n, void* state, float growth_factor, float backoff_factor,
                                  int growth_interval, float min_scale, float max_scale, void* stream) {
  OCR_CHECK_ARG(grad && state && n > 0 && ((uintptr_t)grad & 3) == 0 && ((uintptr_t)state & 3) == 0);
  OCR_CHECK_ARG(growth_factor >= 1.f && backoff_factor > 0.f && backoff_factor <= 1.f && growth_interval > 0);
  OCR_CHECK_ARG(min_scale > 0.f && min_scale <= max_scale && max_scale <= 3.4028234664e38f);
  const GradCheckP p = split_head_tail(grad, n, GradCheckP{growth_factor, backoff_factor, min_scale, max_scale,
                                                           (unsigned)growth_interval, 0, 0, 0});
  hipLaunchKernelGGL(grad_check_kernel, dim3(ogrid(p.n4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(grad), p, static_cast<ocr_loss_scale_state*>(state));
  return ocr_launch_status();
}

extern "C" int ocr_adam_step_dyn(void* w, const void* g, void* m, void* v, void* ema, int64_t n,
                                 int64_t n_regularized, float lr_t, float beta1, float beta2, float eps,
                                 float weight_decay, float grad_scale, float ema_decay, const void* state,
                                 void* stream) {
  OCR_CHECK_ARG(w && g && m && v && state && n > 0 && n_regularized >= 0 && n_regularized <= n);
  AdamDynP a{{lr_t, beta1, beta2, eps, weight_decay, grad_scale, ema_decay, n, n_regularized},
             static_cast<const ocr_loss_scale_state*>(state)};
  hipLaunchKernelGGL(adam_kernel<AdamDynP>, dim3(ogrid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     static_cast<float*>(w), static_cast<const float*>(g), static_cast<float*>(m),
                     static_cast<float*>(v), static_cast<float*>(ema));
  return ocr_launch_status();
}

extern "C" int ocr_momentum_step_dyn(void* w, const void* g, void* accum, void* ema, int64_t n,
                                     int64_t n_regularized, float lr, float momentum, float weight_decay,
                                     float grad_scale, float ema_decay, const void* state, void* stream) {
  OCR_CHECK_ARG(w && g && accum && state && n > 0 && n_regularized >= 0 && n_regularized <= n);
  MomDynP a{{lr, momentum, weight_decay, grad_scale, ema_decay, n, n_regularized},
            static_cast<const ocr_loss_scale_state*>(state)};
  hipLaunchKernelGGL(momentum_kernel<MomDynP>, dim3(ogrid(n)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, static_cast<float*>(w),
                     static_cast<const float*>(g), static_cast<float*>(accum),
                     static_cast<float*>(ema));
  return ocr_launch_status();
}

// ---- global-norm gradient clipping -------------------------------------------------------------------------------
extern "C" int ocr_grad_clip_init(void* clip_state, void* stream) {
  OCR_CHECK_ARG(clip_state && ((uintptr_t)clip_state & 3) == 0);
  hipLaunchKernelGGL(grad_clip_init_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<ocr_grad_clip_state*>(clip_state));
  return ocr_launch_status();
}

// (the head in front of the 16-byte boundary only ever lowers the float4 count: n / 4 bounds the grid of any alignment)
extern "C" size_t ocr_grad_clip_workspace(int64_t n) { return (size_t)clip_grid(n > 0 ? n / 4 : 0) * sizeof(double); }

static int grad_clip_args(const void* grad, int64_t n, const void* clip_state, float clip_norm, const void* workspace,
                          size_t ws_bytes) {
  OCR_CHECK_ARG(grad && clip_state && workspace && n > 0);
  OCR_CHECK_ARG(((uintptr_t)grad & 3) == 0 && ((uintptr_t)clip_state & 3) == 0 && ((uintptr_t)workspace & 7) == 0);
  OCR_CHECK_ARG(clip_norm > 0.f && clip_norm <= 3.4028234664e38f);                  // (false for NaN)
  if (ws_bytes < ocr_grad_clip_workspace(n)) return OCR_ERR_WORKSPACE;
  return OCR_OK;
}

extern "C" int ocr_grad_clip_f32(const void* grad, int64_t n, void* clip_state, float clip_norm, float base,
                                 void* workspace, size_t ws_bytes, void* stream) {
  const int rc = grad_clip_args(grad, n, clip_state, clip_norm, workspace, ws_bytes);
  if (rc != OCR_OK) return rc;
  const GradClipP p{split_head_tail(grad, n, GradCheckP{}), clip_norm, base};
  hipLaunchKernelGGL(grad_clip_kernel<false>, dim3(clip_grid(p.c.n4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(grad), p, static_cast<ocr_grad_clip_state*>(clip_state),
                     static_cast<ocr_loss_scale_state*>(nullptr), static_cast<double*>(workspace));
  return ocr_launch_status();
}

extern "C" int ocr_grad_check_clip_f32(const void* grad, int64_t n, void* state, float growth_factor, float backoff_factor,
                                       int growth_interval, float min_scale, float max_scale, void* clip_state,
                                       float clip_norm, float grad_scale, void* workspace, size_t ws_bytes, void* stream) {
  OCR_CHECK_ARG(state && ((uintptr_t)state & 3) == 0 && state != clip_state);
  OCR_CHECK_ARG(growth_factor >= 1.f && backoff_factor > 0.f && backoff_factor <= 1.f && growth_interval > 0);
  OCR_CHECK_ARG(min_scale > 0.f && min_scale <= max_scale && max_scale <= 3.4028234664e38f);
  const int rc = grad_clip_args(grad, n, clip_state, clip_norm, workspace, ws_bytes);
  if (rc != OCR_OK) return rc;
  const GradClipP p{split_head_tail(grad, n, GradCheckP{growth_factor, backoff_factor, min_scale, max_scale,
                                                        (unsigned)growth_interval, 0, 0, 0}),
                    clip_norm, grad_scale};
  hipLaunchKernelGGL(grad_clip_kernel<true>, dim3(clip_grid(p.c.n4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(grad), p, static_cast<ocr_grad_clip_state*>(clip_state),
                     static_cast<ocr_loss_scale_state*>(state), static_cast<double*>(workspace));
  return ocr_launch_status();
}

extern "C" int ocr_adam_step_clip(void* w, const void* g, void* m, void* v, void* ema, int64_t n,
                                  int64_t n_regularized, float lr_t, float beta1, float beta2, float eps,
                                  float weight_decay, float ema_decay, const void* clip_state, void* stream) {
  OCR_CHECK_ARG(w && g && m && v && clip_state && n > 0 && n_regularized >= 0 && n_regularized <= n);
  AdamClipP a{{lr_t, beta1, beta2, eps, weight_decay, 0.f, ema_decay, n, n_regularized},
              static_cast<const ocr_grad_clip_state*>(clip_state)};
  hipLaunchKernelGGL(adam_kernel<AdamClipP>, dim3(ogrid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     static_cast<float*>(w), static_cast<const float*>(g), static_cast<float*>(m),
                     static_cast<float*>(v), static_cast<float*>(ema));
  return ocr_launch_status();
}

extern "C" int ocr_momentum_step_clip(void* w, const void* g, void* accum, void* ema, int64_t n,
                                      int64_t n_regularized, float lr, float momentum, float weight_decay,
                                      float ema_decay, const void* clip_state, void* stream) {
  OCR_CHECK_ARG(w && g && accum && clip_state && n > 0 && n_regularized >= 0 && n_regularized <= n);
  MomClipP a{{lr, momentum, weight_decay, 0.f, ema_decay, n, n_regularized},
             static_cast<const ocr_grad_clip_state*>(clip_state)};
  hipLaunchKernelGGL(momentum_kernel<MomClipP>, dim3(ogrid(n)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, static_cast<float*>(w),
                     static_cast<const float*>(g), static_cast<float*>(accum),
                     static_cast<float*>(ema));
  return ocr_launch_status();
}

// ---- gradient accumulation ---------------------------------------------------------------------------------------
extern "C" int ocr_grad_accum_init(void* state, int k, void* stream) {
  OCR_CHECK_ARG(state && ((uintptr_t)state & 3) == 0 && k >= 1);
  hipLaunchKernelGGL(grad_accum_init_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<ocr_grad_accum_state*>(state), (unsigned)k);
  return ocr_launch_status();
}

extern "C" int ocr_grad_accum_f32(void* grad, void* acc, int64_t n, const void* state, void* stream) {
  OCR_CHECK_ARG(grad && acc && state && n > 0 && grad != acc);
  OCR_CHECK_ARG(((uintptr_t)grad & 3) == 0 && ((uintptr_t)acc & 3) == 0 && ((uintptr_t)state & 3) == 0);
  OCR_CHECK_ARG((((uintptr_t)grad ^ (uintptr_t)acc) & 15) == 0);       // one head length serves both buffers
  const GradCheckP p = split_head_tail(grad, n, GradCheckP{});
  hipLaunchKernelGGL(grad_accum_kernel, dim3(clip_grid(p.n4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<float*>(grad), static_cast<float*>(acc), p,
                     static_cast<const ocr_grad_accum_state*>(state));
  return ocr_launch_status();
}

extern "C" int ocr_grad_accum_advance(void* state, void* stream) {
  OCR_CHECK_ARG(state && ((uintptr_t)state & 3) == 0);
  hipLaunchKernelGGL(grad_accum_advance_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<ocr_grad_accum_state*>(state));
  return ocr_launch_status();
}

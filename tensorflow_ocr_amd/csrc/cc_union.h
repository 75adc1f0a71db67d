// The lock-free union-find of the connected-component kernels, shared by decode.hip (ocr_link_cc, ocr_mask_cc) and
// decode_grid.hip (ocr_link_cc_grid): device helpers only, no kernel lives here.  A set's root is its smallest pixel
// index, so the partition and the numbering that follows do not depend on scheduling.
#ifndef OCR_CC_UNION_H_
#define OCR_CC_UNION_H_

#include "common.h"

// ---- union-find on pixel indices (roots = smallest index of the set) -----------------------
__device__ __forceinline__ int uf_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int* parent, int i) {
  for (;;) {
    const int p = uf_load(parent + i);
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
  for (int guard = 0; guard < (1 << 22); ++guard) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }       // attach the larger root under the smaller
    const int old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

struct CcP {
  int n, h, w, min_size;
  float tp, tl;
  int ls, lo;   // element stride / offset inside link_score (1,0: [8][n][h][w]; 2,1: [8][n][h][w][2])
};

// ---- the same union-find on a tile's 1024 LDS slots ------------------------------------------
__device__ __forceinline__ int lds_find(volatile int* lp, int i) {
  for (;;) {
    const int p = lp[i];
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void lds_unite(int* lp, int a, int b) {
  for (int guard = 0; guard < (1 << 20); ++guard) {
    a = lds_find(lp, a);
    b = lds_find(lp, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lp + a, b);
    if (old == a) return;
    a = old;
  }
}

#endif  // OCR_CC_UNION_H_

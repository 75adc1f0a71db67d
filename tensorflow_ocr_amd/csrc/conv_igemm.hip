// Implicit-GEMM NHWC convolution on gfx950 MFMA (f16 in, f32 accumulate, f16 out).
//
// Replaces slim.conv2d on the hot path (reference nets/vgg.py:14-39,
// nets/resnet_v1.py:97-105, nets/model_vgg_16.py:111-131) and, with the
// transposed/flipped weight pack, its input gradient.
//
// Work decomposition (one workgroup = 8 waves = 512 threads, 2 waves per SIMD):
//   * output tile  = TH rows x 32 columns of one image x BN couts; each wave owns 64 couts x 128
//     pixels wherever cout allows (256 couts x 8 rows, 128 couts x 16 rows);
//   * the input halo tile for one CK-wide channel chunk is staged ONCE in LDS ([HT][WT][CK] f16,
//     pixel stride padded so the 16-byte fragment reads are conflict-free) and re-read at shifted
//     addresses by all kh*kw taps: no im2col is ever materialised and each input byte crosses
//     L2->LDS once per cout tile; the next chunk's halo is prefetched into registers;
//   * per tap a [BN][CK] weight slice is streamed through a 2-deep LDS ring by LDS-DMA
//     (global_load_lds_dwordx4: the slice of tap t+1 lands under the MFMAs of tap t, no VGPRs);
//   * MFMA v_mfma_f32_16x16x32_f16 (multi-tap layers) or v_mfma_f32_32x32x16_f16 (1x1) with
//     A = weights (rows = cout) and B = activations (cols = pixels), so each lane ends up holding 4
//     consecutive couts of one pixel per register quad -> 8-byte packed LDS writes in the epilogue,
//     then 16-byte coalesced row stores to HBM;
//   * the epilogue optionally adds bias / ReLU, accumulates into an existing f16 tensor, and emits
//     per-tile per-cout sum and sum of squares of the stored (f16-rounded) values for training-mode
//     batch norm (or, in the input-gradient form, the producing layer's BN-backward sums).
#include "common.h"
#include "conv_epilogue.h"
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

namespace {

struct ConvP {
  int n, h, w, cin, oh, ow, cout, kh, kw, stride, dil, pt, pl, flip, flags;
  int tiles_x, tiles_y, n_tiles, HT, WT, halo_bytes;
  int xcd_swizzle;
  int pw;         // 1: pointwise GEMM kernel (conv_pw_kernel) on flat 256-pixel tiles
  long long npix; // n * oh * ow
  int m16;        // 1: v_mfma_f32_16x16x32_f16 tiles, 0: v_mfma_f32_32x32x16_f16
  BnRed br;       // br.y != nullptr: fused BN-backward reduction (see conv_epilogue.h)
  half_t* pool_out;          // conv_c64_persist_kernel<64, true>: [n][ceil(oh/2)][ceil(ow/2)][cout] pooled output
  unsigned char* pool_idx;   // ... and its first-max positions (ocr_maxpool_f16's argmax format), may be null
};


// LDS pixel / weight-row stride: CK f16 + padding that makes the 16-byte fragment reads
// conflict-free for the lane->(row, k-group) map of the MFMA shape in use.
OCR_DIAG_DECLARE(ocr_diag_conv)

constexpr int conv_pstr(int ck, bool m16) { return ck * 2 + (m16 ? 32 : 16); }

// Weight slices go global -> LDS by LDS-DMA (global_load_lds_dwordx4: no VGPR round trip, no
// ds_write).  The DMA image is lane-linear, so the rows are unpadded and the bank-conflict-free
// layout is an XOR swizzle of the 16-byte chunk index applied on the SOURCE address and again on
// the fragment read: chunk' = chunk ^ wswz(row).
constexpr int conv_wrs(int ck) { return ck * 2; }
__device__ __forceinline__ int wswz(int row, int ck, bool m16) {
  return ck == 64 ? ((row >> 1) & 7) : m16 ? (((row >> 3) & 1) << 1) : ((row >> 2) & 3);
}

template <int BN, int CK, int WCO, bool M16, int TH, int NW = 2>
__global__ __launch_bounds__(512) void conv_igemm_kernel(
    ConvP p, const half_t* __restrict__ x, const half_t* __restrict__ w,
    const float* __restrict__ bias, half_t* __restrict__ y,
    float* __restrict__ stats) {
  constexpr int NT = 512;
  constexpr int WPX = 8 / WCO;
  constexpr int TCO = BN / WCO / 32;
  constexpr int TPX = TH / WPX;   // tile rows (of 32 px) per wave
  static_assert(TH % WPX == 0 && (TPX <= 8) && (8 % TPX == 0), "a wave's rows lie in one 8-row epilogue pass");
  constexpr int PSTR = conv_pstr(CK, M16);
  constexpr int KSTEPS = CK / 16;
  constexpr int CPP = CK / 8;  // 16-byte chunks per pixel / per weight row
  constexpr int NWLD = (BN * CPP + NT - 1) / NT;
  constexpr int WRS = conv_wrs(CK);   // weight row stride in LDS (unpadded, swizzled)

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* halo = smem;
  char* wbuf = smem + p.halo_bytes;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;
  const int hh = lane >> 5;
  const int wco = wave % WCO;
  const int wpx = wave / WCO;

  // XCD-aware order: hardware deals consecutive workgroup ids round-robin to the 8 XCDs (private
  // L2 each); remap so that each XCD runs a CONTIGUOUS range of logical tiles -- the cout tiles of
  // one pixel tile and its spatial neighbours then share halo and weights through one L2
  int bid = blockIdx.x;
  if (p.xcd_swizzle) bid = (bid & 7) * (int)(gridDim.x >> 3) + (bid >> 3);
  const int nt = bid % p.n_tiles;
  int mt = bid / p.n_tiles;
  const int txi = mt % p.tiles_x;
  int tmp = mt / p.tiles_x;
  const int tyi = tmp % p.tiles_y;
  const int img = tmp / p.tiles_y;
  const int co0 = nt * BN;

  const int iy0 = tyi * TH * p.stride - p.pt;
  const int ix0 = txi * TILE_W * p.stride - p.pl;
  const int ntaps = p.kh * p.kw;
  const int nchunks = p.cin / CK;
  const int WT = p.WT;
  const int halo_px = p.HT * WT;

  // accumulators: 32x32 tiles (16 regs) or, with M16, 16x16 tiles (4 regs) of the same wave tile
  constexpr int AI = M16 ? TCO * 2 : TCO, AT = M16 ? TPX * 2 : TPX, AE = M16 ? 4 : 16;
  typename std::conditional<M16, f32x4, f32x16>::type acc[AI][AT];
#pragma unroll
  for (int i = 0; i < AI; ++i)
#pragma unroll
    for (int t = 0; t < AT; ++t)
#pragma unroll
      for (int e = 0; e < AE; ++e) acc[i][t][e] = 0.f;

  // per-lane LDS byte offsets
  // (32x32x16: lane -> row l&31, k-group l>>5;  16x16x32: row l&15, k-group l>>4; 8 k per group)
  const int frow = M16 ? (lane & 15) : r, fkg = M16 ? (lane >> 4) : hh;
  const int a_lane = (wco * TCO * 32 + frow) * WRS;                       // weights (row part)
  const int fx = wswz(frow, CK, M16);
  // byte offset of this lane's 8 k-values of k-step ks inside its weight row
  auto a_k = [&](int ks) { return (((M16 ? ks * 4 : ks * 2) + fkg) ^ fx) << 4; };
  const int b_lane = (frow * p.stride) * PSTR + fkg * 16;                 // activations
  const int b_half = 16 * p.stride * PSTR;                                // M16: second 16 px of a row
  const int b_row = p.stride * WT * PSTR;                                 // per tile row

  auto dma_w = [&](int tap, int cc, int buf) {
    const int tapw = p.flip ? (ntaps - 1 - tap) : tap;
    const half_t* src = w + ((size_t)tapw * p.cout + co0) * p.cin + cc * CK;
#pragma unroll
    for (int u = 0; u < NWLD; ++u) {
      const int idx = u * NT + tid;
      const int rr = idx / CPP, c = idx % CPP;
      if (idx < BN * CPP)     // whole waves: BN * CPP is a multiple of 64
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(src + (size_t)rr * p.cin + ((c ^ wswz(rr, CK, M16)) << 3)),
            (__attribute__((address_space(3))) void*)(wbuf + buf * (BN * WRS) + (u * NT + (tid & ~63)) * 16),
            16, 0, 0);
    }
  };
  // halo staging split into issue-early (global -> registers, right after the previous chunk's
  // halo has been handed to LDS) and write-late (registers -> LDS at the chunk boundary), so the
  // global latency of chunk cc+1 hides under the kh*kw taps of chunk cc.
  // (8-row tiles narrower than 128 couts keep their registers for occupancy)
  constexpr int NH = TH > 8 ? 10 : BN >= 128 ? (CK == 32 ? 7 : 6) : 1;
  const int halo_total = halo_px * CPP;
  const bool prefetch = NH > 1 && halo_total <= NH * NT && nchunks > 1;
  u32x4 hreg[NH];
  // BUFFER loads with the range check doing the zero padding (per-image descriptor, an offset beyond it reads as
  // zero): under `if (inside)` hipcc branches around every load and waits for each before the next
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<half_t*>(x) + (size_t)img * p.h * p.w * p.cin, 0, p.h * p.w * p.cin * 2, 0x00020000);
  auto halo_load = [&](int cc) {
#pragma unroll
    for (int u = 0; u < NH; ++u) {
      const int idx = u * NT + tid;
      const int hp = idx / CPP, c = idx % CPP;
      const int hy = hp / WT, hx = hp - hy * WT;
      const int iy = iy0 + hy, ix = ix0 + hx;
      const bool ok = (idx < halo_total) & ((unsigned)iy < (unsigned)p.h) & ((unsigned)ix < (unsigned)p.w);
      const unsigned off = ok ? (unsigned)(((iy * p.w + ix) * p.cin + cc * CK + c * 8) * 2) : 0x80000000u;
      hreg[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0));
    }
  };
  auto halo_store = [&]() {
#pragma unroll
    for (int u = 0; u < NH; ++u) {
      const int idx = u * NT + tid;
      if (idx < halo_total)
        *reinterpret_cast<u32x4*>(halo + (idx / CPP) * PSTR + (idx % CPP) * 16) = hreg[u];
    }
  };

  int wb = 0;
  OCR_DIAG_BEGIN()
  if (prefetch) halo_load(0);
  for (int cc = 0; cc < nchunks; ++cc) {
    __syncthreads();  // previous chunk's halo fully consumed
    // ---- stage the halo tile of this channel chunk ----
    if (prefetch) {
      halo_store();
    } else {
      const int total = halo_total;
      const half_t* xb = x + (size_t)img * p.h * p.w * p.cin + cc * CK;
      for (int base = 0; base < total; base += NT * 4) {
        u32x4 v[4];
        int off[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          int idx = base + u * NT + tid;
          v[u] = u32x4{0u, 0u, 0u, 0u};
          off[u] = -1;
          if (idx < total) {
            int hp = idx / CPP, c = idx % CPP;
            int hy = hp / WT, hx = hp - hy * WT;
            int iy = iy0 + hy, ix = ix0 + hx;
            off[u] = hp * PSTR + c * 16;
            if (iy >= 0 && iy < p.h && ix >= 0 && ix < p.w)
              v[u] = *reinterpret_cast<const u32x4*>(
                  xb + ((size_t)iy * p.w + ix) * p.cin + c * 8);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (off[u] >= 0) *reinterpret_cast<u32x4*>(halo + off[u]) = v[u];
      }
    }
    // NW weight slots: the slices of taps 0 .. NW-2 go out now, tap t+NW-1's at tap t (NW = 2: one tap ahead — 32 MFMAs
    // per wave on the 256 x 32 tiles, less than an L2 round trip: fc6's 144 tap steps per tile each waited for their
    // slice; NW = 4 requests it three taps ahead)
#pragma unroll
    for (int j = 0; j < NW - 1; ++j)
      if (j < ntaps) dma_w(j, cc, (wb + j) % NW);
    if (prefetch && cc + 1 < nchunks) halo_load(cc + 1);
    for (int tap = 0; tap < ntaps; ++tap) {
      // The weight slice of this tap came by LDS-DMA (dma_w, issued one tap ago; at tap 0 just above, with the NH
      // register loads of the next chunk's halo behind it): retire it EXPLICITLY.  hipcc does not count an LDS-DMA among
      // the accesses a workgroup barrier has to wait for — whether `s_waitcnt vmcnt(0)` appears in front of the barrier
      // depended on what else was outstanding (found in round 4: with one more field in ConvP this kernel's
      // <64,64,2,1,8> instantiation was scheduled differently and read a weight slice that had not landed).
      if constexpr (NW == 2) {
        if (tap == 0 && prefetch && cc + 1 < nchunks) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NH) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        // vector-memory operations issued AFTER this tap's slice (they retire in order): the slices of the taps up to
        // NW-2 ahead (NWLD requests per thread each: BN * CPP is a multiple of the workgroup here) and, for the first
        // NW-1 taps of a chunk, the next chunk's NH halo requests issued behind the initial slices
        int later = tap + NW - 2 < ntaps - 1 ? NW - 2 : ntaps - 1 - tap;
        const int nh = (tap <= NW - 2 && prefetch && cc + 1 < nchunks) ? NH : 0;
        switch (later * NWLD + nh) {
          case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
          case NWLD: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWLD) : "memory"); break;
          case 2 * NWLD: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NWLD) : "memory"); break;
          case NH: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NH) : "memory"); break;
          case NWLD + NH: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWLD + NH) : "memory"); break;
          case 2 * NWLD + NH: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NWLD + NH) : "memory"); break;
          default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
      }
      // after this barrier: buf[wb] (this tap, and at tap 0 the halo) is visible and
      // buf[wb^1] is free (its readers finished tap-1)
      __syncthreads();
      auto restage = [&]() {
        // lands under this tap's (and the next NW-2 taps') MFMAs; retired by the counted wait above
        if (tap + NW - 1 < ntaps) dma_w(tap + NW - 1, cc, (wb + NW - 1) % NW);
      };
      if constexpr (BN == 128 && !M16) restage();
      const int ky = tap / p.kw, kx = tap - ky * p.kw;
      const char* ab = wbuf + wb * (BN * WRS) + a_lane;
      const char* bb = halo + b_lane + ((ky * p.dil) * WT + kx * p.dil) * PSTR +
                       (wpx * TPX) * b_row;
      if constexpr (M16) {
        // pixel fragments in groups of <= 4 so that at most 8 fragments are live beside the accumulators
        constexpr int TG = TH > 8 ? 2 : AT > 4 ? 4 : AT;
#pragma unroll
        for (int ks = 0; ks < CK / 32; ++ks) {
          half8_t a[AI];
#pragma unroll
          for (int i = 0; i < AI; ++i)
            a[i] = *reinterpret_cast<const half8_t*>(ab + i * 16 * WRS + a_k(ks));
#pragma unroll
          for (int t0 = 0; t0 < AT; t0 += TG) {
            half8_t b[TG];
#pragma unroll
            for (int t = 0; t < TG; ++t)
              b[t] = *reinterpret_cast<const half8_t*>(bb + ((t0 + t) >> 1) * b_row + ((t0 + t) & 1) * b_half +
                                                       ks * 64);
            if (ks == 0 && t0 == 0) {
              __builtin_amdgcn_sched_barrier(0);
              restage();
              __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < AI; ++i)
#pragma unroll
              for (int t = 0; t < TG; ++t)
                acc[i][t0 + t] = OCR_MFMA_16x16x32(a[i], b[t], acc[i][t0 + t], 0, 0, 0);
            if constexpr (BN == 256) __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else if constexpr (BN == 128) {
      // software-pipelined k-steps: the LDS reads of step ks+1 are issued before the MFMAs of
      // step ks (two named fragment sets; sched_barrier keeps hipcc from sinking the reads)
      half8_t a0[TCO], b0[TPX], a1[TCO], b1[TPX];
#pragma unroll
      for (int i = 0; i < TCO; ++i) a0[i] = *reinterpret_cast<const half8_t*>(ab + i * 32 * WRS + a_k(0));
#pragma unroll
      for (int t = 0; t < TPX; ++t) b0[t] = *reinterpret_cast<const half8_t*>(bb + t * b_row);
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ks += 2) {
        if (ks + 1 < KSTEPS) {
#pragma unroll
          for (int i = 0; i < TCO; ++i)
            a1[i] = *reinterpret_cast<const half8_t*>(ab + i * 32 * WRS + a_k(ks + 1));
#pragma unroll
          for (int t = 0; t < TPX; ++t)
            b1[t] = *reinterpret_cast<const half8_t*>(bb + t * b_row + (ks + 1) * 32);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TCO; ++i)
#pragma unroll
          for (int t = 0; t < TPX; ++t)
            acc[i][t] = OCR_MFMA_32x32x16(a0[i], b0[t], acc[i][t], 0, 0, 0);
        if (ks + 1 < KSTEPS) {
          if (ks + 2 < KSTEPS) {
#pragma unroll
            for (int i = 0; i < TCO; ++i)
              a0[i] = *reinterpret_cast<const half8_t*>(ab + i * 32 * WRS + a_k(ks + 2));
#pragma unroll
            for (int t = 0; t < TPX; ++t)
              b0[t] = *reinterpret_cast<const half8_t*>(bb + t * b_row + (ks + 2) * 32);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < TCO; ++i)
#pragma unroll
            for (int t = 0; t < TPX; ++t)
              acc[i][t] = OCR_MFMA_32x32x16(a1[i], b1[t], acc[i][t], 0, 0, 0);
        }
      }
      } else if constexpr (!M16) {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          half8_t a[TCO], b[TPX];
#pragma unroll
          for (int i = 0; i < TCO; ++i)
            a[i] = *reinterpret_cast<const half8_t*>(ab + i * 32 * WRS + a_k(ks));
#pragma unroll
          for (int t = 0; t < TPX; ++t)
            b[t] = *reinterpret_cast<const half8_t*>(bb + t * b_row + ks * 32);
          if (ks == 0) {
            // the next tap's weight slice goes to the other LDS buffer while the first
            // fragments are in flight (not between the barrier and the first reads)
            __builtin_amdgcn_sched_barrier(0);
            restage();
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int i = 0; i < TCO; ++i)
#pragma unroll
            for (int t = 0; t < TPX; ++t)
              acc[i][t] = OCR_MFMA_32x32x16(a[i], b[t], acc[i][t], 0, 0, 0);
        }
      }
      wb = NW == 2 ? (wb ^ 1) : (wb + 1) % NW;
    }
  }

  OCR_DIAG_END(ocr_diag_conv)
  // ---- epilogue: accumulators -> LDS [256 px][<=128 couts] f16 -> coalesced rows, in passes of
  // 8 tile rows x <=128 couts (the waves owning that slice are the active ones) ----
  constexpr int EP = TH / 8;          // 8-row passes
  constexpr int EBN = BN > 128 ? 128 : BN;
  constexpr int EWCO = BN > 128 ? 2 : WCO;
  const int tiles_y8 = (p.oh + TILE_H - 1) / TILE_H;
#pragma unroll
  for (int q = 0; q < EP; ++q) {
    const int ty8 = tyi * EP + q;                       // this pass as an 8-row tile index
    if (ty8 >= tiles_y8) break;
    const int mt8 = (img * tiles_y8 + ty8) * p.tiles_x + txi;
    const bool rows_here = (wpx * TPX) / 8 == q;
    const int wpx8 = ((wpx * TPX) % 8) / TPX;           // wave's position inside the pass
#pragma unroll
    for (int h = 0; h < BN / EBN; ++h) {
      __syncthreads();
      const bool active = rows_here && (BN <= 128 || (wco >> 1) == h);
      if constexpr (M16)
        conv_epilogue16<EBN, TCO, TPX, EWCO, NT>(acc, smem, p.flags, bias, y, stats, img, ty8, txi, mt8,
                                                 co0 + h * EBN, p.oh, p.ow, p.cout, BN > 128 ? (wco & 1) : wco,
                                                 wpx8, active, p.br.y ? &p.br : nullptr);
      else
        conv_epilogue<EBN, TCO, TPX, EWCO, NT>(acc, smem, p.flags, bias, y, stats, img, ty8, txi, mt8,
                                               co0 + h * EBN, p.oh, p.ow, p.cout, BN > 128 ? (wco & 1) : wco,
                                               wpx8, active, p.br.y ? &p.br : nullptr);
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Pointwise (1x1, stride 1) convolutions as a plain GEMM:  y[px][co] = sum_ci x[px][ci] * w[co][ci].
// (ResNet bottleneck / shortcut / feature-merge convs, fc7, and their input gradients.)
// The tap-sweeping kernel above degenerates here to one tap per 64-channel chunk: two barriers, a
// halo hand-off and an exposed weight fetch per 32 MFMAs.  This kernel is the canonical
// double-buffered GEMM instead: tile = 256 consecutive pixels of the flattened [N*H*W] index x BN
// couts, K in 64-channel stages; BOTH operands are K-contiguous in HBM, staged by LDS-DMA into
// unpadded 128-byte rows with the chunk index XOR-swizzled on the source address (weights:
// (row>>1)&7, pixels: px&7 -- conflict-free for the 16x16x32 fragment reads), stage s+1 landing
// under the 64 MFMAs per wave of stage s; one barrier per stage.  Pixels past the end read a zero
// page.  Same epilogue (and batch-norm statistics per 256-pixel tile) as the kernel above.
__device__ const u32x4 ocr_conv_zero_page[4] = {};

template <int BN, int WCO, bool EPI_LOADS>
__global__ __launch_bounds__(512) void conv_pw_kernel(
    ConvP p, const half_t* __restrict__ x, const half_t* __restrict__ w,
    const float* __restrict__ bias, half_t* __restrict__ y, float* __restrict__ stats) {
  constexpr int NT = 512;
  constexpr int WPX = 8 / WCO;
  constexpr int TCO = BN / WCO / 32;
  constexpr int TPX = 8 / WPX;
  constexpr int AI = TCO * 2, AT = TPX * 2;
  constexpr int RS = 128;                       // bytes per staged row (64 channels)
  constexpr int ABYTES = BN * RS, BBYTES = 256 * RS, STAGE = ABYTES + BBYTES;
  constexpr int NA = BN * 8 / NT, NB = 256 * 8 / NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wco = wave % WCO, wpx = wave / WCO;
  const int frow = lane & 15, fkg = lane >> 4;

  int bid = blockIdx.x;
  // XCD-aware order (see conv_igemm_kernel): the cout tiles of one pixel tile run on ONE XCD, whose L2 then serves the
  // pixel rows to all of them — dealt round-robin, every XCD fetched every pixel tile (PMC: 256 -> 1024 launches read
  // 1.9x their operand bytes)
  if (p.xcd_swizzle) bid = (bid & 7) * (int)(gridDim.x >> 3) + (bid >> 3);
  const int nt = bid % p.n_tiles;
  const int mt = bid / p.n_tiles;
  const int co0 = nt * BN;
  const long long px0 = (long long)mt * 256;
  const int nk = p.cin / 64;

  f32x4 acc[AI][AT];
#pragma unroll
  for (int i = 0; i < AI; ++i)
#pragma unroll
    for (int t = 0; t < AT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][t][e] = 0.f;

  const int a_lane = (wco * TCO * 32 + frow) * RS;
  const int b_lane = (wpx * TPX * 32 + frow) * RS;
  const int fxa = (frow >> 1) & 7, fxb = frow & 7;

  const __attribute__((address_space(1))) void* zero =
      (const __attribute__((address_space(1))) void*)(&ocr_conv_zero_page[0]);
  auto dma_stage = [&](int kc, int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + ABYTES;
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      const int idx = u * NT + tid;
      const int rr = idx >> 3, c = idx & 7;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(w + (size_t)(co0 + rr) * p.cin + kc * 64 +
                                                          ((c ^ ((rr >> 1) & 7)) << 3)),
          (__attribute__((address_space(3))) void*)(As + (u * NT + (tid & ~63)) * 16), 16, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int idx = u * NT + tid;
      const int pr = idx >> 3, c = idx & 7;
      const long long gp = px0 + pr;
      const __attribute__((address_space(1))) void* src =
          gp < p.npix ? (const __attribute__((address_space(1))) void*)(x + (size_t)gp * p.cin + kc * 64 +
                                                                        ((c ^ (pr & 7)) << 3))
                      : zero;
      __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(Bs + (u * NT + (tid & ~63)) * 16),
                                       16, 0, 0);
    }
  };

  dma_stage(0, 0);
  int buf = 0;
  for (int kc = 0; kc < nk; ++kc) {
    // after this barrier: stage kc has landed (the explicit vmcnt(0): hipcc does not count an LDS-DMA among the accesses
    // a workgroup barrier waits for — see conv_igemm_kernel), and stage kc-1's readers are done, so the other buffer
    // may be overwritten
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kc + 1 < nk) dma_stage(kc + 1, buf ^ 1);
    const char* ab = smem + buf * STAGE + a_lane;
    const char* bb = smem + buf * STAGE + ABYTES + b_lane;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      half8_t a[AI];
#pragma unroll
      for (int i = 0; i < AI; ++i)
        a[i] = *reinterpret_cast<const half8_t*>(ab + i * 16 * RS + (((ks * 4 + fkg) ^ fxa) << 4));
      constexpr int TG = AT > 4 ? 4 : AT;
#pragma unroll
      for (int t0 = 0; t0 < AT; t0 += TG) {
        half8_t b[TG];
#pragma unroll
        for (int t = 0; t < TG; ++t)
          b[t] = *reinterpret_cast<const half8_t*>(bb + (t0 + t) * 16 * RS + (((ks * 4 + fkg) ^ fxb) << 4));
#pragma unroll
        for (int i = 0; i < AI; ++i)
#pragma unroll
          for (int t = 0; t < TG; ++t)
            acc[i][t0 + t] = OCR_MFMA_16x16x32(a[i], b[t], acc[i][t0 + t], 0, 0, 0);
      }
    }
    buf ^= 1;
  }

  // epilogue on the flat tile: "row" r of the 8x32 layout = pixels px0 + 32r .. +31
  // The store-only epilogue takes a 256-cout tile in two 128-cout halves (the staging tile and its reduction
  // scratch share the LDS with nothing else then).  The epilogue WITH global operands stages all 256 couts at once:
  // in halves the second half's 64 accumulator registers stay live under the first half's operand batch and the
  // kernel spilled 120 registers — scratch reloads wait on the same counter as the operand loads and serialise
  // them (ResNet's 64 -> 256 input-gradient convolutions ran at 1.8-3 TB/s).
  constexpr int EBN = EPI_LOADS ? BN : (BN > 128 ? 128 : BN);
  constexpr int EWCO = EBN < BN ? 2 : WCO;
  const int rows = (int)(p.npix / 32);
#pragma unroll
  for (int h = 0; h < BN / EBN; ++h) {
    __syncthreads();
    const bool active = EBN == BN || (wco >> 1) == h;
    conv_epilogue16<EBN, TCO, TPX, EWCO, NT, EPI_LOADS>(acc, smem, p.flags, bias, y, stats, 0, mt, 0, mt, co0 + h * EBN,
                                             rows, 32, p.cout, EBN < BN ? (wco & 1) : wco, wpx, active,
                                             p.br.y ? &p.br : nullptr);
  }
}

// ---------------------------------------------------------------------------------------------
// conv_pw_kernel with the PIXEL OPERAND TRANSFORMED WHILE IT IS STAGED (ResNet bottlenecks, training).
// The element-wise passes around a 1x1 convolution read and write the widest tensors of a unit only to hand
// them to that convolution; here the convolution's own loader applies them and WRITES the transformed operand
// back once (other consumers still need it), so one full read of that tensor disappears per pass:
//   MODE 1 (forward):  v = relu(half(s0*f0 + f2) + r),  r = f1 ? half(s1*f1 + f3) : s1
//                      = the unit output relu(bn(conv3) + shortcut) of the PREVIOUS unit (nets/resnet_v1.py:107;
//                      f1/f3: the projection shortcut's own batch norm), consumed as conv1 / shortcut input;
//                      `out` receives v, `bits` its ReLU mask (one byte per 8 channels)
//   MODE 2 (backward): v = half(f0*s0 + f1*s1 + f2) = the batch-norm backward apply dy = A*dz + B*y + C
//                      (ocr_bn_bwd_coefficients), consumed as the input-gradient GEMM's operand; `out` receives dy
//                      for the weight gradient that follows.  PROJ here = the batch norm is followed by a ReLU: s0 is
//                      the ACTIVATION's gradient and dz = s0 * [s1*f0 + f3 > 0] (f0 = A is the BN's scale, f3 its
//                      shift: the mask of the stored 16-bit activation, as conv_stem_wgrad_kernel evaluates it).
//   MODE 3 (forward):  v = half(max(s0*f0 + f2, 0)) = relu(bn(conv2)) — bn_relu_kernel's expression — consumed as conv3's
//                      input (nets/resnet_v1.py:99-105); `out` receives the activation for the weight gradient.
// Weights still arrive by LDS-DMA; the pixel rows go global -> registers (requested under the previous stage's
// MFMAs) -> transform -> ds_write into the same swizzled slots the DMA form fills, so the MFMA loop and the
// epilogues are conv_pw_kernel's.  The VALU work (60-75 operations per 16-byte chunk) equals what the separate
// pass spent and stays under the kernel's HBM time (memory-bound launches: MFMA pipe ~0.2 busy).  Only the first
// cout tile writes `out` / `bits`.
struct PwX {
  const half_t *s0, *s1;
  const float *f0, *f1, *f2, *f3;
  half_t* out;
  unsigned char* bits;
};

// LDS-only barrier: the waves' own ds_writes are complete, nothing is said about vector memory.  __syncthreads()
// waits vmcnt(0) — in this kernel that would be the operand loads of the NEXT stage and the side-write stores of
// this one, i.e. one full HBM round trip per K stage (measured: 7.9 us per stage with it).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int BN, int WCO, bool EPI_LOADS, int MODE, bool PROJ>
__global__ __launch_bounds__(512) void conv_pwx_kernel(
    ConvP p, PwX t, const half_t* __restrict__ w, half_t* __restrict__ y, float* __restrict__ stats) {
  constexpr int NT = 512;
  constexpr int WPX = 8 / WCO;
  constexpr int TCO = BN / WCO / 32;
  constexpr int TPX = 8 / WPX;
  constexpr int AI = TCO * 2, AT = TPX * 2;
  constexpr int RS = 128;
  constexpr int ABYTES = BN * RS, BBYTES = 256 * RS, STAGE = ABYTES + BBYTES;
  constexpr int NA = BN * 8 / NT, NB = 256 * 8 / NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* coef = reinterpret_cast<float*>(smem + 2 * STAGE);     // [4][cin]: f0, f1, f2, f3 (absent arrays: zeros)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wco = wave % WCO, wpx = wave / WCO;
  const int frow = lane & 15, fkg = lane >> 4;

  int bid = blockIdx.x;
  if (p.xcd_swizzle) bid = (bid & 7) * (int)(gridDim.x >> 3) + (bid >> 3);      // see conv_pw_kernel
  const int nt = bid % p.n_tiles;
  const int mt = bid / p.n_tiles;
  const int co0 = nt * BN;
  const long long px0 = (long long)mt * 256;
  const int nk = p.cin / 64;
  const bool writer = nt == 0;
  constexpr bool proj = MODE == 1 && PROJ;
  constexpr bool relu2 = MODE == 2 && PROJ;

  f32x4 acc[AI][AT];
#pragma unroll
  for (int i = 0; i < AI; ++i)
#pragma unroll
    for (int tt = 0; tt < AT; ++tt)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][tt][e] = 0.f;

  const int a_lane = (wco * TCO * 32 + frow) * RS;
  const int b_lane = (wpx * TPX * 32 + frow) * RS;
  const int fxa = (frow >> 1) & 7, fxb = frow & 7;

  // this thread's slot in a staged row: position (tid & 7) of row (tid >> 3) + 64 u; the slot holds logical
  // 16-byte chunk position ^ swizzle(row) — weights (row >> 1) & 7, pixels row & 7 (the layout conv_pw_kernel's
  // LDS-DMA produces, so the fragment reads below are its own)
  const int prl = tid >> 3;
  const int cs = (tid & 7) ^ (prl & 7);
  const int csa = (tid & 7) ^ ((prl >> 1) & 7);         // weight rows prl + 64 u: ((prl + 64 u) >> 1) & 7 == (prl >> 1) & 7
  half8_t ra[NA], r0[NB], r1[NB];
  // everything travels through registers: no vmcnt is waited at a barrier
  auto request = [&](int kc) {
#pragma unroll
    for (int u = 0; u < NA; ++u)
      ra[u] = *reinterpret_cast<const half8_t*>(w + (size_t)(co0 + prl + 64 * u) * p.cin + kc * 64 + csa * 8);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const long long gp = px0 + prl + 64 * u;
      if (gp < p.npix) {
        const size_t off = (size_t)gp * p.cin + kc * 64 + cs * 8;
        r0[u] = *reinterpret_cast<const half8_t*>(t.s0 + off);
        if (MODE != 3) r1[u] = *reinterpret_cast<const half8_t*>(t.s1 + off);
      }
    }
  };
  auto stash = [&](int kc, int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + ABYTES;
#pragma unroll
    for (int u = 0; u < NA; ++u) *reinterpret_cast<half8_t*>(As + (u * NT + tid) * 16) = ra[u];
    const int ch = kc * 64 + cs * 8;
    float c0[8], c1[8], c2[8], c3[8];
    *reinterpret_cast<f32x4*>(c0) = *reinterpret_cast<const f32x4*>(coef + ch);
    *reinterpret_cast<f32x4*>(c0 + 4) = *reinterpret_cast<const f32x4*>(coef + ch + 4);
    *reinterpret_cast<f32x4*>(c2) = *reinterpret_cast<const f32x4*>(coef + 2 * p.cin + ch);
    *reinterpret_cast<f32x4*>(c2 + 4) = *reinterpret_cast<const f32x4*>(coef + 2 * p.cin + ch + 4);
    if (MODE == 2) {
      *reinterpret_cast<f32x4*>(c1) = *reinterpret_cast<const f32x4*>(coef + p.cin + ch);
      *reinterpret_cast<f32x4*>(c1 + 4) = *reinterpret_cast<const f32x4*>(coef + p.cin + ch + 4);
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const long long gp = px0 + prl + 64 * u;
      half8_t v;
      if (gp < p.npix) {
        unsigned m = 0;
        if (proj || relu2) {
          // the fourth coefficient row is re-read from LDS per row group (the index passes through an opaque register, so
          // the read is not hoisted): held across the loop next to the other three it pushed this instantiation over the
          // 256-register file, and the spill's reload sat inside the K loop, on the counter the operand loads wait on
          int c3i = 3 * p.cin + ch;
          asm volatile("" : "+v"(c3i));
          *reinterpret_cast<f32x4*>(c3) = *reinterpret_cast<const f32x4*>(coef + c3i);
          *reinterpret_cast<f32x4*>(c3 + 4) = *reinterpret_cast<const f32x4*>(coef + c3i + 4);
          if (proj) {                                     // (the 256-cout projection form: the second row as well)
            *reinterpret_cast<f32x4*>(c1) = *reinterpret_cast<const f32x4*>(coef + c3i - 2 * p.cin);
            *reinterpret_cast<f32x4*>(c1 + 4) = *reinterpret_cast<const f32x4*>(coef + c3i - 2 * p.cin + 4);
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (MODE == 1) {                    // bn_add_relu_kernel's expression, operation for operation
            const float z = (float)(half_t)__builtin_fmaf((float)r0[u][e], c0[e], c2[e]);
            float rv = (float)r1[u][e];
            if (proj) rv = (float)(half_t)__builtin_fmaf(rv, c1[e], c3[e]);
            const float f = z + rv;
            v[e] = (half_t)(f > 0.f ? f : 0.f);
            m |= (f > 0.f && (float)v[e] > 0.f ? 1u : 0u) << e;
          } else if (MODE == 3) {
            const float f = __builtin_fmaf((float)r0[u][e], c0[e], c2[e]);
            v[e] = (half_t)(f > 0.f ? f : 0.f);
          } else if (relu2) {
            const float yf = (float)r1[u][e];
            const float dzf = __builtin_fmaf(yf, c0[e], c3[e]) > OCR_RELU_TIE ? (float)r0[u][e] : 0.f;
            v[e] = (half_t)__builtin_fmaf(c0[e], dzf, __builtin_fmaf(c1[e], yf, c2[e]));
          } else {
            v[e] = (half_t)__builtin_fmaf(c0[e], (float)r0[u][e], __builtin_fmaf(c1[e], (float)r1[u][e], c2[e]));
          }
        }
        if (writer) {
          const size_t off = (size_t)gp * p.cin + ch;
          *reinterpret_cast<half8_t*>(t.out + off) = v;
          if (MODE == 1 && t.bits != nullptr) t.bits[off >> 3] = (unsigned char)m;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (half_t)0.f;
      }
      *reinterpret_cast<half8_t*>(Bs + (u * NT + tid) * 16) = v;
    }
  };

  request(0);
  for (int i = tid; i < 4 * p.cin; i += NT) {
    const int arr = i / p.cin, chn = i - arr * p.cin;
    const float* src = arr == 0 ? t.f0 : arr == 1 ? t.f1 : arr == 2 ? t.f2 : t.f3;
    coef[i] = src != nullptr ? src[chn] : 0.f;
  }
  lds_barrier();
  stash(0, 0);
  if (nk > 1) request(1);
  int buf = 0;
  for (int kc = 0; kc < nk; ++kc) {
    // after this barrier stage kc is complete in `buf` (every wave's ds_writes precede its arrival) and the readers
    // of the other buffer (stage kc-1's MFMAs) are done.  The operands of stage kc+1 were requested one iteration
    // ago and are turned into LDS rows now; stage kc+2 is requested behind them, under this stage's MFMAs.
    lds_barrier();
    if (kc + 1 < nk) {
      stash(kc + 1, buf ^ 1);
      if (kc + 2 < nk) request(kc + 2);
    }
    const char* ab = smem + buf * STAGE + a_lane;
    const char* bb = smem + buf * STAGE + ABYTES + b_lane;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      half8_t a[AI];
#pragma unroll
      for (int i = 0; i < AI; ++i)
        a[i] = *reinterpret_cast<const half8_t*>(ab + i * 16 * RS + (((ks * 4 + fkg) ^ fxa) << 4));
      constexpr int TG = AT > 4 ? 4 : AT;
#pragma unroll
      for (int t0 = 0; t0 < AT; t0 += TG) {
        half8_t b[TG];
#pragma unroll
        for (int tt = 0; tt < TG; ++tt)
          b[tt] = *reinterpret_cast<const half8_t*>(bb + (t0 + tt) * 16 * RS + (((ks * 4 + fkg) ^ fxb) << 4));
#pragma unroll
        for (int i = 0; i < AI; ++i)
#pragma unroll
          for (int tt = 0; tt < TG; ++tt)
            acc[i][t0 + tt] = OCR_MFMA_16x16x32(a[i], b[tt], acc[i][t0 + tt], 0, 0, 0);
      }
    }
    buf ^= 1;
  }

  constexpr int EBN = EPI_LOADS ? BN : (BN > 128 ? 128 : BN);
  constexpr int EWCO = EBN < BN ? 2 : WCO;
  const int rows = (int)(p.npix / 32);
#pragma unroll
  for (int h = 0; h < BN / EBN; ++h) {
    __syncthreads();
    const bool active = EBN == BN || (wco >> 1) == h;
    // MODE 2: the descriptor is passed as it stands (all-null = no BN operands: every use is guarded by a flag or a field
    // test).  With `p.br.y ? &p.br : nullptr` hipcc kept a null-descriptor path beside every operand load of the epilogue
    // and, unable to count the outstanding loads across the two paths, put `s_waitcnt vmcnt(0)` at each merge: the
    // batch's loads went out one at a time, each behind the previous one's round trip.
    const BnRed* brp = MODE == 2 ? &p.br : (p.br.y ? &p.br : nullptr);
    conv_epilogue16<EBN, TCO, TPX, EWCO, NT, EPI_LOADS>(acc, smem, p.flags, nullptr, y, stats, 0, mt, 0, mt, co0 + h * EBN,
                                             rows, 32, p.cout, EBN < BN ? (wco & 1) : wco, wpx, active, brp);
  }
}

// ---------------------------------------------------------------------------------------------
// 3x3 / stride 1 / dilation 1 layers with cin % 64 == 0: FOUR waves per workgroup, ONE per SIMD, each
// with the whole 512-entry register file (wave tile 128 couts x 128 pixels = 256 accumulator registers,
// fragments of the next k-step double-buffered in the remaining VGPRs).
//
// Why: PMC + in-kernel clock stamps on the 8-wave kernel above (profiles/r02_clock_diag.json,
// r02_pmc_mfma.json): its main loop keeps the matrix pipe busy 63 % of its cycles (47 % of the launch)
// with the two waves of a SIMD running the same read -> wait -> MFMA program in lockstep behind one
// barrier per tap, and it issues 0.375 ds_read_b128 per MFMA.  Here
//   * a "step" = one tap x 32 input channels = 64 MFMAs (16x16x32) per wave; the 8 weight + 8 pixel
//     fragments of step s+1 are read WHILE the MFMAs of step s issue (0.25 ds_read_b128 per MFMA),
//     every LDS address is a per-lane base register + an immediate (taps fully unrolled): no address
//     arithmetic in the loop;
//   * BOTH operands arrive by LDS-DMA (global_load_lds_dwordx4): the halo tile of a 64-channel chunk
//     ([10][34] pixels x 128 B, chunk index XOR (pixel & 7): conflict-free for every tap shift) is
//     double-buffered and fetched under the previous chunk's 18 steps; the [256][32] weight slice of
//     a step goes through a 4-deep ring, fetched 3 steps ahead; waits are COUNTED (s_waitcnt vmcnt(N),
//     never 0 in the loop) and the one barrier per step is a raw s_barrier placed where the wave
//     already holds the fragments of the step it is about to issue, so a barrier costs its skew only;
//   * out-of-image halo pixels read a zero page; the tail issues clamped (redundant) DMAs so that the
//     vmcnt arithmetic is the same in every step.
// Same tile geometry (8 x 32 pixels x 256 couts), weight pack, epilogue and batch-norm partials as
// conv_igemm_kernel<256,64,4,true,8>: a drop-in for that instantiation.
// Cache policy of the output stores of the wave-private epilogues (measurement switch, -DOCR_CONV_NT_STORE=mask: 1 = the
// persistent 64-channel kernel, 2 = conv3x3_w4s, 4 = conv3x3_w4): a conv output is written once; non-temporal stores keep it
// from evicting the halo rows and weight slices the neighbouring workgroups are about to read.
#ifndef OCR_CONV_NT_STORE
#define OCR_CONV_NT_STORE 7          // A/B in one gpurun call, ms per step: 0 -> 18.67 / 18.67, 1 -> 18.59 / 18.67, 3 -> 18.59 / 18.62, 7 -> 18.53 / 18.57
#endif
#define OCR_EPI_STORE(bit, ptr, val)                                                   \
  do {                                                                                 \
    if constexpr ((OCR_CONV_NT_STORE & (bit)) != 0) __builtin_nontemporal_store(val, ptr); \
    else *(ptr) = (val);                                                               \
  } while (0)
template <int N> struct IC { static constexpr int value = N; };
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(IC<I>{});
    static_for<I + 1, N>(f);
  }
}

// dev ablations (never in a shipped library): 1 = no weight DMA in the loop, 2 = no halo DMA in the loop,
// 4 = no barrier, 8 = no fragment reads, 16 = no vmcnt wait
#ifndef W4_ABL
#define W4_ABL 0
#endif
constexpr int W4_HT = 10, W4_WT = 34;
constexpr int W4_HSLOTS = ((W4_HT * W4_WT * 8 + 255) / 256) * 256;   // 16-byte slots per halo buffer (2816)
constexpr int W4_HBYTES = W4_HSLOTS * 16;                            // 45056
constexpr int W4_NH = W4_HSLOTS / 256;                               // halo DMA rounds per chunk (11)
constexpr int W4_WSTEP = 256 * 64;                                   // bytes of one step's weight slice
constexpr int W4_RING = 4, W4_AHEAD = 3;
constexpr int W4_LDS = 2 * W4_HBYTES + W4_RING * W4_WSTEP;           // 155648

// EPI: the epilogue's mode as a COMPILE-TIME constant.  With the flags read at run time every round carried the
// machinery of all modes (the ACCUM add computed and selected away, the ReLU and mask compares, the BN-backward operand's
// conversions behind uniform branches): 32.9 k of a tile's 126-205 k cycles were epilogue (in-kernel stamps,
// libocr_hip_diag.so) — 16 rounds x 2 k cycles on a single wave per SIMD, where every issued instruction is serial time.
//   0 generic (run-time flags: ACCUM and anything else)   1 STATS (forward, BN nets)        2 STATS + fused BN-backward sums
//   3 BIAS + RELU (forward, bias nets)                     4 as 2, storing dz (store_dz)    5 plain store
// [z > thr] as 1.f / 0.f WITHOUT a compare and a select: v_cmp writes a lane mask to an SGPR pair, the v_cndmask that
// reads it needs wait states behind it (296 s_nop in the fused-sum epilogue of conv3x3_w4_kernel) and neither packs.
// clamp((z - thr) * 2^60) is exact for the f16 build: z and thr = 2^-25 are f32, so z > thr means z - thr >= 2^-48 and the
// product is >= 2^12 (clamped to 1), z <= thr gives <= 0 (clamped to 0); thr = -inf (no ReLU) gives +inf -> 1.  The bf16
// build's threshold (2^-134) sits among the f32 subnormals, where no scale separates the two sides: it keeps the compare.
__device__ __forceinline__ float epi_step(float z, float thr, float nthr_h) {
#ifdef OCR_BF16
  (void)nthr_h;
  return z > thr ? 1.f : 0.f;
#else
  (void)thr;
  return __builtin_amdgcn_fmed3f(__builtin_fmaf(z, 0x1p60f, nthr_h), 0.f, 1.f);
#endif
}
// four f32 -> four 16-bit values by TWO packed converts (round to nearest even: v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32).
// Element by element hipcc built a quad from two scalar converts, one packed convert, a pack and an alignbit: five
// instructions where two do, on the one wave a SIMD holds in these epilogues (every issued instruction is serial time).
__device__ __forceinline__ half4_t epi_pack4(float a, float b, float c, float d) {
  const half2_t lo = __builtin_convertvector(f32x2{a, b}, half2_t);
  const half2_t hi = __builtin_convertvector(f32x2{c, d}, half2_t);
  return half4_t{lo[0], lo[1], hi[0], hi[1]};
}
template <int EPI>
__global__ __launch_bounds__(256) void conv3x3_w4_kernel(
    ConvP p, const half_t* __restrict__ x, const half_t* __restrict__ w,
    const float* __restrict__ bias, half_t* __restrict__ y, float* __restrict__ stats) {
  constexpr int BN = 256, TH = 8, WT = W4_WT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wbuf = smem + 2 * W4_HBYTES;
  OCR_DIAG_WG_BEGIN()

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wco = wave & 1, wpx = wave >> 1;        // cout half (128), pixel half (4 rows)
  const int L = lane & 15, kg = lane >> 4;

  int bid = blockIdx.x;
  if (p.xcd_swizzle) bid = (bid & 7) * (int)(gridDim.x >> 3) + (bid >> 3);
  const int nt = bid % p.n_tiles;
  int mt = bid / p.n_tiles;
  const int txi = mt % p.tiles_x;
  const int tmp = mt / p.tiles_x;
  const int tyi = tmp % p.tiles_y;
  const int img = tmp / p.tiles_y;
  const int co0 = nt * BN;
  const int iy0 = tyi * TH - p.pt, ix0 = txi * TILE_W - p.pl;
  const int nchunks = p.cin / 64;

  // ---- per-lane DMA sources -------------------------------------------------------------------
  // LDS-DMA by BUFFER loads (buffer_load_dwordx4 ... lds): the per-lane part of every address is a constant
  // 32-bit offset, the part that changes from DMA to DMA (channel chunk, tap, cout quarter) is scalar, so
  // a DMA costs no vector instruction; a halo slot outside the image carries an offset beyond the
  // descriptor's range and the range check writes zeros into its LDS slot (no zero page, no select).
  // With one wave per SIMD every instruction between two MFMAs costs issue cycles (see the main loop).
  constexpr unsigned OOB = 0x80000000u;              // + any scalar offset of a < 2 GiB tensor: still out of range
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<half_t*>(x) + (size_t)img * p.h * p.w * p.cin, 0, p.h * p.w * p.cin * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<half_t*>(w), 0, 9 * p.cout * p.cin * 2, 0x00020000);
  unsigned hvo[W4_NH];                               // byte offset of this lane's halo slot in the image
#pragma unroll
  for (int u = 0; u < W4_NH; ++u) {
    const int idx = u * 256 + tid;
    const int hp = idx >> 3, sl = idx & 7;
    const int hy = hp / WT, hx = hp - hy * WT;
    const int iy = iy0 + hy, ix = ix0 + hx;
    hvo[u] = (hp < W4_HT * WT && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w)
                 ? (unsigned)(((iy * p.w + ix) * p.cin + ((sl ^ (hp & 7)) << 3)) * 2)
                 : OOB;
  }
  // weights: slot idx = u*256 + tid -> row u*64 + (tid>>2), stored chunk tid&3 holds logical chunk c ^ swz
  const int wrow = tid >> 2;
  const unsigned wvo = (unsigned)((wrow * p.cin + (((tid & 3) ^ (((wrow >> 3) & 1) << 1)) << 3)) * 2);

  auto dma_halo = [&](int cc, int hb, int u) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        xrs, (__attribute__((address_space(3))) void*)(smem + hb * W4_HBYTES + (u * 256 + wave * 64) * 16), 16,
        hvo[u], cc * 128, 0, 0);
  };
  // quarter u (64 couts) of the [256 couts][32 channels] slice of (chunk cc, tap, k-half ks) -> ring slot
  auto dma_wq = [&](int cc, int tap, int ks, int ring, int u) {
    const int tapw = p.flip ? (8 - tap) : tap;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        wrs, (__attribute__((address_space(3))) void*)(wbuf + ring * W4_WSTEP + (u * 256 + wave * 64) * 16), 16,
        wvo, (((tapw * p.cout + co0 + u * 64) * p.cin) + cc * 64 + ks * 32) * 2, 0, 0);
  };
  auto dma_w = [&](int cc, int tap, int ks, int ring) {
#pragma unroll
    for (int u = 0; u < 4; ++u) dma_wq(cc, tap, ks, ring, u);
  };

  // ---- per-lane LDS read bases ------------------------------------------------------------------
  // pixel fragment of tile t at tap (ky,kx): halo pixel hp = (wpx*4 + (t>>1) + ky)*34 + (t&1)*16 + kx + L,
  // 16-byte chunk (ks*4 + kg) ^ (hp & 7); hp & 7 = (L + u) & 7 with u = (2*((t>>1)+ky) + kx) & 7 STATIC
  // (wpx*4*34 and 16 are multiples of 8): 16 per-lane bases (2 k-halves x 8 values of u), the rest is
  // an immediate offset.
  unsigned tb[2][8];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int u = 0; u < 8; ++u)
      tb[ks][u] = (unsigned)((wpx * 4 * WT + L) * 128 + (((ks * 4 + kg) ^ ((L + u) & 7)) << 4));
  // weight fragment of cout tile i: row wco*128 + i*16 + L of the step's slice, chunk kg ^ swz(row)
  const unsigned a_lane = (unsigned)(2 * W4_HBYTES + (wco * 128 + L) * 64 + ((kg ^ (((L >> 3) & 1) << 1)) << 4));

  f32x4 acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  half8_t fa[2][8], fb[2][8];

  OCR_DIAG_BEGIN()
  // ---- prologue: halo of chunk 0, weight slices of steps 0..2 -----------------------------------
#pragma unroll
  for (int u = 0; u < W4_NH; ++u) dma_halo(0, 0, u);
  dma_w(0, 0, 0, 0);
  dma_w(0, 0, 1, 1);
  dma_w(0, 1, 0, 2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  {
    // fragments of step 0 (tap 0, ks 0) into set 0
#pragma unroll
    for (int i = 0; i < 8; ++i) fa[0][i] = *reinterpret_cast<const half8_t*>(smem + (a_lane + i * 1024));
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int u = (2 * (t >> 1)) & 7;
      fb[0][t] = *reinterpret_cast<const half8_t*>(smem + (tb[0][u] + ((t >> 1) * WT + (t & 1) * 16) * 128));
    }
  }

  int hsel = 0;                                   // halo buffer of the chunk being computed
  for (int cc = 0; cc < nchunks; ++cc) {
    const int s0 = cc * 18;                       // global step index of this chunk's step 0
    const int ccn = cc + 1 < nchunks ? cc + 1 : cc;   // clamped: the tail re-fetches (harmless)
    static_for<0, 18>([&](auto J) {
      constexpr int j = decltype(J)::value;
      constexpr int P = j & 1, Q = P ^ 1;
      // next step (whose fragments are read during this one)
      constexpr int jn = (j + 1) % 18;
      constexpr int tapn = jn >> 1, ksn = jn & 1, kyn = tapn / 3, kxn = tapn % 3;
      // step whose weight slice is fetched during this one
      constexpr int jd = (j + W4_AHEAD) % 18;
      constexpr bool dnext = j + W4_AHEAD >= 18;
      // weights of step s+1 landed (own share): everything older than the 4 DMAs of step s+2 and the
      // halo DMA issued in step s-1
      constexpr int jp = (j + 17) % 18;
      constexpr int nh_prev = (jp >= 1 && jp <= W4_NH) ? 1 : 0;
      if constexpr (!(W4_ABL & 16)) {
        if constexpr (nh_prev) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      }
      if constexpr (!(W4_ABL & 4)) __builtin_amdgcn_s_barrier();
      // DMA: halo piece of the next chunk (steps 1..11), then the weight slice of step s+3
      const int sd_ring = (s0 + j + W4_AHEAD) & (W4_RING - 1);
      const int d_cc = dnext ? ccn : cc;
      auto dma_w1 = [&](int u) {
        if constexpr (W4_ABL & 1) return;
        dma_wq(d_cc, jd >> 1, jd & 1, sd_ring, u);
      };
      if constexpr (j == 17) {
        hsel ^= 1;                                // the prefetched fragments belong to the next chunk
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int u = 0; u < 8; ++u) tb[ks][u] = hsel ? tb[ks][u] + W4_HBYTES : tb[ks][u] - W4_HBYTES;
      }
      const unsigned abase = a_lane + (unsigned)(((s0 + j + 1) & (W4_RING - 1)) * W4_WSTEP);
      // 64 MFMAs of this step from set P.  Everything else is handed out ONE OPERATION PER MFMA GAP: with one
      // wave per SIMD an instruction between two MFMAs is free only when it is (nearly) alone there — clustered
      // behind every 8th MFMA the same reads and DMAs cost 5.7 cycles per instruction (18 % of the loop).
      // Odd gaps 1..31: the 16 fragment reads of the next step into set Q (pixel fragments first: all eight are
      // needed by the next step's first group); gap 32: the halo DMA; gaps 36..48: the four weight DMAs.
      auto read_b = [&](int t) {
        if constexpr (W4_ABL & 8) return;
        const int u = (2 * ((t >> 1) + kyn) + kxn) & 7;
        fb[Q][t] = *reinterpret_cast<const half8_t*>(smem + (tb[ksn][u] + (((t >> 1) + kyn) * WT + (t & 1) * 16 + kxn) * 128));
      };
      auto read_a = [&](int i) {
        if constexpr (W4_ABL & 8) return;
        fa[Q][i] = *reinterpret_cast<const half8_t*>(smem + (abase + i * 1024));
      };
#pragma unroll
      for (int g = 0; g < 8; ++g) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if (j == 17 && g == 7 && t == 7) mfma16_acc_drain(acc[g][t], fa[P][g], fb[P][t]);   // see common.h
          else mfma16_acc(acc[g][t], fa[P][g], fb[P][t]);
          const int m = g * 8 + t;
          if (m & 1) {
            if (m < 16) read_b(m >> 1);
            else if (m < 32) read_a((m >> 1) - 8);
          } else if (m == 32) {
            if constexpr (j >= 1 && j <= W4_NH && !(W4_ABL & 2)) dma_halo(ccn, hsel ^ 1, j - 1);
          } else if (m >= 36 && m <= 48 && (m & 3) == 0) {
            dma_w1((m - 36) >> 2);
          }
        }
      }
    });
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");   // the tail's redundant DMAs must not land in the epilogue's LDS
  OCR_DIAG_END(ocr_diag_conv)

  // ---- epilogue, WAVE-PRIVATE: a wave owns 128 couts of 128 pixels, i.e. whole 256-byte pieces of 128
  // output rows.  16 rounds of (16 pixels x 64 couts): accumulator quads -> this wave's 2 KB staging rows
  // (16-byte chunk index XOR (pixel & 7)) -> 128-byte coalesced row pieces, batch-norm partials (of the
  // STORED 16-bit values; with `br` the producing layer's BN-backward sums) accumulated per lane over the
  // rounds and folded over the wave at the end.  No block barrier after the first one, no shared
  // staging: the block-staged epilogue of the 8-wave kernel cost this kernel 16 % of its run time
  // (4 waves doing two block-wide passes).  The per-wave partials are summed through LDS at the end.
  __syncthreads();                                   // every wave's DMAs have landed: the LDS is free
  {
    const int mt8 = (img * p.tiles_y + tyi) * p.tiles_x + txi;
    char* const stage = smem + wave * 2048;
    const bool has_bias = EPI == 0 ? (p.flags & OCR_CONV_BIAS) != 0 : EPI == 3;
    const bool relu = EPI == 0 ? (p.flags & OCR_CONV_RELU) != 0 : EPI == 3;
    const bool accum = EPI == 0 ? (p.flags & OCR_CONV_ACCUM_F16) != 0 : false;
    const bool do_stats = EPI == 0 ? (p.flags & OCR_CONV_STATS) != 0 : (EPI == 1 || EPI == 2 || EPI == 4);
    const bool has_br = EPI == 0 ? p.br.y != nullptr : (EPI == 2 || EPI == 4);      // (fields read by value: a pointer to p.br would pin the kernel arguments in scratch)
    const int g4 = lane >> 4;                        // accumulator layout: pixel L, couts 4*g4..+3 of a 16x16 tile
    const int c8 = lane & 7, pg = lane >> 3;         // read-back layout: 16-byte chunk of a pixel's 64 couts, pixel
    const int cow = co0 + wco * 128;
    // the tile's 256 bias values through LDS (PixelLink's VGG has biases, no BN): a round would fetch 16 of them
    float* const lbias = reinterpret_cast<float*>(smem + 4 * 2048 + 4096);
    if (has_bias) {
      lbias[tid] = bias[co0 + tid];
      __syncthreads();
    }
    float s[2][8], q2[2][8];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[hf][e] = 0.f; q2[hf][e] = 0.f; }
    // this lane's 2 x 8 couts are fixed over the rounds: the producing layer's BN parameters once, up front
    // (scale / shift decide the ReLU mask per element; mean / invstd enter linearly and are applied to the
    // sums at the end: sum dz*xhat = invstd * (sum dz*y - mean * sum dz))
    float bsc[2][8], bsh[2][8];
    const float relu_thr = p.br.relu ? OCR_RELU_TIE : -INFINITY;   // no ReLU: every element passes
    const float nthr_h = -relu_thr * 0x1p60f;                      // (epi_step)
    const bool sdz = EPI == 0 ? (has_br && p.br.store_dz != 0) : EPI == 4;
    if (has_br) {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int cc = cow + hf * 64 + c8 * 8 + e;
          bsc[hf][e] = p.br.scale[cc]; bsh[hf][e] = p.br.shift[cc];
        }
    }
    // Round it = 2*t + hf (16 rounds).  The BN-backward operand `p.br.y` of the WHOLE tile (128 KB: the main loop's
    // LDS is free now) is fetched by LDS-DMA up front, 32 one-KB transfers per wave all in flight at once, each lane
    // fetching the 16 bytes it will read back itself (slot = lane: no swizzle needed).  Fetched round by round into
    // registers (four rounds ahead, all the registers allowed) the loads shared the vmcnt queue with the rounds'
    // stores, so every round waited for a store's acknowledgement: the fused reduction cost conv3's input gradients
    // +155 us on 465 (per-layer table, profiles/r03_w4_per_layer.json) — more than a separate pass over both tensors.
    half8_t oq[2];
    // element offset of (round, k): a per-lane base computed once + a wave-uniform delta; bounds as "rows / columns
    // left" (the epilogue is bound by instruction issue: a dozen 64-bit address and compare instructions per
    // store were a tenth of it)
    const size_t pbase = (((size_t)img * p.oh + tyi * TH + wpx * 4) * p.ow + txi * TILE_W + pg) * p.cout + cow + c8 * 8;
    const int rows_left = p.oh - (tyi * TH + wpx * 4), cols_left = p.ow - (txi * TILE_W + pg);
    auto round_off = [&](int it, int k, bool& ok) __attribute__((always_inline)) {
      const int t = it >> 1, hf = it & 1;
      ok = ((t >> 1) < rows_left) & ((t & 1) * 16 + k * 8 < cols_left);
      return pbase + (size_t)(((t >> 1) * p.ow + (t & 1) * 16 + k * 8) * p.cout + hf * 64);
    };
    char* const ylds = smem + 16384 + wave * 32768;   // past the staging rows, the partial sums and the bias values
    if (has_br) {
      const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<half_t*>(p.br.y) + (size_t)img * p.oh * p.ow * p.cout, 0, p.oh * p.ow * p.cout * 2, 0x00020000);
      const unsigned ybase = (unsigned)((((tyi * TH + wpx * 4) * p.ow + txi * TILE_W + pg) * p.cout + cow + c8 * 8) * 2);
#pragma unroll
      for (int it = 0; it < 16; ++it)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int t = it >> 1, hf = it & 1;
          const bool ok = ((t >> 1) < rows_left) & ((t & 1) * 16 + k * 8 < cols_left);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(
              yrs, (__attribute__((address_space(3))) void*)(ylds + (it * 2 + k) * 1024), 16, ok ? ybase : 0x80000000u,
              (((t >> 1) * p.ow + (t & 1) * 16 + k * 8) * p.cout + hf * 64) * 2, 0, 0);
        }
    }
    // Software-pipelined over the 16 rounds (round 5): the rounds were a serial chain on the one wave a SIMD holds — stage,
    // read back (an LDS round trip), then ~60 instructions of sums and stores that wait for it: ~880 cycles a round, 14 k
    // per tile and the same on a single workgroup as on a full chip (scripts/epilogue_probe.py), i.e. latency, not
    // bandwidth.  Now round r's read-back is issued FIRST, round r+1 is converted and staged into the second staging
    // buffer while it is in flight, and only then is round r consumed.
    char* const stage2 = smem + 147456 + wave * 2048;    // behind the operand tile: W4_LDS leaves 8 KB there
    auto stage_round = [&](auto IT) __attribute__((always_inline)) {
      constexpr int it = decltype(IT)::value;
      constexpr int t = it >> 1, hf = it & 1;
      char* const st = (it & 1) ? stage2 : stage;
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int i = hf * 4 + ii;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (has_bias) bv = *reinterpret_cast<const f32x4*>(lbias + (wco * 128 + i * 16 + g4 * 4));   // one LDS read, not four loads
        float vq4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = acc[i][t][e];
          if (has_bias) v += bv[e];        // (an unconditional "+ 0.f" is not folded away: -0.f + 0.f = +0.f)
          if (relu) v = v > 0.f ? v : 0.f;
          vq4[e] = v;
        }
        const half4_t o = epi_pack4(vq4[0], vq4[1], vq4[2], vq4[3]);
        *reinterpret_cast<half4_t*>(st + L * 128 + (((ii * 2 + (g4 >> 1)) ^ (L & 7)) << 4) + (g4 & 1) * 8) = o;
      }
    };
    stage_round(IC<0>{});
    if (has_br) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the operand tile has landed (behind round 0's staging)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    static_for<0, 16>([&](auto IT) {
      constexpr int it = decltype(IT)::value;
      constexpr int hf = it & 1;
      const char* const st = (it & 1) ? stage2 : stage;
      if (accum) {                                  // old gradient of this round
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          bool ok;
          const size_t off = round_off(it, k, ok);
          if (ok) oq[k] = *reinterpret_cast<const half8_t*>(y + off);
        }
      }
      half8_t vv[2], yv2[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int px = k * 8 + pg;
        vv[k] = *reinterpret_cast<const half8_t*>(st + px * 128 + ((c8 ^ (px & 7)) << 4));
        if (has_br) yv2[k] = *reinterpret_cast<const half8_t*>(ylds + (it * 2 + k) * 1024 + lane * 16);
      }
      if constexpr (it + 1 < 16) stage_round(IC<it + 1>{});      // into the OTHER buffer, while the reads above are in flight
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        bool ok;
        const size_t off = round_off(it, k, ok);
        if (ok) {
          half8_t v = vv[k];
          const half8_t yv = yv2[k];
          if (accum) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] + (float)oq[k][e]);
          }
          if (sdz) {                                // store the gradient PAST the ReLU (BnRed::store_dz)
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (!((float)yv[e] * bsc[hf][e] + bsh[hf][e] > relu_thr)) v[e] = (half_t)0.f;
          }
          OCR_EPI_STORE(4, reinterpret_cast<half8_t*>(y + off), v);
          if (do_stats) {
            if (has_br) {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float yf = (float)yv[e];
                const float dz = epi_step(yf * bsc[hf][e] + bsh[hf][e], relu_thr, nthr_h) * (float)v[e];   // mask of the stored activation
                s[hf][e] += dz;
                q2[hf][e] += dz * yf;
              }
            } else {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float f = (float)v[e];
                s[hf][e] += f;
                q2[hf][e] += f * f;
              }
            }
          }
        }
      }
    });
    if (do_stats) {
      if (has_br) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int cc = cow + hf * 64 + c8 * 8 + e;
            q2[hf][e] = (q2[hf][e] - p.br.mean[cc] * s[hf][e]) * p.br.invstd[cc];
          }
      }
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma unroll
          for (int o = 8; o < 64; o <<= 1) {         // the 8 pixel lanes of a chunk, fixed order
            s[hf][e] += __shfl_xor(s[hf][e], o, 64);
            q2[hf][e] += __shfl_xor(q2[hf][e], o, 64);
          }
        }
      // the two pixel halves of a cout range meet in LDS (fixed order: deterministic), one partial row per tile
      float* const red = reinterpret_cast<float*>(smem + 4 * 2048);     // [2 pixel halves][2][256]
      if (pg == 0) {
        float* row = red + wpx * 512 + wco * 128 + c8 * 8;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            row[hf * 64 + e] = s[hf][e];
            row[256 + hf * 64 + e] = q2[hf][e];
          }
      }
      __syncthreads();
      for (int i = tid; i < 512; i += 256)
        stats[((size_t)mt8 * 2 + (i >> 8)) * p.cout + co0 + (i & 255)] = red[i] + red[512 + i];
    }
  }
  OCR_DIAG_WG_END(ocr_diag_conv)
}

// ---------------------------------------------------------------------------------------------
// The same design for the 64- and 128-cout 3x3 layers (conv1_2, conv2_x and the input gradients that end in
// 64 / 128 channels): large maps, little arithmetic per output byte — conv1_2 moves 2.1 GB for 0.62 TFLOP, so
// its floor is the HBM stream (0.43 ms), not MFMA.  What these layers need is the output stores and halo
// fetches of one workgroup running UNDER the MFMAs of another, so here a workgroup is small enough for TWO
// per CU (4 waves x 256 registers, <= 80 KB of LDS):
//   * tile 8 x 32 pixels x BN couts (BN = 64 or 128), wave w owns tile rows 2w, 2w+1 (64 pixels) x all couts;
//   * 32-channel halo chunks ([10][34] pixels x 64 B, chunk index XOR ((p & 3) ^ ((p >> 1) & 3)): conflict-free
//     for every tap shift), double-buffered, one step = one tap (K = 32) = BN/16 x 4 MFMAs per wave; the
//     loop body is a PAIR of chunks (18 steps, fragment-set parity and halo buffer static);
//   * weight slices [BN][32] through the same 4-deep LDS-DMA ring, counted vmcnt, one raw barrier per step;
//   * the same wave-private epilogue (per-wave batch-norm partials summed through LDS at the end).
constexpr int W4S_HSLOTS = ((W4_HT * W4_WT * 4 + 255) / 256) * 256;   // 16-byte slots per halo buffer (1536)
constexpr int W4S_HBYTES = W4S_HSLOTS * 16;                          // 24576
constexpr int W4S_NH = W4S_HSLOTS / 256;                             // halo DMA rounds per chunk (6)
__device__ __forceinline__ int w4s_swz(int hp) { return (hp & 3) ^ ((hp >> 1) & 3); }
// weight ring depth: a step is only BN/16 x 4 MFMAs (256 cycles for BN = 64), an LDS-DMA takes 500+ cycles under
// load to land: the 4 KB slices of the 64-cout variant are fetched 6 steps ahead (8 slots), the 8 KB slices
// of the 128-cout variant 3 ahead (4 slots); both rings are 32 KB -> 80 KB with the two halo buffers
constexpr int w4s_ring(int bn) { return bn == 64 ? 8 : 4; }
constexpr int w4s_ahead(int bn) { return bn == 64 ? 6 : 3; }
constexpr int w4s_lds(int bn) { return 2 * W4S_HBYTES + w4s_ring(bn) * bn * 64; }

template <int BN, int EPI>                       // EPI: the epilogue mode at compile time (see conv3x3_w4_kernel)
__global__ __launch_bounds__(256, 2) void conv3x3_w4s_kernel(
    ConvP p, const half_t* __restrict__ x, const half_t* __restrict__ w,
    const float* __restrict__ bias, half_t* __restrict__ y, float* __restrict__ stats) {
  constexpr int TH = 8, WT = W4_WT, AI = BN / 16, AT = 4, NW = BN / 64, WSTEP = BN * 64;
  constexpr int RING = w4s_ring(BN), AHEAD = w4s_ahead(BN);
  // halo pieces of the next chunk: two per step in the chunk's first three steps (6 pieces), so that the last
  // one has five steps to land before the fragments of the next chunk's first step are read (step 8)
  constexpr int HPS = 2, HSTEPS = W4S_NH / HPS;
  OCR_DIAG_WG_BEGIN()
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wbuf = smem + 2 * W4S_HBYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // = pixel quarter: tile rows 2w, 2w+1
  const int L = lane & 15, kg = lane >> 4;

  int bid = blockIdx.x;
  if (p.xcd_swizzle) bid = (bid & 7) * (int)(gridDim.x >> 3) + (bid >> 3);
  const int nt = bid % p.n_tiles;
  int mt = bid / p.n_tiles;
  const int txi = mt % p.tiles_x;
  const int tmp = mt / p.tiles_x;
  const int tyi = tmp % p.tiles_y;
  const int img = tmp / p.tiles_y;
  const int co0 = nt * BN;
  const int iy0 = tyi * TH - p.pt, ix0 = txi * TILE_W - p.pl;
  const int npairs = p.cin / 64;                                 // pairs of 32-channel chunks

  // LDS-DMA by buffer loads, as in conv3x3_w4_kernel: per-lane offsets are constants, the moving part of every
  // address is scalar, the range check zero-fills halo slots outside the image
  constexpr unsigned OOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<half_t*>(x) + (size_t)img * p.h * p.w * p.cin, 0, p.h * p.w * p.cin * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<half_t*>(w), 0, 9 * p.cout * p.cin * 2, 0x00020000);
  unsigned hvo[W4S_NH];
#pragma unroll
  for (int u = 0; u < W4S_NH; ++u) {
    const int idx = u * 256 + tid;
    const int hp = idx >> 2, sl = idx & 3;
    const int hy = hp / WT, hx = hp - hy * WT;
    const int iy = iy0 + hy, ix = ix0 + hx;
    hvo[u] = (hp < W4_HT * WT && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w)
                 ? (unsigned)(((iy * p.w + ix) * p.cin + ((sl ^ w4s_swz(hp)) << 3)) * 2)
                 : OOB;
  }
  const int wrow = tid >> 2;
  const unsigned wvo = (unsigned)((wrow * p.cin + (((tid & 3) ^ (((wrow >> 3) & 1) << 1)) << 3)) * 2);

  auto dma_halo = [&](int q, int hb, int u) {       // 32-channel chunk q of this tile -> halo buffer hb
    if constexpr ((W4_ABL & 2) != 0) { if (q > 0) return; }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        xrs, (__attribute__((address_space(3))) void*)(smem + hb * W4S_HBYTES + (u * 256 + wave * 64) * 16), 16,
        hvo[u], q * 64, 0, 0);
  };
  // 64-cout part u of the [BN couts][32 channels] slice of (chunk q, tap) -> ring slot
  auto dma_wq = [&](int q, int tap, int ring, int u) {
    const int tapw = p.flip ? (8 - tap) : tap;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        wrs, (__attribute__((address_space(3))) void*)(wbuf + ring * WSTEP + (u * 256 + wave * 64) * 16), 16, wvo,
        (((tapw * p.cout + co0 + u * 64) * p.cin) + q * 32) * 2, 0, 0);
  };
  auto dma_w = [&](int q, int tap, int ring) {
#pragma unroll
    for (int u = 0; u < NW; ++u) dma_wq(q, tap, ring, u);
  };

  // pixel fragment of tile t at tap (ky,kx): hp = (2*wave + (t>>1) + ky)*34 + (t&1)*16 + kx + L; the swizzle
  // key hp & 7 = (L + 4*(wave&1) + u) & 7 with u = (2*((t>>1)+ky) + kx) & 7 static
  unsigned tb[8];
#pragma unroll
  for (int u = 0; u < 8; ++u)
    tb[u] = (unsigned)((wave * 2 * WT + L) * 64 + ((kg ^ w4s_swz((L + 4 * (wave & 1) + u) & 7)) << 4));
  const unsigned a_lane = (unsigned)(2 * W4S_HBYTES + L * 64 + ((kg ^ (((L >> 3) & 1) << 1)) << 4));

  f32x4 acc[AI][AT];
#pragma unroll
  for (int i = 0; i < AI; ++i)
#pragma unroll
    for (int t = 0; t < AT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  half8_t fa[AI], fb[2][AT];      // weight fragments: each is re-read right behind the only MFMA group that uses it

  OCR_DIAG_BEGIN()
#pragma unroll
  for (int u = 0; u < W4S_NH; ++u) dma_halo(0, 0, u);
#pragma unroll
  for (int sI = 0; sI < AHEAD; ++sI) dma_w(sI / 9, sI % 9, sI);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < AI; ++i) fa[i] = *reinterpret_cast<const half8_t*>(smem + (a_lane + i * 1024));
#pragma unroll
  for (int t = 0; t < AT; ++t)
    fb[0][t] = *reinterpret_cast<const half8_t*>(smem + (tb[(2 * (t >> 1)) & 7] + ((t >> 1) * WT + (t & 1) * 16) * 64));

  for (int pr = 0; pr < npairs; ++pr) {
    const int s0 = pr * 18;
    const int q0 = pr * 2;                          // this pair's first 32-channel chunk
    const int qlast = 2 * npairs - 1;
    static_for<0, 18>([&](auto J) {
      constexpr int j = decltype(J)::value;
      constexpr int P = j & 1, Q = P ^ 1;
      constexpr int c = j / 9;                      // chunk of the pair = halo buffer
      constexpr int jn = (j + 1) % 18, cn = jn / 9, tapn = jn % 9, kyn = tapn / 3, kxn = tapn % 3;
      constexpr int jd = (j + AHEAD) % 18, cd = jd / 9, tapd = jd % 9;
      constexpr bool dnext = j + AHEAD >= 18;
      // the weight slice of step s+1 (own share) has landed once nothing older than the DMAs of the steps
      // s-AHEAD+2 .. s-1 (slices of s+2 .. s+AHEAD-1 and the halo pieces issued in those steps) is outstanding
      constexpr int outstanding = [] {
        int n = 0;
        for (int k = 1; k <= AHEAD - 2; ++k) {
          const int jk = (j + 18 - k) % 18;
          n += NW + ((jk % 9) < HSTEPS ? HPS : 0);
        }
        return n;
      }();
      if constexpr (!(W4_ABL & 16)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(outstanding) : "memory");
      if constexpr (!(W4_ABL & 4)) __builtin_amdgcn_s_barrier();
      const int sd_ring = (s0 + j + AHEAD) & (RING - 1);
      int qd = q0 + cd + (dnext ? 2 : 0);
      qd = qd > qlast ? qlast : qd;                 // tail: redundant re-fetch keeps the vmcnt arithmetic uniform
      int qh = q0 + c + 1;
      qh = qh > qlast ? qlast : qh;
      const unsigned abase = a_lane + (unsigned)(((s0 + j + 1) & (RING - 1)) * WSTEP);
      auto read_b = [&](int t) {
        if constexpr ((W4_ABL & 8) != 0) return;
        const int u = (2 * ((t >> 1) + kyn) + kxn) & 7;
        fb[Q][t] = *reinterpret_cast<const half8_t*>(
            smem + (tb[u] + cn * W4S_HBYTES + (((t >> 1) + kyn) * WT + (t & 1) * 16 + kxn) * 64));
      };
      auto read_a = [&](int i) {
        if constexpr ((W4_ABL & 8) != 0) return;
        fa[i] = *reinterpret_cast<const half8_t*>(smem + (abase + i * 1024));
      };
      // one operation per MFMA gap (see conv3x3_w4_kernel): pixel fragments behind the first MFMAs of groups 0
      // and 1, the halo pieces behind their third, the weight DMAs in groups 2.., weight fragment g (single
      // buffered) behind the last MFMA of the only group that uses it
#pragma unroll
      for (int g = 0; g < AI; ++g) {
#pragma unroll
        for (int t = 0; t < AT; ++t) {
          if (j == 17 && g == AI - 1 && t == AT - 1) mfma16_acc_drain(acc[g][t], fa[g], fb[P][t]);   // see common.h
          else mfma16_acc(acc[g][t], fa[g], fb[P][t]);
          if (t == AT - 1) {
            read_a(g);
          } else if (g < 2) {
            if (t < 2) read_b(g * 2 + t);
            else if constexpr ((j % 9) < HSTEPS) dma_halo(qh, c ^ 1, (j % 9) * HPS + g);
          } else if (t == 1 && g - 2 < NW) {
            if constexpr (!(W4_ABL & 1)) dma_wq(qd, tapd, sd_ring, g - 2);
          }
        }
      }
    });
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");
  OCR_DIAG_END(ocr_diag_conv)
  __syncthreads();                                   // every wave's DMAs have landed: the LDS is free
  if constexpr ((W4_ABL & 32) != 0) {
    if (acc[0][0][0] == 12345.f) y[0] = (half_t)1;     // keeps the accumulators alive
    return;
  }
  {
    const int mt8 = (img * p.tiles_y + tyi) * p.tiles_x + txi;
    char* const stage = smem + wave * 2048;
    const bool has_bias = EPI == 0 ? (p.flags & OCR_CONV_BIAS) != 0 : EPI == 3;
    const bool relu = EPI == 0 ? (p.flags & OCR_CONV_RELU) != 0 : EPI == 3;
    const bool accum = EPI == 0 ? (p.flags & OCR_CONV_ACCUM_F16) != 0 : false;
    const bool do_stats = EPI == 0 ? (p.flags & OCR_CONV_STATS) != 0 : (EPI == 1 || EPI == 2 || EPI == 4);
    const bool has_br = EPI == 0 ? p.br.y != nullptr : (EPI == 2 || EPI == 4);
    const int g4 = lane >> 4;
    const int c8 = lane & 7, pg = lane >> 3;
    // the tile's BN bias values through LDS (see conv3x3_w4_kernel)
    float* const lbias = reinterpret_cast<float*>(smem + 4 * 2048 + 4096);
    if (has_bias) {
      if (tid < BN) lbias[tid] = bias[co0 + tid];
      __syncthreads();
    }
    float s[NW][8], q2[NW][8];
#pragma unroll
    for (int hf = 0; hf < NW; ++hf)
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[hf][e] = 0.f; q2[hf][e] = 0.f; }
    // (scale / shift decide the ReLU mask per element; mean / invstd enter linearly and are applied to the
    // sums at the end: sum dz*xhat = invstd * (sum dz*y - mean * sum dz))
    float bsc[NW][8], bsh[NW][8];
    const float relu_thr = p.br.relu ? OCR_RELU_TIE : -INFINITY;   // no ReLU: every element passes
    const float nthr_h = -relu_thr * 0x1p60f;                      // (epi_step)
    const bool sdz = EPI == 0 ? (has_br && p.br.store_dz != 0) : EPI == 4;
    if (has_br) {
#pragma unroll
      for (int hf = 0; hf < NW; ++hf)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int cc = co0 + hf * 64 + c8 * 8 + e;
          bsc[hf][e] = p.br.scale[cc]; bsh[hf][e] = p.br.shift[cc];
        }
    }
    // Round it = NW*t + hf.  The BN-backward operand of the whole tile (32 KB x NW: the main loop's LDS is free) comes
    // by LDS-DMA up front, all transfers in flight at once, each lane fetching the 16 bytes it reads back itself (see
    // conv3x3_w4_kernel's epilogue: register prefetches share the vmcnt queue with the rounds' stores)
    constexpr int NR = AT * NW;
    half8_t oq[2];
    // element offset of (round, k): per-lane base + wave-uniform delta; bounds as rows / columns left (see conv3x3_w4)
    const size_t pbase = (((size_t)img * p.oh + tyi * TH + wave * 2) * p.ow + txi * TILE_W + pg) * p.cout + co0 + c8 * 8;
    const int rows_left = p.oh - (tyi * TH + wave * 2), cols_left = p.ow - (txi * TILE_W + pg);
    auto round_off = [&](int it, int k, bool& ok) __attribute__((always_inline)) {
      const int t = it / NW, hf = it % NW;
      ok = ((t >> 1) < rows_left) & ((t & 1) * 16 + k * 8 < cols_left);
      return pbase + (size_t)(((t >> 1) * p.ow + (t & 1) * 16 + k * 8) * p.cout + hf * 64);
    };
    static_assert(16384 + 4 * NR * 2048 <= w4s_lds(BN), "operand tile past the kernel's LDS");
    char* const ylds = smem + 16384 + wave * (NR * 2048);   // past the staging rows, the partial sums and the bias values
    if (has_br) {
      const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<half_t*>(p.br.y) + (size_t)img * p.oh * p.ow * p.cout, 0, p.oh * p.ow * p.cout * 2, 0x00020000);
      const unsigned ybase = (unsigned)((((tyi * TH + wave * 2) * p.ow + txi * TILE_W + pg) * p.cout + co0 + c8 * 8) * 2);
#pragma unroll
      for (int it = 0; it < NR; ++it)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int t = it / NW, hf = it % NW;
          const bool ok = ((t >> 1) < rows_left) & ((t & 1) * 16 + k * 8 < cols_left);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(
              yrs, (__attribute__((address_space(3))) void*)(ylds + (it * 2 + k) * 1024), 16, ok ? ybase : 0x80000000u,
              (((t >> 1) * p.ow + (t & 1) * 16 + k * 8) * p.cout + hf * 64) * 2, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < AT; ++t) {
#pragma unroll
      for (int hf = 0; hf < NW; ++hf) {
        const int it = t * NW + hf;
        if (accum) {                                  // old gradient of this round: in flight under the staging
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            bool ok;
            const size_t off = round_off(it, k, ok);
            if (ok) oq[k] = *reinterpret_cast<const half8_t*>(y + off);
          }
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          const int i = hf * 4 + ii;
          f32x4 bv = {0.f, 0.f, 0.f, 0.f};
          if (has_bias) bv = *reinterpret_cast<const f32x4*>(lbias + (i * 16 + g4 * 4));   // one LDS read, not four loads
          float vq4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = acc[i][t][e];
            if (has_bias) v += bv[e];        // (an unconditional "+ 0.f" is not folded away: -0.f + 0.f = +0.f)
            if (relu) v = v > 0.f ? v : 0.f;
            vq4[e] = v;
          }
          const half4_t o = epi_pack4(vq4[0], vq4[1], vq4[2], vq4[3]);
          *reinterpret_cast<half4_t*>(stage + L * 128 + (((ii * 2 + (g4 >> 1)) ^ (L & 7)) << 4) + (g4 & 1) * 8) = o;
        }
        if (it == 0 && has_br) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the operand tile has landed (behind round 0's staging)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          bool ok;
          const size_t off = round_off(it, k, ok);
          const int px = k * 8 + pg;
          if (ok) {
            half8_t v = *reinterpret_cast<const half8_t*>(stage + px * 128 + ((c8 ^ (px & 7)) << 4));
            half8_t yv;
            if (has_br) yv = *reinterpret_cast<const half8_t*>(ylds + (it * 2 + k) * 1024 + lane * 16);
            if (accum) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] + (float)oq[k][e]);
            }
            if (sdz) {                                // store the gradient PAST the ReLU (BnRed::store_dz)
#pragma unroll
              for (int e = 0; e < 8; ++e)
                if (!((float)yv[e] * bsc[hf][e] + bsh[hf][e] > relu_thr)) v[e] = (half_t)0.f;
            }
            OCR_EPI_STORE(2, reinterpret_cast<half8_t*>(y + off), v);
            if (do_stats) {
              if (has_br) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  const float yf = (float)yv[e];
                  const float dz = epi_step(yf * bsc[hf][e] + bsh[hf][e], relu_thr, nthr_h) * (float)v[e];   // mask of the stored activation
                  s[hf][e] += dz;
                  q2[hf][e] += dz * yf;
                }
              } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  const float f = (float)v[e];
                  s[hf][e] += f;
                  q2[hf][e] += f * f;
                }
              }
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
    if (do_stats) {
      if (has_br) {
#pragma unroll
        for (int hf = 0; hf < NW; ++hf)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int cc = co0 + hf * 64 + c8 * 8 + e;
            q2[hf][e] = (q2[hf][e] - p.br.mean[cc] * s[hf][e]) * p.br.invstd[cc];
          }
      }
#pragma unroll
      for (int hf = 0; hf < NW; ++hf)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma unroll
          for (int o = 8; o < 64; o <<= 1) {
            s[hf][e] += __shfl_xor(s[hf][e], o, 64);
            q2[hf][e] += __shfl_xor(q2[hf][e], o, 64);
          }
        }
      // the four waves (pixel quarters) meet in LDS, summed in wave order: one partial row per tile
      float* const red = reinterpret_cast<float*>(smem + 4 * 2048);     // [4 waves][2][BN]
      if (pg == 0) {
        float* row = red + wave * 2 * BN + c8 * 8;
#pragma unroll
        for (int hf = 0; hf < NW; ++hf)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            row[hf * 64 + e] = s[hf][e];
            row[BN + hf * 64 + e] = q2[hf][e];
          }
      }
      __syncthreads();
      if (tid < 2 * BN)
        stats[((size_t)mt8 * 2 + tid / BN) * p.cout + co0 + tid % BN] =
            ((red[tid] + red[2 * BN + tid]) + red[4 * BN + tid]) + red[6 * BN + tid];
    }
  }
  OCR_DIAG_WG_END(ocr_diag_conv)
}

// ---------------------------------------------------------------------------------------------
// 64 input channels, 3x3 / stride 1, on large maps (conv1_2 forward / input gradient: 2.1 GB of activations
// for 0.62 TFLOP — the floor is the HBM stream, not MFMA; also ResNet's block1 3x3).  The tap-sweeping
// kernels re-fetch 72 KB of weight slices per 32 KB of output here.  This variant is PERSISTENT and
// WEIGHT-STATIONARY:
//   * a workgroup stages all nine [64 couts][64 channels] slices of its cout tile in LDS once (72 KB, rows of
//     128 B, chunk ^ ((row >> 1) & 7)) and then walks 8 x 32-pixel tiles;
//   * the 64-channel halo of a tile (10 x 34 pixels x 128 B, chunk ^ (pixel & 7), zero padding by the buffer
//     range check) goes global -> LDS by LDS-DMA into one of TWO buffers: the halo of tile k+1 is requested
//     before tile k's MFMAs and has their whole duration to land (the first version of this kernel
//     carried it through registers: six 16-byte loads per thread with their address arithmetic, six LDS
//     stores and two block barriers per tile);
//   * wave w owns tile row w (32 pixels) x all 64 couts: 18 k-steps of 8 MFMAs from LDS alone; its output
//     rows are whole 128-byte lines, so the epilogue is wave-private — staged through 4 KB of the halo
//     buffer the tile was just computed from (dead by then);
//   * the epilogue's global operands (BN-backward operand, old gradient under ACCUM) are requested before
//     the MFMAs; batch-norm partials are accumulated per lane over ALL tiles of the wave and leave as
//     one row per wave of the grid (ocr_conv2d_num_mtiles: 8 x workgroups per cout tile).
// Per tile: DMA(k+1) | MFMAs(k) | wait for DMA(k+1) + barrier (every wave is done reading halo k, halo k+1 is
// visible) | epilogue(k) | barrier (staging reads done: the buffer may receive DMA(k+2)).  The wait sits BEFORE
// the epilogue's stores are issued, so it never waits for them.
typedef short c64_short4v __attribute__((__vector_size__(4 * sizeof(short))));
typedef __attribute__((address_space(3))) c64_short4v* c64_lds_s4_ptr;
__device__ __forceinline__ half8_t c64_tr_pair(const char* base, int second_off) {
  c64_short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((c64_lds_s4_ptr)(base));
  c64_short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((c64_lds_s4_ptr)(base + second_off));
  typedef short short8v __attribute__((ext_vector_type(8)));
  short8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(half8_t, v);
}
constexpr int C64_NH = 6;                                          // halo DMA rounds of 512 slots (2720 slots used)
constexpr int C64_LDS = 2 * W4_HBYTES + 9 * 64 * 128;              // 163840 = the whole LDS

template <int BN, bool POOL = false, int EPI = 0>   // EPI: the epilogue mode at compile time (see conv3x3_w4_kernel)
__global__ __launch_bounds__(512) void conv_c64_persist_kernel(
    ConvP p, const half_t* __restrict__ x, const half_t* __restrict__ w,
    const float* __restrict__ bias, half_t* __restrict__ y, float* __restrict__ stats) {
  static_assert(BN == 64, "one 64-cout tile per workgroup");
  constexpr int TH = 8, WT = W4_WT, AI = 4, AT = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wst = smem + 2 * W4_HBYTES;             // [9][64 couts][128 B]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // = tile row
  const int L = lane & 15, kg = lane >> 4;
  const int nt = blockIdx.x % p.n_tiles;
  const int co0 = nt * BN;
  const int m_first = blockIdx.x / p.n_tiles, m_step = gridDim.x / p.n_tiles;
  const int m_tiles = p.n * p.tiles_x * p.tiles_y;
  const int ntile = m_first < m_tiles ? (m_tiles - m_first + m_step - 1) / m_step : 0;
  const bool has_bias = EPI == 0 ? (p.flags & OCR_CONV_BIAS) != 0 : EPI == 3;
  const bool relu = EPI == 0 ? (p.flags & OCR_CONV_RELU) != 0 : EPI == 3;
  const bool accum = EPI == 0 ? (p.flags & OCR_CONV_ACCUM_F16) != 0 : false;
  const bool do_stats = EPI == 0 ? (p.flags & OCR_CONV_STATS) != 0 : (EPI == 1 || EPI == 2 || EPI == 4 || EPI == 6 || EPI == 7);
  const bool has_br = EPI == 0 ? p.br.y != nullptr : (EPI == 2 || EPI == 4 || EPI == 6 || EPI == 7);  // (fields read by value: a pointer to p.br would pin the arguments in scratch)
  // mode 6 = mode 2 with the producing layer's y RECOMPUTED (BnRed::first_x4): conv1_1 under conv1_2's input gradient
  // mode 7 = mode 6 that does NOT store the gradient: conv1_1's weight gradient is its only other reader, and
  //   dW = A .* (V^T dz) + B .* (M W) + C .* m        (dy = A dz + B y + C per channel; V = the 27-value image patches,
  //   M = V^T V and m = sum V: ocr_conv2d_first_moments_f16 has them) needs only S1 = V^T dz, which this epilogue
  //   accumulates per wave on the matrix cores (BnRed::first_s1) — the 1 GiB gradient is neither written nor read again
  constexpr bool RECOMP = EPI == 6 || EPI == 7;
  constexpr bool FWG = EPI == 7;
  f32x16 s1acc[FWG ? 2 : 1];
  if constexpr (FWG) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) s1acc[i][e] = 0.f;
  }
  const int r32 = lane & 31, h32 = lane >> 5;         // the 32x32x16 MFMA's lane -> (row / pixel, k half) map
  half8_t fw[RECOMP ? 3 : 1][2];                      // first-layer weights: the same for every tile
  if constexpr (RECOMP) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        fw[ky][i] = *reinterpret_cast<const half8_t*>(p.br.first_wf + ((size_t)(ky * p.cout + co0 + i * 32 + r32)) * 16 + 8 * h32);
  }

  // weights -> LDS, once: slot tap*512 + tid -> row tid>>3, stored chunk tid&7 holds logical chunk c ^ swz
  {
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<half_t*>(w), 0, 9 * p.cout * p.cin * 2, 0x00020000);
    const int rr = tid >> 3, c = tid & 7;
    const unsigned wvo = (unsigned)((rr * p.cin + ((c ^ ((rr >> 1) & 7)) << 3)) * 2);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int tapw = p.flip ? (8 - tap) : tap;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wrs, (__attribute__((address_space(3))) void*)(wst + tap * 8192 + wave * 1024), 16, wvo,
          ((tapw * p.cout + co0) * p.cin) * 2, 0, 0);
    }
  }

  auto tile_of = [&](int k, int& img, int& tyi, int& txi) __attribute__((always_inline)) {
    const int mt = m_first + k * m_step;
    txi = mt % p.tiles_x;
    const int tmp = mt / p.tiles_x;
    tyi = tmp % p.tiles_y;
    img = tmp / p.tiles_y;
  };
  // halo of this workgroup's k-th tile -> buffer hb (6 rounds of 512 slots; slots past the 340 pixels fall
  // into the buffer's padding, the waves that would leave it sit the last round out)
  constexpr unsigned OOB = 0x80000000u;
  auto dma_tile = [&](int k, int hb) __attribute__((always_inline)) {
    int img, tyi, txi;
    tile_of(k, img, tyi, txi);
    const int iy0 = tyi * TH - p.pt, ix0 = txi * TILE_W - p.pl;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<half_t*>(x) + (size_t)img * p.h * p.w * p.cin, 0, p.h * p.w * p.cin * 2, 0x00020000);
#pragma unroll
    for (int u = 0; u < C64_NH; ++u) {
      if (u == C64_NH - 1 && (u * 512 + wave * 64) * 16 >= W4_HBYTES) continue;      // waves 4..7, last round
      const int idx = u * 512 + tid;
      const int hp = idx >> 3, sl = idx & 7;
      const int hy = hp / WT, hx = hp - hy * WT;
      const int iy = iy0 + hy, ix = ix0 + hx;
      const unsigned off = ((hp < W4_HT * WT) & ((unsigned)iy < (unsigned)p.h) & ((unsigned)ix < (unsigned)p.w))
                               ? (unsigned)(((iy * p.w + ix) * p.cin + ((sl ^ (hp & 7)) << 3)) * 2)
                               : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          xrs, (__attribute__((address_space(3))) void*)(smem + hb * W4_HBYTES + (u * 512 + wave * 64) * 16), 16, off,
          0, 0, 0);
    }
  };

  // pixel fragment of 16-pixel group t at tap (ky,kx): halo pixel hp = (wave + ky)*34 + t*16 + kx + L, chunk
  // (ks*4 + kg) ^ (hp & 7); hp & 7 = (L + 2*wave + u) & 7 with u = (2*ky + kx) & 7 static
  unsigned tb[2][8];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int u = 0; u < 8; ++u)
      tb[ks][u] = (unsigned)((wave * WT + L) * 128 + (((ks * 4 + kg) ^ ((L + 2 * wave + u) & 7)) << 4));
  unsigned ab[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    ab[ks] = (unsigned)(2 * W4_HBYTES + L * 128 + (((ks * 4 + kg) ^ ((L >> 1) & 7)) << 4));

  // batch-norm partials: per lane over all tiles of this wave (its 8 couts are fixed; so are the producing layer's
  // BN coefficients of the fused BN-backward reduction: scale / shift decide the ReLU mask per element, mean /
  // invstd enter linearly and are applied to the sums at the end)
  const int c8 = lane & 7, pg = lane >> 3;
  float s[8], q2[8], bsc[8], bsh[8];
  const float relu_thr = p.br.relu ? OCR_RELU_TIE : -INFINITY;
  const bool sdz = EPI == 0 ? (has_br && p.br.store_dz != 0) : EPI == 4;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s[e] = 0.f;
    q2[e] = 0.f;
    bsc[e] = has_br ? p.br.scale[co0 + c8 * 8 + e] : 0.f;
    bsh[e] = has_br ? p.br.shift[co0 + c8 * 8 + e] : 0.f;
  }

  // this lane's 16 bias values (its accumulator quads' couts are fixed over the tiles)
  float bvv[AI][4];
#pragma unroll
  for (int i = 0; i < AI; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) bvv[i][e] = has_bias ? bias[co0 + i * 16 + (lane >> 4) * 4 + e] : 0.f;

  if (ntile > 0) dma_tile(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int k = 0; k < ntile; ++k) {
    const int hb = k & 1;
    int img, tyi, txi;
    tile_of(k, img, tyi, txi);
#ifndef C64_ABL
#define C64_ABL 0      // dev ablations: 1 no halo DMA in the loop, 2 no output stores, 4 no MFMAs, 8 no epilogue at all, 16 no MFMA loop at all
#endif
    // (modes 2 / 4 issue it BEHIND their operand requests below: in front of them hipcc waited for it — vmcnt(0) — before
    // the first request, i.e. the next tile's halo had to land before this tile's MFMAs could start)
    constexpr bool kDmaLate = !RECOMP && (EPI == 2 || EPI == 4);
    if (!kDmaLate && (C64_ABL & 1) == 0 && k + 1 < ntile) dma_tile(k + 1, hb ^ 1);        // lands under this tile's MFMAs
    // the epilogue's global operands of THIS tile, requested ahead of the MFMAs
    half8_t yq[4], oq[4];
    const int oy = tyi * TH + wave;
    {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int ox = txi * TILE_W + kk * 8 + pg;
        if constexpr (!RECOMP && (EPI == 2 || EPI == 4)) {
          // branch-free (a position outside the map reads element 0 and is ignored below): under `if (inside)` hipcc put
          // `s_waitcnt vmcnt(0)` in front of each of the four requests — each waited for the halo DMA issued just above
          // and for the request before it, at the head of every tile
          const bool inside = oy < p.oh && ox < p.ow;
          const size_t off = inside ? (((size_t)img * p.oh + oy) * p.ow + ox) * p.cout + co0 + c8 * 8 : 0;
          yq[kk] = *reinterpret_cast<const half8_t*>(p.br.y + off);
        } else if (oy < p.oh && ox < p.ow) {
          const size_t off = (((size_t)img * p.oh + oy) * p.ow + ox) * p.cout + co0 + c8 * 8;
          if (!RECOMP && do_stats && has_br) yq[kk] = *reinterpret_cast<const half8_t*>(p.br.y + off);
          if (accum) oq[kk] = *reinterpret_cast<const half8_t*>(y + off);
        }
      }
    }
    if (kDmaLate && (C64_ABL & 1) == 0 && k + 1 < ntile) dma_tile(k + 1, hb ^ 1);
    // mode 6: the image pixels of this wave's row of the first layer instead — per kernel row ky two adjacent pixels
    // (8 bytes each, 4 channels) per lane, exactly the fragment first_mfma reads from its LDS halo; zero outside
    u32x2 fim[RECOMP ? 3 : 1][2];
    if constexpr (RECOMP) {
      const half_t* xim = p.br.first_x4 + (size_t)img * p.oh * p.ow * 4;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int iy = oy + ky - 1, ix = txi * TILE_W + r32 + 2 * h32 - 1 + j;
          fim[ky][j] = u32x2{0u, 0u};
          if ((unsigned)iy < (unsigned)p.oh && (unsigned)ix < (unsigned)p.ow)
            fim[ky][j] = *reinterpret_cast<const u32x2*>(xim + ((size_t)iy * p.ow + ix) * 4);
        }
    }

    f32x4 acc[AI][AT];
#pragma unroll
    for (int i = 0; i < AI; ++i)
#pragma unroll
      for (int t = 0; t < AT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned hoff = (unsigned)(hb * W4_HBYTES);
    // 18 k-steps (tap, k-half) of 8 MFMAs, software-pipelined by hand: the six fragment reads of step s+1 are
    // issued behind the MFMAs of step s (pixel fragments double-buffered, weight fragment i re-read right behind
    // its last use), the MFMAs are asm statements so that the order holds.  Left to the compiler's schedule of
    // the builtins, both waves of a SIMD read, waited, then multiplied — in phase, nothing overlapped: 7 800
    // cycles per tile for 4 608 cycles of MFMAs + 3 400 of LDS reads (ablation: 0.48 of the kernel's 0.74 ms).
    if constexpr ((C64_ABL & 16) == 0) {
      half8_t fa[AI], fb[2][AT];
#pragma unroll
      for (int i = 0; i < AI; ++i) fa[i] = *reinterpret_cast<const half8_t*>(smem + (ab[0] + i * 2048));
#pragma unroll
      for (int t = 0; t < AT; ++t) fb[0][t] = *reinterpret_cast<const half8_t*>(smem + (hoff + tb[0][0] + (t * 16) * 128));
      static_for<0, 18>([&](auto J) {
        constexpr int j = decltype(J)::value;
        constexpr int P = j & 1, Q = P ^ 1;
        constexpr int jn = (j + 1) % 18, tapn = jn >> 1, ksn = jn & 1, kyn = tapn / 3, kxn = tapn % 3;
#pragma unroll
        for (int i = 0; i < AI; ++i)
#pragma unroll
          for (int t = 0; t < AT; ++t) {
            if (j == 17 && i == AI - 1 && t == AT - 1) mfma16_acc_v_drain(acc[i][t], fa[i], fb[P][t]);   // see common.h
            else mfma16_acc_v(acc[i][t], fa[i], fb[P][t]);
            if constexpr (j < 17) {
              if (i == 0) {
                const int u = (2 * kyn + kxn) & 7;
                fb[Q][t] = *reinterpret_cast<const half8_t*>(smem + (hoff + tb[ksn][u] + (kyn * WT + t * 16 + kxn) * 128));
              }
              if (t == AT - 1) fa[i] = *reinterpret_cast<const half8_t*>(smem + (ab[ksn] + tapn * 8192 + i * 2048));
            }
          }
      });
    }
    // halo k+1 (and the operands above) have landed; behind the barrier every wave is done reading halo k
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    // ---- wave-private epilogue: accumulator quads -> this wave's [32 px][64 co] staging rows in the dead halo
    // buffer (16-byte chunk index XOR (pixel & 7)) -> whole 128-byte output rows
    char* const stage = smem + hb * W4_HBYTES + wave * 4096;
    if ((C64_ABL & 8) != 0) {
      if (acc[0][0][0] == 12345.f) y[0] = (half_t)1;       // keeps the accumulators alive
      __builtin_amdgcn_s_barrier();
      continue;
    }
    {
      const int g4 = lane >> 4;
#pragma unroll
      for (int i = 0; i < AI; ++i) {
#pragma unroll
        for (int t = 0; t < AT; ++t) {
          const int px = t * 16 + L;
          float vq4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = acc[i][t][e];
            if (has_bias) v += bvv[i][e];        // (an unconditional "+ 0.f" is not folded away: -0.f + 0.f = +0.f)
            if (relu) v = v > 0.f ? v : 0.f;
            vq4[e] = v;
          }
          const half4_t o = epi_pack4(vq4[0], vq4[1], vq4[2], vq4[3]);
          *reinterpret_cast<half4_t*>(stage + px * 128 + (((i * 2 + (g4 >> 1)) ^ (px & 7)) << 4) + (g4 & 1) * 8) = o;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if constexpr (POOL) {
      // bias + ReLU layers followed by their 2x2/2 max-pool, the full-resolution activation read by nobody else
      // (PixelLink's conv1_2: nets/vgg.py:17-18): the two tile rows of a wave pair are staged side by side, so after a
      // workgroup barrier each lane pools one 2x2 window of 8 channels and ONLY the pooled tile (+ first-max positions,
      // window order (dy, dx) as ocr_maxpool_f16) leaves the CU — 1/4 of the bytes, and no pooling pass afterwards
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const char* pair = smem + hb * W4_HBYTES + (wave & ~1) * 4096;
      const int pp = (wave & 1) * 8 + pg;                     // pooled pixel of the row pair
      const int oy0 = tyi * TH + (wave & ~1), ox0 = txi * TILE_W + 2 * pp;
      const int poh = (p.oh + 1) >> 1, pow2 = (p.ow + 1) >> 1;
      const int poy = oy0 >> 1, pox = ox0 >> 1;
      if (poy < poh && pox < pow2) {
        float m[8];
        unsigned long long am = 0ull;
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx) {
            if (oy0 + dy < p.oh && ox0 + dx < p.ow) {
              const int px = 2 * pp + dx;
              const half8_t v = *reinterpret_cast<const half8_t*>(pair + dy * 4096 + px * 128 + ((c8 ^ (px & 7)) << 4));
              const unsigned long long pos = (unsigned long long)(dy * 2 + dx);
#pragma unroll
              for (int e = 0; e < 8; ++e)
                if ((float)v[e] > m[e]) {
                  m[e] = (float)v[e];
                  am = (am & ~(0xffull << (8 * e))) | (pos << (8 * e));
                }
            }
          }
        half8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)m[e];
        const size_t off = (((size_t)img * poh + poy) * pow2 + pox) * p.cout + co0 + c8 * 8;
        *reinterpret_cast<half8_t*>(p.pool_out + off) = o;
        if (p.pool_idx != nullptr) *reinterpret_cast<unsigned long long*>(p.pool_idx + off) = am;
      }
    } else {
    half8_t vq[RECOMP ? 4 : 1];
    half8_t dzq[FWG ? 4 : 1];
    if constexpr (RECOMP) {
      // the gradient chunks out of the staging rows first, then the same rows carry this wave's row of y: six MFMAs on
      // the fragments fetched above (first_mfma's sequence for one tile row), rounded to the storage type as the
      // forward rounds it, staged in the layout the chunks are read back in
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int px = kk * 8 + pg;
        vq[kk] = *reinterpret_cast<const half8_t*>(stage + px * 128 + ((c8 ^ (px & 7)) << 4));
      }
      f32x16 ya[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) ya[i][e] = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const half4_t lo = __builtin_bit_cast(half4_t, fim[ky][0]), hi = __builtin_bit_cast(half4_t, fim[ky][1]);
        const half8_t b = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int i = 0; i < 2; ++i) ya[i] = OCR_MFMA_32x32x16(fw[ky][i], b, ya[i], 0, 0, 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();                    // every lane holds its gradient chunks
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          half4_t o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (half_t)ya[i][q * 4 + e];
          *reinterpret_cast<half4_t*>(stage + r32 * 128 + (((i * 4 + q) ^ (r32 & 7)) << 4) + h32 * 8) = o;
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int px = kk * 8 + pg;
        yq[kk] = *reinterpret_cast<const half8_t*>(stage + px * 128 + ((c8 ^ (px & 7)) << 4));
      }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int px = kk * 8 + pg;
      const int ox = txi * TILE_W + px;
      if constexpr (FWG) {
#pragma unroll
        for (int e = 0; e < 8; ++e) dzq[kk][e] = (half_t)0.f;       // outside the map: no contribution
      }
      if (oy < p.oh && ox < p.ow) {
        half8_t v;
        if constexpr (RECOMP) v = vq[kk];
        else v = *reinterpret_cast<const half8_t*>(stage + px * 128 + ((c8 ^ (px & 7)) << 4));
        const size_t off = (((size_t)img * p.oh + oy) * p.ow + ox) * p.cout + co0 + c8 * 8;
        if (accum) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] + (float)oq[kk][e]);
        }
        if (sdz) {                                    // store the gradient PAST the ReLU (BnRed::store_dz)
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (!((float)yq[kk][e] * bsc[e] + bsh[e] > relu_thr)) v[e] = (half_t)0.f;
        }
        if constexpr (!FWG) {
          if ((C64_ABL & 2) == 0 || v[0] == (half_t)12345.f) OCR_EPI_STORE(1, reinterpret_cast<half8_t*>(y + off), v);
        }
        if (do_stats) {
          if (has_br) {
            float dzf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float yf = (float)yq[kk][e];
              const bool pass = yf * bsc[e] + bsh[e] > relu_thr;                      // mask of the stored activation
              const float dz = pass ? (float)v[e] : 0.f;
              dzf[e] = dz;
              s[e] += dz;
              q2[e] += dz * yf;
            }
            if constexpr (FWG) {
              // the masked gradient back to 16 bits (exact: it came from there) by packed converts of the f32 values the
              // sums use — a select per 16-bit element and the re-packing were 50 instructions a tile on a kernel that is
              // bound by instruction issue
#pragma unroll
              for (int e = 0; e < 8; e += 2) {
                const half2_t h2 = __builtin_convertvector(f32x2{dzf[e], dzf[e + 1]}, half2_t);
                dzq[kk][e] = h2[0];
                dzq[kk][e + 1] = h2[1];
              }
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float f = (float)v[e];
              s[e] += f;
              q2[e] += f * f;
            }
          }
        }
      }
    }
    if constexpr (FWG) {
      // S1 += V^T dz over this wave's 32 pixels: M = 32 patch slots, N = 64 channels (two halves), K = pixels.  The 4 KB
      // staging rows are dead (every lane holds its chunks); they now carry the dz half tile [32 px][32 ch] (64-byte
      // rows) and, behind it, the patch rows [32 px][32 slots]: slot ky*10 + kx*3 + c (30 used, slot ky*10 + 9 is the
      // image's zero 4th channel) — both MFMA operands come out of transposing reads (conv_first.hip's weight gradient)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      char* const dzt = stage;
      char* const pat = stage + 2048;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        // lanes h32 = 0 hold the pixels kx = 0, 1 (6 values -> 3 dwords at slot ky*10), lanes h32 = 1 the pixel kx = 2
        // (+ the zero-weight kx = 3): 2 dwords at slot ky*10 + 6 (the second one written twice: one code path)
        const unsigned a0 = fim[ky][0][0], a1 = fim[ky][0][1], b0 = fim[ky][1][0], b1 = fim[ky][1][1];
        const unsigned w1 = h32 ? a1 : ((a1 & 0xffffu) | (b0 << 16));
        const unsigned w2 = h32 ? a1 : ((b0 >> 16) | (b1 << 16));
        char* const row = pat + r32 * 64 + ky * 20 + h32 * 12;
        *reinterpret_cast<unsigned*>(row) = a0;
        *reinterpret_cast<unsigned*>(row + 4) = w1;
        *reinterpret_cast<unsigned*>(row + (h32 ? 4 : 8)) = w2;
      }
      const int li = lane & 15, g4 = lane >> 4;
      const int tr_lane = (8 * (g4 >> 1) + (li >> 2)) * 64 + (16 * (g4 & 1) + 4 * (li & 3)) * 2;
      half8_t pf[2];
#pragma unroll
      for (int nh = 0; nh < 2; ++nh) {
        if ((c8 >> 2) == nh) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
            *reinterpret_cast<half8_t*>(dzt + (kk * 8 + pg) * 64 + (c8 & 3) * 16) = dzq[kk];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (nh == 0) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) pf[ks] = c64_tr_pair(pat + tr_lane + ks * 16 * 64, 4 * 64);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const half8_t df = c64_tr_pair(dzt + tr_lane + ks * 16 * 64, 4 * 64);
          s1acc[nh] = OCR_MFMA_32x32x16(pf[ks], df, s1acc[nh], 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                  // the second half overwrites the rows just read
      }
    }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // own staging reads are done ...
    __builtin_amdgcn_s_barrier();                         // ... and everyone's: the buffer may receive the halo of tile k+2
  }
  if constexpr (FWG) {
    // the eight waves' S1 blocks meet in LDS (dead by now: every wave is behind the last tile's closing barrier) and
    // leave as ONE [32][64] block per workgroup, summed in wave order
    float* const red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int nh = 0; nh < 2; ++nh)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        red[wave * 2048 + ((e & 3) + 8 * (e >> 2) + 4 * h32) * 64 + nh * 32 + r32] = s1acc[nh][e];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = u * 512 + tid;
      float a = red[i];
#pragma unroll
      for (int w8 = 1; w8 < 8; ++w8) a += red[w8 * 2048 + i];
      p.br.first_s1[(size_t)blockIdx.x * 2048 + i] = a;
    }
  }
  if (do_stats) {
    if (has_br) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        q2[e] = (q2[e] - p.br.mean[co0 + c8 * 8 + e] * s[e]) * p.br.invstd[co0 + c8 * 8 + e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) {
        s[e] += __shfl_xor(s[e], o, 64);
        q2[e] += __shfl_xor(q2[e], o, 64);
      }
    }
    if (pg == 0) {
      float* row = stats + ((size_t)(m_first * 8 + wave) * 2) * p.cout + co0 + c8 * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        row[e] = s[e];
        row[p.cout + e] = q2[e];
      }
    }
  }
}

struct TileCfg { int bn, ck, th; };

// persistent weight-stationary variant: cin == 64, 64-cout tiles, 16x16x32 MFMA, 8-row tiles
static bool conv_c64_ok(const ConvP& p) {
  static const int on = [] { const char* e = getenv("OCR_CONV_PERSIST"); return e ? atoi(e) : 1; }();
  return on && p.m16 && p.cin == 64 && p.kh == 3 && p.kw == 3 && p.dil == 1 && p.stride == 1 &&
         p.n * p.tiles_x * ocr_cdiv(p.oh, 8) >= 128 &&   // enough pixel tiles to amortise the weight staging
         (size_t)p.h * p.w * p.cin * 2 < (1u << 31);      // per-image buffer descriptors
}

// workgroups per cout tile of the persistent 64-channel kernel: one workgroup per CU in all
static int c64_per(int m_tiles, int n_tiles) {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  int per = cus / n_tiles;
  if (per < 1) per = 1;
  if (per > m_tiles) per = m_tiles;
  return per;
}

// the epilogue mode of the wave-private-epilogue kernels, a compile-time constant in the kernel (see
// conv3x3_w4_kernel): anything unusual takes the generic instantiation (0), which reads the flags at run time
static int epi_mode(const ConvP& p) {
  const bool br = p.br.y != nullptr;
  const int fl = p.flags;
  if (p.br.first_x4 != nullptr) return p.br.first_s1 != nullptr ? 7 : 6;      // (conv_c64_persist_kernel only: the entry point checks the family)
  if (fl == OCR_CONV_STATS && !br) return 1;
  if (fl == OCR_CONV_STATS && br && p.br.mask == nullptr && p.br.mask_bits == nullptr) return p.br.store_dz ? 4 : 2;
  if (fl == (OCR_CONV_BIAS | OCR_CONV_RELU) && !br) return 3;
  if (fl == 0 && !br) return 5;
  return 0;
}

// 4-wave kernel: 3x3 / stride 1 / dilation 1, 64-channel chunks, 256-cout tiles, 16x16x32 MFMA
static bool conv_w4_ok(const ConvP& p) {
  static const int on = [] { const char* e = getenv("OCR_CONV_W4"); return e ? atoi(e) : 1; }();
  return on && p.m16 && p.kh == 3 && p.kw == 3 && p.dil == 1 && p.stride == 1 && p.cin % 64 == 0 && p.cout % 256 == 0;
}

// small-tile variant: two workgroups per CU; couts in 64- or 128-wide tiles (the 256-multiples go to conv3x3_w4)
static int conv_w4s_bn(const ConvP& p) {
  static const int on = [] { const char* e = getenv("OCR_CONV_W4S"); return e ? atoi(e) : 1; }();
  if (!(on && p.m16 && p.kh == 3 && p.kw == 3 && p.dil == 1 && p.stride == 1 && p.cin % 64 == 0)) return 0;
  if (p.cout % 256 == 0) return 0;
  // cin = cout = 64 on large maps (conv1_2): 72 KB of weight slices per 32 KB of output make the streamed-weight
  // form no faster than the weight-stationary persistent kernel (0.93 vs 0.91 ms at 32 x 512^2; ablations in
  // DESIGN.md) — that layer keeps conv_c64_persist_kernel
  if (p.cin == 64 && p.cout == 64 && conv_c64_ok(p)) return 0;
  return p.cout % 128 == 0 ? 128 : p.cout % 64 == 0 ? 64 : 0;
}

// Which kernel runs one call, on what grid, leaving how many partial rows — the ONE place this is decided: the launch
// (dispatch / dispatch_pwx), the row count the caller allocates (ocr_conv2d_num_mtiles), the name ocr_conv2d_variant
// reports and the entry points that exist for one family only all read it.
struct ConvPlan {
  enum Family { PW, PWX, W4S, W4, C64, IGEMM } family = IGEMM;
  int status = OCR_OK;            // OCR_ERR_UNSUPPORTED: no kernel takes this call
  int bn = 0, ck = 0, th = 0;     // the tile the launch uses (PW with cin = 64: not always the TileCfg's)
  int epi = 0;                    // W4S / W4 / C64: epi_mode; PW / PWX: the epilogue has global operands
  int ring = 2;                   // IGEMM: slots of the weight ring
  unsigned grid = 0, block = 512;
  size_t lds = 0;
  int xcd_swizzle = 0, tiles_y = 0, n_tiles = 0;      // ConvP's fields as the launch passes them
  int rows = 0;                   // partial rows [rows][2][cout] the launch writes
};

// p: filled, with the flags and p.br of the call; pool: the pooled epilogue (ocr_conv2d_relu_pool_f16); pwx: the
// operand-transforming pointwise kernel's MODE (0: the plain entry points)
static ConvPlan conv_plan(const ConvP& p, const TileCfg& c, bool pool = false, int pwx = 0) {
  ConvPlan s;
  s.bn = c.bn; s.ck = c.ck; s.th = c.th;
  s.tiles_y = p.tiles_y;
  s.n_tiles = p.n_tiles;
  if (p.pw || pwx) {
    s.family = pwx ? ConvPlan::PWX : ConvPlan::PW;
    if (pool || (pwx && (!p.pw || p.cin < 128))) {       // (cin = 64: one stage, nothing to overlap the loads with)
      s.status = OCR_ERR_UNSUPPORTED;
      return s;
    }
    // two instantiations: the epilogue with global operands (ACCUM / BN-backward / tail) batches its loads
    // ahead of its stores (conv_epilogue.h) and needs ~40 more registers than the store-only one; the backward
    // form of the operand-transforming kernel always carries the fused BN-backward reduction
    s.epi = pwx ? pwx == 2 : (p.flags & OCR_CONV_ACCUM_F16) != 0 || p.br.y != nullptr;
    // cin = 64 (one K stage, nothing to prefetch under) without global operands in the epilogue: 128-cout tiles
    // need 70 KB of LDS and 118 registers — two workgroups per CU, whose phases overlap (ResNet's 64 -> 256
    // forward convolutions: one 256-cout workgroup per CU exposes its fetch latency on every tile)
    // (the same split for the epilogue WITH global operands — ResNet stage-1 tails, 64 -> 256 input gradients with four
    // operand streams — and 128-cout tiles on ONE stage buffer for store-only launches were measured too: not faster)
    if (!pwx && c.bn == 256 && p.cin == 64 && !s.epi) {
      s.bn = 128;
      s.n_tiles = p.cout / 128;
    }
    const size_t stage = (size_t)s.bn * 128 + 256 * 128;
    // one K stage (cin = 64): nothing to double-buffer; the transforming kernel: two stages + coefficients
    const size_t main_bytes = pwx ? 2 * stage + (size_t)p.cin * 16 : (p.cin == 64 ? 1 : 2) * stage;
    if (main_bytes > 160 * 1024) s.status = OCR_ERR_UNSUPPORTED;
    // the store-only epilogue takes a 256-cout tile in two halves, the one with global operands in one piece
    const size_t epi_bytes = conv_epilogue_lds(s.epi ? s.bn : (s.bn > 128 ? 128 : s.bn), 512);
    s.lds = main_bytes > epi_bytes ? main_bytes : epi_bytes;
    s.rows = (int)((p.npix + 255) / 256);                // flat 256-pixel tiles
    s.grid = (unsigned)s.rows * s.n_tiles;
    s.xcd_swizzle = s.n_tiles > 1 && s.grid % 8 == 0;
    return s;
  }
  s.rows = p.n * p.tiles_x * ocr_cdiv(p.oh, TILE_H);     // one row per 8-row pixel tile (the persistent kernel: below)
  const bool tail = p.br.mask != nullptr || p.br.mask_bits != nullptr;   // only the kernels ending in conv_epilogue_store implement it
  const bool tile64 = c.ck == 64 && c.th == 8;
  if (const int bn = tail || pool ? 0 : conv_w4s_bn(p)) {
    s.family = ConvPlan::W4S;
    s.bn = bn; s.ck = 64; s.th = 8;
    s.epi = epi_mode(p);
    s.tiles_y = ocr_cdiv(p.oh, 8);                 // (the tile configuration may have chosen 16-row tiles)
    s.n_tiles = p.cout / bn;
    s.block = 256;
    s.lds = (size_t)w4s_lds(bn);
  } else if (c.bn == 256 && tile64 && !tail && !pool && conv_w4_ok(p)) {
    s.family = ConvPlan::W4;
    s.epi = epi_mode(p);
    s.block = 256;
    s.lds = (size_t)W4_LDS;
  } else if (c.bn == 64 && tile64 && conv_c64_ok(p)) {
    s.family = ConvPlan::C64;
    // (the pooled variant exists for bias + ReLU layers only: its other modes are the generic instantiation)
    s.epi = pool && epi_mode(p) != 3 ? 0 : epi_mode(p);
    s.lds = (size_t)C64_LDS;
    const int per = c64_per(p.n * p.tiles_x * p.tiles_y, p.n_tiles);
    s.grid = (unsigned)(per * p.n_tiles);
    s.rows = 8 * per;                              // one row per wave of the persistent grid, not per tile ...
    if (per <= 0) s.status = OCR_ERR_HIP;
    if (tail) s.status = OCR_ERR_UNSUPPORTED;      // ... which the tail's kernels would not fill
    return s;
  } else {
    s.family = ConvPlan::IGEMM;
    // a three-slot weight ring for the 256-cout tiles, the slice requested two taps ahead (a four-slot ring was measured
    // too, on fc6 — 144 tap steps of 32 MFMAs per tile — and the strided ResNet convolutions: headline 19.85 -> 19.96 ms,
    // ResNet 39.31 -> 39.22: the tap step's cost is not the slice's fetch)
    if (c.bn == 256 && p.m16 && c.th == 8 && p.kh * p.kw >= 3 &&
        (size_t)p.halo_bytes + 3 * c.bn * conv_wrs(c.ck) <= 160 * 1024)
      s.ring = 3;
    const size_t main_bytes = (size_t)p.halo_bytes + s.ring * c.bn * conv_wrs(c.ck);
    const size_t epi_bytes = conv_epilogue_lds(c.bn > 128 ? 128 : c.bn, 512);
    s.lds = main_bytes > epi_bytes ? main_bytes : epi_bytes;
    if (s.lds > 160 * 1024 || pool) s.status = OCR_ERR_UNSUPPORTED;
  }
  s.grid = (unsigned)(p.n * p.tiles_x * s.tiles_y * s.n_tiles);
  s.xcd_swizzle = s.grid % 8 == 0;      // XCD-aware order: A/B -0.04 ms on the headline step (profiles/r06_ab_xcd_swizzle.txt)
  return s;
}

// A kernel and whether its dynamic-LDS limit has been raised (once per process; not atomic).
template <typename... KA>
struct Kern {
  void (*fn)(KA...);
  bool configured;
};
typedef Kern<ConvP, const half_t*, const half_t*, const float*, half_t*, float*> ConvKern;
typedef Kern<ConvP, PwX, const half_t*, half_t*, float*> PwxKern;

template <typename... KA>
static int launch_planned(Kern<KA...>& k, const ConvPlan& s, hipStream_t st, KA... args) {
  void (*const fn)(KA...) = k.fn;
  if (!k.configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(160 * 1024)) != hipSuccess)
      return OCR_ERR_HIP;
    k.configured = true;
  }
  hipLaunchKernelGGL(fn, dim3(s.grid), dim3(s.block), s.lds, st, args...);
  return ocr_launch_status();
}

// p as the planned launch passes it
static ConvP planned_params(const ConvP& p, const ConvPlan& s) {
  ConvP q = p;
  q.tiles_y = s.tiles_y;
  q.n_tiles = s.n_tiles;
  q.xcd_swizzle = s.xcd_swizzle;
  return q;
}

template <int BN, int WCO>
static ConvKern* pw_kern(const ConvPlan& s) {
  static ConvKern k[2] = {{conv_pw_kernel<BN, WCO, false>}, {conv_pw_kernel<BN, WCO, true>}};
  return &k[s.epi];
}

template <int BN, int CK, int WCO, int TH = 8>
static ConvKern* igemm_kern(const ConvPlan& s, bool m16) {
  static ConvKern k[2] = {{conv_igemm_kernel<BN, CK, WCO, false, TH>}, {conv_igemm_kernel<BN, CK, WCO, true, TH>}};
  if constexpr (BN == 256 && TH == 8) {
    static_assert((BN * (CK / 8)) % 512 == 0, "counted waits: every thread issues the same number of requests");
    static ConvKern k3 = {conv_igemm_kernel<BN, CK, WCO, true, TH, 3>};
    if (s.ring == 3) return &k3;
  }
  return &k[m16];
}

template <int BN>
static ConvKern* w4s_kern(const ConvPlan& s) {
  static ConvKern k[6] = {{conv3x3_w4s_kernel<BN, 0>}, {conv3x3_w4s_kernel<BN, 1>}, {conv3x3_w4s_kernel<BN, 2>},
                          {conv3x3_w4s_kernel<BN, 3>}, {conv3x3_w4s_kernel<BN, 4>}, {conv3x3_w4s_kernel<BN, 5>}};
  return &k[s.epi];
}

template <bool P>
static ConvKern* c64_kern(const ConvPlan& s) {
  static ConvKern k[8] = {{conv_c64_persist_kernel<64, P, 0>}, {conv_c64_persist_kernel<64, P, P ? 0 : 1>},
                          {conv_c64_persist_kernel<64, P, P ? 0 : 2>}, {conv_c64_persist_kernel<64, P, 3>},
                          {conv_c64_persist_kernel<64, P, P ? 0 : 4>}, {conv_c64_persist_kernel<64, P, P ? 0 : 5>},
                          {conv_c64_persist_kernel<64, P, P ? 0 : 6>}, {conv_c64_persist_kernel<64, P, P ? 0 : 7>}};
  return &k[s.epi];
}

static ConvKern* conv_kern(const ConvPlan& s, const ConvP& p) {
  static ConvKern w4[6] = {{conv3x3_w4_kernel<0>}, {conv3x3_w4_kernel<1>}, {conv3x3_w4_kernel<2>},
                           {conv3x3_w4_kernel<3>}, {conv3x3_w4_kernel<4>}, {conv3x3_w4_kernel<5>}};
  const bool k64 = s.ck == 64;
  switch (s.family) {
    case ConvPlan::PW: return s.bn == 256 ? pw_kern<256, 4>(s) : s.bn == 128 ? pw_kern<128, 2>(s) : pw_kern<64, 1>(s);
    case ConvPlan::W4S: return s.bn == 128 ? w4s_kern<128>(s) : w4s_kern<64>(s);
    case ConvPlan::W4: return &w4[s.epi];
    case ConvPlan::C64: return p.pool_out ? c64_kern<true>(s) : c64_kern<false>(s);
    case ConvPlan::IGEMM:
      if (s.bn == 256) return k64 ? igemm_kern<256, 64, 4>(s, p.m16) : igemm_kern<256, 32, 4>(s, p.m16);
      if (s.bn == 128 && s.th == 16) return k64 ? igemm_kern<128, 64, 2, 16>(s, p.m16) : igemm_kern<128, 32, 2, 16>(s, p.m16);
      if (s.bn == 128) return k64 ? igemm_kern<128, 64, 2>(s, p.m16) : igemm_kern<128, 32, 2>(s, p.m16);
      if (s.bn == 64) return k64 ? igemm_kern<64, 64, 2>(s, p.m16) : igemm_kern<64, 32, 2>(s, p.m16);
      return k64 ? igemm_kern<32, 64, 1>(s, p.m16) : igemm_kern<32, 32, 1>(s, p.m16);
    case ConvPlan::PWX: break;
  }
  return nullptr;
}

static int dispatch(const ConvP& p, const ConvPlan& s, const void* x, const void* w_kc, const void* bias, void* y,
                    void* stats, hipStream_t st) {
  if (s.status != OCR_OK) return s.status;
  ConvKern* k = conv_kern(s, p);
  if (!k) return OCR_ERR_UNSUPPORTED;
  return launch_planned(*k, s, st, planned_params(p, s), static_cast<const half_t*>(x), static_cast<const half_t*>(w_kc),
                        static_cast<const float*>(bias), static_cast<half_t*>(y), static_cast<float*>(stats));
}

template <int MODE>
static int dispatch_pwx(const ConvP& p, const ConvPlan& s, const PwX& t, const void* w, void* y, void* stats,
                        hipStream_t st) {
  if (s.status != OCR_OK) return s.status;
  constexpr bool EL = MODE == 2;
  static PwxKern kerns[3][2] = {
      {{conv_pwx_kernel<64, 1, EL, MODE, false>}, {conv_pwx_kernel<64, 1, EL, MODE, true>}},
      {{conv_pwx_kernel<128, 2, EL, MODE, false>}, {conv_pwx_kernel<128, 2, EL, MODE, true>}},
      {{conv_pwx_kernel<256, 4, EL, MODE, false>}, {conv_pwx_kernel<256, 4, EL, MODE, true>}}};
  const bool proj = (MODE == 1 && t.f1 != nullptr) ||    // the shortcut is a projection: its batch norm is applied too
                    (MODE == 2 && t.f3 != nullptr);      // the batch norm above is followed by a ReLU: its mask is applied too
  return launch_planned(kerns[s.bn == 256 ? 2 : s.bn == 128][proj], s, st, planned_params(p, s), t,
                        static_cast<const half_t*>(w), static_cast<half_t*>(y), static_cast<float*>(stats));
}

// Tile selection.  Workgroup tile = BN couts x (TH rows x 32 columns) pixels, CK input channels per
// LDS stage.  Per-wave register tile is 64 couts x 128 px wherever cout allows (accumulators = 128
// VGPRs), so narrow layers get taller pixel tiles: that halves the fragment reads per MFMA of the
// 64-/128-cout layers and amortises each streamed weight slice over more pixels.

// 1x1 stride-1 convs whose pixel count is a multiple of 32 go to the pointwise GEMM kernel
static bool conv_is_pw(const ocr_conv_desc* d) {
  static const int on = [] { const char* e = getenv("OCR_CONV_PW"); return e ? atoi(e) : 1; }();
  return on && d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad_top == 0 && d->pad_left == 0 &&
         d->oh == d->h && d->ow == d->w && d->cin % 64 == 0 && d->cout % 64 == 0 &&
         ((long long)d->n * d->oh * d->ow) % 32 == 0;
}

int fill_params(const ocr_conv_desc* d, ConvP* p, TileCfg* cfg) {
  OCR_CHECK_ARG(d != nullptr);
  OCR_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->oh > 0 && d->ow > 0);
  OCR_CHECK_ARG(d->kh > 0 && d->kw > 0 && d->stride > 0 && d->dilation > 0);
  OCR_CHECK_SHAPE(d->cin % 32 == 0 && d->cout % 32 == 0);
  p->pool_out = nullptr;
  p->pool_idx = nullptr;
  p->xcd_swizzle = 0;
  p->n = d->n; p->h = d->h; p->w = d->w; p->cin = d->cin;
  p->oh = d->oh; p->ow = d->ow; p->cout = d->cout;
  p->kh = d->kh; p->kw = d->kw; p->stride = d->stride; p->dil = d->dilation;
  p->pt = d->pad_top; p->pl = d->pad_left; p->flip = d->flip_taps; p->flags = d->flags;
  // MFMA shape: on random data the chip holds a higher clock on 16x16x32 than on 32x32x16 at equal
  // cycles per FLOP (MI355X_MICROARCH.md "DVFS give-back" item 7; measured here +3..5 % on the 3x3
  // layers, -20 % on the 1x1 fc7 whose per-tap loop is too short).
  p->m16 = d->kh * d->kw > 1;
  const int c64 = d->cin % 64 == 0;
  TileCfg cand[6];
  int nc = 0;
  if (d->cout % 256 == 0) { if (c64) cand[nc++] = {256, 64, 8}; cand[nc++] = {256, 32, 8}; }
  if (d->cout % 128 == 0) {
    if (d->oh > 8) { if (c64) cand[nc++] = {128, 64, 16}; cand[nc++] = {128, 32, 16}; }
    if (c64) cand[nc++] = {128, 64, 8};
    cand[nc++] = {128, 32, 8};
  } else if (d->cout % 64 == 0) {
    if (c64) cand[nc++] = {64, 64, 8};
    cand[nc++] = {64, 32, 8};
  } else {
    if (c64) cand[nc++] = {32, 64, 8};
    cand[nc++] = {32, 32, 8};
  }
  p->npix = (long long)d->n * d->oh * d->ow;
  p->pw = conv_is_pw(d);
  if (p->pw) {
    *cfg = {d->cout % 256 == 0 ? 256 : d->cout % 128 == 0 ? 128 : 64, 64, 8};
    p->HT = p->WT = 0; p->tiles_x = p->tiles_y = 0; p->halo_bytes = 0;
    p->n_tiles = d->cout / cfg->bn;
    p->br = BnRed{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    return OCR_OK;
  }
  p->WT = (TILE_W - 1) * d->stride + (d->kw - 1) * d->dilation + 1;
  p->tiles_x = ocr_cdiv(d->ow, TILE_W);
  for (int i = 0; i < nc; ++i) {
    const TileCfg c = cand[i];
    const int HT = (c.th - 1) * d->stride + (d->kh - 1) * d->dilation + 1;
    const size_t pstr = conv_pstr(c.ck, p->m16);
    if ((size_t)HT * p->WT * pstr + 2 * (size_t)c.bn * conv_wrs(c.ck) > 160 * 1024) continue;   // halo + weight ring
    *cfg = c;
    p->HT = HT;
    p->tiles_y = ocr_cdiv(d->oh, c.th);
    p->halo_bytes = (int)(HT * p->WT * pstr);
    p->n_tiles = d->cout / c.bn;
    p->br = BnRed{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    return OCR_OK;
  }
  return OCR_ERR_UNSUPPORTED;
}

}  // namespace

OCR_DIAG_READER(ocr_diag_read_conv, ocr_diag_conv)

// every entry point opens with it: the filled parameters p and tile cfg of d, or fill_params' code
#define OCR_CONV_FILL(d, p, cfg)                        \
  ConvP p;                                              \
  TileCfg cfg;                                          \
  do {                                                  \
    const int rc_ = fill_params(d, &p, &cfg);           \
    if (rc_ != OCR_OK) return rc_;                      \
  } while (0)

static BnRed bn_red(const void* bn_y, const void* bn_scale, const void* bn_shift, const void* bn_mean,
                    const void* bn_invstd, int bn_relu) {
  return BnRed{static_cast<const half_t*>(bn_y), static_cast<const float*>(bn_scale), static_cast<const float*>(bn_shift),
               static_cast<const float*>(bn_mean), static_cast<const float*>(bn_invstd), bn_relu};
}

extern "C" int ocr_conv2d_num_mtiles(const ocr_conv_desc* d) {
  if (!d) return OCR_ERR_INVALID_ARG;
  ConvP p;
  TileCfg c;
  if (fill_params(d, &p, &c) != OCR_OK)            // (no kernel takes d: the row count of its pixel tiles, as ever)
    return conv_is_pw(d) ? (int)(((long long)d->n * d->oh * d->ow + 255) / 256)
                         : d->n * ocr_cdiv(d->ow, TILE_W) * ocr_cdiv(d->oh, TILE_H);
  const ConvPlan s = conv_plan(p, c);
  return s.status == OCR_OK ? s.rows : s.status;
}

// The name is the NOMINAL tile of the family, which is not always the launched one: pointwise cin = 64 launches
// without global operands in the epilogue run conv_pw_kernel<128,2> under the name <256,4>, and a bottleneck tail
// (which a descriptor cannot express) moves the 4-wave families' shapes to conv_igemm_kernel.
extern "C" int ocr_conv2d_variant(const ocr_conv_desc* d, char* out, size_t cap) {
  OCR_CONV_FILL(d, p, c);
  OCR_CHECK_ARG(out && cap > 0);
  const ConvPlan s = conv_plan(p, c);
  switch (s.family) {
    case ConvPlan::PW:
    case ConvPlan::PWX: snprintf(out, cap, "conv_pw_kernel<%d,%d>", c.bn, c.bn == 256 ? 4 : c.bn == 128 ? 2 : 1); break;
    case ConvPlan::W4S: snprintf(out, cap, "conv3x3_w4s_kernel<%d>", s.bn); break;
    case ConvPlan::W4: snprintf(out, cap, "conv3x3_w4_kernel"); break;
    case ConvPlan::C64: snprintf(out, cap, "conv_c64_persist_kernel<64>"); break;
    case ConvPlan::IGEMM:
      snprintf(out, cap, "conv_igemm_kernel<%d,%d,%d,%d,%d>", c.bn, c.ck, c.bn == 256 ? 4 : c.bn == 32 ? 1 : 2, p.m16, c.th);
  }
  return OCR_OK;
}

extern "C" int ocr_conv2d_f16(const ocr_conv_desc* d, const void* x, const void* w_kc,
                              const void* bias, void* y, void* stats, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(x && w_kc && y);
  OCR_CHECK_ARG(!(d->flags & OCR_CONV_BIAS) || bias);
  OCR_CHECK_ARG(!(d->flags & OCR_CONV_STATS) || stats);
  return dispatch(p, conv_plan(p, cfg), x, w_kc, bias, y, stats, static_cast<hipStream_t>(stream));
}

extern "C" int ocr_conv2d_bnred_f16(const ocr_conv_desc* d, const void* x, const void* w_kc, void* y,
                                    void* partial, const void* bn_y, const void* bn_scale,
                                    const void* bn_shift, const void* bn_mean, const void* bn_invstd,
                                    int bn_relu, int store_masked, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(x && w_kc && y && partial && bn_y && bn_scale && bn_shift && bn_mean && bn_invstd);
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_BIAS | OCR_CONV_RELU)));
  p.flags |= OCR_CONV_STATS;
  p.br = bn_red(bn_y, bn_scale, bn_shift, bn_mean, bn_invstd, bn_relu);
  p.br.store_dz = store_masked;
  return dispatch(p, conv_plan(p, cfg), x, w_kc, nullptr, y, partial, static_cast<hipStream_t>(stream));
}

// the two entry points below exist for the persistent kernel's 64 -> 64 launches only
static bool first_ok(const ConvP& p, const ConvPlan& s) { return s.family == ConvPlan::C64 && p.cout == 64; }

// ocr_conv2d_bnred_f16 for the convolution that consumes conv1_1's activation (conv1_2 of nets/vgg.py:17): the fused
// BN-backward sums need conv1_1's y, and instead of reading 128 B per pixel the epilogue evaluates it again from the
// 8-byte image pixels (BnRed::first_x4).  conv_c64_persist_kernel only (64 -> 64 channels, the shape of that layer).
extern "C" int ocr_conv2d_bnred_first_f16(const ocr_conv_desc* d, const void* x, const void* w_kc, void* y,
                                          void* partial, const void* x4, const void* w_first,
                                          const void* bn_scale, const void* bn_shift, const void* bn_mean,
                                          const void* bn_invstd, int bn_relu, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(x && w_kc && y && partial && x4 && w_first && bn_scale && bn_shift && bn_mean && bn_invstd);
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_BIAS | OCR_CONV_RELU | OCR_CONV_ACCUM_F16)));
  p.flags |= OCR_CONV_STATS;
  p.br = bn_red(nullptr, bn_scale, bn_shift, bn_mean, bn_invstd, bn_relu);
  p.br.first_x4 = static_cast<const half_t*>(x4);
  p.br.first_wf = static_cast<const half_t*>(w_first);
  const ConvPlan s = conv_plan(p, cfg);
  if (!first_ok(p, s)) return OCR_ERR_UNSUPPORTED;
  return dispatch(p, s, x, w_kc, nullptr, y, partial, static_cast<hipStream_t>(stream));
}

// ocr_conv2d_bnred_first_f16 that does not store the gradient but the sums conv1_1's weight gradient is made of
// (epilogue mode 7 of conv_c64_persist_kernel; the finishing step is ocr_conv2d_first_wgrad_sums_f32, conv_first.hip).
extern "C" int ocr_conv2d_bnred_first_wgrad_blocks(const ocr_conv_desc* d) {
  ConvP p;
  TileCfg cfg;
  if (fill_params(d, &p, &cfg) != OCR_OK) return -1;
  const ConvPlan s = conv_plan(p, cfg);
  return first_ok(p, s) && s.status == OCR_OK ? (int)s.grid : -1;
}

extern "C" int ocr_conv2d_bnred_first_wgrad_f16(const ocr_conv_desc* d, const void* x, const void* w_kc, void* partial,
                                                const void* x4, const void* w_first, const void* bn_scale,
                                                const void* bn_shift, const void* bn_mean, const void* bn_invstd,
                                                int bn_relu, void* s1_blocks, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(x && w_kc && partial && x4 && w_first && bn_scale && bn_shift && bn_mean && bn_invstd && s1_blocks);
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_BIAS | OCR_CONV_RELU | OCR_CONV_ACCUM_F16)));
  p.flags |= OCR_CONV_STATS;
  p.br = bn_red(nullptr, bn_scale, bn_shift, bn_mean, bn_invstd, bn_relu);
  p.br.first_x4 = static_cast<const half_t*>(x4);
  p.br.first_wf = static_cast<const half_t*>(w_first);
  p.br.first_s1 = static_cast<float*>(s1_blocks);
  const ConvPlan s = conv_plan(p, cfg);
  if (!first_ok(p, s)) return OCR_ERR_UNSUPPORTED;
  return dispatch(p, s, x, w_kc, nullptr, nullptr, partial, static_cast<hipStream_t>(stream));
}

// 1x1 convolution whose input is the previous bottleneck's output relu(bn(conv3) + shortcut), computed while the
// operand is loaded; x_out (and mask_bits) receive that output.  y = conv(x_out) with the usual BN partial sums
// (OCR_CONV_STATS) of the convolution itself.  nets/resnet_v1.py:96-107.
extern "C" int ocr_conv2d_pw_bnaddrelu_f16(const ocr_conv_desc* d, const void* prev_y, const void* prev_scale,
                                           const void* prev_shift, const void* shortcut, const void* sc_scale,
                                           const void* sc_shift, void* x_out, void* mask_bits, const void* w_kc,
                                           void* y, void* stats, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(prev_y && prev_scale && prev_shift && shortcut && x_out && w_kc && y);
  OCR_CHECK_ARG((sc_scale == nullptr) == (sc_shift == nullptr));
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_BIAS | OCR_CONV_RELU | OCR_CONV_ACCUM_F16)));
  OCR_CHECK_ARG(!(d->flags & OCR_CONV_STATS) || stats);
  PwX t{static_cast<const half_t*>(prev_y), static_cast<const half_t*>(shortcut), static_cast<const float*>(prev_scale),
        static_cast<const float*>(sc_scale), static_cast<const float*>(prev_shift), static_cast<const float*>(sc_shift),
        static_cast<half_t*>(x_out), static_cast<unsigned char*>(mask_bits)};
  return dispatch_pwx<1>(p, conv_plan(p, cfg, false, 1), t, w_kc, y, stats, static_cast<hipStream_t>(stream));
}

// 1x1 convolution whose input x = relu(prev_y * prev_scale + prev_shift) — the batch norm + ReLU of the layer before it —
// is computed while it is loaded and written to x_out (the weight gradient reads it): replaces ocr_bn_relu_f16 +
// ocr_conv2d_f16 and one full read of x.
extern "C" int ocr_conv2d_pw_bnrelu_f16(const ocr_conv_desc* d, const void* prev_y, const void* prev_scale,
                                        const void* prev_shift, void* x_out, const void* w_kc, void* y, void* stats,
                                        void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(prev_y && prev_scale && prev_shift && x_out && w_kc && y);
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_BIAS | OCR_CONV_RELU | OCR_CONV_ACCUM_F16)));
  OCR_CHECK_ARG(!(d->flags & OCR_CONV_STATS) || stats);
  PwX t{static_cast<const half_t*>(prev_y), nullptr, static_cast<const float*>(prev_scale), nullptr,
        static_cast<const float*>(prev_shift), nullptr, static_cast<half_t*>(x_out), nullptr};
  return dispatch_pwx<3>(p, conv_plan(p, cfg, false, 3), t, w_kc, y, stats, static_cast<hipStream_t>(stream));
}

// Input-gradient 1x1 convolution whose operand is the batch-norm backward apply dy = A*dz + B*bn_y_in + C of the
// layer above (coefficients: ocr_bn_bwd_coefficients), computed while loading; dy_out receives it (the weight
// gradient reads it next).  The epilogue carries the fused BN-backward reduction of the layer BELOW as
// ocr_conv2d_bnred_f16 does (bn_* arguments: that layer).
extern "C" int ocr_conv2d_pw_bnbwd_bnred_f16(const ocr_conv_desc* d, const void* dz, const void* y_above,
                                             const void* coef_a, const void* coef_b, const void* coef_c, void* dy_out,
                                             const void* w_kc, void* dx, void* partial, const void* bn_y,
                                             const void* bn_scale, const void* bn_shift, const void* bn_mean,
                                             const void* bn_invstd, int bn_relu, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(dz && y_above && coef_a && coef_b && coef_c && dy_out && w_kc && dx);
  OCR_CHECK_ARG(partial && bn_y && bn_scale && bn_shift && bn_mean && bn_invstd);
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_BIAS | OCR_CONV_RELU | OCR_CONV_ACCUM_F16)));
  p.flags |= OCR_CONV_STATS;
  p.br = bn_red(bn_y, bn_scale, bn_shift, bn_mean, bn_invstd, bn_relu);
  PwX t{static_cast<const half_t*>(dz), static_cast<const half_t*>(y_above), static_cast<const float*>(coef_a),
        static_cast<const float*>(coef_b), static_cast<const float*>(coef_c), nullptr, static_cast<half_t*>(dy_out),
        nullptr};
  return dispatch_pwx<2>(p, conv_plan(p, cfg, false, 2), t, w_kc, dx, partial, static_cast<hipStream_t>(stream));
}

// conv + bias + ReLU + 2x2/2 max-pool in one kernel for 64 -> 64 channel 3x3 layers (PixelLink's conv1_2 and the same
// layer at 1024^2 inference): only the pooled activation and its first-max positions are written.
extern "C" int ocr_conv2d_relu_pool_f16(const ocr_conv_desc* d, const void* x, const void* w_kc, const void* bias,
                                        void* pooled, void* argmax_u8, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(x && w_kc && pooled);
  OCR_CHECK_ARG(!(d->flags & OCR_CONV_BIAS) || bias);
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_STATS | OCR_CONV_ACCUM_F16)));
  p.pool_out = static_cast<half_t*>(pooled);
  p.pool_idx = static_cast<unsigned char*>(argmax_u8);
  const ConvPlan s = conv_plan(p, cfg, true);
  if (s.family != ConvPlan::C64) return OCR_ERR_UNSUPPORTED;
  return dispatch(p, s, x, w_kc, bias, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

// q = (P * m) >> (31 + l) == P / d for every P < 2^31 (round-up method: m = ceil(2^(31+l) / d), l = ceil(log2 d))
static void magic31(unsigned d, unsigned long long* m, int* l) {
  int k = 0;
  while ((1ull << k) < d) ++k;
  *l = k;
  *m = ((1ull << (31 + k)) + d - 1) / d;
}

// the bottleneck tail of ocr_conv2d_bnred_tail_f16 in p (its arguments checked by the caller)
static int set_tail(ConvP& p, const ocr_conv_desc* d, const void* bn_y, const void* bn_mean, const void* bn_invstd,
                    const void* tail_out, const void* tail_mask_bits, const void* sub_grad) {
  p.flags |= OCR_CONV_STATS;
  p.br = bn_red(bn_y, nullptr, nullptr, bn_mean, bn_invstd, 0);
  p.br.mask = static_cast<const half_t*>(tail_mask_bits ? nullptr : tail_out);
  p.br.mask_bits = static_cast<const unsigned char*>(tail_mask_bits);
  if (sub_grad != nullptr) {
    OCR_CHECK_SHAPE((long long)d->n * d->oh * d->ow < (1ll << 31));
    p.br.sub = static_cast<const half_t*>(sub_grad);
    p.br.sub_h = d->oh;
    p.br.sub_w = d->ow;
    magic31((unsigned)(d->oh * d->ow), &p.br.sub_m_hw, &p.br.sub_l_hw);
    magic31((unsigned)d->ow, &p.br.sub_m_w, &p.br.sub_l_w);
  }
  return OCR_OK;
}

extern "C" int ocr_conv2d_bnred_tail_f16(const ocr_conv_desc* d, const void* x, const void* w_kc, void* y,
                                         void* partial, const void* bn_y, const void* bn_mean,
                                         const void* bn_invstd, const void* tail_out, const void* tail_mask_bits,
                                         const void* sub_grad, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(x && w_kc && y && partial && bn_y && bn_mean && bn_invstd && (tail_out || tail_mask_bits));
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_BIAS | OCR_CONV_RELU)));
  if (const int rc = set_tail(p, d, bn_y, bn_mean, bn_invstd, tail_out, tail_mask_bits, sub_grad)) return rc;
  return dispatch(p, conv_plan(p, cfg), x, w_kc, nullptr, y, partial, static_cast<hipStream_t>(stream));
}

// ocr_conv2d_pw_bnbwd_bnred_f16's loader (the BN-backward apply of the layer ABOVE computed on the operand rows, optionally
// with that layer's ReLU mask) in front of the other epilogues of the pointwise kernel: plain store, accumulate
// (OCR_CONV_ACCUM_F16 in d->flags), or the bottleneck tail of ocr_conv2d_bnred_tail_f16 (bn_y ... sub_grad as there; all
// null: no tail, `partial` unused).
extern "C" int ocr_conv2d_pw_bnbwd_tail_f16(const ocr_conv_desc* d, const void* dz, const void* y_above, const void* coef_a,
                                            const void* coef_b, const void* coef_c, const void* relu_shift, void* dy_out,
                                            const void* w_kc, void* dx, void* partial, const void* bn_y,
                                            const void* bn_mean, const void* bn_invstd, const void* tail_out,
                                            const void* tail_mask_bits, const void* sub_grad, void* stream) {
  OCR_CONV_FILL(d, p, cfg);
  OCR_CHECK_ARG(dz && y_above && coef_a && coef_b && coef_c && dy_out && w_kc && dx);
  OCR_CHECK_ARG(!(d->flags & (OCR_CONV_BIAS | OCR_CONV_RELU | OCR_CONV_STATS)));
  const bool tail = bn_y != nullptr;
  if (tail) {
    OCR_CHECK_ARG(partial && bn_mean && bn_invstd && (tail_out || tail_mask_bits));
    if (const int rc = set_tail(p, d, bn_y, bn_mean, bn_invstd, tail_out, tail_mask_bits, sub_grad)) return rc;
  } else {
    OCR_CHECK_ARG(!bn_mean && !bn_invstd && !tail_out && !tail_mask_bits && !sub_grad);
  }
  PwX t{static_cast<const half_t*>(dz), static_cast<const half_t*>(y_above), static_cast<const float*>(coef_a),
        static_cast<const float*>(coef_b), static_cast<const float*>(coef_c), static_cast<const float*>(relu_shift),
        static_cast<half_t*>(dy_out), nullptr};
  return dispatch_pwx<2>(p, conv_plan(p, cfg, false, 2), t, w_kc, dx, tail ? partial : nullptr,
                         static_cast<hipStream_t>(stream));
}

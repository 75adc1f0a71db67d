/*
 * ocr_decode_grid.h — part of the C ABI of libocr_hip.so, included by ocr_hip.h (include that one): the link (PixelLink)
 * decode over a GRID of G (pixel threshold, link threshold) pairs in one launch sequence (csrc/decode_grid.hip), so that
 * an evaluation can search the two decode thresholds behind ONE forward pass.  Conventions and status codes as in
 * ocr_hip.h; OCR_ABI_VERSION is unchanged, the entries are new.
 *
 * SLICES.  A slice is b = g * n + i: grid point g of G, image i of n.  Slice b reads the maps of image i = b mod n — the
 * maps are never replicated — and every output has G * n leading rows.  The stages behind these two
 * (ocr_min_area_rects, ocr_link_boxes, ocr_eval_collect) take a batch of any size and run unchanged on N = G * n; the
 * matchers run once per grid point on that point's n contiguous slices.
 */
#ifndef OCR_DECODE_GRID_H_
#define OCR_DECODE_GRID_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * ocr_link_cc_grid: ocr_link_cc for every grid point at once.  pixel_score f32 [n][h][w]; link_score addressed as
 * ocr_link_cc addresses it (element ((d * n + i) * h * w + pixel) * link_elem_stride + link_elem_offset over
 * [8][n][h][w]); pixel_thresh / link_thresh: G floats each IN HOST MEMORY, read before the entry returns and carried to
 * the kernels as a table in their arguments (no device upload, nothing to keep alive).  Outputs: labels int32
 * [G*n][h][w], ncomp int32 [G*n], comps int32 [G*n][max_comps][2] = (smallest pixel index, size).
 *
 * Slice b = g * n + i equals, bit for bit, what ocr_link_cc writes for image i with (pixel_thresh[g], link_thresh[g]):
 * the same strict > comparisons in f32 (NaN is never above a threshold), links of INTERIOR pixels only, components of
 * more than min_size pixels, dense ids ascending with the smallest pixel index of each component, ncomp the true count,
 * and rows of comps at or beyond min(ncomp, max_comps) not written.  The structure is ocr_link_cc's tiled union-find with
 * the slice in the launch grid: an init pass that reads a pixel's score once and decides all G slices from it, 32x32
 * tiles united in LDS, the tile-border edges, then root / count / assign / relabel — seven launches whatever G is.
 * Workspace: ocr_link_cc_grid_workspace(G, n, h, w) bytes, G times ocr_link_cc's (0 for a non-positive extent).
 *
 * Status: OCR_ERR_INVALID_ARG for a null pointer, a non-positive G, n, h, w or max_comps, or a bad link stride / offset;
 * OCR_ERR_UNSUPPORTED for G > 65 (64 grid points and a base pair), G * n > 65535, h or w < 3, or G * n * h * w >
 * INT32_MAX; OCR_ERR_WORKSPACE for ws_bytes below the workspace size.  Nothing is written on error.
 * ------------------------------------------------------------------------- */
size_t ocr_link_cc_grid_workspace(int G, int n, int h, int w);
int ocr_link_cc_grid(const void* pixel_score, const void* link_score, int link_elem_stride, int link_elem_offset, int n,
                     int h, int w, int G, const float* pixel_thresh_host, const float* link_thresh_host, int min_size,
                     void* labels_i32, void* ncomp_i32, void* comps_i32, int max_comps, void* workspace, size_t ws_bytes,
                     void* stream);

/* ------------------------------------------------------------------------- *
 * ocr_component_scores_grid: ocr_component_scores for labels int32 [G*n][h][w] (ocr_link_cc_grid's) against pixel_score
 * f32 [n][h][w], slice b reading map b mod n; ncomp int32 [G*n] -> comp_score f32 [G*n][max_comps].  Bit-equal per slice
 * to ocr_component_scores: q = (uint32)rintf(clamp(s, 0, 1) * 2^24) with NaN -> 0, 64-bit integer sums of q and of the
 * pixel count, mean = f32(f64(sum) / f64(count) / 16777216.0); an id outside 1..max_comps is ignored, an id without
 * pixels and the rows at or beyond min(ncomp, max_comps) score 0.  Workspace: ocr_component_scores_grid_workspace(G, n,
 * max_comps) bytes.  Status: OCR_ERR_INVALID_ARG for a null pointer or a non-positive extent; OCR_ERR_UNSUPPORTED for
 * G > 65, G * n or max_comps beyond 65535, or a map side beyond 32768; OCR_ERR_WORKSPACE; nothing is written on error.
 * ------------------------------------------------------------------------- */
size_t ocr_component_scores_grid_workspace(int G, int n, int max_comps);
int ocr_component_scores_grid(const void* labels_i32, const void* pixel_score_f32, const void* ncomp_i32, int G, int n, int h,
                              int w, int max_comps, void* comp_score_f32, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OCR_DECODE_GRID_H_ */

/*
 * ocr_map_fuse.h — part of the C ABI of libocr_hip.so, included by ocr_hip.h (include that one): multi-scale and flip
 * testing for the link (PixelLink) geometry by SCORE-MAP fusion on the device (csrc/map_fuse.hip).  A segmentation
 * detector does not fuse boxes: each pass's pixel and link probabilities are resampled onto one fusion grid and averaged,
 * and the link decode (ocr_link_cc -> ocr_min_area_rects -> ocr_component_scores -> ocr_link_boxes) runs once on the
 * result.  Conventions and status codes as in ocr_hip.h; OCR_ABI_VERSION is unchanged, the entry is new.  f32 in memory,
 * every operation below rounded to f32 with no contraction, no atomics.
 */
#ifndef OCR_MAP_FUSE_H_
#define OCR_MAP_FUSE_H_

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * ocr_link_map_accumulate: adds ONE forward pass of a batch of n images to the fusion-grid accumulator.  It reads the
 * LOGITS of PixelLinkNet — pixel_logits f32 [n][hs][ws][2] (8-byte aligned), link_logits f32 [n][hs][ws][16] (16-byte
 * aligned, a pixel's row is read with 16-byte loads) — so it stands in for ocr_softmax_pairs, ocr_link_softmax_stack and
 * the copy of index 1 at once: per pass the logits are read once and the accumulator is read (first == 0) and written
 * once.  acc f32 [9][n][hf][wf]: plane 0 is P(text), plane 1 + d is P(link d positive), index 1 of pair d in
 * ocr_link_cc's direction order (left, left_down, left_up, right, right_down, right_up, up, down).  acc[0] is ocr_link_cc's
 * pixel_score [n][hf][wf] and acc + n*hf*wf its link_score [8][n][hf][wf] with element stride 1, offset 0: no copy.
 *
 * Per cell (y, x) of the fusion grid and per plane:
 *   ry = (float)hs / (float)hf;  sy = ((float)y + 0.5f) * ry - 0.5f;  y0 = floorf(sy);  ty = sy - y0
 *   y0 < 0: y0 = 0, ty = 0;   y0 >= hs - 1: y0 = hs - 1, ty = 0;   y1 = min(y0 + 1, hs - 1)
 *   x likewise with ws, wf, tx — the half-pixel-centre rule of cv2.resize on float data, clamped at the edges.
 *   flip != 0 (the pass saw the images mirrored left to right): the taps are read at columns ws - 1 - x0 and ws - 1 - x1,
 *   and link plane d reads logit pair perm[d], the direction with the opposite dx and the same dy (left <-> right,
 *   left_down <-> right_down, left_up <-> right_up; up and down stay), derived from the direction table at compile time.
 *   Probability at a tap, ocr_softmax_pairs' expression for index 1, operation for operation:
 *     mx = fmaxf(a, b); ea = expf(a - mx); eb = expf(b - mx); p = eb / (ea + eb)
 *   top = (tx == 0) ? p00 : p00 * (1 - tx) + p01 * tx;  bot likewise on row y1;  v = (ty == 0) ? top : top * (1 - ty) + bot * ty
 *   A tap of zero weight is never used: a NaN logit reaches only the cells that really sample it.
 *   acc = first ? weight * v : acc + weight * v
 * One thread owns a cell for the whole launch (grid-stride loop over a capped grid): the result is bit-reproducible and
 * independent of scheduling.  The host passes NORMALISED weights, float32(w_s / sum w) formed in float64; there is no
 * finishing pass, so the first pass of a batch has first != 0 and acc needs no zeroing.
 *
 * Status: OCR_ERR_INVALID_ARG for a null pointer, a misaligned logits pointer, a non-positive n, hs, ws, hf or wf, or a
 * non-finite or non-positive weight; OCR_ERR_UNSUPPORTED for n > 65535 or n*hf*wf or n*hs*ws above INT32_MAX; nothing is
 * written on error.
 *
 * BUILD-DEFINED (no published multi-scale PixelLink script is on any machine that built this and none is pinned by a
 * test): the sampling rule above; that PROBABILITIES are averaged, not logits; the weights; the mirrored direction
 * pairing.  Whether multi-scale or flip fusion raises the F-measure is unmeasured. */
int ocr_link_map_accumulate(const void* pixel_logits_f32, const void* link_logits_f32, int n, int hs, int ws, int flip,
                            float weight, int first, void* acc_f32, int hf, int wf, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OCR_MAP_FUSE_H_ */

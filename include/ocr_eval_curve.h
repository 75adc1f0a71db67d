/*
 * ocr_eval_curve.h — part of the C ABI of libocr_hip.so, included by ocr_hip.h (include that one): the score-threshold
 * sweep (precision / recall curve) and average precision of a held-out evaluation pass, counted on the device from what ONE
 * matching pass leaves there (csrc/eval_curve.hip).  Conventions and status codes as in ocr_hip.h; OCR_ABI_VERSION is
 * unchanged, the entries are new.
 */
#ifndef OCR_EVAL_CURVE_H_
#define OCR_EVAL_CURVE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * ocr_eval_curve_batch / ocr_eval_ic15_curve_batch: for n images in one call, without a host synchronisation, the counters
 * of T score thresholds from the outputs of ocr_eval_match_batch (tp, fp uint8 [n][max_d], ng, gignored uint8 [n][max_g]) /
 * ocr_eval_ic15_match_batch (det_match int32 [n][max_d], gt_match int32 [n][max_g], ng), together with ocr_eval_collect's
 * det_score f32 [n][max_d] and nd int32 [n], and thresholds f32 [T].  Counts outside [0, max_d] / [0, max_g] are clamped.
 * Integers and f32 compares only.  Status: OCR_ERR_INVALID_ARG for a null required pointer, a non-positive n, max_d or
 * max_g, or a pool given in part; OCR_ERR_UNSUPPORTED for max_d > 1024, max_g > 254, n > 65535 or T outside 1..64; nothing
 * is written on error.
 *
 * Both rules become one state per detection d of image i:
 *                 absent                              care, unmatched    care, matched     care ground truths
 *   raster        neither tp nor fp, or d >= nd       fp                 tp                g < ng with gignored == 0
 *   IC15          det_match == -2, or d >= nd         det_match == -1    det_match >= 0    g < ng with gt_match != -2
 * A detection is KEPT at threshold t iff d < nd and det_score[d] >= thresholds[t], compared in f32: a NaN score is never
 * kept, a NaN threshold keeps nothing.  Because the raster walk decides a detection from the detections before it, and
 * the IC15 walk restricted to a score prefix leaves exactly the full-list matches inside the prefix,
 * row t equals what the matcher gives on the list filtered by thresholds[t] — provided the list is in ocr_eval_collect's
 * order.
 *
 * curve int64 [T][4] is ADDED TO (integer atomics), so one buffer serves a whole pass: row t = {care ground truths,
 * matched kept detections, care unmatched kept detections, kept detections}, the slots of ocr_eval_match_batch's record
 * (precision = [1] / ([1] + [2]), recall = [1] / [0]).  unsorted int32 [1] is OR-ED INTO: non-zero if some image's scores
 * over d < nd are not non-increasing with the NaNs last (ocr_eval_collect's order, on which the prefix property and
 * ocr_eval_ap's search rest).  ocr_eval_curve_init zeroes the T rows, the flag and, when given, ap f64 [1].
 *
 * The AP pool rows of these n images (optional: all three NULL, nothing is kept): pool_score f32 [n][max_d] (the scores
 * of d < nd, NaN beyond), pool_cum int32 [n][max_d][2] (inclusive prefix counts, in d order, of the care and of the
 * matched detections; a NaN-scored detection counts as absent), pool_nd int32 [n] (the clamped nd).  The caller passes
 * pointers offset to image_sequence * max_d inside a pass-wide pool, so the host never needs a device count.
 *
 * ocr_eval_ap: once at the end of a pass, over the pool of n_img images.  A slot (i, d) is image sequence i, detection d <
 * pool_nd[i]; (j, e) is BEFORE (i, d) when score(j, e) > score(i, d), or the scores are equal and (j, e) is
 * lexicographically smaller.  With M = 1 + the matched slots before a matched slot, C = 1 + the care slots before it,
 *   ap f64 [1] = (1 / G) * sum over the matched slots of M / C,   G = record[0] (int64, read on the device); G <= 0: 0.
 * M and C are integers; every term is one IEEE f64 division, the terms are summed over a FIXED partition (256 consecutive
 * slots per partial, the partials strided over 256 accumulators) and fixed trees, so the result does not depend on
 * scheduling; one more division by G.  Status: OCR_ERR_INVALID_ARG for a null pointer or a non-positive extent,
 * OCR_ERR_UNSUPPORTED for max_d > 1024 or n_img > 65535, OCR_ERR_WORKSPACE for ws_bytes below ocr_eval_ap_workspace(n_img,
 * max_d) (the partial sums; 0 for a non-positive extent); nothing is written on error.
 * BUILD-DEFINED (the official ICDAR script is on no machine that built this and is pinned by no test; this is its
 * compute_ap over the pooled confidences of the care detections as remembered): the tie rule above, a NaN-scored
 * detection is outside AP (and never kept by the curve), the detection order is ocr_eval_collect's. */
int ocr_eval_curve_init(void* curve_i64, int T, void* unsorted_i32, void* ap_f64, void* stream);
int ocr_eval_curve_batch(const void* tp_u8, const void* fp_u8, const void* det_score_f32, const void* nd_i32,
                         const void* ng_i32, const void* gignored_u8, const void* thresholds_f32, int n, int max_d, int max_g,
                         int T, void* curve_i64, void* unsorted_i32, void* pool_score_f32, void* pool_cum_i32,
                         void* pool_nd_i32, void* stream);
int ocr_eval_ic15_curve_batch(const void* det_match_i32, const void* gt_match_i32, const void* det_score_f32,
                              const void* nd_i32, const void* ng_i32, const void* thresholds_f32, int n, int max_d, int max_g,
                              int T, void* curve_i64, void* unsorted_i32, void* pool_score_f32, void* pool_cum_i32,
                              void* pool_nd_i32, void* stream);
size_t ocr_eval_ap_workspace(int n_img, int max_d);
int ocr_eval_ap(const void* pool_score_f32, const void* pool_cum_i32, const void* pool_nd_i32, int n_img, int max_d,
                const void* record_i64, void* ap_f64, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OCR_EVAL_CURVE_H_ */

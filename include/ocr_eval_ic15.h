/*
 * ocr_eval_ic15.h — part of the C ABI of libocr_hip.so, included by ocr_hip.h (include that one): held-out evaluation by
 * the ICDAR-2015 Task-1 localisation protocol on the device (csrc/eval_ic15.hip).  Conventions and status codes as in
 * ocr_hip.h; OCR_ABI_VERSION is unchanged, the entries are new.
 */
#ifndef OCR_EVAL_IC15_H_
#define OCR_EVAL_IC15_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * ocr_eval_ic15_match_batch: the official ICDAR-2015 matching (polygon IoU, don't-care regions) for n images in one call,
 * without a host synchronisation.  f64 and integers.  Operands as ocr_eval_match_batch: dets int32 [n][max_d][4][2] with
 * nd [n] rows in ocr_eval_collect's order, gts int32 [n][max_g][4][2] with ng [n] rows, gdontcare u8 [n][max_g] (the `###`
 * transcriptions); counts outside [0, max_d] / [0, max_g] are clamped, coordinates to |c| <= 2^22.  Status: OCR_ERR_INVALID_ARG
 * for a null required pointer or a non-positive extent, OCR_ERR_UNSUPPORTED for max_d > 1024, max_g > 254 or n > 65535,
 * OCR_ERR_WORKSPACE for ws_bytes below ocr_eval_ic15_workspace; nothing is written on error.
 *
 * Polygons.  A quad is taken counter-clockwise by the sign of its integer shoelace sum s (either orientation is
 * accepted); area = |s| / 2, exact in f64.  Its kind is the number of negative turns (integer cross products of
 * consecutive edges) after that: 0 convex, 1 one reflex vertex, 2 or more a bow-tie; s = 0 with fewer than 2 negative
 * turns is an empty polygon.  A bow-tie or empty polygon has intersection 0 with everything.  area(det and gt) is the sum
 * of two Sutherland-Hodgman clips of the CONVEX one of the two against the triangles (v0 v1 v2), (v0 v2 v3) of the other,
 * v0 its reflex vertex if it has one (a triangle of no positive area is skipped); reflex against reflex is outside the
 * contract and gives 0.  Inside tests of input vertices are exact (integers below 2^47 in f64).  Pairs whose axis-aligned
 * bounding boxes are disjoint are 0 without clipping.
 *
 * Per image, with prec(d, g) = area(d and g) / area(d) (0 for area(d) = 0) and
 * iou(g, d) = area(g and d) / (area(g) + area(d) - area(g and d)) (0 for a denominator of 0), IEEE f64 divisions:
 *   a detection d is DON'T-CARE if some g with gdontcare[g] has prec(d, g) > area_prec_thr
 *   for g ascending, g neither don't-care nor a bow-tie: the FIRST d ascending that is unmatched, not don't-care and has
 *   iou(g, d) > iou_thr (strict) is matched with g
 * det_match int32 [n][max_d]: the ground truth index, -1 unmatched, -2 don't-care; -1 at and beyond nd[i].
 * gt_match int32 [n][max_g]: the detection index, -1 unmatched, -2 don't-care or bow-tie; -1 at and beyond ng[i].
 * inter_f64 (optional, NULL: not exported): area(g and d) f64 [n][max_g][max_d] of the pairs g < ng[i], d < nd[i]; other
 * entries are not written.  record int64 [4] = {ground truths neither don't-care nor bow-tie, matched, detections not
 * don't-care - matched, detections before the don't-care filter} is ADDED TO (integer atomics), the slots of
 * ocr_eval_match_batch's record: ocr_eval_record_init zeroes it, precision = [1] / ([1] + [2]), recall = [1] / [0].
 * BUILD-DEFINED (the official script is pinned by no test): the detection order is ocr_eval_collect's (the script reads
 * the submission file's), either orientation is accepted (the script rejects counter-clockwise input), a bow-tie meets
 * nothing.  Workspace: ocr_eval_ic15_workspace(n, max_d, max_g) bytes (0 for a non-positive extent): the pair areas,
 * polygon areas, normalised polygons and kinds. */
size_t ocr_eval_ic15_workspace(int n, int max_d, int max_g);
int ocr_eval_ic15_match_batch(const void* dets_i32, const void* nd_i32, const void* gts_i32, const void* ng_i32,
                              const void* gdontcare_u8, int n, int max_d, int max_g, double iou_thr, double area_prec_thr,
                              void* det_match_i32, void* gt_match_i32, void* inter_f64, void* record_i64, void* workspace,
                              size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OCR_EVAL_IC15_H_ */

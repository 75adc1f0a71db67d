/*
 * ocr_multiscale.h — part of the C ABI of libocr_hip.so, included by ocr_hip.h (include that one): multi-scale RBOX
 * inference on the device (csrc/multiscale.hip).  The per-scale results of ocr_rbox_decode -> ocr_lanms ->
 * ocr_quad_mean_score are pooled per image in original-image pixels, then fused across scales by score-ordered NMS,
 * optionally with a score-weighted vote.  Conventions and status codes as in ocr_hip.h; OCR_ABI_VERSION is unchanged, the
 * entries are new.  f32 and integers in memory; the vote sums in f64.  No atomic decides an order anywhere below.
 */
#ifndef OCR_MULTISCALE_H_
#define OCR_MULTISCALE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * ocr_ms_pool_append: appends ONE scale's detections of a batch of n images to the pooled lists.  Inputs are ocr_lanms's
 * outputs at this scale (merged f32 [n][max_k][9], keep_idx int32 [n][max_k], n_keep int32 [n]), passed uint8 [n][max_k] or
 * NULL (the box_thresh mask, per KEEP SLOT), mean f32 [n][max_k] (ocr_quad_mean_score of each keep slot on this scale's
 * score map), ratio f32 [n][2] = (ratio_w, ratio_h) of this scale, and scale_id.  Per image i, the keep slots j <
 * min(max(n_keep[i], 0), max_k) with passed NULL or passed[i][j] != 0 are appended after pool_count[i] IN KEEP ORDER
 * (compaction by ballot and prefix count): row = merged[i][keep_idx[i][j]] with x / ratio_w, y / ratio_h (the IEEE f32
 * division, as ocr_eval_collect's) and column 8 = mean[i][j]; pool_scale gets scale_id.  A slot whose row has a non-finite
 * divided coordinate or a non-finite mean — or whose keep index is outside [0, max_k) — is NOT appended and is counted
 * in pool_nonfinite[i].  pool f32 [n][max_pool][9], pool_scale int32 [n][max_pool]; nothing is written at or beyond row
 * max_pool.  pool_total[i] is advanced by the number of appendable rows and keeps the TRUE count; pool_count[i] =
 * min(pool_total[i], max_pool).  The host zeroes pool_count, pool_total and pool_nonfinite (int32 [n] each) once per batch,
 * then appends the scales in turn on one stream.  Status: OCR_ERR_INVALID_ARG for a null required pointer, a non-positive
 * n, max_k or max_pool, or a negative scale_id; OCR_ERR_UNSUPPORTED for n > 65535; nothing is written on error.
 *
 * ocr_quad_fuse: standard score-ordered NMS over each image's pooled list pool[i][:min(max(pool_count[i], 0), max_pool)],
 * mode 0 = suppress, mode 1 = vote.  Outputs in ocr_lanms's layout, so that ocr_eval_collect takes (fused, keep_idx,
 * n_keep) as they are: fused f32 [n][max_pool][9] (the pool rows below the count; rows at and beyond it are not written),
 * keep_idx int32 [n][max_pool] (pool indices of the kept quads in rank order; entries at and beyond n_keep are not
 * written), n_keep int32 [n], owner int32 [n][max_pool] (pool index of the kept quad that claimed row j, j itself if it is
 * kept, -1 at and beyond the count).  fused must not overlap pool.
 *   Rank: stable, by descending score (column 8); ties stay in pool order (scale-major as appended); NaN scores last.
 *   Sweep: in rank order, a row not yet claimed is kept and claims every later-ranked unclaimed row j with
 *   iou(kept, j) > iou_thresh, so owner[j] is the FIRST kept quad in rank order that overlaps j.  iou is ocr_lanms's
 *   convex-quad Sutherland-Hodgman clipper (oracle/lanms_oracle.c, operation for operation, the same device code),
 *   including the bounding-box early-out for iou_thresh >= 1e-3, whose verdict is the same.
 *   Mode 1, for each kept quad k: its members are the rows with owner == k, visited in rank order, k first.  Member j's
 *   four vertices are shifted cyclically by the r in {0,1,2,3} that minimises d_r = sum over v = 0..3 of
 *   (x_j[(v+r)%4] - x_k[v])^2 + (y_j[(v+r)%4] - y_k[v])^2, every term in f64 from the f32 values, added in that order
 *   starting from 0 (x term, then y term, vertex by vertex); ties take the smallest r.  With s_j the member's score and
 *   q_jc its shifted coordinates, W = sum (double)s_j and C_c = sum (double)s_j * (double)q_jc in visiting order, and
 *   fused[k][c] = (float)(C_c / W) for c < 8; W == 0 leaves the coordinates as they are.  The score stays s_k, so the kept
 *   list stays in descending score order; rows of non-kept quads equal the pool rows.
 * max_pool <= 4096 (64 mask words per row).  Status: OCR_ERR_INVALID_ARG for a null required pointer, a non-positive n or
 * max_pool, or a mode other than 0 / 1; OCR_ERR_UNSUPPORTED for max_pool > 4096 or n > 65535; OCR_ERR_WORKSPACE for
 * ws_bytes below ocr_quad_fuse_workspace(n, max_pool) (0 for a non-positive extent); nothing is written on error.  All
 * counts zero is OCR_OK with n_keep = 0.
 *
 * BUILD-DEFINED (no published multi-scale EAST script is on any machine that built this and none is pinned by a test;
 * parity with one is unpinned): the pooled score is the mean pixel score of the quad on its own scale's score map — a
 * value in [0, 1] that compares across scales, unlike LANMS's sum of pixel scores, which grows with the scale; the tie
 * order (pool order, scale-major); NaN scores last; the vote, its score weights and its cyclic vertex shift (which keeps
 * a member whose angle fell on the other side of the RBOX angle range from voting with rotated corners).  Whether the
 * vote improves the F-measure over plain suppression is unmeasured. */
int ocr_ms_pool_append(const void* merged_f32, const void* keep_idx_i32, const void* n_keep_i32, const void* passed_u8,
                       const void* mean_f32, const void* ratio_f32, int scale_id, int n, int max_k, int max_pool,
                       void* pool_f32, void* pool_scale_i32, void* pool_count_i32, void* pool_total_i32,
                       void* pool_nonfinite_i32, void* stream);
size_t ocr_quad_fuse_workspace(int n, int max_pool);
int ocr_quad_fuse(const void* pool_f32, const void* pool_count_i32, int n, int max_pool, float iou_thresh, int mode,
                  void* fused_f32, void* keep_idx_i32, void* n_keep_i32, void* owner_i32, void* workspace, size_t ws_bytes,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OCR_MULTISCALE_H_ */

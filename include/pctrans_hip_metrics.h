/* Validation metrics from label maps: entry points of libpctrans_hip.so.  Included by pctrans_hip.h (status codes, PCT_API,
 * conventions: there); include that header, not this one.  The caller (pctrans_amd/metrics.py: label_overlap, cvppp_metrics,
 * bbbc_metrics, MaskFormer.validation_metrics) takes them for dense device label maps; everything else keeps the table-based
 * torch formulation.
 *
 * Every metric here is a function of the contingency table of the two maps -- T[g, p] = pixels whose ground-truth value is the
 * g-th and whose predicted value is the p-th distinct value, in ascending order -- and of its row and column totals.
 * pct_label_overlap builds them in one pass over the maps with integer atomics, pct_label_metrics applies the rules,
 * O(G * P) integer work per image.  Side 0 is the prediction, side 1 the ground truth, in every [.., 2, ..] output.
 *
 * Compaction: a presence-bitmap pass of its own in csrc/label_metrics.hip, not the census of pctrans_hip_targets.h -- the
 * prediction is read through the foreground map and both maps are ranked in the same two launches, which the census (one
 * map, an ignore label, centre sums) would do in ten. */
#ifndef PCTRANS_HIP_METRICS_H
#define PCTRANS_HIP_METRICS_H

#ifdef __cplusplus
extern "C" {
#endif

#define PCT_METRICS_MAX_VALUES 512             /* distinct values per map and image, background included */
#define PCT_METRICS_WORKSPACE_PER_IMAGE 278528 /* bytes: 2 x 8 192 bitmap + 2 x 131 072 value -> index table */
#define PCT_METRICS_COLUMNS 12                 /* float64 columns of pct_label_metrics */
#define PCT_METRICS_STATUS_PRED_VALUE 1        /* a predicted label is negative, above 65 535 or not integral */
#define PCT_METRICS_STATUS_PRED_COUNT 2        /* more than PCT_METRICS_MAX_VALUES distinct predicted values */
#define PCT_METRICS_STATUS_GT_VALUE 4          /* the same for the ground truth */
#define PCT_METRICS_STATUS_GT_COUNT 8
#define PCT_METRICS_STATUS_EMPTY_PRED 16       /* no predicted value other than 0: the BBBC metrics the reference cannot form are 0 */
#define PCT_METRICS_STATUS_EMPTY_GT 32         /* no ground-truth value other than 0 */

/* ---- replaces the per-(label, label) mask sums the reference's metrics are built from: `(inLabel == i) * (gtLabel == j)` and its
 *      three np.sum per pair (lib/evaluate/CVPPP_evaluate.pyx: Dice, called from BestDice for every pair), `m & (pred == idx)`
 *      per (instance, prediction) pair (connectomics/inference/evaluation/metrics_bbbc.py: agg_jc_index), the per-instance
 *      masks and overlaps of get_fast_pq and np.unique / remap_label; and the trainer's device -> host copy of the label maps
 *      and `seg_outputs * fg` (connectomics/engine/trainer.py:398-450, 497-573) (csrc/label_metrics.hip) ----------------------
 *   pred, gt      [batch, height, width] dense, each of its own dtype: 0 uint8, 1 int16, 2 int32, 3 int64, 4 float32
 *   fg            [batch, height, width] uint8 or NULL: where it is 0 the predicted label reads as 0, whatever it holds
 *   workspace     device scratch, 16-byte aligned, batch * PCT_METRICS_WORKSPACE_PER_IMAGE bytes; need not be cleared
 *   values        [batch, 2, 512] int32 out: the distinct values of each map in ascending order, then zeros
 *   areas         [batch, 2, 512] int32 out: the pixel count of each value (the table's column and row sums), then zeros
 *   num           [batch, 2] int32 out: the number of distinct values (may exceed 512: the outputs then hold the first 512)
 *   range         [batch, 2, 2] int32 out: the lowest and highest raw value of each map
 *   table         [batch, 512, 512] int32 out, 16-byte aligned: T[n, g, p]; cleared by this call, zeros past num
 *   status        [batch] int32 out: 0, or PCT_METRICS_STATUS_* bits.  A pixel whose value on either side is outside the covered
 *                 values or past the first 512 is in no table cell; with a VALUE or COUNT bit set the caller is expected to
 *                 discard the outputs
 * Table pass: many workgroups per image, each over a contiguous run of pixels; a wave compares every lane's (g, p) pair with its
 * neighbour's and the head of each run of equal pairs adds the run's length in ONE integer atomic (a run that crosses a wave or
 * workgroup boundary is added in two).  Integer atomics only: two calls give the same bits.
 * Geometry: 0 < batch <= 65535, height * width < 2^24 (every count and product of two counts is exact in int64, every count in
 * fp64); anything else returns PCT_ERR_UNSUPPORTED before any launch.  Five launches on `stream`, no allocation, no host
 * synchronisation. */
PCT_API int pct_label_overlap(const void *pred, int pred_dtype, const void *gt, int gt_dtype, const uint8_t *fg, int batch,
                              int height, int width, void *workspace, int32_t *values, int32_t *areas, int32_t *num,
                              int32_t *range, int32_t *table, int32_t *status, void *stream);

/* ---- replaces SymmetricBestDice / BestDice / AbsDiffFGLabels (CVPPP_evaluate.pyx) and agg_jc_index, pixel_f1 and get_fast_pq at
 *      match_iou = 0.5 after remap_label (metrics_bbbc.py), per image (trainer.py:432-435, 539-546) ------------------------------
 *   values, areas, num, range, table   as pct_label_overlap left them
 *   metrics       [batch, 12] float64 out:
 *                   0 BD(pred, gt)  1 BD(gt, pred)  2 SBD = min of the two  3 |DiffFG|       -- CVPPP: background is the lowest
 *                     value PRESENT in each map; BD(a, b) = sum over the other values i of a, ascending, of max_j 2 |A_i n B_j| /
 *                     (|A_i| + |B_j|), divided by (max_a - min_a) on raw values (absent integers count in the divisor); 0 when
 *                     max_a = min_a
 *                   4 AJI  5 pixel F1  6 DQ  7 SQ  8 PQ                                      -- BBBC: value 0 is background whether
 *                     present or not, the other values are the instances in ascending order.  AJI follows the reference's
 *                     procedure: ground-truth instances in ascending order; a prediction offers (|m n p|, |m u p|) if not yet
 *                     taken and (0, |m|) if taken; the FIRST prediction of maximal quotient is taken (prediction 1 when all are
 *                     0, taken or not); the pixels of never-taken predictions are added to the union.  F1 = 2 TP / (2 TP + FP +
 *                     FN) of foreground pixels.  A pair is matched when its IoU is strictly above 1/2; DQ = tp / (tp + fp / 2
 *                     + fn / 2), SQ = sum IoU / (tp + 1e-6) in (ground-truth, prediction) order, PQ = DQ * SQ
 *                   9 .. 11 zero
 *                 Each ratio is one fp64 division of exact integers; each sum is taken in ascending label order.  A column
 *                 whose divisor is 0 (no prediction, no instance, no foreground at all) is 0: see the EMPTY status bits
 *   counts        [batch, 4] int32 out: tp, fp, fn of PQ and the number of predictions AJI took
 * One launch of one workgroup per image on `stream`, no allocation, no host synchronisation.  Geometry as pct_label_overlap
 * (0 < batch <= 65535, else PCT_ERR_UNSUPPORTED before the launch). */
PCT_API int pct_label_metrics(const int32_t *values, const int32_t *areas, const int32_t *num, const int32_t *range,
                              const int32_t *table, int batch, double *metrics, int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_METRICS_H */

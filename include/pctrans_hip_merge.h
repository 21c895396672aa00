/* Small-object merging of label maps: entry point of libpctrans_hip.so.  Included by pctrans_hip.h (status codes, PCT_API,
 * conventions: there); include that header, not this one.  The caller (pctrans_amd/label_merge.py: merge_small_objects,
 * MaskFormer.test_labels, MaskFormer.validation_metrics(merge=True)) takes it for dense device label maps; everything else keeps
 * the table-based torch formulation.
 *
 * `seg[seg == ids] = max_ids` of the reference moves ALL pixels of one current label to another, so the current map is
 * cur[original value] and a label's pixel count, row sum and column sum are additive under a merge.  One census of the image
 * (distinct values, ascending ranks, count / row sum / column sum per rank), a sequential procedure over at most 512 table rows
 * that reads at most window^2 pixels per visit, and one relabel pass replace the reference's per-label passes over the image. */
#ifndef PCTRANS_HIP_MERGE_H
#define PCTRANS_HIP_MERGE_H

#ifdef __cplusplus
extern "C" {
#endif

#define PCT_MERGE_MAX_VALUES 512             /* distinct values per image, background included */
#define PCT_MERGE_MAX_PASSES 8               /* (threshold, window) passes of one call */
#define PCT_MERGE_MAX_WINDOW 31              /* side of the crop around a centroid */
#define PCT_MERGE_WORKSPACE_PER_IMAGE 147456 /* bytes: 8 192 bitmap + 131 072 value -> rank table + 2 x 4 096 sums */
#define PCT_MERGE_STATUS_VALUE 1             /* a label is negative, above 65 535 or not integral */
#define PCT_MERGE_STATUS_COUNT 2             /* more than PCT_MERGE_MAX_VALUES distinct values */
#define PCT_MERGE_STATUS_TIE 4               /* a decision met a tie: the result follows this library's order (below) */

/* ---- replaces merge_func and its three merge_small_object passes, `seg_outputs * fg` and the device -> host copy of the label
 *      maps before them (connectomics/engine/trainer.py:744-777, called from test_cvppp :452-495; commented out at :423-424)
 *      (csrc/label_merge.hip) ---------------------------------------------------------------------------------------------------
 *   labels        [batch, height, width] dense, dtype: 0 uint8, 1 int16, 2 int32, 3 int64, 4 float32
 *   fg            [batch, height, width] uint8 or NULL: where it is 0 the label reads as 0, whatever it holds
 *   passes        [num_passes, 2] int32 in HOST memory, read before the launches: (threshold, window) of each pass in order,
 *                 1 <= num_passes <= 8, threshold >= 0, 1 <= window <= 31; the reference runs (5, 5), (20, 11), (50, 11)
 *   workspace     device scratch, 16-byte aligned, batch * PCT_MERGE_WORKSPACE_PER_IMAGE bytes; need not be cleared
 *   out           [batch, height, width] of the dtype of `labels`: the merged maps; every element is written
 *   values        [batch, 512] int32 out: the distinct values of the gated map in ascending order, then zeros
 *   final         [batch, 512] int32 out: the value that each of them carries after the last pass, then zeros
 *   areas_before  [batch, 512] int32 out: the pixel count of each value in the gated map
 *   areas_after   [batch, 512] int32 out: the pixel count of each value in `out` (0 for a value that was merged away)
 *   num           [batch] int32 out: the number of distinct values (may exceed 512: the outputs then hold the first 512)
 *   merges        [batch, 8] int32 out: merges made by each pass, zeros past num_passes
 *   status        [batch] int32 out: 0, or PCT_MERGE_STATUS_* bits.  With VALUE or COUNT set the caller is expected to discard
 *                 the image's outputs (an uncovered pixel is copied through the gate and takes part in nothing)
 * One pass (threshold, window): the snapshot is the values present in the current map with their pixel counts at the start of the
 * pass.  Every value whose snapshot count is <= threshold is visited in ascending order, value 0 like any other.  Its crop is
 * seg[r : r + window, c : c + window] with r = sum_rows // count - window // 2 from the LIVE sums and numpy's slice rules (a
 * negative start wraps: lo = max(start + n, 0); hi = min(start + window, n); empty when lo >= hi).  With fewer than three distinct
 * current values in the crop nothing happens.  Ordered by count descending, THEN VALUE ASCENDING: if 0 is first the target is the
 * best value other than 0 and the visited one, otherwise the first value (nothing happens if that is the visited one).  The
 * reference orders equal counts by numpy's unstable sort; a decision where that can matter -- 0 and the visited value share the
 * top count, or more than one eligible value has the best count -- sets TIE.
 * Geometry: 0 < batch <= 65535, height * width < 2^24 (every sum stays below 2^48, exact in 64-bit integers; integer atomics
 * only: two calls give the same bits); anything else returns PCT_ERR_UNSUPPORTED before any launch, a wrong `passes` or a null
 * pointer PCT_ERR_BAD_ARG.  Six launches on `stream`, no allocation, no host synchronisation, no floating point. */
PCT_API int pct_label_merge_small(const void *labels, int dtype, const uint8_t *fg, int batch, int height, int width,
                                  const int32_t *passes, int num_passes, void *workspace, void *out, int32_t *values,
                                  int32_t *final, int32_t *areas_before, int32_t *areas_after, int32_t *num, int32_t *merges,
                                  int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_MERGE_H */

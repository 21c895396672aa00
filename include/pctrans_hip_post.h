/* Opt-in instance post-processing entry points of libpctrans_hip.so.  Included by pctrans_hip.h (status codes, PCT_API,
 * conventions: there); include that header, not this one.  What is declared here is reached only when a caller switches it on
 * (MaskFormer.postprocess = "hip", PCT_POSTPROCESS): the default eval path keeps its torch formulation, so pctrans_hip.h keeps
 * exactly the entry points that have a default call site.
 *
 * Common to the five entries:
 *   dataset     0 = CVPPP (threshold 0.69, merge 0.5 / hard 0.6, NMS 0.72), 1 = BBBC (threshold 0.05, merge 0.15, soft mean);
 *               the constants of the reference's instance_inference (arch/maskformer.py:267-346).  Anything else: PCT_ERR_BAD_ARG.
 *   logits      [batch, num_query, h, w] fp32, or bf16 as raw bit patterns, contiguous
 *   bits        [batch, num_query, PW] 32-bit words, PW = 4 * ceil(height*width / 128), 16-byte aligned: bit (p % 32) of word
 *               (p / 32) is pixel p = y * width + x of the mask at (height, width); bits and words past height*width are zero
 *   areas       [batch, num_query] int32, the number of set pixels per plane
 *   labels      [batch, height, width] int16: 0 = background, k = the k-th surviving instance in ascending order of area
 * Geometry: num_query <= 512, 2*height*width + 1 < 2^24 (so that every area, intersection and dice operand is an integer that
 * fp32 holds exactly), height + width <= 8000 (the resize keeps 8 * (height + width) bytes of tap tables in LDS),
 * batch <= 65535; otherwise PCT_ERR_UNSUPPORTED and callers keep their torch formulation.  batch == 0 returns 0 and launches nothing; num_query == 0 writes all-zero labels.
 * Every call is a fixed sequence of launches on `stream`, with no host synchronisation, no allocation and no atomic operation:
 * it may be recorded into a HIP graph and replayed, and its results are bit-identical from call to call. */
#ifndef PCTRANS_HIP_POST_H
#define PCTRANS_HIP_POST_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- resize + threshold: replaces F.interpolate(..., "bilinear", align_corners=False) of MaskFormer.forward
 * (arch/maskformer.py:236-240) and `mask_pred.sigmoid() > threshold` with its per-query `.sum()` (:283-286, :310-313) ----------
 * One launch.  The resize from (h, w) to (height, width) is evaluated in fp32 per output pixel and never stored; equal sizes are
 * a plain copy.  Tap indices and weights come from the exact source coordinate ((2 d + 1) * in - out) / (2 * out), clamped at 0.
 * The threshold is taken on the logit: a pixel is set where x > (float)log(t / (1 - t)), the logarithm in double. */
PCT_API int pct_instance_masks_f32(const float *logits, int batch, int num_query, int h, int w, int height, int width,
                                   int dataset, uint32_t *bits, int32_t *areas, void *stream);
PCT_API int pct_instance_masks_bf16(const void *logits, int batch, int num_query, int h, int w, int height, int width,
                                    int dataset, uint32_t *bits, int32_t *areas, void *stream);

/* ---- bit planes -> label map: replaces the rest of instance_inference (arch/maskformer.py:286-346) with mask_post (:403-431),
 * dice_for (:392-401), mask_nms (:357-390) and comput_mmi (:349-355) ---------------------------------------------------------------
 * `bits` / `areas` as pct_instance_masks_* wrote them.  Queries with area > 40 are kept; pairwise intersections are popcounts;
 * dice = (2 I + 1) / (a_i + a_j + 1) by IEEE fp32 division, compared in fp32; first-come clustering in query order whose member
 * lists are not filtered against earlier clusters; cluster mean = count / size in fp32 (CVPPP: > (float)0.6 gives a new hard
 * plane, areas and intersections recomputed by popcount; BBBC: the mean is the mask, its area (sum of counts) / size exactly);
 * CVPPP NMS in descending area (equal areas: a stable ascending sort, reversed) on max(I / a_i, I / a_j) >= 0.72 in double with
 * comput_mmi's 1e-5 when an area is 0; survivors ascending by area, stably; label = 1-based position of the first maximum.
 * `workspace`: caller-owned, 16-byte aligned, nothing is allocated inside the call; with NQ = batch * num_query,
 * QW = ceil(num_query / 32) and r4(x) = x rounded up to a multiple of 4,
 *   4 * (NQ * PW  +  r4(NQ * num_query)  +  r4(NQ * QW)  +  5 * r4(NQ)  +  4 * batch)  bytes
 * (merged planes, intersections, cluster member sets, cluster sums / areas / sizes / order, per-image counts).  No word of it
 * is read before the call has written it.  Five launches for BBBC, seven for CVPPP. */
PCT_API int pct_instance_labels_from_bits(const uint32_t *bits, const int32_t *areas, int batch, int num_query, int height,
                                          int width, int dataset, void *workspace, int16_t *labels, void *stream);

/* ---- the two stages in one call: what MaskFormer.forward does in eval mode after the head (arch/maskformer.py:236-257) ------
 * `workspace`: as above, plus the thresholded planes and their areas in front,
 *   4 * (NQ * PW  +  r4(NQ))  bytes more. */
PCT_API int pct_instance_labels_f32(const float *logits, int batch, int num_query, int h, int w, int height, int width,
                                    int dataset, void *workspace, int16_t *labels, void *stream);
PCT_API int pct_instance_labels_bf16(const void *logits, int batch, int num_query, int h, int w, int height, int width,
                                     int dataset, void *workspace, int16_t *labels, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_POST_H */

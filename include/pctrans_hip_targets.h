/* Instance targets from label maps: entry points of libpctrans_hip.so.  Included by pctrans_hip.h (status codes, PCT_API,
 * conventions: there); include that header, not this one.  The caller (pctrans_amd/targets.py: prepare_instance_targets,
 * MaskFormer.prepare_instance_targets) takes them for dense device label maps; everything else keeps the torch formulation. */
#ifndef PCTRANS_HIP_TARGETS_H
#define PCTRANS_HIP_TARGETS_H

#ifdef __cplusplus
extern "C" {
#endif

#define PCT_TARGETS_MAX_INSTANCES 512          /* kept ids per image: the column limit of pct_lsap_f32's callers */
#define PCT_TARGETS_WORKSPACE_PER_IMAGE 151552 /* bytes: 8 192 bitmap + 12 288 totals + 131 072 value -> plane table */
#define PCT_TARGETS_STATUS_VALUE 1             /* status bit: a label is negative, above 65 535 or not integral */
#define PCT_TARGETS_STATUS_COUNT 2             /* status bit: more than PCT_TARGETS_MAX_INSTANCES kept ids */

/* ---- replaces, per image, the host loop of the reference trainer (connectomics/engine/trainer.py:231-319,
 *      prepare_intance_targets with POSITION_POINTS_NUM == 1):
 *          classes = torch.unique(gt_mask); classes = classes[classes != ignore_label]
 *          for class_id in classes: pos_xy = (gt_mask == class_id).nonzero().flip(1); mean(pos_xy.float(), 0) / W
 *      (csrc/instance_targets.hip) -----------------------------------------------------------------------------------------------
 *   labels        [batch, height, width] dense, of `dtype`: 0 uint8, 1 int16, 2 int32, 3 int64, 4 float32
 *   ignore_label  the value left out of the ids; a value outside 0 .. 65 535 leaves nothing out
 *   workspace     device scratch, 16-byte aligned, batch * PCT_TARGETS_WORKSPACE_PER_IMAGE bytes; need not be cleared.
 *                 pct_instance_targets_planes reads the value -> plane tables this call leaves in it
 *   ids           [batch, 512] int32 out: the kept label values of image n in ascending order, then zeros
 *   pixels        [batch, 512] int32 out: the pixel count of each kept id, then zeros
 *   centres       [batch, 512, 2] fp32 out: (sum x / count / width, sum y / count / width) of each kept id -- BOTH divided by
 *                 the width, as the reference does -- from exact integer sums, the two divisions in fp64, rounded to fp32 once;
 *                 then zeros
 *   num           [batch] int32 out: the number of kept ids (may exceed 512: the outputs then hold the first 512)
 *   status        [batch] int32 out: 0, or PCT_TARGETS_STATUS_* bits.  A label outside the covered values belongs to no id, is
 *                 not foreground in any plane and sets the VALUE bit; the caller is expected to discard the outputs
 * Integer atomics only (OR of presence bits, integer adds): two calls on the same map give the same bits, and the sums are exact
 * for every covered size.  Geometry: 0 < batch <= 65535, height * width < 2^31 - 1; anything else returns PCT_ERR_UNSUPPORTED
 * before any launch.  Five launches on `stream`, no allocation, no host synchronisation. */
PCT_API int pct_instance_targets_census(const void *labels, int dtype, int batch, int height, int width, int ignore_label,
                                        void *workspace, int32_t *ids, int32_t *pixels, float *centres, int32_t *num,
                                        int32_t *status, void *stream);

/* ---- replaces `gt_mask == class_id` per instance, torch.stack, the host -> device copy of the stack (trainer.py:252, 281, 288),
 *      fg_masks = gt_mask > 0 (trainer.py:302) and the consumers' torch.cat(masks).to(float32) ----------------------------------
 *   labels, dtype, batch, height, width   as given to the census
 *   workspace     as the census left it
 *   counts        [batch] int32: the planes of each image.  counts[n] > num[n] gives all-zero planes past the kept ids (an image
 *                 without instances is given one zero plane by the caller); counts[n] <= 512
 *   total_planes  sum of counts, max_count their largest: the host's copy of the same numbers
 *   starts        [batch] int32 out: the first plane of each image, the exclusive prefix sum of counts
 *   masks         [total_planes, height, width] uint8 out: 1 where the pixel's label is the plane's id, else 0
 *   planes        the same as fp32 1.0 / 0.0, or NULL
 *   fg            [batch, height, width] uint8 out: 1 where the label is > 0, or NULL
 *                 masks, planes and fg are 16-byte aligned and their allocations padded to a multiple of 16 ELEMENTS (the
 *                 padding is written with zeros): every store is 16 bytes wide and aligned, row and plane tails included
 * height * width a multiple of 16: a label is read once per pixel and group of planes; otherwise once per plane.
 * Geometry as the census.  Two launches on `stream` (three with fg when height * width is no multiple of 16), no allocation, no
 * host synchronisation. */
PCT_API int pct_instance_targets_planes(const void *labels, int dtype, int batch, int height, int width, const void *workspace,
                                        const int32_t *counts, long long total_planes, int max_count, int32_t *starts,
                                        uint8_t *masks, float *planes, uint8_t *fg, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_TARGETS_H */

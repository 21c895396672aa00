"""Instance targets from label maps: what the reference trainer's `prepare_intance_targets`
(connectomics/engine/trainer.py:231-319) builds before every `model(volume, target, True)` -- per image the instance ids, one
bool mask per id, the instances' centre points and the foreground mask -- as a library call, on the host formulation or on the
device kernels (C ABI `pct_instance_targets_census`, `pct_instance_targets_planes`, include/pctrans_hip_targets.h; kernels
pctrans_amd/csrc/instance_targets.hip).

`prepare_instance_targets(..., mode="torch")` is the definition: the trainer's loop restated (torch.unique, one `map == id`,
nonzero and float mean per instance, a stack, a copy of the stack to the device).  `mode="hip"` gives the same list from two
kernel sequences: only the label map crosses the bus, the masks are written on the device, and the fp32 planes the loss and
matcher kernels read come out of the same kernel (`TargetList.planes`), so that the consumers run no torch.cat(masks).float().

The device path costs ONE small device -> host copy: the per-image instance counts and status words, which size the outputs.
That copy is a host synchronisation, so the call cannot sit inside a graph capture.  There is no other synchronisation.

Unlike the project's other switches the default is "hip" wherever `supported` holds (process default: PCT_TARGETS = hip |
torch): nothing called this function before it existed, so no behaviour changes, and the kernels' output is exact -- masks,
labels, foreground, counts equal the torch mode bit for bit, and the centre points are the exact rational centres rounded to
fp32 once (the torch chain rounds a float mean and then a division) -- so there is no numerical trade to weigh."""
import os
import random

import torch

from . import _lib, _timing

MAX_INSTANCES = 512       # csrc/label_census.hpp: LC_MAX; PCT_TARGETS_MAX_INSTANCES (the matcher's column limit)
MAX_LABEL = 65535         # label values the device tables cover: 0 .. 65 535
MAX_BATCH = 65535
WORKSPACE_PER_IMAGE = 151552          # PCT_TARGETS_WORKSPACE_PER_IMAGE
STATUS_VALUE, STATUS_COUNT = 1, 2     # PCT_TARGETS_STATUS_*
_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4}


class TargetList(list):
    """The reference's list of per-image dicts ("labels", "masks", "center_points", and "fg_masks" with the semantic loss), plus,
    from the device path, the same masks as the consumers' kernels read them: `.planes` fp32 [sum G, H, W], `.starts` and
    `.counts` int32 device vectors (each image's first plane and plane count) and `.counts_host`, the counts as a list.  All
    four are None for a list the torch mode built."""
    planes = None
    starts = None
    counts = None
    counts_host = None


def default():
    """Process default of `prepare_instance_targets(mode=None)`: PCT_TARGETS = hip | torch (default hip: see the module text)."""
    return _lib.env_switch("PCT_TARGETS", "hip")


def supported(label_maps, points_num, device):
    """What the kernels cover: points_num == 1, the library present, a GPU device, [0 < N <= 65535, H, W] maps of uint8 / int16 /
    int32 / int64 / float32 with H * W < 2^31.  (The label VALUES -- integral, 0 .. 65 535, at most MAX_INSTANCES kept ids per
    image -- are checked on the device: prepare_instance_targets returns the torch mode's result where they do not hold.)"""
    if points_num != 1 or not torch.is_tensor(label_maps) or label_maps.dim() != 3 or label_maps.dtype not in _DTYPES:
        return False
    device = torch.device(device) if device is not None else label_maps.device
    if device.type != "cuda" or not torch.cuda.is_available() or not os.path.exists(_lib.LIB_PATH):
        return False
    N, H, W = label_maps.shape
    return 0 < N <= MAX_BATCH and 0 < H * W < 2 ** 31 - 1


def handed_planes(targets, masks, like):
    """`targets.planes` when the list carries planes that agree with its dicts' masks (`masks`: the list of them) in count, size
    and device -- the consumers then read them instead of building torch.cat(masks).float() -- else None."""
    planes = getattr(targets, "planes", None)
    counts = getattr(targets, "counts_host", None)
    if planes is None or counts is None or targets.starts is None or targets.counts is None:
        return None
    if (planes.dim() != 3 or planes.dtype != torch.float32 or planes.device != like.device or not planes.is_contiguous()
            or len(counts) != len(masks) or planes.shape[0] != sum(counts)
            or any(int(m.shape[0]) != c or tuple(m.shape[-2:]) != tuple(planes.shape[-2:]) for m, c in zip(masks, counts))):
        return None
    return planes


def _torch_targets(label_maps, points_num, semantic_loss_on, instance_discriminative, ignore_label, device):
    """The trainer's loop, image by image and instance by instance, where the label map lives; results moved to `device`."""
    out = TargetList()
    for gt in label_maps:
        ids = torch.unique(gt)                                   # ascending
        ids = ids[ids != ignore_label]
        width = gt.shape[-1]                                     # both coordinates are divided by the LAST dimension
        masks, points = [], []
        for v in ids:
            m = gt == v
            xy = m.nonzero().flip(dims=[1])                      # (x, y) of the instance's pixels, row-major order
            if points_num == 1:
                points.append(xy.to(torch.float).mean(dim=0) / width)
            else:
                if len(xy) < points_num:                         # too small: no mask, no points -- the label stays
                    continue
                drawn = xy[random.sample(range(len(xy)), points_num - 1)] / width
                centre = xy.to(torch.float).mean(dim=0) / width
                points.append(torch.cat([drawn, centre[None, :]]))
            masks.append(m)
        if masks:
            masks, points = torch.stack(masks), torch.stack(points)
        else:                                                    # one all-zero float plane, zero points
            masks = torch.zeros((1,) + tuple(gt.shape))
            points = torch.zeros((1, 2)) if points_num == 1 else torch.zeros((1, points_num, 2))
        labels = ids if instance_discriminative else (ids > 0)
        item = {"labels": labels.to(device, dtype=torch.int64), "masks": masks.to(device), "center_points": points.to(device)}
        if semantic_loss_on:
            item["fg_masks"] = (gt > 0).to(item["masks"])
        out.append(item)
    return out


def _pad16(n):
    return (n + 15) // 16 * 16


def _hip_targets(label_maps, semantic_loss_on, instance_discriminative, ignore_label, device):
    """The device path, or None when a status word reports label values the kernels do not cover."""
    maps = label_maps
    if maps.device != device:                                    # the label map crosses the bus once, as it is
        maps = maps.to(device, non_blocking=maps.is_pinned())
    maps = maps.contiguous()
    N, H, W = maps.shape
    P = H * W
    dtype = _DTYPES[maps.dtype]
    ignore = -1                                                  # a value no pixel has leaves nothing out
    if float(ignore_label) == int(ignore_label):
        ignore = int(ignore_label)
        if not maps.dtype.is_floating_point:                     # `ids != ignore_label` compares in the map's dtype: -1 is 255 in uint8
            ignore = int(torch.tensor([ignore], dtype=torch.int64).to(maps.dtype).item())
        if not 0 <= ignore <= MAX_LABEL:
            ignore = -1
    L = _lib.lib()
    ws = torch.empty(N * WORKSPACE_PER_IMAGE // 4, dtype=torch.int32, device=device)
    ids = torch.empty((N, MAX_INSTANCES), dtype=torch.int32, device=device)
    pixels = torch.empty((N, MAX_INSTANCES), dtype=torch.int32, device=device)
    centres = torch.empty((N, MAX_INSTANCES, 2), dtype=torch.float32, device=device)
    word = torch.empty((2, N), dtype=torch.int32, device=device)                     # num, status: what the host copy reads
    stream = torch.cuda.current_stream(device).cuda_stream
    with torch.cuda.device(device):
        with _timing.timed("instance_targets census", centres):
            rc = L.pct_instance_targets_census(maps.data_ptr(), dtype, N, H, W, ignore, ws.data_ptr(), ids.data_ptr(),
                                               pixels.data_ptr(), centres.data_ptr(), word[0].data_ptr(), word[1].data_ptr(),
                                               stream)
        _lib.check(rc, "instance_targets_census")
        num, status = word.cpu().tolist()                        # the call's one device -> host copy
        if any(status):
            return None
        counts_host = [max(g, 1) for g in num]                   # an image without instances gets one zero plane
        total = sum(counts_host)
        counts = word[0].clamp(min=1)
        starts = torch.empty(N, dtype=torch.int32, device=device)
        masks_buf = torch.empty(_pad16(total * P), dtype=torch.bool, device=device)
        planes_buf = torch.empty(_pad16(total * P), dtype=torch.float32, device=device)
        fg_buf = torch.empty(_pad16(N * P), dtype=torch.bool, device=device) if semantic_loss_on else None
        with _timing.timed("instance_targets planes", planes_buf):
            rc = L.pct_instance_targets_planes(maps.data_ptr(), dtype, N, H, W, ws.data_ptr(), counts.data_ptr(), total,
                                               max(counts_host), starts.data_ptr(), masks_buf.data_ptr(), planes_buf.data_ptr(),
                                               fg_buf.data_ptr() if semantic_loss_on else None, stream)
        _lib.check(rc, "instance_targets_planes")
    masks = masks_buf[:total * P].view(total, H, W)
    planes = planes_buf[:total * P].view(total, H, W)
    fg = fg_buf[:N * P].view(N, H, W) if semantic_loss_on else None
    labels = ids.to(torch.int64) if instance_discriminative else (ids > 0).to(torch.int64)
    out = TargetList()
    at = 0
    for n, g in enumerate(num):
        if g:
            item = {"labels": labels[n, :g], "masks": masks[at:at + g], "center_points": centres[n, :g]}
        else:                                                    # the torch mode's float zero plane and zero point
            item = {"labels": labels[n, :0], "masks": planes[at:at + 1], "center_points": centres[n, :1]}
        if semantic_loss_on:
            item["fg_masks"] = fg[n] if g else fg[n].to(torch.float32)
        out.append(item)
        at += counts_host[n]
    out.planes, out.starts, out.counts, out.counts_host = planes, starts, counts, counts_host
    return out


def prepare_instance_targets(label_maps, points_num=1, semantic_loss_on=False, instance_discriminative=False, ignore_label=0,
                             device=None, mode=None):
    """label_maps [N, H, W] (CPU or device; uint8 / int16 / int32 / int64 / float32: the trainer's targets[0]) -> TargetList of
    N dicts on `device` (default: the maps' device):
        labels         int64 [G]: the ids present, ascending, without `ignore_label` (instance_discriminative), else ids > 0
        masks          bool [G, H, W]: map == id; an image without instances gives ONE all-zero float32 plane
        center_points  fp32 [G, 2] = (mean x, mean y) / W -- both divided by the width; [G, points_num, 2] with
                       points_num > 1: points_num - 1 pixels drawn with random.sample in the reference's order, then the
                       centre; an instance of fewer than points_num pixels then loses its mask and points, not its label
        fg_masks       (semantic_loss_on) map > 0, in the masks' dtype
    mode "torch": the trainer's host loop restated -- the definition.  mode "hip": the same list from the device kernels, where
    `supported` holds; the masks are views of one allocation and the list carries the fp32 planes (see TargetList).  Label
    values the kernels do not cover (not integral, outside 0 .. 65 535, more than MAX_INSTANCES ids in an image) are found on
    the device and give the torch mode's result.  mode None: PCT_TARGETS, default "hip" -- the output is exact and the function
    has no earlier behaviour to keep.  The hip mode makes one small device -> host copy (counts and status), a host
    synchronisation: not for use inside a graph capture."""
    if not torch.is_tensor(label_maps) or label_maps.dim() != 3:
        raise ValueError("label_maps must be a [N, H, W] tensor")
    if points_num < 1:
        raise ValueError("points_num must be at least 1")
    mode = default() if mode is None else mode
    if mode not in ("hip", "torch"):
        raise ValueError("mode must be 'hip' or 'torch', got %r" % (mode,))
    device = torch.device(device) if device is not None else label_maps.device
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if mode == "hip" and supported(label_maps, points_num, device):
        got = _hip_targets(label_maps, semantic_loss_on, instance_discriminative, ignore_label, device)
        if got is not None:
            return got
    return _torch_targets(label_maps, points_num, semantic_loss_on, instance_discriminative, ignore_label, device)

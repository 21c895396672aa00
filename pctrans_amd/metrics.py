"""Validation metrics from label maps: what the reference trainer computes after every eval forward -- SymmetricBestDice and
AbsDiffFGLabels for CVPPP (connectomics/engine/trainer.py:398-450, lib/evaluate/CVPPP_evaluate.pyx), the aggregated Jaccard
index, pixel F1 and panoptic quality for BBBC (trainer.py:497-573, connectomics/inference/evaluation/metrics_bbbc.py) -- as a
library call, on a table-based torch formulation or on the device kernels (C ABI `pct_label_overlap`, `pct_label_metrics`,
include/pctrans_hip_metrics.h; kernels pctrans_amd/csrc/label_metrics.hip).

Every one of them is a function of the contingency table of the two maps (pixels per (ground-truth value, predicted value)
pair) and its row and column totals; no per-mask pass over the image is needed.

    label_overlap(pred, gt, fg=None)                  the table, the sorted values, their pixel counts, the raw value ranges
    cvppp_metrics(pred, gt, fg=None)                  best_dice_pred, best_dice_gt, sbd, abs_diff_fg          [N] float64 each
    bbbc_metrics(pred, gt, fg=None)                   aji, dice, dq, sq, pq [N] float64; tp, fp, fn, taken [N] int32
    instance_metrics(pred, gt, dataset, fg=None)      one of the two, by dataset name

`mode="torch"` is the definition used for CPU tensors and for whatever the kernels do not cover: one torch.unique and one
bincount per image, then the O(G * P) rules on the host.  `mode="hip"` gives the same numbers from six launches for the whole
batch, without a device -> host copy of the maps; the results stay on the device.  The process default is PCT_METRICS = hip |
torch, "hip" where `supported` holds: nothing called these functions before they existed, and the integer outputs are exact
while every ratio is one fp64 division of exact integers, so there is no numerical trade to weigh.

The status word of the kernels rides on every result as `.status` ([N] int32 on the maps' device; STATUS_* bits).  With
`check=True` (default) the metric functions read it -- ONE small device -> host copy, a host synchronisation, so not inside a
graph capture -- and return the torch mode's result where a map holds values the kernels do not cover (not integral, outside
0 .. 65 535, more than MAX_VALUES distinct values in an image).  With `check=False` nothing is read: reading `.status` is then
the caller's synchronisation and the caller's decision.

The workspace and the table come from a per-(device, batch) cache, as in postprocess.py: a call allocates nothing but its
results, calls of one batch size on one device share the buffers and must be ordered on one stream; `clear_workspaces()`
drops them.  The table handed out by `label_overlap` is therefore a clone."""
import os

import torch

from . import _lib

MAX_VALUES = 512          # csrc/label_census.hpp: LC_MAX; PCT_METRICS_MAX_VALUES (distinct values per map, background included)
MAX_LABEL = 65535
MAX_BATCH = 65535
MAX_PIXELS = 2 ** 24      # height * width below this
WORKSPACE_PER_IMAGE = 278528          # PCT_METRICS_WORKSPACE_PER_IMAGE
COLUMNS = 12                          # PCT_METRICS_COLUMNS
STATUS_PRED_VALUE, STATUS_PRED_COUNT, STATUS_GT_VALUE, STATUS_GT_COUNT = 1, 2, 4, 8   # PCT_METRICS_STATUS_*
STATUS_EMPTY_PRED, STATUS_EMPTY_GT = 16, 32
STATUS_FALLBACK = STATUS_PRED_VALUE | STATUS_PRED_COUNT | STATUS_GT_VALUE | STATUS_GT_COUNT
DATASETS = ("CVPPP", "BBBC")
_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4}
_CVPPP_KEYS = ("best_dice_pred", "best_dice_gt", "sbd", "abs_diff_fg")
_BBBC_KEYS = ("aji", "dice", "dq", "sq", "pq")
_BBBC_COUNTS = ("tp", "fp", "fn", "taken")
_WORKSPACES = {}


class Metrics(dict):
    """name -> [N] tensor, plus `.status`: [N] int32 STATUS_* bits, and `.mode`: the formulation that produced the numbers."""
    status = None
    mode = None


class Overlap:
    """values [N, 2, K] (side 0: prediction, side 1: ground truth; ascending, then zeros), areas [N, 2, K], num [N, 2],
    range [N, 2, 2] (lowest, highest raw value), table [N, K, K] (T[n, g, p]), status [N].  K = MAX_VALUES from the kernels;
    the torch mode widens K where an image has more distinct values."""

    def __init__(self, values, areas, num, range_, table, status, mode):
        self.values, self.areas, self.num, self.range, self.table, self.status, self.mode = (
            values, areas, num, range_, table, status, mode)


def default():
    """Process default of the `mode` argument: PCT_METRICS = hip | torch (default hip: see the module text)."""
    return _lib.env_switch("PCT_METRICS", "hip")


def _mode(mode):
    mode = default() if mode is None else mode
    if mode not in ("hip", "torch"):
        raise ValueError("mode must be 'hip' or 'torch', got %r" % (mode,))
    return mode


def supported(pred, gt, fg=None):
    """What the kernels cover: the library present, two [0 < N <= 65535, H, W] maps of uint8 / int16 / int32 / int64 / float32
    on one GPU with H * W < 2^24, and an `fg` (if any) of the same shape there.  (The label VALUES are checked on the device:
    see the status word.)"""
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dim() != 3 or pred.shape != gt.shape:
        return False
    if pred.dtype not in _DTYPES or gt.dtype not in _DTYPES or not pred.is_cuda or pred.device != gt.device:
        return False
    if fg is not None and (not torch.is_tensor(fg) or fg.shape != pred.shape or fg.device != pred.device
                           or fg.dtype not in (torch.bool, torch.uint8)):
        return False
    if not os.path.exists(_lib.LIB_PATH):
        return False
    N, H, W = pred.shape
    return 0 < N <= MAX_BATCH and 0 < H * W < MAX_PIXELS


def clear_workspaces():
    """Drop every cached workspace.  Not while a captured graph that recorded a call of this module is still to be replayed."""
    _WORKSPACES.clear()


def _workspace(device, N):
    """(scratch bytes, table [N, 512, 512] int32) of a device and batch size."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    got = _WORKSPACES.get((idx, N))
    if got is None:
        got = (torch.empty((N * WORKSPACE_PER_IMAGE,), dtype=torch.uint8, device=device),
               torch.empty((N, MAX_VALUES, MAX_VALUES), dtype=torch.int32, device=device))
        _WORKSPACES[(idx, N)] = got
    return got


def _check_maps(pred, gt, fg):
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dim() != 3 or pred.shape != gt.shape:
        raise ValueError("pred and gt must be [N, H, W] tensors of one shape")
    if fg is not None and (not torch.is_tensor(fg) or fg.shape != pred.shape):
        raise ValueError("fg must have the maps' shape")


# ---------------------------------------------------------------- device path

def _hip_overlap(pred, gt, fg):
    """-> Overlap whose table is the cached buffer (valid until the next call of this batch size on this device)."""
    dev = pred.device
    pred, gt = pred.contiguous(), gt.contiguous()
    if fg is not None:
        fg = fg.contiguous()
        fg = fg.view(torch.uint8) if fg.dtype == torch.bool else fg
    N, H, W = pred.shape
    ws, table = _workspace(dev, N)
    values = torch.empty((N, 2, MAX_VALUES), dtype=torch.int32, device=dev)
    areas = torch.empty((N, 2, MAX_VALUES), dtype=torch.int32, device=dev)
    num = torch.empty((N, 2), dtype=torch.int32, device=dev)
    rng = torch.empty((N, 2, 2), dtype=torch.int32, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().pct_label_overlap(pred.data_ptr(), _DTYPES[pred.dtype], gt.data_ptr(), _DTYPES[gt.dtype],
                                          fg.data_ptr() if fg is not None else None, N, H, W, ws.data_ptr(), values.data_ptr(),
                                          areas.data_ptr(), num.data_ptr(), rng.data_ptr(), table.data_ptr(), status.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "label_overlap")
    return Overlap(values, areas, num, rng, table, status, "hip")


def _hip_metrics(pred, gt, fg):
    """-> (metrics [N, 12] float64, counts [N, 4] int32, status [N] int32), all on the device, nothing read back."""
    ov = _hip_overlap(pred, gt, fg)
    dev, N = pred.device, pred.shape[0]
    metrics = torch.empty((N, COLUMNS), dtype=torch.float64, device=dev)
    counts = torch.empty((N, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().pct_label_metrics(ov.values.data_ptr(), ov.areas.data_ptr(), ov.num.data_ptr(), ov.range.data_ptr(),
                                          ov.table.data_ptr(), N, metrics.data_ptr(), counts.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "label_metrics")
    return metrics, counts, ov.status


# ---------------------------------------------------------------- torch formulation

def _torch_image(pred, gt, fg):
    """One image -> (vP, vG sorted distinct values, aP, aG int64 pixel counts, T int64 [G, P]) on the CPU."""
    if fg is not None:
        pred = torch.where(fg != 0, pred, torch.zeros((), dtype=pred.dtype, device=pred.device))
    vP, iP = torch.unique(pred.reshape(-1), sorted=True, return_inverse=True)
    vG, iG = torch.unique(gt.reshape(-1), sorted=True, return_inverse=True)
    nP, nG = vP.numel(), vG.numel()
    T = torch.bincount(iG * nP + iP, minlength=nG * nP).view(nG, nP).cpu()
    return vP.cpu(), vG.cpu(), T.sum(0), T.sum(1), T


def _ordered_sum(terms):
    s = 0.0
    for x in terms.tolist():
        s += x
    return s


def _best_dice(T, a_in, a_other, lo, hi):
    """T [other, in]: sum over the `in` values but the lowest, ascending, of the best dice against the `other` values but the
    lowest, divided by the raw value range."""
    if not hi > lo:
        return 0.0
    if T.shape[0] < 2 or T.shape[1] < 2:
        return 0.0
    dice = (2 * T[1:, 1:]).double() / (a_other[1:, None] + a_in[None, 1:]).double()
    return _ordered_sum(dice.max(dim=0).values) / float(hi - lo)


def _cvppp_rules(vP, vG, aP, aG, T):
    loP, hiP, loG, hiG = float(vP[0]), float(vP[-1]), float(vG[0]), float(vG[-1])
    bdp = _best_dice(T, aP, aG, loP, hiP)
    bdg = _best_dice(T.t(), aG, aP, loG, hiG)
    return bdp, bdg, min(bdp, bdg), abs((hiP - loP) - (hiG - loG))


def _bbbc_rules(vP, vG, aP, aG, T):
    p0, g0 = int(bool(vP[0] == 0)), int(bool(vG[0] == 0))
    P, G = vP.numel() - p0, vG.numel() - g0
    Tf, bP, bG = T[g0:, p0:], aP[p0:], aG[g0:]                # instances only
    # AJI: the reference's sequential procedure
    taken = torch.zeros(P, dtype=torch.bool)
    c = u = 0
    if P > 0:
        for g in range(G):
            inter = torch.where(taken, torch.zeros_like(Tf[g]), Tf[g])
            union = torch.where(taken, bG[g].expand(P), bG[g] + bP - Tf[g])
            q = inter.double() / union.double()
            hit = int((q == q.max()).nonzero()[0])            # the first maximum
            c += int(inter[hit])
            u += int(union[hit])
            taken[hit] = True
        u += int(bP[~taken].sum())
    aji = c / u if u > 0 else 0.0
    # pixel F1 of foreground against foreground
    tp_pix = int(Tf.sum())
    den = int(bP.sum()) + int(bG.sum())                       # 2 TP + FP + FN
    f1 = 2 * tp_pix / den if den > 0 else 0.0
    # PQ at 0.5: IoU strictly above 1/2, decided in integers
    union = bG[:, None] + bP[None, :] - Tf
    matched = 2 * Tf > union
    iou = Tf.double() / union.clamp(min=1).double()
    tp = int(matched.sum())
    fp, fn = P - tp, G - tp
    den = tp + 0.5 * fp + 0.5 * fn
    dq = tp / den if den > 0 else 0.0
    sq = _ordered_sum(iou[matched]) / (tp + 1e-6)             # boolean indexing keeps (ground-truth, prediction) order
    return (aji, f1, dq, sq, dq * sq), (tp, fp, fn, int(taken.sum()))


def _torch_status(vP, vG, nP, nG):
    def bad(v):
        v = v.double()
        return bool(((v < 0) | (v > MAX_LABEL) | (v != v.trunc())).any())
    s = (STATUS_PRED_VALUE if bad(vP) else 0) | (STATUS_GT_VALUE if bad(vG) else 0)
    s |= (STATUS_PRED_COUNT if nP > MAX_VALUES else 0) | (STATUS_GT_COUNT if nG > MAX_VALUES else 0)
    s |= (0 if bool((vP != 0).any()) else STATUS_EMPTY_PRED) | (0 if bool((vG != 0).any()) else STATUS_EMPTY_GT)
    return s


def _torch_metrics(pred, gt, fg):
    """-> (metrics [N, 12] float64, counts [N, 4] int32, status [N] int32) on the maps' device."""
    rows, cnts, status = [], [], []
    for n in range(pred.shape[0]):
        vP, vG, aP, aG, T = _torch_image(pred[n], gt[n], None if fg is None else fg[n])
        cv = _cvppp_rules(vP, vG, aP, aG, T)
        bb, cn = _bbbc_rules(vP, vG, aP, aG, T)
        rows.append(list(cv) + list(bb) + [0.0] * (COLUMNS - 9))
        cnts.append(list(cn))
        status.append(_torch_status(vP, vG, vP.numel(), vG.numel()))
    dev = pred.device
    return (torch.tensor(rows, dtype=torch.float64).reshape(-1, COLUMNS).to(dev),
            torch.tensor(cnts, dtype=torch.int32).reshape(-1, 4).to(dev), torch.tensor(status, dtype=torch.int32).to(dev))


def _torch_overlap(pred, gt, fg):
    per = [_torch_image(pred[n], gt[n], None if fg is None else fg[n]) for n in range(pred.shape[0])]
    N = len(per)
    K = max([MAX_VALUES] + [max(p[0].numel(), p[1].numel()) for p in per])
    vdtype = torch.float64 if (pred.dtype.is_floating_point or gt.dtype.is_floating_point) else torch.int64
    values = torch.zeros((N, 2, K), dtype=vdtype)
    areas = torch.zeros((N, 2, K), dtype=torch.int64)
    num = torch.zeros((N, 2), dtype=torch.int32)
    rng = torch.zeros((N, 2, 2), dtype=vdtype)
    table = torch.zeros((N, K, K), dtype=torch.int64)
    status = torch.zeros((N,), dtype=torch.int32)
    for n, (vP, vG, aP, aG, T) in enumerate(per):
        nP, nG = vP.numel(), vG.numel()
        values[n, 0, :nP], values[n, 1, :nG] = vP.to(vdtype), vG.to(vdtype)
        areas[n, 0, :nP], areas[n, 1, :nG] = aP, aG
        num[n, 0], num[n, 1] = nP, nG
        rng[n, 0, 0], rng[n, 0, 1], rng[n, 1, 0], rng[n, 1, 1] = vP[0], vP[-1], vG[0], vG[-1]
        table[n, :nG, :nP] = T
        status[n] = _torch_status(vP, vG, nP, nG)
    dev = pred.device
    return Overlap(values.to(dev), areas.to(dev), num.to(dev), rng.to(dev), table.to(dev), status.to(dev), "torch")


# ---------------------------------------------------------------- public functions

def label_overlap(pred, gt, fg=None, mode=None):
    """pred, gt [N, H, W] label maps; fg: optional foreground map, where it is 0 the predicted label reads as 0 (the trainer's
    `seg_outputs * fg`).  -> Overlap (see there).  mode "hip": int32 tensors of K = MAX_VALUES from the kernels, the status
    word unread; where `supported` does not hold, and in mode "torch": the torch formulation (int64, or float64 values for
    float maps), K widened where an image has more distinct values."""
    _check_maps(pred, gt, fg)
    if _mode(mode) == "hip" and supported(pred, gt, fg):
        ov = _hip_overlap(pred, gt, fg)
        ov.table = ov.table.clone()
        return ov
    return _torch_overlap(pred, gt, fg)


def _all_metrics(pred, gt, fg, mode, check):
    _check_maps(pred, gt, fg)
    if _mode(mode) == "hip" and supported(pred, gt, fg):
        metrics, counts, status = _hip_metrics(pred, gt, fg)
        if not check or not any(s & STATUS_FALLBACK for s in status.cpu().tolist()):   # the call's one device -> host copy
            return metrics, counts, status, "hip"
    return _torch_metrics(pred, gt, fg) + ("torch",)


def _result(keys, columns, status, mode):
    out = Metrics(zip(keys, columns))
    out.status, out.mode = status, mode
    return out


def cvppp_metrics(pred, gt, fg=None, mode=None, check=True):
    """-> Metrics of [N] float64 tensors on the maps' device: best_dice_pred = BD(pred, gt), best_dice_gt = BD(gt, pred),
    sbd = min of the two, abs_diff_fg = |(max_pred - min_pred) - (max_gt - min_gt)|.  Background is the lowest value present
    in each map; absent integers of a map's value range add 0 to its sum and 1 to its divisor."""
    m, _, status, mode = _all_metrics(pred, gt, fg, mode, check)
    return _result(_CVPPP_KEYS, [m[:, i] for i in range(4)], status, mode)


def bbbc_metrics(pred, gt, fg=None, mode=None, check=True):
    """-> Metrics on the maps' device: aji, dice (pixel F1), dq, sq, pq [N] float64; tp, fp, fn (of PQ at IoU > 0.5) and taken
    (the predictions AJI took) [N] int32.  Value 0 is background; the other values are the instances in ascending order, as
    after the reference's remap_label.  Where the reference cannot form a number (no prediction, no instance) it is 0 and
    `.status` carries STATUS_EMPTY_PRED / STATUS_EMPTY_GT."""
    m, c, status, mode = _all_metrics(pred, gt, fg, mode, check)
    return _result(_BBBC_KEYS + _BBBC_COUNTS, [m[:, 4 + i] for i in range(5)] + [c[:, i] for i in range(4)], status, mode)


def instance_metrics(pred, gt, dataset, fg=None, mode=None, check=True):
    """cvppp_metrics for dataset "CVPPP", bbbc_metrics for "BBBC"."""
    if dataset == "CVPPP":
        return cvppp_metrics(pred, gt, fg, mode, check)
    if dataset == "BBBC":
        return bbbc_metrics(pred, gt, fg, mode, check)
    raise ValueError("instance_metrics: unknown dataset %r" % (dataset,))

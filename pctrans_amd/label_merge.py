"""Small-object merging of label maps: the reference's merge_func (connectomics/engine/trainer.py:744-777), the last step of
its CVPPP test path (test_cvppp, :452-495) -- three passes of merge_small_object that relabel every instance of at most 5, 20
and 50 pixels to the dominant label in a 5 x 5, 11 x 11 and 11 x 11 window around the instance's centroid -- as a library call,
on a table-based torch formulation or on the device kernels (C ABI `pct_label_merge_small`, include/pctrans_hip_merge.h; kernels
pctrans_amd/csrc/label_merge.hip).

    merge_small_objects(labels, fg=None, passes=((5, 5), (20, 11), (50, 11)), mode=None, check=True)   -> the merged maps

`seg[seg == ids] = max_ids` moves all pixels of one current label to another, so the current map is cur[original value] and a
label's pixel count, row sum and column sum are additive under a merge.  One census of the image, a sequential procedure over
the table rows that reads at most window^2 pixels per visit and one relabel replace the per-label passes over the image.

One pass (threshold, window): the snapshot is the values present in the current map with their counts at the start of the pass;
every value whose snapshot count is <= threshold is visited in ascending order (0 like any other); the crop is
seg[r : r + window, c : c + window] around the LIVE centroid (floor division) with numpy's slice rules -- a negative start wraps,
so on a map larger than the window a centroid within window // 2 of the top or left border gives an empty crop; with fewer than
three distinct values in the crop nothing happens; ordered by count descending, THEN VALUE ASCENDING, the target is the best
value other than 0 and the visited one if 0 is first, else the first value (nothing if that is the visited one).  The reference
orders equal counts by numpy's unstable sort: where that can matter (0 and the visited value share the top count, or more than
one eligible value has the best count) STATUS_TIE is set and the result is this library's order.

`mode="torch"` is the definition used for CPU tensors and for whatever the kernels do not cover: one torch.unique and three
bincounts per image, then the table procedure on the host.  `mode="hip"` gives the same maps from six launches for the whole
batch without a device -> host copy of the maps.  The process default is PCT_LABEL_MERGE = hip | torch, "hip" where `supported`
holds: nothing called this function before it existed and the outputs are exact integers.

The result is the merged maps (the dtype and device of `labels`) and carries `.status` [N] int32 (STATUS_* bits), `.values` and
`.final` [N, K] (the distinct gated values in ascending order and the value each ends as; K = MAX_VALUES and int32 from the
kernels, widened and int64 / float64 in torch mode), `.merges` [N, MAX_PASSES] int32 (per pass), `.areas_before`, `.areas_after`
[N, K], `.num` [N] and `.mode`.  With `check=True` (default) the status is read -- ONE small device -> host copy, a host
synchronisation, so not inside a graph capture -- and an image with STATUS_VALUE or STATUS_COUNT gets the torch mode's map (its
table rows are then the torch mode's first K entries converted to int32).  With `check=False` nothing is read.

The workspace comes from a per-(device, batch) cache, as in metrics.py; `clear_workspaces()` drops it."""
import ctypes
import os

import torch

from . import _lib

MAX_VALUES = 512          # csrc/label_census.hpp: LC_MAX; PCT_MERGE_MAX_VALUES (distinct values per image, background included)
MAX_PASSES = 8            # PCT_MERGE_MAX_PASSES
MAX_WINDOW = 31           # PCT_MERGE_MAX_WINDOW
MAX_LABEL = 65535
MAX_BATCH = 65535
MAX_PIXELS = 2 ** 24      # height * width below this
WORKSPACE_PER_IMAGE = 147456          # PCT_MERGE_WORKSPACE_PER_IMAGE
STATUS_VALUE, STATUS_COUNT, STATUS_TIE = 1, 2, 4      # PCT_MERGE_STATUS_*
STATUS_FALLBACK = STATUS_VALUE | STATUS_COUNT
PASSES = ((5, 5), (20, 11), (50, 11))                 # merge_func
_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4}
_WORKSPACES = {}


def default():
    """Process default of the `mode` argument: PCT_LABEL_MERGE = hip | torch (default hip: see the module text)."""
    return _lib.env_switch("PCT_LABEL_MERGE", "hip")


def _mode(mode):
    mode = default() if mode is None else mode
    if mode not in ("hip", "torch"):
        raise ValueError("mode must be 'hip' or 'torch', got %r" % (mode,))
    return mode


def supported(labels, fg=None):
    """What the kernels cover: the library present, a [0 < N <= 65535, H, W] map of uint8 / int16 / int32 / int64 / float32 on a
    GPU with H * W < 2^24, and an `fg` (if any) of the same shape there.  (The label VALUES are checked on the device: see the
    status word.)"""
    if not torch.is_tensor(labels) or labels.dim() != 3 or labels.dtype not in _DTYPES or not labels.is_cuda:
        return False
    if fg is not None and (not torch.is_tensor(fg) or fg.shape != labels.shape or fg.device != labels.device
                           or fg.dtype not in (torch.bool, torch.uint8)):
        return False
    if not os.path.exists(_lib.LIB_PATH):
        return False
    N, H, W = labels.shape
    return 0 < N <= MAX_BATCH and 0 < H * W < MAX_PIXELS


def clear_workspaces():
    """Drop every cached workspace.  Not while a captured graph that recorded a call of this module is still to be replayed."""
    _WORKSPACES.clear()


def _workspace(device, N):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    got = _WORKSPACES.get((idx, N))
    if got is None:
        got = torch.empty((N * WORKSPACE_PER_IMAGE,), dtype=torch.uint8, device=device)
        _WORKSPACES[(idx, N)] = got
    return got


def _check_args(labels, fg, passes):
    if not torch.is_tensor(labels) or labels.dim() != 3:
        raise ValueError("labels must be an [N, H, W] tensor")
    if fg is not None and (not torch.is_tensor(fg) or fg.shape != labels.shape):
        raise ValueError("fg must have the maps' shape")
    passes = tuple((int(t), int(w)) for t, w in passes)
    if not 1 <= len(passes) <= MAX_PASSES or any(t < 0 or not 1 <= w <= MAX_WINDOW for t, w in passes):
        raise ValueError("passes must be 1 .. %d (threshold >= 0, 1 <= window <= %d) pairs, got %r" % (MAX_PASSES, MAX_WINDOW, passes))
    return passes


def _carry(out, status, values, final, merges, before, after, num, mode):
    out.status, out.values, out.final, out.merges, out.mode = status, values, final, merges, mode
    out.areas_before, out.areas_after, out.num = before, after, num
    return out


# ---------------------------------------------------------------- device path

def _hip_merge(labels, fg, passes):
    dev = labels.device
    labels = labels.contiguous()
    if fg is not None:
        fg = fg.contiguous()
        fg = fg.view(torch.uint8) if fg.dtype == torch.bool else fg
    N, H, W = labels.shape
    ws = _workspace(dev, N)
    out = torch.empty_like(labels)
    table = lambda k: torch.empty((N, k), dtype=torch.int32, device=dev)
    values, final, before, after, merges = table(MAX_VALUES), table(MAX_VALUES), table(MAX_VALUES), table(MAX_VALUES), table(MAX_PASSES)
    num = torch.empty((N,), dtype=torch.int32, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    host_passes = (ctypes.c_int32 * (2 * len(passes)))(*[x for p in passes for x in p])
    with torch.cuda.device(dev):
        rc = _lib.lib().pct_label_merge_small(labels.data_ptr(), _DTYPES[labels.dtype], fg.data_ptr() if fg is not None else None,
                                              N, H, W, ctypes.cast(host_passes, ctypes.c_void_p), len(passes),
                                              ws.data_ptr(), out.data_ptr(), values.data_ptr(), final.data_ptr(),
                                              before.data_ptr(), after.data_ptr(), num.data_ptr(), merges.data_ptr(),
                                              status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "label_merge_small")
    return _carry(out, status, values, final, merges, before, after, num, "hip")


# ---------------------------------------------------------------- torch formulation

def _crop_range(start, window, n):
    """numpy's seg[start : start + window] on an axis of n (start + window > 0)."""
    lo = max(start + n, 0) if start < 0 else min(start, n)
    return lo, min(start + window, n)


def _torch_image(seg, fg, passes):
    """One image -> (merged map on its device, values, final (tensors on the CPU), before, after, merges (lists), ties)."""
    if fg is not None:
        seg = torch.where(fg != 0, seg, torch.zeros((), dtype=seg.dtype, device=seg.device))
    H, W = seg.shape
    values, inv = torch.unique(seg.reshape(-1), sorted=True, return_inverse=True)
    K = values.numel()
    at = torch.arange(H * W, device=seg.device)
    ys, xs = torch.div(at, W, rounding_mode="floor").double(), (at % W).double()
    cnt = torch.bincount(inv, minlength=K).cpu().tolist()
    sr = [int(v) for v in torch.bincount(inv, weights=ys, minlength=K).cpu().tolist()]       # (exact: far below 2^53)
    sc = [int(v) for v in torch.bincount(inv, weights=xs, minlength=K).cpu().tolist()]
    values, ranks = values.cpu(), inv.view(H, W).cpu()
    before = list(cnt)
    cur = torch.arange(K)
    zero = int(torch.searchsorted(values, torch.zeros((), dtype=values.dtype))) if bool((values == 0).any()) else -1
    merges, ties = [0] * MAX_PASSES, 0
    for p, (threshold, window) in enumerate(passes):
        snap = list(cnt)
        for k in range(K):
            if snap[k] == 0 or snap[k] > threshold:
                continue
            assert cnt[k] > 0                                   # only the visited value vanishes
            r0, r1 = _crop_range(sr[k] // cnt[k] - window // 2, window, H)
            c0, c1 = _crop_range(sc[k] // cnt[k] - window // 2, window, W)
            if r0 >= r1 or c0 >= c1:
                continue
            hist = torch.bincount(cur[ranks[r0:r1, c0:c1]].reshape(-1), minlength=K).tolist()
            present = [v for v in range(K) if hist[v]]
            if len(present) < 3:
                continue
            top = max(hist)
            zero_first = zero >= 0 and hist[zero] == top
            eligible = [v for v in present if v != zero and v != k] if zero_first else present
            best = max(hist[v] for v in eligible)
            winners = [v for v in eligible if hist[v] == best]
            ties += int(len(winners) > 1 or (zero_first and k != zero and hist[k] == top))
            target = winners[0]                                 # count descending, then value ascending
            if target == k:
                continue
            cnt[target], sr[target], sc[target] = cnt[target] + cnt[k], sr[target] + sr[k], sc[target] + sc[k]
            cnt[k] = sr[k] = sc[k] = 0
            cur[cur == k] = target
            merges[p] += 1
    final = values[cur]
    out = final.to(seg.device)[inv].view(H, W)
    return out, values, final, before, cnt, merges, ties


def _torch_status(values, ties):
    v = values.double()
    bad = bool(((v < 0) | (v > MAX_LABEL) | (v != v.trunc())).any())
    return (STATUS_VALUE if bad else 0) | (STATUS_COUNT if values.numel() > MAX_VALUES else 0) | (STATUS_TIE if ties else 0)


def _torch_merge(labels, fg, passes):
    N = labels.shape[0]
    per = [_torch_image(labels[n], None if fg is None else fg[n], passes) for n in range(N)]
    K = max([MAX_VALUES] + [p[1].numel() for p in per])
    vdtype = torch.float64 if labels.dtype.is_floating_point else torch.int64
    values, final = torch.zeros((N, K), dtype=vdtype), torch.zeros((N, K), dtype=vdtype)
    before, after = torch.zeros((N, K), dtype=torch.int64), torch.zeros((N, K), dtype=torch.int64)
    merges = torch.zeros((N, MAX_PASSES), dtype=torch.int32)
    num, status = torch.zeros((N,), dtype=torch.int32), torch.zeros((N,), dtype=torch.int32)
    for n, (_, v, f, b, a, m, ties) in enumerate(per):
        k = v.numel()
        values[n, :k], final[n, :k] = v.to(vdtype), f.to(vdtype)
        before[n, :k], after[n, :k] = torch.tensor(b, dtype=torch.int64), torch.tensor(a, dtype=torch.int64)
        merges[n] = torch.tensor(m, dtype=torch.int32)
        num[n], status[n] = k, _torch_status(v, ties)
    dev = labels.device
    out = torch.stack([p[0] for p in per]) if N else torch.empty_like(labels)
    return _carry(out, status.to(dev), values.to(dev), final.to(dev), merges.to(dev), before.to(dev), after.to(dev), num.to(dev),
                  "torch")


# ---------------------------------------------------------------- public function

def merge_small_objects(labels, fg=None, passes=PASSES, mode=None, check=True):
    """labels [N, H, W] label maps; fg: optional foreground map, where it is 0 the label reads as 0 (the trainer's
    `seg_outputs * fg`); passes: (threshold, window) pairs in order.  -> the merged maps, carrying the tables and the status
    (see the module text)."""
    passes = _check_args(labels, fg, passes)
    if not (_mode(mode) == "hip" and supported(labels, fg)):
        return _torch_merge(labels, fg, passes)
    out = _hip_merge(labels, fg, passes)
    if check:
        bad = [n for n, s in enumerate(out.status.cpu().tolist()) if s & STATUS_FALLBACK]   # the call's one device -> host copy
        if bad:
            idx = torch.tensor(bad, device=labels.device)
            ref = _torch_merge(labels[idx], None if fg is None else fg[idx], passes)
            out[idx] = ref
            out.merges[idx] = ref.merges
            for mine, theirs in ((out.values, ref.values), (out.final, ref.final), (out.areas_before, ref.areas_before),
                                 (out.areas_after, ref.areas_after)):
                mine[idx] = theirs[:, :MAX_VALUES].to(torch.int32)
    return out

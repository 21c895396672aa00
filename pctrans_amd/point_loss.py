"""Python entry of the point-sampled mask losses (C ABI `pct_point_sample_f32`, `pct_point_mask_loss_forward_f32`,
`pct_point_mask_loss_backward_f32`, `pct_point_select_uncertain_f32`, include/pctrans_hip_train.h; kernels
pctrans_amd/csrc/point_loss.hip).

`point_sample_planes` is the gather (detectron2's point_sample on planes picked through an index); `point_mask_losses` is the
criterion's sigmoid_ce_loss + dice_loss on point samples of matched (prediction, target) planes with a HIP backward that
scatters with fixed-point LDS accumulators (deterministic: two calls give the same bits).  Opt-in: `SetCriterion.point_loss`
and `Point_HungarianMatcher.point_sample` are "torch" unless set to "hip" (process default: PCT_POINT_LOSS).
`select_uncertain_points` picks the most uncertain of the criterion's oversampled candidates in one launch (no logits in memory,
no topk); it acts inside the "hip" loss path when `SetCriterion.point_select` is "hip" (process default: PCT_POINT_SELECT).
`match_costs` is the matcher's whole cost pass (`pct_point_match_cost_f32`: both gathers, BCE, dice and the three contractions
in one kernel plus a small finishing one); `Point_HungarianMatcher.match_cost` is "torch" unless set to "hip" (process default:
PCT_MATCH_COST).

The `*_many` functions give the selection, the loss and the cost pass a head dimension (`pct_point_select_uncertain_many_f32`,
`pct_point_mask_loss_forward_many_f32`, `pct_point_match_cost_many_f32`): the decoder's prediction heads, separate tensors of one
geometry, go through ONE launch each, their addresses in a small table passed with the launch; per head the bits are those of the
single-head call.  They act when `SetCriterion.loss_heads` / `Point_HungarianMatcher.cost_heads` is "batched" (process default:
PCT_LOSS_HEADS, "each")."""
import ctypes
import os

import torch

from . import _lib, _timing

BAND_ROWS = 32        # rows of one backward workgroup's band (csrc/point_loss.hip: PL_BAND_ROWS)
MAX_WIDTH = 256       # widest prediction plane the loss kernels cover (PL_MAX_WIDTH)
MAX_CANDIDATES = 65536  # most candidates per pair the selection covers (PL_SELECT_MAX_CAND)
UNSUPPORTED = -4      # PCT_ERR_UNSUPPORTED
MATCH_QUERY_GROUP = 128   # queries / targets of one workgroup of the cost kernel, points of one pass, most chunks of the points
MATCH_TARGET_GROUP = 64   # and the workgroups the split aims for (csrc/point_loss.hip: MC_QGROUP, MC_GGROUP, MC_SUB,
MATCH_POINTS_PER_PASS = 128   # MC_MAX_CHUNKS, MC_WANT_GROUPS): the workspace formula of the header
MATCH_MAX_CHUNKS = 32
MATCH_WANT_GROUPS = 512
MATCH_MAX_BATCH = 65535
MAX_HEADS = 16        # heads of one *_many launch (include/pctrans_hip_train.h: PCT_POINT_MAX_HEADS); more go in groups


def default():
    """Process default of `SetCriterion.point_loss` / `Point_HungarianMatcher.point_sample`: PCT_POINT_LOSS = hip | torch
    (default torch)."""
    return _lib.env_switch("PCT_POINT_LOSS")


def select_default():
    """Process default of `SetCriterion.point_select`: PCT_POINT_SELECT = hip | torch (default torch)."""
    return _lib.env_switch("PCT_POINT_SELECT")


def match_cost_default():
    """Process default of `Point_HungarianMatcher.match_cost`: PCT_MATCH_COST = hip | torch (default torch)."""
    return _lib.env_switch("PCT_MATCH_COST")


def heads_default():
    """Process default of `SetCriterion.loss_heads` / `Point_HungarianMatcher.cost_heads`: PCT_LOSS_HEADS = each | batched
    (default each)."""
    v = os.environ.get("PCT_LOSS_HEADS") or "each"
    if v not in ("each", "batched"):
        raise RuntimeError("PCT_LOSS_HEADS must be 'each' or 'batched', got %r" % v)
    return v


def _planes_ok(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= 3 and t.is_contiguous()


def sample_supported(planes):
    """CUDA fp32 contiguous planes whose in-plane offsets fit 32 bits: what the gather covers."""
    return _planes_ok(planes) and 0 < planes.shape[-1] * planes.shape[-2] < 2 ** 31 - 1


def loss_supported(pred_masks, tgt_planes):
    """CUDA fp32 contiguous predictions no wider than MAX_WIDTH and fp32 contiguous targets: what the loss kernels cover."""
    return (sample_supported(pred_masks) and sample_supported(tgt_planes) and pred_masks.device == tgt_planes.device
            and pred_masks.shape[-1] <= MAX_WIDTH)


def _index(idx, n, dev):
    if idx is None:
        return None
    idx = idx.to(device=dev, dtype=torch.int32).contiguous()
    if idx.dim() != 1 or idx.shape[0] != n:
        raise RuntimeError("index must be a vector of %d plane numbers, got %s" % (n, tuple(idx.shape)))
    return idx


def _ptr(t):
    return t.data_ptr() if t is not None else None


def point_sample_planes(planes, plane_index, coords, planes_per_coord_row=1):
    """planes [..., H, W] fp32 on the device (leading dimensions flattened to num_planes); plane_index int [K] or None
    (identity, K = num_planes); coords [rows, P, 2] in (x, y) order, row k // planes_per_coord_row serving output row k.
    -> [K, P] fp32, F.grid_sample(planes[plane_index], 2 * coords - 1, align_corners=False) without the indexed copy.
    No gradient."""
    if not planes.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if not sample_supported(planes):
        raise RuntimeError("point_sample_planes needs contiguous fp32 planes")
    H, W = planes.shape[-2:]
    num_planes = planes.numel() // (H * W)
    coords = coords.detach().to(device=planes.device, dtype=torch.float32).contiguous()
    if coords.dim() != 3 or coords.shape[2] != 2:
        raise RuntimeError("coords must be [rows, P, 2]")
    K = num_planes if plane_index is None else int(plane_index.shape[0])
    idx = _index(plane_index, K, planes.device)
    rows, P = int(coords.shape[0]), int(coords.shape[1])
    per_row = int(planes_per_coord_row)
    if per_row < 1 or (K > 0 and (K - 1) // per_row >= rows):
        raise RuntimeError("coords has %d rows, %d outputs at %d per row need more" % (rows, K, per_row))
    out = torch.empty((K, P), dtype=torch.float32, device=planes.device)
    with torch.cuda.device(planes.device), _timing.timed("point_sample", out):
        rc = _lib.lib().pct_point_sample_f32(planes.data_ptr(), _ptr(idx), coords.data_ptr(), num_planes, H, W, K, P, rows,
                                             per_row, out.data_ptr(), torch.cuda.current_stream(planes.device).cuda_stream)
    _lib.check(rc, "point_sample")
    return out


def select_supported(pred_masks, cand_coords, num_keep):
    """What the selection covers: planes as the gather's, fp32 contiguous candidates [K, S, 2] on the planes' device with
    0 < S <= MAX_CANDIDATES, and 0 <= num_keep <= S."""
    return (sample_supported(pred_masks) and torch.is_tensor(cand_coords) and cand_coords.is_cuda
            and cand_coords.device == pred_masks.device and cand_coords.dtype == torch.float32 and cand_coords.dim() == 3
            and cand_coords.shape[2] == 2 and cand_coords.is_contiguous() and 0 < cand_coords.shape[1] <= MAX_CANDIDATES
            and 0 <= int(num_keep) <= cand_coords.shape[1])


def select_uncertain_points(pred_masks, src_index, cand_coords, num_keep, out=None, with_index=True):
    """The num_keep most uncertain (smallest |logit|) of each pair's candidates, in ascending candidate number
    (pct_point_select_uncertain_f32: ties at the threshold go to the lowest candidate numbers, NaN logits first).
    pred_masks [..., H, W] fp32 on the device; src_index int [K] plane numbers or None (identity); cand_coords [K, S, 2] (x, y).
    out: None, or fp32 contiguous [K, P, 2] with P >= num_keep whose rows' first num_keep points are written in place, the rest
    left as they are.  -> (coords, index): coords is `out`, or a new [K, num_keep, 2]; index int32 [K, num_keep] candidate
    numbers, or None with with_index=False.  No gradient."""
    if not pred_masks.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    num_keep = int(num_keep)
    cand_coords = cand_coords.detach()
    if not select_supported(pred_masks, cand_coords, num_keep):
        raise RuntimeError("select_uncertain_points needs contiguous fp32 device planes and candidates [K, S <= %d, 2], "
                           "0 <= num_keep <= S" % MAX_CANDIDATES)
    dev = pred_masks.device
    H, W = pred_masks.shape[-2:]
    K, S = int(cand_coords.shape[0]), int(cand_coords.shape[1])
    src = _index(src_index, K, dev)
    if out is None:
        out = torch.empty((K, num_keep, 2), dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.float32 and out.dim() == 3 and out.is_contiguous()
              and out.shape[0] == K and out.shape[1] >= num_keep and out.shape[2] == 2):
        raise RuntimeError("out must be contiguous fp32 [%d, >= %d, 2] on the planes' device" % (K, num_keep))
    index = torch.empty((K, num_keep), dtype=torch.int32, device=dev) if with_index else None
    with torch.cuda.device(dev), _timing.timed("point_select", out):
        rc = _lib.lib().pct_point_select_uncertain_f32(
            pred_masks.data_ptr(), _ptr(src), pred_masks.numel() // (H * W), H, W, cand_coords.data_ptr(), K, S, num_keep,
            out.data_ptr(), int(out.shape[1]), _ptr(index), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "point_select_uncertain")
    return out, index


def match_cost_supported(pred, tgt_planes, num_points=1, max_targets=1):
    """What `match_costs` covers: pred [B, Q, H, W] and tgt_planes [n, Ht, Wt] CUDA fp32 contiguous on one device with planes as
    the gather's, B <= MATCH_MAX_BATCH, at least one query, point and target column."""
    return (sample_supported(pred) and pred.dim() == 4 and _planes_ok(tgt_planes) and tgt_planes.dim() == 3
            and 0 < tgt_planes.shape[-1] * tgt_planes.shape[-2] < 2 ** 31 - 1 and pred.device == tgt_planes.device
            and 0 < pred.shape[0] <= MATCH_MAX_BATCH and pred.shape[1] > 0 and 0 < int(num_points) <= 2 ** 30
            and int(max_targets) > 0
            and -(-pred.shape[1] // MATCH_QUERY_GROUP) * -(-int(max_targets) // MATCH_TARGET_GROUP) <= 65535)


def match_cost_workspace_bytes(batch, num_query, max_targets, num_points):
    """The workspace formula of include/pctrans_hip_train.h."""
    qg, gg = -(-num_query // MATCH_QUERY_GROUP), -(-max_targets // MATCH_TARGET_GROUP)
    chunks = max(1, min(MATCH_MAX_CHUNKS, -(-num_points // MATCH_POINTS_PER_PASS), -(-MATCH_WANT_GROUPS // (batch * qg * gg))))
    Qp, Gp = qg * MATCH_QUERY_GROUP, gg * MATCH_TARGET_GROUP
    return 4 * batch * chunks * (2 * Qp * Gp + Qp + Gp)


def match_costs(pred, tgt_planes, starts, counts, coords, cost_mask, cost_dice, max_targets=None):
    """The matcher's cost matrices in one call (pct_point_match_cost_f32).  pred [B, Q, H, W] fp32 contiguous on the device;
    tgt_planes [sum G, Ht, Wt] fp32, image b owning planes starts[b] .. starts[b] + counts[b] (int32 [B] device tensors);
    coords [B, P, 2] (x, y), one row per image.  max_targets: the number of columns (the largest count; it is read from `counts`
    with one host synchronisation when not given).  -> cost [B, Q, max_targets] fp32, zero past an image's count.  No gradient."""
    if not pred.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = pred.device
    starts = starts.to(device=dev, dtype=torch.int32).contiguous()
    counts = counts.to(device=dev, dtype=torch.int32).contiguous()
    gmax = int(counts.max()) if max_targets is None else int(max_targets)
    coords = coords.detach().to(device=dev, dtype=torch.float32).contiguous()
    if coords.dim() != 3 or coords.shape[2] != 2 or coords.shape[0] != pred.shape[0]:
        raise RuntimeError("coords must be [B, P, 2]")
    P = int(coords.shape[1])
    if not match_cost_supported(pred, tgt_planes, P, gmax):
        raise RuntimeError("match_costs needs contiguous fp32 device planes, pred [B, Q, H, W], at least one point and target")
    B, Q, H, W = pred.shape
    if tuple(starts.shape) != (B,) or tuple(counts.shape) != (B,):
        raise RuntimeError("starts and counts must be vectors of %d entries" % B)
    Ht, Wt = tgt_planes.shape[-2:]
    cost = torch.empty((B, Q, gmax), dtype=torch.float32, device=dev)
    ws = torch.empty(match_cost_workspace_bytes(B, Q, gmax, P) // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("point_match_cost", cost):
        rc = _lib.lib().pct_point_match_cost_f32(
            pred.data_ptr(), B, Q, H, W, tgt_planes.data_ptr(), int(tgt_planes.shape[0]), Ht, Wt, starts.data_ptr(),
            counts.data_ptr(), gmax, coords.data_ptr(), P, float(cost_mask), float(cost_dice), ws.data_ptr(), cost.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "point_match_cost")
    return cost


def point_mask_loss_forward(pred_planes, src_index, tgt_planes, tgt_index, coords):
    """-> (x [K, P], t [K, P], sums [K, 4]) of pct_point_mask_loss_forward_f32; pred_planes [..., H, W], tgt_planes
    [..., Ht, Wt], coords [K, P, 2]."""
    if not pred_planes.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = pred_planes.device
    H, W = pred_planes.shape[-2:]
    Ht, Wt = tgt_planes.shape[-2:]
    K, P = int(coords.shape[0]), int(coords.shape[1])
    src, tgt = _index(src_index, K, dev), _index(tgt_index, K, dev)
    x = torch.empty((K, P), dtype=torch.float32, device=dev)
    t = torch.empty((K, P), dtype=torch.float32, device=dev)
    sums = torch.zeros((K, 4), dtype=torch.float32, device=dev) if P == 0 else torch.empty((K, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("point_loss forward", x):
        rc = _lib.lib().pct_point_mask_loss_forward_f32(
            pred_planes.data_ptr(), _ptr(src), pred_planes.numel() // (H * W), H, W, tgt_planes.data_ptr(), _ptr(tgt),
            tgt_planes.numel() // (Ht * Wt), Ht, Wt, coords.data_ptr(), K, P, x.data_ptr(), t.data_ptr(), sums.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "point_mask_loss_forward")
    return x, t, sums


def point_mask_loss_backward(x, t, coords, alpha, beta, gamma, height, width):
    """-> grad_planes [K, height, width] fp32 of pct_point_mask_loss_backward_f32: alpha, beta, gamma [K] fp32 on the device."""
    if not x.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    K, P = x.shape
    dev = x.device
    coef = [c.detach().to(device=dev, dtype=torch.float32).contiguous() for c in (alpha, beta, gamma)]
    if any(tuple(c.shape) != (K,) for c in coef) or tuple(t.shape) != (K, P) or tuple(coords.shape) != (K, P, 2):
        raise RuntimeError("point_mask_loss_backward: x, t [K, P], coords [K, P, 2], alpha, beta, gamma [K]")
    if P == 0:
        return torch.zeros((K, height, width), dtype=torch.float32, device=dev)
    grad = torch.empty((K, height, width), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("point_loss backward", grad):
        rc = _lib.lib().pct_point_mask_loss_backward_f32(
            x.data_ptr(), t.data_ptr(), coords.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(), coef[2].data_ptr(), K, P,
            int(height), int(width), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "point_mask_loss_backward")
    return grad


class PointMaskLossFunction(torch.autograd.Function):
    """(pred_masks [B, Q, H, W]) -> (loss_mask, loss_dice).  Saves the point logits and labels [K, P], the coordinates and the
    four sums per pair; the prediction is read in place through src_index and receives a placed (not accumulated) gradient."""

    @staticmethod
    def forward(ctx, pred_masks, src_index, tgt_planes, tgt_index, coords, num_masks):
        x, t, sums = point_mask_loss_forward(pred_masks, src_index, tgt_planes, tgt_index, coords)
        P = coords.shape[1]
        loss_mask = sums[:, 0].sum() / P / num_masks
        loss_dice = (1 - (2 * sums[:, 1] + 1) / (sums[:, 2] + sums[:, 3] + 1)).sum() / num_masks
        ctx.save_for_backward(x, t, coords, sums, src_index)
        ctx.num_masks, ctx.shape, ctx.dtype = float(num_masks), tuple(pred_masks.shape), pred_masks.dtype
        return loss_mask, loss_dice

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mask, grad_dice):
        x, t, coords, sums, src_index = ctx.saved_tensors
        K, P = x.shape
        H, W = ctx.shape[-2:]
        grad = torch.zeros(ctx.shape, dtype=torch.float32, device=x.device)
        if K == 0 or P == 0 or not ctx.needs_input_grad[0]:
            return (grad.to(ctx.dtype) if ctx.needs_input_grad[0] else None), None, None, None, None, None
        num = 2 * sums[:, 1] + 1
        den = sums[:, 2] + sums[:, 3] + 1
        gd = grad_dice.float() / ctx.num_masks
        alpha = (grad_mask.float() / (P * ctx.num_masks)).expand(K)
        beta = gd * num / (den * den)
        gamma = 2 * gd / den
        planes = point_mask_loss_backward(x, t, coords, alpha, beta, gamma, H, W)
        grad.view(-1, H, W)[src_index.long()] = planes                    # matched planes are distinct: a placement
        return grad.to(ctx.dtype), None, None, None, None, None


def point_mask_losses(pred_masks, src_idx, tgt_planes, tgt_index, coords, num_masks):
    """sigmoid_ce_loss and dice_loss of loss/maskformer_criterion.py on point samples, without the indexed copies.
    pred_masks [B, Q, H, W] fp32 contiguous on the device (differentiable); src_idx [K] plane numbers b * Q + q of the matched
    queries, distinct; tgt_planes [sum G, Ht, Wt] fp32; tgt_index [K]; coords [K, P, 2] (x, y) in [0, 1]; num_masks a number.
    -> (loss_mask, loss_dice), zero-dimensional tensors."""
    if not loss_supported(pred_masks, tgt_planes):
        raise RuntimeError("point_mask_losses needs contiguous fp32 device planes, predictions at most %d wide" % MAX_WIDTH)
    dev = pred_masks.device
    coords = coords.detach().to(device=dev, dtype=torch.float32).contiguous()
    if coords.dim() != 3 or coords.shape[2] != 2:
        raise RuntimeError("coords must be [K, P, 2]")
    K = int(coords.shape[0])
    src_index, tgt_index = _index(src_idx, K, dev), _index(tgt_index, K, dev)
    if K == 0 or coords.shape[1] == 0:
        zero = pred_masks.sum() * 0
        return zero, zero.clone()
    return PointMaskLossFunction.apply(pred_masks, src_index, tgt_planes.detach(), tgt_index, coords, float(num_masks))


# ---- several prediction heads in one launch ---------------------------------------------------------------------------------

def _heads_alike(preds):
    """A non-empty sequence of tensors of one shape, dtype and device."""
    return (isinstance(preds, (list, tuple)) and len(preds) > 0 and all(torch.is_tensor(p) for p in preds)
            and all(p.shape == preds[0].shape and p.dtype == preds[0].dtype and p.device == preds[0].device for p in preds))


def _head_table(preds):
    """The host array of device pointers the *_many entries take."""
    return (ctypes.c_void_p * len(preds))(*[p.data_ptr() for p in preds])


def _head_groups(num_heads):
    return [(h0, min(h0 + MAX_HEADS, num_heads)) for h0 in range(0, num_heads, MAX_HEADS)]


def _index_many(idx, heads, n, dev):
    if idx is None:
        return None
    idx = idx.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(idx.shape) != (heads, n):
        raise RuntimeError("index must be [%d, %d] plane numbers, got %s" % (heads, n, tuple(idx.shape)))
    return idx


def _part(t, h0, h1):
    return None if t is None else t[h0:h1].data_ptr()


def draw_head_coords(num_heads, num_pairs, num_sampled, num_random, device):
    """The random numbers of `num_heads` per-head `loss_masks` calls, drawn ahead: per head, in order, torch.rand(K, num_sampled, 2)
    then (num_random > 0) torch.rand(K, num_random, 2), into slices of two preallocated tensors.  The generator ends where the
    per-head calls leave it.  -> (candidates [heads, K, num_sampled, 2], fresh [heads, K, num_random, 2])."""
    cand = torch.empty((num_heads, num_pairs, num_sampled, 2), dtype=torch.float32, device=device)
    fresh = torch.empty((num_heads, num_pairs, max(num_random, 0), 2), dtype=torch.float32, device=device)
    for h in range(num_heads):
        torch.rand(num_pairs, num_sampled, 2, out=cand[h])
        if num_random > 0:
            torch.rand(num_pairs, num_random, 2, out=fresh[h])
    return cand, fresh


def select_many_supported(preds, cand_coords, num_keep):
    """Heads of one shape, dtype and device that each pass `select_supported` with their candidates [heads, K, S, 2]."""
    return (_heads_alike(preds) and torch.is_tensor(cand_coords) and cand_coords.dim() == 4
            and cand_coords.shape[0] == len(preds) and cand_coords.is_contiguous()
            and all(select_supported(p, cand_coords[h], num_keep) for h, p in enumerate(preds)))


def select_uncertain_points_many(preds, src_index, cand_coords, num_keep, out=None, with_index=True):
    """`select_uncertain_points` of every head in one launch (pct_point_select_uncertain_many_f32; more than MAX_HEADS heads in
    groups).  preds: a sequence of [..., H, W] fp32 device tensors of one shape; src_index int [heads, K] or None; cand_coords
    [heads, K, S, 2]; out None or fp32 contiguous [heads, K, P >= num_keep, 2].  -> (coords, index [heads, K, num_keep] or None);
    head h holds the bits of select_uncertain_points(preds[h], src_index[h], cand_coords[h], ...).  No gradient."""
    preds = list(preds)
    if not preds or not all(torch.is_tensor(p) and p.is_cuda for p in preds):
        raise RuntimeError("Not implemented on the CPU")
    num_keep = int(num_keep)
    cand_coords = cand_coords.detach()
    if not select_many_supported(preds, cand_coords, num_keep):
        raise RuntimeError("select_uncertain_points_many needs contiguous fp32 device planes of one shape and candidates "
                           "[heads, K, S <= %d, 2], 0 <= num_keep <= S" % MAX_CANDIDATES)
    dev = preds[0].device
    H, W = preds[0].shape[-2:]
    heads, K, S = len(preds), int(cand_coords.shape[1]), int(cand_coords.shape[2])
    src = _index_many(src_index, heads, K, dev)
    if out is None:
        out = torch.empty((heads, K, num_keep, 2), dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.float32 and out.dim() == 4 and out.is_contiguous()
              and tuple(out.shape[:2]) == (heads, K) and out.shape[2] >= num_keep and out.shape[3] == 2):
        raise RuntimeError("out must be contiguous fp32 [%d, %d, >= %d, 2] on the planes' device" % (heads, K, num_keep))
    index = torch.empty((heads, K, num_keep), dtype=torch.int32, device=dev) if with_index else None
    for h0, h1 in _head_groups(heads):
        with torch.cuda.device(dev), _timing.timed("point_select many", out):
            rc = _lib.lib().pct_point_select_uncertain_many_f32(
                _head_table(preds[h0:h1]), h1 - h0, _part(src, h0, h1), preds[0].numel() // (H * W), H, W,
                cand_coords[h0:h1].data_ptr(), K, S, num_keep, out[h0:h1].data_ptr(), int(out.shape[2]), _part(index, h0, h1),
                torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "point_select_uncertain_many")
    return out, index


def loss_many_supported(preds, tgt_planes):
    """Heads of one shape, dtype and device that each pass `loss_supported`."""
    return _heads_alike(preds) and all(loss_supported(p, tgt_planes) for p in preds)


def point_mask_loss_forward_many(preds, src_index, tgt_planes, tgt_index, coords):
    """-> (x [heads, K, P], t [heads, K, P], sums [heads, K, 4]) of pct_point_mask_loss_forward_many_f32; src_index, tgt_index
    int32 [heads, K] on the device, coords [heads, K, P, 2]."""
    if not preds[0].is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = preds[0].device
    H, W = preds[0].shape[-2:]
    Ht, Wt = tgt_planes.shape[-2:]
    heads, K, P = len(preds), int(coords.shape[1]), int(coords.shape[2])
    src, tgt = _index_many(src_index, heads, K, dev), _index_many(tgt_index, heads, K, dev)
    x = torch.empty((heads, K, P), dtype=torch.float32, device=dev)
    t = torch.empty((heads, K, P), dtype=torch.float32, device=dev)
    sums = (torch.zeros if P == 0 else torch.empty)((heads, K, 4), dtype=torch.float32, device=dev)
    for h0, h1 in _head_groups(heads):
        with torch.cuda.device(dev), _timing.timed("point_loss forward many", x):
            rc = _lib.lib().pct_point_mask_loss_forward_many_f32(
                _head_table(preds[h0:h1]), h1 - h0, _part(src, h0, h1), preds[0].numel() // (H * W), H, W, tgt_planes.data_ptr(),
                _part(tgt, h0, h1), tgt_planes.numel() // (Ht * Wt), Ht, Wt, coords[h0:h1].data_ptr(), K, P, x[h0:h1].data_ptr(),
                t[h0:h1].data_ptr(), sums[h0:h1].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "point_mask_loss_forward_many")
    return x, t, sums


class PointMaskLossManyFunction(torch.autograd.Function):
    """(pred_masks of every head, each [B, Q, H, W]) -> (loss_mask [heads], loss_dice [heads]).  Saves per head what
    PointMaskLossFunction saves, stacked; the backward is ONE call of the single-head backward entry on heads * K pairs (it never
    reads a prediction), its compact planes placed into each head's zero gradient."""

    @staticmethod
    def forward(ctx, src_index, tgt_planes, tgt_index, coords, num_masks, *preds):
        x, t, sums = point_mask_loss_forward_many(preds, src_index, tgt_planes, tgt_index, coords)
        P = coords.shape[2]
        loss_mask = sums[:, :, 0].sum(1) / P / num_masks
        loss_dice = (1 - (2 * sums[:, :, 1] + 1) / (sums[:, :, 2] + sums[:, :, 3] + 1)).sum(1) / num_masks
        ctx.save_for_backward(x, t, coords, sums, src_index)
        ctx.num_masks, ctx.shape, ctx.dtype = float(num_masks), tuple(preds[0].shape), preds[0].dtype
        return loss_mask, loss_dice

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mask, grad_dice):
        x, t, coords, sums, src_index = ctx.saved_tensors
        heads, K, P = x.shape
        H, W = ctx.shape[-2:]
        needs = ctx.needs_input_grad[5:]
        if not any(needs):
            return (None,) * (5 + heads)
        num = 2 * sums[:, :, 1] + 1
        den = sums[:, :, 2] + sums[:, :, 3] + 1
        gd = (grad_dice.float() / ctx.num_masks)[:, None]
        alpha = (grad_mask.float() / (P * ctx.num_masks))[:, None].expand(heads, K)
        beta = gd * num / (den * den)
        gamma = 2 * gd / den
        planes = point_mask_loss_backward(x.view(heads * K, P), t.view(heads * K, P), coords.view(heads * K, P, 2),
                                          alpha.reshape(-1), beta.reshape(-1), gamma.reshape(-1), H, W).view(heads, K, H, W)
        rows = src_index.long()
        grads = []
        for h in range(heads):
            if not needs[h]:
                grads.append(None)
                continue
            grad = torch.zeros(ctx.shape, dtype=torch.float32, device=x.device)
            grad.view(-1, H, W)[rows[h]] = planes[h]                      # matched planes are distinct: a placement
            grads.append(grad.to(ctx.dtype))
        return (None,) * 5 + tuple(grads)


def point_mask_losses_many(preds, src_index, tgt_planes, tgt_index, coords, num_masks):
    """`point_mask_losses` of every head with one forward launch and one backward launch.  preds: a sequence of [B, Q, H, W] fp32
    contiguous device tensors of one shape (each differentiable); src_index, tgt_index [heads, K]; tgt_planes [sum G, Ht, Wt]
    shared by the heads; coords [heads, K, P, 2].  -> (loss_mask [heads], loss_dice [heads]); head h equals
    point_mask_losses(preds[h], src_index[h], tgt_planes, tgt_index[h], coords[h], num_masks) up to the order of its K-term sum,
    and its gradient bit for bit."""
    preds = list(preds)
    if not loss_many_supported(preds, tgt_planes):
        raise RuntimeError("point_mask_losses_many needs contiguous fp32 device planes of one shape, predictions at most %d wide"
                           % MAX_WIDTH)
    dev = preds[0].device
    coords = coords.detach().to(device=dev, dtype=torch.float32).contiguous()
    if coords.dim() != 4 or coords.shape[0] != len(preds) or coords.shape[3] != 2:
        raise RuntimeError("coords must be [heads, K, P, 2]")
    heads, K = len(preds), int(coords.shape[1])
    src_index, tgt_index = _index_many(src_index, heads, K, dev), _index_many(tgt_index, heads, K, dev)
    if src_index is None or tgt_index is None:
        raise RuntimeError("point_mask_losses_many needs src_index and tgt_index [heads, K]")
    if K == 0 or coords.shape[2] == 0:
        zero = torch.stack([p.sum() * 0 for p in preds])
        return zero, zero.clone()
    return PointMaskLossManyFunction.apply(src_index, tgt_planes.detach(), tgt_index, coords, float(num_masks), *preds)


def match_costs_many_supported(preds, tgt_planes, num_points=1, max_targets=1):
    """Heads of one shape, dtype and device that each pass `match_cost_supported`, a group of heads times the images within the
    launch grid."""
    return (_heads_alike(preds) and all(match_cost_supported(p, tgt_planes, num_points, max_targets) for p in preds)
            and min(len(preds), MAX_HEADS) * preds[0].shape[0] <= MATCH_MAX_BATCH)


def match_cost_many_workspace_bytes(num_heads, batch, num_query, max_targets, num_points):
    """The workspace formula of the header: the single-head size, planned for `batch` images, once per head."""
    return num_heads * match_cost_workspace_bytes(batch, num_query, max_targets, num_points)


def match_costs_many(preds, tgt_planes, starts, counts, coords, cost_mask, cost_dice, max_targets=None):
    """`match_costs` of every head in one call (pct_point_match_cost_many_f32; more than MAX_HEADS heads in groups).  preds: a
    sequence of [B, Q, H, W] fp32 contiguous device tensors of one shape; coords [heads, B, P, 2], head h's rows at [h].
    -> cost [heads, B, Q, max_targets] fp32; cost[h] holds the bits of match_costs(preds[h], ..., coords[h], ...).  No gradient."""
    preds = list(preds)
    if not preds or not all(torch.is_tensor(p) and p.is_cuda for p in preds):
        raise RuntimeError("Not implemented on the CPU")
    dev = preds[0].device
    starts = starts.to(device=dev, dtype=torch.int32).contiguous()
    counts = counts.to(device=dev, dtype=torch.int32).contiguous()
    gmax = int(counts.max()) if max_targets is None else int(max_targets)
    coords = coords.detach().to(device=dev, dtype=torch.float32).contiguous()
    heads = len(preds)
    if coords.dim() != 4 or coords.shape[3] != 2 or tuple(coords.shape[:2]) != (heads, preds[0].shape[0]):
        raise RuntimeError("coords must be [heads, B, P, 2]")
    P = int(coords.shape[2])
    if not match_costs_many_supported(preds, tgt_planes, P, gmax):
        raise RuntimeError("match_costs_many needs contiguous fp32 device planes, preds [B, Q, H, W] of one shape, at least one "
                           "point and target")
    B, Q, H, W = preds[0].shape
    if tuple(starts.shape) != (B,) or tuple(counts.shape) != (B,):
        raise RuntimeError("starts and counts must be vectors of %d entries" % B)
    Ht, Wt = tgt_planes.shape[-2:]
    cost = torch.empty((heads, B, Q, gmax), dtype=torch.float32, device=dev)
    per_head = match_cost_workspace_bytes(B, Q, gmax, P) // 4
    ws = torch.empty(min(heads, MAX_HEADS) * per_head, dtype=torch.float32, device=dev)     # groups run one after the other
    for h0, h1 in _head_groups(heads):
        with torch.cuda.device(dev), _timing.timed("point_match_cost many", cost):
            rc = _lib.lib().pct_point_match_cost_many_f32(
                _head_table(preds[h0:h1]), h1 - h0, B, Q, H, W, tgt_planes.data_ptr(), int(tgt_planes.shape[0]), Ht, Wt,
                starts.data_ptr(), counts.data_ptr(), gmax, coords[h0:h1].data_ptr(), P, float(cost_mask), float(cost_dice),
                ws.data_ptr(), cost[h0:h1].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "point_match_cost_many")
    return cost

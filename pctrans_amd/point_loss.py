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
PCT_MATCH_COST)."""
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


def default():
    """Process default of `SetCriterion.point_loss` / `Point_HungarianMatcher.point_sample`: PCT_POINT_LOSS = hip | torch
    (default torch)."""
    v = os.environ.get("PCT_POINT_LOSS") or "torch"
    if v not in ("hip", "torch"):
        raise RuntimeError("PCT_POINT_LOSS must be 'hip' or 'torch', got %r" % v)
    return v


def select_default():
    """Process default of `SetCriterion.point_select`: PCT_POINT_SELECT = hip | torch (default torch)."""
    v = os.environ.get("PCT_POINT_SELECT") or "torch"
    if v not in ("hip", "torch"):
        raise RuntimeError("PCT_POINT_SELECT must be 'hip' or 'torch', got %r" % v)
    return v


def match_cost_default():
    """Process default of `Point_HungarianMatcher.match_cost`: PCT_MATCH_COST = hip | torch (default torch)."""
    v = os.environ.get("PCT_MATCH_COST") or "torch"
    if v not in ("hip", "torch"):
        raise RuntimeError("PCT_MATCH_COST must be 'hip' or 'torch', got %r" % v)
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

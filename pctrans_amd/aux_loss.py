"""Python entry of the criterion's two small losses on the device (C ABI `pct_refpoint_l1_forward_f32`,
`pct_refpoint_l1_backward_f32`, `pct_sigmoid_focal_strided_forward_f32`, `pct_sigmoid_focal_strided_backward_f32`,
include/pctrans_hip_aux_loss.h; kernels pctrans_amd/csrc/aux_losses.hip).

`refpoint_l1_losses` is SetCriterion.loss_refpoints of ALL supervised heads of a step -- gather, l1_loss, sum, division -- in one
launch, with a one-launch backward that writes the whole gradient of the stacked reference points.  `sem_focal_loss` is
SetCriterion.loss_sem -- the strided slice of the foreground maps, the cast, the count and sigmoid_focal_loss with gamma = 2 -- in
two launches forward and one backward.  No host synchronisation, bit-identical from call to call.  SetCriterion does not call
them yet: `refpoint_default()` / `sem_default()` (PCT_REFPOINT_LOSS, PCT_SEM_LOSS; default "torch") are the process defaults
its two switches will take."""
import os

import torch

from . import _lib, _timing

MAX_HEADS = 16                        # PCT_POINT_MAX_HEADS
MAX_DIMS = 8                          # csrc/aux_losses.hip: RP_MAX_DIMS
FOCAL_WORKSPACE_BYTES = 2048          # PCT_FOCAL_WORKSPACE_BYTES
FG_DTYPES = {torch.bool: 0, torch.uint8: 0, torch.float32: 4}     # fg_dtype of include/pctrans_hip_aux_loss.h


def refpoint_default():
    """Process default of the criterion's reference-point switch: PCT_REFPOINT_LOSS = hip | torch (default torch)."""
    return _lib.env_switch("PCT_REFPOINT_LOSS")


def sem_default():
    """Process default of the criterion's semantic-loss switch: PCT_SEM_LOSS = hip | torch (default torch)."""
    return _lib.env_switch("PCT_SEM_LOSS")


def _device_fp32(t, dim):
    return (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == dim and t.is_contiguous())


def supported_refpoint(points, target_points):
    """The library present, no autocast, CUDA fp32 contiguous points [heads <= MAX_HEADS, rows < 2^31 - 1, dims <= MAX_DIMS] and
    target_points [num_targets, dims] on one device: what the kernels cover."""
    if not (_device_fp32(points, 3) and _device_fp32(target_points, 2)) or points.device != target_points.device:
        return False
    if torch.is_autocast_enabled("cuda") or not os.path.exists(_lib.LIB_PATH):
        return False
    heads, rows, dims = points.shape
    return (0 < heads <= MAX_HEADS and 0 < dims <= MAX_DIMS and rows < 2 ** 31 - 1 and target_points.shape[1] == dims
            and target_points.shape[0] < 2 ** 31 - 1)


def strided_size(size, stride):
    """len(range(stride // 2, size, stride)): the length of the slice [stride // 2::stride] of `size` elements."""
    return max(0, -(-(size - stride // 2) // stride))


def _focal_geometry(logits, fg, stride):
    """(batch, out_h, out_w, height, width), or None when logits [N, h, w] / [N, 1, h, w] are not the strided slice of fg [N, H, W]."""
    if logits.dim() == 4 and logits.shape[1] == 1:
        N, h, w = logits.shape[0], logits.shape[2], logits.shape[3]
    elif logits.dim() == 3:
        N, h, w = logits.shape
    else:
        return None
    if fg.dim() != 3 or fg.shape[0] != N or stride < 1:
        return None
    H, W = fg.shape[1:]
    if N == 0 or h == 0 or w == 0 or h != strided_size(H, stride) or w != strided_size(W, stride):
        return None
    return N, h, w, H, W


def supported_sem(logits, fg, stride):
    """The library present, no autocast, CUDA fp32 contiguous logits [N, h, w] or [N, 1, h, w], a contiguous bool / uint8 / fp32
    fg [N, H, W] on the same device with (h, w) the size of fg[:, stride // 2::stride, stride // 2::stride], fewer than 2^31 - 1
    outputs: what the kernels cover."""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous()):
        return False
    if not (torch.is_tensor(fg) and fg.device == logits.device and fg.dtype in FG_DTYPES and fg.is_contiguous()):
        return False
    if torch.is_autocast_enabled("cuda") or not os.path.exists(_lib.LIB_PATH):
        return False
    return _focal_geometry(logits, fg, stride) is not None and logits.numel() < 2 ** 31 - 1


def dense_maps(maps):
    """The images' maps as one [N, H, W] tensor.  Maps that are consecutive slices of one dense buffer (how the device target
    path makes them) come back as a view of it: nothing is copied.  Anything else is torch.stack(maps), which promotes a float
    map among bool ones to fp32."""
    first = maps[0]
    if (all(torch.is_tensor(m) and m.dim() == 2 and m.is_contiguous() and m.dtype == first.dtype and m.shape == first.shape
            and m.device == first.device for m in maps) and first.numel() > 0):
        step = first.numel()
        store = first.untyped_storage().data_ptr()
        if all(m.untyped_storage().data_ptr() == store and m.storage_offset() == first.storage_offset() + n * step
               for n, m in enumerate(maps)):
            return first.as_strided((len(maps),) + tuple(first.shape), (step, first.shape[1], 1), first.storage_offset())
    return torch.stack(list(maps))


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def refpoint_l1_forward(points, target_points, src, tgt, num_masks):
    """-> (loss [heads] fp32, status [] int32) of pct_refpoint_l1_forward_f32.  src, tgt: int32 [heads, pairs]."""
    if not points.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = points.device
    heads, rows, dims = points.shape
    pairs = int(src.shape[1])
    loss = torch.empty(heads, dtype=torch.float32, device=dev)
    status = torch.empty((), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _timing.timed("refpoint_l1 forward", loss):
        rc = _lib.lib().pct_refpoint_l1_forward_f32(
            _ptr(points), _ptr(target_points), _ptr(src), _ptr(tgt), heads, rows, dims, int(target_points.shape[0]), pairs,
            float(num_masks), loss.data_ptr(), status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "refpoint_l1_forward")
    return loss, status


def refpoint_l1_backward(points, target_points, src, tgt, num_masks, grad_loss):
    """-> grad_points [heads, rows, dims] fp32 of pct_refpoint_l1_backward_f32, every element written."""
    if not points.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = points.device
    heads, rows, dims = points.shape
    grad_loss = grad_loss.detach().to(device=dev, dtype=torch.float32).contiguous()
    grad = torch.empty_like(points)
    with torch.cuda.device(dev), _timing.timed("refpoint_l1 backward", grad):
        rc = _lib.lib().pct_refpoint_l1_backward_f32(
            _ptr(points), _ptr(target_points), _ptr(src), _ptr(tgt), grad_loss.data_ptr(), heads, rows, dims,
            int(target_points.shape[0]), int(src.shape[1]), float(num_masks), _ptr(grad),
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "refpoint_l1_backward")
    return grad


def sem_focal_forward(logits, fg, stride, alpha):
    """-> (loss [] fp32, num_pos [] fp32) of pct_sigmoid_focal_strided_forward_f32."""
    if not logits.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    geo = _focal_geometry(logits, fg, stride)
    if geo is None or fg.dtype not in FG_DTYPES:
        raise RuntimeError("sem_focal_forward: logits %s are not the stride-%d slice of a bool / uint8 / fp32 map %s"
                           % (tuple(logits.shape), stride, tuple(fg.shape)))
    dev = logits.device
    N, h, w, H, W = geo
    # two allocations: the caller may scale the loss in place, and the backward's saved num_pos must not share its version counter
    loss = torch.empty((), dtype=torch.float32, device=dev)
    num_pos = torch.empty((), dtype=torch.float32, device=dev)
    ws = torch.empty(FOCAL_WORKSPACE_BYTES // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("sem_focal forward", loss):
        rc = _lib.lib().pct_sigmoid_focal_strided_forward_f32(
            logits.data_ptr(), fg.data_ptr(), FG_DTYPES[fg.dtype], N, h, w, H, W, int(stride), float(alpha), ws.data_ptr(),
            loss.data_ptr(), num_pos.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "sigmoid_focal_strided_forward")
    return loss, num_pos


def sem_focal_backward(logits, fg, stride, alpha, num_pos, grad_loss):
    """-> grad_logits (the logits' shape) fp32 of pct_sigmoid_focal_strided_backward_f32, every element written."""
    if not logits.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = logits.device
    N, h, w, H, W = _focal_geometry(logits, fg, stride)
    grad_loss = grad_loss.detach().to(device=dev, dtype=torch.float32).contiguous()
    grad = torch.empty_like(logits)
    with torch.cuda.device(dev), _timing.timed("sem_focal backward", grad):
        rc = _lib.lib().pct_sigmoid_focal_strided_backward_f32(
            logits.data_ptr(), fg.data_ptr(), FG_DTYPES[fg.dtype], num_pos.data_ptr(), grad_loss.data_ptr(), N, h, w, H, W,
            int(stride), float(alpha), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "sigmoid_focal_strided_backward")
    return grad


class RefPointL1Function(torch.autograd.Function):
    """(points [heads, rows, dims]) -> (loss [heads], status).  Saves the operands alone; the status word is a second,
    non-differentiable output.  The targets receive no gradient."""

    @staticmethod
    def forward(ctx, points, target_points, src, tgt, num_masks):
        loss, status = refpoint_l1_forward(points, target_points, src, tgt, num_masks)
        ctx.save_for_backward(points, target_points, src, tgt)
        ctx.num_masks = float(num_masks)
        ctx.mark_non_differentiable(status)
        return loss, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_status):
        points, target_points, src, tgt = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        return refpoint_l1_backward(points, target_points, src, tgt, ctx.num_masks, grad_loss), None, None, None, None


class SemFocalFunction(torch.autograd.Function):
    """(logits [N, h, w] or [N, 1, h, w]) -> loss [].  Saves the logits, the maps and the forward's count of positives."""

    @staticmethod
    def forward(ctx, logits, fg, stride, alpha):
        loss, num_pos = sem_focal_forward(logits, fg, stride, alpha)
        ctx.save_for_backward(logits, fg, num_pos)
        ctx.stride, ctx.alpha = int(stride), float(alpha)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        logits, fg, num_pos = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return sem_focal_backward(logits, fg, ctx.stride, ctx.alpha, num_pos, grad_loss), None, None, None


def refpoint_l1_losses(points, target_points, src, tgt, num_masks):
    """L1 loss between matched reference points and target points of every head.  points [heads, rows, dims] fp32 contiguous on
    the device (differentiable); target_points [num_targets, dims]; src, tgt int [heads, pairs]: pair k of head h matches row
    src[h, k] of points[h] with row tgt[h, k] of target_points.  -> loss [heads] = (sum of the pairs' absolute differences) /
    num_masks.  Its attribute `status` is a zero-dimensional int32 device tensor counting the pairs with an index out of range
    (they add nothing and receive no gradient); reading it is the caller's synchronisation."""
    if not supported_refpoint(points, target_points):
        raise RuntimeError("refpoint_l1_losses needs contiguous fp32 device points [heads <= %d, rows, dims <= %d] and "
                           "target_points [num_targets, dims], outside autocast" % (MAX_HEADS, MAX_DIMS))
    src = src.detach().to(device=points.device, dtype=torch.int32).contiguous()
    tgt = tgt.detach().to(device=points.device, dtype=torch.int32).contiguous()
    if src.dim() != 2 or src.shape[0] != points.shape[0] or tgt.shape != src.shape:
        raise RuntimeError("src and tgt must be [heads, pairs]")
    loss, status = RefPointL1Function.apply(points, target_points.detach(), src, tgt, num_masks)
    loss.status = status
    return loss


def sem_focal_loss(logits, fg, stride=8, alpha=0.25):
    """Sigmoid focal loss (gamma = 2) of logits [N, h, w] or [N, 1, h, w] (fp32 contiguous on the device, differentiable) against
    fg[:, stride // 2::stride, stride // 2::stride] of the bool / uint8 / fp32 maps fg [N, H, W], summed and divided by the
    clamped number of positive targets.  -> loss []."""
    if not supported_sem(logits, fg, stride):
        raise RuntimeError("sem_focal_loss needs contiguous fp32 device logits that are the stride-%d slice of contiguous "
                           "bool / uint8 / fp32 maps, outside autocast" % stride)
    return SemFocalFunction.apply(logits, fg.detach(), stride, alpha)

"""Python entry of the differentiable fused MSDeformAttn front-end (C ABI `pct_ms_deform_attn_fused_backward_f32`,
include/pctrans_hip_msda_train.h; kernels pctrans_amd/csrc/msda_fused_backward.hip around the routed backward).
`ms_deform_attn_fused_train` is a torch.autograd.Function on the raw `sampling_offsets` / `attention_weights` Linear outputs:
its forward is the eval path's one launch (MSDA.ms_deform_attn_fused_forward), its backward returns grad_value, grad_offsets and
grad_logits directly -- no locations tensor, no softmax output and no gradient of either as an autograd tensor.  MSDeformAttn takes
it when a gradient is required and its `train_front` switch is "hip" (PCT_MSDA_TRAIN); otherwise it uses the torch chain of
pixel_decoder/ops/modules/ms_deform_attn.py."""

import torch

from . import MultiScaleDeformableAttention as MSDA
from . import _lib, _timing

MAX_SAMPLES = 64        # num_levels * num_point of a record, the kernels' bound


def default():
    """Process default of MSDeformAttn's `train_front` switch: PCT_MSDA_TRAIN = hip | torch (default torch)."""
    return _lib.env_switch("PCT_MSDA_TRAIN")


def covered(value, reference_points, offsets, logits):
    """True where the Function can run: fp32 device tensors outside autocast, value [N, S, M, 16], offsets [N, Lq, M, L, P, 2]
    with P 4 or 8 and L * P <= 64, logits of N * Lq * M * L * P elements, 2-d reference points [N or 1, Lq, L, 2] that require
    no gradient (the entry returns none for them), everything on one device."""
    ts = (value, reference_points, offsets, logits)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    if torch.is_autocast_enabled("cuda") or len({t.device for t in ts}) != 1:
        return False
    if value.dim() != 4 or offsets.dim() != 6 or reference_points.dim() != 4 or reference_points.requires_grad:
        return False
    if not MSDA.fused_forward_supported(value, reference_points, offsets):
        return False
    N, S, M, D = value.shape
    Lq, L, P = offsets.shape[1], offsets.shape[3], offsets.shape[4]
    if tuple(offsets.shape) != (N, Lq, M, L, P, 2) or logits.numel() != N * Lq * M * L * P or L * P > MAX_SAMPLES:
        return False
    return tuple(reference_points.shape[1:]) == (Lq, L, 2) and reference_points.shape[0] in (1, N)


def workspace_bytes(N, Lq, M, L, P):
    """include/pctrans_hip_msda_train.h: the recomputed locations (8 bytes per sample) and weights (4 bytes per sample)."""
    return 12 * N * Lq * M * L * P


def _dense(t):
    """contiguous and 16-byte aligned (a view at an odd offset is copied)"""
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def fused_backward(value, shapes, level_start, reference_points, offsets, logits, grad_output, im2col_step=128):
    """-> (grad_value, grad_offsets, grad_logits) of ms_deform_attn(value, ref + offsets / (W_l, H_l), softmax(logits)) for the
    output gradient grad_output [N, Lq, M * 16]; shaped as value, offsets and logits.  The C entry allocates nothing; this wrapper
    takes the outputs and the workspace from torch's caching allocator, which also works inside a graph capture."""
    if not value.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if not covered(value, reference_points, offsets, logits):
        raise RuntimeError("msda_train.fused_backward: operands outside what the kernels cover (see msda_train.covered)")
    N, S, M, D = value.shape
    Lq, L, P = offsets.shape[1], offsets.shape[3], offsets.shape[4]
    if grad_output.dtype != torch.float32 or grad_output.device != value.device or grad_output.numel() != N * Lq * M * D:
        raise RuntimeError("msda_train.fused_backward: grad_output must be float32 [N, Lq, M * D] on value's device")
    if shapes.dtype != torch.int64 or level_start.dtype != torch.int64 or tuple(shapes.shape) != (L, 2) or level_start.numel() != L:
        raise RuntimeError("spatial_shapes [L, 2] and level_start_index [L] must be int64")
    v, off, lg, go = _dense(value), _dense(offsets), _dense(logits), _dense(grad_output)
    ref, batch_stride = MSDA._reference_points(reference_points.detach(), N, Lq, L, "Lq")
    grad_offsets, grad_logits = torch.empty_like(off), torch.empty_like(lg)
    if N == 0 or Lq == 0:                               # the entry launches nothing: no sample reads the value
        return torch.zeros_like(v), grad_offsets, grad_logits
    grad_value = torch.empty_like(v)
    ws = torch.empty((workspace_bytes(N, Lq, M, L, P) // 4,), dtype=torch.float32, device=value.device)
    _lib.prepare_device(value.device)
    with torch.cuda.device(value.device), _timing.timed("fused backward", value):
        rc = _lib.lib().pct_ms_deform_attn_fused_backward_f32(
            v.data_ptr(), shapes.contiguous().data_ptr(), level_start.contiguous().data_ptr(), ref.data_ptr(), batch_stride,
            off.data_ptr(), lg.data_ptr(), go.data_ptr(), N, S, M, D, L, Lq, P, int(im2col_step), ws.data_ptr(),
            grad_value.data_ptr(), grad_offsets.data_ptr(), grad_logits.data_ptr(),
            torch.cuda.current_stream(value.device).cuda_stream)
    _lib.check(rc, "ms_deform_attn_fused_backward")
    return grad_value, grad_offsets, grad_logits


class MSDeformAttnFusedFunction(torch.autograd.Function):
    """(value, offsets, logits) -> out [N, Lq, M * 16].  Saves those three; shapes, level starts and reference points are
    non-differentiable inputs kept by reference."""

    @staticmethod
    def forward(ctx, value, shapes, level_start, reference_points, offsets, logits, im2col_step):
        out = MSDA.ms_deform_attn_fused_forward(value, shapes, level_start, reference_points, offsets, logits)
        ctx.save_for_backward(value, offsets, logits)
        ctx.shapes, ctx.level_start, ctx.reference_points, ctx.im2col_step = shapes, level_start, reference_points, int(im2col_step)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        value, offsets, logits = ctx.saved_tensors
        # one entry gives all three: with only grad_value wanted the other two are the routed backward's scratch and are dropped
        gv, goff, glog = fused_backward(value, ctx.shapes, ctx.level_start, ctx.reference_points, offsets, logits,
                                        grad_out.contiguous(), ctx.im2col_step)
        need = ctx.needs_input_grad
        return (gv if need[0] else None, None, None, None, goff if need[4] else None,
                glog.view(logits.shape) if need[5] else None, None)


def ms_deform_attn_fused_train(value, shapes, level_start, reference_points, offsets, logits, im2col_step=128):
    """Differentiable MSDeformAttn middle section on the raw Linear outputs: value [N, S, M, 16], reference_points [N or 1, Lq, L,
    2], offsets [N, Lq, M, L, P, 2], logits [N, Lq, M, L * P], all contiguous fp32 on the device -> [N, Lq, M * 16], bit for bit
    the eval path's fused forward.  Anything `covered` refuses raises here."""
    if not covered(value, reference_points, offsets, logits):
        raise RuntimeError("ms_deform_attn_fused_train: operands outside what the kernels cover (see msda_train.covered)")
    return MSDeformAttnFusedFunction.apply(value, shapes, level_start, reference_points, offsets, logits, im2col_step)

"""Python entry of the fused dynamic mask head kernel (C ABI `pct_dynamic_mask_head_forward`,
include/pctrans_hip.h; kernel pctrans_amd/csrc/dyn_mask_head.hip) and of its backward
(`pct_dynamic_mask_head_backward_f32`, include/pctrans_hip_train.h; csrc/dyn_mask_head_bwd.hip).  `dynamic_mask_head_forward` is forward only;
`dynamic_mask_head_train` is the differentiable fp32 head: the same forward kernel, nothing saved but the three inputs, the
MLP recomputed inside the backward kernel.  The decoder takes it when gradients are needed and its `dmh_train` switch is
"hip" (PCT_DMH_TRAIN); otherwise it uses its differentiable batched torch formulation
(mask2former_transformer_decoder.py in this package)."""
import os

import torch

from . import _lib, _timing

_OUT = {torch.float32: 0, torch.bfloat16: 2}


def supported(mask_feats, rel_coord=True):
    return mask_feats.is_cuda and mask_feats.dim() == 4 and mask_feats.shape[1] == 16


def train_default():
    """Process default of the decoder's `dmh_train` switch: PCT_DMH_TRAIN = hip | torch (default torch)."""
    return _lib.env_switch("PCT_DMH_TRAIN")


def fused_geometry(H, W, target_size):
    """The shapes csrc/dyn_mask_head_fused.hip covers (one launch, no logits workspace): 128-pixel-wide maps, a multiple
    of 8 rows, attention-mask target an exact 1/2, 1/4 or 1/8 of the map."""
    th, tw = int(target_size[0]), int(target_size[1])
    if W != 128 or H < 8 or H % 8 or th <= 0 or tw <= 0 or H % th or W % tw or H // th != W // tw:
        return False
    return H // th in (2, 4, 8)


def dynamic_mask_head_forward(mask_feats, ref_xy, params, stride, rel_coord, target_size, out_dtype=torch.float32,
                              feats_f32=None, kernel=None):
    """mask_feats [N, 16, H, W]; ref_xy [N, Q, 2] normalised (x, y); params [N, Q, G] in parse_dynamic_params order.
    -> (logits upsampled x2 [N, Q, 2H, 2W] in `out_dtype`, attention mask bool [N, Q, th*tw], True = may not attend).
    `feats_f32`: optional fp32 contiguous copy of mask_feats made by the caller (the decoder calls this 10 times on the
    same features).  `kernel` (bf16 outputs only; tests and A/B runs): None = the one-launch kernel where its geometry
    applies, else the two-launch MFMA path; "fused" / "mfma" / "valu" force one (PCT_DMH_KERNEL sets the default)."""
    if not mask_feats.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    N, C, H, W = mask_feats.shape
    Q = params.shape[1]
    G = (C + (2 if rel_coord else 0)) * 8 + 64 + 8 + 8 + 8 + 1
    if params.shape != (N, Q, G):
        raise RuntimeError("params must be [N, Q, %d], got %s" % (G, tuple(params.shape)))
    if out_dtype not in _OUT:
        raise RuntimeError("out_dtype must be float32 or bfloat16")
    feats = feats_f32 if feats_f32 is not None else mask_feats.detach().float().contiguous()
    assert feats.shape == mask_feats.shape and feats.dtype == torch.float32 and feats.is_contiguous()
    prm = params.detach().float().contiguous()
    ref = ref_xy.detach().float().contiguous() if rel_coord else None
    if rel_coord and tuple(ref.shape) != (N, Q, 2):
        raise RuntimeError("ref_xy must be [N, Q, 2]")
    th, tw = int(target_size[0]), int(target_size[1])
    up = torch.empty((N, Q, 2 * H, 2 * W), dtype=out_dtype, device=mask_feats.device)
    amask = torch.empty((N, Q, th * tw), dtype=torch.bool, device=mask_feats.device)
    if kernel is None:
        kernel = os.environ.get("PCT_DMH_KERNEL") or None
    if kernel not in (None, "fused", "mfma", "valu"):
        raise RuntimeError("kernel must be None, 'fused', 'mfma' or 'valu'")
    if out_dtype == torch.bfloat16 and kernel in (None, "fused") and (kernel == "fused" or fused_geometry(H, W, (th, tw))):
        # bf16-autocast configuration, one pass over the pixels: the logits plane never goes to memory
        ws = torch.empty((N * ((Q + 1) // 2) * 1280,), dtype=torch.int32, device=mask_feats.device)   # 5120 B per pair
        with torch.cuda.device(mask_feats.device), _timing.timed("mask_head one-pass", feats):
            rc = _lib.lib().pct_dynamic_mask_head_forward_fused_bf16(
                feats.data_ptr(), ref.data_ptr() if rel_coord else None, prm.data_ptr(), N, C, Q, H, W, int(stride),
                1 if rel_coord else 0, th, tw, ws.data_ptr(), up.data_ptr(), amask.data_ptr(),
                torch.cuda.current_stream(mask_feats.device).cuda_stream)
        _lib.check(rc, "dynamic_mask_head_forward_fused_bf16")
        return up, amask
    if out_dtype == torch.bfloat16 and kernel != "valu":
        # bf16-autocast configuration: MLP on MFMA + streaming resize (two launches, bf16 logits workspace)
        scratch = torch.empty((N, Q, H, W), dtype=torch.bfloat16, device=mask_feats.device)
        with torch.cuda.device(mask_feats.device), _timing.timed("mask_head two-launch", feats):
            rc = _lib.lib().pct_dynamic_mask_head_forward_mfma(
                feats.data_ptr(), ref.data_ptr() if rel_coord else None, prm.data_ptr(), N, C, Q, H, W, int(stride),
                1 if rel_coord else 0, th, tw, scratch.data_ptr(), up.data_ptr(), amask.data_ptr(),
                torch.cuda.current_stream(mask_feats.device).cuda_stream)
        _lib.check(rc, "dynamic_mask_head_forward_mfma")
        return up, amask
    with torch.cuda.device(mask_feats.device):
        rc = _lib.lib().pct_dynamic_mask_head_forward(
            feats.data_ptr(), ref.data_ptr() if rel_coord else None, prm.data_ptr(), N, C, Q, H, W, int(stride),
            1 if rel_coord else 0, th, tw, _OUT[out_dtype], up.data_ptr(), amask.data_ptr(),
            torch.cuda.current_stream(mask_feats.device).cuda_stream)
    _lib.check(rc, "dynamic_mask_head_forward")
    return up, amask


def backward_workspace_bytes(N, Q, H, W, G):
    """include/pctrans_hip_train.h, pct_dynamic_mask_head_backward_f32: per-tile parameter partials + per-group feature partials."""
    return 4 * N * (((H * W + 127) // 128) * Q * G + 8 * 16 * H * W)


def dynamic_mask_head_backward(mask_feats, ref_xy, params, grad_up, stride, rel_coord):
    """Backward of the fp32 `dynamic_mask_head_forward`.  mask_feats [N, 16, H, W]; ref_xy [N, Q, 2] (ignored without
    rel_coord); params [N, Q, G]; grad_up [N, Q, 2H, 2W], the gradient of the upsampled logits.
    -> (grad_feat [N, 16, H, W], grad_ref [N, Q, 2] or None without rel_coord, grad_params [N, Q, G]), fp32, contiguous.
    Deterministic: two calls on the same operands give the same bits.  The C entry allocates nothing; this wrapper allocates
    the outputs and the partial-sum workspace (up to 72 MB at 2 x 300 queries, 128 x 128) from torch's caching allocator per
    call, which also works inside a graph capture (the capture's private pool)."""
    if not mask_feats.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    N, C, H, W = mask_feats.shape
    Q = params.shape[1]
    G = (C + (2 if rel_coord else 0)) * 8 + 64 + 8 + 8 + 8 + 1
    if params.shape != (N, Q, G):
        raise RuntimeError("params must be [N, Q, %d], got %s" % (G, tuple(params.shape)))
    if tuple(grad_up.shape) != (N, Q, 2 * H, 2 * W):
        raise RuntimeError("grad_up must be [N, Q, 2H, 2W] = %s, got %s" % ((N, Q, 2 * H, 2 * W), tuple(grad_up.shape)))
    feats = mask_feats.detach().float().contiguous()
    prm = params.detach().float().contiguous()
    gup = grad_up.detach().float().contiguous()
    ref = ref_xy.detach().float().contiguous() if rel_coord else None
    if rel_coord and tuple(ref.shape) != (N, Q, 2):
        raise RuntimeError("ref_xy must be [N, Q, 2]")
    dev = mask_feats.device
    grad_feat = torch.empty((N, C, H, W), dtype=torch.float32, device=dev)
    grad_params = torch.empty((N, Q, G), dtype=torch.float32, device=dev)
    grad_ref = torch.empty((N, Q, 2), dtype=torch.float32, device=dev) if rel_coord else None
    ws = torch.empty((max(backward_workspace_bytes(N, Q, H, W, G) // 4, 4),), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("mask_head backward", feats):
        rc = _lib.lib().pct_dynamic_mask_head_backward_f32(
            feats.data_ptr(), ref.data_ptr() if rel_coord else None, prm.data_ptr(), gup.data_ptr(), N, C, Q, H, W,
            int(stride), 1 if rel_coord else 0, ws.data_ptr(), grad_feat.data_ptr(),
            grad_ref.data_ptr() if rel_coord else None, grad_params.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "dynamic_mask_head_backward")
    return grad_feat, grad_ref, grad_params


class DynamicMaskHeadFunction(torch.autograd.Function):
    """fp32 dynamic mask head with a HIP backward: (mask_feats, ref_xy, params) -> (up_logits, attn_mask).  Saves its three
    inputs and nothing else; the attention mask carries no gradient."""

    @staticmethod
    def forward(ctx, mask_feats, ref_xy, params, stride, rel_coord, target_size):
        up, amask = dynamic_mask_head_forward(mask_feats, ref_xy, params, stride, rel_coord, target_size,
                                              out_dtype=torch.float32)
        ctx.save_for_backward(mask_feats, ref_xy, params)
        ctx.stride, ctx.rel_coord = int(stride), bool(rel_coord)
        ctx.mark_non_differentiable(amask)
        return up, amask

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_up, _grad_mask):
        mask_feats, ref_xy, params = ctx.saved_tensors
        grad_feat, grad_ref, grad_params = dynamic_mask_head_backward(mask_feats, ref_xy, params, grad_up, ctx.stride,
                                                                      ctx.rel_coord)
        need = ctx.needs_input_grad
        return (grad_feat.to(mask_feats.dtype) if need[0] else None,
                grad_ref.to(ref_xy.dtype) if need[1] and grad_ref is not None else None,
                grad_params.to(params.dtype) if need[2] else None, None, None, None)


def dynamic_mask_head_train(mask_feats, ref_xy, params, stride, rel_coord, target_size):
    """Differentiable fp32 head: -> (up_logits fp32 [N, Q, 2H, 2W], attn_mask bool [N, Q, th*tw], no gradient).  Inputs may
    be views (the decoder's transposed [Q, N, ...] tensors): autograd maps the contiguous gradients back."""
    return DynamicMaskHeadFunction.apply(mask_feats, ref_xy, params, stride, rel_coord, target_size)

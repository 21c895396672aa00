"""Instance post-processing on the device (C ABI: include/pctrans_hip_post.h; kernels: csrc/instance_post.hip): query mask
logits -> [N, H, W] int16 instance-id maps for a whole batch, in one sequence of launches on the current stream, with no host
synchronisation and no [N, Q, H, W] tensor at input resolution.  The semantics are those of MaskFormer.instance_inference with
mask_post / dice_for / mask_nms / comput_mmi (arch/maskformer.py).  MaskFormer.forward takes this path in eval mode when its
`postprocess` switch is "hip" (process default: PCT_POSTPROCESS); the default is its torch formulation.

    instance_labels(pred_masks, size, dataset)            logits [N, Q, h, w] -> labels [N, H, W] int16
    instance_masks(pred_masks, size, dataset)             the threshold stage alone -> (bits [N, Q, PW] int32, areas [N, Q] int32)
    instance_labels_from_bits(bits, areas, size, dataset) the rest

The workspace comes from a per-(device, geometry) cache, so a call allocates nothing but its outputs and a captured HIP graph
replays on the addresses it recorded.  Call once outside the capture first, as for every other entry of the package.  Two
consequences of that cache:
  * it never evicts on its own (a captured graph may hold a buffer's address): a process that evaluates images of many
    different sizes keeps one buffer per (device, N, Q, H, W) alive -- 845 MB at 128 x 100 x 512 x 512, `workspace_bytes` tells.
    `clear_workspaces()` drops them all; call it between geometries when memory matters and no captured graph uses them.
  * calls of one geometry share one buffer, so they must be ordered on one stream (or by events): two streams running the
    same geometry at the same time would overwrite each other's intermediate planes."""

import torch

from . import _lib

DATASETS = {"CVPPP": 0, "BBBC": 1}
MAX_QUERIES = 512
_WORKSPACES = {}


def default():
    """Process default of MaskFormer's `postprocess` switch: PCT_POSTPROCESS = hip | torch (default torch)."""
    return _lib.env_switch("PCT_POSTPROCESS")


def plane_words(H, W):
    """32-bit words per bit plane: 4 * ceil(H * W / 128)."""
    return 4 * ((H * W + 127) // 128)


def _r4(x):
    return (x + 3) // 4 * 4


def workspace_bytes(N, Q, H, W, with_masks=True):
    """include/pctrans_hip_post.h: pct_instance_labels_from_bits, plus the planes and areas of the one-call entries."""
    nq, pw, qw = N * Q, plane_words(H, W), (Q + 31) // 32
    words = nq * pw + _r4(nq * Q) + _r4(nq * qw) + 5 * _r4(nq) + 4 * N
    if with_masks:
        words += nq * pw + _r4(nq)
    return 4 * words


def supported(pred_masks, size, dataset):
    """The geometry the kernels cover (pctrans_hip_post.h); device tensors only."""
    H, W = int(size[0]), int(size[1])
    return (pred_masks.is_cuda and pred_masks.dim() == 4 and dataset in DATASETS
            and pred_masks.dtype in (torch.float32, torch.bfloat16) and pred_masks.shape[1] <= MAX_QUERIES
            and pred_masks.shape[0] <= 65535 and H > 0 and W > 0 and 2 * H * W + 1 < 2 ** 24 and H + W <= 8000)


def clear_workspaces():
    """Drop every cached workspace (their memory returns to torch's allocator).  Not while a captured graph that recorded a
    call of this module is still to be replayed."""
    _WORKSPACES.clear()


def _workspace(device, key, nbytes):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ws = _WORKSPACES.get((idx,) + key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=device)
        _WORKSPACES[(idx,) + key] = ws
    return ws


def _args(pred_masks, size, dataset):
    if not pred_masks.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if dataset not in DATASETS:
        raise ValueError("instance post-processing: unknown dataset %r" % (dataset,))
    if pred_masks.dim() != 4 or pred_masks.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("pred_masks must be [N, Q, h, w] float32 or bfloat16")
    return pred_masks.detach().contiguous(), int(size[0]), int(size[1])


def instance_masks(pred_masks, size, dataset):
    """Resize to `size` (bilinear, align_corners=False, fp32) + threshold on the logit -> (bits [N, Q, PW] int32 with 1 bit per
    pixel, areas [N, Q] int32)."""
    x, H, W = _args(pred_masks, size, dataset)
    N, Q, h, w = x.shape
    bits = torch.empty((N, Q, plane_words(H, W)), dtype=torch.int32, device=x.device)
    areas = torch.empty((N, Q), dtype=torch.int32, device=x.device)
    fn = _lib.lib().pct_instance_masks_bf16 if x.dtype == torch.bfloat16 else _lib.lib().pct_instance_masks_f32
    with torch.cuda.device(x.device):
        rc = fn(x.data_ptr(), N, Q, h, w, H, W, DATASETS[dataset], bits.data_ptr(), areas.data_ptr(),
                torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, "instance_masks")
    return bits, areas


def instance_labels_from_bits(bits, areas, size, dataset):
    """(bits, areas) of `instance_masks` -> labels [N, H, W] int16."""
    if not bits.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if dataset not in DATASETS:
        raise ValueError("instance post-processing: unknown dataset %r" % (dataset,))
    H, W = int(size[0]), int(size[1])
    N, Q = areas.shape
    if tuple(bits.shape) != (N, Q, plane_words(H, W)) or bits.dtype != torch.int32 or areas.dtype != torch.int32:
        raise RuntimeError("bits must be int32 [N, Q, %d] and areas int32 [N, Q]" % plane_words(H, W))
    bits, areas = bits.contiguous(), areas.contiguous()
    labels = torch.empty((N, H, W), dtype=torch.int16, device=bits.device)
    ws = _workspace(bits.device, ("bits", N, Q, H, W), workspace_bytes(N, Q, H, W, with_masks=False))
    with torch.cuda.device(bits.device):
        rc = _lib.lib().pct_instance_labels_from_bits(bits.data_ptr(), areas.data_ptr(), N, Q, H, W, DATASETS[dataset],
                                                      ws.data_ptr(), labels.data_ptr(),
                                                      torch.cuda.current_stream(bits.device).cuda_stream)
    _lib.check(rc, "instance_labels_from_bits")
    return labels


def instance_labels(pred_masks, size, dataset):
    """pred_masks [N, Q, h, w] (fp32, or bf16 under autocast) -> labels [N, H, W] int16 at size = (H, W); 0 = background."""
    x, H, W = _args(pred_masks, size, dataset)
    N, Q, h, w = x.shape
    labels = torch.empty((N, H, W), dtype=torch.int16, device=x.device)
    ws = _workspace(x.device, ("logits", N, Q, H, W), workspace_bytes(N, Q, H, W))
    fn = _lib.lib().pct_instance_labels_bf16 if x.dtype == torch.bfloat16 else _lib.lib().pct_instance_labels_f32
    with torch.cuda.device(x.device):
        rc = fn(x.data_ptr(), N, Q, h, w, H, W, DATASETS[dataset], ws.data_ptr(), labels.data_ptr(),
                torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, "instance_labels")
    return labels

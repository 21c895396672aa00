"""Python entry of the pixel-embedding loss on the device (C ABI `pct_instance_label_map_f32`,
`pct_discriminative_loss_forward_f32`, `pct_discriminative_loss_backward_f32`, include/pctrans_hip_train.h; kernels
pctrans_amd/csrc/embedding_loss.hip).

`instance_label_map` is the label map of `SetCriterion.loss_embedding` (nearest resize of every target mask, zero plane, argmax)
read straight from the full-resolution planes; `discriminative_loss` is loss/maskformer_criterion.py's function of the same name
on such a label map with a HIP backward: no torch.unique, no membership matrix, no host synchronisation, bit-identical from call
to call.  Opt-in: `SetCriterion.emb_loss` is "torch" unless set to "hip" (process default: PCT_EMB_LOSS)."""

import torch

from . import _lib, _timing

MAX_CHANNELS = 128    # csrc/embedding_loss.hip: EL_MAX_E (channel tiles of 32: 1, 2 or 4 of them)
MAX_LABELS = 1024     # EL_MAX_L, the LSAP kernel's declared target limit
PIXELS_PER_PASS = 256   # EL_SUB
MAX_CHUNKS = 64       # EL_MAX_CHUNKS
SLOT = 34             # EL_SLOT: floats of a workspace slot up to 32 channels (`channel_slots(E) + 2` in general)
TABLE_ROW = 68        # EL_ROW: floats of a table row up to 32 channels (`table_row(E)` in general)
UNSUPPORTED = -4      # PCT_ERR_UNSUPPORTED


def default():
    """Process default of `SetCriterion.emb_loss`: PCT_EMB_LOSS = hip | torch (default torch)."""
    return _lib.env_switch("PCT_EMB_LOSS")


def supported(embedding, num_labels):
    """CUDA fp32 contiguous [B, E <= MAX_CHANNELS, h, w] with h * w < 2^31 - 1 and 1 <= num_labels <= MAX_LABELS: what the loss
    kernels cover."""
    return (torch.is_tensor(embedding) and embedding.is_cuda and embedding.dtype == torch.float32 and embedding.dim() == 4
            and embedding.is_contiguous() and 0 < embedding.shape[0] <= 65535 and 1 <= embedding.shape[1] <= MAX_CHANNELS
            and 0 < embedding.shape[2] * embedding.shape[3] < 2 ** 31 - 1 and 1 <= int(num_labels) <= MAX_LABELS)


def chunks(pixels):
    """(passes of PIXELS_PER_PASS pixels per chunk, chunks) of include/pctrans_hip_train.h."""
    return _lib.chunk_plan(pixels, PIXELS_PER_PASS, MAX_CHUNKS)


def channel_slots(channels):
    """nch of include/pctrans_hip_train.h: 32, 64 or 128 channel slots for up to 32, 64, 128 channels."""
    return 32 if channels <= 32 else 64 if channels <= 64 else 128


def table_row(channels):
    """Floats of one label's row of the table: n_g, c_g, sum (r - delta_v)^2, 0, mu_g[nch], T_g[nch]."""
    return 4 + 2 * channel_slots(channels)


def workspace_bytes(batch, pixels, num_labels, channels=32):
    """The workspace formula of include/pctrans_hip_train.h."""
    slot = channel_slots(channels) + 2
    return 4 * batch * (chunks(pixels)[1] * (slot * 32 * (num_labels // 32 + 1) + 1) + 4 * -(-num_labels // 32))


def instance_label_map(planes, starts, counts, size):
    """planes [sum G, Ht, Wt] fp32 contiguous on the device, image b owning planes starts[b] .. starts[b] + counts[b] (int32 [B]
    device tensors); size (h, w).  -> int32 [B, h, w]: 1 + the lowest g whose nearest-resized mask is positive, 0 where none is."""
    if not planes.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if not (planes.dtype == torch.float32 and planes.dim() == 3 and planes.is_contiguous()):
        raise RuntimeError("instance_label_map needs contiguous fp32 planes [n, Ht, Wt]")
    dev = planes.device
    starts = starts.to(device=dev, dtype=torch.int32).contiguous()
    counts = counts.to(device=dev, dtype=torch.int32).contiguous()
    if starts.dim() != 1 or starts.shape != counts.shape:
        raise RuntimeError("starts and counts must be vectors of one length")
    B, (h, w) = int(starts.shape[0]), (int(size[0]), int(size[1]))
    n, Ht, Wt = planes.shape
    labels = torch.empty((B, h, w), dtype=torch.int32, device=dev)
    if n == 0:                                 # no plane at all: there is no pointer to hand over, and every label is 0
        return labels.zero_()
    with torch.cuda.device(dev), _timing.timed("instance_label_map", labels):
        rc = _lib.lib().pct_instance_label_map_f32(planes.data_ptr(), n, Ht, Wt, starts.data_ptr(), counts.data_ptr(), B, h, w,
                                                   labels.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "instance_label_map")
    return labels


def discriminative_loss_forward(embedding, labels, num_labels, delta_v, delta_d, alpha, beta, gama):
    """-> (loss [] fp32, table [B, num_labels + 1, table_row(E)] fp32, status [] int32) of pct_discriminative_loss_forward_f32."""
    if not embedding.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = embedding.device
    B, E, h, w = embedding.shape
    L = int(num_labels)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    status = torch.empty((), dtype=torch.int32, device=dev)
    table = torch.empty((B, L + 1, table_row(E)), dtype=torch.float32, device=dev)
    ws = torch.empty(workspace_bytes(B, h * w, L, E) // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("discriminative_loss forward", loss):
        rc = _lib.lib().pct_discriminative_loss_forward_f32(
            embedding.data_ptr(), labels.data_ptr(), B, E, h, w, L, float(delta_v), float(delta_d), float(alpha), float(beta),
            float(gama), ws.data_ptr(), table.data_ptr(), loss.data_ptr(), status.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "discriminative_loss_forward")
    return loss, table, status


def discriminative_loss_backward(embedding, labels, table, grad_out, num_labels, delta_v):
    """-> grad_embedding [B, E, h, w] fp32 of pct_discriminative_loss_backward_f32; grad_out a zero-dimensional device tensor."""
    if not embedding.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = embedding.device
    B, E, h, w = embedding.shape
    grad_out = grad_out.detach().to(device=dev, dtype=torch.float32).reshape(()).contiguous()
    grad = torch.empty_like(embedding)
    with torch.cuda.device(dev), _timing.timed("discriminative_loss backward", grad):
        rc = _lib.lib().pct_discriminative_loss_backward_f32(
            embedding.data_ptr(), labels.data_ptr(), table.data_ptr(), grad_out.data_ptr(), B, E, h, w, int(num_labels),
            float(delta_v), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "discriminative_loss_backward")
    return grad


class DiscriminativeLossFunction(torch.autograd.Function):
    """(embedding [B, E, h, w]) -> (loss, status).  Saves the embedding, the labels and the per-label table; the status word is a
    second, non-differentiable output."""

    @staticmethod
    def forward(ctx, embedding, labels, num_labels, delta_v, delta_d, alpha, beta, gama):
        loss, table, status = discriminative_loss_forward(embedding, labels, num_labels, delta_v, delta_d, alpha, beta, gama)
        ctx.save_for_backward(embedding, labels, table)
        ctx.num_labels, ctx.delta_v = int(num_labels), float(delta_v)
        ctx.mark_non_differentiable(status)
        return loss, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_status):
        embedding, labels, table = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        return (discriminative_loss_backward(embedding, labels, table, grad_loss, ctx.num_labels, ctx.delta_v),) + (None,) * 7


def discriminative_loss(embedding, labels, num_labels, delta_v=0.5, delta_d=3, alpha=1, beta=1, gama=0.001):
    """loss/maskformer_criterion.py's discriminative_loss on the device.  embedding [B, E, h, w] fp32 contiguous (differentiable);
    labels int [B, h, w] in 0 .. num_labels, 0 the background; num_labels the largest label any image can hold (a shape, known
    on the host).  -> the loss, a zero-dimensional tensor.  Its attribute `status` is a zero-dimensional int32 device tensor
    counting the labels outside 0 .. num_labels (they count as background); reading it is the caller's synchronisation."""
    if not torch.is_tensor(embedding) or not embedding.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if not supported(embedding, num_labels):
        raise RuntimeError("discriminative_loss needs a contiguous fp32 device embedding [B, E <= %d, h, w] and "
                           "1 <= num_labels <= %d" % (MAX_CHANNELS, MAX_LABELS))
    labels = labels.detach().to(device=embedding.device, dtype=torch.int32).contiguous()
    if tuple(labels.shape) != (embedding.shape[0],) + tuple(embedding.shape[2:]):
        raise RuntimeError("labels must be [B, h, w], got %s" % (tuple(labels.shape),))
    loss, status = DiscriminativeLossFunction.apply(embedding, labels, int(num_labels), delta_v, delta_d, alpha, beta, gama)
    loss.status = status
    return loss

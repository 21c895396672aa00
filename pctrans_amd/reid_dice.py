"""Python entry of the mask side of the query-contrast ("re-id") loss on the device (C ABI `pct_reid_dice_rows_forward_f32`,
`pct_reid_dice_rows_backward_f32`, include/pctrans_hip_reid.h; kernels pctrans_amd/csrc/reid_dice.hip).

`dice_rows` is the rows of query_contrast.dice_for that select_pos_neg_mask keeps -- row k_i of image n_i for every item i --
with a HIP backward: no [N, Q, P] sigmoid tensor, no [N, Q, Q] matrix, no host synchronisation, bit-identical from call to
call.  Opt-in: `MultiScaleMaskedTransformerDecoder.reid_dice` is "torch" unless set to "hip" (process default: PCT_REID_DICE)."""

import torch

from . import _lib, _timing

MAX_QUERIES = 1024        # csrc/reid_dice.hip: RD_MAX_Q (rows per image <= Q)
MAX_CHUNKS = 128          # RD_MAX_CHUNKS
PIXELS_PER_PASS = 64      # RD_FWD_PIX
MAX_BATCH = 65535
UNSUPPORTED = -4          # PCT_ERR_UNSUPPORTED


def default():
    """Process default of `MultiScaleMaskedTransformerDecoder.reid_dice`: PCT_REID_DICE = hip | torch (default torch)."""
    return _lib.env_switch("PCT_REID_DICE")


def supported(logits, rows_per_image):
    """CUDA fp32 contiguous [N <= MAX_BATCH, Q <= MAX_QUERIES, h, w] with h * w < 2^31 - 1 and at most Q rows in every image
    (rows_per_image: the host's counts, one per image): what the kernels cover."""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4
            and logits.is_contiguous()):
        return False
    N, Q, h, w = logits.shape
    rows = [int(r) for r in rows_per_image]
    return (0 < N <= MAX_BATCH and 0 < Q <= MAX_QUERIES and 0 < h * w < 2 ** 31 - 1 and len(rows) == N
            and all(0 <= r <= Q for r in rows))


def chunks(pixels):
    """(passes of PIXELS_PER_PASS pixels per chunk, chunks) of include/pctrans_hip_reid.h."""
    return _lib.chunk_plan(pixels, PIXELS_PER_PASS, MAX_CHUNKS)


def chain_length(pixels):
    """The longest chain of fp32 additions an output of the forward passes through: the pixels of one accumulator's fmaf chain
    plus the partials of one reduction."""
    passes, n = chunks(pixels)
    return passes * PIXELS_PER_PASS + n


def workspace_bytes(batch, num_query, pixels, num_rows, backward=False):
    """The workspace formulas of include/pctrans_hip_reid.h (forward, or backward)."""
    if backward:
        return 4 * (3 * num_rows * num_query + num_rows + batch * num_query)
    return 4 * chunks(pixels)[1] * (num_rows + batch) * num_query


def dice_rows_forward(logits, image_start, key):
    """-> (D [I, Q] fp32, s [N, Q] fp32, status [] int32) of pct_reid_dice_rows_forward_f32."""
    if not logits.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = logits.device
    N, Q, h, w = logits.shape
    I = int(key.shape[0])
    dice = torch.empty((I, Q), dtype=torch.float32, device=dev)
    sums = torch.empty((N, Q), dtype=torch.float32, device=dev)
    status = torch.zeros((), dtype=torch.int32, device=dev)
    if I == 0:                                 # nothing to launch: no row, and nobody reads s
        return dice, sums.zero_(), status
    ws = torch.empty(workspace_bytes(N, Q, h * w, I) // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("reid_dice forward", dice):
        rc = _lib.lib().pct_reid_dice_rows_forward_f32(
            logits.data_ptr(), image_start.data_ptr(), key.data_ptr(), N, Q, h, w, I, ws.data_ptr(), sums.data_ptr(),
            dice.data_ptr(), status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "reid_dice_rows_forward")
    return dice, sums, status


def dice_rows_backward(logits, image_start, key, dice, sums, grad_dice):
    """-> grad_logits [N, Q, h, w] fp32 of pct_reid_dice_rows_backward_f32."""
    if not logits.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = logits.device
    N, Q, h, w = logits.shape
    I = int(key.shape[0])
    grad_dice = grad_dice.detach().to(device=dev, dtype=torch.float32).contiguous()
    grad = torch.empty_like(logits)
    ws = torch.empty(workspace_bytes(N, Q, h * w, I, backward=True) // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("reid_dice backward", grad):
        rc = _lib.lib().pct_reid_dice_rows_backward_f32(
            logits.data_ptr(), image_start.data_ptr(), key.data_ptr() if I else None, dice.data_ptr() if I else None,
            sums.data_ptr() if I else None, grad_dice.data_ptr() if I else None, N, Q, h, w, I, ws.data_ptr(), grad.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "reid_dice_rows_backward")
    return grad


class DiceRowsFunction(torch.autograd.Function):
    """(logits [N, Q, h, w]) -> (D [I, Q], status).  Saves the logits, the row list, D and s -- nothing of the logits' size
    beyond the logits themselves; the status word is a second, non-differentiable output."""

    @staticmethod
    def forward(ctx, logits, image_start, key):
        dice, sums, status = dice_rows_forward(logits, image_start, key)
        ctx.save_for_backward(logits, image_start, key, dice, sums)
        ctx.mark_non_differentiable(status)
        return dice, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dice, _grad_status):
        logits, image_start, key, dice, sums = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return dice_rows_backward(logits, image_start, key, dice, sums, grad_dice), None, None


def dice_rows(logits, image_start, key):
    """Rows of the pairwise soft dice of sigmoid masks.  logits [N, Q, h, w] fp32 contiguous on the device (differentiable);
    image_start int [N + 1]: image n owns rows image_start[n] .. image_start[n + 1] - 1; key int [I]: the query of each row
    (keys may repeat and need not be sorted).  -> D [I, Q]: D[i] is row key[i] of query_contrast.dice_for(logits[n_i]).  Its
    attribute `status` is a zero-dimensional int32 device tensor counting the rows whose key is outside [0, Q) (their rows of
    D are 0 and they receive and send no gradient); reading it is the caller's synchronisation."""
    if not torch.is_tensor(logits) or not logits.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if not (logits.dtype == torch.float32 and logits.dim() == 4 and logits.is_contiguous()
            and 0 < logits.shape[0] <= MAX_BATCH and 0 < logits.shape[1] <= MAX_QUERIES
            and 0 < logits.shape[2] * logits.shape[3] < 2 ** 31 - 1):
        raise RuntimeError("dice_rows needs contiguous fp32 device logits [N <= %d, Q <= %d, h, w]" % (MAX_BATCH, MAX_QUERIES))
    image_start = image_start.detach().to(device=logits.device, dtype=torch.int32).contiguous()
    key = key.detach().to(device=logits.device, dtype=torch.int32).contiguous()
    if image_start.dim() != 1 or image_start.shape[0] != logits.shape[0] + 1 or key.dim() != 1:
        raise RuntimeError("image_start must be [N + 1] and key [I]")
    dice, status = DiceRowsFunction.apply(logits, image_start, key)
    dice.status = status
    return dice

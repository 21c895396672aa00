"""Python entry of the query side of the query-contrast ("re-id") loss on the device and of the per-item reduction of both of its
sides (C ABI `pct_reid_nearest_positive_f32`, `pct_reid_query_rows_forward_f32`, `pct_reid_query_rows_backward_f32`,
`pct_contrast_loss_rows_f32`, include/pctrans_hip_reid_query.h; kernels pctrans_amd/csrc/reid_query.hip).

`nearest_positive` is what query_contrast._plan keeps of the [N, Q, Q] cosine table; `query_rows` is the rows of the per-image
Gram matrix that select_pos_neg_query keeps, with their cosines and a HIP backward: no [N, Q, Q, C] broadcast, no [I, Q - 1, C]
gather, bit-identical from call to call; `contrast_loss_rows` is _contrast_softplus of the criterion on such rows (or on
reid_dice.dice_rows'), loss and coefficients in one launch.  Opt-in: `MultiScaleMaskedTransformerDecoder.reid_query` and
`SetCriterion.contrast_loss` are "torch" unless set to "hip" (process defaults: PCT_REID_QUERY, PCT_CONTRAST_LOSS)."""

import torch

from . import _lib, _timing

MAX_QUERIES = 1024        # csrc/reid_query.hip: RQ_MAX_Q (rows per image <= Q)
MAX_CHANNELS = 512        # RQ_MAX_C, and channels % 4 == 0
MAX_BATCH = 65535
LANE_CHANNELS = 8         # RQ_LANE_CHANNELS: the fmaf chain of one lane's part of a dot product
WAVE_STEPS = 6            # RQ_WAVE_STEPS: the additions of the butterfly over the wave
CHAIN_LENGTH = LANE_CHANNELS + WAVE_STEPS     # the L of include/pctrans_hip_reid_query.h


def default():
    """Process default of `MultiScaleMaskedTransformerDecoder.reid_query`: PCT_REID_QUERY = hip | torch (default torch)."""
    return _lib.env_switch("PCT_REID_QUERY")


def contrast_default():
    """Process default of `SetCriterion.contrast_loss`: PCT_CONTRAST_LOSS = hip | torch (default torch)."""
    return _lib.env_switch("PCT_CONTRAST_LOSS")


def _query_ok(query):
    return (torch.is_tensor(query) and query.is_cuda and query.dtype == torch.float32 and query.dim() == 3
            and query.is_contiguous() and 0 < query.shape[0] <= MAX_QUERIES and 0 < query.shape[1] <= MAX_BATCH
            and 0 < query.shape[2] <= MAX_CHANNELS and query.shape[2] % 4 == 0 and query.data_ptr() % 16 == 0)


def supported(query, rows_per_image):
    """CUDA fp32 contiguous 16-byte aligned [Q <= MAX_QUERIES, N <= MAX_BATCH, C <= MAX_CHANNELS, C % 4 == 0] with at most Q rows
    in every image (rows_per_image: the host's counts, one per image): what the kernels cover."""
    if not _query_ok(query):
        return False
    Q, N, _ = query.shape
    rows = [int(r) for r in rows_per_image]
    return len(rows) == N and all(0 <= r <= Q for r in rows)


def workspace_bytes(num_query, channels, num_rows):
    """The backward's workspace formula of include/pctrans_hip_reid_query.h."""
    return 4 * num_rows * (channels + 2 * num_query + 1)


def _need(query):
    if not torch.is_tensor(query) or not query.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if not _query_ok(query):
        raise RuntimeError("reid_query needs a contiguous fp32 device query [Q <= %d, N <= %d, C <= %d, C %% 4 == 0]"
                           % (MAX_QUERIES, MAX_BATCH, MAX_CHANNELS))


def nearest_positive(query, pos_lists):
    """query [Q, N, C]; pos_lists: per image the matched queries in matcher order (Python ints).  -> nearest, a list of N lists
    of Q ints: the position in pos_lists[n] of the matched query that query r is most cosine-similar to (first maximum; -1 for an
    image without matched queries).  The .tolist() is the call's one device->host copy."""
    _need(query)
    Q, N, C = query.shape
    if len(pos_lists) != N:
        raise RuntimeError("pos_lists must hold one list per image")
    pmax = max((len(p) for p in pos_lists), default=0)
    if pmax == 0:
        return [[-1] * Q for _ in range(N)]
    if pmax > Q or any(not 0 <= int(k) < Q for p in pos_lists for k in p):
        raise RuntimeError("matched queries must lie in [0, %d), at most %d per image" % (Q, Q))
    dev = query.device
    pos = torch.tensor([list(p) + [-1] * (pmax - len(p)) for p in pos_lists], dtype=torch.int32).to(dev)
    nearest = torch.empty((N, Q), dtype=torch.int32, device=dev)
    query = query.detach()
    with torch.cuda.device(dev), _timing.timed("reid_query nearest", nearest):
        rc = _lib.lib().pct_reid_nearest_positive_f32(query.data_ptr(), pos.data_ptr(), Q, N, C, pmax, nearest.data_ptr(),
                                                      torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "reid_nearest_positive")
    return nearest.tolist()


def query_rows_forward(query, image_start, key):
    """-> (S [I, Q], Cs [I, Q], norm [N, Q]) fp32 of pct_reid_query_rows_forward_f32."""
    if not query.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = query.device
    Q, N, C = query.shape
    I = int(key.shape[0])
    dots = torch.empty((I, Q), dtype=torch.float32, device=dev)
    cosines = torch.empty((I, Q), dtype=torch.float32, device=dev)
    norm = torch.empty((N, Q), dtype=torch.float32, device=dev)
    if I == 0:                                 # nothing to launch: no row, and nobody reads the norms
        return dots, cosines, norm.zero_()
    with torch.cuda.device(dev), _timing.timed("reid_query forward", dots):
        rc = _lib.lib().pct_reid_query_rows_forward_f32(
            query.data_ptr(), image_start.data_ptr(), key.data_ptr(), Q, N, C, I, norm.data_ptr(), dots.data_ptr(),
            cosines.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "reid_query_rows_forward")
    return dots, cosines, norm


def query_rows_backward(query, image_start, key, norm, cosines, grad_dots, grad_cosines):
    """-> grad_query [Q, N, C] fp32 of pct_reid_query_rows_backward_f32."""
    if not query.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = query.device
    Q, N, C = query.shape
    I = int(key.shape[0])
    grad_dots = grad_dots.detach().to(device=dev, dtype=torch.float32).contiguous()
    grad_cosines = grad_cosines.detach().to(device=dev, dtype=torch.float32).contiguous()
    grad = torch.empty_like(query)
    ws = torch.empty(max(4, workspace_bytes(Q, C, I) // 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timing.timed("reid_query backward", grad):
        rc = _lib.lib().pct_reid_query_rows_backward_f32(
            query.data_ptr(), image_start.data_ptr(), key.data_ptr() if I else None, norm.data_ptr() if I else None,
            cosines.data_ptr() if I else None, grad_dots.data_ptr() if I else None, grad_cosines.data_ptr() if I else None,
            Q, N, C, I, ws.data_ptr(), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "reid_query_rows_backward")
    return grad


class QueryRowsFunction(torch.autograd.Function):
    """(query [Q, N, C]) -> (S [I, Q], Cs [I, Q]).  Saves the query, the row list, the norms and Cs."""

    @staticmethod
    def forward(ctx, query, image_start, key):
        dots, cosines, norm = query_rows_forward(query, image_start, key)
        ctx.save_for_backward(query, image_start, key, norm, cosines)
        return dots, cosines

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dots, grad_cosines):
        query, image_start, key, norm, cosines = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return query_rows_backward(query, image_start, key, norm, cosines, grad_dots, grad_cosines), None, None


def query_rows(query, image_start, key):
    """Rows of the per-image Gram matrix of the queries and their cosines.  query [Q, N, C] fp32 contiguous on the device
    (differentiable); image_start int [N + 1]: image n owns rows image_start[n] .. image_start[n + 1] - 1; key: the query of each
    row, a Python list or a tensor [I] (keys may repeat and need not be sorted; one outside [0, Q) raises: the plan is a Python
    list on the host).  -> (S, Cs), both [I, Q]: S[i, q] = <x[n_i, q], x[n_i, k_i]>, Cs[i, q] = S[i, q] / (m_q m_k) with
    m = max(|x|, 1e-12) as F.normalize."""
    _need(query)
    Q, N, _ = query.shape
    keys = key.tolist() if torch.is_tensor(key) else [int(k) for k in key]
    if any(not 0 <= k < Q for k in keys):
        raise RuntimeError("keys must lie in [0, %d)" % Q)
    image_start = torch.as_tensor(image_start).detach().to(device=query.device, dtype=torch.int32).contiguous()
    key_t = (key.detach() if torch.is_tensor(key) else torch.tensor(keys)).to(device=query.device, dtype=torch.int32).contiguous()
    if image_start.dim() != 1 or image_start.shape[0] != N + 1 or key_t.dim() != 1:
        raise RuntimeError("image_start must be [N + 1] and key [I]")
    return QueryRowsFunction.apply(query, image_start, key_t)


def contrast_loss_rows_forward(rows, image_of, key, owner, temperature):
    """-> (loss [I], coef [I, Q]) fp32 of pct_contrast_loss_rows_f32."""
    if not rows.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dev = rows.device
    I, Q = rows.shape
    N = int(owner.shape[0])
    loss = torch.empty((I,), dtype=torch.float32, device=dev)
    coef = torch.empty((I, Q), dtype=torch.float32, device=dev)
    if I == 0:
        return loss, coef
    with torch.cuda.device(dev), _timing.timed("reid_query contrast", loss):
        rc = _lib.lib().pct_contrast_loss_rows_f32(
            rows.data_ptr(), image_of.data_ptr(), key.data_ptr(), owner.data_ptr(), I, Q, N, 1.0 / float(temperature),
            loss.data_ptr(), coef.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "contrast_loss_rows")
    return loss, coef


class ContrastLossFunction(torch.autograd.Function):
    """(rows [I, Q]) -> loss [I].  Saves the coefficients d loss_i / d rows[i, q] the forward's launch wrote."""

    @staticmethod
    def forward(ctx, rows, image_of, key, owner, temperature):
        loss, coef = contrast_loss_rows_forward(rows, image_of, key, owner, temperature)
        ctx.save_for_backward(coef)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        coef, = ctx.saved_tensors
        return grad_loss[:, None] * coef, None, None, None, None


def contrast_supported(rows, image_of, key, owner):
    """What pct_contrast_loss_rows_f32 covers: fp32 device rows [I, Q <= MAX_QUERIES] with int index tensors on the same device."""
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2
            and 0 < rows.shape[1] <= MAX_QUERIES):
        return False
    return all(torch.is_tensor(t) and t.device == rows.device and not t.is_floating_point() for t in (image_of, key, owner)) \
        and image_of.shape == key.shape == rows.shape[:1] and owner.dim() == 2 and owner.shape[1] == rows.shape[1] \
        and 0 < owner.shape[0] <= MAX_BATCH


def contrast_loss_rows(rows, image_of, key, owner, temperature):
    """The per-item contrast loss of SetCriterion.loss_reid_query / loss_reid_mask on rows [I, Q] (differentiable): item i of
    image image_of[i] with its own query key[i]; owner [N, Q]: the item whose cluster holds query q, -1 for a matched query.
    -> loss [I] = softplus(lse_{negatives}(rows / temperature) + lse_{positives}(-rows / temperature)); an item without negatives
    gives exactly 0."""
    if not torch.is_tensor(rows) or not rows.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if not contrast_supported(rows, image_of, key, owner):
        raise RuntimeError("contrast_loss_rows needs fp32 device rows [I, Q <= %d] and int image_of [I], key [I], owner [N, Q]"
                           % MAX_QUERIES)
    if not float(temperature) > 0:
        raise RuntimeError("temperature must be positive")
    i32 = lambda t: t.detach().to(dtype=torch.int32).contiguous()
    return ContrastLossFunction.apply(rows.contiguous(), i32(image_of), i32(key), i32(owner), float(temperature))

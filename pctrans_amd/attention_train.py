"""Python entry of the differentiable fp32 cross-attention (C ABI `pct_cross_attention_forward_f32` /
`pct_cross_attention_backward_f32`, include/pctrans_hip_attn_train.h; kernels pctrans_amd/csrc/cross_attention_train.hip).
`cross_attention_train` is a torch.autograd.Function on the split operands the projections write -- no per-head
concatenation, no [N, heads, Q, S] tensor in forward or backward; it keeps the five operands, `out` and `lse` for the backward
and nothing else.  CrossAttentionLayer takes it when a gradient is required and its `attn_train` switch is "hip"
(PCT_ATTN_TRAIN); otherwise it uses the torch chain of transformer_decoder/attention.py.

The helpers both differentiable attention paths share live here (self_attention_train.py imports them): HEAD_DIM, _HEADS,
_dense, workspace_bytes, the operand check _operands_ok, and the allocate / launch / check steps _dense_operands, _out_and_lse,
_workspace and _call."""

import torch

from . import _lib, _timing

HEAD_DIM = 16
_HEADS = (4, 8)
# Measured as replays of a HIP graph of one forward + backward (tools/bench_attn_train.py, N = 2, 8 heads): the kernels take 0.38 -
# 0.92 x the torch chain's time up to 1 024 keys and 1.13 - 1.30 x at 3 136 and 4 096.  Key counts in between were not timed.
# Beyond MAX_KEYS the same kernels with the keys of a workgroup divided over several are the faster path
# (split_key_attention_train.py, CrossAttentionLayer.attn_train_split; profiles/attn_train_split.json).
MAX_KEYS = 1024


def default():
    """Process default of CrossAttentionLayer's `attn_train` switch: PCT_ATTN_TRAIN = hip | torch (default torch)."""
    return _lib.env_switch("PCT_ATTN_TRAIN")


def _mask_ok(attn_mask, N, Q, S, device):
    return attn_mask is None or (attn_mask.dtype == torch.bool and attn_mask.device == device
                                 and tuple(attn_mask.shape) in ((N, 1, Q, S), (N, Q, S)))


def _operands_ok(q_ops, k_ops, heads):
    """Five fp32 device tensors on one device outside autocast: q_ops [Q, N, heads * 16], k_ops [S, N, heads * 16], heads 4 or
    8, at least one query, key and image, N within the grid's z extent and every tensor below 2^31 elements."""
    ts = tuple(q_ops) + tuple(k_ops)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 for t in ts):
        return False
    if torch.is_autocast_enabled("cuda") or len({t.device for t in ts}) != 1:
        return False
    Q, N, C = q_ops[0].shape
    S = k_ops[0].shape[0]
    if heads not in _HEADS or C != heads * HEAD_DIM or min(Q, N, S) < 1 or N > 65535 or max(Q, S) * N * C >= 2 ** 31:
        return False
    return all(tuple(t.shape) == (Q, N, C) for t in q_ops) and all(tuple(t.shape) == (S, N, C) for t in k_ops)


def covered(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None):
    """True where the kernels can run: five fp32 device operands [Q | S, N, heads * 16] outside autocast, heads 4 or 8, at
    least one query, key and image, a bool mask [N, 1, Q, S] (or [N, Q, S]) or none, a bool row_open of N * Q elements or
    none, everything on one device."""
    if not _operands_ok((q_c, q_s), (k_c, k_p, v), heads):
        return False
    (Q, N, _), S = q_c.shape, k_c.shape[0]
    if not _mask_ok(attn_mask, N, Q, S, q_c.device):
        return False
    if row_open is not None and (row_open.dtype != torch.bool or row_open.device != q_c.device or row_open.numel() != N * Q):
        return False
    return True


def supported(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None):
    """What CrossAttentionLayer sends to the kernels: everything `covered` with at most MAX_KEYS keys.  Beyond that the torch chain
    is the faster one on the device (profiles/attn_train.json) and keeps the call."""
    return covered(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open) and k_c.shape[0] <= MAX_KEYS


def workspace_bytes(N, heads, Q):
    """include/pctrans_hip_attn_train.h, pct_cross_attention_backward_f32, and include/pctrans_hip_self_attn_train.h,
    pct_self_attention_backward_f32: D = rowsum(grad_out * out), one float per row."""
    return 4 * N * heads * Q


def _dense(t):
    """fp32, contiguous, 16-byte aligned (a view at an odd offset is copied)."""
    t = t.detach().float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _dense_operands(operands):
    """The five operands as the kernels read them (`_dense`)."""
    if not operands[0].is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    return [_dense(t) for t in operands]


def _out_and_lse(q_c, heads):
    Q, N, C = q_c.shape
    return (torch.empty((Q, N, C), dtype=torch.float32, device=q_c.device),
            torch.empty((2, N, heads, Q), dtype=torch.float32, device=q_c.device))


def _workspace(q_c, heads):
    """The backward's N * heads * Q floats, from torch's caching allocator (which also works inside a graph capture)."""
    Q, N, _ = q_c.shape
    return torch.empty((max(workspace_bytes(N, heads, Q) // 4, 4),), dtype=torch.float32, device=q_c.device)


def _call(name, label, ref, *args):
    """C ABI entry pct_`name` on `ref`'s device and current stream, timed as `label`; a status other than 0 raises."""
    with torch.cuda.device(ref.device), _timing.timed(label, ref):
        rc = getattr(_lib.lib(), "pct_" + name)(*args, torch.cuda.current_stream(ref.device).cuda_stream)
    _lib.check(rc, name)


def _bytes(t):
    return None if t is None else t.detach().contiguous().view(torch.uint8)


def _ptr(t):
    return None if t is None else t.data_ptr()


def cross_attention_forward(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None):
    """-> (out [Q, N, heads * 16] fp32, lse [2, N, heads, Q] fp32: row maximum + log of the row sum and its low-order word).
    A row with nothing attendable: out 0, lse 0."""
    ops = _dense_operands((q_c, q_s, k_c, k_p, v))
    (Q, N, _), S = q_c.shape, k_c.shape[0]
    m, ro = _bytes(attn_mask), _bytes(row_open)
    out, lse = _out_and_lse(q_c, heads)
    _call("cross_attention_forward_f32", "cross_attention train forward", out, *[t.data_ptr() for t in ops], _ptr(m), _ptr(ro),
          N, heads, Q, S, float(2 * HEAD_DIM) ** -0.5, out.data_ptr(), lse.data_ptr())
    return out, lse


def cross_attention_backward(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open, out, lse, grad_out):
    """-> (grad_q_c, grad_q_s, grad_k_c, grad_k_p, grad_v), fp32 contiguous in the operands' layouts.  Deterministic: two calls
    on the same operands give the same bits.  The C entry allocates nothing; this wrapper takes the outputs and the
    N * heads * Q float workspace from torch's caching allocator, which also works inside a graph capture."""
    ops = _dense_operands((q_c, q_s, k_c, k_p, v))
    (Q, N, _), S = q_c.shape, k_c.shape[0]
    l, go = _dense(lse), _dense(grad_out)
    m, ro = _bytes(attn_mask), _bytes(row_open)
    grads = [torch.empty_like(t) for t in ops]
    ws = _workspace(q_c, heads)
    _call("cross_attention_backward_f32", "cross_attention train backward", go, *[t.data_ptr() for t in ops], _ptr(m), _ptr(ro),
          out.data_ptr(), l.data_ptr(), go.data_ptr(), N, heads, Q, S, float(2 * HEAD_DIM) ** -0.5, ws.data_ptr(),
          *[g.data_ptr() for g in grads])
    return tuple(grads)


class CrossAttentionTrainFunction(torch.autograd.Function):
    """(q_c, q_s, k_c, k_p, v) -> out.  Saves the five operands, out and lse; the mask and row_open are non-differentiable
    inputs kept by reference."""

    @staticmethod
    def forward(ctx, q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open):
        out, lse = cross_attention_forward(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open)
        ctx.save_for_backward(q_c, q_s, k_c, k_p, v, out, lse)
        ctx.heads, ctx.attn_mask, ctx.row_open = int(heads), attn_mask, row_open
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q_c, q_s, k_c, k_p, v, out, lse = ctx.saved_tensors
        grads = cross_attention_backward(q_c, q_s, k_c, k_p, v, ctx.heads, ctx.attn_mask, ctx.row_open, out, lse, grad_out)
        need = ctx.needs_input_grad
        return tuple(g if need[i] else None for i, g in enumerate(grads)) + (None, None, None)


def cross_attention_train(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None):
    """Differentiable fp32 cross-attention on split operands: per head the query is [q_c | q_s] and the key [k_c | k_p], the
    score scale is 32^-0.5.  attn_mask bool [N, 1, Q, S], True = may not attend; row_open bool [N, 1, Q, 1], True = the query
    ignores its mask row.  -> out [Q, N, heads * 16].  Anything `covered` refuses raises here (`supported` adds the key count up
    to which the kernels are the faster path; that is the caller's choice, not a limit of the kernels)."""
    if not covered(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open):
        raise RuntimeError("cross_attention_train: operands outside what the kernels cover (see attention_train.covered)")
    return CrossAttentionTrainFunction.apply(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open)

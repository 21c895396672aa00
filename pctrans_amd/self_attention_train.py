"""Python entry of the differentiable fp32 self-attention (C ABI `pct_self_attention_forward_f32` /
`pct_self_attention_backward_f32`, include/pctrans_hip_self_attn_train.h; kernels pctrans_amd/csrc/self_attention_train.hip).
`self_attention_train` is a torch.autograd.Function on the five tensors SelfAttentionLayer's projections write -- the two
operand adds are made inside the kernels, there is no [N, heads, Q, Q] tensor in forward or backward; it keeps the five operands,
`out` and `lse` for the backward and nothing else.  SelfAttentionLayer takes it when a gradient is required, it has no mask and
its `self_attn_train` switch is "hip" (PCT_SELF_ATTN_TRAIN); otherwise it uses the torch chain of
transformer_decoder/attention.py."""

import torch

from . import _lib
from .attention_train import (HEAD_DIM, _call, _dense, _dense_operands, _operands_ok, _out_and_lse, _workspace,  # noqa: F401
                              workspace_bytes)

# The backward keeps k and v of one (image, head) in LDS (csrc/self_attention_train.hip: SAT_MAX_Q)
MAX_QUERIES = 512


def default():
    """Process default of SelfAttentionLayer's `self_attn_train` switch: PCT_SELF_ATTN_TRAIN = hip | torch (default torch)."""
    return _lib.env_switch("PCT_SELF_ATTN_TRAIN")


def covered(q_c, q_p, k_c, k_p, v, heads):
    """True where the kernels can run: five fp32 device operands [Q, N, heads * 16] of one shape outside autocast, heads 4 or
    8, 1 <= Q <= MAX_QUERIES, at least one image, everything on one device."""
    return _operands_ok((q_c, q_p), (k_c, k_p, v), heads) and q_c.shape[0] == k_c.shape[0] <= MAX_QUERIES


def supported(q_c, q_p, k_c, k_p, v, heads):
    """What SelfAttentionLayer sends to the kernels.  The same as `covered`: forward + backward were measured faster than the
    torch chain at every query count timed (100, 300 and 512: profiles/self_attn_train.json), so there is no speed rule."""
    return covered(q_c, q_p, k_c, k_p, v, heads)


def self_attention_forward(q_c, q_p, k_c, k_p, v, heads):
    """-> (out [Q, N, heads * 16] fp32, lse [2, N, heads, Q] fp32: row maximum + log of the row sum and its low-order word)."""
    ops = _dense_operands((q_c, q_p, k_c, k_p, v))
    Q, N, _ = q_c.shape
    out, lse = _out_and_lse(q_c, heads)
    _call("self_attention_forward_f32", "self_attention train forward", out, *[t.data_ptr() for t in ops], N, heads, Q,
          float(HEAD_DIM) ** -0.5, out.data_ptr(), lse.data_ptr())
    return out, lse


def self_attention_backward(q_c, q_p, k_c, k_p, v, heads, out, lse, grad_out):
    """-> (grad_q, grad_k, grad_v), fp32 contiguous in the operands' layout; grad_q is the gradient of q_c and of q_p, grad_k
    that of k_c and of k_p.  Deterministic: two calls on the same operands give the same bits.  The C entry allocates nothing;
    this wrapper takes the outputs and the N * heads * Q float workspace from torch's caching allocator, which also works
    inside a graph capture."""
    ops = _dense_operands((q_c, q_p, k_c, k_p, v))
    Q, N, C = q_c.shape
    l, go = _dense(lse), _dense(grad_out)
    grads = [torch.empty((Q, N, C), dtype=torch.float32, device=q_c.device) for _ in range(3)]
    ws = _workspace(q_c, heads)
    _call("self_attention_backward_f32", "self_attention train backward", go, *[t.data_ptr() for t in ops], out.data_ptr(),
          l.data_ptr(), go.data_ptr(), N, heads, Q, float(HEAD_DIM) ** -0.5, ws.data_ptr(), *[g.data_ptr() for g in grads])
    return tuple(grads)


class SelfAttentionTrainFunction(torch.autograd.Function):
    """(q_c, q_p, k_c, k_p, v) -> out.  Saves the five operands, out and lse."""

    @staticmethod
    def forward(ctx, q_c, q_p, k_c, k_p, v, heads):
        out, lse = self_attention_forward(q_c, q_p, k_c, k_p, v, heads)
        ctx.save_for_backward(q_c, q_p, k_c, k_p, v, out, lse)
        ctx.heads = int(heads)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q_c, q_p, k_c, k_p, v, out, lse = ctx.saved_tensors
        gq, gk, gv = self_attention_backward(q_c, q_p, k_c, k_p, v, ctx.heads, out, lse, grad_out)
        need = ctx.needs_input_grad
        return tuple(g if need[i] else None for i, g in enumerate((gq, gq, gk, gk, gv))) + (None,)


def self_attention_train(q_c, q_p, k_c, k_p, v, heads):
    """Differentiable fp32 self-attention on the projections' outputs: per head q = q_c + q_p, k = k_c + k_p, the score scale
    is 16^-0.5, no mask.  -> out [Q, N, heads * 16].  Anything `covered` refuses raises here."""
    if not covered(q_c, q_p, k_c, k_p, v, heads):
        raise RuntimeError("self_attention_train: operands outside what the kernels cover (see self_attention_train.covered)")
    return SelfAttentionTrainFunction.apply(q_c, q_p, k_c, k_p, v, heads)

"""Python entry of the differentiable fp32 self-attention (C ABI `pct_self_attention_forward_f32` /
`pct_self_attention_backward_f32`, include/pctrans_hip_self_attn_train.h; kernels pctrans_amd/csrc/self_attention_train.hip).
`self_attention_train` is a torch.autograd.Function on the five tensors SelfAttentionLayer's projections write -- the two
operand adds are made inside the kernels, there is no [N, heads, Q, Q] tensor in forward or backward; it keeps the five operands,
`out` and `lse` for the backward and nothing else.  SelfAttentionLayer takes it when a gradient is required, it has no mask and
its `self_attn_train` switch is "hip" (PCT_SELF_ATTN_TRAIN); otherwise it uses the torch chain of
transformer_decoder/attention.py."""

import torch

from . import _lib, _timing

HEAD_DIM = 16
_HEADS = (4, 8)
# The backward keeps k and v of one (image, head) in LDS (csrc/self_attention_train.hip: SAT_MAX_Q)
MAX_QUERIES = 512


def default():
    """Process default of SelfAttentionLayer's `self_attn_train` switch: PCT_SELF_ATTN_TRAIN = hip | torch (default torch)."""
    return _lib.env_switch("PCT_SELF_ATTN_TRAIN")


def covered(q_c, q_p, k_c, k_p, v, heads):
    """True where the kernels can run: five fp32 device operands [Q, N, heads * 16] of one shape outside autocast, heads 4 or
    8, 1 <= Q <= MAX_QUERIES, at least one image, everything on one device."""
    ts = (q_c, q_p, k_c, k_p, v)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 for t in ts):
        return False
    if torch.is_autocast_enabled("cuda"):
        return False
    Q, N, C = q_c.shape
    if heads not in _HEADS or C != heads * HEAD_DIM or min(Q, N) < 1 or N > 65535 or Q > MAX_QUERIES:
        return False
    if any(tuple(t.shape) != (Q, N, C) for t in ts[1:]):
        return False
    return Q * N * C < 2 ** 31 and len({t.device for t in ts}) == 1


def supported(q_c, q_p, k_c, k_p, v, heads):
    """What SelfAttentionLayer sends to the kernels.  The same as `covered`: forward + backward were measured faster than the
    torch chain at every query count timed (100, 300 and 512: profiles/self_attn_train.json), so there is no speed rule."""
    return covered(q_c, q_p, k_c, k_p, v, heads)


def workspace_bytes(N, heads, Q):
    """include/pctrans_hip_self_attn_train.h, pct_self_attention_backward_f32: D = rowsum(grad_out * out), one float per row."""
    return 4 * N * heads * Q


def _dense(t):
    """fp32, contiguous, 16-byte aligned (a view at an odd offset is copied)."""
    t = t.detach().float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def self_attention_forward(q_c, q_p, k_c, k_p, v, heads):
    """-> (out [Q, N, heads * 16] fp32, lse [2, N, heads, Q] fp32: row maximum + log of the row sum and its low-order word)."""
    if not q_c.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    Q, N, C = q_c.shape
    ops = [_dense(t) for t in (q_c, q_p, k_c, k_p, v)]
    out = torch.empty((Q, N, C), dtype=torch.float32, device=q_c.device)
    lse = torch.empty((2, N, heads, Q), dtype=torch.float32, device=q_c.device)
    with torch.cuda.device(q_c.device), _timing.timed("self_attention train forward", out):
        rc = _lib.lib().pct_self_attention_forward_f32(
            *[t.data_ptr() for t in ops], N, heads, Q, float(HEAD_DIM) ** -0.5, out.data_ptr(), lse.data_ptr(),
            torch.cuda.current_stream(q_c.device).cuda_stream)
    _lib.check(rc, "self_attention_forward_f32")
    return out, lse


def self_attention_backward(q_c, q_p, k_c, k_p, v, heads, out, lse, grad_out):
    """-> (grad_q, grad_k, grad_v), fp32 contiguous in the operands' layout; grad_q is the gradient of q_c and of q_p, grad_k
    that of k_c and of k_p.  Deterministic: two calls on the same operands give the same bits.  The C entry allocates nothing;
    this wrapper takes the outputs and the N * heads * Q float workspace from torch's caching allocator, which also works
    inside a graph capture."""
    if not q_c.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    Q, N, C = q_c.shape
    ops = [_dense(t) for t in (q_c, q_p, k_c, k_p, v)]
    l, go = _dense(lse), _dense(grad_out)
    grads = [torch.empty((Q, N, C), dtype=torch.float32, device=q_c.device) for _ in range(3)]
    ws = torch.empty((max(workspace_bytes(N, heads, Q) // 4, 4),), dtype=torch.float32, device=q_c.device)
    with torch.cuda.device(q_c.device), _timing.timed("self_attention train backward", go):
        rc = _lib.lib().pct_self_attention_backward_f32(
            *[t.data_ptr() for t in ops], out.data_ptr(), l.data_ptr(), go.data_ptr(), N, heads, Q, float(HEAD_DIM) ** -0.5,
            ws.data_ptr(), *[g.data_ptr() for g in grads], torch.cuda.current_stream(q_c.device).cuda_stream)
    _lib.check(rc, "self_attention_backward_f32")
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

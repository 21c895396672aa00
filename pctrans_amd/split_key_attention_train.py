"""Python entry of the differentiable fp32 cross-attention with the keys divided over several workgroups (C ABI
`pct_cross_attention_split_forward_f32` / `pct_cross_attention_split_backward_f32`, include/pctrans_hip_attn_train_split.h; kernels
pctrans_amd/csrc/cross_attention_train_split.hip).  The kernels behind attention_train.py give one workgroup to 16 queries of one
(image, head), and that workgroup walks all the keys: 2 images with 100 queries and 8 heads are 112 workgroups on 256 compute
units, each wave of which makes 49 dependent steps at 3 136 keys.  Here the 64-key chunks of such a workgroup are divided over
`splits` workgroups in the forward and in both sweeps of the backward's query pass; partial results go to a workspace and small
launches combine them in a fixed order (forward 2 launches, backward 4).  `splits` == 1 gives attention_train's bits in all seven
results, and so does any split count on a query whose live keys all lie in one split's range.  CrossAttentionLayer sends its fp32
training calls here when its `attn_train_split` switch is "hip" (PCT_ATTN_TRAIN_SPLIT) and `plan` finds at least two splits; the
default is "torch", today's routing.  The helpers of attention_train.py are used as they are."""

import torch

from . import _lib, attention_train
from .attention_train import HEAD_DIM, _bytes, _call, _dense, _dense_operands, _out_and_lse, _ptr

CHUNK = 64                       # keys per chunk (csrc/cross_attention_train_split.hip: XS_CHUNK)
# The plan: as many splits as bring the query-side grid to TARGET_WORKGROUPS, each with at least MIN_CHUNKS chunks to walk, never
# more than the entry's MAX_SPLITS, and no call of fewer than MIN_KEYS keys.  Module attributes, so that a test or a measurement
# can force a plan.  MIN_KEYS: this route takes only what attention_train.supported leaves to the torch chain.
# Measured with tools/bench_attn_train_split.py (profiles/attn_train_split.json; replays of a HIP graph of one forward + backward,
# 8 heads, three alternating rounds, the torch chain twice per round): at (100 queries, 3 136 keys) and (300, 4 096) with 1, 2 and
# 4 images the plan's count and each of 4 / 8 / 16 splits took less time than the torch chain in every round -- the plan's count
# 0.52 - 0.83 x, worst round against the chain's best -- where the two torch arms differ by at most 1 %; 2 splits are 0.72 -
# 0.85 x and at 300 queries of one image 1.06 x.  The fastest timed count brings the query-side grid to 450 - 2 400 workgroups (8
# splits up to 152 unsplit workgroups, 4 or 8 from 224), 16 splits are slower than 8 everywhere, and the plan's count is within
# 4 % of the fastest timed one except at 300 queries of one image (7 splits of 64 chunks: 12 % behind 8).  Other batch sizes and
# key counts between 1 025 and 3 135 were not timed.  At 784 and 1 024 keys 4 splits took 0.75 - 0.77 x the unsplit kernels' time in
# replay; MIN_KEYS stays above them, with the unsplit route's rule.
MAX_SPLITS = 16
MIN_CHUNKS = 4
TARGET_WORKGROUPS = 1024
MIN_KEYS = attention_train.MAX_KEYS + 1


def default():
    """Process default of CrossAttentionLayer's `attn_train_split` switch: PCT_ATTN_TRAIN_SPLIT = hip | torch (default torch)."""
    return _lib.env_switch("PCT_ATTN_TRAIN_SPLIT")


def chunks(S):
    return -(-S // CHUNK)


def chunk_ranges(S, splits):
    """[(first chunk, one past the last chunk)] of every split: csrc/cross_attention_train_split.hip's key_range.  For
    1 <= splits <= chunks(S) the ranges are non-empty, ascending and partition [0, chunks(S))."""
    nch = chunks(S)
    return [(j * nch // splits, (j + 1) * nch // splits) for j in range(splits)]


def workgroups(Q, N, heads):
    """The unsplit query-side grid: one workgroup per 16 queries of an (image, head)."""
    return -(-Q // 16) * heads * N


def plan(Q, N, heads, S):
    """The `splits` the route would use for Q queries, N images and S keys; below 2 the call is not routed here.  Never more
    than min(16, chunks), whatever the constants are set to."""
    if S < MIN_KEYS:
        return 1
    wg = max(1, workgroups(Q, N, heads))
    return max(0, min(MAX_SPLITS, 16, chunks(S), chunks(S) // MIN_CHUNKS, -(-TARGET_WORKGROUPS // wg)))


def covered(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None):
    """True where the kernels can run: the conditions of attention_train.covered."""
    return attention_train.covered(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open)


def supported(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None):
    """What CrossAttentionLayer sends here: everything `covered` for which `plan` finds at least two splits."""
    if not covered(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open):
        return False
    return plan(q_c.shape[0], q_c.shape[1], heads, k_c.shape[0]) >= 2


def workspace_bytes(N, heads, Q, splits):
    """Bytes of workspace either direction needs (pct_cross_attention_split_train_workspace)."""
    n = _lib.lib().pct_cross_attention_split_train_workspace(N, heads, Q, splits)
    if n < 0:
        _lib.check(int(n), "cross_attention_split_train_workspace")
    return int(n)


def _splits(splits, q_c, heads, S):
    Q, N, _ = q_c.shape
    return max(1, plan(Q, N, heads, S)) if splits is None else int(splits)


def _workspace(q_c, heads, splits):
    """(tensor, bytes) from torch's caching allocator (which also works inside a graph capture)."""
    Q, N, _ = q_c.shape
    need = workspace_bytes(N, heads, Q, splits)
    return torch.empty((max(need // 8, 2),), dtype=torch.float64, device=q_c.device), need


def cross_attention_forward(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None, splits=None):
    """attention_train.cross_attention_forward with the keys divided over `splits` workgroups (None: `plan`, at least 1; the
    entry uses min(splits, chunks)).  -> (out [Q, N, heads * 16] fp32, lse [2, N, heads, Q] fp32); a row with nothing attendable:
    out 0, lse 0."""
    ops = _dense_operands((q_c, q_s, k_c, k_p, v))
    (Q, N, _), S = q_c.shape, k_c.shape[0]
    splits = _splits(splits, q_c, heads, S)
    m, ro = _bytes(attn_mask), _bytes(row_open)
    out, lse = _out_and_lse(q_c, heads)
    ws, need = _workspace(q_c, heads, splits)
    _call("cross_attention_split_forward_f32", "cross_attention train forward S=%d x%d" % (S, splits), out,
          *[t.data_ptr() for t in ops], _ptr(m), _ptr(ro), N, heads, Q, S, float(2 * HEAD_DIM) ** -0.5, splits, ws.data_ptr(), need,
          out.data_ptr(), lse.data_ptr())
    return out, lse


def cross_attention_backward(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open, out, lse, grad_out, splits=None):
    """attention_train.cross_attention_backward with the two sweeps of the query pass divided over `splits` workgroups.
    -> (grad_q_c, grad_q_s, grad_k_c, grad_k_p, grad_v).  Deterministic: two calls on the same operands give the same bits.  The
    C entry allocates nothing; outputs and workspace come from torch's caching allocator."""
    ops = _dense_operands((q_c, q_s, k_c, k_p, v))
    (Q, N, _), S = q_c.shape, k_c.shape[0]
    splits = _splits(splits, q_c, heads, S)
    l, go = _dense(lse), _dense(grad_out)
    m, ro = _bytes(attn_mask), _bytes(row_open)
    grads = [torch.empty_like(t) for t in ops]
    ws, need = _workspace(q_c, heads, splits)
    _call("cross_attention_split_backward_f32", "cross_attention train backward S=%d x%d" % (S, splits), go,
          *[t.data_ptr() for t in ops], _ptr(m), _ptr(ro), out.data_ptr(), l.data_ptr(), go.data_ptr(), N, heads, Q, S,
          float(2 * HEAD_DIM) ** -0.5, splits, ws.data_ptr(), need, *[g.data_ptr() for g in grads])
    return tuple(grads)


class SplitCrossAttentionTrainFunction(torch.autograd.Function):
    """(q_c, q_s, k_c, k_p, v) -> out.  Saves the five operands, out and lse, and keeps the split count; the mask and row_open
    are non-differentiable inputs kept by reference."""

    @staticmethod
    def forward(ctx, q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open, splits):
        out, lse = cross_attention_forward(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open, splits)
        ctx.save_for_backward(q_c, q_s, k_c, k_p, v, out, lse)
        ctx.heads, ctx.attn_mask, ctx.row_open, ctx.splits = int(heads), attn_mask, row_open, int(splits)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q_c, q_s, k_c, k_p, v, out, lse = ctx.saved_tensors
        grads = cross_attention_backward(q_c, q_s, k_c, k_p, v, ctx.heads, ctx.attn_mask, ctx.row_open, out, lse, grad_out,
                                         ctx.splits)
        need = ctx.needs_input_grad
        return tuple(g if need[i] else None for i, g in enumerate(grads)) + (None, None, None, None)


def cross_attention_train(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None, splits=None):
    """attention_train.cross_attention_train on the split kernels: the same operands, mask, row_open and result; `splits` None:
    `plan`'s count, at least 1.  Anything `covered` refuses raises here."""
    if not covered(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open):
        raise RuntimeError("cross_attention_train: operands outside what the kernels cover (see split_key_attention_train.covered)")
    splits = _splits(splits, q_c, heads, k_c.shape[0])
    return SplitCrossAttentionTrainFunction.apply(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open, splits)

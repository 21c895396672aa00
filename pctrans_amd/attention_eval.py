"""Python entry of the decoder's attention in fp32 evaluation (C ABI `pct_cross_attention_eval_f32` /
`pct_self_attention_eval_f32`, include/pctrans_hip_attn_eval.h; kernels pctrans_amd/csrc/attention_eval.hip): the forwards of
attention_train.py and self_attention_train.py without a backward -- no lse, any query count, a wave's loads one key step ahead
-- with the same bits in `out`.  No per-head concatenation, no operand add and no [N, heads, Q, S] tensor is formed.
CrossAttentionLayer and SelfAttentionLayer take them when no gradient is required and their `attn_eval` switch is "hip"
(PCT_ATTN_EVAL); otherwise they keep the branch they had.  There is no backward: operands that require a gradient raise."""

import torch

from . import _lib, attention_train
from .attention_train import HEAD_DIM, _bytes, _call, _dense_operands, _ptr

# Speed rule (tools/bench_attention_eval.py on an MI355X, profiles/attention_eval.json; 8 heads, batches 1 / 8 / 32, replays of a
# HIP graph of one call, three alternating rounds, the torch chain timed twice as its own control: spread <= 5 %).  The kernel
# took 0.25 - 0.61 x the torch chain's time at every shape timed -- cross: 100 queries at 256 / 1 024 / 4 096 keys, 300 queries at
# 374 / 1 452 / 5 655 keys; self: 100 / 300 / 600 queries -- but one: 100 queries on 4 096 keys of ONE image, 1.005 x, a tie.
# That grid is 7 x 8 = 56 workgroups of 64 key steps each on 256 CUs; the 300 queries of one image on 5 655 keys (152 workgroups)
# took 0.61 x.  So: up to MAX_KEYS keys, MAX_QUERIES queries and MAX_BATCH images (beyond them nothing was timed), and above
# LONG_KEYS keys only grids of at least MIN_LONG_GRID workgroups (ceil(Q / 16) * heads * batch); between 56 and 152 workgroups
# at those key counts nothing was timed, and what was not timed stays with torch.
MAX_KEYS = 5655
MAX_QUERIES = 600
MAX_BATCH = 32
LONG_KEYS = 1452
MIN_LONG_GRID = 152


def default():
    """Process default of the layers' `attn_eval` switch: PCT_ATTN_EVAL = hip | torch (default torch)."""
    return _lib.env_switch("PCT_ATTN_EVAL")


def covered(q_a, q_b, k_a, k_b, v, heads, attn_mask=None, row_open=None):
    """True where the kernels can run, for both forms (the self form: q_a = q_c, q_b = q_p, keys of the queries' count, no
    mask): attention_train.covered's predicate -- five fp32 device operands [Q | S, N, heads * 16] outside autocast, heads 4 or
    8, at least one query, key and image, a bool mask [N, 1, Q, S] (or [N, Q, S]) or none, a bool row_open of N * Q elements or
    none, everything on one device.  No query limit."""
    return attention_train.covered(q_a, q_b, k_a, k_b, v, heads, attn_mask, row_open)


def supported(q_a, q_b, k_a, k_b, v, heads, attn_mask=None, row_open=None):
    """What the layers send to the kernels: everything `covered` in the region where the kernel was timed faster than the torch
    chain by more than the control's spread (the rule above)."""
    if not covered(q_a, q_b, k_a, k_b, v, heads, attn_mask, row_open):
        return False
    (Q, N, _), S = q_a.shape, k_a.shape[0]
    if S > MAX_KEYS or Q > MAX_QUERIES or N > MAX_BATCH:
        return False
    return S <= LONG_KEYS or -(-Q // 16) * heads * N >= MIN_LONG_GRID


def _no_grad_only(name, operands):
    if torch.is_grad_enabled() and any(t.requires_grad for t in operands):
        raise RuntimeError("%s has no backward: call it under no_grad or on detached operands (the differentiable kernels are "
                           "attention_train.cross_attention_train / self_attention_train.self_attention_train)" % name)


def cross_attention(q_c, q_s, k_c, k_p, v, heads, attn_mask=None, row_open=None):
    """fp32 cross-attention on split operands: per head the query is [q_c | q_s] and the key [k_c | k_p], the score scale is
    32^-0.5.  attn_mask bool [N, 1, Q, S], True = may not attend; row_open bool [N, 1, Q, 1], True = the query ignores its mask
    row.  -> out [Q, N, heads * 16] fp32, the bits of attention_train.cross_attention_forward's; a row with nothing
    attendable is 0.  Anything `covered` refuses raises."""
    ops = _dense_operands((q_c, q_s, k_c, k_p, v))
    _no_grad_only("attention_eval.cross_attention", (q_c, q_s, k_c, k_p, v))
    if not covered(q_c, q_s, k_c, k_p, v, heads, attn_mask, row_open):
        raise RuntimeError("attention_eval.cross_attention: operands outside what the kernels cover (see attention_eval.covered)")
    (Q, N, C), S = q_c.shape, k_c.shape[0]
    m, ro = _bytes(attn_mask), _bytes(row_open)
    out = torch.empty((Q, N, C), dtype=torch.float32, device=q_c.device)
    _call("cross_attention_eval_f32", "cross_attention eval", out, *[t.data_ptr() for t in ops], _ptr(m), _ptr(ro), N, heads, Q, S,
          float(2 * HEAD_DIM) ** -0.5, out.data_ptr())
    return out


def self_attention(q_c, q_p, k_c, k_p, v, heads):
    """fp32 self-attention on the five projections' outputs: per head q = q_c + q_p, k = k_c + k_p, the score scale is 16^-0.5, no
    mask.  -> out [Q, N, heads * 16] fp32, the bits of self_attention_train.self_attention_forward's, at any query count.
    Anything `covered` refuses raises."""
    ops = _dense_operands((q_c, q_p, k_c, k_p, v))
    _no_grad_only("attention_eval.self_attention", (q_c, q_p, k_c, k_p, v))
    if not covered(q_c, q_p, k_c, k_p, v, heads) or q_c.shape[0] != k_c.shape[0]:
        raise RuntimeError("attention_eval.self_attention: operands outside what the kernels cover (see attention_eval.covered)")
    Q, N, C = q_c.shape
    out = torch.empty((Q, N, C), dtype=torch.float32, device=q_c.device)
    _call("self_attention_eval_f32", "self_attention eval", out, *[t.data_ptr() for t in ops], N, heads, Q, float(HEAD_DIM) ** -0.5,
          out.data_ptr())
    return out

"""Python entry of the split-operand cross-attention with the keys divided over several workgroups (C ABI
`pct_cross_attention_split_keys_bf16`, include/pctrans_hip_xattn_split.h; kernels pctrans_amd/csrc/cross_attention.hip, the
PARTIAL instantiations and the combine).  The kernels behind fused_ops.cross_attention and ragged_attention.cross_attention give
one workgroup to each (image, 4 heads, up to 4 query tiles), and that workgroup walks all the keys: one image with 100 queries
and 8 heads is 4 workgroups on 256 compute units, each walking 64 chunks at 4 096 keys.  Here the chunks of such a workgroup are
divided over `splits` workgroups that leave unnormalised partial results in a workspace, and a second small launch combines them
in a fixed order.  CrossAttentionLayer sends its bf16 eval calls here when its `split_keys` switch is "hip"
(PCT_XATTN_SPLIT_KEYS) and `plan` finds at least two splits; the default is "torch", today's routing."""

import torch

from . import _lib, _timing, ragged_attention

HEAD_DIM = ragged_attention.HEAD_DIM
CHUNK = 64                       # keys per chunk (csrc/cross_attention.hip: XA_CH)
# The plan: as many splits as bring the grid to TARGET_WORKGROUPS, each with at least MIN_CHUNKS chunks to walk, never more than
# the entry's MAX_SPLITS, and no call of fewer than MIN_KEYS keys.  Module attributes, so that a test or a measurement can force
# a plan.  Measured with tools/bench_split_key_attention.py (profiles/split_key_attention.json; 8 heads, 100 / 300 queries, batch
# 1 - 64, 256 - 5 655 keys, the cores at 2 / 4 / 8 / 16 splits against today's route): 512 = two workgroups per compute unit, the
# kernel's occupancy -- on grids of 640 workgroups no split count is faster at 1 024 keys, on grids of up to 320 the plan's
# count is; below 1 024 keys (256, 512, 768 timed) the cores are 1.05 - 1.21 x today's at every split count, one more launch for a
# walk that is short already.  Key counts between 768 and 1 024 are excluded with the slower ones.
MAX_SPLITS = 16
MIN_CHUNKS = 4
TARGET_WORKGROUPS = 512
MIN_KEYS = 1024


def default():
    """Process default of CrossAttentionLayer's `split_keys` switch: PCT_XATTN_SPLIT_KEYS = hip | torch (default torch)."""
    return _lib.env_switch("PCT_XATTN_SPLIT_KEYS")


def chunks(S):
    return -(-S // CHUNK)


def chunk_ranges(S, splits):
    """[(first chunk, one past the last chunk)] of every split: csrc/cross_attention.hip's xa_split_begin.  For
    1 <= splits <= chunks(S) the ranges are non-empty, ascending and partition [0, chunks(S))."""
    nch = chunks(S)
    return [(j * nch // splits, (j + 1) * nch // splits) for j in range(splits)]


def covered(q_content, k_content, v, num_heads, attn_mask):
    """True where the kernels can run: the conditions of ragged_attention.covered."""
    return ragged_attention.covered(q_content, k_content, v, num_heads, attn_mask)


def plan(L, N, num_heads, S):
    """The `splits` the route would use for L queries, N images and S keys; below 2 the call is not routed here.  Never more
    than the C entry takes, min(16, chunks), whatever the constants are set to."""
    if S < MIN_KEYS:
        return 1
    wg = max(1, ragged_attention.workgroups(L, N, num_heads))
    return max(0, min(MAX_SPLITS, 16, chunks(S), chunks(S) // MIN_CHUNKS, -(-TARGET_WORKGROUPS // wg)))


def supported(q_content, k_content, v, num_heads, attn_mask):
    """What CrossAttentionLayer sends here: everything `covered` for which `plan` finds at least two splits."""
    if not covered(q_content, k_content, v, num_heads, attn_mask):
        return False
    return plan(q_content.shape[0], q_content.shape[1], num_heads, k_content.shape[0]) >= 2


def workspace_bytes(N, num_heads, L, splits):
    n = _lib.lib().pct_cross_attention_split_keys_workspace(N, num_heads, L, splits)
    if n < 0:
        _lib.check(int(n), "cross_attention_split_keys_workspace")
    return int(n)


def cross_attention(q_content, q_pos, k_content, k_pos, v, num_heads, attn_mask=None, row_open=None, splits=None):
    """ragged_attention.cross_attention with the keys divided over `splits` workgroups (None: `plan`, at least 1).  The same
    operands and result layout; `splits` == 1 gives that function's bits.  The workspace comes from the caching allocator."""
    L, N, C = q_content.shape
    S = k_content.shape[0]
    if splits is None:
        splits = max(1, plan(L, N, num_heads, S))
    qc, qp, kc, kp, vv = (ragged_attention._dense(t) for t in (q_content, q_pos, k_content, k_pos, v))
    m, pitch = ragged_attention.pitched_mask(attn_mask, N, L, S) if attn_mask is not None else (None, 0)
    ro = row_open.reshape(N, L).contiguous() if (row_open is not None and m is not None) else None
    if ro is not None and ro.dtype != torch.bool:
        raise RuntimeError("row_open must be a bool tensor")
    out = torch.empty((L, N, C), dtype=torch.bfloat16, device=qc.device)
    need = workspace_bytes(N, num_heads, L, splits)
    ws = torch.empty((need // 4,), dtype=torch.float32, device=qc.device) if need else None
    with torch.cuda.device(qc.device), _timing.timed("cross_attention split keys S=%d x%d" % (S, splits), qc):
        rc = _lib.lib().pct_cross_attention_split_keys_bf16(
            qc.data_ptr(), qp.data_ptr(), kc.data_ptr(), kp.data_ptr(), vv.data_ptr(),
            m.data_ptr() if m is not None else None, pitch, ro.data_ptr() if ro is not None else None, N, num_heads, L, S,
            float(2 * HEAD_DIM) ** -0.5, splits, ws.data_ptr() if ws is not None else None, need, out.data_ptr(),
            torch.cuda.current_stream(qc.device).cuda_stream)
    _lib.check(rc, "cross_attention_split_keys")
    return out

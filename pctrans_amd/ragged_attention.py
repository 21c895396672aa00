"""Python entry of the split-operand cross-attention for any key count (C ABI `pct_cross_attention_ragged_bf16`,
include/pctrans_hip_xattn.h; kernel pctrans_amd/csrc/cross_attention.hip, the RAGGED instantiations).  fused_ops.cross_attention
takes key counts that are multiples of 64; the unpadded evaluation images give none (520 x 696: 374 / 1 452 / 5 655 keys per
level), and their layers concatenate the operands per head, write V^T and run the generic kernel.  CrossAttentionLayer sends them
here instead when its `ragged_keys` switch is "hip" (PCT_XATTN_RAGGED); the default is "torch", today's routing.

The mask goes to the kernel as [N, L, pitch] bytes with pitch % 16 == 0: as it is where S % 16 == 0, otherwise copied once into
a pitched buffer whose pad bytes stay uninitialised (the kernel never trusts a byte at a position >= S)."""

import torch

from . import _lib, _timing

HEAD_DIM = 16
# Measured with tools/bench_ragged_attention.py (profiles/ragged_attention.json; 8 heads, 100 / 300 queries, batch 2 / 8 / 128, the
# seven key counts of the unpadded evaluation images): see `supported`.  80 workgroups = batch 8 with 300 queries, the smallest
# timed grid on which the cores are faster at every key count; 484 and 4 221 keys are the timed counts next to the slower ones
SMALL_GRID = 80
SHORT_KEYS, LONG_KEYS = 484, 4221


def default():
    """Process default of CrossAttentionLayer's `ragged_keys` switch: PCT_XATTN_RAGGED = hip | torch (default torch)."""
    return _lib.env_switch("PCT_XATTN_RAGGED")


def _aligned(t):
    """A contiguous tensor goes to the kernel as it is and must sit on 16 bytes; anything else is copied, and a copy is aligned."""
    return not t.is_contiguous() or t.data_ptr() % 16 == 0


def covered(q_content, k_content, v, num_heads, attn_mask):
    """True where the kernel can run: bf16 device tensors [tokens, N, heads*16] on one device, heads % 4 == 0, at least one
    key, boolean mask [N,1,L,S] (or none), operands on 16-byte boundaries, every operand below 2^31 - 1 elements; forward only.
    False, never an exception."""
    ts = (q_content, k_content, v)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 3 for t in ts):
        return False
    if len({t.device for t in ts}) != 1:
        return False
    L, N, C = q_content.shape
    S = k_content.shape[0]
    if num_heads <= 0 or C != num_heads * HEAD_DIM or num_heads % 4 or S < 1:
        return False
    if tuple(k_content.shape) != (S, N, C) or tuple(v.shape) != (S, N, C):
        return False
    if max(L, S) * N * C >= 2 ** 31 - 1:
        return False
    if attn_mask is not None:
        if not (torch.is_tensor(attn_mask) and attn_mask.dtype == torch.bool and attn_mask.device == q_content.device
                and tuple(attn_mask.shape) == (N, 1, L, S)):
            return False
        if S % 16 == 0 and not _aligned(attn_mask):
            return False
    return all(_aligned(t) for t in ts)


def workgroups(L, N, num_heads):
    """The kernel's grid: one workgroup per (image, 4 heads, up to 4 query tiles of 16); each walks all the keys."""
    return N * (num_heads // 4) * (((L + 15) // 16 + 3) // 4)


def supported(q_content, k_content, v, num_heads, attn_mask):
    """What CrossAttentionLayer sends to the kernel: everything `covered`, but a call of fewer than SMALL_GRID workgroups with
    more than SHORT_KEYS and fewer than LONG_KEYS keys.  There (8 - 32 workgroups at 1 452 and 1 936 keys) the cores alone --
    V projection, mask pad and this kernel against the concatenations, V^T and the generic kernel -- took 1.04 - 1.34 x the
    parent's time on the device (profiles/ragged_attention.json): a handful of workgroups walking thousands of keys one after the
    other is latency, and the generic kernel's wave per (image, head, 16 queries) fills more of the device.  Key counts between the
    timed ones are excluded with them."""
    if not covered(q_content, k_content, v, num_heads, attn_mask):
        return False
    L, N, S = q_content.shape[0], q_content.shape[1], k_content.shape[0]
    return not (workgroups(L, N, num_heads) < SMALL_GRID and SHORT_KEYS < S < LONG_KEYS)


def _dense(t):
    """Contiguous and 16-byte aligned (a view at an odd offset is copied)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def pitched_mask(attn_mask, N, L, S):
    """-> (bool [N, L, pitch] with pitch % 16 == 0, pitch).  S % 16 == 0: the mask itself.  Otherwise one copy into a buffer of
    pitch = 16 * ceil(S / 16) from the caching allocator; its pad bytes are not written."""
    m = attn_mask.reshape(N, L, S)
    if S % 16 == 0:
        return _dense(m), S
    pitch = 16 * ((S + 15) // 16)
    buf = torch.empty((N, L, pitch), dtype=torch.bool, device=m.device)
    buf[:, :, :S].copy_(m)
    return buf, pitch


def cross_attention(q_content, q_pos, k_content, k_pos, v, num_heads, attn_mask=None, row_open=None):
    """fused_ops.cross_attention for any number of keys S >= 1: softmax(mask(q k^T / sqrt(32))) v per head with
    q = [q_content_h | q_pos_h], k = [k_content_h | k_pos_h], all operands [tokens, N, heads*16] bf16 -> [L, N, heads*16] bf16.
    Bit-identical to fused_ops.masked_attention on the per-head concatenations.  `row_open`: bool [N, L] (or anything reshapeable
    to it), True = that query ignores its mask row and attends to every key."""
    L, N, C = q_content.shape
    S = k_content.shape[0]
    qc, qp, kc, kp, vv = (_dense(t) for t in (q_content, q_pos, k_content, k_pos, v))
    m, pitch = pitched_mask(attn_mask, N, L, S) if attn_mask is not None else (None, 0)
    ro = row_open.reshape(N, L).contiguous() if (row_open is not None and m is not None) else None
    if ro is not None and ro.dtype != torch.bool:
        raise RuntimeError("row_open must be a bool tensor")
    out = torch.empty((L, N, C), dtype=torch.bfloat16, device=qc.device)
    with torch.cuda.device(qc.device), _timing.timed("cross_attention ragged S=%d" % S, qc):
        rc = _lib.lib().pct_cross_attention_ragged_bf16(
            qc.data_ptr(), qp.data_ptr(), kc.data_ptr(), kp.data_ptr(), vv.data_ptr(),
            m.data_ptr() if m is not None else None, pitch, ro.data_ptr() if ro is not None else None, N, num_heads, L, S,
            float(2 * HEAD_DIM) ** -0.5, out.data_ptr(), torch.cuda.current_stream(qc.device).cuda_stream)
    _lib.check(rc, "cross_attention_ragged")
    return out

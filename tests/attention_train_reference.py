"""Float64 reference of the differentiable cross-attention on split operands (pctrans_amd/attention_train.py): forward, the
analytic backward, the torch chain the kernels replace (the yardstick, in any dtype), and the seeded cases the CPU and GPU
tests share.  Conventions as callsite_reference.cross_operands / attention: per head the query is [content 16 | position 16]
and the key likewise, the score scale is 32^-0.5, a mask entry True = may not attend, row_open True = the query ignores its
mask row.  A row with nothing attendable (a "dead" row) is NaN in torch; here, as in the kernels, its output and every gradient
through it are 0 and its lse is 0."""
import functools

import numpy as np
import torch

import hard_inputs as H

HD = 16
SCALE = float(2 * HD) ** -0.5
F64 = torch.float64


def _heads_first(t, heads):
    """[T, N, heads * 16] -> [N, heads, T, 16]"""
    T, N, _ = t.shape
    return t.reshape(T, N, heads, HD).permute(1, 2, 0, 3)


def _rows(t):
    """[N, heads, T, 16] -> [T, N, heads * 16]"""
    N, h, T, _ = t.shape
    return t.permute(2, 0, 1, 3).reshape(T, N, h * HD)


def effective_mask(mask, row_open, N, Q, S):
    """bool [N, 1, Q, S] (True = dead position) or None."""
    if mask is None:
        return None
    m = mask.reshape(N, 1, Q, S)
    if row_open is not None:
        m = m & ~row_open.reshape(N, 1, Q, 1)
    return m


def forward64(q_c, q_s, k_c, k_p, v, heads, mask=None, row_open=None):
    """-> out [Q, N, heads * 16], lse [N, heads, Q], p [N, heads, Q, S], dead [N, Q] (rows with nothing attendable), float64."""
    Q, N, _ = q_c.shape
    S = k_c.shape[0]
    qc, qs, kc, kp, vh = (_heads_first(t.to(F64), heads) for t in (q_c, q_s, k_c, k_p, v))
    s = (qc @ kc.transpose(2, 3) + qs @ kp.transpose(2, 3)) * SCALE
    m = effective_mask(mask, row_open, N, Q, S)
    dead = torch.zeros(N, Q, dtype=torch.bool)
    if m is not None:
        s = s.masked_fill(m, float("-inf"))
        dead = m.all(-1).reshape(N, Q)
    live = ~dead.reshape(N, 1, Q, 1)
    mx = torch.where(live, s.amax(-1, keepdim=True), torch.zeros((), dtype=F64))
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    p = torch.where(live, e / torch.where(live, l, torch.ones((), dtype=F64)), torch.zeros((), dtype=F64))
    lse = torch.where(live, mx + torch.log(torch.where(live, l, torch.ones((), dtype=F64))), torch.zeros((), dtype=F64))
    return _rows(p @ vh), lse.squeeze(-1), p, dead


def backward64(q_c, q_s, k_c, k_p, v, heads, mask, row_open, grad_out):
    """Analytic gradients in float64, in the operands' layouts: (grad_q_c, grad_q_s, grad_k_c, grad_k_p, grad_v)."""
    qc, qs, kc, kp, vh, go = (_heads_first(t.to(F64), heads) for t in (q_c, q_s, k_c, k_p, v, grad_out))
    out, _, p, _ = forward64(q_c, q_s, k_c, k_p, v, heads, mask, row_open)
    d = (go * _heads_first(out, heads)).sum(-1, keepdim=True)            # [N, heads, Q, 1]
    ds = p * (go @ vh.transpose(2, 3) - d)                                # zero where p is
    pt, dst = p.transpose(2, 3), ds.transpose(2, 3)
    return (_rows(ds @ kc * SCALE), _rows(ds @ kp * SCALE), _rows(dst @ qc * SCALE), _rows(dst @ qs * SCALE), _rows(pt @ go))


def torch_chain(q_c, q_s, k_c, k_p, v, heads, mask=None, row_open=None):
    """The statements the kernels replace (CrossAttentionLayer.forward_post + attention_core), differentiable, in the
    operands' dtype and on their device: two concatenations, q * scale, matmul, masked_fill, softmax, matmul."""
    Q, N, C = q_c.shape
    S = k_c.shape[0]
    hd = C // heads
    q = torch.cat([q_c.view(Q, N, heads, hd), q_s.view(Q, N, heads, hd)], dim=3).view(Q, N, 2 * C)
    k = torch.cat([k_c.view(S, N, heads, hd), k_p.view(S, N, heads, hd)], dim=3).view(S, N, 2 * C)
    qh = (q * float(2 * hd) ** -0.5).reshape(Q, N, heads, 2 * hd).permute(1, 2, 0, 3)
    kh = k.reshape(S, N, heads, 2 * hd).permute(1, 2, 3, 0)
    vh = v.reshape(S, N, heads, hd).permute(1, 2, 0, 3)
    scores = torch.matmul(qh, kh)
    m = effective_mask(mask, row_open, N, Q, S)
    if m is not None:
        scores = scores.masked_fill(m, float("-inf"))
    return torch.matmul(torch.softmax(scores, dim=-1), vh).permute(2, 0, 1, 3).reshape(Q, N, C)


def torch_chain_grads(ops, heads, mask, row_open, grad_out):
    """(out, five gradients) of `torch_chain` by autograd, in the dtype and on the device of `ops`."""
    leaves = [t.detach().clone().requires_grad_(True) for t in ops]
    out = torch_chain(*leaves, heads, mask, row_open)
    return out.detach(), torch.autograd.grad(out, leaves, grad_out)


# ---- cases ------------------------------------------------------------------------------------------------------------------
N = 2
QS = (1, 16, 17, 100)
SS = (1, 63, 64, 65, 196, 784)
BIG = (300, 1024)                        # one case in configs[3]'s range
FAMILIES = ("noise", "noise_open", "noise_nomask", "peaked", "one_hot", "underflow", "window_masks")


def _split(t, heads):
    """[T, N, heads * 32] with per-head [content 16 | position 16] -> two [T, N, heads * 16]."""
    T, n, _ = t.shape
    t = t.reshape(T, n, heads, 2, HD)
    return t[:, :, :, 0].reshape(T, n, heads * HD).contiguous(), t[:, :, :, 1].reshape(T, n, heads * HD).contiguous()


def _seed(family, Q, S, heads):
    return 100000 * FAMILIES.index(family) + 1000 * heads + 7 * Q + S


@functools.lru_cache(maxsize=None)
def case(family, Q, S, heads):
    """-> dict of CPU tensors: the five fp32 operands `ops`, `mask` (bool [N, 1, Q, S] or None), `row_open` (bool [N, 1, Q, 1]
    or None), `grad_out` fp32, `dead_rows` [(n, q)] (rows with nothing attendable), `blocked_key` (a key masked for every
    query, or None), and the float64 reference: `out`, `lse`, `grads`.  Built once per process; treat as read-only.

    noise: Gaussian operands and a random mask (half the entries dead) without row_open; where S > 1 one key is masked for every
    query, where Q > 2 the last query of image 0 is fully masked (a dead row; short rows may be dead by chance as well).
    noise_open: such a mask with a fully masked row and row_open = mask.all(-1), as the decoder builds it: no dead row.
    noise_nomask: no mask.  peaked / one_hot / underflow / window_masks: the score families and the window masks of
    hard_inputs.py at this geometry (window masks declare their dead rows; Q < 4 has no room for them and runs unmasked)."""
    rng = np.random.RandomState(_seed(family, Q, S, heads))
    mask = row_open = blocked = None
    if family.startswith("noise"):
        ops = [torch.from_numpy(rng.standard_normal((T, N, heads * HD)).astype(np.float32)) for T in (Q, Q, S, S, S)]
        if family != "noise_nomask":
            m = rng.random_sample((N, 1, Q, S)) < 0.5
            if family == "noise":
                if S > 1:
                    blocked = S // 2
                    m[:, :, :, blocked] = True
                if Q > 2:
                    m[0, 0, Q - 1] = True
            else:
                m[N - 1, 0, Q // 2] = True
                row_open = torch.from_numpy(m.all(-1, keepdims=True))
            mask = torch.from_numpy(m)
    else:
        if family == "one_hot":
            q, k, _ = H._one_hot_operands(rng, Q, S, N, heads, 2 * HD)
            v = H._bf16(rng.standard_normal((S, N, heads * HD)) * 4)
        else:
            q, k = H._randn_operands(rng, Q, S, N, heads, 2 * HD, 100.0 if family == "underflow" else 12.0)
            v = H._bf16(rng.standard_normal((S, N, heads * HD)))
        ops = list(_split(q.float(), heads)) + list(_split(k.float(), heads)) + [v.float()]
        if family == "window_masks" and Q >= 4:
            m, _, declared = H._window_mask(rng, Q, S, N)
            mask = torch.from_numpy(m)
    grad_out = torch.from_numpy(rng.standard_normal((Q, N, heads * HD)).astype(np.float32))
    out, lse, p, dead = forward64(*ops, heads, mask, row_open)
    dead_rows = [(int(n), int(q)) for n, q in dead.nonzero().tolist()]
    if family == "window_masks" and mask is not None:
        assert dead_rows == sorted((int(n), int(q)) for n, q in declared)
    if family in ("noise_open", "noise_nomask", "peaked", "one_hot", "underflow"):
        assert not dead_rows
    grads = backward64(*ops, heads, mask, row_open, grad_out)
    return dict(ops=ops, mask=mask, row_open=row_open, grad_out=grad_out, heads=heads, dead_rows=dead_rows, blocked_key=blocked,
                out=out, lse=lse, grads=grads)

"""Float64 reference of the differentiable self-attention on the projections' outputs (pctrans_amd/self_attention_train.py):
forward, the analytic backward, the torch chain the kernels replace (the yardstick, in any dtype), and the seeded cases the CPU
and GPU tests share.  Per head q = fl32(q_c + q_p) and k = fl32(k_c + k_p) -- the fp32 sums, as torch's add and the kernels
form them -- widened; the score scale is 16^-0.5; there is no mask, keys are the queries."""
import functools

import numpy as np
import torch

import hard_inputs as H

HD = 16
SCALE = float(HD) ** -0.5
F64 = torch.float64
N = 2
FAMILIES = ("noise", "peaked", "underflow", "one_hot")
# one row; the seams of a 16-row tile; the seams of four waves times 16 keys; configs[2]'s count
QS = (1, 15, 16, 17, 63, 64, 65, 100)
BIG = 300                                # configs[3]'s count
CASES = [(f, Q, 8) for f in FAMILIES for Q in QS]
CASES += [(f, Q, 4) for f in ("noise", "underflow") for Q in (17, 100)]
CASES += [("noise", BIG, 8)]


def _heads_first(t, heads):
    """[T, N, heads * 16] -> [N, heads, T, 16]"""
    T, n, _ = t.shape
    return t.reshape(T, n, heads, HD).permute(1, 2, 0, 3)


def _rows(t):
    """[N, heads, T, 16] -> [T, N, heads * 16]"""
    n, h, T, _ = t.shape
    return t.permute(2, 0, 1, 3).reshape(T, n, h * HD)


def _summed(q_c, q_p, k_c, k_p):
    """q and k as the kernels see them: the sum in the operands' precision (one rounding), then float64."""
    return (q_c + q_p).to(F64), (k_c + k_p).to(F64)


def forward64(q_c, q_p, k_c, k_p, v, heads):
    """-> out [Q, N, heads * 16], lse [N, heads, Q], p [N, heads, Q, Q], float64."""
    q, k = _summed(q_c, q_p, k_c, k_p)
    qh, kh, vh = (_heads_first(t, heads) for t in (q, k, v.to(F64)))
    s = qh @ kh.transpose(2, 3) * SCALE
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    p = e / l
    return _rows(p @ vh), (mx + torch.log(l)).squeeze(-1), p


def backward64(q_c, q_p, k_c, k_p, v, heads, grad_out):
    """Analytic gradients in float64, in the operands' layout: (grad_q, grad_k, grad_v).  grad_q is the gradient of q_c and of
    q_p, grad_k that of k_c and of k_p."""
    q, k = _summed(q_c, q_p, k_c, k_p)
    qh, kh, vh, go = (_heads_first(t, heads) for t in (q, k, v.to(F64), grad_out.to(F64)))
    out, _, p = forward64(q_c, q_p, k_c, k_p, v, heads)
    d = (go * _heads_first(out, heads)).sum(-1, keepdim=True)            # [N, heads, Q, 1]
    ds = p * (go @ vh.transpose(2, 3) - d)
    return _rows(ds @ kh * SCALE), _rows(ds.transpose(2, 3) @ qh * SCALE), _rows(p.transpose(2, 3) @ go)


def torch_chain(q_c, q_p, k_c, k_p, v, heads):
    """The statements the kernels replace (SelfAttentionLayer.forward_post + attention_core), differentiable, in the operands'
    dtype and on their device: two adds, q * scale, matmul, softmax, matmul, the permutes."""
    Q, n, C = q_c.shape
    hd = C // heads
    q = q_c + q_p
    k = k_c + k_p
    qh = (q * float(hd) ** -0.5).reshape(Q, n, heads, hd).permute(1, 2, 0, 3)
    kh = k.reshape(Q, n, heads, hd).permute(1, 2, 3, 0)
    vh = v.reshape(Q, n, heads, hd).permute(1, 2, 0, 3)
    p = torch.softmax(torch.matmul(qh, kh), dim=-1)
    return torch.matmul(p, vh).permute(2, 0, 1, 3).reshape(Q, n, C)


def torch_chain_grads(ops, heads, grad_out):
    """(out, five leaf gradients) of `torch_chain` by autograd, in the dtype and on the device of `ops`."""
    leaves = [t.detach().clone().requires_grad_(True) for t in ops]
    out = torch_chain(*leaves, heads)
    return out.detach(), torch.autograd.grad(out, leaves, grad_out)


def _seed(family, Q, heads):
    return 100000 * FAMILIES.index(family) + 1000 * heads + 7 * Q + 3


def _two_parts(rng, t):
    """t (fp32 holding bf16 values) -> content and position parts, fp32, whose fp32 sum is t exactly: the position part is a
    bf16 value of 1/4 to 3/4 of t, so the difference has at most 9 significant bits."""
    u = torch.from_numpy(rng.uniform(0.25, 0.75, size=tuple(t.shape)).astype(np.float32))
    pos = (t * u).bfloat16().float()
    return (t.double() - pos.double()).float(), pos


@functools.lru_cache(maxsize=None)
def case(family, Q, heads):
    """-> dict of CPU tensors: the five fp32 operands `ops`, `grad_out` fp32, `q` and `k` (the fp32 values the family builds,
    which the parts sum to; None for noise, whose parts are drawn directly), and the float64 reference: `out`, `lse`, `p`,
    `grads` = (grad_q, grad_k, grad_v).  Built once per process; treat as read-only.

    noise: Gaussian parts.  peaked / underflow / one_hot: the score families of hard_inputs.py at head dim 16 with keys =
    queries, q and k each split into two parts."""
    rng = np.random.RandomState(_seed(family, Q, heads))
    q = k = None
    if family == "noise":
        ops = [torch.from_numpy(rng.standard_normal((Q, N, heads * HD)).astype(np.float32)) for _ in range(5)]
    else:
        if family == "one_hot":
            q, k, _ = H._one_hot_operands(rng, Q, Q, N, heads, HD)
            v = H._bf16(rng.standard_normal((Q, N, heads * HD)) * 4)
        else:
            q, k = H._randn_operands(rng, Q, Q, N, heads, HD, 100.0 if family == "underflow" else 12.0)
            v = H._bf16(rng.standard_normal((Q, N, heads * HD)))
        q, k = q.float(), k.float()
        ops = list(_two_parts(rng, q)) + list(_two_parts(rng, k)) + [v.float()]
    grad_out = torch.from_numpy(rng.standard_normal((Q, N, heads * HD)).astype(np.float32))
    out, lse, p = forward64(*ops, heads)
    grads = backward64(*ops, heads, grad_out)
    return dict(ops=ops, grad_out=grad_out, heads=heads, q=q, k=k, out=out, lse=lse, p=p, grads=grads)

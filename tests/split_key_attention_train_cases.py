"""What tests/test_split_key_attention_train_cpu.py and tests/test_split_key_attention_train_gpu.py share: the case lists, the
window case whose queries each see one split's keys only, the fp32 torch yardstick with dead rows taken out, the accuracy rule,
and a float64 NumPy restatement of the split algebra of pctrans_amd/csrc/cross_attention_train_split.hip -- per split (m, l, acc)
and their combine, D as the sum of the splits' partial sums, grad_q as the sum of the splits' partial sums -- with three wrong
combines beside it.  The reference is attention_train_reference.py (R)."""
import functools

import numpy as np
import torch

import attention_train_reference as R

CHUNK = 64
NAMES = ("out", "grad_q_c", "grad_q_s", "grad_k_c", "grad_k_p", "grad_v")

# property (a): one split is the unsplit kernels, bit for bit
ONE_SPLIT = [(f, Q, S, heads) for f in ("noise", "noise_open", "window_masks") for Q, S in ((17, 65), (100, 196), (1, 784))
             for heads in (8, 4)]
# accuracy: more than one block, ragged last chunks, one chunk beyond 1 024 keys, a single query over two chunks
SHAPES = ((17, 129), (100, 196), (16, 1025), (1, 65))
SPLITS = (2, 3, 16)
ACCURACY = [(f, Q, S, 8, s) for f in R.FAMILIES for Q, S in SHAPES for s in SPLITS]
ACCURACY += [(f, Q, S, 4, s) for f in ("noise", "window_masks", "underflow") for Q, S, s in ((17, 129, 3), (100, 196, 2))]
BIG = (100, 3136)                          # the largest level of a 448^2 crop: 49 chunks
WINDOW = dict(Q=17, S=330, splits=3)       # property (b): 6 chunks, the last ragged; the second query tile holds one real query


def chunks(S):
    return -(-S // CHUNK)


def used_splits(S, splits):
    return min(splits, chunks(S))


def key_ranges(S, splits):
    """[(first key, one past the last key)] per split, from the rule of split_key_attention_train.chunk_ranges (the CPU test
    pins the two against each other)."""
    nch, s = chunks(S), used_splits(S, splits)
    return [(j * nch // s * CHUNK, min((j + 1) * nch // s * CHUNK, S)) for j in range(s)]


@functools.lru_cache(maxsize=None)
def window_case(heads):
    """Property (b) at WINDOW: Gaussian operands, and a mask under which query q of image n sees keys of split (q + n) % splits
    only -- between 1 and 40 random keys of that range, its first key for the first query of each split and its last key for the
    second.  No dead row, no row_open.  -> the dict of R.case, with `live_split` [N, Q]."""
    Q, S, splits = WINDOW["Q"], WINDOW["S"], WINDOW["splits"]
    rng = np.random.RandomState(4711 + heads)
    ops = [torch.from_numpy(rng.standard_normal((T, R.N, heads * R.HD)).astype(np.float32)) for T in (Q, Q, S, S, S)]
    grad_out = torch.from_numpy(rng.standard_normal((Q, R.N, heads * R.HD)).astype(np.float32))
    ranges = key_ranges(S, splits)
    m = np.ones((R.N, 1, Q, S), dtype=bool)
    live_split = np.zeros((R.N, Q), dtype=np.int64)
    seen = {}
    for n in range(R.N):
        for q in range(Q):
            j = (q + n) % splits
            lo, hi = ranges[j]
            keys = set(rng.choice(np.arange(lo, hi), size=rng.randint(1, min(40, hi - lo) + 1), replace=False).tolist())
            nth = seen.get((n, j), 0)
            seen[(n, j)] = nth + 1
            if nth == 0:
                keys.add(lo)
            elif nth == 1:
                keys.add(hi - 1)
            m[n, 0, q, sorted(keys)] = False
            live_split[n, q] = j
    mask = torch.from_numpy(m)
    out, lse, _, dead = R.forward64(*ops, heads, mask, None)
    assert not bool(dead.any())
    grads = R.backward64(*ops, heads, mask, None, grad_out)
    return dict(ops=ops, mask=mask, row_open=None, grad_out=grad_out, heads=heads, dead_rows=[], blocked_key=None, out=out, lse=lse,
                grads=grads, live_split=torch.from_numpy(live_split))


# ---- the yardstick and the rule of tests/test_attention_train_gpu.py ----------------------------------------------------------------
_YARD = {}


def yardstick(c, key, device):
    """(out, five gradients) of the fp32 torch chain on `device`, float64 on the CPU, the dead rows taken out of the chain as
    tests/test_attention_train_gpu.py does (their mask rows cleared, their grad_out rows zeroed).  Computed once per `key`."""
    if (key, device) not in _YARD:
        mask, go = c["mask"], c["grad_out"].clone()
        if c["dead_rows"]:
            mask = mask.clone()
            for n, q in c["dead_rows"]:
                mask[n, 0, q] = False
                go[q, n] = 0
        dev = lambda t: None if t is None else t.to(device)
        out, grads = R.torch_chain_grads([t.to(device) for t in c["ops"]], c["heads"], dev(mask), dev(c["row_open"]), go.to(device))
        _YARD[(key, device)] = tuple(t.double().cpu() for t in (out,) + tuple(grads))
    return _YARD[(key, device)]


def live_rows(c):
    Q = c["ops"][0].shape[0]
    live = torch.ones(Q, R.N, dtype=torch.bool)
    for n, q in c["dead_rows"]:
        live[q, n] = False
    return live


def rule(c, got, yard):
    """name -> (e_got, bound) under  e <= 2 * e_torch + 2^-22 * max|ref|  for `out` (live rows) and the five gradients; `got`
    and `yard` are (out, five gradients) as float64 CPU tensors."""
    live = live_rows(c)
    fig = {}
    for name, g, y, w in zip(NAMES, got, yard, (c["out"],) + tuple(c["grads"])):
        if name == "out":
            g, y, w = g[live], y[live], w[live]
        top = float(w.abs().max()) if w.numel() else 0.0
        e_got, e_torch = (float((t - w).abs().max()) if w.numel() else 0.0 for t in (g, y))
        if not np.isfinite(e_got):
            e_got = float("inf")
        fig[name] = (e_got, 2 * e_torch + 2.0 ** -22 * top)
    return fig


def lse_bound(c):
    return 2.0 ** -20 * max(1.0, float(c["lse"].abs().max()))


# ---- the split algebra in float64 -----------------------------------------------------------------------------------------------------
def _heads_first(t, heads):
    return R._heads_first(t.to(R.F64), heads).numpy()


def scores64(c):
    """[N, heads, Q, S] float64 scaled scores, -inf where the query may not attend."""
    heads = c["heads"]
    qc, qs, kc, kp = (_heads_first(t, heads) for t in c["ops"][:4])
    s = (qc @ kc.transpose(0, 1, 3, 2) + qs @ kp.transpose(0, 1, 3, 2)) * R.SCALE
    Q, S = s.shape[2], s.shape[3]
    m = R.effective_mask(c["mask"], c["row_open"], R.N, Q, S)
    if m is not None:
        s = np.where(np.broadcast_to(m.numpy(), s.shape), -np.inf, s)
    return s


def split_maxima(c, splits):
    """[splits, N, heads, Q]: each split's row maximum, -inf where the row has no live key there."""
    s = scores64(c)
    return np.stack([s[..., lo:hi].max(-1) for lo, hi in key_ranges(s.shape[3], splits)])


def split_algebra(c, splits, variant=None):
    """(out, lse, five gradients) as float64 tensors in the layouts of R.forward64 / R.backward64, formed the way the split
    kernels form them.  variant: None, or one of the wrong combines "no_factor" (the factor exp(m_j - M) dropped from l and acc),
    "lse_last_max" (lse from the last split's maximum in place of M), "delta_split0" (D from split 0 alone)."""
    heads = c["heads"]
    s = scores64(c)
    S = s.shape[3]
    ranges = key_ranges(S, splits)
    qc, qs, kc, kp, vh, go = (_heads_first(t, heads) for t in tuple(c["ops"]) + (c["grad_out"],))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # forward partials: (m_j, l_j, acc_j), (-inf, 0, 0) where a row has nothing attendable in the range
        parts = []
        for lo, hi in ranges:
            sj = s[..., lo:hi]
            mj = sj.max(-1)
            e = np.where(np.isinf(sj), 0.0, np.exp(sj - np.where(np.isinf(mj), 0.0, mj)[..., None]))
            parts.append((mj, e.sum(-1), e @ vh[:, :, lo:hi]))
        M = np.max(np.stack([p[0] for p in parts]), axis=0)
        dead = np.isinf(M)
        l, acc = np.zeros_like(M), np.zeros(M.shape + (R.HD,))
        for mj, lj, aj in parts:                                          # ascending j
            f = np.where(np.isinf(mj), 0.0, np.exp(mj - np.where(dead, 0.0, M)))
            if variant == "no_factor":
                f = np.where(np.isinf(mj), 0.0, 1.0)
            l += lj * f
            acc += aj * f[..., None]
        out = np.where(dead[..., None], 0.0, acc / np.where(dead, 1.0, l)[..., None])
        top = parts[-1][0] if variant == "lse_last_max" else M
        lse = np.where(dead, 0.0, top + np.log(np.where(dead, 1.0, l)))
        # backward on the true lse of the row (a wrong forward combine is judged on the forward's results)
        lse_true = np.where(dead, 0.0, M + np.log(np.where(dead, 1.0, l))) if variant in (None, "delta_split0") else R_lse(c)
        p = np.where(np.isinf(s), 0.0, np.exp(np.where(np.isinf(s), 0.0, s) - lse_true[..., None]))
        dp = go @ vh.transpose(0, 1, 3, 2)
        d_parts = [(p[..., lo:hi] * dp[..., lo:hi]).sum(-1) for lo, hi in ranges]
        d = d_parts[0].copy() if variant == "delta_split0" else sum(d_parts[1:], d_parts[0].copy())
        ds = p * (dp - d[..., None])
        dq_c, dq_s = np.zeros_like(qc), np.zeros_like(qs)
        for lo, hi in ranges:                                             # ascending j, scaled once at the end
            dq_c += ds[..., lo:hi] @ kc[:, :, lo:hi]
            dq_s += ds[..., lo:hi] @ kp[:, :, lo:hi]
        dst, pt = ds.transpose(0, 1, 3, 2), p.transpose(0, 1, 3, 2)
        grads = (dq_c * R.SCALE, dq_s * R.SCALE, dst @ qc * R.SCALE, dst @ qs * R.SCALE, pt @ go)
    rows = lambda a: R._rows(torch.from_numpy(np.ascontiguousarray(a)))
    return rows(out), torch.from_numpy(lse), tuple(rows(g) for g in grads)


def R_lse(c):
    return c["lse"].numpy()

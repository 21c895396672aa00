"""Float64 reference of the mask side of the query-contrast loss on the device (pctrans_amd/reid_dice.py; kernels
csrc/reid_dice.hip), its input families, and the bounds the tests hold fp32 results to.  Nothing here depends on the code under
test (`chunks` restates the header's split).

D[i, q] = (2 num + 1) / den, num = sum_p x[k_i, p] x[q, p], den = s[k_i] + s[q] + 1, s[q] = sum_p x[q, p], x = sigmoid(z).

Forward bound (`expected`: dbound), from the kernels' arithmetic, u = 2^-24:
* the sigmoid is expf(-|z|), 1 + e, a division and (for z < 0) a product: expf is good to 2 ulp = 4 u, the division to 1 ulp = 2 u,
  the addition and the product to u each: C_SIG = 8 (in units of u), as point_loss_reference.py counts its sigmoid.
* every term of num and s is positive.  A term of num has two sigmoid factors and one rounding (the fmaf), a term of s one factor
  (the product with the row of ones is exact); an output then passes through L = chain_length(P) additions (the pixels of one
  accumulator's chain plus the chunks of the reduction), each rounding a partial sum that is no larger than the whole:
  |d num| <= (2 C_SIG + L) u num, |d s| <= (C_SIG + L) u s.
* the quotient rule: |d D| <= 2 |d num| / den + D |d den| / den, with 2 num + 1 (two roundings), den (two additions) and the
  division (one) on top: 5 u D.

Gradient bound (gbound).  dz = S w, S = sum of the terms of the issue's closed form, w = x (1 - x).  With A the sum of the terms'
absolute values:
* a = 2 G / den: den carries |d s| of two sums and two additions, the quotient two roundings: REL_A = (C_SIG + L + 4) u.
  b = -G D / den carries D's relative error as well, at most 2 (2 C_SIG + L) u + 5 u by the quotient rule above (both of its parts
  are at most D): REL_B = REL_A + (2 (2 C_SIG + L) + 5) u >= REL_A, used for every term.
* a term multiplies by one sigmoid (C_SIG u) and joins chains over the rows of the image and over the queries, the y of a key row
  through both: (Q + R + 8) u.  So |d S| <= A REL_S, REL_S = REL_B + (C_SIG + Q + R + 8) u.
* w: fl(1 - x~) = (1 - x) - x delta + one rounding, |delta| <= C_SIG u, so |d(1 - x)| <= C_SIG u x + u (1 - x) and
  |d w| <= (C_SIG + 2) u w + C_SIG u x^2: the second part is the absolute floor at saturated positive logits, where fp32 holds
  x = 1 and w = 0.  The product S w: 2 u more.  Below z = -87 fp32 loses x itself: 2^-126 A.
  |d dz| <= A ((REL_S + (C_SIG + 4) u) w + C_SIG u x^2 + 2^-126).
"""
import functools

import torch

U = 2.0 ** -24
C_SIG = 8
PIXELS_PER_PASS, MAX_CHUNKS = 64, 128

# Q, h, w, rows per image (N = their number).  The smallest shapes that reach each way the kernels can go wrong: one tile with
# ragged edges; an image without rows and unsorted keys; several query tiles of one group (100); three query groups, two row
# tiles, 65 chunks of two passes with a ragged tail (300 at 97 x 85 = 8245 pixels); the query limit with three row tiles of one
# forward sweep and the wide kernel of the backward (1024 with 64 rows: one sweep, one row group); and images of 100 and 65
# rows (Q = 128): the forward sweeps the chunk twice (96 rows a sweep, the row of ones in the second), the backward takes two
# row groups of 64 with a ragged last tile (36 rows, and 1 row)
SHAPES = [(5, 6, 5, (2, 1)), (37, 14, 18, (3, 0, 1)), (100, 33, 29, (20, 20)), (300, 97, 85, (33, 60)), (1024, 8, 8, (64,)),
          (128, 8, 8, (100, 65))]
FAMILIES = ("normal", "sparse hot", "saturated", "all cold")
GRADS = ("random", "negative")


def chunks(pixels):
    """(passes, chunks) of include/pctrans_hip_reid.h."""
    subs = -(-pixels // PIXELS_PER_PASS)
    passes = -(-subs // MAX_CHUNKS)
    return passes, -(-subs // passes)


def chain_length(pixels):
    passes, n = chunks(pixels)
    return passes * PIXELS_PER_PASS + n


def chunk_pixels(pixels):
    return chunks(pixels)[0] * PIXELS_PER_PASS


@functools.lru_cache(maxsize=None)
def rows_of(Q, h, w, counts, seed=0):
    """-> (image_start [N + 1] int32, key [I] int32): distinct keys per image in random (unsorted) order.  Read-only."""
    g = torch.Generator().manual_seed(100 * seed + Q + 7 * h)
    keys, starts = [], [0]
    for c in counts:
        keys.append(torch.randperm(Q, generator=g)[:c])
        starts.append(starts[-1] + c)
    return torch.tensor(starts, dtype=torch.int32), torch.cat(keys).to(torch.int32)


@functools.lru_cache(maxsize=None)
def family(name, Q, h, w, counts, seed=0):
    """-> logits [N, Q, h, w] fp32 on the CPU.  Cached: treat as read-only."""
    N, P = len(counts), h * w
    g = torch.Generator().manual_seed(1000 * seed + 13 * Q + P + len(name))
    q = torch.arange(Q)[:, None]
    p = torch.arange(P)[None, :]
    if name == "normal":
        z = 3 * torch.randn(N, Q, P, generator=g)
    elif name == "sparse hot":
        # -12 everywhere; +6 on the first and last pixel of the map (every query) and on the first and last pixel of every
        # pixel chunk (alternating queries)
        cp = chunk_pixels(P)
        edge = ((p % cp == 0) | (p % cp == cp - 1)) & ((q + p // cp) % 2 == 0)
        hot = edge | (p == 0) | (p == P - 1)
        z = torch.where(hot, 6.0, -12.0)[None].repeat(N, 1, 1)
    elif name == "saturated":
        # +-40 in blocks of 5 pixels, a checkerboard over (query, block); the last pixel's block is +40 for every other query
        z = torch.where((q + p // 5) % 2 == 0, 40.0, -40.0)[None].repeat(N, 1, 1)
    elif name == "all cold":
        z = torch.full((N, Q, P), -30.0)
    else:
        raise KeyError(name)
    return z.reshape(N, Q, h, w).float().contiguous()


@functools.lru_cache(maxsize=None)
def grad_in(kind, Q, h, w, counts, seed=0):
    """The incoming gradient G [I, Q] fp32: random, or scaled and negative."""
    g = torch.Generator().manual_seed(17 * seed + Q + sum(counts))
    G = torch.randn(sum(counts), Q, generator=g)
    return G if kind == "random" else -37.5 * G.abs()


def _images(image_start, N):
    st = [int(v) for v in image_start.tolist()]
    return [(n, st[n], st[n + 1]) for n in range(N)]


def dice64(z, image_start, key, drop_pixels=0):
    """-> (D [I, Q], s [N, Q]) in float64 from fp32 logits.  A key outside [0, Q) gives a zero row.  drop_pixels: leave the last
    pixels out of every sum (the known-wrong results of the CPU test)."""
    N, Q = z.shape[:2]
    x = z.detach().cpu().double().flatten(2).sigmoid()
    if drop_pixels:
        x = x[:, :, :x.shape[2] - drop_pixels]
    s = x.sum(-1)
    key = key.long()
    D = torch.zeros(key.shape[0], Q, dtype=torch.float64)
    for n, a, b in _images(image_start, N):
        for i in range(a, b):
            k = int(key[i])
            if 0 <= k < Q:
                D[i] = (2 * (x[n] @ x[n, k]) + 1) / (s[n, k] + s[n] + 1)
    return D, s


def grad64(z, image_start, key, G, D=None, s=None, w_is_x=False):
    """The issue's closed form in float64 -> (dz [N, Q, h, w], A: the same sums over the terms' absolute values, without w).
    D, s: the forward's results to differentiate through (default: the exact ones).  w_is_x: the known-wrong factor."""
    N, Q, h, w = z.shape
    zz = z.detach().cpu().double().flatten(2)
    x = zz.sigmoid()
    wgt = x if w_is_x else x * (-zz).sigmoid()                  # x (1 - x) without the cancellation at saturated logits
    if D is None:
        D, s = dice64(z, image_start, key)
    G = G.detach().cpu().double()
    key = key.long()
    dz, A = torch.zeros_like(x), torch.zeros_like(x)
    for n, i0, i1 in _images(image_start, N):
        ok = [i for i in range(i0, i1) if 0 <= int(key[i]) < Q]
        if not ok:
            continue
        idx = torch.tensor(ok)
        kk = key[idx]
        den = s[n, kk][:, None] + s[n][None, :] + 1
        a, b = 2 * G[idx] / den, -G[idx] * D[idx] / den
        for out, aa, bb in ((dz, a, b), (A, a.abs(), b.abs())):
            t = aa.t() @ x[n, kk]                               # sum_i a[i, q] x[k_i, p]
            t.index_add_(0, kk, aa @ x[n])                      # rows k_i: sum_q' a[i, q'] x[q', p]
            c = bb.sum(0)
            c.index_add_(0, kk, bb.sum(1))
            out[n] = t + c[:, None]
    return (dz * wgt).reshape(N, Q, h, w), A.reshape(N, Q, h, w)


def bounds(z, image_start, key, G):
    """-> (dbound [I, Q], gbound [N, Q, h, w]): the module docstring."""
    N, Q, h, w = z.shape
    L = chain_length(h * w)
    D, s = dice64(z, image_start, key)
    x = z.detach().cpu().double().flatten(2).sigmoid()
    key = key.long()
    dbound = torch.zeros_like(D)
    rmax = 0
    for n, a, b in _images(image_start, N):
        rmax = max(rmax, b - a)
        for i in range(a, b):
            k = int(key[i])
            if 0 <= k < Q:
                den = s[n, k] + s[n] + 1
                num = x[n] @ x[n, k]
                dbound[i] = (2 * (2 * C_SIG + L) * U * num + D[i] * (C_SIG + L) * U * (s[n, k] + s[n])) / den + 5 * U * D[i]
    _, A = grad64(z, image_start, key, G, D, s)
    rel_b = (C_SIG + L + 4) * U + (2 * (2 * C_SIG + L) + 5) * U
    rel_s = rel_b + (C_SIG + Q + rmax + 8) * U
    xx = x.reshape(N, Q, h, w)
    wgt = xx * (1 - xx)
    gbound = A * ((rel_s + (C_SIG + 4) * U) * wgt + C_SIG * U * xx * xx + 2.0 ** -126)
    return dbound, gbound


@functools.lru_cache(maxsize=None)
def expected(name, kind, Q, h, w, counts, seed=0):
    """-> dict(z, image_start, key, G, D, s, dz, dbound, gbound) of one case.  Cached: treat as read-only."""
    z = family(name, Q, h, w, counts, seed)
    image_start, key = rows_of(Q, h, w, counts, seed)
    G = grad_in(kind, Q, h, w, counts, seed)
    D, s = dice64(z, image_start, key)
    dz, _ = grad64(z, image_start, key, G, D, s)
    dbound, gbound = bounds(z, image_start, key, G)
    return dict(z=z, image_start=image_start, key=key, G=G, D=D, s=s, dz=dz, dbound=dbound, gbound=gbound)


def torch_chain(z, image_start, key, G):
    """The parent's path (query_contrast.select_pos_neg_mask's expression) in the dtype and on the device of z, and its
    autograd gradient -> (D [I, Q], dz)."""
    zz = z.detach().clone().requires_grad_(True)
    x = zz.flatten(2).sigmoid()
    s = x.sum(-1)
    dice = (2 * torch.bmm(x, x.transpose(1, 2)) + 1) / (s[:, :, None] + s[:, None, :] + 1)
    st = image_start.tolist()
    img = torch.tensor([n for n in range(z.shape[0]) for _ in range(st[n], st[n + 1])], dtype=torch.long, device=z.device)
    rows = dice[img, key.long().to(z.device)]
    grad, = torch.autograd.grad((rows * G.to(device=z.device, dtype=z.dtype)).sum(), zz)
    return rows.detach(), grad


def cases():
    return [(name, Q, h, w, counts) for (Q, h, w, counts) in SHAPES for name in FAMILIES]

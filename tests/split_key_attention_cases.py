"""Shapes and inputs the two split-key cross-attention test files share (a plain helper module, like ragged_attention_cases.py).

KEYS: 65 = 2 chunks with a 1-key tail; 129 = 3 chunks, the last a single key; 200 = a tail of 8; 208 = S % 16 == 0 (the mask goes
to the kernel unpitched) but ragged; 256 = aligned, no tail; 374 = 6 chunks with a tail of 54.  Every `splits` from 2 to
min(6, chunks).  QUERIES: one partial tile; a second tile group of one tile.

exact_mask: masks on which the combine is exact -- each row's live keys lie inside one split's chunk range, so that row's
weights are exp(0) = 1 for the live split and 0 for the others, whose partial results are zeros."""
import numpy as np
import torch

KEYS = (65, 129, 200, 208, 256, 374)
QUERIES, HEADS, BATCHES = (10, 65), (4, 8), (1, 3)
MAX_TESTED_SPLITS = 6
HARD_GEOMETRIES = [(37, 200, 2, 8, 32), (100, 374, 2, 8, 32), (16, 129, 1, 4, 32)]
LAYER_SHAPE = dict(Q=37, S=13 * 17, N=2, C=128, heads=8)


def chunks(S):
    return -(-S // 64)


def split_counts(S):
    return list(range(2, min(MAX_TESTED_SPLITS, chunks(S)) + 1))


def key_ranges(S, splits):
    """[(first key, one past the last key)] of every split, from split_key_attention.chunk_ranges."""
    from pctrans_amd import split_key_attention
    return [(64 * c0, min(64 * c1, S)) for c0, c1 in split_key_attention.chunk_ranges(S, splits)]


def exact_mask(L, S, N, splits, seed):
    """-> dict(mask bool [N, 1, L, S] (True = dead), row_open bool [N, 1, L, 1], live_split int64 [N, L], key_s_minus_1,
    key_0, opened, dead: (image, row) each).  Rows of image 0, in order: for every split j a row live in that split alone with
    the split's first and last key live; a row live at key S - 1 alone; a row live at key 0 alone; a fully masked row opened by
    row_open; a fully masked row.  Every other row of every image: live in one split drawn at random, about 30 % of its keys
    (at least one).  live_split is -1 on the opened and on the dead row."""
    assert splits + 4 <= L
    rng = np.random.RandomState(seed)
    ranges = key_ranges(S, splits)
    mask = np.ones((N, L, S), dtype=bool)
    live_split = np.zeros((N, L), dtype=np.int64)
    for n in range(N):
        for l in range(L):
            j = l if (n == 0 and l < splits) else int(rng.randint(0, splits))
            lo, hi = ranges[j]
            live = rng.random_sample(hi - lo) < 0.3
            live[int(rng.randint(0, hi - lo))] = True
            if n == 0 and l < splits:
                live[0] = live[-1] = True
            mask[n, l, lo:hi] = ~live
            live_split[n, l] = j
    rows = dict(key_s_minus_1=(0, splits), key_0=(0, splits + 1), opened=(0, splits + 2), dead=(0, splits + 3))
    mask[0, splits:splits + 4] = True
    mask[0, splits, S - 1] = False
    live_split[0, splits] = splits - 1
    mask[0, splits + 1, 0] = False
    live_split[0, splits + 1] = 0
    live_split[0, splits + 2] = live_split[0, splits + 3] = -1
    row_open = np.zeros((N, 1, L, 1), dtype=bool)
    row_open[0, 0, splits + 2, 0] = True
    return dict(mask=torch.from_numpy(mask[:, None]), row_open=torch.from_numpy(row_open),
                live_split=torch.from_numpy(live_split), **rows)


# ---- a float64 restatement of the two kernels' arithmetic (numpy; one head, one image) --------------------------------------
def partials_f64(scores, v, ranges):
    """scores [L, S] float64 with -inf on dead keys, v [S, D]; ranges: key ranges of the splits.
    -> (o [splits, L, D] relative to m, m [splits, L], l [splits, L]): what the partial kernel leaves per split."""
    o, m, l = [], [], []
    for lo, hi in ranges:
        s = scores[:, lo:hi]
        mj = s.max(axis=1)
        safe = np.where(np.isneginf(mj), 0.0, mj)
        p = np.exp(s - safe[:, None])
        o.append(p @ v[lo:hi])
        m.append(mj)
        l.append(p.sum(axis=1))
    return np.stack(o), np.stack(m), np.stack(l)


def combine_f64(o, m, l, weights=True, normalise_first=False, drop_last=False):
    """The combine kernel's statements in float64.  The three switches are the wrong variants the CPU test tells apart:
    no exp(m_j - M) weights; every split normalised by its own l_j before the sum; the last split left out."""
    if drop_last:
        o, m, l = o[:-1], m[:-1], l[:-1]
    M = m.max(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(np.isneginf(m), 0.0, np.exp(m - M[None])) if weights else np.where(np.isneginf(m), 0.0, 1.0)
        if normalise_first:
            per = np.where(l[..., None] > 0, o / l[..., None], 0.0)
            return per.sum(axis=0)
        L = (w * l).sum(axis=0)
        O = (w[..., None] * o).sum(axis=0)
        return O * (1.0 / L)[:, None]

"""Seeded builders of the inputs on which the two value-dependent kernels are hardest, shared by CPU and GPU tests
(numpy RandomState and torch CPU arithmetic only, so the CPU box and the GPU box build the same data):

  * csrc/lsap.hip -- cost families that force long Dijkstra searches, rerouting, exact ties, +inf entries and infeasibility
    that only the search can see, each as `cost [B, Q, Gmax] float32` + ragged `counts` (the launch decides LDS residency
    from Gmax, the kernel solves the first counts[b] columns);
  * csrc/attn_common.hpp -- bf16-exact attention operands whose scores are peaked, monotone in the key index, one-hot,
    windowed by the mask, or spread far enough that most probabilities underflow.

The float64 references live here as well (scipy for LSAP, a plain softmax for attention), computed once per case and
shared read-only between the tests that need them."""
import functools

import numpy as np
import torch

INF = np.float32(np.inf)


# ---- LSAP -------------------------------------------------------------------------------------------------------------
MACHOL_WIEN_GEOMETRIES = [(40, 25), (300, 60), (300, 128), (256, 256), (257, 257), (1024, 512)]


def _ragged_counts(G):
    return [G, G - G // 3, max(2, G // 5)]


def _pad(problems, Q, gmax):
    """[B, Q, gmax] with zeros past a problem's own columns, as the matcher pads."""
    cost = np.zeros((len(problems), Q, gmax), dtype=np.float32)
    for b, c in enumerate(problems):
        assert c.shape[0] == Q and c.dtype == np.float32
        cost[b, :, :c.shape[1]] = c
    return cost, [int(c.shape[1]) for c in problems]


def machol_wien(Q, G, counts=None):
    """c[j, i] = (j + 1)(i + 1) (Machol & Wien 1976): every augmentation reroutes through all targets assigned so far.
    Integers below 2^24: exact in fp32, totals exact in fp64."""
    counts = _ragged_counts(G) if counts is None else counts
    full = np.outer(np.arange(1, Q + 1), np.arange(1, G + 1)).astype(np.float32)
    return _pad([full[:, :g] for g in counts], Q, G)


def rank_one_noise(Q, G, seed):
    """a_j + b_i + 1e-3 u: a rank-one matrix is degenerate (every assignment of the same queries costs the same), the
    small noise makes the optimum unique while the duals stay close together -- long chains with generic values."""
    rng = np.random.RandomState(seed)
    out = []
    for g in _ragged_counts(G):
        a, b = rng.standard_normal((Q, 1)) * 3, rng.standard_normal((1, g)) * 3
        out.append((a + b + 1e-3 * rng.random_sample((Q, g))).astype(np.float32))
    return _pad(out, Q, G)


def duplicated_queries(seed, integer=False, Q=300, G=60):
    """60 distinct rows, each repeated 5 times and interleaved (query j is a copy of row j % 60): copies sit in different
    lanes, in both lane iterations (j and j + 256) and in different waves; the ties between queries are exact.
    `integer`: small integer costs with ties inside the rows as well, and exactly representable totals."""
    rng = np.random.RandomState(seed)
    out = []
    for g in _ragged_counts(G):
        if integer:     # integer rank-one part + {0, 1, 2}: degenerate duals on top of the duplicated rows
            base = rng.randint(0, 20, size=(G, 1)) + rng.randint(0, 20, size=(1, g)) + rng.randint(0, 3, size=(G, g))
        else:
            base = rng.standard_normal((G, g)) * 3
        out.append(base[np.arange(Q) % G].astype(np.float32))
    return _pad(out, Q, G)


def forbidden_pairs(Q, G, seed, density=0.7):
    """70 % of the entries +inf, with a planted finite permutation so that a solution exists."""
    rng = np.random.RandomState(seed)
    out = []
    for g in _ragged_counts(G):
        c = (rng.standard_normal((Q, g)) * 3).astype(np.float32)
        finite = rng.random_sample((Q, g)) >= density
        finite[rng.permutation(Q)[:g], np.arange(g)] = True
        out.append(np.where(finite, c, INF))
    return _pad(out, Q, G)


def hall_violation(Q, G, seed):
    """Three problems; in the middle one every column has finite entries, but targets 7 and G - 3 share their single
    finite query: infeasible through the search only (Hall's condition fails for that pair of targets)."""
    cost, counts = forbidden_pairs(Q, G, seed, density=0.3)
    counts = [G, G, counts[2]]
    rng = np.random.RandomState(seed + 1)
    cost[1] = (rng.standard_normal((Q, G)) * 3).astype(np.float32)
    only = Q // 2 + 3
    for t in (7, G - 3):
        keep = cost[1, only, t]
        cost[1, :, t] = INF
        cost[1, only, t] = keep
    return cost, counts


def magnitudes(Q, G, seed):
    """One generic matrix scaled by 1e30 and by 1e-30 (fp32 range, fp64 duals), and one offset by 1e6, where fp32
    quantises the differences between entries to 1/16."""
    rng = np.random.RandomState(seed)
    c = rng.standard_normal((Q, G)) * 3
    out = [(c * 1e30).astype(np.float32), (c[:, :G - G // 3] * 1e-30).astype(np.float32),
           (1e6 + c[:, :max(2, G // 5)]).astype(np.float32)]
    return _pad(out, Q, G)


def noise(Q, G, seed):
    """The easy family the older tests use (dense Gaussian), for comparison."""
    rng = np.random.RandomState(seed)
    return _pad([(rng.standard_normal((Q, g)) * 3).astype(np.float32) for g in _ragged_counts(G)], Q, G)


def matcher_like(seed=0, counts=(12, 7), copies=5, size=32):
    """Collapsed queries of a trained model: every prediction is one target's logits (+-4) plus small noise, and each such
    prediction appears `copies` times (interleaved, exact copies).  -> (outputs, targets) for Point_HungarianMatcher."""
    rng = np.random.RandomState(seed)
    Q = copies * max(counts)
    pred = np.zeros((len(counts), Q, size, size), dtype=np.float32)
    targets = []
    for b, g in enumerate(counts):
        yy, xx = np.mgrid[0:size, 0:size]
        cy, cx, rad = rng.randint(4, size - 4, g), rng.randint(4, size - 4, g), rng.randint(3, 9, g)
        masks = (((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2)
                 <= rad[:, None, None] ** 2).astype(np.float32)
        logits = (8.0 * masks - 4.0 + 0.05 * rng.standard_normal(masks.shape)).astype(np.float32)
        pred[b] = logits[np.arange(Q) % g]
        targets.append({"masks": torch.from_numpy(masks)})
    return {"pred_masks": torch.from_numpy(pred)}, targets


def matcher_like_costs(seed=0):
    """The matcher's own cost matrices for `matcher_like`, formed on the CPU."""
    from pctrans_amd.loss.matcher import Point_HungarianMatcher
    outputs, targets = matcher_like(seed)
    m = Point_HungarianMatcher(cost_mask=5.0, cost_dice=5.0, num_points=256)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        C, counts = m._batched_costs(outputs, targets)
    return C.numpy().astype(np.float32), counts


LSAP_CASES = {"machol_wien-%dx%d" % qg: functools.partial(machol_wien, *qg) for qg in MACHOL_WIEN_GEOMETRIES}
# both declared limits in one launch, next to the two trivial problem sizes
LSAP_CASES["machol_wien-1024x512"] = functools.partial(machol_wien, 1024, 512, counts=[512, 0, 1])
LSAP_CASES.update({
    "rank_one_noise-300x60": functools.partial(rank_one_noise, 300, 60, 11),
    "rank_one_noise-300x128": functools.partial(rank_one_noise, 300, 128, 12),
    "rank_one_noise-257x257": functools.partial(rank_one_noise, 257, 257, 13),
    "duplicated_queries": functools.partial(duplicated_queries, 21),
    "duplicated_queries-integer": functools.partial(duplicated_queries, 22, integer=True),
    "forbidden_pairs-300x60": functools.partial(forbidden_pairs, 300, 60, 31),
    "forbidden_pairs-300x128": functools.partial(forbidden_pairs, 300, 128, 32),
    "magnitudes-300x60": functools.partial(magnitudes, 300, 60, 41),
    "magnitudes-300x128": functools.partial(magnitudes, 300, 128, 42),
    "matcher_like": matcher_like_costs,
})
LSAP_INTEGER_CASES = {n for n in LSAP_CASES if n.startswith("machol_wien") or n.endswith("-integer")}


def scipy_solve(cost, counts):
    """-> per problem (query of each target [g] int64, total in fp64) by scipy.optimize.linear_sum_assignment on the
    widened costs, as the reference's matcher calls it; raises where scipy raises."""
    from scipy.optimize import linear_sum_assignment
    out = []
    for b, g in enumerate(counts):
        c = cost[b, :, :g].astype(np.float64)
        ri, ci = linear_sum_assignment(c)
        rows = np.empty(g, dtype=np.int64)
        rows[ci] = ri
        out.append((rows, float(c[rows, np.arange(g)].sum())))
    return out


@functools.lru_cache(maxsize=None)
def lsap_case(name):
    """(cost, counts, scipy's answer) of a named case, built and solved once per process; treat as read-only."""
    cost, counts = LSAP_CASES[name]()
    cost.setflags(write=False)
    return cost, counts, scipy_solve(cost, counts)


def sap_sweeps(c):
    """Plain restatement of the shortest-augmenting-path loop (Crouse 2016; one augmentation per target over the queries,
    the orientation scipy and csrc/lsap.hip use) for one [Q, g] fp64 matrix -> (query of each target, number of Dijkstra
    sweeps).  Ties: a free query first, then the lower index."""
    Q, g = c.shape
    u, v = np.zeros(g), np.zeros(Q)
    tgt_of_query, query_of_tgt = np.full(Q, -1), np.full(g, -1)
    sweeps = 0
    for cur in range(g):
        shortest, path = np.full(Q, np.inf), np.full(Q, -1)
        scanned_q, scanned_t = np.zeros(Q, dtype=bool), np.zeros(g, dtype=bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            sweeps += 1
            scanned_t[i] = True
            r = min_val + c[:, i] - u[i] - v
            better = ~scanned_q & (r < shortest)
            path[better] = i
            shortest[better] = r[better]
            cand = np.where(scanned_q, np.inf, shortest)
            low = cand.min()
            if low == np.inf:
                raise ValueError("cost matrix is infeasible")
            ties = np.flatnonzero(cand == low)
            free = ties[tgt_of_query[ties] < 0]
            j = int(free[0] if free.size else ties[0])
            min_val = low
            scanned_q[j] = True
            if tgt_of_query[j] < 0:
                sink = j
            else:
                i = int(tgt_of_query[j])
        others = scanned_t.copy()
        others[cur] = False
        u[cur] += min_val
        u[others] += min_val - shortest[query_of_tgt[others]]
        v[scanned_q] -= min_val - shortest[scanned_q]
        j = sink
        while True:
            t = path[j]
            tgt_of_query[j] = t
            j, query_of_tgt[t] = query_of_tgt[t], j
            if t == cur:
                break
    return query_of_tgt, sweeps


# ---- attention --------------------------------------------------------------------------------------------------------
# (L, S, N, heads, head_dim): every L, S, N of the issue, both head dims of masked_attention, 4 and 8 heads where the
# cross-attention kernel applies (head_dim 32, S % 64 == 0), ragged last steps (S % 32 in {25, 18, 4, 22}), S < 32
ATTN_GEOMETRIES = [
    (16, 25, 1, 8, 16), (37, 50, 2, 8, 32), (100, 64, 1, 4, 32), (37, 100, 1, 8, 16), (100, 256, 2, 8, 32),
    (100, 374, 2, 8, 32), (37, 1024, 1, 4, 32), (100, 1024, 2, 8, 16), (16, 64, 2, 8, 32), (100, 1024, 1, 8, 32),
]
ATTN_FAMILIES = ["peaked", "ascending", "descending", "one_hot", "window_masks", "v_outliers", "underflow"]
VD = 16                      # value dims per head


def _bf16(a):
    """float array -> torch.bfloat16 tensor (round to nearest even)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16()


def _randn_operands(rng, L, S, N, heads, hd, score_std):
    """q, k ~ N(0, c^2) with c^4 = score_std^2: the scaled scores have that standard deviation."""
    c = np.sqrt(score_std)
    return _bf16(rng.standard_normal((L, N, heads * hd)) * c), _bf16(rng.standard_normal((S, N, heads * hd)) * c)


def _ramp_operands(rng, L, S, N, heads, hd, descending):
    """score(l, s) = scale * r(s) * sum_m c[l, m] with r(s) = s (or S - 1 - s): key dims come in pairs holding
    32 * (r // 32) and r % 32 (both bf16-exact up to 1023), the query holds the same positive weight on both dims of a pair.
    The per-key score step runs from about 1/64 to 1/2 over the queries."""
    r = (S - 1 - np.arange(S)) if descending else np.arange(S)
    k = np.zeros((S, N, heads, hd // 2, 2))
    k[..., 0] = (32 * (r // 32))[:, None, None, None]
    k[..., 1] = (r % 32)[:, None, None, None]
    step = 2.0 ** rng.randint(-6, 0, size=(L, N, heads, 1))                     # score gained per key
    w = 2.0 ** rng.randint(-3, 1, size=(L, N, heads, hd // 2))
    w = w / w.sum(-1, keepdims=True) * step * np.sqrt(hd)
    q = np.repeat(_bf16(w).float().numpy()[..., None], 2, axis=-1)              # rounded first, then paired
    return _bf16(q.reshape(L, N, heads * hd)), _bf16(k.reshape(S, N, heads * hd))


def _one_hot_keys(rng, L, S, N, heads):
    """p[n, h, l]: over the queries of the case, the first key, keys 31 and 32, S - 33, S - 1, the ragged tail, and every
    residue mod 32 (spread over the 32-key steps); the remaining queries draw theirs at random."""
    steps = (S + 31) // 32
    must = [0, 31, 32, S - 33, S - 1, 32 * (S // 32), 32 * (S // 32) + (S % 32) // 2]
    must += [32 * ((5 * r + 1) % steps) + r for r in range(32)]
    must = [p for p in must if 0 <= p < S]
    p = rng.randint(0, S, size=N * heads * L)
    p[:len(must)] = must[:p.size]
    return p.reshape(N, heads, L)


def _one_hot_operands(rng, L, S, N, heads, hd):
    """score(l, s) = -B * scale * ((a_l - a_s)^2 + (b_l - b_s)^2) + const(l) for key s = 32 a_s + b_s and the query's key
    p = 32 a_l + b_l, expanded as B (2 a_l a_s - a_s^2) + ...: integer operands below 2^24, squares stored in two bf16-exact
    parts.  B * scale = 64 (head dim 16) or 90.5 (head dim 32): every other key is at least that far below p(l).  The two
    digits sit in different halves of the head (content / positional dims of the cross-attention kernel); the dims
    the query leaves at zero hold noise in the keys."""
    p = _one_hot_keys(rng, L, S, N, heads)
    B = 256.0 if hd == 16 else 512.0
    s = np.arange(S)
    k = rng.standard_normal((S, N, heads, hd))
    q = np.zeros((L, N, heads, hd))
    for off, dq, dk in ((0, p // 32, s // 32), (hd // 2, p % 32, s % 32)):
        k[..., off] = dk[:, None, None]
        k[..., off + 1] = (32 * (dk ** 2 // 32))[:, None, None]
        k[..., off + 2] = (dk ** 2 % 32)[:, None, None]
        q[..., off] = 2 * B * dq.transpose(2, 0, 1)
        q[..., off + 1] = q[..., off + 2] = -B
    return _bf16(q.reshape(L, N, heads * hd)), _bf16(k.reshape(S, N, heads * hd)), p


def _window_mask(rng, L, S, N):
    """[N, 1, L, S] bool, True = dead: a contiguous live window of at most 5 % of S per query (at least one key) -- by
    turns anywhere, wholly inside the ragged tail (the last step where S % 32 == 0), behind at least two (one, for short S)
    wholly dead 32-key steps, and at the very first keys; plus a few fully masked rows.  -> (mask, windows [N, L, 2])."""
    wmax = max(1, int(0.05 * S))
    tail = 32 * (S // 32) if S % 32 else max(0, S - 32)
    mask = np.ones((N, 1, L, S), dtype=bool)
    win = np.zeros((N, L, 2), dtype=np.int64)
    for n in range(N):
        for l in range(L):
            w = int(rng.randint(1, wmax + 1))
            kind = (l + n) % 4
            if kind == 0:
                lo = int(rng.randint(0, S - w + 1))
            elif kind == 1:
                w = min(w, S - tail)
                lo = int(rng.randint(tail, S - w + 1))
            elif kind == 2:
                first = 64 if S >= 64 + w else (32 if S >= 32 + w else 0)
                lo = int(rng.randint(first, S - w + 1))
            else:
                lo = 0
            mask[n, 0, l, lo:lo + w] = False
            win[n, l] = (lo, lo + w)
    dead_rows = sorted({(0, 3), (N - 1, L - 1), (0, min(17, L - 2))})
    for n, l in dead_rows:
        mask[n, 0, l] = True
        win[n, l] = (0, 0)
    return mask, win, dead_rows


def attention_f64(q, k, v, mask, heads):
    """softmax(mask(q k^T / sqrt(head_dim))) v per head in float64 on the exact bf16 operands.
    -> want [L, N, heads * 16], A = sum_i p_i |v_i| in the same layout, p [N, heads, L, S]; NaN on fully masked rows."""
    L, N, E = q.shape
    S = k.shape[0]
    hd = E // heads
    qh = q.double().reshape(L, N, heads, hd).permute(1, 2, 0, 3)
    kh = k.double().reshape(S, N, heads, hd).permute(1, 2, 3, 0)
    vh = v.double().reshape(S, N, heads, VD).permute(1, 2, 0, 3)
    s = torch.matmul(qh, kh) * float(hd) ** -0.5
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, -1)
    back = lambda t: t.permute(2, 0, 1, 3).reshape(L, N, heads * VD)
    return back(torch.matmul(p, vh)), back(torch.matmul(p, vh.abs())), p, s


@functools.lru_cache(maxsize=2)
def attention_case(family, geometry):
    """-> dict: q [L, N, heads*hd], k [S, N, heads*hd], v [S, N, heads*16] bf16 CPU tensors, mask (bool [N, 1, L, S] or
    None), heads, and the float64 reference (want, A, p, scores); family extras (`hot`, `windows`, `dead_rows`,
    `outliers`).  Built once per process; treat as read-only."""
    L, S, N, heads, hd = geometry
    rng = np.random.RandomState(1000 * ATTN_FAMILIES.index(family) + ATTN_GEOMETRIES.index(geometry))
    case = dict(heads=heads, mask=None, geometry=geometry)
    v = _bf16(rng.standard_normal((S, N, heads * VD)))
    if family in ("peaked", "window_masks", "v_outliers"):
        q, k = _randn_operands(rng, L, S, N, heads, hd, 12.0)
    elif family == "underflow":
        q, k = _randn_operands(rng, L, S, N, heads, hd, 100.0)
    elif family in ("ascending", "descending"):
        q, k = _ramp_operands(rng, L, S, N, heads, hd, family == "descending")
    else:
        q, k, case["hot"] = _one_hot_operands(rng, L, S, N, heads, hd)
        v = _bf16(rng.standard_normal((S, N, heads * VD)) * 4)
    if family == "window_masks":
        mask, case["windows"], case["dead_rows"] = _window_mask(rng, L, S, N)
        case["mask"] = torch.from_numpy(mask)
    if family == "v_outliers":
        # +-1e3 (bf16-exact) in half of the value dims of the tenth of the keys that matter least to any query of the head
        p = attention_f64(q, k, v, None, heads)[2]
        worst = p.amax(dim=2)                                                           # [N, heads, S]
        order = worst.argsort(dim=-1)[..., :max(1, S // 10)].numpy()                    # [N, heads, S // 10]
        vv = v.float().numpy().reshape(S, N, heads, VD).copy()
        for n in range(N):
            for h in range(heads):
                keys = order[n, h][worst[n, h, order[n, h]].numpy() < 1e-3]             # "little": below 1e-3 for every query
                vv[keys, n, h, ::2] = np.where(rng.random_sample((keys.size, VD // 2)) < 0.5, -1e3, 1e3)
        v = _bf16(vv.reshape(S, N, heads * VD))
        case["outliers"] = torch.from_numpy(np.abs(vv) == 1e3).reshape(S, N, heads, VD).permute(1, 2, 0, 3)  # [N, heads, S, 16]
    case.update(q=q, k=k, v=v)
    case["want"], case["A"], case["p"], case["scores"] = attention_f64(q, k, v, case["mask"], heads)
    return case

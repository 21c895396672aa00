"""Float64 reference of the query side of the query-contrast loss on the device and of the per-item contrast reduction
(pctrans_amd/reid_query.py; kernels csrc/reid_query.hip), the inputs of its GPU tests, and the bounds the tests hold fp32 results
to.  Nothing here depends on the code under test.  Plain helpers, no tests.

Bounds, with u = 2^-24 (fp32 unit roundoff) and L = CHAIN_LENGTH, the number of fp32 additions a dot product of the kernels
passes through (include/pctrans_hip_reid_query.h: 8 fmaf per lane + 6 butterfly steps; L <= C + 8):
  dots      |S - S64| <= L u abs_sum                     abs_sum = sum_c |x_q[c] x_k[c]|   (each product enters an fmaf unrounded)
  cosines   |Cs - Cs64| <= (2 L + 6) u                   the dot's L u (abs_sum <= |x_q| |x_k|), L / 2 u per squared norm under
                                                         the root of each of the two norms, and 6 roundings: two roots, the two
                                                         clamps' product, the division, and two to spare
  nearest   a chosen positive's float64 cosine is within 2 (2 L + 6) u of the row's maximum (both cosines compared carry the
            cosine bound), and it IS the float64 first argmax wherever the top-two gap exceeds that
  loss      |loss - loss64| <= (2 Q + 32) u (1 + |loss64|)    two sums of at most Q terms, their exp / log / log1p at a few u
  coef      |coef - coef64| <= (2 Q + 32) u inv_t             |coef| <= inv_t
  backward  |g - g64| <= (T + 8) u abs_sum per element   T = the products of that element's sum as grad64 expands it: per item of
            the image gS x_k, gC / (m m) x_k and b x_q / m^2 (3 I_n), and per item whose key is the element's query the same three
            over all queries (3 Q); 8 for the roundings inside a coefficient.  The kernel adds at most I_n + Q + 8 numbers."""
import functools

import torch

U = 2.0 ** -24
CHAIN_LENGTH = 14
MAX_QUERIES, MAX_CHANNELS, MAX_BATCH = 1024, 512, 65535
COS_EPS, NORM_EPS = 1e-8, 1e-12
COS_BOUND = (2 * CHAIN_LENGTH + 6) * U
GAP = 2 * COS_BOUND

# (N, Q, C, positives per image): C below and above one wave's 256-channel pass, Q no multiple of 32 (nor of the 4 rows of a
# workgroup), an image without items, a single-instance image (every unmatched query joins its cluster: no negatives)
SHAPES = ((3, 37, 24, (5, 0, 1)), (2, 70, 256, (9, 33)))
SEEDS = (11, 12)


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """-> (query [Q, N, C] fp32 seeded gaussians, pos_lists: per image its matched queries in a shuffled order)."""
    N, Q, C, counts = SHAPES[shape]
    g = torch.Generator().manual_seed(SEEDS[shape])
    query = torch.randn(Q, N, C, generator=g)
    pos_lists = [torch.randperm(Q, generator=g)[:c].tolist() for c in counts]
    return query, pos_lists


def cos64(query, pos_lists):
    """-> per image the float64 cosines [Q, P_n] of every query against the image's positives, as F.cosine_similarity: each
    norm clamped at 1e-8."""
    x = query.double()
    out = []
    for n, pl in enumerate(pos_lists):
        X = x[:, n]
        nr = X.norm(dim=1).clamp(min=COS_EPS)
        out.append((X @ X[pl].t()) / (nr[:, None] * nr[pl][None, :]) if pl else X.new_zeros(X.shape[0], 0))
    return out


def nearest64(query, pos_lists):
    """-> (nearest: N lists of Q positions, the first float64 maximum, -1 without positives; gap: N tensors [Q] with the
    difference of the two largest cosines, inf with fewer than two positives)."""
    nearest, gap = [], []
    for c in cos64(query, pos_lists):
        Q, P = c.shape
        if P == 0:
            nearest.append([-1] * Q)
            gap.append(torch.full((Q,), float("inf"), dtype=torch.float64))
            continue
        nearest.append(c.argmax(1).tolist())          # (argmax returns the first maximum)
        top = c.topk(min(2, P), dim=1).values
        gap.append(top[:, 0] - top[:, 1] if P > 1 else torch.full((Q,), float("inf"), dtype=torch.float64))
    return nearest, gap


def plan_of(nearest, pos_lists, Q):
    """The items of query_contrast._plan, restated: per image and matched query with a non-empty cluster
    (image, key, cluster, negatives)."""
    plan = []
    for n, pl in enumerate(pos_lists):
        if not pl:
            continue
        clusters = {p: [] for p in pl}
        for r in range(Q):
            if r not in clusters:
                clusters[pl[nearest[n][r]]].append(r)
        for p in pl:
            if clusters[p]:
                plan.append((n, p, clusters[p], [q for q in range(Q) if q != p and q not in set(clusters[p])]))
    return plan


def rows_of(plan, N, Q):
    """-> (image_start [N + 1], key [I], image_of [I], owner [N, Q]) int32 of a plan."""
    counts = [sum(1 for p in plan if p[0] == n) for n in range(N)]
    starts = [0]
    for c in counts:
        starts.append(starts[-1] + c)
    owner = torch.full((N, Q), -1, dtype=torch.int32)
    for i, (n, _, cluster, _) in enumerate(plan):
        owner[n, cluster] = i
    return (torch.tensor(starts, dtype=torch.int32), torch.tensor([p[1] for p in plan], dtype=torch.int32),
            torch.tensor([p[0] for p in plan], dtype=torch.int32), owner)


def _images(image_start, n_items):
    st = image_start.tolist()
    img = [0] * n_items
    for n in range(len(st) - 1):
        for i in range(st[n], st[n + 1]):
            img[i] = n
    return img


def rows64(query, image_start, key):
    """-> (norm [N, Q] = max(|x|, 1e-12), S [I, Q], Cs [I, Q], S_abs [I, Q]) in float64."""
    x = query.double()
    Q, N, _ = x.shape
    norm = x.norm(dim=2).t().clamp(min=NORM_EPS).contiguous()
    I = int(key.shape[0])
    img = _images(image_start, I)
    S, S_abs, Cs = x.new_zeros(I, Q), x.new_zeros(I, Q), x.new_zeros(I, Q)
    for i in range(I):
        n, k = img[i], int(key[i])
        S[i] = x[:, n] @ x[k, n]
        S_abs[i] = x[:, n].abs() @ x[k, n].abs()
        Cs[i] = S[i] / (norm[n] * norm[n, k])
    return norm, S, Cs, S_abs


def grad64(query, image_start, key, gS, gC, norm, Cs):
    """The closed form of include/pctrans_hip_reid_query.h in float64, with the norms and cosines the forward wrote.
    -> (grad [Q, N, C], abs_sum [Q, N, C], T [Q, N]: the number of products of each element's sum)."""
    x, gS, gC, norm, Cs = query.double(), gS.double(), gC.double(), norm.double(), Cs.double()
    Q, N, C = x.shape
    st = image_start.tolist()
    g, g_abs, T = torch.zeros_like(x), torch.zeros_like(x), torch.zeros(Q, N, dtype=torch.float64)
    for n in range(N):
        lo, hi = st[n], st[n + 1]
        if hi == lo:
            continue
        X, m = x[:, n], norm[n]
        keys = key[lo:hi].long()
        live = (m > NORM_EPS).double()
        a1, a2 = gS[lo:hi], gC[lo:hi] / (m[None, :] * m[keys][:, None])
        b = -gC[lo:hi] * Cs[lo:hi]
        K = X[keys]
        gn = (a1 + a2).t() @ K + ((b.sum(0) * live / m ** 2)[:, None]) * X
        gn_abs = (a1.abs() + a2.abs()).t() @ K.abs() + ((b.abs().sum(0) * live / m ** 2)[:, None]) * X.abs()
        Tn = torch.full((Q,), 3.0 * (hi - lo), dtype=torch.float64)
        Y, Y_abs = (a1 + a2) @ X, (a1.abs() + a2.abs()) @ X.abs()
        for j, k in enumerate(keys.tolist()):
            gn[k] += Y[j] + b[j].sum() * live[k] / m[k] ** 2 * X[k]
            gn_abs[k] += Y_abs[j] + b[j].abs().sum() * live[k] / m[k] ** 2 * X[k].abs()
            Tn[k] += 3.0 * Q
        g[:, n], g_abs[:, n], T[:, n] = gn, gn_abs, Tn
    return g, g_abs, T


def contrast64(rows, image_of, key, owner, inv_t):
    """-> (loss [I], coef [I, Q]) in float64.  The two sums are of positive terms: they are their own abs_sum."""
    z = rows.double() * inv_t
    I, Q = z.shape
    loss, coef = z.new_zeros(I), z.new_zeros(I, Q)
    for i in range(I):
        n, k = int(image_of[i]), int(key[i])
        pos = owner[n] == i
        neg = ~pos
        neg[k] = False
        pos[k] = False
        if not bool(neg.any()) or not bool(pos.any()):
            continue
        A, B = torch.logsumexp(z[i][neg], 0), torch.logsumexp(-z[i][pos], 0)
        t = A + B
        loss[i] = t.clamp(min=0) + torch.log1p(torch.exp(-t.abs()))      # (F.softplus returns its argument above 20)
        s = torch.sigmoid(t)
        coef[i][neg] = s * torch.softmax(z[i][neg], 0) * inv_t
        coef[i][pos] = -s * torch.softmax(-z[i][pos], 0) * inv_t
    return loss, coef


@functools.lru_cache(maxsize=None)
def expected(shape):
    """Everything the tests of one shape share, computed once: inputs, the float64 plan, rows, seeded incoming gradients."""
    N, Q, C, counts = SHAPES[shape]
    query, pos_lists = inputs(shape)
    nearest, gap = nearest64(query, pos_lists)
    plan = plan_of(nearest, pos_lists, Q)
    image_start, key, image_of, owner = rows_of(plan, N, Q)
    norm, S, Cs, S_abs = rows64(query, image_start, key)
    g = torch.Generator().manual_seed(100 + shape)
    gS = torch.randn(len(plan), Q, generator=g)
    gC = torch.randn(len(plan), Q, generator=g)
    return dict(query=query, pos_lists=pos_lists, nearest=nearest, gap=gap, plan=plan, image_start=image_start, key=key,
                image_of=image_of, owner=owner, norm=norm, S=S, Cs=Cs, S_abs=S_abs, gS=gS, gC=gC)

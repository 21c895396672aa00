"""Plain helpers of the validation-metric tests (pctrans_amd/metrics.py; kernels csrc/label_metrics.hip): the literal numpy
restatement of the metric definitions, a second numpy version built on the contingency table for large maps, known-wrong
variants of the literal one, and the input builders.

`literal(pred, gt)` goes through per-pair boolean masks and Python loops and never forms a contingency table: it is an
independent check of the table derivation.  Its only shortcut is to skip a label value that no pixel has where the
definition gives that value the term 0 anyway (an absent j has dice 0 with every i; an absent i adds 0 to the sum) -- the
divisor still counts every integer.  Bounds the tests hold the package to:
    integer outputs (table, areas, values, tp / fp / fn / taken, |DiffFG|)     exact
    AJI, DQ, F1 and a Best Dice of one term                                    one fp64 division of exact integers: bit-equal
                                                                               (F1 is held to 4 * 2^-53 relative)
    Best Dice, SQ                                                              n * 2^-53 * value for n summed terms
PQ = DQ * SQ inherits SQ's bound plus one rounding."""
import numpy as np

EPS = 2.0 ** -53
VARIANTS = ("ge_half", "last_max", "no_take_on_zero_row", "bd_present_divisor", "bg_zero_cvppp")


# ---------------------------------------------------------------- literal definitions

def _best_dice_literal(a, b, variant=None):
    """-> (BD(a, b), number of summed non-zero-capable terms)."""
    lo_a, hi_a, lo_b, hi_b = int(a.min()), int(a.max()), int(b.min()), int(b.max())
    if variant == "bg_zero_cvppp":
        lo_a = lo_b = 0
    if hi_a <= lo_a:
        return 0.0, 0
    present_a, present_b = set(np.unique(a).tolist()), set(np.unique(b).tolist())
    s, terms = 0.0, 0
    for i in range(lo_a + 1, hi_a + 1):
        if i not in present_a:
            continue                                   # A_i empty: every dice is 0 (or 0 by the both-empty rule)
        A = a == i
        best = 0.0
        for j in range(lo_b + 1, hi_b + 1):
            if j not in present_b:
                continue                               # B_j empty: 2 * 0 / (|A_i| + 0) = 0
            B = b == j
            best = max(best, 2 * int((A & B).sum()) / (int(A.sum()) + int(B.sum())))
        s += best
        terms += 1
    div = terms if variant == "bd_present_divisor" else hi_a - lo_a
    return s / div, terms


def _instances(m):
    return [int(v) for v in np.unique(m) if v != 0]


def _aji_literal(pred, gt, variant=None):
    gts, preds = _instances(gt), _instances(pred)
    if not preds:
        return 0.0, 0
    taken = [False] * len(preds)
    c = u = 0
    for g in gts:
        m = gt == g
        offers = []
        for k, p in enumerate(preds):
            if taken[k]:
                offers.append((0, int(m.sum())))
            else:
                q = pred == p
                inter = int((m & q).sum())
                offers.append((inter, int(m.sum()) + int(q.sum()) - inter))
        quot = [i / un for i, un in offers]
        best = max(quot)
        hits = [k for k, x in enumerate(quot) if x == best]
        hit = hits[-1] if variant == "last_max" else hits[0]
        if variant == "no_take_on_zero_row" and best == 0:
            c, u = c, u + int(m.sum())
            continue
        c += offers[hit][0]
        u += offers[hit][1]
        taken[hit] = True
    u += sum(int((pred == p).sum()) for k, p in enumerate(preds) if not taken[k])
    return (c / u if u else 0.0), sum(taken)


def _f1_literal(pred, gt):
    a, b = pred != 0, gt != 0
    tp, fp, fn = int((a & b).sum()), int((a & ~b).sum()), int((~a & b).sum())
    den = 2 * tp + fp + fn
    return 2 * tp / den if den else 0.0


def _pq_literal(pred, gt, variant=None):
    gts, preds = _instances(gt), _instances(pred)
    tp, s = 0, 0.0
    for g in gts:
        m = gt == g
        for p in preds:
            q = pred == p
            inter = int((m & q).sum())
            iou = inter / (int(m.sum()) + int(q.sum()) - inter)
            if iou >= 0.5 if variant == "ge_half" else iou > 0.5:
                tp += 1
                s += iou
    fp, fn = len(preds) - tp, len(gts) - tp
    den = tp + 0.5 * fp + 0.5 * fn
    dq = tp / den if den else 0.0
    sq = s / (tp + 1e-6)
    return dq, sq, dq * sq, tp, fp, fn


def literal(pred, gt, variant=None):
    """pred, gt: 2-D integer numpy arrays -> dict of the nine metrics, the integer outputs and the term counts of the sums."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    bdp, n_p = _best_dice_literal(pred, gt, variant)
    bdg, n_g = _best_dice_literal(gt, pred, variant)
    aji, taken = _aji_literal(pred, gt, variant)
    dq, sq, pq, tp, fp, fn = _pq_literal(pred, gt, variant)
    return {"best_dice_pred": bdp, "best_dice_gt": bdg, "sbd": min(bdp, bdg),
            "abs_diff_fg": float(abs((int(pred.max()) - int(pred.min())) - (int(gt.max()) - int(gt.min())))),
            "aji": aji, "dice": _f1_literal(pred, gt), "dq": dq, "sq": sq, "pq": pq, "tp": tp, "fp": fp, "fn": fn, "taken": taken,
            "terms_pred": n_p, "terms_gt": n_g}


def literal_table(pred, gt):
    """(values_pred, values_gt, areas_pred, areas_gt, T[g, p]) from one mask pair per cell."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    vp, vg = np.unique(pred), np.unique(gt)
    T = np.array([[int(((gt == g) & (pred == p)).sum()) for p in vp] for g in vg], dtype=np.int64).reshape(len(vg), len(vp))
    return vp, vg, np.array([int((pred == p).sum()) for p in vp]), np.array([int((gt == g).sum()) for g in vg]), T


# ---------------------------------------------------------------- table-based numpy version

def table(pred, gt):
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    vp, ip = np.unique(pred.ravel(), return_inverse=True)
    vg, ig = np.unique(gt.ravel(), return_inverse=True)
    T = np.bincount(ig.ravel() * len(vp) + ip.ravel(), minlength=len(vg) * len(vp)).reshape(len(vg), len(vp)).astype(np.int64)
    return vp, vg, T.sum(0), T.sum(1), T


def _bd_table(T, a_in, a_other, lo, hi):
    if hi <= lo or T.shape[0] < 2 or T.shape[1] < 2:
        return 0.0, max(0, T.shape[1] - 1) if hi > lo else 0
    dice = (2 * T[1:, 1:]) / (a_other[1:, None] + a_in[None, 1:])
    s = 0.0
    for x in dice.max(axis=0).tolist():
        s += x
    return s / (hi - lo), T.shape[1] - 1


def from_table(pred, gt):
    """The same dict as `literal`, from the contingency table."""
    vp, vg, ap, ag, T = table(pred, gt)
    bdp, n_p = _bd_table(T, ap, ag, int(vp[0]), int(vp[-1]))
    bdg, n_g = _bd_table(T.T, ag, ap, int(vg[0]), int(vg[-1]))
    p0, g0 = int(vp[0] == 0), int(vg[0] == 0)
    Tf, bp, bg = T[g0:, p0:], ap[p0:], ag[g0:]
    G, P = Tf.shape
    taken = np.zeros(P, dtype=bool)
    c = u = 0
    if P:
        for g in range(G):
            inter = np.where(taken, 0, Tf[g])
            union = np.where(taken, bg[g], bg[g] + bp - Tf[g])
            hit = int(np.argmax(inter / union))
            c += int(inter[hit])
            u += int(union[hit])
            taken[hit] = True
        u += int(bp[~taken].sum())
    den = int(bp.sum()) + int(bg.sum())
    union = bg[:, None] + bp[None, :] - Tf
    matched = 2 * Tf > union
    tp = int(matched.sum())
    fp, fn = P - tp, G - tp
    s = 0.0
    for x in (Tf[matched] / union[matched]).tolist():
        s += x
    dd = tp + 0.5 * fp + 0.5 * fn
    dq = tp / dd if dd else 0.0
    sq = s / (tp + 1e-6)
    return {"best_dice_pred": bdp, "best_dice_gt": bdg, "sbd": min(bdp, bdg),
            "abs_diff_fg": float(abs((int(vp[-1]) - int(vp[0])) - (int(vg[-1]) - int(vg[0])))),
            "aji": c / u if u else 0.0, "dice": 2 * int(Tf.sum()) / den if den else 0.0, "dq": dq, "sq": sq, "pq": dq * sq,
            "tp": tp, "fp": fp, "fn": fn, "taken": int(taken.sum()), "terms_pred": n_p, "terms_gt": n_g}


# ---------------------------------------------------------------- comparison

FLOAT_KEYS = ("best_dice_pred", "best_dice_gt", "sbd", "abs_diff_fg", "aji", "dice", "dq", "sq", "pq")
INT_KEYS = ("tp", "fp", "fn", "taken")


def mismatches(got, want, keys=FLOAT_KEYS + INT_KEYS):
    """The keys of `got` (floats / ints of one image) outside their bound against the reference dict `want`."""
    bad = []
    for k in keys:
        g, w = got[k], want[k]
        if k in INT_KEYS or k in ("abs_diff_fg", "aji", "dq"):
            ok = g == w
        elif k == "dice":
            ok = abs(g - w) <= 4 * EPS * abs(w)
        elif k == "best_dice_pred":
            ok = abs(g - w) <= want["terms_pred"] * EPS * abs(w) if want["terms_pred"] > 1 else g == w
        elif k == "best_dice_gt":
            ok = abs(g - w) <= want["terms_gt"] * EPS * abs(w) if want["terms_gt"] > 1 else g == w
        elif k == "sbd":
            ok = abs(g - w) <= max(want["terms_pred"], want["terms_gt"]) * EPS * abs(w)
        elif k == "sq":
            ok = abs(g - w) <= max(want["tp"], 1) * EPS * abs(w)
        else:                                          # pq = dq * sq
            ok = abs(g - w) <= (max(want["tp"], 1) + 1) * EPS * abs(w)
        if not ok:
            bad.append((k, g, w))
    return bad


# ---------------------------------------------------------------- inputs

def blocks(H, W, bh, bw, first=1, step=1, limit=None):
    """Label map of bh x bw blocks numbered first, first + step, ... in row-major order; blocks past `limit` are background."""
    ys, xs = np.arange(H)[:, None] // bh, np.arange(W)[None, :] // bw
    k = ys * ((W + bw - 1) // bw) + xs
    out = first + step * k
    if limit is not None:
        out = np.where(k < limit, out, 0)
    return out.astype(np.int64)


def _shift(m, dy, dx):
    out = np.zeros_like(m)
    H, W = m.shape
    out[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = m[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return out


def spaced_blocks(H, W, bh, bw, limit=None):
    """Blocks with a background frame: a one-pixel gap between neighbours."""
    m = blocks(H, W, bh, bw, limit=limit)
    ys, xs = np.arange(H)[:, None] % bh, np.arange(W)[None, :] % bw
    return np.where((ys == 0) | (xs == 0), 0, m)


def small_builders(H, W):
    """name -> (pred, gt): maps of at most 20 labels, each built to exercise one rule."""
    bh, bw = max(H // 4, 2), max(W // 4, 2)
    gt = spaced_blocks(H, W, bh, bw)
    out = {}
    out["blocks_shifted"] = (_shift(gt, 2, 3), gt)
    out["stripes_vs_blocks"] = (blocks(H, W, H, max(W // 7, 1)) * (np.arange(W)[None, :] % 5 != 0), gt)
    out["checkerboard"] = (1 + (np.arange(H)[:, None] + np.arange(W)[None, :]) % 2, gt)          # no run longer than 1
    out["one_label"] = (np.full((H, W), 3, dtype=np.int64), gt)                                  # one run
    out["one_label_both"] = (np.full((H, W), 3, dtype=np.int64), np.full((H, W), 1, dtype=np.int64))
    out["gaps"] = (np.where(gt > 0, 3 * _shift(gt, 1, 1) + 2, 0) * (_shift(gt, 1, 1) > 0), np.where(gt > 0, 5 * gt - 3, 0))
    out["no_background"] = (blocks(H, W, bh, bw, first=3), blocks(H, W, bh + 1, bw + 2, first=2))
    big = np.array([0, 7, 40000, 65535, 65534, 12])
    out["raw_65535"] = (big[_shift(gt, 1, 2) % 6], big[gt % 6][:, ::-1].copy())
    out["empty_pred"] = (np.zeros((H, W), dtype=np.int64), gt)
    out["empty_gt"] = (gt, np.zeros((H, W), dtype=np.int64))
    out["empty_both"] = (np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64))
    # IoU exactly 1/2: 3 px, 3 px, 2 shared -- beside a well-matched pair
    p, g = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    g[1, 1:4] = 1
    p[1, 2:5] = 1
    g[5:9, 5:9] = 2
    p[5:9, 5:10] = 2
    out["iou_half"] = (p, g)
    # two predictions tying on IoU for ground-truth 1 (2 of its 8 px each, 6 px in all); prediction 2's rest lies in ground-truth 2
    p, g = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    g[2, 2:10] = 1
    g[4:8, 2:8] = 2
    p[2, 2:4] = 1
    p[0, 0:4] = 1
    p[2, 6:8] = 2
    p[4, 2:6] = 2
    out["iou_tie"] = (p, g)
    # AJI quirk: ground-truth 1 overlaps nothing -> takes the untaken prediction 1, which ground-truth 2 overlaps
    p, g = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    g[1:3, 1:5] = 1
    g[6:10, 2:8] = 2
    g[12:15, 2:6] = 3
    p[6:10, 2:9] = 1
    p[12:15, 3:7] = 2
    out["aji_zero_row"] = (p, g)
    return out


def many_values(k, H=96, W=96):
    """A map of exactly k distinct values: k - 1 instances of 4 x 4 blocks on background (511 fit in 96 x 96)."""
    assert (H // 4) * (W // 4) > k - 1
    return np.where(blocks(H, W, 4, 4) <= k - 1, blocks(H, W, 4, 4, first=1, step=3), 0)


def random_instances(H, W, count, seed, radius=(4, 9)):
    """About `count` discs of random radius on background, later ones over earlier ones; values 1 .. count."""
    rng = np.random.RandomState(seed)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    out = np.zeros((H, W), dtype=np.int64)
    for k in range(1, count + 1):
        cy, cx, r = rng.randint(0, H), rng.randint(0, W), rng.randint(radius[0], radius[1] + 1)
        out[(ys - cy) ** 2 + (xs - cx) ** 2 <= r * r] = k
    return out


def perturbed(m, seed):
    """A prediction for ground truth `m`: shifted, some instances dropped, some merged, renumbered."""
    rng = np.random.RandomState(seed)
    out = _shift(m, int(rng.randint(-2, 3)), int(rng.randint(-2, 3)))
    ids = np.unique(out)
    ids = ids[ids != 0]
    lut = np.zeros(int(m.max()) + 1, dtype=np.int64)
    lut[ids] = rng.permutation(len(ids)) + 1
    drop = ids[rng.rand(len(ids)) < 0.1]
    lut[drop] = 0
    merge = ids[rng.rand(len(ids)) < 0.05]
    if len(merge) > 1:
        lut[merge] = lut[merge[0]]
    return lut[out]

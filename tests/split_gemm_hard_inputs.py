"""Seeded builders of the operands on which the split-bf16 GEMM kernels are hardest, with their float64 references, shared
by the CPU and GPU tests (numpy and torch CPU arithmetic only, so both boxes build the same data):

  * csrc/linear_k128_split.hip (and its fp32-MFMA twin linear_k128.hip), csrc/linear_ln_split.hip, csrc/ffn_fused_split.hip,
    csrc/conv1x1_split.hip with split_tr_gemm.hpp (plain and in front of GroupNorm), and the 3 x 3 product of csrc/fpn_stage.hip;
    the arithmetic of csrc/split_bf16.hpp.

The kernels evaluate a . w from the three-way split a = a1 + a2 + a3 (a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2),
round to nearest even, `split3` emulates it on the bit pattern and keeps bf16 subnormals) as
    hi = sum a1 w1,      lo = sum a1 w2 + a2 w1 + a2 w2 + a1 w3 + a3 w1,      result = fl32(hi + lo)
and drop a2 w3 + a3 w2 + a3 w3 (`six_terms`, `dropped`).

Exactness rule (every builder of `planes`, `range` and `containment` obeys it; `check_accumulators` asserts it on integers):
the pieces of a row of x are integers times 2^ex[row], those of a row of w integers times 2^ew[column].  All a1 w1 products
are multiples of a quantum q_hi with sum_k |a1 w1| / q_hi < 2^24, the five small terms are multiples of q_lo with the sum of
their magnitudes / q_lo < 2^24, and the dropped terms are zero.  Then every partial sum of hi and of lo is an fp32 number in
any order of accumulation, hi + lo is rounded once and the float64 value T of the product is exact.  With u = 2^-24:

    |got - want| <= 2u (|T| + |want|),      want = act(T + bias) in float64                                 (`bound`)

(u |T| is the one rounding of hi + lo, u |want| that of the bias add; the factor 2 is slack for an epilogue that applies an
affine with one more rounding, as fpn_stage's fmaf does not even need.)  Nothing in the bound is measured.

Families:
  planes       operands put together from short pieces, each a small odd multiple of a power of two, found by searching a menu
               for the combinations that `split3` returns unchanged (ties to even admit some 17-bit sums):
                   x3    x three non-zero pieces, w first plane only      probes a1w1, a2w1, a3w1
                   w3    x first plane only, w three non-zero pieces      probes a1w2, a1w3
                   x2w2  both operands planes 1 and 2                     probes a2w2 (and a1w2, a2w1 again)
               and the `cancel` form of each: pairs of k (x2w2: quads) carry weights +c / -c and operands that agree in the
               leading pieces and differ in the probed one only (x3: a2 on even rows, a3 on odd rows; w3: by column), so the
               output consists of the probed plane alone and a missing or mis-paired term is an error of order 1.  In the
               plain forms every k and every column is non-zero, in the cancel forms every k sits in a pair: each k index and
               each output column carries a probed term in every row.  (For K > 256 a row keeps 256 non-zero k, a window
               rotated by 252 with the row that keeps pairs whole.)  With x_add (plain forms only) x + x_add is the menu value:
               x_add moves the first piece inside its binade, and the stored x splits exactly as well (a segment of a multi
               call that does not add multiplies it).  In front of a norm (`layer_norm_case`, `groupnorm_case`, `ffn_case`) the
               cancel forms make the pre-norm values obey the exactness rule of norm_hard_inputs.py, whose bound then holds
               unchanged; the comments at those builders say how each case is arranged so that it does.
  routing      bias / ReLU entries.  W is a signed permutation times a power of two (n > K: rotated selections; K > 128: one
               weight per block of 128 k, x alive in block (row mod blocks) only), x generic fp32 with three live planes, all
               elements distinct, rows scaled by 2^(5 ((r mod 9) - 4)): the output is +-2^j x[r, pi(c)] bit for bit (compared as
               values, -0 == +0).  The mirror has one-hot rows of x and generic W: out[r, c] = W[c, k(r)] bit for bit.  With
               x_add the selected value is fl32(x + x_add).
  range        the x3 / w3 data with rows of x scaled by 2^s and columns of w by 2^t, operands inside [2^-103, 2^100], every
               partial product inside fp32's normal range; same bound.  One more case puts x in [2^-110, 2^-103): its third
               pieces are bf16 subnormals and the split is still exact.
  containment  the x3 data with a NaN in one row, +inf in another and the largest finite fp32 (>= 0x7F7F8000: a1 overflows, the
               split is inf - inf) in a third; pixels for the NCHW entries.  Two launches: every row that no poisoned operand
               reaches keeps the bits of the clean run; in a reached row every output is non-finite, behind a ReLU as well.

fpn_stage takes `planes` (x3 and its cancel form) and `containment` on its 3 x 3 product only: the lateral input is zero with an
identity norm, so y = enc exactly.  It does not take `routing`, and the lateral product is not probed: its 2 x 2 mean rounds
before the split, so no operand with prescribed pieces can be put in front of it."""
import functools
import types

import numpy as np
import torch

U = 2.0 ** -24
VARIANTS = ["x3", "w3", "x2w2"]
KEPT = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]          # (piece of x, piece of w): hi, then the five terms of lo
BIG = 0x7F7FFFFF                                                    # largest finite fp32, above the split's domain


# ---- the split, emulated ----------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even, subnormals kept, overflow to inf) as an fp32 array."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32)
    out = r.view(np.float32).copy()
    out[np.isnan(x)] = np.nan
    return out


def split3(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a1 = bf16_rne(x)
        r = x - a1
        a2 = bf16_rne(r)
        s = r - a2
        a3 = bf16_rne(s)
    return a1, a2, a3


def six_terms(x, w, drop=(), xplanes=(0, 1, 2), wplanes=(0, 1, 2)):
    """x [rows, K], w [n, K] fp32 -> (hi, lo) float64 [rows, n].  `drop`: terms of KEPT left out; xplanes / wplanes: which
    piece sits in which plane (the mutations of the sensitivity test)."""
    a = [p.astype(np.float64) for p in split3(x)]
    b = [p.astype(np.float64) for p in split3(w)]
    a, b = [a[i] for i in xplanes], [b[j] for j in wplanes]
    hi = a[0] @ b[0].T
    lo = np.zeros_like(hi)
    for (i, j) in KEPT[1:]:
        if (i, j) not in drop:
            lo = lo + a[i] @ b[j].T
    return hi, lo


def dropped(x, w):
    a = [p.astype(np.float64) for p in split3(x)]
    b = [p.astype(np.float64) for p in split3(w)]
    return a[1] @ b[2].T + a[2] @ b[1].T + a[2] @ b[2].T


def relu_keep_nan(v):
    """the ReLU of the kernels' epilogues"""
    v = np.asarray(v)
    return np.where((v > 0) | (v != v), v, np.zeros_like(v))


# ---- integer pieces -----------------------------------------------------------------------------------------------------------
def _tz(a):
    """least number of trailing zero bits over the non-zero entries of an integer array (None: all zero)"""
    a = np.abs(a[a != 0]).astype(np.int64)
    if a.size == 0:
        return None
    return int(np.min(np.log2((a & -a).astype(np.float64))).round())


def _prod(a, b):
    """integer matrix product a @ b.T; carried in float64, where every intermediate is an exact integer (asserted)"""
    ta, tb = _tz(a) or 0, _tz(b) or 0                              # common factors 2^ta, 2^tb taken out first
    a, b = a >> ta, b >> tb
    assert float(np.abs(a).max(initial=0)) * float(np.abs(b).max(initial=0)) * a.shape[1] < 2.0 ** 53
    return (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64) << (ta + tb)


def _absprod(a, b):
    return _prod(np.abs(a), np.abs(b))


def check_accumulators(X, W):
    """X, W: three int64 piece arrays each ([rows, K], [n, K]).  Asserts the rule, -> T as integers (units 2^(ex + ew))."""
    g = _tz(X[0]), _tz(W[0])
    if g[0] is not None and g[1] is not None:
        assert int(_absprod(X[0], W[0]).max()) >> (g[0] + g[1]) < 2 ** 24, "hi chain can round"
    tzs = [_tz(X[i]) + _tz(W[j]) for (i, j) in KEPT[1:] if _tz(X[i]) is not None and _tz(W[j]) is not None]
    lo_abs = sum(_absprod(X[i], W[j]) for (i, j) in KEPT[1:])
    if tzs:
        assert int(np.max(lo_abs)) >> min(tzs) < 2 ** 24, "lo chain can round"
    for (i, j) in ((1, 2), (2, 1), (2, 2)):
        assert not X[i].any() or not W[j].any(), "a dropped term is alive"
    return sum(_prod(X[i], W[j]) for (i, j) in KEPT)


def _to_f32(ints, exps):
    """integers times 2^exps[row] -> fp32, asserted exact"""
    v = np.ldexp(ints.astype(np.float64), np.asarray(exps, dtype=np.int64)[:, None])
    f = v.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), v), "operand is not an fp32 number"
    return f


def assert_split(f32, P, exps):
    """`split3` returns exactly the pieces P (integers times 2^exps[row]) and they sum to the operand"""
    got = split3(f32)
    for g, p in zip(got, P):
        assert np.array_equal(g.astype(np.float64), np.ldexp(p.astype(np.float64), np.asarray(exps, dtype=np.int64)[:, None]))
    assert np.array_equal(sum(g.astype(np.float64) for g in got), f32.astype(np.float64))     # a1 + a2 + a3 == x


# ---- menus --------------------------------------------------------------------------------------------------------------------
ODD = (1, 3, 5, 7)


@functools.lru_cache(maxsize=None)
def menu(kind, wide):
    """All (p1, p2, p3) with p_i = +-odd * 2^s_i (integers, unit 2^-20 of the leading piece) that `split3` returns unchanged.
    kind 3: three pieces, 2: planes 1 and 2, 1: first plane; wide: the larger second pieces (K <= 128 only: the lo rule)."""
    s2s = (11, 12) if wide else (10, 11)
    if kind == 1:
        return np.array([(m, 0, 0) for m in ODD], dtype=np.int64)
    cand = []
    for m1 in ODD:
        for s2 in ((11,) if kind == 2 else s2s):
            for m2 in ODD:
                for g2 in (1, -1):
                    if kind == 2:
                        cand.append((m1 << 20, g2 * (m2 << s2), 0))
                        continue
                    for s3 in (0, 1, 2):
                        for m3 in ODD:
                            for g3 in (1, -1):
                                cand.append((m1 << 20, g2 * (m2 << s2), g3 * (m3 << s3)))
    cand = np.array(cand, dtype=np.int64)
    total = cand.sum(axis=1).astype(np.float64)
    f = total.astype(np.float32)
    ok = f.astype(np.float64) == total
    a = split3(f)
    for i in range(3):
        ok &= a[i].astype(np.float64) == cand[:, i].astype(np.float64)
    out = cand[ok]
    assert len(out) >= 16, (kind, wide, len(out))
    return out


def _draw(rng, table, shape):
    """-> three integer piece arrays of `shape`, random signs"""
    idx = rng.randint(0, len(table), size=shape)
    sign = rng.choice([-1, 1], size=shape)
    return [table[idx, i] * sign for i in range(3)]


def _first_plane(rng, shape):
    return [rng.choice(ODD, size=shape).astype(np.int64) * rng.choice([-1, 1], size=shape), np.zeros(shape, np.int64),
            np.zeros(shape, np.int64)]


def _partners(table, probed):
    """for every menu entry the entries that agree with it in all pieces but `probed` (and differ there)"""
    keep = [i for i in range(3) if i != probed]
    out = []
    for e in table:
        same = np.all(table[:, keep] == e[keep], axis=1) & (table[:, probed] != e[probed])
        out.append(np.nonzero(same)[0])
    return out


def _cancel_side(rng, table, count, K, probes, unit, rotate=True, block=1, positive=False):
    """`count` rows of K values in groups of `unit` consecutive k (row i rotated by i % 2 when unit == 2): inside a group the
    entries agree but for the piece probes[(i // block) % len(probes)].  positive: no negative values (a hidden layer behind a
    ReLU).  -> three piece arrays [count, K] in the order (A, A', A, A', ...)"""
    P = [np.zeros((count, K), np.int64) for _ in range(3)]
    which = np.asarray(probes)[(np.arange(count) // block) % len(probes)]
    for pr in sorted(set(probes)):
        rows = np.nonzero(which == pr)[0]
        lists = _partners(table, pr)
        cnt = np.array([len(p) for p in lists])
        pad = np.zeros((len(table), max(1, cnt.max())), np.int64)
        for j, p in enumerate(lists):
            pad[j, :len(p)] = p
        have = np.nonzero(cnt)[0]
        assert len(have) >= 8
        first = have[rng.randint(0, len(have), size=(len(rows), K // 2))]
        second = pad[first, rng.randint(0, 1 << 30, size=first.shape) % cnt[first]]
        sign = rng.choice([1, 1] if positive else [-1, 1], size=first.shape)
        for piece in range(3):
            vals = np.empty((len(rows), K), np.int64)
            vals[:, 0::2], vals[:, 1::2] = table[first, piece] * sign, table[second, piece] * sign
            if unit == 4:                                        # (A, A', A, A') per quad: repeat each pair
                quad = vals.reshape(len(rows), K // 4, 4)
                quad[:, :, 2:] = quad[:, :, :2]
            P[piece][rows] = vals
    if unit == 2 and rotate:
        odd = (np.arange(count) % 2 == 1)[:, None]
        P = [np.where(odd, np.roll(p, 1, axis=1), p) for p in P]
    return P


def _alternating(rng, count, K):
    """first-plane rows (-1)^k * (+-odd): any two neighbouring k carry +c / -c"""
    mag = rng.choice(ODD, size=(count, 1)).astype(np.int64) * rng.choice([-1, 1], size=(count, 1))
    alt = np.where(np.arange(K) % 2 == 0, 1, -1)[None, :]
    return [mag * alt, np.zeros((count, K), np.int64), np.zeros((count, K), np.int64)]


def _seed(*parts):
    h = 0
    for p in parts:
        if isinstance(p, str):
            p = sum((i + 1) * ord(ch) for i, ch in enumerate(p))
        h = (h * 1000003 + int(p) + 17) % (2 ** 31 - 1)
    return h


# ---- the 2-d cases: y = act((x [+ x_add]) w^T + bias) --------------------------------------------------------------------------
def bound(T, want):
    return 2.0 * U * (np.abs(T) + np.abs(want))


def _finish(case, T, bias, relu):
    case.T = T
    pre = T + (0.0 if bias is None else bias.astype(np.float64)[None, :])
    case.want = np.maximum(pre, 0.0) if relu else pre
    case.bound = bound(T, case.want)
    case.bias, case.relu = bias, relu
    return case


@functools.lru_cache(maxsize=None)
def gemm_case(family, variant, cancel, rows, n, K, relu=False, with_bias=True, period=0, ex_set=(-2, -1, 0, 1, 2),
              ew_set=(-1, 0, 1), use_add=True, seed=0, w_probes=(1, 2), x_probes=(1, 2), x_block=1, w_block=1,
              x_positive=False):
    """One product.  -> case with x [rows, K], w [n, K], bias [n] or None, x_add [period, K] or None (fp32 numpy), the exact T,
    want and bound (float64), and the exponents.  ex / ew cycle through ex_set / ew_set by row (row mod period with x_add)
    and column.  x and x_add depend on (family, variant, cancel, rows, K, period, exponents, seed) alone: cases that differ in
    n, the epilogue or `use_add` (False: the product of the stored x without x_add, a segment of a multi call) share them.
    Cancel forms only: variant "x2" is x3 with two-piece x (probes a2 w1 alone; its x has 12 bits); x_probes / w_probes: the
    pieces probed, changing every x_block rows / w_block columns; x_positive: x >= 0, the signs of a pair sit in w."""
    assert not (cancel and period) and K % 4 == 0
    rx = np.random.RandomState(_seed(family, variant, cancel, rows, K, period, seed, *ex_set, *x_probes, x_block, x_positive))
    rw = np.random.RandomState(_seed(family, variant, cancel, rows, n, K, relu, with_bias, period, use_add, seed, *ew_set, *w_probes, w_block,
                                     x_positive))
    alive = min(K, 256)
    wide = alive <= 128
    xkind, wkind = {"x3": (3, 1), "w3": (1, 3), "x2w2": (2, 2), "x2": (2, 1)}[variant]
    assert cancel or variant != "x2"
    idx = np.arange(rows) % period if period else np.arange(rows)
    D = None
    if period and xkind != 1:
        # x + x_add is the menu value and x_add moves its first piece inside the binade, off its lower end (where a second
        # piece of the other sign would leave it): first piece 5 stored as 5, 6 or 7, first piece 7 as 7, 6 or 5.  Elements a
        # period apart share their x_add element, hence its sign and the first piece
        table = menu(xkind, wide)
        t5, t7 = table[(table[:, 0] >> 20) == 5], table[(table[:, 0] >> 20) == 7]
        sgn = rx.choice([-1, 1], size=(period, K))
        seven = rx.randint(0, 2, size=(period, K)) == 1
        p5, p7 = rx.randint(0, len(t5), size=(rows, K)), rx.randint(0, len(t7), size=(rows, K))
        X = [np.where(seven[idx], t7[p7, i], t5[p5, i]) * sgn[idx] for i in range(3)]
        D = rx.randint(0, 3, size=(period, K)) * np.where(seven, 1, -1) * sgn * (1 << 20)
    elif period:
        X = _first_plane(rx, (rows, K))
        D = rx.randint(-2, 3, size=(period, K)).astype(np.int64)
    elif not cancel:
        X = _first_plane(rx, (rows, K)) if xkind == 1 else _draw(rx, menu(xkind, wide), (rows, K))
    elif variant in ("x3", "x2"):
        X = _cancel_side(rx, menu(xkind, wide), rows, K, x_probes if variant == "x3" else (1,), 2, block=x_block, positive=x_positive)
    elif variant == "w3":
        X = _alternating(rx, rows, K)
        if x_positive:                                           # +m everywhere: the pair's signs go into w below
            X[0] = np.abs(X[0])
    else:                                                        # quads x (A, A', A, A'), w (B, -B, -B', B')
        X = _cancel_side(rx, menu(2, wide), rows, K, (1,), 4, positive=x_positive)
    if not cancel:
        W = _first_plane(rw, (n, K)) if wkind == 1 else _draw(rw, menu(wkind, wide), (n, K))
    elif variant in ("x3", "x2"):
        W = _alternating(rw, n, K)
    elif variant == "w3":
        # (a window of live k must not cut a pair; with x >= 0 the pairs are (B, -B') at (2i, 2i + 1))
        W = _cancel_side(rw, menu(3, wide), n, K, w_probes, 2, rotate=K <= alive and not x_positive, block=w_block)
        if x_positive:
            for p in W:
                p[:, 1::2] *= -1
    else:
        W = _cancel_side(rw, menu(2, wide), n, K, (1,), 4)
        for p in W:
            q = p.reshape(n, K // 4, 4)
            q[:, :, :] = np.stack([q[:, :, 0], -q[:, :, 0], -q[:, :, 1], q[:, :, 1]], axis=2)
    if K > alive:                                                # at most 256 non-zero k per row, rotated with the row
        # (by 252: windows overlap, so that the shift that keeps the pairs of an odd x3 row whole leaves no k out)
        start = (alive - 4) * np.arange(rows) + (np.arange(rows) % 2 if cancel and variant in ("x3", "x2") else 0)
        live = ((np.arange(K)[None, :] - start[:, None]) % K) < alive
        X = [p * live for p in X]
        assert live.any(axis=0).all()
    ex = np.asarray(ex_set)[idx % len(ex_set)] - (0 if xkind == 1 else 20)
    ew = np.asarray(ew_set)[np.arange(n) % len(ew_set)] - (0 if wkind == 1 else 20)
    case = types.SimpleNamespace(family=family, variant=variant, cancel=cancel, rows=rows, n=n, K=K, period=period, ex=ex, ew=ew,
                                 use_add=bool(period) and use_add)
    w = _to_f32(sum(W), ew)
    assert_split(w, W, ew)
    if period:
        Xs = [X[0] - D[idx], X[1], X[2]]                         # what is stored: the menu value less the shared term
        case.x, case.x_add = _to_f32(sum(Xs), ex), _to_f32(D, ex[:period])
        assert_split(case.x, Xs, ex)                             # the stored operand splits exactly too
        xe = case.x + case.x_add[idx]                            # fp32 add
        assert_split(xe, X, ex)
        if not use_add:
            X, xe = Xs, case.x
    else:
        case.x, case.x_add = _to_f32(sum(X), ex), None
        xe = case.x
        assert_split(xe, X, ex)
    case.x_eff, case.w = xe, w
    # every k and every output column carries every live plane, the probed ones included, in some row / at some k
    for P_, kind in ((X, xkind), (W, wkind)):
        for piece in range(kind):
            assert (P_[piece] != 0).any(axis=0).all() and (P_[piece] != 0).any(axis=1).all(), (variant, piece)
    Tint = check_accumulators(X, W)
    assert float(np.abs(Tint).max()) < 2.0 ** 53
    scale = (ex[:, None] + ew[None, :]).astype(np.int64)
    T = np.ldexp(Tint.astype(np.float64), scale)
    assert not dropped(xe, w).any()
    if cancel:                                                   # the output consists of the probed plane alone
        assert not _prod(X[0], W[0]).any()
    assert scale.min() >= -126 and np.abs(T).max() < 2.0 ** 127              # every partial product a normal fp32
    bias = None
    if with_bias:                                                # any fp32 will do for the bound
        bias = (rw.randint(-9, 10, size=n) * np.ldexp(1.0, ew + int(np.median(ex)) + (8 if cancel else 24))).astype(np.float32)
    return _finish(case, T, bias, relu)


def emulate(case, x_eff=None, **mutation):
    """The six-term scheme in float64 with the kernel's roundings: fl32(hi + lo), + bias in fp32, ReLU."""
    with np.errstate(invalid="ignore", over="ignore"):
        hi, lo = six_terms(case.x_eff if x_eff is None else x_eff, case.w, **mutation)
    with np.errstate(invalid="ignore", over="ignore"):
        v = hi.astype(np.float32) + lo.astype(np.float32)
        if case.bias is not None:
            v = v + case.bias[None, :]
    return relu_keep_nan(v) if case.relu else v


def ratio(case, got):
    """worst |got - want| / bound; the bound is zero only where want and T are, and there got must be zero"""
    got = np.asarray(got, dtype=np.float64).reshape(case.want.shape)
    assert np.isfinite(got).all(), "non-finite output"
    err = np.abs(got - case.want)
    zero = case.bound == 0
    if (err[zero] != 0).any():
        return float("inf")
    return float((err[~zero] / case.bound[~zero]).max()) if (~zero).any() else 0.0


# ---- Linear + residual + LayerNorm(128): the cancel forms in front of the norm ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_norm_case(variant, rows, K, w_probes=(1, 2), seed=0):
    """norm(residual + x w^T + bias) with the cancel form of `variant` as the product: T is then a small multiple of the row's
    quantum q_r (a power of two), the residual is k q_r with |k| <= 64 and the bias zero (a per-column bias cannot be exact next
    to per-row quanta), so the pre-norm values obey `check_exact` of norm_hard_inputs.py with n = 128 and its bound holds
    unchanged.  The plain forms cannot: their T needs the one rounding of hi + lo.  (w3 probes ONE plane of w per case, w_probes =
    (1,) or (2,): with both in the columns of one row the row's values would span more than 24 bits.)
    -> a case as norm_hard_inputs builds them (inputs x, weight, bias, residual, gamma, beta; eps, want, bound) + .gemm"""
    import norm_hard_inputs as nh
    g = gemm_case("planes", variant, True, rows, 128, K, False, False, 0, (-2, -1, 0, 1, 2), (0,), seed=seed, w_probes=w_probes)
    rng = np.random.RandomState(_seed("layer_norm", variant, rows, K, seed, *w_probes))
    unit = np.ldexp(1.0, (g.ex + g.ew[0]).astype(np.int64))                      # T = integers times unit[row]
    Tint = np.rint(g.T / unit[:, None]).astype(np.int64)
    assert np.array_equal(Tint * unit[:, None], g.T)
    tz = np.array([_tz(row) or 0 for row in Tint])
    quantum = unit * 2.0 ** tz
    residual = rng.randint(-64, 65, size=(rows, 128)) * quantum[:, None]
    gamma, beta = nh._gamma_beta(rng, 128)
    pre = residual + g.T
    nh.check_exact(pre, quantum)
    assert (g.T != 0).mean() > 0.8                                                # the product is alive nearly everywhere
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    case = types.SimpleNamespace(family="planes", variant=variant, eps=1e-5, gemm=g, pre=pre, quantum=quantum,
                                 inputs=dict(x=t(g.x), weight=t(g.w), bias=t(np.zeros(128)), residual=t(residual), gamma=t(gamma),
                                             beta=t(beta)))
    assert np.array_equal(case.inputs["residual"].double().numpy(), residual)
    want, gz = nh.normalise_f64(pre, gamma[None].astype(np.float64), beta[None].astype(np.float64), case.eps)
    case.want, case.bound = torch.from_numpy(want), torch.from_numpy(nh.bound(want, gz, 128))
    return case


def layer_norm_emulate(case, **mutation):
    """the six-term product with the kernel's roundings, the residual added in fp32, the norm in float64"""
    import norm_hard_inputs as nh
    pre = emulate(case.gemm, **mutation) + case.inputs["residual"].numpy()
    i = case.inputs
    return nh.normalise_f64(pre.astype(np.float64), i["gamma"].double().numpy()[None], i["beta"].double().numpy()[None], case.eps)[0]


def _quantum(sets):
    """float64 [S, n] -> [S]: the largest power of two that divides every value of a set (1 for a set of zeros)"""
    m, e = np.frexp(sets)
    M = np.rint(np.ldexp(m, 53)).astype(np.int64)
    low = np.where(M != 0, e - 53 + np.log2((M & -M).astype(np.float64), where=M != 0, out=np.zeros(M.shape)), np.inf)
    low = low.min(axis=1)
    return np.ldexp(1.0, np.where(np.isfinite(low), low, 0).astype(np.int64))


def _norm_case(pre, n_out, inputs, gamma_sets, beta_sets, to_out, **extra):
    """Assert the rule of norm_hard_inputs.py on the pre-norm sets and attach its reference and bound, unchanged."""
    import norm_hard_inputs as nh
    quantum = _quantum(pre)
    nh.check_exact(pre, quantum)
    case = types.SimpleNamespace(family="planes", eps=1e-5, pre=pre, quantum=quantum, inputs=inputs, **extra)
    want, gz = nh.normalise_f64(pre, gamma_sets, beta_sets, case.eps)
    case.want = torch.from_numpy(np.ascontiguousarray(to_out(want)))
    case.bound = torch.from_numpy(np.ascontiguousarray(to_out(nh.bound(want, gz, pre.shape[1]))))
    return case


def _t(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    assert np.array_equal(t.double().numpy(), np.asarray(a, dtype=np.float64))      # the input is an fp32 number
    return t


# ---- conv1x1 + GroupNorm(32, 128) into token rows ------------------------------------------------------------------------------
GROUPNORM_VARIANTS = [("x3", (1, 2)), ("w3", (1, 2)), ("x2w2", (1, 2))]


@functools.lru_cache(maxsize=None)
def groupnorm_case(variant, K, H, W, N=2):
    """GroupNorm(32, 128)(conv1x1(x) + bias) as token rows with the cancel form of `variant` as the product.  A set is (image,
    group of 4 channels) = 4 H W values: the probed piece changes with the image (x3: a2 in image 0, a3 in image 1) or with the
    group (w3), never inside a set, so a set's values are small multiples of one quantum and `check_exact` holds with n = 4 H W.
    The bias is -1, 0 or 1 times the coarsest quantum."""
    import norm_hard_inputs as nh
    HW = H * W
    g = gemm_case("planes", variant, True, N * HW, 128, K, False, False, 0, (0,), (0,), x_block=HW, w_block=4)
    rng = np.random.RandomState(_seed("groupnorm", variant, K, H, W, N))
    sets = lambda rows: rows_to_nchw(rows, N, H, W).reshape(N * 32, 4 * HW)
    bias = rng.randint(-1, 2, size=128) * _quantum(sets(g.T)).max()
    pre = sets(g.T + bias[None, :])
    gamma, beta = nh._gamma_beta(rng, 128)
    inputs = dict(x=_t(rows_to_nchw(g.x, N, H, W)), weight=_t(g.w.reshape(128, K, 1, 1)), bias=_t(bias), gamma=_t(gamma), beta=_t(beta))
    return _norm_case(pre, 4 * HW, inputs, *nh._group_layout(N, 32, HW, gamma, beta), gemm=g, variant=variant)


def groupnorm_emulate(case, **mutation):
    import norm_hard_inputs as nh
    i, g = case.inputs, case.gemm
    N, K, H, W = i["x"].shape
    pre = emulate(g, **mutation) + i["bias"].numpy()[None, :]
    gamma, beta, to_out = nh._group_layout(N, 32, H * W, i["gamma"].numpy(), i["beta"].numpy())
    sets = rows_to_nchw(pre.astype(np.float64), N, H, W).reshape(N * 32, 4 * H * W)
    return to_out(nh.normalise_f64(sets, gamma, beta, case.eps)[0])


# ---- the fused FFN: norm(x + W2 relu(W1 x + b1) + b2) --------------------------------------------------------------------------
# first GEMM (W1 x, K = 128): x is the row's own residual, so it must be short next to the product's quantum:
#     w3    x first plane, W1 three pieces, one probed piece per case      a1w2, a1w3
#     x2    x two pieces, W1 first plane                                   a2w1
#     x2w2  both two pieces                                                a2w2
# (a3w1 cannot be probed there under the rule: a three-piece x has at least 17 bits, all of them fixed by ties once a1 is chosen,
# so no pair agrees in a1 and a2 and differs in a3, and 128 values of 17 bits leave no room for the product.)  b1 = 0, W2 has two
# entries of +-2^j per row with j chosen so that W2 relu(T1) lands on x's quantum.
# second GEMM (W2 h, K = F): W1 = 0 exactly, so h = relu(b1) = b1 carries the pieces (positive; the same in every row):
#     x3    b1 three pieces (one probed piece per case), W2 first plane    a1w1 (cancelled), a2w1, a3w1
#     w3    b1 first plane, W2 three pieces in pairs (B, -B')              a1w2, a1w3
#     x2w2  both two pieces                                                a2w2
# x = k q with |k| <= 64 is the residual alone.
FFN_VARIANTS = [(1, "w3", (1,)), (1, "w3", (2,)), (1, "x2", (1,)), (1, "x2w2", (1,)),
                (2, "x3", (1,)), (2, "x3", (2,)), (2, "w3", (1,)), (2, "w3", (2,)), (2, "x2w2", (1,))]
FFN_GEOMETRIES = [(rows, F) for F in (32, 96) for rows in (37, 257)]
FFN_RANGE = (-40, -13, 0, 21, 40)


def poisoned_rows(case, name="x", big=True):
    """A norm case with a NaN, +inf and (big) the largest finite fp32 in three rows of input `name` -> (case, [rows] mask)"""
    bad = types.SimpleNamespace(**vars(case))
    t = case.inputs[name].clone()
    rows, cols = t.shape
    a, b, c = rows // 2, rows - 1, 1
    t[a, cols // 3], t[b, cols - 1] = float("nan"), float("inf")
    hit = np.zeros(rows, bool)
    hit[[a, b]] = True
    if big:
        t[c, 0] = float(np.array([BIG], np.uint32).view(np.float32)[0])
        hit[c] = True
    bad.inputs = dict(case.inputs, **{name: t})
    return bad, hit


@functools.lru_cache(maxsize=None)
def ffn_case(which, variant, probes, rows, F, ex_set=(-2, -1, 0, 1, 2)):
    """-> a case as norm_hard_inputs builds them (inputs x, w1, b1, w2, b2, gamma, beta); .gemm: the probed product, .which.
    ex_set: the exponents of the rows of a first-GEMM case (FFN_RANGE: the `range` family, rows from 2^-40 to 2^40 -- the squares
    of the norm stay inside fp32)."""
    import norm_hard_inputs as nh
    rng = np.random.RandomState(_seed("ffn", which, variant, rows, F, *probes))
    gamma, beta = nh._gamma_beta(rng, 128)
    if which == 1:
        g = gemm_case("planes", variant, True, rows, F, 128, True, False, 0, ex_set, (0,), w_probes=probes)
        hid = g.want                                             # relu(T1), exact
        assert (hid > 0).mean() > 0.2
        alive = hid.any(axis=1)
        lift = np.log2(_quantum(g.x.astype(np.float64))[alive] / _quantum(hid)[alive]).min()
        w2 = nh._sparse(rng, 128, F, 2, [-1.0, 1.0]) * 2.0 ** max(0.0, lift)
        x, w1, b1 = g.x, g.w, np.zeros(F)
    else:
        g = gemm_case("planes", variant, True, 1, 128, F, False, False, 0, (0,), (0,), w_probes=probes, x_probes=probes,
                      x_positive=True)
        assert (g.x >= 0).all()
        hid = np.repeat(g.x.astype(np.float64), rows, axis=0)    # relu(0 + b1) = b1 in every row
        w1, b1, w2 = np.zeros((F, 128)), g.x[0], g.w
        x = rng.randint(-64, 65, size=(rows, 128)) * _quantum(g.T)[0]
    inputs = dict(x=_t(x), w1=_t(w1), b1=_t(b1), w2=_t(w2), b2=_t(np.zeros(128)), gamma=_t(gamma), beta=_t(beta))
    if which == 2:
        T2 = np.repeat(g.T, rows, axis=0)
    else:                                                        # the second product of a first-GEMM case is exact as well
        T2 = hid @ inputs["w2"].double().numpy().T               # (16-bit values times +-2^j, two per column)
        unit = _quantum(hid)[:, None]                            # (rows in units of their own: a power of two commutes with the split)
        check_accumulators(split_ints_any((hid / unit).astype(np.float32)), split_ints_any(inputs["w2"].numpy()))
    pre = inputs["x"].double().numpy() + T2
    ident = lambda a: a
    return _norm_case(pre, 128, inputs, gamma[None].astype(np.float64), beta[None].astype(np.float64), ident, gemm=g, which=which,
                      variant=variant)


def split_ints_any(f32):
    """the pieces of an fp32 array as integers in units of its own finest bit"""
    a = [p.astype(np.float64) for p in split3(f32)]
    q = min(_quantum(p.reshape(1, -1))[0] for p in a if p.any())
    return [np.rint(p / q).astype(np.int64) for p in a]


def ffn_emulate(case, **mutation):
    """the probed product with the kernel's roundings and `mutation`, the other product and the residual in fp32, the norm in float64"""
    import norm_hard_inputs as nh
    i, g = case.inputs, case.gemm
    if case.which == 1:
        hid = emulate(g, **mutation)                             # relu(fl32(hi + lo))
        hi, lo = six_terms(hid, i["w2"].numpy())
        t2 = hi.astype(np.float32) + lo.astype(np.float32)
    else:
        t2 = np.repeat(emulate(g, **mutation), i["x"].shape[0], axis=0)
    pre = (i["x"].numpy() + t2).astype(np.float64)
    return nh.normalise_f64(pre, i["gamma"].double().numpy()[None], i["beta"].double().numpy()[None], case.eps)[0]


# linear_add_layer_norm (the LayerNorm epilogue of linear_k128_split.hip, 32 x 32 x 16 MFMAs): rows 33 / 97, one and three full
# tiles + 1 row.  linear_layer_norm (linear_ln_split.hip): K 32 / 96 / 1024 = 1, 3 and 32 k-chunks of 32; rows 7 / 129.
LAYER_NORM_VARIANTS = [("x3", (1, 2)), ("w3", (1,)), ("w3", (2,)), ("x2w2", (1, 2))]
LAYER_NORM_GEOMETRIES = {"linear_add_layer_norm": [(33, 128), (97, 128)],
                         "linear_layer_norm": [(rows, K) for K in (32, 96, 1024) for rows in (7, 129)]}


# ---- routing ------------------------------------------------------------------------------------------------------------------
def row_scales(count):
    return 2.0 ** (5.0 * ((np.arange(count) % 9) - 4))


def _generic(rng, shape, scales):
    """randn times scales, every element distinct in magnitude (duplicates are drawn again), the three planes alive"""
    v = (rng.standard_normal(shape) * scales[:, None]).astype(np.float32)
    for _ in range(50):
        _, first = np.unique(np.abs(v), return_index=True)
        again = np.ones(v.size, bool)
        again[first] = False
        again |= (v.reshape(-1) == 0)
        if not again.any():
            break
        fresh = (rng.standard_normal(shape) * scales[:, None]).astype(np.float32)
        v.reshape(-1)[again] = fresh.reshape(-1)[again]
    assert len(np.unique(np.abs(v))) == v.size and (v != 0).all()
    a = split3(v)
    assert all((p != 0).mean() > 0.9 for p in a)
    assert np.array_equal(sum(p.astype(np.float64) for p in a), v.astype(np.float64))       # a1 + a2 + a3 == x
    return v


@functools.lru_cache(maxsize=None)
def routing_case(mirror, rows, n, K, relu=False, period=0, seed=0):
    """-> case with x, w, x_add and `expect` [rows, n] fp32: the bits the kernel must return (compared as values)."""
    rng = np.random.RandomState(_seed("routing", mirror, rows, n, K, relu, period, seed))
    blocks = max(1, K // 128)
    kb = K // blocks
    case = types.SimpleNamespace(family="routing", mirror=mirror, rows=rows, n=n, K=K, period=period, relu=relu, bias=None)
    idx = np.arange(rows) % period if period else np.arange(rows)
    if not mirror:
        pi = rng.permutation(kb)
        w = np.zeros((n, K), np.float32)
        sel = np.zeros((n, blocks), np.int64)
        for c in range(n):
            for b in range(blocks):
                sel[c, b] = b * kb + (pi[c % kb] + 17 * (c // kb) + 5 * b) % kb
                w[c, sel[c, b]] = rng.choice([-1.0, 1.0]) * 2.0 ** rng.randint(-3, 4)
        assert (w != 0).any(axis=0).all()                        # every k is selected
        x = _generic(rng, (rows, K), row_scales(rows))
        xa = _generic(rng, (period, K), row_scales(period)) if period else None
        xe = x + xa[idx] if period else x                        # fl32(x + x_add)
        if blocks > 1:                                           # row r lives in block r mod blocks alone
            live = (np.arange(K)[None, :] // kb) == (np.arange(rows)[:, None] % blocks)
            assert not period
            x = xe = np.where(live, x, np.float32(0))
        pick = sel[:, np.arange(rows) % blocks].T                # [rows, n]
        expect = xe[np.arange(rows)[:, None], pick] * w[np.arange(n)[None, :], pick]
    else:
        assert not period
        k_of = (5 * np.arange(rows) + 3) % K
        x = np.zeros((rows, K), np.float32)
        x[np.arange(rows), k_of] = 1.0
        xa, xe = None, x
        w = _generic(rng, (n, K), row_scales(n))
        expect = w[:, k_of].T.copy()
    case.x, case.w, case.x_add, case.x_eff = x, w, xa, xe
    case.expect = relu_keep_nan(expect).astype(np.float32) if relu else expect.astype(np.float32)
    return case


def multi_routing():
    """The routing case of 135 rows, n = 256 and x_add with period 45 as three segments 128 / 256 / 128 of one multi call: the
    first and the last (rows 0-127 and 128-255 of W) add x_add, the middle one (all of W) does not.
    -> (case, [(w, use_add, expect)])"""
    case = routing_case(False, MULTI_ROWS, 256, 128, False, MULTI_PERIOD)
    k_of = np.abs(case.w).argmax(axis=1)
    plain = case.x[:, k_of] * case.w[np.arange(256), k_of][None, :]
    assert np.array_equal(case.x_eff[:, k_of] * case.w[np.arange(256), k_of][None, :], case.expect)
    return case, [(case.w[:128], True, case.expect[:, :128]), (case.w, False, plain), (case.w[128:], True, case.expect[:, 128:])]


def routed_ok(case, got):
    """bit for bit as values (-0 == +0)"""
    return np.array_equal(np.asarray(got, dtype=np.float32).reshape(case.expect.shape), case.expect)


# ---- containment --------------------------------------------------------------------------------------------------------------
def poisoned(case, only_nan=False):
    """-> (x with a NaN, +inf and the largest finite fp32 in three rows, [rows] mask of the rows a poisoned operand reaches).
    With x_add the +inf sits in x_add: it reaches its row in every period.  only_nan: the NaN alone (the fp32-MFMA kernel
    has no split that turns an inf or an overflow into NaN: its ReLU rightly returns 0 for -inf)."""
    x = case.x.copy()
    xa = None if case.x_add is None else case.x_add.copy()
    rows, K = x.shape
    a, b, c = rows // 2, rows - 1, 1
    hit = np.zeros(rows, bool)
    x[a, K // 3] = np.nan
    hit[a] = True
    if only_nan:
        return x, xa, hit
    x[c, K - 1] = np.array([BIG], np.uint32).view(np.float32)[0]
    hit[c] = True
    if xa is None:
        x[b, 0] = np.inf
        hit[b] = True
    else:
        xa[b % case.period, 0] = np.inf
        hit[np.arange(rows) % case.period == b % case.period] = True
    return x, xa, hit


def contained(hit, clean, bad):
    """-> (every output of a reached row is non-finite and the clean run is finite, the other rows kept their bits)"""
    clean = np.asarray(clean, dtype=np.float32).reshape(len(hit), -1)
    bad = np.asarray(bad, dtype=np.float32).reshape(len(hit), -1)
    return (bool(np.isfinite(clean).all()) and not bool(np.isfinite(bad[hit]).any()),
            np.array_equal(clean[~hit].view(np.uint32), bad[~hit].view(np.uint32)))


# ---- NCHW helpers -------------------------------------------------------------------------------------------------------------
def rows_to_nchw(x, N, H, W):
    """[N * H * W, K] pixel rows -> [N, K, H, W]"""
    return np.ascontiguousarray(x.reshape(N, H * W, -1).transpose(0, 2, 1)).reshape(N, -1, H, W)


def nchw_to_rows(y):
    N, C = y.shape[:2]
    return np.ascontiguousarray(y.reshape(N, C, -1).transpose(0, 2, 1)).reshape(-1, C)


# ---- the 3 x 3 product of fpn_stage -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fpn_case(cancel, H, W, N=2, seed=0):
    """enc [N, 128, H, W] with three live pieces per element (x3), W3 [128, 128, 3, 3] first plane with 256 of its 1152
    (ci, tap) alive per output channel (window rotated by 256 with co: the lo rule), b3 [128].  The cancel form pairs the
    channels (2i, 2i + 1): equal but for a2 (even co ... every pixel) and weights +c / -c.
    -> case with the im2col rows x [N H W, 1152] (k = ci * 9 + tap), w [128, 1152], T, want = relu(T + b3), bound."""
    rng = np.random.RandomState(_seed("fpn", cancel, H, W, N, seed))
    table = menu(3, False)
    P = N * H * W
    if not cancel:
        E = _draw(rng, table, (P, 128))
        Wm = _first_plane(rng, (128, 1152))
    else:
        E = _cancel_side(rng, table, P, 128, (1, 2), 2)
        E = [np.where((np.arange(P) % 2 == 1)[:, None], np.roll(p, -1, axis=1), p) for p in E]     # undo the rotation: pairs (2i, 2i+1)
        mag = rng.choice(ODD, size=(128, 1, 9)).astype(np.int64) * rng.choice([-1, 1], size=(128, 1, 9))
        Wm = [(mag * np.where(np.arange(128) % 2 == 0, 1, -1)[None, :, None] * np.ones((128, 128, 9), np.int64)).reshape(128, 1152),
              np.zeros((128, 1152), np.int64), np.zeros((128, 1152), np.int64)]
    live = ((np.arange(1152)[None, :] - 256 * np.arange(128)[:, None]) % 1152) < 256
    if cancel:                                                   # keep pairs whole: the window starts at an even channel's first tap
        live = ((np.arange(1152)[None, :] // 18 - 14 * np.arange(128)[:, None]) % 64) < 14
    assert live.any(axis=0).all() and live.sum(axis=1).max() <= 256
    Wm = [p * live for p in Wm]

    def im2col(a):                                               # [P, 128] -> [P, 1152], zero padding
        m = a.reshape(N, H, W, 128)
        pad = np.zeros((N, H + 2, W + 2, 128), a.dtype)
        pad[:, 1:-1, 1:-1] = m
        taps = [pad[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]
        return np.stack(taps, axis=-1).reshape(P, 1152)         # k = ci * 9 + tap

    zeros_p, zeros_c = np.zeros(P, np.int64), np.zeros(128, np.int64)
    enc = _to_f32(sum(E), zeros_p - 20)
    assert_split(enc, E, zeros_p - 20)
    X = [im2col(p) for p in E]
    w = _to_f32(sum(Wm), zeros_c)
    assert_split(w, Wm, zeros_c)
    Tint = check_accumulators(X, Wm)
    T = np.ldexp(Tint.astype(np.float64), -20)
    case = types.SimpleNamespace(family="planes", variant="x3", cancel=cancel, H=H, W=W, N=N, rows=P, n=128, K=1152)
    case.enc, case.w3 = rows_to_nchw(enc, N, H, W), w.reshape(128, 128, 3, 3)
    case.x = case.x_eff = im2col(enc)
    case.w, case.x_add, case.period = w, None, 0
    bias = (rng.randint(-9, 10, size=128) * 2.0 ** (-12 if cancel else 4)).astype(np.float32)
    return _finish(case, T, bias, True)


def fpn_poisoned(case):
    """-> (enc with a NaN, +inf and the largest finite fp32 in three pixels, [N H W] mask: their 3 x 3 neighbourhoods)"""
    enc = case.enc.copy()
    N, _, H, W = enc.shape
    spots = [(0, 41, H // 2, W // 2, np.nan), (N - 1, 127, H - 1, W - 1, np.inf),
             (0, 0, 0, min(W - 1, 32), np.array([BIG], np.uint32).view(np.float32)[0])]
    hit = np.zeros((N, H, W), bool)
    for (n, c, y, x, v) in spots:
        enc[n, c, y, x] = v
        hit[n, max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
    return enc, hit.reshape(-1)


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
# linear_k128 (linear_k128_split.hip): tiles of 32 rows, 128 output columns per workgroup slice, 32 per wave.  rows 7 / 33 / 97:
# a ragged single tile, one full + 1 row, three full + 1; n 128 / 256 / 384: 1, 2 and 3 slices.  spl_launch: nslots = 512 /
# min(slices, 8) rounded to 8, at least 8, so these run 8 slots with at most one tile each.  BIG_ROWS: n = 1024 has 8 slices and
# 64 slots; 6280 rows = 197 tiles (the last of 8 rows), 197 = 3 * 64 + 5: slots 0-4 own 4 tiles (two paired trips), the others
# 3 (a trip and the remainder, whose second body runs past the end); with x_add (8 images of 785 rows) the HAS_X2 loop and its
# tile + 2 nslots prefetch.  x_add with period 45 over 135 rows: the wrap falls inside tiles 1, 2 and 4.
BIG_ROWS, BIG_IMAGES = 6280, 8
LINEAR_GEOMETRIES = [(rows, n, (i + j) % 2 == 1, (i + 2 * j) % 3 != 0, 0)                    # (rows, n, relu, bias, period)
                     for i, rows in enumerate((7, 33, 97)) for j, n in enumerate((128, 256, 384))]
LINEAR_GEOMETRIES += [(135, 256, False, True, 45), (135, 128, True, False, 45)]
BIG_GEOMETRY = (BIG_ROWS, 1024, True, True, BIG_ROWS // BIG_IMAGES)
MULTI_SEGMENTS = (128, 256, 128)
MULTI_ROWS, MULTI_PERIOD = 97 + 38, 45                           # 135 rows: three images of 45
# conv1x1_nchw (conv1x1_split.hip): 128 pixels per tile, k in double-buffered steps of 16: K = 16 one step, 48 an odd number,
# 256 sixteen; H W = 128 / 256: one and two tiles per image, N = 2
CONV_GEOMETRIES = [(K, H, W) for K in (16, 48, 256) for (H, W) in ((8, 16), (8, 32))]
# fpn_stage: tiles of 4 rows x 32 columns: 5 x 33 and 8 x 64 hang over / fill both edges
FPN_GEOMETRIES = [(5, 33), (8, 64)]

PLANES = [(v, c) for v in VARIANTS for c in (False, True)]
RANGES = {  # name -> (variant, ex_set, ew_set): operands inside [2^-103, 2^100], partial products normal
    "x_small": ("x3", (-102, -95, -70), (0, 40, 97)),
    "x_large": ("x3", (60, 70, 76), (-103, -60, 0)),
    "w_small": ("w3", (0, 40, 97), (-102, -95, -70)),
    "w_large": ("w3", (-103, -60, 0), (60, 70, 76)),
    # x in [2^-110, 2^-103): third pieces down to 2^-129, most of them bf16 subnormals; the split is still exact
    "x_subnormal_pieces": ("x3", (-109, -108, -106), (5, 40, 97)),
}


def linear_planes(geometry, variant, cancel):
    rows, n, relu, with_bias, period = geometry
    build = gemm_case if rows < 1000 else gemm_case.__wrapped__          # (the large case is not kept: 150 MB of float64 each)
    return build("planes", variant, cancel, rows, n, 128, relu, with_bias, 0 if cancel else period)


def linear_range(geometry, name):
    rows, n, relu, with_bias, period = geometry
    variant, ex_set, ew_set = RANGES[name]
    return gemm_case("range", variant, False, rows, n, 128, relu, with_bias, period, ex_set, ew_set)


def conv_planes(geometry, variant, cancel):
    K, H, W = geometry
    return gemm_case("planes", variant, cancel, 2 * H * W, 128, K, False, True, 0)


def conv_range(geometry, name):
    K, H, W = geometry
    variant, ex_set, ew_set = RANGES[name]
    return gemm_case("range", variant, False, 2 * H * W, 128, K, False, True, 0, ex_set, ew_set)


MULTI_ADD = (True, False, True)                                   # add_x2 of the three segments


def multi_cases(variant, cancel):
    """Three segments 128 / 256 / 128 over the same rows (the builder gives them the same x and x_add).  Plain forms: x_add
    with period 45, added by the first and the last segment; cancel forms: no x_add.  -> [case per segment]"""
    period = 0 if cancel else MULTI_PERIOD
    cases = [gemm_case("planes", variant, cancel, MULTI_ROWS, n, 128, False, s != 1, period, use_add=MULTI_ADD[s])
             for s, n in enumerate(MULTI_SEGMENTS)]
    assert all(np.array_equal(c.x, cases[0].x) for c in cases)
    return cases


def name(val):
    return "-".join(str(int(p) if isinstance(p, bool) else p) for p in val) if isinstance(val, tuple) else str(val)

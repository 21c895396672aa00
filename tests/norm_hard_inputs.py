"""Seeded builders of the inputs on which the normalising kernels are hardest, with their float64 references, shared by
the CPU and GPU tests (numpy RandomState and torch CPU arithmetic only, so both boxes build the same data):

  * csrc/add_layernorm.hip, the LayerNorm epilogues of linear_k128.hip, linear_k128_split.hip, linear_ln_split.hip and
    ffn_fused_split.hip, csrc/groupnorm_flatten.hip and the per-tile GroupNorm records of conv1x1_split.hip.

Exactness rule (every builder obeys it, `check_exact` asserts it): all pre-normalisation values of a normalised set are
multiples of a quantum q, n * max|v| / q < 2^24 for the set size n, and n is a power of two.  Then every partial sum of
the set is an fp32 number whatever the order, the mean is exact and so is v - mean: the only roundings left in a two-pass
kernel are those of the centred sum of squares, the rsqrt and the affine tail.  With u = 2^-24, z the normalised value:

    |got - want| <= (n/2 + 16) u |gamma z| + 2u |want|                                                      (`bound`)

(a sum of n non-negative squares has relative error <= (n - 1) u in any order, rsqrt halves it; the squares themselves, the
1/n, the + eps -- also eps rounded to fp32, u/2 relative at most --, rsqrt, two multiplies and the + beta are the "about 6"
further roundings that the 16 covers; 2u |want| is the final add and the rounding of the stored result.)

Families:
  offset       v = s_r (offset + k q), integer k in [-16, 16], q = 1/4, offset 4096 (LayerNorm) or 2^20 / n (GroupNorm,
               n = 1024 and 4096): mean over spread from about 100 to 2400.  At n = 16384 (16 channels x 32 x 32) the rule
               caps offset / q below 2^24 / n = 1024, too little for a one-pass variance to leave the n/2 bound by 100 times
               with that spread: there offset = 128 and k in [-4, 4] (mean over spread 200).
               Row (or image-group) r is scaled by s_r = 2^(5 ((r mod 9) - 4)): sets that share a wave, an LDS reduction
               slot or an MFMA tile differ by up to 2^40.
  eps_matters  offset 0 or 1 (GroupNorm: min(1, 2^11 / n), the largest power of two the rule admits), q = 2^-12: the variance
               is of the order of 1e-5; eps 1e-5 and 1e-3.
  constant     every value of a set equal (0, +-3 * 2^k): the output is bit-exactly beta.
  nonfinite    the offset case with one NaN in one set and one +inf in another.

A per-column bias cannot be exact next to per-row scales over 2^40, so in the GEMM kernels' `offset` cases the Linear
biases are zero (they are small dyadics in `eps_matters` and a constant in `constant`); for conv1x1 + GroupNorm the scale
goes by group only, since the offset is the convolution's per-channel bias."""
import copy
import functools
import types

import numpy as np
import torch

U = 2.0 ** -24
FAMILIES = ["offset", "eps_matters", "constant", "nonfinite"]
EPS_VARIANTS = [(0, 1e-5), (1, 1e-5), (0, 1e-3), (1, 1e-3)]          # (offset switch, eps) of the eps_matters family
Q_EPS = 2.0 ** -12
# values of the constant sets: zero and 3 * 2^k over the exponent range of the row scales, both signs
CONSTANTS = [0.0, 3.0, -3.0 * 2.0 ** -20, 3.0 * 2.0 ** 20, 3.0 * 2.0 ** 7, -3.0 * 2.0 ** -3, 3.0 * 2.0 ** -11, -0.0]
# ... where a constant Linear bias of 1/2 is added in the epilogue: c + 1/2 must keep few enough mantissa bits for every
# partial sum j * (c + 1/2), j <= 128, to stay exact
GEMM_CONSTANTS = [0.0, 3.0, 3.0 * 2.0 ** 8, -3.0 * 2.0 ** -4, 3.0 * 2.0 ** 4, -3.0 * 2.0 ** 6, 3.0 * 2.0 ** -2]


def row_scales(count):
    return 2.0 ** (5.0 * ((np.arange(count) % 9) - 4))


def variants(family):
    """the variants a family has for every entry: (offset switch, eps) pairs, or the two ways to make a GEMM vanish"""
    return {"eps_matters": list(range(len(EPS_VARIANTS))), "constant": [0, 1]}.get(family, [0])


def check_exact(pre, quantum):
    """pre [S, n] float64 (the pre-norm values of S sets), quantum [S] or scalar: the exactness rule."""
    pre = np.asarray(pre, dtype=np.float64)
    S, n = pre.shape
    assert n > 0 and n & (n - 1) == 0, n
    q = np.broadcast_to(np.asarray(quantum, dtype=np.float64), (S,))[:, None]
    ratio = pre / q
    assert np.array_equal(ratio, np.rint(ratio)), "values are not multiples of the quantum"
    worst = float((n * np.abs(ratio).max(axis=1)).max())
    assert worst < 2.0 ** 24, worst
    assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)


def normalise_f64(pre, gamma, beta, eps):
    """The plain formula in float64 on sets [S, n] -> (want, gamma * z)."""
    pre = np.asarray(pre, dtype=np.float64)
    mean = pre.mean(axis=1, keepdims=True)
    d = pre - mean
    var = (d * d).mean(axis=1, keepdims=True)
    gz = np.asarray(gamma, dtype=np.float64) * (d / np.sqrt(var + eps))
    return gz + np.asarray(beta, dtype=np.float64), gz


def bound(want, gz, n):
    return (n / 2.0 + 16.0) * U * np.abs(gz) + 2.0 * U * np.abs(want)


def _gamma_beta(rng, c):
    gamma = rng.uniform(0.5, 1.5, c) * np.where(rng.random_sample(c) < 0.25, -1.0, 1.0)
    return gamma.astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _seed(*parts):
    h = 0
    for p in parts:
        h = (h * 1000003 + (FAMILIES.index(p) if isinstance(p, str) else int(p)) + 17) % (2 ** 31 - 1)
    return h


def _identity(a):
    return a


def _finish(case, pre, quantum, gamma_sets, beta_sets, to_out=_identity):
    """Assert the rule, attach the sets and the float64 reference in the kernel's output layout."""
    check_exact(pre, quantum)
    case.pre, case.quantum, case.n = pre, np.broadcast_to(np.asarray(quantum, dtype=np.float64), (pre.shape[0],)), pre.shape[1]
    case.gamma_sets, case.beta_sets, case.to_out = gamma_sets, beta_sets, to_out
    want, gz = normalise_f64(pre, gamma_sets, beta_sets, case.eps)
    case.want_sets, case.gz_sets = want, gz
    case.want = torch.from_numpy(np.ascontiguousarray(to_out(want)))
    case.bound = torch.from_numpy(np.ascontiguousarray(to_out(bound(want, gz, case.n))))
    case.beta_out = _t(to_out(np.broadcast_to(np.asarray(beta_sets, dtype=np.float32), pre.shape)))
    case.poisoned = None
    return case


def _poisoned(clean, edits, sets):
    """The clean case with non-finite values written into copies of some inputs; `sets`: the sets they reach."""
    case = copy.copy(clean)
    case.family, case.clean = "nonfinite", clean
    case.inputs = dict(clean.inputs)
    for name, index, value in edits:
        t = case.inputs[name].clone()
        t[index] = value
        case.inputs[name] = t
    hit = np.zeros(clean.pre.shape[0], dtype=bool)
    hit[list(sets)] = True
    case.poisoned_sets = hit
    case.poisoned = torch.from_numpy(np.ascontiguousarray(clean.to_out(np.broadcast_to(hit[:, None], clean.pre.shape))))
    return case


def _eps_variant(variant, n=1):
    """-> (offset, eps): offset 0, or the largest power of two <= 1 the rule admits for sets of n values"""
    switch, eps = EPS_VARIANTS[variant]
    return (min(1.0, 2.0 ** 11 / n) if switch and n > 1024 else float(switch)), eps


def _new(family, eps, **inputs):
    return types.SimpleNamespace(family=family, eps=eps, inputs=inputs)


# ---- add_layer_norm ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def add_layer_norm_case(family, rows, cols, with_y, variant=0):
    """inputs x, y (or None) [rows, cols], gamma, beta.  With y the offset is split between x and y (3/4 + 1/4) and so is
    k, so that x + y is exact."""
    if family == "nonfinite":
        clean = add_layer_norm_case("offset", rows, cols, with_y)
        a, b = rows // 2, rows - 1
        return _poisoned(clean, [("x", (a, cols // 3), float("nan")), ("y" if with_y else "x", (b, cols - 1), float("inf"))],
                         [a, b])
    rng = np.random.RandomState(_seed(family, rows, cols, with_y, variant))
    gamma, beta = _gamma_beta(rng, cols)
    kx, ky = rng.randint(-8, 9, size=(rows, cols)), rng.randint(-8, 9, size=(rows, cols))
    eps = 1e-5
    if family == "offset":
        s = row_scales(rows)[:, None]
        x, y, quantum = s * (3072.0 + kx / 4.0), s * (1024.0 + ky / 4.0), s[:, 0] / 4.0
    elif family == "eps_matters":
        off, eps = _eps_variant(variant)
        x, y, quantum = 0.75 * off + kx * Q_EPS, 0.25 * off + ky * Q_EPS, Q_EPS
    else:
        c = np.asarray(CONSTANTS)[(np.arange(rows) + variant) % len(CONSTANTS)][:, None] * np.ones((1, cols))
        y = c / 3.0
        x, quantum = c - y, np.where(c[:, 0] == 0, 1.0, np.abs(c[:, 0]) / 3.0)
    if not with_y:
        x, y = x + y, None
    case = _new(family, eps, x=_t(x), y=None if y is None else _t(y), gamma=_t(gamma), beta=_t(beta))
    pre = case.inputs["x"].double().numpy() + (0.0 if y is None else case.inputs["y"].double().numpy())
    return _finish(case, pre, quantum, gamma[None].astype(np.float64), beta[None].astype(np.float64))


# ---- Linear + residual + LayerNorm(128) ----------------------------------------------------------------------------------
def _sparse(rng, out_features, k, nonzeros, values):
    w = np.zeros((out_features, k))
    for c in range(out_features):
        w[c, rng.choice(k, nonzeros, replace=False)] = rng.choice(values, nonzeros)
    return w


@functools.lru_cache(maxsize=None)
def linear_layer_norm_case(family, rows, K, variant=0, relu_input=True):
    """inputs x [rows, K] (integers: 0..3 behind a ReLU, else -4..4), weight [128, K] (8 entries of {-1, -1/2, 1/2, 1} per row:
    the first bf16 plane holds them), bias [128], residual [rows, 128], gamma, beta: norm(residual + x W^T + bias)."""
    if family == "nonfinite":
        clean = linear_layer_norm_case("offset", rows, K, 0, relu_input)
        a, b = rows // 2, rows - 1
        return _poisoned(clean, [("residual", (a, 41), float("nan")), ("residual", (b, 127), float("inf"))], [a, b])
    rng = np.random.RandomState(_seed(family, rows, K, variant, relu_input))
    gamma, beta = _gamma_beta(rng, 128)
    w = _sparse(rng, 128, K, 8, [-1.0, -0.5, 0.5, 1.0])
    x = rng.randint(0, 4, size=(rows, K)) if relu_input else rng.randint(-4, 5, size=(rows, K))
    x = x.astype(np.float64)
    k = rng.randint(-16, 17, size=(rows, 128))
    bias, eps = np.zeros(128), 1e-5
    if family == "offset":
        s = row_scales(rows)[:, None]
        x, res, quantum = s * x, s * (4096.0 + k / 4.0), s[:, 0] / 4.0
    elif family == "eps_matters":
        off, eps = _eps_variant(variant)
        w, bias, res, quantum = w * 2.0 ** -11, rng.randint(-8, 9, size=128) * Q_EPS, off + k * Q_EPS, Q_EPS
    else:
        if variant == 0:
            x = np.zeros_like(x)
        else:
            w = np.zeros_like(w)
        res = np.asarray(GEMM_CONSTANTS)[np.arange(rows) % len(GEMM_CONSTANTS)][:, None] * np.ones((1, 128))
        bias, quantum = np.full(128, 0.5), 2.0 ** -5
    case = _new(family, eps, x=_t(x), weight=_t(w), bias=_t(bias), residual=_t(res), gamma=_t(gamma), beta=_t(beta))
    i = case.inputs
    pre = (i["residual"].double() + i["x"].double() @ i["weight"].double().t() + i["bias"].double()).numpy()
    return _finish(case, pre, quantum, gamma[None].astype(np.float64), beta[None].astype(np.float64))


# ---- fused FFN ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ffn_case(family, rows, F, variant=0):
    """inputs x [rows, 128], w1 [F, 128], b1 [F], w2 [128, F], b2 [128], gamma, beta: norm(x + W2 relu(W1 x + b1) + b2).
    x is its own residual, so the offset sits in x (4096 + k/4 splits exactly into the bf16 planes) and every row of W1 is
    +1, -1, +1, -1 on four columns: the offset cancels exactly in the hidden layer.  W2: two entries of +-1 per row."""
    if family == "nonfinite":
        clean = ffn_case("offset", rows, F)
        a, b = rows // 2, rows - 1
        return _poisoned(clean, [("x", (a, 41), float("nan")), ("x", (b, 127), float("inf"))], [a, b])
    rng = np.random.RandomState(_seed(family, rows, F, variant))
    gamma, beta = _gamma_beta(rng, 128)
    w1 = np.zeros((F, 128))
    for f in range(F):
        w1[f, rng.choice(128, 4, replace=False)] = [1.0, -1.0, 1.0, -1.0]
    w2 = _sparse(rng, 128, F, 2, [-1.0, 1.0])
    k = rng.randint(-16, 17, size=(rows, 128))
    b1, b2, eps = np.zeros(F), np.zeros(128), 1e-5
    if family == "offset":
        s = row_scales(rows)[:, None]
        x, quantum = s * (4096.0 + k / 4.0), s[:, 0] / 4.0
    elif family == "eps_matters":
        off, eps = _eps_variant(variant)
        x, quantum = off + k * Q_EPS, Q_EPS
        b1, b2 = rng.randint(-8, 9, size=F) * Q_EPS, rng.randint(-8, 9, size=128) * Q_EPS
    else:
        x = np.asarray(GEMM_CONSTANTS)[np.arange(rows) % len(GEMM_CONSTANTS)][:, None] * np.ones((1, 128))
        if variant == 0:                           # linear2 has no weight: its constant bias is all that reaches the sum
            w2, b1 = np.zeros_like(w2), rng.randint(-8, 9, size=F) / 4.0
        else:                                      # the hidden layer is dead: W1 x = 0 on a constant row, b1 < 0
            b1 = np.full(F, -1.0)
        b2, quantum = np.full(128, 0.5), 2.0 ** -5
    case = _new(family, eps, x=_t(x), w1=_t(w1), b1=_t(b1), w2=_t(w2), b2=_t(b2), gamma=_t(gamma), beta=_t(beta))
    i = case.inputs
    hid = torch.relu(i["x"].double() @ i["w1"].double().t() + i["b1"].double())
    pre = (i["x"].double() + hid @ i["w2"].double().t() + i["b2"].double()).numpy()
    if family != "constant":                       # the hidden values obey the rule as well (small dyadics)
        check_exact(hid.numpy().reshape(rows, -1)[:, :32], quantum)
    return _finish(case, pre, quantum, gamma[None].astype(np.float64), beta[None].astype(np.float64))


# ---- GroupNorm into token rows -------------------------------------------------------------------------------------------
def _group_layout(N, groups, HW, gamma, beta):
    """sets are (image, group): cpg * HW contiguous NCHW values -> (gamma, beta per set element; sets -> [N, HW, 128] tokens)"""
    cpg = 128 // groups
    per = lambda a: np.tile(np.repeat(a.astype(np.float64).reshape(groups, cpg), HW, axis=1), (N, 1))
    to_out = lambda sets: np.asarray(sets).reshape(N, 128, HW).transpose(0, 2, 1)
    return per(gamma), per(beta), to_out


@functools.lru_cache(maxsize=None)
def groupnorm_case(family, H, W, groups, variant=0, N=2):
    """inputs x [N, 128, H, W], gamma, beta: GroupNorm(groups, 128) then flatten(2).transpose(1, 2)."""
    HW, cpg = H * W, 128 // groups
    n, S = cpg * HW, N * groups
    if family == "nonfinite":
        clean = groupnorm_case("offset", H, W, groups, 0, N)
        ga, gb = groups // 3, groups - 1               # image 0 / group ga gets the NaN, image 1 / last group the +inf
        return _poisoned(clean, [("x", (0, ga * cpg + 1, H // 2, 3), float("nan")),
                                 ("x", (1, 127, H - 1, W - 1), float("inf"))], [ga, groups + gb])
    rng = np.random.RandomState(_seed(family, H, W, groups, variant, N))
    gamma, beta = _gamma_beta(rng, 128)
    k = rng.randint(-16, 17, size=(S, n))
    eps = 1e-5
    if family == "offset":
        s = row_scales(S)[:, None]
        off = 2.0 ** 20 / n
        if n > 4096:         # 16 channels x 32 x 32: the rule caps offset / q below 2^24 / n = 1024, so the spread shrinks instead
            off, k = 128.0, rng.randint(-4, 5, size=(S, n))
        v, quantum = s * (off + k / 4.0), s[:, 0] / 4.0
    elif family == "eps_matters":
        off, eps = _eps_variant(variant, n)
        v, quantum = off + k * Q_EPS, Q_EPS
    else:
        c = np.asarray(CONSTANTS)[(np.arange(S) + variant) % len(CONSTANTS)]
        v, quantum = c[:, None] * np.ones((1, n)), np.where(c == 0, 1.0, np.abs(c) / 3.0)
    case = _new(family, eps, x=_t(v.reshape(N, 128, H, W)), gamma=_t(gamma), beta=_t(beta))
    case.groups = groups
    return _finish(case, case.inputs["x"].double().numpy().reshape(S, n), quantum, *_group_layout(N, groups, HW, gamma, beta))


@functools.lru_cache(maxsize=None)
def conv_groupnorm_case(family, K, H, W, variant=0, N=2):
    """inputs x [N, K, H, W] (integers -4..4), weight [128, K, 1, 1] (two entries of {-1, -1/2, 1/2, 1} per row), bias [128], gamma, beta:
    GroupNorm(32, 128)(conv1x1(x)) as token rows.  The offset is the convolution's bias; group g is scaled by
    2^(5 ((g mod 9) - 4)) through its weight rows and biases."""
    HW, groups, cpg = H * W, 32, 4
    n, S = cpg * HW, N * groups
    if family == "nonfinite":
        clean = conv_groupnorm_case("offset", K, H, W, 0, N)
        ga = 11                                        # NaN in a bias: that group in every image; +inf in a pixel of the last
        return _poisoned(clean, [("bias", (ga * cpg + 2,), float("nan")), ("x", (N - 1, K // 2, H - 1, 5), float("inf"))],
                         [i * groups + ga for i in range(N)] + [(N - 1) * groups + g for g in range(groups)])
    rng = np.random.RandomState(_seed(family, K, H, W, variant, N))
    gamma, beta = _gamma_beta(rng, 128)
    w = _sparse(rng, 128, K, 2, [-1.0, -0.5, 0.5, 1.0])     # (two entries: the product must not widen the spread much)
    x = rng.randint(-4, 5, size=(N, K, HW)).astype(np.float64)
    kc = rng.randint(-16, 17, size=128)
    eps = 1e-5
    if family == "offset":
        s = np.repeat(row_scales(groups), cpg)
        w, bias, quantum = w * s[:, None], s * (2.0 ** 20 / n + kc / 4.0), np.tile(row_scales(groups), N) / 4.0
    elif family == "eps_matters":
        off, eps = _eps_variant(variant, n)
        w, bias, quantum = w * 2.0 ** -11, off + kc * Q_EPS, Q_EPS
    else:
        if variant == 0:
            x = np.zeros_like(x)
        else:
            w = np.zeros_like(w)
        c = np.asarray(CONSTANTS)[np.arange(groups) % len(CONSTANTS)]
        bias, quantum = np.repeat(c, cpg), np.tile(np.where(c == 0, 1.0, np.abs(c) / 3.0), N)
    case = _new(family, eps, x=_t(x.reshape(N, K, H, W)), weight=_t(w.reshape(128, K, 1, 1)), bias=_t(bias), gamma=_t(gamma),
                beta=_t(beta))
    i = case.inputs
    pre = torch.matmul(i["weight"].double().view(128, K), i["x"].double().view(N, K, HW)) + i["bias"].double()[None, :, None]
    return _finish(case, pre.numpy().reshape(S, n), quantum, *_group_layout(N, groups, HW, gamma, beta))


# ---- the matrix: entry -> (builder(family, *geometry, variant), geometries) -----------------------------------------------
ENTRIES = {
    "add_layer_norm": (add_layer_norm_case, [(rows, cols, with_y) for cols in (64, 128, 256) for rows in (7, 1031)
                                             for with_y in (True, False)]),
    # the wrapper takes the K = 128 kernel from 4096 rows on; x is the attention output there, not behind a ReLU
    "linear_add_layer_norm": (functools.partial(linear_layer_norm_case, relu_input=False), [(4099, 128)]),
    "linear_layer_norm": (linear_layer_norm_case, [(rows, K) for K in (32, 96, 1024) for rows in (7, 129)]),
    "ffn_layer_norm": (ffn_case, [(rows, F) for F in (32, 96) for rows in (37, 257)]),
    "groupnorm_flatten": (groupnorm_case, [(H, W, groups) for (H, W) in ((16, 16), (32, 32)) for groups in (32, 8)]),
    "conv1x1_groupnorm_tokens": (conv_groupnorm_case, [(K, H, W) for K in (32, 256) for (H, W) in ((8, 32), (32, 32))]),
}


def case_ids(entry, families=FAMILIES):
    """[(family, geometry, variant)] of an entry, for pytest.mark.parametrize"""
    return [(f, g, v) for g in ENTRIES[entry][1] for f in families for v in variants(f)]


def build(entry, family, geometry, variant=0):
    return ENTRIES[entry][0](family, *geometry, variant=variant)


def case_name(val):
    return "-".join(str(int(p) if isinstance(p, bool) else p) for p in val) if isinstance(val, tuple) else str(val)


# ---- checks on a kernel's output (torch, any device) ---------------------------------------------------------------------
def error_ratio(case, got):
    """worst |got - want| / bound over the output (offset and eps_matters)."""
    got = got.detach().double().cpu().reshape(case.want.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return float(((got - case.want).abs() / case.bound.clamp_min(1e-300)).max())


def is_beta(case, got):
    """constant: bit-exactly beta in every set"""
    return torch.equal(got.detach().cpu().reshape(case.beta_out.shape), case.beta_out)


def nonfinite_ok(case, got_clean, got_poisoned):
    """-> (the poisoned sets are entirely non-finite, everything else has the bits of the clean run)"""
    a = got_clean.detach().cpu().reshape(case.poisoned.shape)
    b = got_poisoned.detach().cpu().reshape(case.poisoned.shape)
    hit = case.poisoned
    return (not bool(torch.isfinite(b[hit]).any()) and bool(torch.isfinite(a).all()),
            torch.equal(a[~hit].view(torch.int32), b[~hit].view(torch.int32)))

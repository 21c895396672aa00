"""Float64 restatement of the dynamic mask head forward with each kernel path's documented rounding points, and the seeded
inputs of tests/test_dmh_exact_cpu.py and tests/test_dmh_exact_gpu.py (numpy RandomState only, so every box builds the same
data).  The rounding points are those of the kernels' headers:

  path "f32"        csrc/dyn_mask_head.hip, fp32 output: none; attention mask  v < 0
  path "valu_bf16"  csrc/dyn_mask_head.hip, bf16 output: logits to bf16 before the resizes, upsampled output to bf16
  path "mfma"       csrc/dyn_mask_head_mfma.hip and csrc/dyn_mask_head_fused.hip (csrc/dmh_common.hpp): features, W0's feature
                    weights, x0, W1, x1, w2 and the logits to bf16; coordinate term and biases in fp32; output to bf16
  bf16 paths' attention mask: bf16(sigmoid(bf16(v))) < 0.5, which is  bf16(v) < -2^-8  (the bf16 values below 0.5 are 2^-9
  apart; at bf16(v) = -2^-8 itself sigmoid lies 2^-24 / 48 above the rounding midpoint, so the fp32 evaluation decides).

Resize indices and weights are computed in fp32 exactly as `dm_bilinear_src` does; everything else is float64.

Three families of inputs:
  A1 / A2  "exact": every term of every accumulation of the chain is an integer multiple of one power of two q with
           sum |terms| <= 2^24 q, so every partial sum in every order is exact in fp32 and the float64 value, rounded where the
           path rounds, is the only right answer (`forward(..., exact=True)` checks the condition and lists violations).
  C        generic values with, per accumulation of K terms, the order-independent budget (K + 1) 2^-23 sum |terms|.  The
           factor is DERIVED, not measured: recursive summation of K products and a bias in any order commits at most K
           roundings of partial sums bounded by sum |terms|; the unit is 2^-23 and not 2^-24 because the matrix core's
           internal summation is not documented to round each partial sum to nearest.  A rounded quantity is "stable" when
           its pre-rounding reference value is farther from the nearest bf16 rounding boundary than the difference
           accumulated so far: it then has the reference's bits and carries difference 0; otherwise it carries e + ulp_bf16.
"""
import functools

import numpy as np

STRIDE = 4

# (N, Q, H, W, target): the smallest shapes at which each branch of the four kernels is taken
GEOMETRIES = [
    (1, 1, 1, 1, (1, 1)),          # degenerate axes: both clamps coincide in y and x
    (1, 2, 1, 16, (1, 4)),         # one row: both y clamps coincide; x2 fast path, vector loads
    (2, 3, 5, 1, (2, 1)),          # one column: both x clamps coincide; generic upsample
    (3, 7, 9, 6, (5, 4)),          # W % 4 == 2: generic upsample, scalar loads, two bands, H*W % 8 != 0
    (1, 5, 9, 7, (4, 3)),          # odd W: scalar output stores in the VALU kernel
    (2, 7, 33, 20, (9, 5)),        # W % 4 == 0, W % 8 != 0: x2 fast path with scalar loads
    (1, 3, 40, 36, (10, 9)),       # the same classes at an exact 1/4 target
    (2, 5, 16, 24, (8, 12)),       # W % 8 == 0: vector loads and stores
    (1, 101, 8, 16, (4, 8)),       # odd Q: a half-empty last query pair
    (1, 4, 70, 128, (35, 64)),     # H*W no multiple of the logits kernel's 512-pixel block; many resize bands, ragged last
    (1, 3, 24, 128, (12, 64)),     # one-launch kernel: three bands, target 1/2
    (2, 5, 8, 128, (2, 32)),       # one-launch kernel: one band (top and bottom edge in one workgroup), target 1/4
    (1, 2, 16, 128, (2, 16)),      # one-launch kernel: two bands, target 1/8
]
GENERIC_GEOMETRIES = [(2, 7, 33, 20, (9, 5)), (1, 5, 9, 7, (4, 3)), (2, 5, 16, 24, (8, 12)), (1, 3, 24, 128, (12, 64))]
GENERIC_VARIANTS = ["refpts", "scale8", "dead_half", "chan1e3"]          # each one seeded case on GENERIC_GEOMETRIES[2]
PATHS = ("f32", "valu_bf16", "mfma")


# ---- bf16 in float64 ----------------------------------------------------------------------------------------------------
def bf16(x):
    """Round to nearest even at 8 significant bits (normal range)."""
    x = np.asarray(x, np.float64)
    q = np.ldexp(1.0, np.frexp(x)[1] - 8)
    return np.rint(x / q) * q


def bf16_ulp(x):
    return np.ldexp(1.0, np.frexp(np.abs(x))[1] - 8)


def bf16_margin(x):
    """Distance from x to the nearest bf16 rounding boundary (a midpoint of two neighbouring bf16 values)."""
    a = np.abs(np.asarray(x, np.float64))
    q = bf16_ulp(a)
    t = a / q                                            # in [128, 256)
    d = np.abs(t - np.floor(t) - 0.5)
    return np.minimum(d, t - 127.75) * q                 # below a power of two the spacing halves


def is_bf16(x):
    return np.array_equal(bf16(x), np.asarray(x, np.float64))


# ---- resize -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bilinear_src(out_size, in_size):
    """`dm_bilinear_src` for every destination index, in fp32: (i0, i1, weight of i1, weight of i0)."""
    scale = np.float32(0.5) if out_size == 2 * in_size else np.float32(in_size) / np.float32(out_size)
    src = scale * (np.arange(out_size, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, lam.astype(np.float64), (np.float32(1) - lam).astype(np.float64)


def lin(a, iy, ix):
    """The blend as a linear map with non-negative weights, horizontal stage first like the kernels."""
    y0, y1, ly, hy = iy
    x0, x1, lx, hx = ix
    t = hx * a[..., x0] + lx * a[..., x1]
    return hy[:, None] * t[..., y0, :] + ly[:, None] * t[..., y1, :]


def is_half_target(H, W, target):
    th, tw = target
    return H % th == 0 and W % tw == 0 and H // th == W // tw and H // th in (2, 4, 8)


# ---- the head -----------------------------------------------------------------------------------------------------------
def _k(a, kmax=60):
    """Smallest k with a * 2^k all integers."""
    a = np.asarray(a, np.float64).ravel()
    a = a[a != 0]
    for k in range(kmax + 1):
        s = np.ldexp(a, k)
        if np.all(s == np.rint(s)):
            return k
    return kmax + 1


def _stage(pre, D, rounded, relu):
    """value, carried difference, stable set of one rounding point (module docstring)."""
    val = np.maximum(pre, 0.0) if relu else pre
    if not rounded:
        return val, (np.where(pre < -D, 0.0, D) if relu else D), None      # a unit dead on both sides carries nothing
    stable = bf16_margin(pre) > D
    if relu:
        stable = np.where(pre < 0, -pre > D, stable)
    return bf16(val), np.where(stable, 0.0, D + bf16_ulp(np.abs(pre) + D)), stable


U = 2.0 ** -23
T_BF16 = -(2.0 ** -8) * (1 + 2.0 ** -8)      # bf16(v) < -2^-8  <=>  v < T_BF16 (the tie goes to the even -2^-8)


def forward(feats, ref, params, rel, target, path, stride=STRIDE, exact=False):
    """feats [N, 16, H, W], ref [N, Q, 2], params [N, Q, G] (fp32 values) -> dict; see the module docstring."""
    assert path in PATHS
    f32in = lambda a: np.asarray(a, np.float32).astype(np.float64)
    feats, params = f32in(feats), f32in(params)
    N, C, H, W = feats.shape
    Q, HW = params.shape[1], H * W
    cin = C + (2 if rel else 0)
    o = cin * 8
    assert params.shape[2] == o + 89
    w0 = params[..., :o].reshape(N, Q, 8, cin)
    w1, w2 = params[..., o:o + 64].reshape(N, Q, 8, 8), params[..., o + 64:o + 72]
    b0, b1, b2 = params[..., o + 72:o + 80], params[..., o + 80:o + 88], params[..., o + 88]
    hidden = path == "mfma"
    rb = bf16 if hidden else (lambda a: a)
    viol = []

    def cond(what, k, sumabs):
        if exact and float(np.max(sumabs)) > 2.0 ** (24 - k):
            viol.append("%s: sum|terms| %g > 2^24 * 2^-%d" % (what, float(np.max(sumabs)), k))

    # layer 0
    f = rb(feats).reshape(N, C, HW)
    w0f = rb(w0[..., 2:] if rel else w0)
    pre = b0[..., None] + np.einsum("nqkc,ncp->nqkp", w0f, f)
    sumabs = np.abs(b0)[..., None] + np.einsum("nqkc,ncp->nqkp", np.abs(w0f), np.abs(f))
    k0 = max(_k(b0), _k(w0f) + _k(f)) if exact else 0
    extra = 0.0
    if rel:
        refd = f32in(ref)
        rx, ry = refd[..., 0] * (W * stride), refd[..., 1] * (H * stride)
        ys, xs = np.divmod(np.arange(HW), W)
        locx, locy = xs * float(stride) + stride // 2, ys * float(stride) + stride // 2
        wx, wy = w0[..., 0], w0[..., 1]
        cx, cy = wx * rx[..., None], wy * ry[..., None]
        pre = pre + wx[..., None] * (rx[..., None, None] - locx) + wy[..., None] * (ry[..., None, None] - locy)
        if hidden:
            # the MFMA paths fold wx rx + wy ry into the bias and split each weight into three bf16 pieces (twelve k-slots)
            # whose magnitudes sum to < (1 + 2^-7) |w|
            sumabs = sumabs + (np.abs(cx) + np.abs(cy))[..., None] + \
                (np.abs(wx)[..., None] * locx + np.abs(wy)[..., None] * locy) * (1 + 2.0 ** -7)
        else:
            # the VALU kernel multiplies each weight by fl(fl(rx) - loc): two more terms, and the two roundings inside each
            ax, ay = np.abs(rx[..., None, None] - locx), np.abs(ry[..., None, None] - locy)
            sumabs = sumabs + np.abs(wx)[..., None] * ax + np.abs(wy)[..., None] * ay
            extra = U * (np.abs(wx)[..., None] * (np.abs(rx)[..., None, None] + ax) +
                         np.abs(wy)[..., None] * (np.abs(ry)[..., None, None] + ay))
        if exact:
            if not (np.array_equal(rx, f32in(rx)) and np.array_equal(ry, f32in(ry))):
                viol.append("ref * (W * stride) is not exact in fp32")
            k0 = max(k0, _k(cx), _k(cy), _k(wx), _k(wy), _k(wx) + _k(rx), _k(wy) + _k(ry))
    cond("layer 0", k0, sumabs)
    # terms: bias, 16 channels; with coordinates two constants and 12 k-slots more (MFMA) or two products more (VALU)
    K0 = 17 if not rel else (31 if hidden else 19)
    x0, d0, s0 = _stage(pre, (K0 + 1) * U * sumabs + extra, hidden, True)
    # layer 1
    w1r = rb(w1)
    pre = b1[..., None] + np.einsum("nqjk,nqkp->nqjp", w1r, x0)
    sumabs = np.abs(b1)[..., None] + np.einsum("nqjk,nqkp->nqjp", np.abs(w1r), np.abs(x0) + d0)
    cond("layer 1", max(_k(b1), _k(w1r) + _k(x0)) if exact else 0, sumabs)
    x1, d1, s1 = _stage(pre, np.einsum("nqjk,nqkp->nqjp", np.abs(w1r), d0) + 10 * U * sumabs, hidden, True)
    # layer 2
    w2r = rb(w2)
    pre = b2[..., None] + np.einsum("nqk,nqkp->nqp", w2r, x1)
    sumabs = np.abs(b2)[..., None] + np.einsum("nqk,nqkp->nqp", np.abs(w2r), np.abs(x1) + d1)
    cond("layer 2", max(_k(b2), _k(w2r) + _k(x1)) if exact else 0, sumabs)
    lg, dL, sL = _stage(pre, np.einsum("nqk,nqkp->nqp", np.abs(w2r), d1) + 10 * U * sumabs, path != "f32", False)
    lg, dL = lg.reshape(N, Q, H, W), np.broadcast_to(dL, pre.shape).reshape(N, Q, H, W)
    unstable = np.zeros_like(lg) if sL is None else (~sL).reshape(N, Q, H, W).astype(np.float64)
    cond("blend stages", (_k(lg) if exact else 0) + 4, np.abs(lg))      # weights are multiples of 1/4, two stages

    out = {"logits": lg, "logit_budget": dL, "viol": viol, "x0": x0, "x1": x1}
    # x2 upsample
    iy, ix = bilinear_src(2 * H, H), bilinear_src(2 * W, W)
    up_pre, mag = lin(lg, iy, ix), lin(np.abs(lg) + dL, iy, ix)
    B = lin(dL, iy, ix) + 5 * U * mag                    # four taps: (K + 1) 2^-23 sum |w tap| covers the blend's roundings
    out["up_pre"] = up_pre
    if path == "f32":
        out["up"], out["up_bound"], out["up_bits"] = up_pre, B, np.zeros(up_pre.shape, bool)
    else:
        out["up"] = bf16(up_pre)
        out["up_bits"] = (lin(unstable, iy, ix) == 0) & (bf16_margin(up_pre) > 5 * U * mag)
        out["up_bound"] = B + 0.5 * bf16_ulp(np.abs(up_pre) + B)
    # attention mask
    th, tw = target
    iy, ix = bilinear_src(th, H), bilinear_src(tw, W)
    v, vmag = lin(lg, iy, ix), lin(np.abs(lg) + dL, iy, ix)
    out["v"] = v
    if path == "f32":
        out["mask"] = v < 0
        thr = 0.0
        amb = (v < 0) & (v >= -(2.0 ** -22))             # fp32 sigmoid returns exactly 0.5 just below 0
    else:
        vb = bf16(v)
        out["mask"] = vb < -(2.0 ** -8)
        thr = T_BF16
        amb = vb == -(2.0 ** -8)
    # weights are fp32 quotients: four roundings of the blend and two of the weights stay under 2^-20 sum |w tap|
    wtol = 0.0 if is_half_target(H, W, target) else 2.0 ** -20
    out["mask_free_exact"] = ((np.abs(v - thr) <= wtol * lin(np.abs(lg), iy, ix)) & (wtol > 0)) | amb
    out["mask_free"] = (np.abs(v - thr) <= lin(dL, iy, ix) + 2.0 ** -20 * vmag) | amb
    return out


# ---- band layout of each kernel (for the seam rows) -----------------------------------------------------------------------
def band_starts(kernel, N, Q, H, W):
    """First feature row of every band of `kernel` ("valu" | "mfma" | "fused"), as the launchers choose them."""
    if kernel == "fused":
        return list(range(0, H, 8))
    TR = min(H, ((48 * 1024 - 16) if kernel == "valu" else 16 * 1024) // (W * 4) - 2)
    while TR > 8 and N * Q * ((H + TR - 1) // TR) < 4096:
        TR = (TR + 1) // 2
    return list(range(0, H, TR))


def seam_rows(N, Q, H, W, fused):
    rows = set()
    for kern in ("valu", "mfma") + (("fused",) if fused else ()):
        for r0 in band_starts(kern, N, Q, H, W)[1:]:
            rows.update((2 * r0 - 1, 2 * r0))
    return sorted(rows)


# ---- family A: exact inputs ---------------------------------------------------------------------------------------------
def a1_features(N, H, W, seed):
    """Non-negative integers of at most 8 bits, a different pattern per channel and image, monotone along neither axis, plus
    isolated impulses at the four corners and next to every border (channels 0 .. 3)."""
    c = np.arange(16)[:, None, None]
    y = np.arange(H)[None, :, None]
    x = np.arange(W)[None, None, :]
    f = np.empty((N, 16, H, W))
    for n in range(N):
        f[n] = ((y * (5 + c) + x * (3 + 2 * c) + ((x * y) % 7) * (c + 1) + c * c + 3 * n + seed) * 37) % 16 + 1
        spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (1, W // 2), (H - 2, W // 3), (H // 2, 1), (H // 3, W - 2)]
        for i, (yy, xx) in enumerate(spots):
            if 0 <= yy < H and 0 <= xx < W:
                f[n, (i + n) % 4, yy, xx] = 255 - 2 * i
    return f


def _pack(w0, w1, w2, b0, b1, b2, rel):
    """w0 [8, 18] (columns 0, 1: coordinate weights) -> one parameter row in parse_dynamic_params order."""
    return np.concatenate([(w0 if rel else w0[:, 2:]).ravel(), w1.ravel(), w2, b0, b1, [b2]])


def _draw_rows(rng, rows, cols, first, second, p_second):
    m = np.zeros((rows, cols))
    for r in range(rows):
        a = rng.randint(cols)
        m[r, a] = first[rng.randint(len(first))]
        if rng.random_sample() < p_second:
            b = (a + 1 + rng.randint(cols - 1)) % cols
            m[r, b] = second[rng.randint(len(second))]
    return m


SEL = [1.0, -1.0]
MIX = [0.5, -0.5, 0.25, -0.25, 1.0, -1.0]


def _query_ok(feats_n, row, rel, ref_q, target, family, want_signs):
    lgs = []
    for path in PATHS:
        o = forward(feats_n[None], ref_q[None, None], row[None, None], rel, target, path, exact=True)
        if o["viol"]:
            return False
        lg = o["logits"]
        if want_signs and lg.size >= 4 and not 0.2 <= float((lg < 0).mean()) <= 0.8:
            return False
        lgs.append(o)
    if family == "a1":          # every intermediate bf16-exact: the hidden roundings change nothing
        if not all(np.array_equal(lgs[0][k], lgs[2][k]) for k in ("x0", "x1", "logits")) or not is_bf16(lgs[0]["logits"]):
            return False
    return True


@functools.lru_cache(maxsize=None)
def exact_case(gi, family, rel, seed=None, Q=None):
    """Inputs of exact family "a1" (pass-through: every intermediate bf16-exact) or "a2" (coordinates and finer dyadic
    weights: pre-rounding values exactly known, not bf16-exact) at GEOMETRIES[gi].  -> dict of fp32 arrays."""
    N, Q0, H, W, target = GEOMETRIES[gi]
    Q = Q0 if Q is None else Q
    seed = (A1_SEEDS if family == "a1" else A2_SEEDS).get(gi, 0) if seed is None else seed
    rng = np.random.RandomState(1000 * gi + seed + (500 if family == "a2" else 0))
    if family == "a1":
        feats = a1_features(N, H, W, seed)
    else:
        feats = a1_features(N, H, W, seed) % 8
        feats[:, 12:] = 0.0
    refs = np.array([0, 63, -16, 80, 17, 40, 64, 5, 33]) / 64.0
    ref = np.zeros((N, Q, 2))
    params = np.zeros((N, Q, (18 if rel else 16) * 8 + 89))
    for n in range(N):
        for q in range(Q):
            ref[n, q] = refs[(q + 2 * n) % 9], refs[(3 * q + n + 1) % 9]
            kind = ["mix", "single", "dead", "mix", "mix"][q % 5] if family == "a1" else "mix"
            for attempt in range(400):
                w0 = np.zeros((8, 18))
                simple = attempt >= 300                       # a difference of two plain channels is always exact
                if family == "a1":
                    w0[:, 2:] = _draw_rows(rng, 8, 16, SEL, MIX, 0.0 if simple else 0.5)
                    w1 = _draw_rows(rng, 8, 8, SEL, MIX, 0.0 if simple else 0.4)
                    b0, b1 = rng.randint(-6, 7, 8).astype(float), rng.randint(-4, 5, 8).astype(float)
                else:
                    w0[:, 2:] = _draw_rows(rng, 8, 16, MIX + [0.125, -0.125], MIX, 0.6)
                    e = rng.randint(2, 5, (8, 2))
                    w0[:, :2] = np.where(rng.random_sample((8, 2)) < 0.6, rng.choice(SEL, (8, 2)) * 2.0 ** -e, 0.0)
                    w1 = _draw_rows(rng, 8, 8, SEL + [0.5, -0.5], [0.5, -0.5, 1.0, -1.0], 0.6)
                    b0, b1 = rng.randint(-6, 7, 8).astype(float), rng.randint(-4, 5, 8) * 0.5
                w2 = np.zeros(8)
                i, j = rng.choice(8, 2, replace=False)
                w2[i], w2[j] = 1.0, (-1.0 if family == "a1" or rng.random_sample() < 0.5 else -0.5)
                b2 = float(2 * rng.randint(-2, 2) + 1)                       # odd
                if family == "a2" and not rel:
                    # without the coordinate term the logits live on a coarse grid (multiples of 2^-5 at the finest) around 0;
                    # an odd multiple of 2^-10 on top keeps every blend with weights k / 16 away from an exact 0
                    b2 += (2 * ((q + n) % 2) + 1) * 2.0 ** -10 * (1 if q % 3 else -1)
                if kind == "single":         # logits = one feature channel unchanged
                    ch = (q + n) % 16
                    w0[:] = 0.0
                    w0[0, 2 + ch] = 1.0
                    w1[:], w2[:], b0[:], b1[:], b2 = 0.0, 0.0, 0.0, 0.0, 0.0
                    w1[0, 0] = w2[0] = 1.0
                elif kind == "dead":         # first layer dead: logits = w2 . relu(b1) + b2 over the whole plane
                    b0[:] = -32768.0
                    b1 = np.abs(b1) + 1.0
                    w2[i], w2[j] = 1.0, -0.5
                    if b1[i] - 0.5 * b1[j] + b2 == 0:
                        b2 -= 2.0
                row = _pack(w0, w1, w2, b0, b1, b2, rel)
                if kind != "mix" or _query_ok(feats[n], row, rel, ref[n, q], target, family, attempt < 200):
                    break
            else:
                raise AssertionError("no exact parameters found for query %d of geometry %d" % (q, gi))
            params[n, q] = row
    return {"feats": feats.astype(np.float32), "ref": ref.astype(np.float32), "params": params.astype(np.float32),
            "rel": rel, "target": target, "geometry": (N, Q, H, W)}


# seeds per geometry under which the census and the caps of tests/test_dmh_exact_cpu.py hold (found by running them)
A1_SEEDS = {2: 34, 3: 3, 4: 93, 5: 332, 6: 37}
A2_SEEDS = {3: 1, 5: 1, 7: 1}


@functools.lru_cache(maxsize=None)
def exact_reference(gi, family, rel, path, Q=None):
    c = exact_case(gi, family, rel, None, Q)
    return forward(c["feats"], c["ref"], c["params"], rel, c["target"], path, exact=True)


# ---- B: census ------------------------------------------------------------------------------------------------------------
def _variants(idx, size):
    """The wrong-neighbour and swapped-weight versions of one axis' (i0, i1, l1, l0): (name, mutated idx, applicable)."""
    i0, i1, l1, l0 = idx
    out = []
    for name, which, step in (("i0-1", 0, -1), ("i0+1", 0, 1), ("i1-1", 1, -1), ("i1+1", 1, 1)):
        old = idx[which]
        new = np.clip(old + step, 0, size - 1)
        m = (new, i1, l1, l0) if which == 0 else (i0, new, l1, l0)
        out.append((name, m, (new != old) & ((l0 if which == 0 else l1) != 0)))      # a zero weight hides its tap by definition
    out.append(("swap", (i0, i1, l0, l1), (l0 != l1) & (i0 != i1)))
    return out


def census(logits, target):
    """For every output row and column of the upsampled plane and every target row of the mask: a wrong neighbour index or
    swapped blend weights must change at least one output bit there.  -> list of blind spots (empty = none)."""
    N, Q, H, W = logits.shape
    blind = []
    iy, ix = bilinear_src(2 * H, H), bilinear_src(2 * W, W)
    base = bf16(lin(logits, iy, ix))
    for name, m, app in _variants(iy, H):
        ch = (bf16(lin(logits, m, ix)) != base).any(axis=(0, 1, 3))
        blind += [("up row", int(r), name) for r in np.nonzero(app & ~ch)[0]]
    for name, m, app in _variants(ix, W):
        ch = (bf16(lin(logits, iy, m)) != base).any(axis=(0, 1, 2))
        blind += [("up col", int(r), name) for r in np.nonzero(app & ~ch)[0]]
    th, tw = target
    iy, ix = bilinear_src(th, H), bilinear_src(tw, W)
    v = lin(logits, iy, ix)
    for name, m, app in _variants(iy, H):
        vm = lin(logits, m, ix)
        for rule, bits in (("f32", lambda t: t < 0), ("bf16", lambda t: bf16(t) < -(2.0 ** -8))):
            ch = (bits(vm) != bits(v)).any(axis=(0, 1, 3))
            blind += [("mask row " + rule, int(r), name) for r in np.nonzero(app & ~ch)[0]]
    return blind


# ---- family C: generic values ---------------------------------------------------------------------------------------------
C_SEEDS = {}
C_SCALE = {}


@functools.lru_cache(maxsize=None)
def generic_case(ci):
    """ci < 4: GENERIC_GEOMETRIES[ci] with operands as the older tests' `_case` draws them (standard normal features, uniform
    reference points, normal parameters * 0.3, coordinate weights * 0.02); ci >= 4: hard-value variant GENERIC_VARIANTS[ci - 4]."""
    variant = None if ci < 4 else GENERIC_VARIANTS[ci - 4]
    N, Q, H, W, target = GENERIC_GEOMETRIES[ci if ci < 4 else 2]
    rng = np.random.RandomState(4000 + 10 * ci + C_SEEDS.get(ci, 0))
    feats = rng.standard_normal((N, 16, H, W))
    ref = rng.random_sample((N, Q, 2))
    params = rng.standard_normal((N, Q, 233)) * C_SCALE.get(ci, 0.3)
    w0 = params[..., :144].reshape(N, Q, 8, 18)
    w0[..., :2] *= 0.02
    if variant == "refpts":
        pts = np.array([0.0, 1.0 - 2.0 ** -24, -0.25, 1.25])
        ref = pts[(np.arange(Q)[None, :, None] + np.arange(2)[None, None, :] + np.arange(N)[:, None, None]) % 4]
    elif variant == "scale8":
        params *= 8.0
    elif variant == "dead_half":
        params[:, ::2, 216:224] = -1000.0
    elif variant == "chan1e3":
        feats[:, 3] *= 1e3
    return {"feats": feats.astype(np.float32), "ref": ref.astype(np.float32), "params": params.astype(np.float32),
            "rel": True, "target": target, "geometry": (N, Q, H, W)}


@functools.lru_cache(maxsize=None)
def generic_reference(ci, path):
    c = generic_case(ci)
    return forward(c["feats"], c["ref"], c["params"], True, c["target"], path)

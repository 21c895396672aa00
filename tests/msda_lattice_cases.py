"""Seeded MSDeformAttn inputs whose samples sit ON the pixel lattice and ON the gate (numpy only, shared by CPU and GPU tests
like msda_cases.py).

grad_sampling_loc is one-sided where a pixel coordinate px = loc * W - 0.5 is an integer k (the cell [k, k + 1] is used:
floor) and at the gate (-1 < px < W, cuh:290-296).  The other MSDA tests leave samples within 1e-3 px of an integer out, since
a kernel forms px with one FMA and the C oracle with two roundings, and the two may floor to different cells.  Here both
roundings are computed for every coordinate,

    two = fl(fl(loc * W) - 0.5)          (the oracle's)
    one = fl(loc * W - 0.5)              (an FMA's; the product is exact in float64)

and a sample is `decided` where they are equal in x and y: there every correct formulation sees the same fp32 coordinate and
nothing has to be masked.  On power-of-two maps loc * W is exact, so every sample is decided (asserted).

Every builder returns make_case's dict plus
    pix      [N, Lq, M, L, P, 2] float32   the pixel coordinates (x, y), `two` above
    decided  [N, Lq, M, L, P]    bool
    exact    [N, Lq, M, L, P]    bool      `pix` is the exact value of loc * W - 0.5 (what float64 arithmetic sees)
    family, geometry                       names for test ids
"""
import numpy as np

from msda_cases import init_like_offsets, make_case, pixel_centres, starts_of

PYR_WIN = [(16, 16), (32, 32), (64, 64)]          # N = 1: 43 008 records, the smallest call the windowed kernels accept
PYR_SMALL = [(16, 16), (8, 8), (4, 4)]
PYR_NONPOW2 = [(17, 22), (33, 44), (65, 87)]
PYR_L5 = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64)]
GEOMETRIES = {"win": (PYR_WIN, 1), "small": (PYR_SMALL, 2), "nonpow2": (PYR_NONPOW2, 1), "l5": (PYR_L5, 1)}
M, D, P = 8, 16, 4

UNDECIDED_CAP = 0.10          # non-power-of-two maps: at most this share of samples may be undecided ...
ON_LATTICE_MIN = 0.50         # ... and at least this share of a lattice family is decided AND on an integer in x or y


def n_px(shapes):
    return sum(h * w for h, w in shapes)


def sizes_wh(shapes):
    """[L, 2] (W_l, H_l) as float64."""
    shapes = np.asarray(shapes, dtype=np.int64)
    return np.stack([shapes[:, 1], shapes[:, 0]], -1).astype(np.float64)


def is_pow2(shapes):
    return all(int(v) & (int(v) - 1) == 0 for v in np.asarray(shapes).ravel())


def pixel_coords(loc, shapes):
    """-> (two, one): fp32 pixel coordinates of fp32 locations [..., L, P, 2] under both roundings."""
    loc = np.asarray(loc)
    assert loc.dtype == np.float32
    wh = sizes_wh(shapes)[:, None, :]                                              # [L, 1, 2]
    two = (loc * wh.astype(np.float32)).astype(np.float32) - np.float32(0.5)
    assert two.dtype == np.float32
    one = (loc.astype(np.float64) * wh - 0.5).astype(np.float32)                   # 24-bit x 7-bit product: exact in float64
    return two, one


def gated_out(c):
    """[N, Lq, M, L, P] bool: px <= -1 or px >= W in either coordinate, by the recorded fp32 coordinate."""
    wh = sizes_wh(c["shapes"])[:, None, :].astype(np.float32)
    return ((c["pix"] <= -1) | (c["pix"] >= wh)).any(-1)


def on_lattice(c):
    """[N, Lq, M, L, P] bool: the recorded coordinate is an integer in x or in y."""
    return (c["pix"] == np.round(c["pix"])).any(-1)


def _finish(c, family, geometry):
    two, one = pixel_coords(c["loc"], c["shapes"])
    c["pix"] = two
    c["decided"] = (two == one).all(-1)
    # ... and where the fp32 coordinate is the exact one, so that float64 arithmetic on the widened location sees it too (a
    # location a few ulps from (-1 + 0.5) / W gives -1 + 2^-25 exactly, which fp32 rounds onto the gate)
    c["exact"] = (two.astype(np.float64) == c["loc"].astype(np.float64) * sizes_wh(c["shapes"])[:, None, :] - 0.5).all(-1)
    c["family"], c["geometry"] = family, geometry
    assert np.isfinite(c["loc"]).all()
    wh = sizes_wh(c["shapes"])[:, None, :]
    if family not in ("gate_neighbours",):                                          # (its random half follows N(0, 2 px))
        assert (two >= -5).all() and (two <= wh + 4).all(), "samples stay near the maps"
    if is_pow2(c["shapes"]):
        assert c["decided"].all(), "power-of-two maps: loc * W is exact, both roundings agree"
    else:
        undecided = 1.0 - float(c["decided"].mean())
        assert undecided <= UNDECIDED_CAP, (family, undecided)
    return c


def projected(shapes):
    """[S, L, 2] float64: every query's own pixel centre in the pixel coordinates (x, y) of every level."""
    return pixel_centres(shapes)[:, None, :] * sizes_wh(shapes)[None] - 0.5


def forced_values(size):
    """The integers every level must hold in x (size = W) and in y (size = H): gated out exactly on -1 and on the size, the
    first and the last column (whose right corners are outside), fully outside."""
    return [-2, -1, 0, size - 2, size - 1, size, size + 1]


def _base(seed, shapes, N):
    """value, attn, shapes, starts of make_case at Lq = S; loc to be replaced."""
    return make_case(seed=seed, N=N, M=M, D=D, Lq=n_px(shapes), P=P, shapes=shapes, model_like=True, px_sigma=2.0)


def lattice(geometry="win", seed=9101, local=True):
    """Every coordinate is an integer k in [-2, W + 1] (resp. H): loc = fl((k + 0.5) / W).  local: k is the cell of the query's
    own position on that level plus an integer in [-3, 3], clipped -- neighbouring queries sample neighbouring texels, what the
    windowed and column kernels stage in LDS; else uniform over [-2, W + 1] (every box is the whole level).  forced_values()
    are planted on every level in x and in y, at the queries nearest to them."""
    shapes, N = GEOMETRIES[geometry]
    c = _base(seed, shapes, N)
    rng = np.random.RandomState(seed + 1)
    sh = c["shapes"]
    L, S = sh.shape[0], n_px(shapes)
    wh = sizes_wh(sh)
    proj = projected(sh)                                                            # [S, L, 2]
    if local:
        k = np.floor(proj)[None, :, None, :, None, :] + rng.randint(-3, 4, size=(N, S, M, L, P, 2))
    else:
        k = np.floor(rng.random_sample((N, S, M, L, P, 2)) * (wh[:, None, :] + 4.0)) - 2.0
    k = np.clip(k, -2.0, wh[:, None, :] + 1.0)
    for l in range(L):
        for axis in range(2):
            for j, v in enumerate(forced_values(int(wh[l, axis]))):
                q = int(np.argmin(np.abs(proj[:, l, axis] - v)))
                k[0, q, j % M, l, axis + 2 * (j // M), axis] = v
    for l in range(L):                                                              # the planted values survived each other
        for axis in range(2):
            assert set(forced_values(int(wh[l, axis]))) <= set(np.unique(k[..., l, :, axis]).astype(int).tolist())
    c["loc"] = ((k + 0.5) / wh[:, None, :]).astype(np.float32)
    c["k"] = k.astype(np.int64)
    c = _finish(c, "lattice" if local else "lattice_uniform", geometry)
    if is_pow2(sh):
        assert np.array_equal(c["pix"], k.astype(np.float32)), "(k + 0.5) / W is exact: both roundings give k"
    else:
        share = float((c["decided"] & on_lattice(c)).mean())
        assert share >= ON_LATTICE_MIN, share
    return c


def _step_ulps(x, steps):
    """fp32 x moved by `steps` (integer array, |steps| <= 2) ulps of x itself, toward +inf for positive steps."""
    x = x.astype(np.float32).copy()
    for n in (1, 2):
        up, down = steps >= n, steps <= -n
        x = np.where(up, np.nextafter(x, np.float32(np.inf)), np.where(down, np.nextafter(x, np.float32(-np.inf)), x))
    return x.astype(np.float32)


def gate_neighbours(geometry="win", seed=9201):
    """About half of the coordinates, chosen at random, sit one or two ulps (of loc) either side of the exact location of an
    integer t in [-1, W]: the cell of the sample's own N(0, 2 px) position plus -1 / 0 / 1, so queries near a border reach the
    gate values -1 and W (H).  Every (gate, step) pair is also planted on every level at the nearest query.  A neighbour is kept
    only where both roundings agree; the other coordinates keep their random value, so a workgroup holds both kinds."""
    shapes, N = GEOMETRIES[geometry]
    c = _base(seed, shapes, N)
    rng = np.random.RandomState(seed + 1)
    sh = c["shapes"]
    L = sh.shape[0]
    wh = sizes_wh(sh)
    base = c["loc"]
    base_pix, _ = pixel_coords(base, sh)
    t = np.clip(np.floor(base_pix.astype(np.float64)) + rng.randint(-1, 2, size=base.shape), -1.0, wh[:, None, :])
    steps = rng.choice([-2, -1, 1, 2], size=base.shape)
    chosen = rng.random_sample(base.shape) < 0.5
    proj = projected(sh)
    for l in range(L):
        for axis in range(2):
            pairs = [(g, s) for g in (-1.0, wh[l, axis]) for s in (-2, -1, 1, 2)]
            for j, (g, s) in enumerate(pairs):
                q = int(np.argmin(np.abs(proj[:, l, axis] - g)))
                slot = (0, q, j % M, l, axis + 2 * (j // M), axis)
                t[slot], steps[slot], chosen[slot] = g, s, True
    cand = _step_ulps(((t + 0.5) / wh[:, None, :]).astype(np.float32), steps)
    two, one = pixel_coords(cand, sh)
    keep = chosen & (two == one)
    c["loc"] = np.where(keep, cand, base).astype(np.float32)
    c["neighbour"] = keep
    c = _finish(c, "gate_neighbours", geometry)
    assert 0.3 < float(keep.mean()) < 0.7
    if is_pow2(sh):
        inside = np.nextafter(np.float32(-1), np.float32(0))                        # gated in, weight ~ 1 on the outside corner
        for l in range(L):
            for axis in range(2):
                px = c["pix"][..., l, :, axis]
                size = np.float32(wh[l, axis])
                assert (px == inside).any() and (px == -1).any(), "both sides of the gate at -1"
                assert ((px < size) & (px > size - np.float32(1e-3))).any() and (px >= size).any(), "both sides of the gate at W / H"
                # the largest coordinate below the size that a fp32 location reaches: one ulp of loc below the exact location
                loc_below = np.nextafter(np.float32((float(size) + 0.5) / float(size)), np.float32(0))
                below = np.float32(loc_below * size) - np.float32(0.5)
                assert below < size and (px == below).any()
    return c


def init_exact(geometry="win", seed=9301):
    """The module's initial offset grid (whole pixels along eight directions) on pixel-centre reference points, no jitter: what
    the first training steps sample.  Samples on the query's own level sit on texels."""
    shapes, N = GEOMETRIES[geometry]
    c = make_case(seed=seed, N=N, M=M, D=D, Lq=n_px(shapes), P=P, shapes=shapes, init_like=True)
    return _finish(c, "init_exact", geometry)


def lattice_nonpow2(seed=9401):
    c = lattice("nonpow2", seed)
    c["family"] = "lattice_nonpow2"
    return c


def init_nonpow2(seed=9501):
    """Only the samples on the query's own level (one level in L = 3) sit on texels -- on another level the query's centre
    falls between them -- so ON_LATTICE_MIN cannot hold for this family; with at most UNDECIDED_CAP of them undecided the share
    that is decided and on the lattice is at least (1 - UNDECIDED_CAP) / L."""
    c = init_exact("nonpow2", seed)
    c["family"] = "init_nonpow2"
    share = float((c["decided"] & on_lattice(c)).mean())
    assert share >= (1.0 - UNDECIDED_CAP) / c["shapes"].shape[0], share
    return c


def inf_level(geometry="win", seed=9601, level=1):
    """The gate made visible in the FORWARD: `value` of one level is all +inf and every sample of that level is gated out on the
    lattice -- exactly on -1 or on W / H in at least one coordinate, or on -2 / W + 1.  A gate with >= or <= lets such a sample in
    with weight 0 and 0 * inf = NaN reaches the output; the reference skips it."""
    c = lattice(geometry, seed)
    rng = np.random.RandomState(seed + 2)
    sh = c["shapes"]
    wh = sizes_wh(sh)
    k = c["k"].astype(np.float64)
    shape = k[..., level, :, 0].shape
    axis = rng.randint(0, 2, size=shape)                                            # the other coordinate keeps its lattice value
    pick = rng.choice([-2.0, -1.0, 1.0, 2.0], size=shape)
    for a in range(2):                                                              # -2, -1 as they are; 1, 2 -> W, W + 1
        gate_k = np.where(pick < 0, pick, wh[level, a] + pick - 1.0)
        k[..., level, :, a] = np.where(axis == a, gate_k, k[..., level, :, a])
    c["loc"] = ((k + 0.5) / wh[:, None, :]).astype(np.float32)
    c["k"] = k.astype(np.int64)
    lo, hi = int(c["starts"][level]), int(c["starts"][level]) + int(sh[level, 0] * sh[level, 1])
    c["value"] = c["value"].copy()
    c["value"][:, lo:hi] = np.inf
    c = _finish(c, "inf_level", geometry)
    assert gated_out(c)[..., level, :].all()
    on_gate = (c["pix"][..., level, :, :] == -1) | (c["pix"][..., level, :, :] == wh[level].astype(np.float32))
    assert float(on_gate.any(-1).mean()) > 0.4, "about half of the level's samples sit exactly on the gate"
    return c


# (id, builder, kwargs): every family on the 43 008-record pyramid, the lattice on the other geometries too
CASES = [
    ("lattice-win", lattice, dict(geometry="win")),
    ("lattice_uniform-win", lattice, dict(geometry="win", seed=9111, local=False)),
    ("gate_neighbours-win", gate_neighbours, dict(geometry="win")),
    ("init_exact-win", init_exact, dict(geometry="win")),
    ("lattice-small", lattice, dict(geometry="small", seed=9121)),
    ("gate_neighbours-small", gate_neighbours, dict(geometry="small", seed=9221)),
    ("init_exact-small", init_exact, dict(geometry="small", seed=9321)),
    ("lattice-l5", lattice, dict(geometry="l5", seed=9131)),
    ("lattice_nonpow2", lattice_nonpow2, dict()),
    ("init_nonpow2", init_nonpow2, dict()),
]
CASE_IDS = [cid for cid, _, _ in CASES]
_made = {}


def records_of(cid):
    """N * Lq * M of the case, without building it (the windowed kernels decline calls of fewer than 32 768 records)."""
    kw = next(x for x in CASES if x[0] == cid)[2]
    shapes, N = GEOMETRIES[kw.get("geometry", "nonpow2")]
    return N * n_px(shapes) * M


def make(cid):
    """The case of that id, built once and not to be written."""
    if cid not in _made:
        _, fn, kw = next(x for x in CASES if x[0] == cid)
        _made[cid] = fn(**kw)
    return _made[cid]


def grad_out_for(c, seed=77):
    N, Lq = c["loc"].shape[:2]
    return np.random.RandomState(seed).standard_normal((N, Lq, M * D)).astype(np.float32)


# ---------------------------------------------------------------- the fused training entry (pctrans_amd/msda_train.py)
FUSED_CASES = {
    # name -> shapes, N, offsets: exact integers in [-3, 3] | the module's real initial grid (fp32; it holds values like
    # cos(pi / 2) = -4.4e-8, which fp32 absorbs into most reference points and float64 does not)
    "int-small": (PYR_SMALL, 2, "int", 9701),
    "init-small": (PYR_SMALL, 2, "init", 9702),
    "int-win": ([(64, 64), (32, 32), (16, 16)], 1, "int", 9703),
    "init-win": ([(64, 64), (32, 32), (16, 16)], 1, "init", 9704),
}
_fused = {}


def fused(name):
    """Operands of the fused entry in the layout of msda_fused_reference.make: pixel-centre reference points (one table for the
    batch), offsets in pixels, logits, grad_out; plus loc32 = fl(ref + fl(offsets / (W, H))), the fp32 location the entry's expand
    kernel forms, its pixel coordinates `pix` and `decided`.  Asserted: loc32 equals the single rounding of the exact sum."""
    if name in _fused:
        return _fused[name]
    shapes, N, kind, seed = FUSED_CASES[name]
    rng = np.random.RandomState(seed)
    sh = np.asarray(shapes, dtype=np.int64)
    assert is_pow2(sh)
    L, S = sh.shape[0], n_px(shapes)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    ref = np.ascontiguousarray(np.broadcast_to(pixel_centres(sh)[None, :, None, :], (1, S, L, 2)), dtype=np.float32)
    if kind == "int":
        offsets = rng.randint(-3, 4, size=(N, S, M, L, P, 2)).astype(np.float32)
    else:
        offsets = np.ascontiguousarray(np.broadcast_to(init_like_offsets(M, P)[None, None, :, None, :, :], (N, S, M, L, P, 2)),
                                       dtype=np.float32)
        assert ((offsets != 0) & (np.abs(offsets) < 1e-6)).any(), "the grid's cos(pi / 2) is not 0"
    logits = rng.standard_normal((N, S, M, L * P)).astype(np.float32)
    grad_out = rng.standard_normal((N, S, M * D)).astype(np.float32)
    wh32 = sizes_wh(sh).astype(np.float32)[None, None, None, :, None, :]
    quot = (offsets / wh32).astype(np.float32)
    loc32 = (ref[:, :, None, :, None, :] + quot).astype(np.float32)
    wide = ref.astype(np.longdouble)[:, :, None, :, None, :] + offsets.astype(np.longdouble) / wh32.astype(np.longdouble)
    assert np.finfo(np.longdouble).nmant >= 63, "the exact sum needs a 64-bit significand"
    assert np.array_equal(loc32, wide.astype(np.float32)), "power-of-two divisors: one rounding either way"
    c = dict(name=name, value=value, shapes=sh, starts=starts_of(sh), ref=ref, offsets=offsets, logits=logits, grad_out=grad_out,
             dims=(N, S, M, D, L, S, P), loc=np.ascontiguousarray(loc32))
    c = _finish(c, "fused_" + kind, name)
    assert float(on_lattice(c).mean()) > 0.2 and gated_out(c).any()
    _fused[name] = c
    return c


_fused_want = {}


def fused_reference(c):
    """float64 gradients of the entry's chain AT THE fp32 LOCATION loc32 (widened), not at the float64 sum ref + offsets / W:
    w = softmax(logits) in float64, the C oracle's float64 backward at (loc32, w), then
    grad_offsets = gloc / (W, H), grad_logits = w * (gw - sum_k w_k gw_k).  Keys as msda_fused_reference.backward."""
    if c["name"] in _fused_want:
        return _fused_want[c["name"]]
    from oracle import msda_oracle as orc
    N, S, Mh, Dd, L, Lq, Pp = c["dims"]
    x = c["logits"].astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    w = (e / e.sum(-1, keepdims=True)).reshape(N, Lq, Mh, L, Pp)
    loc = c["loc"].astype(np.float64)
    gv, gloc, gw = orc.backward(c["value"].astype(np.float64), c["shapes"], c["starts"], loc, w, c["grad_out"].astype(np.float64))
    goff = gloc / sizes_wh(c["shapes"])[None, None, None, :, None, :]
    wf, gwf = w.reshape(N, Lq, Mh, L * Pp), gw.reshape(N, Lq, Mh, L * Pp)
    glog = wf * (gwf - (wf * gwf).sum(-1, keepdims=True))
    r = dict(grad_value=gv, grad_offsets=goff, grad_logits=glog, gloc=gloc, gw=gw, loc=loc, w=w)
    _fused_want[c["name"]] = r
    return r

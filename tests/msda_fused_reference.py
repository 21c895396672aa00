"""Float64 reference of the differentiable fused MSDeformAttn front-end (include/pctrans_hip_msda_train.h) and the seeded cases
its CPU and GPU tests share (numpy only, as msda_cases.py).  The chain

    w   = softmax(attn_logits over L * P)
    loc = ref[:, :, None, :, None, :] + offsets / (W_l, H_l)
    out = ms_deform_attn(value, loc, w)

on top of the C oracle's forward / backward (oracle/msda_oracle.c): with (gv, gloc, gw) the oracle's backward at (loc, w),

    grad_value = gv        grad_offsets = gloc / (W_l, H_l)        grad_logits = w * (gw - sum_k w_k gw_k)
"""
import numpy as np

from msda_cases import pixel_centres, starts_of
from oracle import msda_oracle as orc

PYR3 = [(16, 16), (8, 8), (4, 4)]
RAGGED = [(12, 20), (6, 10), (3, 5)]

# name -> N, M, D, shapes, P, Lq (None: the pyramid's own pixels, Lq = S), refs ("shared" [1, Lq, L, 2] | "per_image"
# [N, Lq, L, 2]), offsets' sigma in pixels, logits' sigma, seed.  The smallest shapes that still cross every seam:
#   ragged_perimg  W and H are no powers of two, so offsets / (W, H) rounds; one reference table per image
#   lq37_p8        Lq != S, 8 points, 4 levels; 3 * 37 * 4 = 444 records leave a partial last workgroup of 64
#   peaked         a near-one-hot softmax
#   far_offsets    most samples fall outside the maps and are gated out
#   win_pyr3       the windowed backward kernel declines calls of fewer than 32 768 records, which is every case above: one image of
#                  a 64-32-16 pyramid (43 008 records) is the smallest of this family it takes; `auto` runs the column kernel there
CASES = {
    "pyr3_shared": dict(N=2, M=8, D=16, shapes=PYR3, P=4, Lq=None, refs="shared", px_sigma=2.0, logit_sigma=1.0, seed=4101),
    "ragged_perimg": dict(N=3, M=8, D=16, shapes=RAGGED, P=4, Lq=None, refs="per_image", px_sigma=2.0, logit_sigma=1.0, seed=4102),
    "lq37_p8": dict(N=3, M=4, D=16, shapes=[(10, 14), (5, 7), (3, 4), (2, 2)], P=8, Lq=37, refs="shared", px_sigma=2.0,
                    logit_sigma=1.0, seed=4103),
    "peaked": dict(N=2, M=8, D=16, shapes=PYR3, P=4, Lq=None, refs="shared", px_sigma=2.0, logit_sigma=12.0, seed=4104),
    "far_offsets": dict(N=2, M=8, D=16, shapes=PYR3, P=4, Lq=None, refs="shared", px_sigma=8.0, logit_sigma=1.0, seed=4105),
    "win_pyr3": dict(N=1, M=8, D=16, shapes=[(64, 64), (32, 32), (16, 16)], P=4, Lq=None, refs="shared", px_sigma=2.0,
                     logit_sigma=1.0, seed=4106),
}
TWO_PX_CASES = ("pyr3_shared", "ragged_perimg", "lq37_p8", "win_pyr3")          # offsets of N(0, 2 px) with N(0, 1) logits

_made = {}


def make(name, **override):
    """The case's fp32 operands: value [N, S, M, D], shapes [L, 2] (H, W), starts [L], ref [N or 1, Lq, L, 2], offsets
    [N, Lq, M, L, P, 2] (pixels), logits [N, Lq, M, L * P], grad_out [N, Lq, M * D].  Built once per name and not to be written."""
    key = (name, tuple(sorted(override.items())))
    if key in _made:
        return _made[key]
    kw = dict(CASES[name], **override)
    rng = np.random.RandomState(kw["seed"])
    shapes = np.asarray(kw["shapes"], dtype=np.int64)
    N, M, D, P, L = kw["N"], kw["M"], kw["D"], kw["P"], shapes.shape[0]
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    Lq = S if kw["Lq"] is None else kw["Lq"]
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    if kw["Lq"] is None:                                       # the encoder's: every pixel's centre, the same point on every level
        ref = np.broadcast_to(pixel_centres(shapes)[None, :, None, :], (1, S, L, 2))
    else:
        ref = rng.random_sample((1, Lq, L, 2))
    if kw["refs"] == "per_image":                              # ... scaled by per-image, per-level valid ratios
        ref = ref * (0.8 + 0.2 * rng.random_sample((N, 1, L, 2)))
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    offsets = (rng.standard_normal((N, Lq, M, L, P, 2)) * kw["px_sigma"]).astype(np.float32)
    logits = (rng.standard_normal((N, Lq, M, L * P)) * kw["logit_sigma"]).astype(np.float32)
    grad_out = rng.standard_normal((N, Lq, M * D)).astype(np.float32)
    c = dict(name=name, value=value, shapes=shapes, starts=starts_of(shapes), ref=ref, offsets=offsets, logits=logits,
             grad_out=grad_out, dims=(N, S, M, D, L, Lq, P))
    _made[key] = c
    return c


def sizes_wh(c):
    """[L, 2] float64 (W_l, H_l): the divisors of the location arithmetic."""
    return np.stack([c["shapes"][:, 1], c["shapes"][:, 0]], -1).astype(np.float64)


def expand(c):
    """-> (loc [N, Lq, M, L, P, 2], w [N, Lq, M, L, P]) float64 from the fp32 operands."""
    N, S, M, D, L, Lq, P = c["dims"]
    x = c["logits"].astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    w = (e / e.sum(-1, keepdims=True)).reshape(N, Lq, M, L, P)
    loc = c["ref"].astype(np.float64)[:, :, None, :, None, :] + c["offsets"].astype(np.float64) / sizes_wh(c)[None, None, None, :, None, :]
    return np.ascontiguousarray(np.broadcast_to(loc, (N, Lq, M, L, P, 2))), w


def forward(c):
    loc, w = expand(c)
    return orc.forward(c["value"].astype(np.float64), c["shapes"], c["starts"], loc, w)


_backward = {}


def backward(c, grad_out=None):
    """-> dict of float64 arrays: grad_value, grad_offsets, grad_logits of the chain, and the unfused op's gloc, gw, the expanded
    loc and w they were taken at.  Computed once per case for the case's own grad_out."""
    own = grad_out is None
    if own and id(c) in _backward:
        return _backward[id(c)]
    N, S, M, D, L, Lq, P = c["dims"]
    loc, w = expand(c)
    go = (c["grad_out"] if own else grad_out).astype(np.float64)
    gv, gloc, gw = orc.backward(c["value"].astype(np.float64), c["shapes"], c["starts"], loc, w, go)
    goff = gloc / sizes_wh(c)[None, None, None, :, None, :]
    wf, gwf = w.reshape(N, Lq, M, L * P), gw.reshape(N, Lq, M, L * P)
    glog = wf * (gwf - (wf * gwf).sum(-1, keepdims=True))
    r = dict(grad_value=gv, grad_offsets=goff, grad_logits=glog, gloc=gloc, gw=gw, loc=loc, w=w)
    if own:
        _backward[id(c)] = r
    return r


def edge_mask(c, eps=1e-3):
    """[N, Lq, M, L, P, 1] bool: samples within eps px of a cell boundary, where floor() flips and grad_loc is discontinuous (as
    tests/test_msda_bwd_col_gpu.py: edge_mask, on the chain's own locations)."""
    loc, _ = expand(c)
    pix = loc * sizes_wh(c)[None, None, None, :, None, :] - 0.5
    return (np.abs(pix - np.round(pix)) < eps).any(-1, keepdims=True)


def gated_out(c):
    """[N, Lq, M, L, P] bool: samples no corner of which lies inside its map (the op's gate: h > -1, w > -1, h < H, w < W)."""
    loc, _ = expand(c)
    pix = loc * sizes_wh(c)[None, None, None, :, None, :] - 0.5
    wh = sizes_wh(c)[None, None, None, :, None, :]
    return ~((pix > -1).all(-1) & (pix < wh).all(-1))

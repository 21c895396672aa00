"""CPU: what tests/msda_lattice_cases.py claims about its inputs, and that those inputs are hard -- that a kernel with a wrong
floor or gate rule could not pass tests/test_msda_lattice_gpu.py.

  * builder claims: both roundings of loc * W - 0.5 give k on power-of-two maps, the forced gate values occur on every level,
    the undecided share and the on-lattice share keep their caps on the non-power-of-two pyramid;
  * the fp32 C oracle (the GPU tests' reference) and the float64 oracle on the widened fp32 locations agree on all three
    gradients of the power-of-two families, i.e. the reference itself is not ambiguous there;
  * hardness: a float64 numpy restatement of the op's backward (cuh:92-164, 290-296) with the cell rule and the two gate
    comparisons as parameters reproduces the oracle with the reference's rules, and with each wrong rule -- left cell at an
    integer, truncation toward zero, `>= -1`, `<= W` -- differs from it by more than 100 x the GPU tolerance
    (2e-5 * max(1, max|ref|)) on the share of grad_sampling_loc elements asserted (and printed) below.
"""
import numpy as np
import pytest

import msda_lattice_cases as LC
from oracle import msda_oracle as orc

GPU_TOL = 2e-5
POW2_CASES = [cid for cid in LC.CASE_IDS if "nonpow2" not in cid]

_oracle = {}


def oracle_backward(cid, dtype):
    """orc.backward of the case in fp32 (on the operands as they are) or float64 (on the widened operands), computed once."""
    key = (cid, np.dtype(dtype).name)
    if key not in _oracle:
        c = LC.make(cid)
        go = LC.grad_out_for(c)
        _oracle[key] = orc.backward(c["value"].astype(dtype), c["shapes"], c["starts"], c["loc"].astype(dtype),
                                    c["attn"].astype(dtype), go.astype(dtype))
    return _oracle[key]


# ---------------------------------------------------------------- builder claims
@pytest.mark.parametrize("size", [4, 8, 16, 32, 64, 128])
def test_lattice_locations_are_exact_on_power_of_two_maps(size):
    """loc = (k + 0.5) / W is exact in fp32 and both roundings of loc * W - 0.5 equal k for every k in [-2, W + 1]."""
    k = np.arange(-2, size + 2, dtype=np.float64)
    loc64 = (k + 0.5) / size
    loc = loc64.astype(np.float32)
    assert np.array_equal(loc.astype(np.float64), loc64)
    two, one = LC.pixel_coords(loc.reshape(1, -1, 1).repeat(2, -1), [(size, size)])
    assert np.array_equal(two[0, :, 0], k.astype(np.float32)) and np.array_equal(one, two)


@pytest.mark.parametrize("cid", LC.CASE_IDS)
def test_builder_claims(cid):
    c = LC.make(cid)
    wh = LC.sizes_wh(c["shapes"])
    pow2 = LC.is_pow2(c["shapes"])
    two, one = LC.pixel_coords(c["loc"], c["shapes"])
    assert np.array_equal(two, c["pix"]) and np.array_equal((two == one).all(-1), c["decided"])
    undecided = 1.0 - float(c["decided"].mean())
    lattice = float((c["decided"] & LC.on_lattice(c)).mean())
    print("%s: undecided %.4f, decided and on the lattice %.4f, gated out %.4f" % (cid, undecided, lattice, LC.gated_out(c).mean()))
    if pow2:
        assert c["decided"].all()
    else:
        assert 0.0 < undecided <= LC.UNDECIDED_CAP                      # (0: the mask would have no reason to exist)
    if c["family"].startswith("lattice"):
        assert lattice >= (1.0 if pow2 else LC.ON_LATTICE_MIN)
        for l in range(wh.shape[0]):
            for axis in range(2):
                # (off the power-of-two maps fl((k + 0.5) / W) * W - 0.5 may miss k by an ulp: there the intended k is checked)
                here = c["pix"][..., l, :, axis] if pow2 else c["k"][..., l, :, axis]
                for v in LC.forced_values(int(wh[l, axis])):
                    assert (here == v).any(), (l, axis, v)
    if c["family"].startswith("init"):
        assert lattice >= (1.0 - LC.UNDECIDED_CAP) / wh.shape[0]
    if c["family"] == "gate_neighbours":
        assert 0.3 < float(c["neighbour"].mean()) < 0.7
        for l in range(wh.shape[0]):
            for axis in range(2):
                px, size = c["pix"][..., l, :, axis], np.float32(wh[l, axis])
                assert (px == np.nextafter(np.float32(-1), np.float32(0))).any() and (px == -1).any()
                assert ((px > size - 1e-3) & (px < size)).any() and (px >= size).any()
    g = LC.gated_out(c)
    assert 0.05 < float(g.mean()) < 0.5                                  # both sides of the gate are populated


def test_inf_level_case():
    c = LC.inf_level()
    assert LC.gated_out(c)[..., 1, :].all() and np.isinf(c["value"]).any()
    out = orc.forward(c["value"], c["shapes"], c["starts"], c["loc"], c["attn"])
    assert np.isfinite(out).all()


@pytest.mark.parametrize("name", list(LC.FUSED_CASES))
def test_fused_cases(name):
    c = LC.fused(name)                                                   # (asserts the single rounding of the location itself)
    assert c["decided"].all() and LC.gated_out(c).any()
    assert float(LC.on_lattice(c).mean()) >= 0.3


# ---------------------------------------------------------------- the two oracles agree
@pytest.mark.parametrize("cid", POW2_CASES)
def test_fp32_oracle_agrees_with_float64_oracle(cid):
    """On power-of-two maps loc * W is exact, and where the subtraction of 0.5 is exact too (`exact`: every sample of the lattice
    families; not a neighbour of -1 such as -1 + 2^-25, which fp32 rounds onto the gate and float64 does not, nor the init
    grid's -1 - 6e-8; 13 % of the samples at most) fp32 and
    float64 pick the same cell and gate and differ by fp32 rounding alone: 16 channels with ~6 roundings each, far below a
    tenth of the GPU tolerance.  grad_value is compared whole: an inexact sample carries a corner weight below 2^-24."""
    c = LC.make(cid)
    print("%s: %.4f of the samples inexact" % (cid, 1.0 - c["exact"].mean()))
    assert c["exact"].all() if c["family"].startswith("lattice") else float(c["exact"].mean()) > 0.85
    got, want = oracle_backward(cid, np.float32), oracle_backward(cid, np.float64)
    for g, w, name in zip(got, want, ("grad_value", "grad_loc", "grad_attn")):
        scale = max(1.0, float(np.abs(w).max()))
        keep = {"grad_value": True, "grad_loc": c["exact"][..., None], "grad_attn": c["exact"]}[name]
        err = float(np.where(keep, np.abs(g - w), 0.0).max())
        print("%s %s: fp32 vs float64 oracle %.2e on a scale of %.1f" % (cid, name, err, scale))
        assert err <= 0.1 * GPU_TOL * scale, name


# ---------------------------------------------------------------- hardness
CELL = {"floor": np.floor, "left": lambda x: np.ceil(x) - 1.0, "trunc": np.trunc}
LOWER = {">": lambda x: x > -1.0, ">=": lambda x: x >= -1.0}
UPPER = {"<": lambda x, size: x < size, "<=": lambda x, size: x <= size}


def np_backward(c, grad_out, cell="floor", lower=">", upper="<"):
    """float64 restatement of cuh:92-164 for grad_sampling_loc and grad_attn_weight with the channel sums taken first.  The
    corner tests are the reference's (cuh:55-80: the low corner is only tested against 0, the high one against the size), so a
    sample let in at px = W reads the next row's first texel as the reference would; a read past the last texel gives 0."""
    value = c["value"].astype(np.float64)
    N, S, Mh, Dd = value.shape
    vpad = np.concatenate([value, np.zeros((N, 1, Mh, Dd))], 1)
    loc, attn = c["loc"].astype(np.float64), c["attn"].astype(np.float64)
    Lq = loc.shape[1]
    go = grad_out.astype(np.float64).reshape(N, Lq, Mh, 1, Dd)
    gl, ga = np.zeros_like(loc), np.zeros_like(attn)
    bi, mi = np.arange(N)[:, None, None, None], np.arange(Mh)[None, None, :, None]
    for l, (H, W) in enumerate(c["shapes"].tolist()):
        x, y = loc[..., l, :, 0] * W - 0.5, loc[..., l, :, 1] * H - 0.5
        gate = LOWER[lower](x) & LOWER[lower](y) & UPPER[upper](x, W) & UPPER[upper](y, H)
        x0, y0 = CELL[cell](x), CELL[cell](y)
        lw, lh = x - x0, y - y0
        hw, hh = 1.0 - lw, 1.0 - lh
        ok = [(y0 >= 0) & (x0 >= 0), (y0 >= 0) & (x0 + 1 <= W - 1), (y0 + 1 <= H - 1) & (x0 >= 0), (y0 + 1 <= H - 1) & (x0 + 1 <= W - 1)]
        first = int(c["starts"][l]) + y0 * W + x0
        d = []
        for valid, off in zip(ok, (0, 1, W, W + 1)):
            idx = np.clip(np.where(valid & gate, first + off, S), 0, S).astype(np.int64)
            d.append((vpad[bi, idx, mi] * go).sum(-1))
        a = attn[..., l, :]
        ga[..., l, :] = np.where(gate, hh * (hw * d[0] + lw * d[1]) + lh * (hw * d[2] + lw * d[3]), 0.0)
        gl[..., l, :, 0] = np.where(gate, a * W * (hh * (d[1] - d[0]) + lh * (d[3] - d[2])), 0.0)
        gl[..., l, :, 1] = np.where(gate, a * H * (hw * (d[2] - d[0]) + lw * (d[3] - d[1])), 0.0)
    return gl, ga


@pytest.mark.parametrize("cid", POW2_CASES)
def test_restatement_with_the_reference_rules_reproduces_the_oracle(cid):
    c = LC.make(cid)
    _, want_loc, want_attn = oracle_backward(cid, np.float64)
    gl, ga = np_backward(c, LC.grad_out_for(c))
    assert float(np.abs(gl - want_loc).max()) <= 1e-10 * max(1.0, float(np.abs(want_loc).max()))
    assert float(np.abs(ga - want_attn).max()) <= 1e-10 * max(1.0, float(np.abs(want_attn).max()))


# variant -> rules, the family that catches it, the least share of its grad_sampling_loc elements beyond 100 x the GPU tolerance.
# Where the shares come from (measured ones are printed by the test; the bounds are what the inputs guarantee):
#   left    every coordinate of `lattice` is an integer; the derivative across the coordinate's own cell boundary jumps for
#           every sample that is gated in, i.e. for most elements
#   trunc   differs from floor only for -1 < px < 0: init_exact's offsets point 1 .. 4 px outward from the border queries,
#           gate_neighbours plants nextafter(-1, 0): a few per cent of the elements
#   >= -1   only samples exactly on -1 with the other coordinate inside: one lattice value in W + 4
#   <= W    likewise on W / H
WRONG = {
    "left_cell_at_an_integer": (dict(cell="left"), "lattice-win", 0.5),
    "truncation_toward_zero": (dict(cell="trunc"), "init_exact-win", 0.01),
    "gate_lower_ge": (dict(lower=">="), "lattice-win", 0.005),
    "gate_upper_le": (dict(upper="<="), "lattice-win", 0.005),
}


@pytest.mark.parametrize("variant", list(WRONG))
def test_each_wrong_rule_is_caught_by_a_wide_margin(variant):
    rules, cid, least = WRONG[variant]
    c = LC.make(cid)
    _, want_loc, want_attn = oracle_backward(cid, np.float32)            # the GPU tests' reference
    gl, ga = np_backward(c, LC.grad_out_for(c), **rules)
    far = 100 * GPU_TOL * max(1.0, float(np.abs(want_loc).max()))
    err = np.abs(gl - want_loc)
    share = float((err > far).mean())
    print("%s on %s: %.4f of grad_sampling_loc beyond 100 x tolerance (worst %.1f x tolerance); grad_attn_weight worst %.1f x" % (
        variant, cid, share, float(err.max()) / (far / 100),
        float(np.abs(ga - want_attn).max()) / (GPU_TOL * max(1.0, float(np.abs(want_attn).max())))))
    assert share >= least


def test_wrong_rules_are_invisible_to_the_masked_comparisons():
    """What the existing tests compare is blind to the rules: with the left cell at an integer, grad_attn_weight stays within the
    tolerance (the forward is continuous) and so does grad_sampling_loc once the samples within 1e-3 px of an integer are left
    out -- which on the lattice family is every sample."""
    c = LC.make("lattice-win")
    _, want_loc, want_attn = oracle_backward("lattice-win", np.float32)
    gl, ga = np_backward(c, LC.grad_out_for(c), cell="left")
    assert float(np.abs(ga - want_attn).max()) <= GPU_TOL * max(1.0, float(np.abs(want_attn).max()))
    pix = c["pix"].astype(np.float64)
    on_edge = (np.abs(pix - np.round(pix)) < 1e-3).any(-1, keepdims=True)
    assert on_edge.all()
    assert float(np.where(on_edge, 0.0, np.abs(gl - want_loc)).max()) == 0.0

"""No GPU: the builders of tests/split_gemm_hard_inputs.py satisfy their own assertions (exact split, accumulator rule, no dropped
term, coverage of every k and column: asserted while a case is built), the float64 emulation of the six-term scheme stays
inside the bound on every case -- the reference alone passes -- and every way of getting the scheme subtly wrong that the GPU
test is meant to catch leaves the bound on the emulation.

Which mutation which `planes` variant catches (plain and cancel form unless noted; `-`: the mutated term is zero there or, in
the plain x2w2 form only, `p`: caught by the plain form, cancelled by construction in the cancel form):

  mutation                         x3    w3    x2w2
  a1w2 removed                     -     yes   p
  a2w1 removed                     yes   -     p
  a2w2 removed                     -     -     yes
  a1w3 removed                     -     yes   -
  a3w1 removed                     yes   -     -
  a2 in place of a3 (x)            yes   -     -
  w2 in place of w3 (w)            -     yes   -
  x planes 1 <-> 2 (loses a1w3)    -     yes   -
  x planes 2 <-> 3 (loses a2w2)    -     -     yes
  w planes 1 <-> 2 (loses a3w1)    yes   -     -
  w planes 2 <-> 3 (loses a2w2)    -     -     yes

(With w in the first plane alone any permutation of x's planes gives the same six products, so a swap inside x shows only against
an operand w with live lower planes, and the other way round.)  The cases in front of a norm (LayerNorm entries, conv1x1 +
GroupNorm, both products of the FFN) are cancel forms and catch their variant's row, piece by probed piece (`x2`, a two-piece x
against a first-plane w, catches a2w1 removed).  `routing` catches: row r taking row r ^ 1, the last ragged row
duplicated, the x_add period off by one."""
import numpy as np
import pytest

import split_gemm_hard_inputs as sg

BOTH, PLAIN = (False, True), (False,)
MUTATIONS = {
    "a1w2 removed": (dict(drop=((0, 1),)), {"w3": BOTH, "x2w2": PLAIN}),
    "a2w1 removed": (dict(drop=((1, 0),)), {"x3": BOTH, "x2w2": PLAIN}),
    "a2w2 removed": (dict(drop=((1, 1),)), {"x2w2": BOTH}),
    "a1w3 removed": (dict(drop=((0, 2),)), {"w3": BOTH}),
    "a3w1 removed": (dict(drop=((2, 0),)), {"x3": BOTH}),
    "a2 in place of a3": (dict(xplanes=(0, 1, 1)), {"x3": BOTH}),
    "w2 in place of w3": (dict(wplanes=(0, 1, 1)), {"w3": BOTH}),
    "x planes 1 <-> 2": (dict(xplanes=(1, 0, 2)), {"w3": BOTH}),
    "x planes 2 <-> 3": (dict(xplanes=(0, 2, 1)), {"x2w2": BOTH}),
    "w planes 1 <-> 2": (dict(wplanes=(1, 0, 2)), {"x3": BOTH}),
    "w planes 2 <-> 3": (dict(wplanes=(0, 2, 1)), {"x2w2": BOTH}),
}


def _planes_cases(variant, cancel, big=False):
    for g in sg.LINEAR_GEOMETRIES + ([sg.BIG_GEOMETRY] if big else []):
        yield "linear %s" % sg.name(g), sg.linear_planes(g, variant, cancel)
    for g in sg.CONV_GEOMETRIES:
        yield "conv %s" % sg.name(g), sg.conv_planes(g, variant, cancel)
    for s, case in enumerate(sg.multi_cases(variant, cancel)):
        yield "multi segment %d" % s, case
    if variant == "x3":
        for g in sg.FPN_GEOMETRIES:
            yield "fpn %s" % sg.name(g), sg.fpn_case(cancel, *g)


def test_split_is_exact_inside_its_domain_and_not_outside():
    rng = np.random.RandomState(0)
    bits = rng.randint(0, 2 ** 32, size=400000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    inside = np.isfinite(x) & (np.abs(x) >= 2.0 ** -110) & ((bits & 0x7FFFFFFF) < 0x7F7F8000)
    a = sg.split3(x[inside])
    assert inside.sum() > 300000
    assert np.array_equal(sum(p.astype(np.float64) for p in a), x[inside].astype(np.float64))
    assert all(np.array_equal(sg.bf16_rne(p), p) for p in a)                       # each piece is a bf16 number
    # the edges of the domain themselves
    edge = np.array([0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F800000], np.uint32).view(np.float32)
    a1, a2, a3 = sg.split3(edge)
    assert np.isfinite(a1[0]) and float(a1[0]) + float(a2[0]) + float(a3[0]) == float(edge[0])
    assert np.isinf(a1[1:]).all() and (a2[1:3] == -np.inf).all() and np.isnan(a3[1:3]).all() and np.isnan(a2[3])
    low = np.float32(2.0 ** -110) * np.float32(1 + 2.0 ** -23)                     # exact: its last bit is 2^-133
    assert sum(float(p[0]) for p in sg.split3(np.array([low]))) == float(low)
    lost = np.float32(2.0 ** -111) * np.float32(1 + 2.0 ** -23)                    # last bit 2^-134: under the last bf16 subnormal
    assert sum(float(p[0]) for p in sg.split3(np.array([lost]))) != float(lost)
    zero = sg.split3(np.array([0.0, -0.0], np.float32))
    assert all(not p.any() for p in zero)


def test_the_relu_of_the_epilogues_is_fmax_but_for_nan():
    """(v > 0 || v != v) ? v : 0 against fmax(v, 0) over every exponent, both signs and a lattice of mantissas"""
    mant = np.array([0, 1, 2, 0x400000, 0x3FFFFF, 0x7FFFFF, 0x555555, 0x2AAAAA, 0x7F8000, 0x000100], np.uint32)
    bits = (np.arange(256, dtype=np.uint32)[:, None, None] << 23) | mant[None, :, None] | (np.array([0, 1], np.uint32) << 31)[None, None, :]
    v = bits.reshape(-1).view(np.float32)
    got = sg.relu_keep_nan(v)
    nan = np.isnan(v)
    assert nan.sum() == 2 * 9 and np.isnan(got[nan]).all()
    assert np.array_equal(got[nan].view(np.uint32), v[nan].view(np.uint32))        # the NaN passes unchanged
    want = np.fmax(v[~nan], np.float32(0))
    assert np.array_equal(got[~nan], want)                                         # as values: -0 == +0
    assert not np.signbit(got[~nan]).any()                                         # and the zero returned is +0, as v_max_f32's


@pytest.mark.parametrize("variant,cancel", sg.PLANES, ids=sg.name)
def test_planes_reference_is_inside_the_bound(variant, cancel):
    for label, case in _planes_cases(variant, cancel, big=True):
        assert sg.ratio(case, sg.emulate(case)) <= 1.0, label
        if cancel:                                               # the output is the probed plane alone: far below one product
            assert np.abs(case.T).max() < 2.0 ** -6 * np.abs(case.x_eff).max() * np.abs(case.w).max() * case.K, label


@pytest.mark.parametrize("name", list(sg.RANGES))
def test_range_reference_is_inside_the_bound(name):
    for g in sg.LINEAR_GEOMETRIES:
        case = sg.linear_range(g, name)
        assert sg.ratio(case, sg.emulate(case)) <= 1.0, g
    for g in sg.CONV_GEOMETRIES:
        case = sg.conv_range(g, name)
        assert sg.ratio(case, sg.emulate(case)) <= 1.0, g
    lo, hi = (2.0 ** -110, 2.0 ** -103) if name == "x_subnormal_pieces" else (2.0 ** -103, 2.0 ** 100)
    for op in (case.x_eff, case.w):
        mag = np.abs(op[op != 0]).astype(np.float64)
        assert mag.min() >= (lo if op is case.x_eff else 2.0 ** -103) and mag.max() < (hi if op is case.x_eff else 2.0 ** 100)
    if name == "x_subnormal_pieces":                             # third pieces under bf16's smallest normal number
        a3 = np.abs(sg.split3(case.x_eff)[2])
        assert (a3[a3 != 0] < 2.0 ** -126).mean() > 0.3 and a3[a3 != 0].min() >= 2.0 ** -133


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_every_mutation_leaves_the_bound(mutation):
    kwargs, matching = MUTATIONS[mutation]
    count = 0
    for variant, forms in matching.items():
        for cancel in forms:
            for label, case in _planes_cases(variant, cancel):
                assert sg.ratio(case, sg.emulate(case, **kwargs)) > 1.0, (mutation, variant, cancel, label)
                count += 1
    assert count >= 17


LN_MUTATIONS = {("x3", (1, 2)): ["a2w1 removed", "a3w1 removed", "a2 in place of a3", "w planes 1 <-> 2"],
                ("w3", (1,)): ["a1w2 removed"],
                ("w3", (2,)): ["a1w3 removed", "w2 in place of w3", "x planes 1 <-> 2"],
                ("x2w2", (1, 2)): ["a2w2 removed", "x planes 2 <-> 3", "w planes 2 <-> 3"]}


@pytest.mark.parametrize("entry", list(sg.LAYER_NORM_GEOMETRIES))
def test_layer_norm_cases_obey_the_norm_rule_and_catch_their_mutations(entry):
    """The cancel forms in front of LayerNorm(128): `check_exact` of norm_hard_inputs.py holds (asserted by the builder), the
    emulation is inside the norm tests' bound and every mutation of the variant's table row leaves it."""
    import norm_hard_inputs as nh
    import torch
    for g in sg.LAYER_NORM_GEOMETRIES[entry]:
        for (variant, probes) in sg.LAYER_NORM_VARIANTS:
            case = sg.layer_norm_case(variant, *g, w_probes=probes)
            assert nh.error_ratio(case, torch.from_numpy(sg.layer_norm_emulate(case))) <= 1.0, (g, variant, probes)
            for m in LN_MUTATIONS[(variant, probes)]:
                got = torch.from_numpy(sg.layer_norm_emulate(case, **MUTATIONS[m][0]))
                assert nh.error_ratio(case, got) > 1.0, (g, variant, probes, m)


NORM_MUTATIONS = {"x3": {(1,): ["a2w1 removed"], (2,): ["a3w1 removed", "a2 in place of a3", "w planes 1 <-> 2"]},
                  "x2": {(1,): ["a2w1 removed"]},
                  "w3": {(1,): ["a1w2 removed"], (2,): ["a1w3 removed", "w2 in place of w3", "x planes 1 <-> 2"]},
                  "x2w2": {(1,): ["a2w2 removed", "x planes 2 <-> 3", "w planes 2 <-> 3"]}}


def _caught(case, emulate, variant, probes):
    import norm_hard_inputs as nh
    import torch
    assert nh.error_ratio(case, torch.from_numpy(emulate(case))) <= 1.0, (variant, probes)
    names = [m for p in probes for m in NORM_MUTATIONS[variant].get((p,), [])]
    assert names
    for m in names:
        assert nh.error_ratio(case, torch.from_numpy(emulate(case, **MUTATIONS[m][0]))) > 1.0, (variant, probes, m)


@pytest.mark.parametrize("geometry", sg.CONV_GEOMETRIES, ids=sg.name)
def test_groupnorm_cases_obey_the_norm_rule_and_catch_their_mutations(geometry):
    """conv1x1 in front of GroupNorm(32, 128): `check_exact` with n = 4 H W holds (asserted by the builder); x3 and w3 probe
    both lower planes in one case (by image, by group)."""
    for (variant, probes) in sg.GROUPNORM_VARIANTS:
        _caught(sg.groupnorm_case(variant, *geometry), sg.groupnorm_emulate, variant, probes if variant != "x2w2" else (1,))


@pytest.mark.parametrize("geometry", sg.FFN_GEOMETRIES, ids=sg.name)
def test_ffn_cases_obey_the_norm_rule_and_catch_their_mutations(geometry):
    """Both products of the fused FFN: the mutation is applied to the probed product (first or second GEMM)."""
    for (which, variant, probes) in sg.FFN_VARIANTS:
        _caught(sg.ffn_case(which, variant, probes, *geometry), sg.ffn_emulate, variant, probes)
    for (which, variant, probes) in sg.FFN_VARIANTS[:4]:           # the range family: first-GEMM cases, rows 2^-40 .. 2^40
        _caught(sg.ffn_case(which, variant, probes, *geometry, ex_set=sg.FFN_RANGE), sg.ffn_emulate, variant, probes)


def test_a_mutation_outside_its_table_row_is_invisible():
    """the `-` entries of the table: e.g. a swap of x's planes cannot show while w lives in its first plane alone"""
    case = sg.linear_planes(sg.LINEAR_GEOMETRIES[4], "x3", False)
    assert sg.ratio(case, sg.emulate(case, xplanes=(1, 0, 2))) <= 1.0            # (a1w1 moves into lo: other roundings, same value)
    assert np.array_equal(sg.emulate(case, drop=((0, 1), (1, 1), (0, 2))), sg.emulate(case))


def _emulated(case, x_eff):
    hi, lo = sg.six_terms(x_eff, case.w)
    got = hi.astype(np.float32) + lo.astype(np.float32)
    return sg.relu_keep_nan(got) if case.relu else got


def _routing_cases():
    for mirror in (False, True):
        for (rows, n, relu, _, period) in sg.LINEAR_GEOMETRIES + [sg.BIG_GEOMETRY]:
            yield sg.routing_case(mirror, rows, n, 128, relu, 0 if mirror else period)
        for (K, H, W) in sg.CONV_GEOMETRIES:
            yield sg.routing_case(mirror, 2 * H * W, 128, K)


def test_routing_reference_is_bit_exact_and_its_mutations_are_not():
    for case in _routing_cases():
        label = (case.mirror, case.rows, case.n, case.K, case.period)
        assert sg.routed_ok(case, _emulated(case, case.x_eff)), label
        rows = case.rows
        swapped = case.x_eff[np.minimum(np.arange(rows) ^ 1, rows - 1)]                # row r takes row r ^ 1
        assert not sg.routed_ok(case, _emulated(case, swapped)), label
        dup = case.x_eff.copy()
        dup[rows - 1] = dup[rows - 2]                                                   # the last ragged row duplicated
        assert not sg.routed_ok(case, _emulated(case, dup)), label
        if case.period:                                                                 # the x_add period off by one
            off = case.x + case.x_add[np.arange(rows) % (case.period - 1)]
            assert not sg.routed_ok(case, _emulated(case, off)), label


def test_containment_builders_and_the_emulation_on_them():
    for g in sg.LINEAR_GEOMETRIES:
        case = sg.linear_range(g, "x_small")
        x, xa, hit = sg.poisoned(case)
        assert 3 <= hit.sum() < case.rows and np.isfinite(x[~hit]).all()
        with np.errstate(invalid="ignore", over="ignore"):
            xe = x if xa is None else x + xa[np.arange(case.rows) % case.period]
            all_bad, others_same = sg.contained(hit, sg.emulate(case), sg.emulate(case, x_eff=xe))
        assert all_bad and others_same, g
    case = sg.fpn_case(False, 5, 33)
    enc, hit = sg.fpn_poisoned(case)
    assert hit.sum() == 9 + 4 + 4 and (~np.isfinite(enc)).sum() == 2           # an inner pixel and two corners; BIG is finite

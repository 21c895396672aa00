"""CPU: the routing rules of tests/callsite_check.py and the coverage of its geometry table.

The rules restate from the geometry alone which entry points, and which kernels behind them, a head forward reaches.
Here they must reproduce the hand-written tables of test_callsite_parity_gpu.py at the four BASELINE configs and the
bench geometry, and GEOMETRIES must put every rule on both of its sides -- the batch-stepped and size-stepped thresholds
with a pair of geometries one image (or one 32-pixel step) apart.  No geometry of the table may be redundant: each one
holds a side, or half of a one-step pair, that no other geometry holds."""
import pytest

import callsite_check as chk
from test_callsite_parity_gpu import CONFIGS, MSDA_FAMILY, _expected

BENCH = (4, 512, 512, 128, 100)                     # bench.py: 4 levels, 512^2, batch 128, 100 queries


def _baseline():
    for name, (depth, H, W, Q, levels, N) in CONFIGS.items():
        yield name, (levels, H, W, N, Q)
    yield "bench", BENCH


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rules_reproduce_the_hand_written_call_counts(precision):
    for name, (levels, H, W, N, Q) in _baseline():
        if name == "bench" and precision == "fp32":
            continue                                    # the bench runs under bf16 autocast only
        assert chk.expected_calls(levels, H, W, N, Q, precision) == _expected(name, precision), name


def test_rules_reproduce_the_hand_written_msda_families():
    for name, (levels, H, W, N, Q) in _baseline():
        assert chk.expected_msda_family(levels, H, W, N) == MSDA_FAMILY[name], name


def test_msda_family_rule_at_its_thresholds():
    # csrc/msda_forward.hip: N*S*M >= 450 000 (3 levels) / 160 000 (4 levels) -> column
    S3 = 40 * 40 + 20 * 20 + 10 * 10                  # 3 levels of a 320^2 image: 2 100 tokens
    n3 = -(-450000 // (S3 * 8))
    assert chk.expected_msda_family(3, 320, 320, n3) == chk.K_COL
    assert chk.expected_msda_family(3, 320, 320, n3 - 1) != chk.K_COL
    assert chk.expected_msda_family(4, 512, 512, 1) == chk.K_COL          # 174 080 >= 160 000
    assert chk.expected_msda_family(4, 384, 384, 1) == chk.K_DPP          # 97 920
    # below the column threshold, the windowed kernel once N * ceil(S / 256) * M >= 3 * 768
    assert chk.expected_msda_family(3, 128, 128, 144) == chk.K_WIN        # S = 336: 144 * 2 * 8 = 2 304, N*S*M 387 072
    assert chk.expected_msda_family(3, 128, 128, 143) == chk.K_DPP


def _rules(g):
    return {r for r, _ in chk.routes(g.levels, g.H, g.W, g.N, g.Q)}


def _side(g, rule):
    sides = {s for r, s in chk.routes(g.levels, g.H, g.W, g.N, g.Q) if r == rule}
    assert len(sides) == 1, (g, rule, sides)
    return sides.pop()


# threshold rules whose two sides must be held by a pair one step apart: the same geometry at batch N and N + 1, or (at
# batch 1) images 32 pixels apart in height
STEPPED = {"msda L=3": "batch", "msda L=4": "batch", "input projections": "batch", "mask projection": ("batch", "height")}


def missing_one_step_pairs(geometries):
    missing = set()
    gs = list(geometries.values())
    for rule, steps in STEPPED.items():
        steps = (steps,) if isinstance(steps, str) else steps
        for step in steps:
            found = False
            for a in gs:
                for b in gs:
                    if rule not in _rules(a) or rule not in _rules(b):
                        continue
                    if step == "batch":
                        adjacent = (a.levels, a.H, a.W) == (b.levels, b.H, b.W) and b.N == a.N + 1
                    else:
                        adjacent = (a.levels, a.W, a.N, b.N) == (b.levels, b.W, 1, 1) and b.H == a.H + 32
                    found |= adjacent and _side(a, rule) != _side(b, rule)
            if not found:
                missing.add((rule, step))
    return missing


def test_every_rule_is_exercised_on_both_sides():
    assert not chk.missing_routes(chk.GEOMETRIES), sorted(chk.missing_routes(chk.GEOMETRIES))


def test_stepped_thresholds_are_held_one_step_apart():
    assert not missing_one_step_pairs(chk.GEOMETRIES), sorted(missing_one_step_pairs(chk.GEOMETRIES))


@pytest.mark.parametrize("name", list(chk.GEOMETRIES))
def test_removing_any_geometry_uncovers_a_rule(name):
    rest = {k: g for k, g in chk.GEOMETRIES.items() if k != name}
    assert chk.missing_routes(rest) or missing_one_step_pairs(rest), "%s exercises nothing the others do not" % name


def test_removing_the_4_level_quad_owner_geometry_fails_coverage():
    rest = {k: g for k, g in chk.GEOMETRIES.items() if k != "l4_384_b1_q100"}
    assert ("msda L=4", "batch") in missing_one_step_pairs(rest)


def test_geometries_are_new_and_well_formed():
    baseline = {key for _, key in _baseline()}
    for name, g in chk.GEOMETRIES.items():
        assert g.key not in baseline, name
        assert g.H % 32 == 0 and g.W % 32 == 0, name
        if g.N > 4:
            assert g.select == [0, -1], name
    assert any(g.N % 2 for g in chk.GEOMETRIES.values())
    assert set(chk.MSDA_THRESHOLD_GEOMETRIES) <= set(chk.GEOMETRIES)
    assert {_side(chk.GEOMETRIES[n], "msda L=%d" % chk.GEOMETRIES[n].levels) for n in chk.MSDA_THRESHOLD_GEOMETRIES} \
        == {"column", "quad-owner"}


def test_mask_head_rule_agrees_with_the_product_predicate():
    """dynamic_mask_head.fused_geometry takes plain integers: compare the restatement with it on every call of every
    geometry (the other predicates need device tensors; the GPU test compares their outcome through the call counts)."""
    from pctrans_amd import dynamic_mask_head as dmh
    for name, g in list(chk.GEOMETRIES.items()) + [(n, chk.Geometry(lv, 50, H, W, N, Q)) for n, (lv, H, W, N, Q)
                                                    in _baseline()]:
        mh, mw = chk.mask_feature_shape(g.levels, g.H, g.W)
        lv = chk.level_shapes(g.levels, g.H, g.W)
        for i, k in enumerate(chk.mask_head_kernels(g.levels, g.H, g.W, 5, "bf16")):
            assert (k == "fused") == dmh.fused_geometry(mh, mw, lv[i % 3]), (name, i)

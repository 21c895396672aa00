"""CPU: the conditions under which tests/test_dmh_exact_gpu.py may demand bits from the dynamic mask head kernels, asserted from
the float64 reference alone (tests/dmh_exact_reference.py):

  * the exact-sum condition of families A1 / A2 at every accumulation of the chain, for every path's rounding points;
  * A1: the hidden roundings change nothing (every intermediate is bf16-exact), the dead and the pass-through query are there;
  * B: the census -- in every output row and column of the upsampled plane and every target row of the mask a wrong
    neighbour index or swapped blend weights change at least one output bit, so an exact comparison cannot be blind there;
  * the caps: at most 1e-3 of a case's mask bits within the weight-rounding band (A), at most 40 % of the upsampled elements
    outside the bit-checked set and at least half of every border row, border column and band-seam row inside it (C);
  * the reference is the same function as the one behind the three dec_dynamic_mask_head_* golden fixtures."""
import numpy as np
import pytest
import torch

import dmh_exact_reference as R

GI = list(range(len(R.GEOMETRIES)))


def test_bf16_helpers_agree_with_torch():
    rng = np.random.RandomState(0)
    x = (rng.standard_normal(20000) * np.exp(rng.uniform(-20, 20, 20000))).astype(np.float32)
    x[:8] = [0.0, 1.0, 255.0, 257.0, 0.00390625, -1.00390625, 1.01171875, -3.0e-5]
    want = torch.from_numpy(x).bfloat16().double().numpy()
    assert np.array_equal(R.bf16(x), want)
    y = x[np.abs(x) > 1e-30].astype(np.float64)
    inside = R.bf16_margin(y) * 0.999                          # moving by less than the margin never changes the rounding
    assert (inside >= 0).all() and R.bf16_margin(0.0) < 0      # zero itself counts as unstable (relu handles its sign)
    assert np.array_equal(R.bf16(y + inside), R.bf16(y)) and np.array_equal(R.bf16(y - inside), R.bf16(y))
    over = R.bf16_margin(y) * 1.001 + R.bf16_ulp(y) * 1e-6                  # ... and moving by more than it does, in one direction
    assert ((R.bf16(y + over) != R.bf16(y)) | (R.bf16(y - over) != R.bf16(y))).all()


def test_x2_index_rule_is_torch_align_corners_false():
    rng = np.random.RandomState(1)
    for H, W in ((1, 1), (5, 1), (9, 6), (8, 16)):
        a = rng.standard_normal((2, 3, H, W))
        want = torch.nn.functional.interpolate(torch.from_numpy(a), size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
        got = R.lin(a, R.bilinear_src(2 * H, H), R.bilinear_src(2 * W, W))
        assert np.abs(got - want.numpy()).max() <= 1e-14


@pytest.mark.parametrize("rel", [True, False])
@pytest.mark.parametrize("family", ["a1", "a2"])
@pytest.mark.parametrize("gi", GI)
def test_exact_families_meet_the_exact_sum_condition_and_the_mask_cap(gi, family, rel):
    N, Q, H, W, target = R.GEOMETRIES[gi]
    for path in R.PATHS:
        o = R.exact_reference(gi, family, rel, path)
        assert o["viol"] == [], (path, o["viol"])
        free = o["mask_free_exact"]
        assert free.mean() <= 1e-3, (path, float(free.mean()))
        if family == "a1" and R.is_half_target(H, W, target):
            assert not free.any()
    lg = R.exact_reference(gi, family, rel, "f32")["logits"]
    if lg[0, 0].size >= 16:
        assert lg.min() < 0 < lg.max()                         # the masks are not constant


@pytest.mark.parametrize("rel", [True, False])
@pytest.mark.parametrize("gi", GI)
def test_a1_is_invariant_under_the_hidden_roundings(gi, rel):
    N, Q, H, W, target = R.GEOMETRIES[gi]
    c = R.exact_case(gi, "a1", rel)
    f32, valu, mfma = (R.exact_reference(gi, "a1", rel, p) for p in R.PATHS)
    for key in ("x0", "x1", "logits", "up_pre", "v"):
        assert np.array_equal(f32[key], mfma[key]) and np.array_equal(f32[key], valu[key]), key
        if key in ("x0", "x1", "logits"):
            assert R.is_bf16(f32[key]), key
    assert np.array_equal(valu["up"], mfma["up"]) and np.array_equal(valu["mask"], mfma["mask"])
    assert R.is_bf16(c["feats"]) and R.is_bf16(c["params"])
    if rel:
        assert not c["params"].reshape(N, Q, -1)[..., :144].reshape(N, Q, 8, 18)[..., :2].any()
    if Q >= 3:
        for n in range(N):
            assert np.array_equal(f32["logits"][n, 1], c["feats"][n, (1 + n) % 16].astype(np.float64))   # one channel unchanged
            dead = f32["logits"][n, 2]
            assert not f32["x0"][n, 2].any() and (dead == dead.flat[0]).all() and dead.flat[0] != 0


@pytest.mark.parametrize("gi", GI)
def test_census_no_row_or_column_is_blind_to_a_wrong_neighbour(gi):
    for rel in (True, False):
        blind = R.census(R.exact_reference(gi, "a1", rel, "mfma")["logits"], R.GEOMETRIES[gi][4])
        assert blind == [], blind[:8]


def test_census_does_see_a_smooth_plane_as_blind():
    """The census itself has teeth: on a plane that is linear in y a wrong vertical neighbour at the interior is invisible
    to the sign-based mask and it says so."""
    lg = np.broadcast_to((np.arange(16.0) + 100.0)[:, None], (1, 1, 16, 8)).copy()
    assert any(b[0].startswith("mask row") for b in R.census(lg, (5, 3)))


@pytest.mark.parametrize("path", ["valu_bf16", "mfma"])
@pytest.mark.parametrize("ci", range(8))
def test_generic_family_caps(ci, path):
    c = R.generic_case(ci)
    N, Q, H, W = c["geometry"]
    o = R.generic_reference(ci, path)
    bits = o["up_bits"]
    assert 1.0 - bits.mean() <= 0.40, float(bits.mean())
    for r in [0, 2 * H - 1] + R.seam_rows(N, Q, H, W, W == 128):
        assert bits[:, :, r, :].mean() >= 0.5, (r, float(bits[:, :, r, :].mean()))
    for x in (0, 2 * W - 1):
        assert bits[:, :, :, x].mean() >= 0.5, (x, float(bits[:, :, :, x].mean()))
    assert o["mask_free"].mean() <= 0.02
    assert (o["up_bound"] > 0).all() and np.isfinite(o["up_bound"]).all()


def test_generic_hard_value_variants_are_what_they_say():
    base = R.generic_case(2)
    assert float(np.abs(R.generic_reference(5, "f32")["logits"]).mean()) > 30 * float(np.abs(R.generic_reference(2, "f32")["logits"]).mean())
    assert {0.0, -0.25, 1.25, 1.0 - 2.0 ** -24} <= set(np.unique(R.generic_case(4)["ref"]).astype(np.float64).tolist())
    x0 = R.generic_reference(6, "f32")["x0"]
    assert not x0[:, ::2].any() and x0[:, 1::2].any()
    assert np.abs(R.generic_case(7)["feats"][:, 3]).mean() > 300 * np.abs(base["feats"][:, 2]).mean()


@pytest.mark.parametrize("tag", ["rel", "norel", "rel_up"])
def test_reference_reproduces_the_golden_fixtures(golden, tag):
    g = golden("dec_dynamic_mask_head_" + tag)
    feats = g["feats"]
    ref = np.ascontiguousarray(np.swapaxes(g["refpts"], 0, 1))
    params = np.ascontiguousarray(np.swapaxes(g["params"], 0, 1))
    rel, stride, tgt, heads = bool(g["rel_coord"]), int(g["stride"]), tuple(int(v) for v in g["target"]), int(g["heads"])
    o = R.forward(feats, ref, params, rel, tgt, "f32", stride=stride)
    scale = max(1.0, float(np.abs(g["logits_x2"]).max()))
    np.testing.assert_allclose(o["up"], g["logits_x2"], rtol=0, atol=1e-4 * scale)
    N, Q = feats.shape[0], ref.shape[1]
    want = g["attn_mask"].reshape(N, heads, Q, -1)[:, 0]
    assert (o["mask"].reshape(N, Q, -1) != want).mean() < 1e-3

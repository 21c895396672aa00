"""CPU: the properties of tests/hard_inputs.py that the GPU tests of csrc/lsap.hip and csrc/attn_common.hpp lean on, stated
on the references alone -- so that no GPU test passes because its input turned out easy after all."""
import math

import numpy as np
import pytest
import torch

import hard_inputs as hi


# ---- LSAP -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hi.LSAP_CASES))
def test_scipy_solves_every_lsap_family(name):
    cost, counts, ref = hi.lsap_case(name)
    Q, gmax = cost.shape[1:]
    assert cost.dtype == np.float32 and gmax == max(counts) and Q <= 1024 and gmax <= 512
    assert len(set(counts)) > 1                                           # ragged: Gmax decides the LDS residency
    for b, g in enumerate(counts):
        rows, total = ref[b]
        assert rows.shape == (g,) and len(set(rows.tolist())) == g and math.isfinite(total)
    if name in hi.LSAP_INTEGER_CASES:
        for b, g in enumerate(counts):
            c = cost[b, :, :g]
            assert (c == np.round(c)).all() and float(np.abs(c).max(initial=0)) * g < 2.0 ** 53    # every total is exact
            assert ref[b][1] == int(ref[b][1])


def test_lsap_families_have_the_structure_they_claim():
    cost, counts = hi.duplicated_queries(21)
    assert cost.shape == (3, 300, 60)
    for j in range(60, 300):
        assert (cost[:, j] == cost[:, j % 60]).all()
    assert len({cost[0, j].tobytes() for j in range(300)}) == 60
    # copies of one row in two lane iterations (j, j + 256 share a lane of the 256-thread block) and in different waves
    assert {(j % 256) // 64 for j in range(0, 300, 60)} == {0, 1, 2, 3} and {j // 256 for j in range(16, 300, 60)} == {0, 1}
    cost, counts = hi.forbidden_pairs(300, 60, 31)
    for b, g in enumerate(counts):
        assert 0.65 < float(np.isinf(cost[b, :, :g]).mean()) < 0.75
    _, _, ref = hi.lsap_case("forbidden_pairs-300x60")
    assert all(math.isfinite(t) for _, t in ref)
    cost, counts = hi.magnitudes(300, 60, 41)
    assert 1e30 < float(np.abs(cost[0]).max()) < 3e38 and 0 < float(np.abs(cost[1, :, :counts[1]]).max()) < 1e-28
    third = cost[2, :, :counts[2]].astype(np.float64)
    assert (third * 16 == np.round(third * 16)).all() and float(third.min()) > 9e5      # fp32 spacing 1/16 at 1e6
    # the long case holds both declared limits and the two trivial problem sizes
    cost, counts = hi.LSAP_CASES["machol_wien-1024x512"]()
    assert cost.shape == (3, 1024, 512) and counts == [512, 0, 1]
    # LDS residency (csrc/lsap.hip keeps the transposed costs in LDS up to 96 KB): both sides are covered
    sizes = {n: hi.lsap_case(n)[0].shape[1] * hi.lsap_case(n)[0].shape[2] * 4 for n in hi.LSAP_CASES}
    assert sizes["machol_wien-300x60"] <= 96 * 1024 < sizes["machol_wien-300x128"]
    assert sizes["duplicated_queries"] <= 96 * 1024 and sizes["forbidden_pairs-300x128"] > 96 * 1024


@pytest.mark.parametrize("Q,G", [(300, 60), (300, 128)])
def test_hall_violation_is_infeasible_through_the_search_only(Q, G):
    cost, counts = hi.hall_violation(Q, G, 51)
    assert counts[0] == counts[1] == G
    assert np.isfinite(cost[1]).any(axis=0).all()                         # no column of +inf: every target has a query
    assert not np.isnan(cost).any() and not np.isneginf(cost).any()
    only = [np.flatnonzero(np.isfinite(cost[1, :, t])) for t in (7, G - 3)]
    assert only[0].size == 1 and np.array_equal(only[0], only[1])
    with pytest.raises(ValueError, match="infeasible"):
        hi.scipy_solve(cost[1:2], counts[1:2])
    with pytest.raises(ValueError, match="infeasible"):
        hi.sap_sweeps(cost[1].astype(np.float64))
    hi.scipy_solve(cost[0:1], counts[0:1])
    hi.scipy_solve(cost[2:3], counts[2:3])


@pytest.mark.parametrize("Q,G", [(300, 60), (300, 128)])
def test_machol_wien_needs_twenty_times_the_sweeps_of_noise(Q, G):
    """Counted with the plain restatement of the shortest-augmenting-path loop, which must reach scipy's totals."""
    sweeps = {}
    for name, (cost, counts) in (("machol_wien", hi.machol_wien(Q, G)), ("noise", hi.noise(Q, G, 5))):
        c = cost[0].astype(np.float64)
        rows, sweeps[name] = hi.sap_sweeps(c)
        want = hi.scipy_solve(cost[:1], counts[:1])[0][1]
        got = float(c[rows, np.arange(G)].sum())
        assert len(set(rows.tolist())) == G
        assert got == want if name == "machol_wien" else abs(got - want) <= 1e-12 * float(np.abs(c[rows, np.arange(G)]).sum())
    print("sweeps %dx%d: machol_wien %d, noise %d" % (Q, G, sweeps["machol_wien"], sweeps["noise"]))
    assert sweeps["noise"] >= G and sweeps["machol_wien"] >= 20 * sweeps["noise"]


@pytest.mark.parametrize("name", ["rank_one_noise-300x60", "duplicated_queries", "duplicated_queries-integer", "matcher_like",
                                  "forbidden_pairs-300x60"])
def test_restatement_reaches_scipys_total(name):
    cost, counts, ref = hi.lsap_case(name)
    for b, g in enumerate(counts):
        c = cost[b, :, :g].astype(np.float64)
        rows, _ = hi.sap_sweeps(c)
        chosen = c[rows, np.arange(g)]
        assert abs(float(chosen.sum()) - ref[b][1]) <= 1e-12 * float(np.abs(chosen).sum())


def test_matcher_like_predictions_are_exact_copies_of_near_perfect_masks():
    outputs, targets = hi.matcher_like()
    pred = outputs["pred_masks"]
    assert pred.shape[1] == 60
    for b, t in enumerate(targets):
        g = t["masks"].shape[0]
        assert torch.equal(pred[b, g:2 * g], pred[b, :g]) and g < 60 // 4
        assert torch.equal(pred[b, :g] > 0, t["masks"] > 0.5)


# ---- attention --------------------------------------------------------------------------------------------------------
CASES = [(f, g) for f in hi.ATTN_FAMILIES for g in hi.ATTN_GEOMETRIES]


def test_geometries_cover_the_sizes_and_routes():
    geo = hi.ATTN_GEOMETRIES
    assert {g[0] for g in geo} == {16, 37, 100} and {g[1] for g in geo} == {25, 50, 64, 100, 256, 374, 1024}
    assert {g[2] for g in geo} == {1, 2} and {g[4] for g in geo} == {16, 32}
    assert {g[3] for g in geo if g[4] == 32 and g[1] % 64 == 0} == {4, 8}                    # cross-attention applies
    assert all(g[3] == 8 for g in geo if g[4] == 16)


@pytest.mark.parametrize("family,geometry", CASES)
def test_operands_are_bf16_and_nan_rows_are_the_fully_masked_ones(family, geometry):
    c = hi.attention_case(family, geometry)
    L, S, N, heads, hd = geometry
    assert c["q"].shape == (L, N, heads * hd) and c["k"].shape == (S, N, heads * hd) and c["v"].shape == (S, N, heads * 16)
    assert all(c[n].dtype == torch.bfloat16 and bool(torch.isfinite(c[n].float()).all()) for n in "qkv")
    dead = torch.zeros(L, N, dtype=torch.bool) if c["mask"] is None else c["mask"].all(-1)[:, 0].t()
    assert torch.equal(torch.isnan(c["want"]).any(-1), dead) and torch.equal(torch.isnan(c["want"]).all(-1), dead)
    assert int(dead.sum()) == (3 if family == "window_masks" else 0)


@pytest.mark.parametrize("geometry", hi.ATTN_GEOMETRIES)
def test_peaked_scores_leave_few_effective_keys(geometry):
    for family in ("peaked", "v_outliers", "underflow"):
        p = hi.attention_case(family, geometry)["p"]
        assert float((1.0 / (p * p).sum(-1)).median()) <= 4.0
    s = hi.attention_case("peaked", geometry)["scores"]
    assert 9.0 < float(s.std()) < 15.0


@pytest.mark.parametrize("geometry", hi.ATTN_GEOMETRIES)
def test_running_maximum_moves_at_every_step_or_never(geometry):
    S = geometry[1]
    for family in ("ascending", "descending"):
        s = hi.attention_case(family, geometry)["scores"]
        d = s[..., 1:] - s[..., :-1]
        assert bool((d > 0).all()) if family == "ascending" else bool((d < 0).all())
        step_max = torch.stack([s[..., k0:k0 + 32].amax(-1) for k0 in range(0, S, 32)], -1)
        run = torch.cummax(step_max, -1).values
        if family == "ascending":       # the maximum changes at every 32-key step: by 1/2 to 16 per full step (1/64 to 1/2
            gain = run[..., 1:] - run[..., :-1]                 # per key), so the rescaling factor is neither 1 nor 0 in fp32
            assert S <= 32 or (bool((gain >= 0.05).all()) and bool((gain <= 16.5).all()))
        else:                           # ... or never after the first key
            assert bool((run == s[..., :1]).all())


@pytest.mark.parametrize("geometry", hi.ATTN_GEOMETRIES)
def test_one_hot_rows_sit_on_their_key_and_the_keys_cover_the_step_layout(geometry):
    L, S, N, heads, hd = geometry
    c = hi.attention_case("one_hot", geometry)
    hot = torch.from_numpy(c["hot"])                                                 # [N, heads, L]
    assert bool((c["p"].gather(-1, hot[..., None]) >= 1 - 1e-12).all())
    rest = c["scores"].clone()
    rest.scatter_(-1, hot[..., None], float("-inf"))
    assert bool((c["scores"].gather(-1, hot[..., None])[..., 0] - rest.amax(-1) >= 60).all())
    used = set(c["hot"].ravel().tolist())
    assert {p % 32 for p in used} == set(range(min(S, 32)))
    assert {0, S - 1} <= used and (S <= 32 or {31, 32, S - 33} <= used)
    assert S % 32 == 0 or any(p >= 32 * (S // 32) for p in used)                     # the ragged tail
    # every row of v is distinguishable, head by head and element by element: a wrong key cannot give the right output
    v = c["v"].float().reshape(S, N, heads, 16)
    want = c["want"].reshape(L, N, heads, 16).permute(1, 2, 0, 3)
    assert torch.equal(want.float(), v.permute(1, 2, 0, 3).gather(2, hot[..., None].expand(-1, -1, -1, 16)))
    for n in range(N):
        for h in range(heads):
            assert len({v[s, n, h].numpy().tobytes() for s in range(S)}) == S


@pytest.mark.parametrize("geometry", hi.ATTN_GEOMETRIES)
def test_window_masks_are_small_and_reach_the_tail_and_dead_leading_steps(geometry):
    L, S, N, heads, hd = geometry
    c = hi.attention_case("window_masks", geometry)
    live = ~c["mask"][:, 0]                                                           # [N, L, S]
    win = c["windows"]
    tail = 32 * (S // 32) if S % 32 else S - 32
    kinds = {"tail": 0, "dead_steps": 0, "first": 0}
    for n in range(N):
        for l in range(L):
            lo, hi_ = win[n, l]
            want = torch.zeros(S, dtype=torch.bool)
            want[lo:hi_] = True
            assert torch.equal(live[n, l], want) and hi_ - lo <= max(1, int(0.05 * S))
            if hi_ > lo:
                kinds["tail"] += lo >= max(tail, 0)
                kinds["dead_steps"] += lo >= (64 if S > 96 else 32)
                kinds["first"] += lo == 0
    assert kinds["tail"] >= 2 and kinds["first"] >= 2 and (S <= 32 or kinds["dead_steps"] >= 2)
    assert sorted(c["dead_rows"]) == sorted((n, l) for n in range(N) for l in range(L) if not live[n, l].any())


@pytest.mark.parametrize("geometry", hi.ATTN_GEOMETRIES)
def test_outliers_sit_on_keys_with_little_probability_and_underflow_underflows(geometry):
    c = hi.attention_case("v_outliers", geometry)
    out = c["outliers"]                                                               # [N, heads, S, 16]
    assert int(out.sum()) > 0 and bool((out.any(-1).sum(-1) <= max(1, geometry[1] // 10)).all())
    mass = (c["p"] * out.any(-1)[:, :, None, :]).sum(-1)
    assert float(mass.max()) < 1e-3 * max(1, geometry[1] // 10) and float(mass.max()) > 0
    # most probabilities are exactly zero in fp32 (exp of less than -104), although every row keeps a key near 1
    s = hi.attention_case("underflow", geometry)["scores"]
    gap = s.amax(-1, keepdim=True) - s
    assert float((gap > 104).double().mean()) > 0.5

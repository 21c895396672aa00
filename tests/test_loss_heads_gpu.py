"""GPU: the head dimension of the point-sampled losses and matcher costs (pct_point_select_uncertain_many_f32,
pct_point_mask_loss_forward_many_f32, pct_point_match_cost_many_f32; pctrans_amd/point_loss.py: *_many; SetCriterion.loss_heads and
Point_HungarianMatcher.cost_heads = "batched").

The single-head kernels have their own float64 tests (test_point_loss_gpu.py, test_point_select_gpu.py, test_match_cost_gpu.py).
What is new is the head dimension, so the main check is bit identity: for every head the *_many entry must write the bits the
single-head entry writes for that head's pointer and that head's slices, NaN rows and zero columns included.  Heads 1, 3, 10, and
17 through the Python grouping (16 + 1); every head its own data and its own index permutation.  One case per entry is also held
to the float64 references inside the bounds those modules derive.

Shapes, the smallest at which the head dimension can go wrong: predictions [2, 5, 33, 20] (ten planes of odd size), targets
[7, 41, 27], K = 6 pairs; 144 candidates keep 36; P = 48 and P = 1030 (more than one point per thread of the 1024 and a ragged
tail); two pairs of 16 385 and 40 961 candidates (the other two kernel classes of the selection); costs for B = 2 images with
3 and 65 targets (a short image, two target groups), Q = 5 and 130 (two query groups), P = 200 (two point passes)."""
import pytest
import torch

import match_cost_reference as M
import point_loss_reference as R
from pctrans_amd import point_loss
from pctrans_amd.loss import maskformer_criterion as crit
from pctrans_amd.loss import matcher as matcher_mod

pytestmark = pytest.mark.gpu

DEV = "cuda"
HEADS = [1, 3, 10, 17]
NPLANES, H, W = 10, 33, 20
NTGT, HT, WT = 7, 41, 27
K = 6
SENTINEL = -7.25


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def data():
    """17 heads of predictions, targets, per-head index permutations (head 1: pair 2 points outside the planes), made once."""
    g = torch.Generator().manual_seed(31)
    preds = [(torch.randn(2, 5, H, W, generator=g) * 3).to(DEV) for _ in range(17)]
    tgt = (torch.rand(NTGT, HT, WT, generator=g) > 0.5).float().to(DEV)
    src = torch.stack([torch.randperm(NPLANES, generator=g)[:K] for _ in range(17)]).int()
    tix = torch.stack([torch.randperm(NTGT, generator=g)[:K] for _ in range(17)]).int()
    src_bad = src.clone()
    src_bad[1, 2] = NPLANES                                                    # one past the last plane
    assert len({tuple(r.tolist()) for r in src}) == 17                          # every head another permutation
    return {"preds": preds, "tgt": tgt, "src": src.to(DEV), "src_bad": src_bad.to(DEV), "tgt_index": tix.to(DEV), "gen": g}


def _select_both(preds, src, cand, keep, extra=3):
    heads, pairs = cand.shape[:2]
    out = torch.full((heads, pairs, keep + extra, 2), SENTINEL, device=DEV)
    got, index = point_loss.select_uncertain_points_many(preds, src, cand, keep, out=out)
    assert got is out and bool((out[:, :, keep:] == SENTINEL).all())           # the rows' tails are the caller's
    for h in range(heads):
        one = torch.full((pairs, keep + extra, 2), SENTINEL, device=DEV)
        _, idx = point_loss.select_uncertain_points(preds[h], None if src is None else src[h], cand[h], keep, out=one)
        assert same_bits(out[h], one) and torch.equal(index[h], idx), h
    return out, index


@pytest.mark.parametrize("heads", HEADS)
def test_selection_is_the_single_head_call_bit_for_bit(data, heads):
    g = torch.Generator().manual_seed(heads)
    cand = torch.rand(heads, K, 144, 2, generator=g).to(DEV)
    src = data["src_bad"][:heads]
    out, index = _select_both(data["preds"][:heads], src, cand, 36)
    if heads > 1:                                                                # the row outside the planes: NaN and -1, alone
        assert bool(out[1, 2, :36].isnan().all()) and bool((index[1, 2] == -1).all())
        assert int(out[:, :, :36].isnan().any(-1).any(-1).sum()) == 1 and int((index < 0).any(-1).sum()) == 1
    else:
        assert bool(out.isfinite().all()) and bool((index >= 0).all())
    # the identity in every head, and no index output
    none, no_index = point_loss.select_uncertain_points_many(data["preds"][:heads], None, cand, 36, with_index=False)
    assert no_index is None
    for h in range(heads):
        assert same_bits(none[h], point_loss.select_uncertain_points(data["preds"][h], None, cand[h], 36)[0])


@pytest.mark.parametrize("S", [16385, 40961])
def test_selection_in_the_other_two_kernel_classes(data, S):
    g = torch.Generator().manual_seed(S)
    cand = torch.rand(3, 2, S, 2, generator=g).to(DEV)
    _select_both(data["preds"][:3], data["src"][:3, :2].contiguous(), cand, S // 4, extra=1)


@pytest.mark.parametrize("P", [48, 1030])
@pytest.mark.parametrize("heads", HEADS)
def test_loss_forward_is_the_single_head_call_bit_for_bit(data, heads, P):
    g = torch.Generator().manual_seed(100 * heads + P)
    coords = torch.rand(heads, K, P, 2, generator=g).to(DEV)
    preds, src, tix = data["preds"][:heads], data["src_bad"][:heads], data["tgt_index"][:heads]
    x, t, sums = point_loss.point_mask_loss_forward_many(preds, src, data["tgt"], tix, coords)
    assert x.shape == (heads, K, P) and t.shape == (heads, K, P) and sums.shape == (heads, K, 4)
    for h in range(heads):
        want = point_loss.point_mask_loss_forward(preds[h], src[h], data["tgt"], tix[h], coords[h])
        assert all(same_bits(a[h], b) for a, b in zip((x, t, sums), want)), h
    nan_rows = x.isnan().all(-1) & t.isnan().all(-1) & sums.isnan().all(-1)
    assert int(nan_rows.sum()) == (1 if heads > 1 else 0) and (heads == 1 or bool(nan_rows[1, 2]))
    assert int(x.isnan().any(-1).sum()) == int(nan_rows.sum())


def _cost_vectors(counts, starts=None):
    starts = [sum(counts[:b]) for b in range(len(counts))] if starts is None else starts
    return torch.tensor(starts, dtype=torch.int32, device=DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("Q", [5, 130])
@pytest.mark.parametrize("heads", HEADS)
def test_costs_are_the_single_head_call_bit_for_bit(heads, Q):
    counts, P = [3, 65], 200
    g = torch.Generator().manual_seed(1000 * heads + Q)
    preds = [(torch.randn(2, Q, 7, 9, generator=g) * 3).to(DEV) for _ in range(heads)]
    tgt = (torch.rand(sum(counts), 14, 18, generator=g) > 0.5).float().to(DEV)
    coords = torch.rand(heads, 2, P, 2, generator=g).to(DEV)
    # the second image's planes as they are, and starting 10 late: its last columns name planes that do not exist
    for starts, nan_from in ((None, None), ([0, 13], 55)):
        s, c = _cost_vectors(counts, starts)
        cost = point_loss.match_costs_many(preds, tgt, s, c, coords, 5.0, 2.0, 65)
        assert cost.shape == (heads, 2, Q, 65)
        for h in range(heads):
            assert same_bits(cost[h], point_loss.match_costs(preds[h], tgt, s, c, coords[h], 5.0, 2.0, 65)), h
        assert bool((cost[:, 0, :, 3:] == 0).all()) and bool(cost[:, 0, :, :3].isfinite().all())     # exactly zero past the count
        if nan_from is None:
            assert bool(cost.isfinite().all()) and bool((cost[:, 1] != 0).all())
        else:
            assert bool(cost[:, 1, :, nan_from:].isnan().all()) and bool(cost[:, 1, :, :nan_from].isfinite().all())
    # planned for 2 images, not for heads * 2: the chunking of the single call (two passes of 128 points: two chunks)
    assert M.plan(2, Q, 65, P) == (128, 2)


def _autograd_case(heads, shape, seed):
    g = torch.Generator().manual_seed(seed)
    n = shape[0] * shape[1]
    preds = [(torch.randn(*shape, generator=g) * 3).to(DEV) for _ in range(heads)]
    tgt = (torch.rand(NTGT, HT, WT, generator=g) > 0.5).float().to(DEV)
    src = torch.stack([torch.randperm(n, generator=g)[:K] for _ in range(heads)]).to(DEV)
    tix = torch.stack([torch.randperm(NTGT, generator=g)[:K] for _ in range(heads)]).to(DEV)
    coords = torch.rand(heads, K, 48, 2, generator=g).to(DEV)
    return preds, tgt, src, tix, coords


@pytest.mark.parametrize("heads,shape", [(10, (2, 5, H, W)), (3, (2, 5, 40, 256))])
def test_losses_and_gradients_against_the_per_head_function(heads, shape):
    """Ten point_mask_losses calls against one point_mask_losses_many: gradients bit for bit for incoming gradients (1, 1) and
    (0.3, 2.0), exact zeros for a head with incoming (0, 0), the loss scalars within 2 K 2^-24 relative (the per-pair terms are
    non-negative, only the order of the final K-term sum differs).  40 x 256: two bands of the backward."""
    preds, tgt, src, tix, coords = _autograd_case(heads, shape, 41 + heads)
    g_m = torch.tensor([1.0, 0.3, 0.0] + [1.0, 0.3] * 4)[:heads].to(DEV)
    g_d = torch.tensor([1.0, 2.0, 0.0] + [1.0, 2.0] * 4)[:heads].to(DEV)
    want = []
    for h in range(heads):
        p = preds[h].clone().requires_grad_(True)
        lm, ld = point_loss.point_mask_losses(p, src[h], tgt, tix[h], coords[h], 6.0)
        (g_m[h] * lm + g_d[h] * ld).backward()
        want.append((lm.detach(), ld.detach(), p.grad))
    runs = []
    for _ in range(2):
        ps = [p.clone().requires_grad_(True) for p in preds]
        lm, ld = point_loss.point_mask_losses_many(ps, src, tgt, tix, coords, 6.0)
        assert lm.shape == (heads,) and ld.shape == (heads,)
        (g_m * lm + g_d * ld).sum().backward()
        runs.append((lm.detach(), ld.detach(), [p.grad for p in ps]))
    lm, ld, grads = runs[0]
    tol = 2 * K * 2.0 ** -24
    for h in range(heads):
        rel_m = abs(float(lm[h]) - float(want[h][0])) / float(want[h][0])
        rel_d = abs(float(ld[h]) - float(want[h][1])) / float(want[h][1])
        print("head %d: loss_mask rel %.3e, loss_dice rel %.3e (bound %.3e)" % (h, rel_m, rel_d, tol))
        assert float(want[h][0]) > 0 and float(want[h][1]) > 0 and rel_m <= tol and rel_d <= tol
        assert same_bits(grads[h], want[h][2]), h
        assert bool((grads[h] != 0).any()) == (h != 2)
    assert heads < 3 or (float(grads[2].abs().max()) == 0.0 and float(want[2][2].abs().max()) == 0.0)
    assert same_bits(lm, runs[1][0]) and same_bits(ld, runs[1][1])             # two calls: the same bits
    assert all(same_bits(a, b) for a, b in zip(grads, runs[1][2]))


def test_a_head_without_gradient_gets_none_and_the_others_theirs():
    preds, tgt, src, tix, coords = _autograd_case(3, (2, 5, H, W), 7)
    ps = [preds[0].clone().requires_grad_(True), preds[1].clone(), preds[2].clone().requires_grad_(True)]
    lm, ld = point_loss.point_mask_losses_many(ps, src, tgt, tix, coords, 6.0)
    (lm + ld).sum().backward()
    assert ps[1].grad is None
    for h in (0, 2):
        p = preds[h].clone().requires_grad_(True)
        a, b = point_loss.point_mask_losses(p, src[h], tgt, tix[h], coords[h], 6.0)
        (a + b).backward()
        assert same_bits(ps[h].grad, p.grad)


# ---- one case per entry against float64 --------------------------------------------------------------------------------------
def test_selection_against_float64(data):
    heads, S, n = 3, 144, 36
    g = torch.Generator().manual_seed(77)
    cand = torch.rand(heads, K, S, 2, generator=g)
    _, index = point_loss.select_uncertain_points_many(data["preds"][:heads], data["src"][:heads], cand.to(DEV), n)
    for h in range(heads):
        planes = data["preds"][h].cpu().flatten(0, 1)
        x64 = R.sample64(planes, data["src"][h].cpu(), cand[h])
        flips = R.flip_candidates(x64, n, R.sample_bound(float(planes.abs().max()), H, W))
        want64 = torch.topk(-x64.abs(), n, dim=1)[1]
        got = index[h].cpu().long()
        assert bool((got[:, 1:] > got[:, :-1]).all())                                       # ascending candidate numbers
        differ = sum(len(set(got[k].tolist()) - set(want64[k].tolist())) for k in range(K))
        print("select many head %d: %d candidates may flip, %d differ from float64" % (h, flips, differ))
        assert differ <= flips <= 0.05 * K * n


def test_loss_forward_against_float64(data):
    heads, P = 3, 1030
    g = torch.Generator().manual_seed(78)
    coords = torch.rand(heads, K, P, 2, generator=g)
    src, tix = data["src"][:heads], data["tgt_index"][:heads]
    x, t, sums = point_loss.point_mask_loss_forward_many(data["preds"][:heads], src, data["tgt"], tix, coords.to(DEV))
    tgt = data["tgt"].cpu()
    for h in range(heads):
        planes = data["preds"][h].cpu().flatten(0, 1)
        x64, t64 = R.sample64(planes, src[h].cpu(), coords[h]), R.sample64(tgt, tix[h].cpu(), coords[h])
        e_x, e_t = R.sample_bound(float(planes.abs().max()), H, W), R.sample_bound(1.0, HT, WT)
        assert float((x[h].cpu().double() - x64).abs().max()) <= e_x and float((t[h].cpu().double() - t64).abs().max()) <= e_t
        err = (sums[h].cpu().double() - R.sums64(x64, t64)).abs()
        tol = R.sums_bound(x64, t64, e_x, e_t)
        print("pct_point_mask_loss_forward_many_f32 head %d: sums error / bound %s" % (h, (err / tol).max(0)[0].tolist()))
        assert bool((err <= tol).all())


def test_costs_against_float64():
    heads, counts, Q, P = 3, [3, 65], 130, 200
    cases = [M.random_case(2, Q, counts, P, seed=60 + h) for h in range(heads)]
    tgt = cases[0][1]
    s, c = _cost_vectors(counts)
    coords = torch.stack([case[2] for case in cases])
    cost = point_loss.match_costs_many([case[0].to(DEV) for case in cases], tgt.to(DEV), s, c, coords.to(DEV), 5.0, 2.0, 65)
    for h in range(heads):
        pred = cases[h][0]
        x64, t64 = M.samples64(pred, tgt, counts, coords[h])
        want = M.cost_from_parts(*M.parts64(x64, t64)[:4], P, 5.0, 2.0, counts)[0]
        bound = M.cost_bound(x64, t64, counts, 5.0, 2.0, *M.sample_errors(pred, tgt))      # B = 2: the plan of the real batch
        err = (cost[h].cpu().double() - want).abs()
        print("pct_point_match_cost_many_f32 head %d: err %.3e, bound %.3e, worst ratio %.3f"
              % (h, float(err.max()), float(bound.max()), float((err / bound.clamp(min=1e-300)).max())))
        assert bool((err <= bound).all())


# ---- whole criterion and matcher ------------------------------------------------------------------------------------------------
def _targets(seed):
    g = torch.Generator().manual_seed(seed)
    return [{"masks": (torch.rand(n, HT, WT, generator=g) > 0.5).float().to(DEV), "labels": torch.ones(n, dtype=torch.long, device=DEV),
             "center_points": torch.rand(n, 2, generator=g).to(DEV)} for n in (2, 3)]


def _ref_points(heads):
    """forward's loops also form loss_refpoints of the later auxiliary heads."""
    return [{"reference_points": torch.full((2, 5, 2), 0.5, device=DEV)} for _ in range(heads - 2)]


def _criterion(num_points=48):
    c = crit.SetCriterion(1, matcher_mod.Point_HungarianMatcher(5.0, 2.0, num_points=num_points), {}, 0.1, ["masks"], num_points,
                          3.0, 0.75)
    c.point_loss = c.point_select = c.matcher.match_cost = "hip"
    return c


def test_criterion_batched_against_each(monkeypatch):
    """final + three auxiliary heads at [2, 5, 33, 20], targets of 2 and 3 instances, the matcher's indices, the same seed: every
    loss within 2 K 2^-24 relative, every prediction's gradient bit for bit, the generator where the per-head path leaves it."""
    targets = _targets(5)
    g = torch.Generator().manual_seed(6)
    base = [(torch.randn(2, 5, H, W, generator=g) * 3).to(DEV) for _ in range(4)]
    torch.manual_seed(1)
    indices = _criterion().matcher.forward_many([{"pred_masks": p} for p in base], targets)
    pairs = sum(len(s) for s, _ in indices[0])
    assert pairs == 5
    got, calls = {}, []
    many = point_loss.point_mask_losses_many
    monkeypatch.setattr(point_loss, "point_mask_losses_many", lambda *a, **k: calls.append(1) or many(*a, **k))
    for mode in ("each", "batched"):
        preds = [p.clone().requires_grad_(True) for p in base]
        outputs = {"pred_masks": preds[3], "aux_outputs": [{"pred_masks": p} for p in preds[:3]], "indices_list": indices,
                   "aux_reference_points": _ref_points(4)}
        c = _criterion()
        c.loss_heads = mode
        torch.manual_seed(2)
        losses = c(outputs, targets)
        names = sorted(["loss_mask", "loss_dice"] + ["%s_%d" % (n, i) for n in ("loss_mask", "loss_dice") for i in range(3)])
        assert set(losses) >= set(names)
        sum((1 + 0.5 * i) * losses[k] for i, k in enumerate(names)).backward()
        got[mode] = ({k: float(losses[k].detach()) for k in names}, [p.grad for p in preds], torch.cuda.get_rng_state())
    assert calls == [1]                                                         # the batched path ran, once, in its mode only
    tol = 2 * pairs * 2.0 ** -24
    for k, v in got["each"][0].items():
        print("%s: each %.9g batched %.9g" % (k, v, got["batched"][0][k]))
        assert v > 0 and abs(got["batched"][0][k] - v) <= tol * v, k
    assert all(same_bits(a, b) and bool((a != 0).any()) for a, b in zip(got["each"][1], got["batched"][1]))
    assert torch.equal(got["each"][2], got["batched"][2])


@pytest.mark.parametrize("variant", ["one head bfloat16", "one head with fewer pairs"])
def test_criterion_batched_falls_back_head_by_head(monkeypatch, variant):
    """A head of another dtype (under autocast), or with another number of matched pairs: nothing batched, no random number
    drawn ahead, the per-head result."""
    for name in ("point_mask_losses_many", "draw_head_coords"):
        monkeypatch.setattr(point_loss, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("batched")))
    targets = _targets(5)
    g = torch.Generator().manual_seed(8)
    base = [(torch.randn(2, 5, H, W, generator=g) * 3).to(DEV) for _ in range(3)]
    full = [(torch.tensor([1, 3]), torch.tensor([0, 1])), (torch.tensor([4, 0, 2]), torch.tensor([2, 0, 1]))]
    indices = [full, full, full]
    if variant == "one head bfloat16":
        base[1] = base[1].bfloat16()
    else:
        indices[1] = [full[0], (torch.tensor([4, 2]), torch.tensor([2, 1]))]
    got = {}
    for mode in ("each", "batched"):
        outputs = {"pred_masks": base[2], "aux_outputs": [{"pred_masks": p} for p in base[:2]], "indices_list": indices,
                   "aux_reference_points": _ref_points(3)}
        c = _criterion()
        c.loss_heads = mode
        torch.manual_seed(2)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=variant == "one head bfloat16"):
            losses = c(outputs, targets)
        got[mode] = ({k: v.detach() for k, v in losses.items()}, torch.cuda.get_rng_state())
    assert all(torch.equal(v, got["batched"][0][k]) for k, v in got["each"][0].items())
    assert torch.equal(got["each"][1], got["batched"][1])


def test_forward_many_batched_against_each(monkeypatch):
    targets = _targets(9)
    g = torch.Generator().manual_seed(10)
    outs = [{"pred_masks": (torch.randn(2, 5, H, W, generator=g) * 3).to(DEV)} for _ in range(4)]
    got, calls = {}, []
    many = point_loss.match_costs_many
    monkeypatch.setattr(point_loss, "match_costs_many", lambda *a, **k: calls.append(1) or many(*a, **k))
    for mode in ("each", "batched"):
        m = matcher_mod.Point_HungarianMatcher(5.0, 2.0, num_points=200)
        m.match_cost, m.cost_heads = "hip", mode
        seen = []
        assign = m._assign_padded
        monkeypatch.setattr(m, "_assign_padded", lambda padded, counts: seen.append((padded.clone(), list(counts))) or assign(padded, counts))
        torch.manual_seed(3)
        result = m.forward_many(outs, targets)
        m.check()
        got[mode] = (seen, result, torch.cuda.get_rng_state())
    assert calls == [1]
    (cost_e, counts_e), (cost_b, counts_b) = got["each"][0][0], got["batched"][0][0]
    assert len(got["each"][0]) == len(got["batched"][0]) == 1 and counts_e == counts_b == [2, 3] * 4
    assert same_bits(cost_e, cost_b) and cost_b.shape == (8, 5, 3)
    for a, b in zip(got["each"][1], got["batched"][1]):
        assert len(a) == len(b) == 2 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    assert torch.equal(got["each"][2], got["batched"][2])

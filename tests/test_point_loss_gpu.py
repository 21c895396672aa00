"""GPU: the point-sampled mask losses on the device (pct_point_sample_f32, pct_point_mask_loss_forward_f32,
pct_point_mask_loss_backward_f32; pctrans_amd/point_loss.py) against the float64 reference of point_loss_reference.py evaluated
on the same fp32 inputs.  Every bound is derived there from the kernel's arithmetic (sample: the rounding of c W - 0.5 and four
fp32 products; sums: P fp32 additions; backward: plus the header's fixed-point quantum), none is tuned to an observed error.

Shapes are the smallest that take every path: K = 3 of 8 planes through a non-identity index, P = 70 (no multiple of 64),
planes of 5 x 7 (one partial band) and (2 BAND_ROWS + 3) x 24 (three bands, the last partial), targets at another resolution;
and one pixel receiving all of P = 37 632 points."""
import math

import pytest
import torch

import point_loss_reference as R
from pctrans_amd import point_loss
from pctrans_amd.loss import maskformer_criterion as crit
from pctrans_amd.loss import matcher as matcher_mod
from pctrans_amd.loss import point_features

pytestmark = pytest.mark.gpu

BR = point_loss.BAND_ROWS
GEOMS = [((5, 7), (9, 11)), ((2 * BR + 3, 24), (30, 50))]
INDEX = [6, 1, 4]
DEV = "cuda"


def hard_coords(K, P, H, W, seed):
    """Uniform points with the special ones in front: exactly 0, the largest fp32 below 1, pixel centres (weights 0 and 1),
    and rows whose two taps straddle each band boundary."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(K, P, 2, generator=g)
    below1 = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    special = [(0.0, 0.0), (below1, below1), (0.0, below1), (below1, 0.0), (0.5 / W, 0.5 / H), ((W - 0.5) / W, (H - 0.5) / H),
               (1.5 / W, 2.5 / H)]
    for b in range(BR, H, BR):                       # y = c H - 0.5 between rows b - 1 and b, and exactly on each of them
        special += [(0.37, (b + 0.2) / H), (0.61, (b - 0.5) / H), (0.12, (b + 0.5) / H)]
    assert len(special) < P
    for k in range(K):
        c[k, :len(special)] = torch.tensor(special)[torch.arange(len(special)).roll(k)]
    return c


def planes_with_extremes(n, H, W, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, H, W, generator=g) * scale
    p[INDEX[0], : H // 2] = 80.0                     # logits of +-80: exp(-|x|) underflows towards 0, exp(|x|) would overflow
    p[INDEX[1], :, : W // 2] = -80.0
    return p


@pytest.mark.parametrize("geom", GEOMS)
def test_gather_against_float64(geom):
    (H, W), _ = geom
    planes = planes_with_extremes(8, H, W, 1)
    coords = hard_coords(3, 70, H, W, 2)
    idx = torch.tensor(INDEX)
    got = point_loss.point_sample_planes(planes.to(DEV), idx.to(DEV), coords.to(DEV), 1)
    want = R.sample64(planes, idx, coords)
    tol = R.sample_bound(float(planes.abs().max()), H, W)
    err = float((got.cpu().double() - want).abs().max())
    print("pct_point_sample_f32 %dx%d: max error %.3e, bound %.3e" % (H, W, err, tol))
    assert got.shape == (3, 70) and err <= tol
    # one coordinate row for four planes each (the matcher's use), identity index
    rows = coords[:2]
    got4 = point_loss.point_sample_planes(planes.to(DEV).view(2, 4, H, W), None, rows.to(DEV), 4)
    assert float((got4.cpu().double() - R.sample64(planes, None, rows, 4)).abs().max()) <= tol
    again = point_loss.point_sample_planes(planes.to(DEV), idx.to(DEV), coords.to(DEV), 1)
    assert torch.equal(got, again)
    # an index outside the planes: NaN for that row, the others untouched
    bad = point_loss.point_sample_planes(planes.to(DEV), torch.tensor([6, 8, -1]).to(DEV), coords.to(DEV), 1)
    assert torch.equal(bad[0], got[0]) and bool(bad[1:].isnan().all())


@pytest.mark.parametrize("geom", GEOMS)
def test_loss_forward_against_float64(geom):
    (H, W), (Ht, Wt) = geom
    pred = planes_with_extremes(8, H, W, 3)
    g = torch.Generator().manual_seed(4)
    tgt = (torch.rand(5, Ht, Wt, generator=g) > 0.5).float()
    tidx = torch.tensor([4, 0, 2])
    coords = hard_coords(3, 70, H, W, 5)
    x, t, sums = point_loss.point_mask_loss_forward(pred.to(DEV), torch.tensor(INDEX).to(DEV), tgt.to(DEV), tidx.to(DEV),
                                                    coords.to(DEV))
    x64, t64 = R.sample64(pred, INDEX, coords), R.sample64(tgt, tidx, coords)
    e_x, e_t = R.sample_bound(float(pred.abs().max()), H, W), R.sample_bound(1.0, Ht, Wt)
    assert float(x64.abs().max()) > 79.0                                         # the +-80 planes are sampled
    assert float((x.cpu().double() - x64).abs().max()) <= e_x and float((t.cpu().double() - t64).abs().max()) <= e_t
    err = (sums.cpu().double() - R.sums64(x64, t64)).abs()
    tol = R.sums_bound(x64, t64, e_x, e_t)
    print("pct_point_mask_loss_forward_f32 %dx%d: sums error / bound %s" % (H, W, (err / tol).max(0)[0].tolist()))
    assert bool(torch.isfinite(sums).all()) and bool((err <= tol).all())
    again = point_loss.point_mask_loss_forward(pred.to(DEV), torch.tensor(INDEX).to(DEV), tgt.to(DEV), tidx.to(DEV),
                                               coords.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip((x, t, sums), again))


COEFFS = {"generic": ([0.3, -0.02, 1e-3], [0.7, 0.4, -2e-4], [0.11, -0.9, 5e-4]),
          "gamma = 0": ([0.3, -0.02, 1e-3], [0.7, 0.4, -2e-4], [0.0, 0.0, 0.0]),
          "alpha = 0": ([0.0, 0.0, 0.0], [0.7, 0.4, -2e-4], [0.11, -0.9, 5e-4]),
          "all zero, tiny, huge": ([0.0, 1e-30, 3e20], [0.0, -1e-32, 1e19], [0.0, 1e-31, -2e20])}


def _backward_case(K, P, H, W, coords, coef, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(K, P, generator=g) * 4
    x[:, 1::9] = 80.0
    x[:, 2::9] = -80.0
    t = torch.rand(K, P, generator=g)
    t[:, ::5] = (t[:, ::5] > 0.5).float()
    a, b, c = (torch.tensor(v[:K], dtype=torch.float32) for v in coef)
    args = [v.to(DEV) for v in (x, t, coords, a, b, c)]
    got = point_loss.point_mask_loss_backward(*args, H, W)
    again = point_loss.point_mask_loss_backward(*args, H, W)
    want, count = R.scatter64(R.grad_x_closed_form(x, t, a, b, c), coords, H, W)
    tol = R.grad_planes_bound(count, a, b, c, H, W)
    err = (got.cpu().double() - want).abs()
    worst = float((err / tol.clamp(min=1e-300)).max())
    print("pct_point_mask_loss_backward_f32 K=%d P=%d %dx%d: max error %.3e, error / bound %.3f" % (K, P, H, W, float(err.max()), worst))
    assert got.shape == (K, H, W) and bool(torch.isfinite(got).all())
    assert bool((err <= tol).all())
    assert torch.equal(got, again)                   # determinism: the same bits from call to call
    return got, want


@pytest.mark.parametrize("name", list(COEFFS))
@pytest.mark.parametrize("geom", GEOMS)
def test_loss_backward_against_float64(geom, name):
    (H, W), _ = geom
    got, want = _backward_case(3, 70, H, W, hard_coords(3, 70, H, W, 6), COEFFS[name], 7)
    if name != "all zero, tiny, huge":
        assert float(want.abs().max()) > 0.01        # the case has a gradient to get wrong
    else:
        assert float(got[0].abs().max()) == 0.0


@pytest.mark.parametrize("P", [70, 37632])
def test_every_point_on_one_pixel_does_not_overflow(P):
    """All P contributions land on the same four accumulators; x = -80 and t = 1 make every one of them the largest the bound
    allows (sigma - t = -1), all of one sign."""
    H, W = 5, 7
    coords = torch.tensor([0.52, 0.47]).expand(1, P, 2).contiguous()
    coef = ([0.9], [0.3], [-0.2])
    got, want = _backward_case(1, P, H, W, coords, coef, 8)
    x = torch.full((1, P), -80.0)
    t = torch.ones(1, P)
    a, b, c = (torch.tensor(v) for v in coef)
    big = point_loss.point_mask_loss_backward(x.to(DEV), t.to(DEV), coords.to(DEV), a.to(DEV), b.to(DEV), c.to(DEV), H, W)
    want, count = R.scatter64(R.grad_x_closed_form(x, t, a, b, c), coords, H, W)
    assert abs(float(want.sum()) + 0.9 * P) <= 1e-6 * P
    assert bool(((big.cpu().double() - want).abs() <= R.grad_planes_bound(count, a, b, c, H, W)).all())


def test_band_boundaries_receive_both_sides():
    """A point between the last row of a band and the first of the next writes to both workgroups' bands."""
    H, W = 2 * BR + 3, 24
    coords = torch.tensor([[[0.5, (BR + 0.25) / H], [0.25, (2 * BR + 0.4) / H]]])
    x, t = torch.tensor([[0.3, -1.2]]), torch.tensor([[1.0, 0.0]])
    a, b, c = torch.tensor([1.0]), torch.tensor([0.5]), torch.tensor([0.25])
    got = point_loss.point_mask_loss_backward(*(v.to(DEV) for v in (x, t, coords, a, b, c)), H, W).cpu().double()
    want, count = R.scatter64(R.grad_x_closed_form(x, t, a, b, c), coords, H, W)
    rows = want[0].abs().sum(1).nonzero().flatten().tolist()
    assert rows == [BR - 1, BR, 2 * BR - 1, 2 * BR]
    assert bool(((got - want).abs() <= R.grad_planes_bound(count, a, b, c, H, W)).all())
    assert bool((got[0].abs().sum(1) > 0)[rows].all())


def test_empty_calls():
    pred = torch.randn(2, 4, 5, 7, device=DEV, requires_grad=True)
    tgt = torch.ones(3, 9, 11, device=DEV)
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    assert point_loss.point_sample_planes(pred.detach(), none, torch.zeros(0, 70, 2, device=DEV)).shape == (0, 70)
    x, t, sums = point_loss.point_mask_loss_forward(pred.detach(), none, tgt, none, torch.zeros(0, 70, 2, device=DEV))
    assert x.shape == (0, 70) and sums.shape == (0, 4)
    assert point_loss.point_mask_loss_backward(x, t, torch.zeros(0, 70, 2, device=DEV), *[torch.zeros(0, device=DEV)] * 3, 5, 7).shape == (0, 5, 7)
    lm, ld = point_loss.point_mask_losses(pred, none, tgt, none, torch.zeros(0, 70, 2, device=DEV), 1.0)
    (lm + ld).backward()
    assert float(lm) == 0.0 and float(ld) == 0.0 and float(pred.grad.abs().max()) == 0.0


# ---- module level ------------------------------------------------------------------------------------------------------------
def _flat_indices(indices, Q, starts):
    src = torch.cat([s + b * Q for b, (s, _) in enumerate(indices)])
    tgt = torch.cat([t + starts[b] for b, (_, t) in enumerate(indices)])
    return src, tgt


def _loss_bounds(pred, src, planes, tgt, coords, num_masks, H, W, Ht, Wt):
    """Bounds on loss_mask, loss_dice and each gradient pixel from the bounds of the pieces."""
    P = coords.shape[1]
    x64, t64 = R.sample64(pred.flatten(0, 1), src, coords), R.sample64(planes, tgt, coords)
    e_x, e_t = R.sample_bound(float(pred.abs().max()), H, W), R.sample_bound(float(planes.abs().max()), Ht, Wt)
    s64, sb = R.sums64(x64, t64), R.sums_bound(x64, t64, e_x, e_t)
    num, den = 2 * s64[:, 1] + 1, s64[:, 2] + s64[:, 3] + 1
    d_num, d_den = 2 * sb[:, 1], sb[:, 2] + sb[:, 3]
    K = len(src)
    # K terms summed and two divisions in fp32: (K + 4) u of the magnitudes
    tol_mask = float(sb[:, 0].sum()) / P / num_masks + (K + 4) * R.U * float(s64[:, 0].sum()) / P / num_masks
    d_ratio = d_num / den + num * d_den / den ** 2
    tol_dice = float(d_ratio.sum()) / num_masks + (K + 8) * R.U * float((1 + num / den).sum()) / num_masks
    a, b, c = R.coefficients64(s64, P, num_masks)
    # the coefficients the kernel gets are fp32 functions of the fp32 sums: relative error of beta, gamma
    rel = d_num / num + 2 * d_den / den + 8 * R.U
    bound = a.abs() + (b.abs() + c.abs()) / 4
    _, count = R.scatter64(torch.zeros_like(x64), coords, H, W)
    # grad_x moves with x (|d sigma| <= 1/4, |d sigma'| <= 1/10: at most bound_k e_x), with t ((|alpha| + |gamma| / 4) e_t)
    tol_grad = R.grad_planes_bound(count, a, b, c, H, W) + count * (bound * (e_x + e_t + rel))[:, None, None]
    return tol_mask, tol_dice, tol_grad


def test_point_mask_losses_against_float64_fixed_coordinates():
    pred, targets, indices = R.module_case()
    planes = torch.cat([t["masks"] for t in targets])
    src, tgt = _flat_indices(indices, 6, [0, 3])
    coords = hard_coords(6, 70, 40, 24, 9)
    p = pred.to(DEV).requires_grad_(True)
    lm, ld = point_loss.point_mask_losses(p, src.to(DEV), planes.to(DEV), tgt.to(DEV), coords.to(DEV), 6.0)
    (2.0 * lm + 0.5 * ld).backward()
    wm, wd, grad = R.losses64(pred, src, planes, tgt, coords, 6.0)
    tol_mask, tol_dice, tol_grad = _loss_bounds(pred, src, planes, tgt, coords, 6.0, 40, 24, 80, 48)
    print("point_mask_losses: loss_mask error %.3e (bound %.3e), loss_dice error %.3e (bound %.3e)"
          % (abs(float(lm) - float(wm)), tol_mask, abs(float(ld) - float(wd)), tol_dice))
    assert abs(float(lm) - float(wm)) <= tol_mask and abs(float(ld) - float(wd)) <= tol_dice
    got = p.grad.cpu().double().flatten(0, 1)
    want = grad(2.0, 0.5).flatten(0, 1)
    assert bool(((got[src] - want[src]).abs() <= 2.0 * tol_grad).all())           # |g_m|, |g_d| <= 2 scale every term
    unmatched = torch.ones(12, dtype=torch.bool)
    unmatched[src] = False
    assert float(got[unmatched].abs().max()) == 0.0 and float(want[unmatched].abs().max()) == 0.0


def _criterion(mode):
    c = crit.SetCriterion(1, matcher_mod.Point_HungarianMatcher(num_points=70), {}, 0.1, ["masks"], 70, 3.0, 0.75)
    c.point_loss = c.matcher.point_sample = mode
    return c


def test_loss_masks_hip_against_torch_same_seed(monkeypatch):
    pred, targets, indices = R.module_case(device=DEV)
    planes = torch.cat([t["masks"] for t in targets]).cpu()
    src, tgt = _flat_indices(indices, 6, [0, 3])
    drawn = {}
    real_losses, real_sample, real_gather = point_loss.point_mask_losses, point_features.point_sample, point_loss.point_sample_planes
    monkeypatch.setattr(point_loss, "point_mask_losses", lambda *a: drawn.__setitem__("hip", a[4]) or real_losses(*a))
    monkeypatch.setattr(point_loss, "point_sample_planes", lambda *a: drawn.__setitem__("candidates", a[2]) or real_gather(*a))
    monkeypatch.setattr(crit, "point_sample", lambda i, pc, **kw: drawn.__setitem__("torch", pc) or real_sample(i, pc, **kw))
    out = {}
    for mode in ("torch", "hip"):
        p = pred.clone().requires_grad_(True)
        torch.manual_seed(11)
        losses = _criterion(mode).loss_masks({"pred_masks": p}, targets, indices, 6.0)
        (losses["loss_mask"] + losses["loss_dice"]).backward()
        out[mode] = (float(losses["loss_mask"]), float(losses["loss_dice"]), p.grad.cpu().double())
    assert set(drawn) == {"hip", "torch", "candidates"} and drawn["hip"].shape == drawn["torch"].shape == (6, 70, 2)
    # the selected coordinates: equal as sets per pair, except for candidates that the sample bound allows to flip
    nu = int(0.75 * 70)
    e_s = R.sample_bound(float(pred.abs().max()), 40, 24)
    flips = R.flip_candidates(R.sample64(pred.cpu().flatten(0, 1), src, drawn["candidates"]), nu, e_s)
    assert flips <= 0.01 * 6 * nu, flips
    differ = 0
    for k in range(6):
        a = {tuple(r) for r in drawn["hip"][k, :nu].cpu().tolist()}
        b = {tuple(r) for r in drawn["torch"][k, :nu].cpu().tolist()}
        differ += len(a - b)
    print("loss_masks: %d candidates may flip, %d selected coordinates differ" % (flips, differ))
    assert differ <= flips
    assert torch.equal(drawn["hip"][:, nu:], drawn["torch"][:, nu:])             # the fresh uniform points: the same draws
    # the hip path against float64 on the coordinates it drew
    coords = drawn["hip"].cpu()
    wm, wd, grad = R.losses64(pred.cpu(), src, planes, tgt, coords, 6.0)
    tol_mask, tol_dice, tol_grad = _loss_bounds(pred.cpu(), src, planes, tgt, coords, 6.0, 40, 24, 80, 48)
    assert abs(out["hip"][0] - float(wm)) <= tol_mask and abs(out["hip"][1] - float(wd)) <= tol_dice
    assert bool(((out["hip"][2].flatten(0, 1)[src] - grad(1.0, 1.0).flatten(0, 1)[src]).abs() <= tol_grad).all())


def test_matcher_hip_against_torch_and_scipy():
    from scipy.optimize import linear_sum_assignment
    pred, targets, _ = R.module_case(device=DEV)
    P, Q, G = 70, 6, 3
    costs, matches = {}, {}
    for mode in ("torch", "hip"):
        m = _criterion(mode).matcher
        torch.manual_seed(13)
        costs[mode] = m._batched_costs({"pred_masks": pred}, targets)[0].cpu().double()
        torch.manual_seed(13)
        matches[mode] = m({"pred_masks": pred}, targets)
        m.check()
    torch.manual_seed(13)
    coords = torch.cat([torch.rand(1, P, 2, device=DEV) for _ in range(2)]).cpu()
    x = R.sample64(pred.cpu().flatten(0, 1), None, coords, Q).view(2, Q, P)
    t = R.sample64(torch.cat([tt["masks"] for tt in targets]).cpu(), None, coords, G).view(2, G, P)
    want = torch.stack([matcher_mod.batch_sigmoid_ce_loss(x[b], t[b]) + matcher_mod.batch_dice_loss(x[b], t[b]) for b in range(2)])
    # the bound: BCE terms are 1-Lipschitz in x and |x|-Lipschitz in t, summed over P points in fp32 and divided by P;
    # dice = 1 - (2 A + 1) / (B + C + 1) with A, B, C sums of P terms within e_x / 4 + e_t of theirs
    xmax = float(pred.abs().max())
    e_x, e_t = R.sample_bound(xmax, 40, 24), R.sample_bound(1.0, 80, 48)
    tol_ce = e_x + e_t * xmax + (2 * P + 16) * R.U * (xmax + 1)                  # two contractions of P terms each
    d_sum = P * (e_x / 4 + e_t + (P + 8) * R.U)
    s = x.sigmoid()
    num = 2 * torch.einsum("bnc,bmc->bnm", s, t) + 1
    den = s.sum(-1)[:, :, None] + t.sum(-1)[:, None, :] + 1
    tol = tol_ce + 2 * d_sum / den + num * 2 * d_sum / den ** 2 + 8 * R.U
    for mode in ("torch", "hip"):
        err = (costs[mode] - want).abs()
        print("matcher costs (%s): error / bound %.3f" % (mode, float((err / tol).max())))
    assert bool(((costs["hip"] - want).abs() <= tol).all())
    for b in range(2):
        ri, ci = linear_sum_assignment(want[b].numpy())
        best = math.fsum(want[b].numpy()[ri, ci])
        i, j = (v.cpu().numpy() for v in matches["hip"][b])
        assert sorted(j.tolist()) == list(range(G)) and len(set(i.tolist())) == G
        assert math.fsum(want[b].numpy()[i, j]) == best
        assert torch.equal(matches["hip"][b][0], matches["torch"][b][0]) and torch.equal(matches["hip"][b][1], matches["torch"][b][1])

"""GPU: the matcher's cost matrices on the device (pct_point_match_cost_f32; pctrans_amd/point_loss.py: match_costs,
Point_HungarianMatcher.match_cost = "hip").

The reference and every bound are in match_cost_reference.py: float64 from sample64 and the matcher's formulas; the bounds come
from the kernel's chain lengths, not from what it returns.  Two comparisons: the contraction alone (float64 on the fp32 samples
the gather returns for the same inputs -- the kernel samples with the gather's code) within the summation bound, and end to end
within that plus the gather's sampling bound.  The torch fp32 chain's own error is printed beside the kernel's.

Shapes: 1, 5, 31, 32, 33, 100 and 1024 queries (one lane, a partial tile, tiles of 32 and one more, a partial group of 128, every
group); counts (3, 0), (1, 37, 33), (64, 65), (512,) (an empty image, one target, a second tile, a second group of 64, every
group); P = 1, 2, 63 .. 65, 127 .. 129 (one pass of 128 points and one more), 777 (seven chunks of one pass) and 12 544 (25 chunks
of four passes, the last one short); 7 x 9 and 32 x 32 predictions, 14 x 18 and 1 x 1 targets."""
import ctypes

import pytest
import torch
from scipy.optimize import linear_sum_assignment

import match_cost_reference as M
from pctrans_amd import _lib, point_loss
from pctrans_amd.loss import matcher as matcher_mod
from pctrans_amd.loss.point_features import point_sample

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.25
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (5.0, 2.0)]           # ce alone (the relative bound), dice alone, a mix


def _vectors(counts):
    starts = [sum(counts[:b]) for b in range(len(counts))]
    return torch.tensor(starts, dtype=torch.int32, device=DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)


def run(pred, tgt, counts, coords, cm, cd):
    starts, cnt = _vectors(counts)
    return point_loss.match_costs(pred.to(DEV), tgt.to(DEV), starts, cnt, coords.to(DEV), cm, cd, max(counts)).cpu().double()


def gathered(pred, tgt, counts, coords):
    """The gather's own fp32 samples x [B, Q, P], t [B, Gmax, P] (zero rows past a count)."""
    B, Q = pred.shape[:2]
    c = coords.to(DEV)
    x = point_loss.point_sample_planes(pred.to(DEV), None, c, Q).view(B, Q, -1).cpu()
    t = torch.zeros(B, max(counts), coords.shape[1])
    at = 0
    for b, g in enumerate(counts):
        if g:
            t[b, :g] = point_loss.point_sample_planes(tgt[at:at + g].to(DEV), None, c[b:b + 1], g).cpu()
        at += g
    return x, t


def torch_chain(pred, tgt, counts, coords, cm, cd):
    """Today's fp32 chain on the device: point_sample, then the matcher's two loss functions per image."""
    B, Q = pred.shape[:2]
    out = torch.zeros(B, Q, max(counts), dtype=torch.float64)
    at = 0
    for b, g in enumerate(counts):
        if g:
            c = coords[b:b + 1].to(DEV)
            x = point_sample(pred[b][:, None].to(DEV), c.repeat(Q, 1, 1), align_corners=False).squeeze(1)
            t = point_sample(tgt[at:at + g][:, None].to(DEV), c.repeat(g, 1, 1), align_corners=False).squeeze(1)
            out[b, :, :g] = (cm * matcher_mod.batch_sigmoid_ce_loss(x, t) + cd * matcher_mod.batch_dice_loss(x, t)).cpu().double()
        at += g
    return out


def check_case(pred, tgt, counts, coords, what, weights=WEIGHTS):
    """Both comparisons for every weight pair; -> the mixed-weight result."""
    P = coords.shape[1]
    xg, tg = gathered(pred, tgt, counts, coords)
    x64, t64 = M.samples64(pred, tgt, counts, coords)
    e_x, e_t = M.sample_errors(pred, tgt)
    parts_g = M.parts64(xg, tg)[:4]
    parts_64 = M.parts64(x64, t64)[:4]
    got = None
    for cm, cd in weights:
        got = run(pred, tgt, counts, coords, cm, cd)
        for b, g in enumerate(counts):
            assert bool((got[b, :, g:] == 0).all()), what                      # exactly zero past the count
        want_g = M.cost_from_parts(*parts_g, P, cm, cd, counts)[0]
        bound_g = M.cost_bound(xg, tg, counts, cm, cd)
        err_g = (got - want_g).abs()
        want = M.cost_from_parts(*parts_64, P, cm, cd, counts)[0]
        bound = M.cost_bound(x64, t64, counts, cm, cd, e_x, e_t)
        err = (got - want).abs()
        err_torch = (torch_chain(pred, tgt, counts, coords, cm, cd) - want).abs()
        print("%s (%g, %g): contraction err %.3e (bound %.3e, worst ratio %.3f); end to end err %.3e (bound %.3e, worst ratio %.3f); "
              "torch chain err %.3e" % (what, cm, cd, float(err_g.max()), float(bound_g.max()),
                                        float((err_g / bound_g.clamp(min=1e-300)).max()), float(err.max()), float(bound.max()),
                                        float((err / bound.clamp(min=1e-300)).max()), float(err_torch.max())))
        assert bool((err_g <= bound_g).all()), what
        assert bool((err <= bound).all()), what
    return got


CASES = [
    (1, 1, (3,), 1, (7, 9), (14, 18)),
    (2, 5, (3, 0), 2, (7, 9), (1, 1)),
    (3, 31, (1, 37, 33), 63, (7, 9), (14, 18)),
    (2, 32, (64, 65), 64, (32, 32), (14, 18)),
    (2, 33, (64, 65), 65, (7, 9), (14, 18)),
    (1, 100, (512,), 127, (7, 9), (14, 18)),
    (3, 100, (1, 37, 33), 128, (7, 9), (1, 1)),
    (1, 33, (3,), 129, (32, 32), (14, 18)),
    (2, 100, (3, 0), 777, (32, 32), (14, 18)),
    (1, 1024, (5,), 65, (7, 9), (14, 18)),
    (1, 33, (5,), 12544, (32, 32), (14, 18)),
]


@pytest.mark.parametrize("B,Q,counts,P,hw,thw", CASES)
def test_cost_against_float64_contraction_and_end_to_end(B, Q, counts, P, hw, thw):
    pred, tgt, coords = M.random_case(B, Q, list(counts), P, hw, thw, seed=B + Q + P)
    check_case(pred, tgt, list(counts), coords, "B%d Q%d G%s P%d" % (B, Q, counts, P))


# ---- hard inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.HARD_CASES))
def test_hard_inputs(name):
    pred, tgt, coords, counts = M.HARD_CASES[name]()
    check_case(pred, tgt, counts, coords, name)


def test_perfect_match_holds_the_relative_bound_where_the_cancelling_form_has_no_digits_left():
    pred, tgt, coords, counts = M.case_perfect_match()
    G, P = counts[0], coords.shape[1]
    xg, tg = gathered(pred, tgt, counts, coords)
    assert torch.equal(xg[0, :G].abs(), torch.full((G, P), 80.0)) and bool(((tg == 0) | (tg == 1)).all())   # the samples are pixels
    ce_sum, _, _, _, tiny = M.parts64(xg, tg)
    want = ce_sum[0] / P
    diag = torch.arange(G)
    assert bool((want[diag, diag] < 2e-35).all()) and bool((want[diag, diag] > 1e-35).all()) and float(tiny[0][diag, diag].max()) == 0
    got = run(pred, tgt, counts, coords, 1.0, 0.0)[0]
    rel = ((got - want).abs() / want)[diag, diag]
    L, chunks = M.plan(1, pred.shape[1], G, P)
    print("perfect match: ce = %.3e, relative error %.3e, bound %.3e" % (float(want[0, 0]), float(rel.max()), (2 * L + chunks + 12) * M.U))
    assert bool((rel <= (2 * L + chunks + 1 + M.FACTOR + 1) * M.U).all())
    # sum softplus(x) - sum x t in fp32, the form the kernel does not use, has no correct digit here
    x32, t32 = xg[0, :G], tg[0, :G]
    cancelling = (torch.nn.functional.softplus(x32).sum(1) - (x32 * t32).sum(1)) / P
    assert bool(((cancelling.double() - want[diag, diag]).abs() > 0.5 * want[diag, diag]).all())


def test_nan_pixel_poisons_its_row_only_and_the_matcher_reports_it():
    pred, tgt, coords = M.random_case(2, 33, [3, 5], 777, seed=9)
    clean = run(pred, tgt, [3, 5], coords, 5.0, 2.0)
    bad = pred.clone()
    bad[1, 7] = float("nan")
    got = run(bad, tgt, [3, 5], coords, 5.0, 2.0)
    assert bool(got[1, 7, :5].isnan().all())
    keep = torch.ones(2, 33, dtype=torch.bool)
    keep[1, 7] = False
    assert torch.equal(got[keep], clean[keep])
    m = matcher_mod.Point_HungarianMatcher(5.0, 2.0, num_points=70)
    m.match_cost = "hip"
    targets = [{"masks": tgt[:3].to(DEV)}, {"masks": tgt[3:].to(DEV)}]
    m.forward({"pred_masks": pred.to(DEV)}, targets)
    m.check()
    m.forward({"pred_masks": bad.to(DEV)}, targets)
    with pytest.raises(ValueError, match="infeasible"):
        m.check()


def test_counts_that_differ_leave_other_images_alone():
    pred, tgt, coords = M.random_case(3, 33, [1, 37, 33], 129, seed=10)
    full = run(pred, tgt, [1, 37, 33], coords, 5.0, 2.0)
    assert bool((full[0, :, 1:] == 0).all()) and bool((full[2, :, 33:] == 0).all()) and bool((full[1] != 0).all())
    alone = run(pred[1:2], tgt[1:38], [37], coords[1:2], 5.0, 2.0)
    # the same chunking (B changes the split only through ceil(512 / groups) >= the two passes of 129 points): the same bits
    assert M.plan(3, 33, 37, 129) == M.plan(1, 33, 37, 129)
    assert torch.equal(full[1], alone[0])
    # a target plane outside the planes: NaN in its column, nothing read
    starts = torch.tensor([0, 1, 60], dtype=torch.int32, device=DEV)
    cnt = torch.tensor([1, 37, 33], dtype=torch.int32, device=DEV)
    out = point_loss.match_costs(pred.to(DEV), tgt.to(DEV), starts, cnt, coords.to(DEV), 5.0, 2.0, 37).cpu()
    assert bool(out[2, :, :11].isfinite().all()) and bool(out[2, :, 11:33].isnan().all()) and bool((out[2, :, 33:] == 0).all())
    assert torch.equal(out[:2].double(), full[:2])


def test_two_calls_give_the_same_bits():
    for B, Q, counts, P in ((2, 100, [64, 65], 777), (1, 33, [5], 12544)):
        pred, tgt, coords = M.random_case(B, Q, counts, P, seed=11)
        a, b = run(pred, tgt, counts, coords, 5.0, 2.0), run(pred, tgt, counts, coords, 5.0, 2.0)
        assert torch.equal(a, b)


def _raw_call(pred, tgt, starts, cnt, gmax, coords, cost, ws, cm=5.0, cd=2.0, P=None):
    B, Q, H, W = pred.shape
    return _lib.lib().pct_point_match_cost_f32(pred.data_ptr(), B, Q, H, W, tgt.data_ptr(), tgt.shape[0], tgt.shape[1], tgt.shape[2],
                                               starts.data_ptr(), cnt.data_ptr(), gmax, coords.data_ptr(),
                                               coords.shape[1] if P is None else P, cm, cd, ws.data_ptr(), cost.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)


def test_guard_bands_around_cost_and_workspace_stay_intact():
    for B, Q, counts, P in ((2, 33, [64, 65], 777), (3, 100, [1, 37, 33], 129)):
        pred, tgt, coords = M.random_case(B, Q, counts, P, seed=12)
        gmax, band = max(counts), 4096
        n_cost, n_ws = B * Q * gmax, point_loss.match_cost_workspace_bytes(B, Q, gmax, P) // 4
        cost = torch.full((band + n_cost + band,), SENTINEL, device=DEV)
        ws = torch.full((band + n_ws + band,), SENTINEL, device=DEV)
        starts, cnt = _vectors(counts)
        rc = _raw_call(pred.to(DEV), tgt.to(DEV), starts, cnt, gmax, coords.to(DEV), cost[band:], ws[band:])
        torch.cuda.synchronize()
        assert rc == 0
        for buf, n in ((cost, n_cost), (ws, n_ws)):
            assert bool((buf[:band] == SENTINEL).all()) and bool((buf[band + n:] == SENTINEL).all())
        assert not bool((cost[band:band + n_cost] == SENTINEL).any())              # fully overwritten
        assert torch.equal(cost[band:band + n_cost].view(B, Q, gmax).cpu().double(), run(pred, tgt, counts, coords, 5.0, 2.0))


def test_captured_call_replays_to_the_eager_bits():
    pred, tgt, coords = M.random_case(2, 100, [64, 65], 777, seed=13)
    p, t, c = pred.to(DEV), tgt.to(DEV), coords.to(DEV)
    starts, cnt = _vectors([64, 65])
    eager = point_loss.match_costs(p, t, starts, cnt, c, 5.0, 2.0, 65).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                # one stream: no parallel branches
        out = point_loss.match_costs(p, t, starts, cnt, c, 5.0, 2.0, 65)
    out.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- the matcher -------------------------------------------------------------------------------------------------------------
def _matcher_case(heads):
    g = torch.Generator().manual_seed(21)
    preds = [(torch.randn(2, 12, 40, 24, generator=g) * 3).to(DEV) for _ in range(heads)]
    masks = [(torch.rand(n, 80, 48, generator=g) > 0.5).float() for n in (3, 5)]
    return preds, masks, [{"masks": m.to(DEV)} for m in masks]


@pytest.mark.parametrize("heads", [1, 10])
def test_matcher_hip_against_torch_same_seed(monkeypatch, heads):
    preds, masks, targets = _matcher_case(heads)
    P, counts = 70, [3, 5]
    real_sample, real_einsum, real_costs = matcher_mod.point_sample, torch.einsum, point_loss.match_costs
    calls, planes_seen = [], []
    monkeypatch.setattr(matcher_mod, "point_sample", lambda *a, **k: calls.append((mode, "point_sample")) or real_sample(*a, **k))
    monkeypatch.setattr(torch, "einsum", lambda *a, **k: calls.append((mode, "einsum")) or real_einsum(*a, **k))
    monkeypatch.setattr(point_loss, "match_costs", lambda *a, **k: planes_seen.append(a[1].data_ptr()) or real_costs(*a, **k))
    result, rng = {}, {}
    for mode in ("torch", "hip"):
        m = matcher_mod.Point_HungarianMatcher(5.0, 2.0, num_points=P)
        m.match_cost = mode
        torch.manual_seed(31)
        outs = [{"pred_masks": p} for p in preds]
        result[mode] = [m.forward(outs[0], targets)] if heads == 1 else m.forward_many(outs, targets)
        m.check()
        rng[mode] = torch.cuda.get_rng_state()
        if mode == "hip" and heads > 1:
            m.forward(outs[0], targets)                                          # a later call with the same masks: still cached
    monkeypatch.undo()
    assert {c[0] for c in calls} == {"torch"} and ("torch", "einsum") in calls and ("torch", "point_sample") in calls
    assert len(planes_seen) == heads + (heads > 1) and len(set(planes_seen)) == 1   # converted once
    assert torch.equal(rng["torch"], rng["hip"])
    torch.manual_seed(31)
    tgt = torch.cat(masks)
    for k in range(heads):
        coords = torch.cat([torch.rand(1, P, 2, device=DEV) for _ in range(2)]).cpu()
        pred = preds[k].cpu()
        C = M.cost64(pred, tgt, counts, coords, 5.0, 2.0)
        x64, t64 = M.samples64(pred, tgt, counts, coords)
        bound = M.cost_bound(x64, t64, counts, 5.0, 2.0, *M.sample_errors(pred, tgt))
        for b, g in enumerate(counts):
            ri, ci = linear_sum_assignment(C[b, :, :g].numpy())
            best = float(C[b, ri, ci].sum())
            slack = 2 * min(12, g) * float(bound[b].max())
            for mode in ("torch", "hip"):
                i, j = (v.cpu() for v in result[mode][k][b])
                assert len(i) == g and sorted(j.tolist()) == list(range(g))
                total = float(C[b, i, j].sum())
                print("head %d image %d %s: total %.9f, optimum %.9f, slack %.3e" % (k, b, mode, total, best, slack))
                if mode == "hip":
                    assert total - best <= slack


def test_matcher_keeps_the_torch_chain_where_the_kernel_does_not_apply(monkeypatch):
    preds, masks, targets = _matcher_case(1)
    called = []
    real = point_loss.match_costs
    monkeypatch.setattr(point_loss, "match_costs", lambda *a, **k: called.append(1) or real(*a, **k))
    got = {}
    for mode in ("torch", "hip"):
        m = matcher_mod.Point_HungarianMatcher(5.0, 2.0, num_points=70)
        m.match_cost = mode
        torch.manual_seed(5)
        got[mode] = m.forward({"pred_masks": preds[0].transpose(2, 3)}, targets)   # not contiguous
    assert not called
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got["torch"], got["hip"]))


# ---- argument errors: status codes, nothing launched ---------------------------------------------------------------------------
def test_argument_errors_return_status_codes_without_a_launch():
    fn = _lib.lib().pct_point_match_cost_f32
    BAD, ALIGN, UNSUP = -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # host pointer, never dereferenced
    assert p % 16 == 0

    def call(pred=p, B=2, Q=5, H=7, W=9, tgt=p, n=3, Ht=14, Wt=18, starts=p, counts=p, gmax=3, coords=p, P=70, ws=p, cost=p):
        return fn(pred, B, Q, H, W, tgt, n, Ht, Wt, starts, counts, gmax, coords, P, 5.0, 2.0, ws, cost, None)
    for kw in (dict(B=-1), dict(Q=-1), dict(gmax=-1), dict(P=-1), dict(n=-1), dict(H=0), dict(Wt=0)):
        assert call(**kw) == BAD, kw
    for name in ("pred", "tgt", "starts", "counts", "coords", "ws", "cost"):
        assert call(**{name: None}) == BAD, name
    assert call(coords=p + 4) == ALIGN and call(ws=p + 8) == ALIGN and call(pred=p + 2) == ALIGN and call(counts=p + 1) == ALIGN
    assert call(H=65536, W=65536) == UNSUP and call(Ht=65536, Wt=65536) == UNSUP and call(B=65536) == UNSUP
    assert call(P=2 ** 30 + 1) == UNSUP
    for kw in (dict(B=0), dict(Q=0), dict(gmax=0), dict(P=0)):       # nothing launched, nothing written
        assert call(**kw) == 0, kw
    assert call(B=0, pred=None, cost=None) == 0
    # the assignment's limits are covered
    assert point_loss.match_cost_supported(torch.zeros(1, 1024, 2, 2, device=DEV), torch.zeros(512, 2, 2, device=DEV), 70, 512)
    # P == 0 leaves the output as it was
    cost = torch.full((2 * 5 * 3,), SENTINEL, device=DEV)
    z = torch.zeros(64, device=DEV)
    zi = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert fn(z.data_ptr(), 2, 5, 2, 2, z.data_ptr(), 3, 2, 2, zi.data_ptr(), zi.data_ptr(), 3, z.data_ptr(), 0, 5.0, 2.0,
              z.data_ptr(), cost.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((cost == SENTINEL).all())
    with pytest.raises(RuntimeError):
        point_loss.match_costs(torch.zeros(2, 5, 2, 2, device=DEV), torch.zeros(3, 2, 2, device=DEV), zi, zi,
                               torch.zeros(2, 0, 2, device=DEV), 5.0, 2.0, 3)

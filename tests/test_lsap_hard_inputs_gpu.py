"""GPU: the batched Hungarian assignment (csrc/lsap.hip) on the cost families of tests/hard_inputs.py -- long searches with
rerouting and dual updates of scanned targets (Machol-Wien, rank-one + noise), exact ties across lanes, lane iterations and
waves (duplicated queries), +inf entries, infeasibility that only the search sees, extreme magnitudes, a trained model's
collapsed queries -- on both sides of the LDS-residency limit and at the declared limits Q = 1024, G = 512.

One launch per case.  The kernel's total, summed in fp64 from the fp32 costs, is compared with scipy's: equal for the integer
families, within 1e-12 * sum|chosen costs| otherwise (fp64 summation order over at most 512 terms).  Totals, not
assignments: on tie-bearing inputs any optimum is right; how many problems also return scipy's assignment is printed."""
import math

import numpy as np
import pytest
import torch

import hard_inputs as hi

pytestmark = pytest.mark.gpu


def _launch(cost, counts):
    from pctrans_amd import fused_ops
    c = torch.tensor(cost).cuda()                                          # (a copy: the cached cases are read-only)
    assert fused_ops.lsap_supported(c)
    rows, status = fused_ops.lsap(c, torch.tensor(counts, dtype=torch.int32))
    return rows.cpu().numpy(), status.cpu().numpy()


def _check_problem(cost, g, rows, ref, exact):
    """rows[:g] an injection into [0, Q), -1 behind; the fp64 total against scipy's.  -> same assignment as scipy?"""
    Q = cost.shape[0]
    assert (rows[g:] == -1).all()
    r = rows[:g].astype(np.int64)
    assert ((r >= 0) & (r < Q)).all() and len(set(r.tolist())) == g
    chosen = cost[r, np.arange(g)].astype(np.float64)
    assert np.isfinite(chosen).all()                                       # never an infinite entry
    total = float(chosen.sum())
    if exact:
        assert total == ref[1], (total, ref[1])
    else:
        assert abs(total - ref[1]) <= 1e-12 * float(np.abs(chosen).sum()), (total, ref[1])
    return bool((r == ref[0]).all())


def _check_case(name):
    cost, counts, ref = hi.lsap_case(name)
    rows, status = _launch(cost, counts)
    assert status.tolist() == [0] * len(counts)
    same = sum(_check_problem(cost[b, :, :g], g, rows[b], ref[b], name in hi.LSAP_INTEGER_CASES)
               for b, g in enumerate(counts))
    print("%s: %d of %d problems with scipy's assignment" % (name, same, len(counts)))
    return rows


@pytest.mark.parametrize("name", sorted(n for n in hi.LSAP_CASES if n != "machol_wien-1024x512"))
def test_hard_costs_reach_scipys_total(name):
    _check_case(name)


def test_machol_wien_at_both_limits_next_to_trivial_problems():
    """(1024, 512) Machol-Wien, the one long case: one workgroup runs about 1.3e5 Dijkstra sweeps over 1024 queries, with
    costs read from global memory (2 MB per problem).  In the same launch a problem without targets and one with a single
    target.  Measured on an MI355X: 1.1 s for this whole test, the 0.3 s of scipy's reference solution included."""
    rows = _check_case("machol_wien-1024x512")
    assert (rows[1] == -1).all() and rows[2, 0] == 0                      # g = 0: nothing; g = 1: the cheapest query


@pytest.mark.parametrize("Q,G", [(300, 60), (300, 128)])
def test_hall_violation_is_reported_and_leaves_its_neighbours_alone(Q, G):
    cost, counts = hi.hall_violation(Q, G, 51)
    rows, status = _launch(cost, counts)
    assert status.tolist() == [0, 1, 0]
    assert (rows[1] == -1).all()
    for b in (0, 2):
        ref = hi.scipy_solve(cost[b:b + 1], counts[b:b + 1])[0]
        _check_problem(cost[b, :, :counts[b]], counts[b], rows[b], ref, exact=False)


def test_matcher_like_totals_agree_between_device_and_host_assignment():
    """Point_HungarianMatcher on a trained model's collapsed queries (exact copies, near-perfect masks), device assignment
    on and off under the same seed: the matched costs, summed exactly, must be equal."""
    from pctrans_amd.loss.matcher import Point_HungarianMatcher
    outputs, targets = hi.matcher_like()
    outputs = {"pred_masks": outputs["pred_masks"].cuda()}
    targets = [{"masks": t["masks"].cuda()} for t in targets]
    m = Point_HungarianMatcher(cost_mask=5.0, cost_dice=5.0, num_points=256)
    torch.manual_seed(1)
    cost = m._batched_costs(outputs, targets)[0].double().cpu().numpy()
    torch.manual_seed(1)
    on_dev = m(outputs, targets)
    m.check()
    m.device_lsap = False
    torch.manual_seed(1)
    on_host = m(outputs, targets)
    same = 0
    for b, ((i, j), (ih, jh)) in enumerate(zip(on_dev, on_host)):
        g = targets[b]["masks"].shape[0]
        assert i.is_cuda and not ih.is_cuda
        i, j, ih, jh = (t.cpu().numpy() for t in (i, j, ih, jh))
        assert len(set(i.tolist())) == g and sorted(j.tolist()) == list(range(g))
        dev, host = math.fsum(cost[b, i, j]), math.fsum(cost[b, ih, jh])
        print("image %d: device %.17g host %.17g" % (b, dev, host))
        assert dev == host
        same += bool((i == ih).all() and (j == jh).all())
    print("matcher_like: %d of %d images with scipy's assignment" % (same, len(on_dev)))


@pytest.mark.parametrize("Q,G", [(1025, 4), (600, 513)])
def test_one_past_either_limit_takes_the_host_path_without_a_launch(Q, G, monkeypatch):
    from pctrans_amd import fused_ops
    from pctrans_amd.loss.matcher import Point_HungarianMatcher
    assert not fused_ops.lsap_supported(torch.zeros(1, Q, G, device="cuda"))
    assert fused_ops.lsap_supported(torch.zeros(1, min(Q, 1024), min(G, 512), device="cuda"))
    calls = []
    real = fused_ops.lsap
    monkeypatch.setattr(fused_ops, "lsap", lambda c, n: (calls.append(tuple(c.shape)), real(c, n))[1])
    g = torch.Generator().manual_seed(Q + G)
    pred = (torch.randn(1, Q, 8, 8, generator=g) * 2).cuda()
    targets = [{"masks": (torch.rand(G, 8, 8, generator=g) > 0.5).float().cuda()}]
    m = Point_HungarianMatcher(cost_mask=5.0, cost_dice=5.0, num_points=32)
    for run in (m, m.forward_many):
        torch.manual_seed(2)
        got = run({"pred_masks": pred}, targets) if run is m else run([{"pred_masks": pred}], targets)[0]
        (i, j), = got
        assert not i.is_cuda and i.shape == (G,) and len(set(i.tolist())) == G and sorted(j.tolist()) == list(range(G))
    assert calls == [] and m.pending_status == []
    with pytest.raises(RuntimeError, match="lsap"):                        # the entry point refuses too
        real(torch.zeros(1, Q, G, device="cuda"), torch.tensor([1], dtype=torch.int32))

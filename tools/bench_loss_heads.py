"""Times the mask losses and the matcher costs of the ten prediction heads of a step, head by head against all heads in one
launch (SetCriterion.loss_heads / Point_HungarianMatcher.cost_heads = "each" | "batched"), on inputs resident in HBM at the two
training geometries of tools/bench_point_loss.py (2 x 100 queries on 224^2 planes with 20 targets, 2 x 300 on 256^2 with 60;
P = 12 544 points; ten heads), both arms alternating in one process:

  loss          ten loss_masks forward + backward with point_loss = point_select = "hip"  (the arm "each" is the path before
                the head dimension existed) against one batched forward + backward of all heads
  forward_many  the ten cost passes and the assignment with match_cost = "hip", head by head against one batched cost pass

HIP events around each arm, one warm-up round, then `--rounds` (at least five) alternating rounds; medians and the spread (min,
max) are reported.  Per arm also the launches of this project's kernels (counted by pctrans_amd._timing in a pass of its own),
the peak of allocated memory above what is resident before the arm, and the bytes of the pre-drawn candidates
(heads * K * 3 P * 8 for "batched", K * 3 P * 8 at a time for "each").

    python tools/bench_loss_heads.py [--out profiles/loss_heads.json] [--quick] [--rounds 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_point_loss import GEOMETRIES, POINTS, PREDICTIONS, make_case   # noqa: E402
from pctrans_amd import _timing                                            # noqa: E402
from pctrans_amd.loss.maskformer_criterion import SetCriterion            # noqa: E402
from pctrans_amd.loss.matcher import Point_HungarianMatcher               # noqa: E402

ARMS = ("each", "batched")


def criterion_for(mode):
    c = SetCriterion(1, Point_HungarianMatcher(cost_mask=5.0, cost_dice=5.0, num_points=POINTS), {}, 0.1, ["masks"], POINTS, 3.0,
                     0.75)
    c.point_loss = c.point_select = c.matcher.match_cost = "hip"
    c.loss_heads = c.matcher.cost_heads = mode
    return c


def loss_pass(criterion, preds, targets, indices, num_masks):
    """-> ([forward, backward] ms, summed loss): the ten heads' mask losses and their backward, in the criterion's mode."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for p in preds:
        p.grad = None
    torch.cuda.synchronize()
    ev[0].record()
    if criterion.loss_heads == "batched":
        outputs = {"pred_masks": preds[-1], "aux_outputs": [{"pred_masks": p} for p in preds[:-1]],
                   "indices_list": indices[:-1] + [indices[-1]]}
        per_head = criterion._loss_masks_batched(outputs, targets, num_masks)
        if per_head is None:
            raise SystemExit("the batched path does not cover this case")
    else:
        per_head = [criterion.loss_masks({"pred_masks": p}, targets, ind, num_masks)
                    for p, ind in zip([preds[-1]] + preds[:-1], [indices[-1]] + indices[:-1])]
    total = sum(5.0 * d["loss_mask"] + 5.0 * d["loss_dice"] for d in per_head)
    ev[1].record()
    total.backward()
    ev[2].record()
    torch.cuda.synchronize()
    return [ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])], float(total.detach())


def match_pass(matcher, outs, targets):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    with torch.no_grad():
        out = matcher.forward_many(outs, targets)
    e1.record()
    torch.cuda.synchronize()
    matcher.check()
    return e0.elapsed_time(e1), out


def launches_and_peak(fn):
    """-> ({kernel name: launches}, peak bytes allocated above what was resident) of one call of fn."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _timing.kernel_timing(True)
    fn()
    rec = _timing.kernel_timing(False)
    torch.cuda.synchronize()
    names = {}
    for r in rec:
        names[r[0]] = names.get(r[0], 0) + 1
    return names, torch.cuda.max_memory_allocated() - base


def stats(v):
    s = sorted(v)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "runs_ms": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the smaller geometry only")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_heads.py needs a GPU: a timing taken elsewhere says nothing about it")
    rounds = max(5, args.rounds)
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "points": POINTS, "heads": PREDICTIONS, "rounds": rounds, "geometries": []}
    for geo in (GEOMETRIES[:1] if args.quick else GEOMETRIES):
        preds, targets = make_case(geo["B"], geo["Q"], geo["size"], geo["G"], dev)
        outs = [{"pred_masks": p.detach()} for p in preds]
        num_masks = 1.0 * sum(len(t["labels"]) for t in targets)
        crits = {mode: criterion_for(mode) for mode in ARMS}
        torch.manual_seed(100)
        indices = crits["each"].matcher.forward_many(outs, targets)
        crits["each"].matcher.check()
        K = sum(int(s.shape[0]) for s, _ in indices[0])
        loss_ms = {m: {"forward": [], "backward": [], "total": []} for m in ARMS}
        many_ms = {m: [] for m in ARMS}
        totals, matched = {}, {}
        for it in range(rounds + 1):                            # the first round warms both arms up
            for mode in ARMS:
                torch.manual_seed(200 + it)
                (fwd, bwd), totals[mode] = loss_pass(crits[mode], preds, targets, indices, num_masks)
                torch.manual_seed(300 + it)
                ms, matched[mode] = match_pass(crits[mode].matcher, outs, targets)
                if it:
                    loss_ms[mode]["forward"].append(fwd)
                    loss_ms[mode]["backward"].append(bwd)
                    loss_ms[mode]["total"].append(fwd + bwd)
                    many_ms[mode].append(ms)
        same = sum(bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
                   for ka, kb in zip(matched["each"], matched["batched"]) for a, b in zip(ka, kb))
        counted = {}
        for mode in ARMS:
            torch.manual_seed(400)
            l_names, l_peak = launches_and_peak(lambda: loss_pass(crits[mode], preds, targets, indices, num_masks))
            torch.manual_seed(500)
            m_names, m_peak = launches_and_peak(lambda: match_pass(crits[mode].matcher, outs, targets))
            counted[mode] = {"loss_launches": l_names, "loss_launches_total": sum(l_names.values()), "loss_peak_bytes": l_peak,
                             "forward_many_launches": m_names, "forward_many_launches_total": sum(m_names.values()),
                             "forward_many_peak_bytes": m_peak}
        cand = K * int(POINTS * 3.0) * 8
        entry = dict(geo, pairs_per_head=K,
                     candidate_bytes={"each": cand, "batched": PREDICTIONS * cand},
                     loss={m: {k: stats(v) for k, v in loss_ms[m].items()} for m in ARMS},
                     forward_many={m: stats(many_ms[m]) for m in ARMS},
                     counted=counted,
                     loss_sum={m: totals[m] for m in ARMS},
                     assignments_equal="%d of %d" % (same, PREDICTIONS * geo["B"]))
        record["geometries"].append(entry)
        print(json.dumps(entry), flush=True)
        del preds, targets, outs, crits, matched, indices
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Times the matcher's cost pass (Point_HungarianMatcher._batched_costs) on inputs resident in HBM at the two training
geometries of tools/bench_point_loss.py (2 x 100 queries on 224^2 planes with 20 targets, 2 x 300 on 256^2 with 60; P = 12 544
points), three paths alternating in one process:

  torch        torch sampling (point_sample) + the torch chain           (point_sample = "torch", match_cost = "torch")
  gather       the device gather + the torch chain: the best path before  (point_sample = "hip",   match_cost = "torch")
  fused        pct_point_match_cost_f32                                   (match_cost = "hip")

  costs        the ten _batched_costs calls of a step
  forward_many the same ten predictions through forward_many, the assignment included
  kernel alone match_costs back to back, and the bytes it has to move (both plane sets once, the cost matrix) over that time

Three timed runs each after one warm-up; medians are reported.

    python tools/bench_match_cost.py [--out profiles/match_cost.json] [--quick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_point_loss import GEOMETRIES, POINTS, PREDICTIONS, make_case   # noqa: E402
from pctrans_amd import point_loss                                         # noqa: E402
from pctrans_amd.loss.matcher import Point_HungarianMatcher               # noqa: E402

HBM_BYTES_PER_S = 8.0e12
PATHS = {"torch": ("torch", "torch"), "gather": ("hip", "torch"), "fused": ("torch", "hip")}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the smaller geometry only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_match_cost.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "points": POINTS, "calls_per_run": PREDICTIONS, "geometries": []}
    for geo in (GEOMETRIES[:1] if args.quick else GEOMETRIES):
        preds, targets = make_case(geo["B"], geo["Q"], geo["size"], geo["G"], dev)
        outs = [{"pred_masks": p.detach()} for p in preds]
        matchers = {}
        for name, (sample, cost) in PATHS.items():
            m = Point_HungarianMatcher(cost_mask=5.0, cost_dice=5.0, num_points=POINTS)
            m.point_sample, m.match_cost = sample, cost
            matchers[name] = m
        cost_ms, many_ms = {k: [] for k in PATHS}, {k: [] for k in PATHS}
        costs, matched = {}, {}
        with torch.no_grad():
            for it in range(4):                                # the first round warms every path up
                for name, m in matchers.items():
                    torch.manual_seed(200 + it)
                    ms, out = timed(lambda: [m._batched_costs(o, targets)[0] for o in outs])
                    if it:
                        cost_ms[name].append(ms)
                    costs[name] = out[0]
                    del out
                    torch.manual_seed(300 + it)
                    ms, out = timed(lambda: m.forward_many(outs, targets))
                    m.check()
                    if it:
                        many_ms[name].append(ms)
                    matched[name] = out
            G = geo["G"]
            diff = float((costs["fused"][:, :, :G] - costs["gather"][:, :, :G]).abs().max())
            same = sum(bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
                       for ka, kb in zip(matched["fused"], matched["gather"]) for a, b in zip(ka, kb))
            planes, starts, counts = matchers["fused"]._match_target_planes(targets, preds[0])
            coords = torch.rand(geo["B"], POINTS, 2, device=dev)
            reps = 50
            kernel_ms, _ = timed(lambda: [point_loss.match_costs(preds[i % PREDICTIONS].detach(), planes, starts, counts, coords,
                                                                 5.0, 5.0, G) for i in range(reps)])
        kernel_us = kernel_ms / reps * 1e3
        moved = 4 * (preds[0].numel() + planes.numel() + geo["B"] * geo["Q"] * G) + 8 * coords.numel() // 2
        ws = point_loss.match_cost_workspace_bytes(geo["B"], geo["Q"], G, POINTS)
        entry = dict(geo, costs_ms={k: v for k, v in cost_ms.items()}, forward_many_ms={k: v for k, v in many_ms.items()},
                     costs_median_ms={k: median(v) for k, v in cost_ms.items()},
                     forward_many_median_ms={k: median(v) for k, v in many_ms.items()},
                     costs_gather_over_fused=median(cost_ms["gather"]) / median(cost_ms["fused"]),
                     costs_torch_over_fused=median(cost_ms["torch"]) / median(cost_ms["fused"]),
                     forward_many_gather_over_fused=median(many_ms["gather"]) / median(many_ms["fused"]),
                     kernel_us_per_call_back_to_back=kernel_us, kernel_bytes_moved=moved, workspace_bytes=ws,
                     kernel_bytes_per_s=moved / (kernel_us * 1e-6),
                     kernel_fraction_of_hbm_peak=moved / (kernel_us * 1e-6) / HBM_BYTES_PER_S,
                     max_abs_cost_difference_fused_vs_gather=diff,
                     assignments_equal_fused_vs_gather="%d of %d" % (same, PREDICTIONS * geo["B"]))
        record["geometries"].append(entry)
        print(json.dumps(entry), flush=True)
        del preds, targets, outs, matchers, costs, matched
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

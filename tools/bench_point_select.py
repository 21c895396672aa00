"""Times the choice of the uncertain points inside SetCriterion.loss_masks (point_loss = "hip") on inputs resident in HBM, the
torch chain (candidate gather + topk + gather + cat) against the selection kernel (point_select = "hip",
pctrans_amd/point_loss.py: select_uncertain_points), at the two training geometries of tools/bench_point_loss.py
(K = 40 pairs on 224^2 planes and K = 120 on 256^2; P = 12 544 points, S = 37 632 candidates, n = 9 408 kept):

  selection stage   from the drawn candidates to the [K, P, 2] coordinates, the fresh uniform tail included; ten calls per run
  kernel alone      pct_point_select_uncertain_f32 into a preallocated row, and the bytes it has to move over that time
  loss_masks        the ten loss_masks calls of a step with their backward

The two paths alternate in one process, three timed runs each after one warm-up; medians are reported.

    python tools/bench_point_select.py [--out profiles/point_select.json] [--quick]
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
from pctrans_amd.loss.maskformer_criterion import SetCriterion, calculate_uncertainty   # noqa: E402
from pctrans_amd.loss.matcher import Point_HungarianMatcher               # noqa: E402

CANDIDATES, KEPT = 3 * POINTS, int(0.75 * POINTS)
HBM_BYTES_PER_S = 8.0e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stage_torch(pred, src, cand):
    K = cand.shape[0]
    logits = point_loss.point_sample_planes(pred, src, cand, 1)
    idx = torch.topk(calculate_uncertainty(logits[:, None])[:, 0, :], k=KEPT, dim=1)[1]
    coords = torch.gather(cand, 1, idx[:, :, None].expand(-1, -1, 2))
    return torch.cat([coords, torch.rand(K, POINTS - KEPT, 2, device=cand.device)], dim=1)


def stage_hip(pred, src, cand):
    K = cand.shape[0]
    coords = torch.empty(K, POINTS, 2, device=cand.device)
    point_loss.select_uncertain_points(pred, src, cand, KEPT, out=coords, with_index=False)
    coords[:, KEPT:] = torch.rand(K, POINTS - KEPT, 2, device=cand.device)
    return coords


def loss_pass(criterion, preds, targets, indices):
    for p in preds:
        p.grad = None
    total = 0
    num_masks = 1.0 * sum(len(t["labels"]) for t in targets)
    for p, ind in zip(preds, indices):
        losses = criterion.loss_masks({"pred_masks": p}, targets, ind, num_masks)
        total = total + 5.0 * losses["loss_mask"] + 5.0 * losses["loss_dice"]
    total.backward()
    return float(total.detach())


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the smaller geometry only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_select.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "points": POINTS, "candidates": CANDIDATES, "kept": KEPT,
              "calls_per_run": PREDICTIONS, "geometries": []}
    for geo in (GEOMETRIES[:1] if args.quick else GEOMETRIES):
        preds, targets = make_case(geo["B"], geo["Q"], geo["size"], geo["G"], dev)
        criterion = SetCriterion(1, Point_HungarianMatcher(cost_mask=5.0, cost_dice=5.0, num_points=POINTS), {}, 0.1, ["masks"],
                                 POINTS, 3.0, 0.75)
        criterion.point_loss = criterion.matcher.point_sample = "hip"
        torch.manual_seed(7)
        indices = criterion.matcher.forward_many([{"pred_masks": p} for p in preds], targets)
        criterion.matcher.check()
        Q = geo["Q"]
        srcs = [torch.cat([s.to(dev) + b * Q for b, (s, _) in enumerate(ind)]).to(torch.int32) for ind in indices]
        K = int(srcs[0].shape[0])
        cands = [torch.rand(K, CANDIDATES, 2, device=dev) for _ in preds]
        stages = {"torch": stage_torch, "hip": stage_hip}
        stage_ms, loss_ms, loss_value = {"torch": [], "hip": []}, {"torch": [], "hip": []}, {}
        same = None
        for it in range(4):                                    # the first round warms both paths up
            for mode in ("torch", "hip"):
                torch.manual_seed(200 + it)
                ms, out = timed(lambda: [stages[mode](p.detach(), s, c) for p, s, c in zip(preds, srcs, cands)])
                if it:
                    stage_ms[mode].append(ms)
                if mode == "torch":                              # the kept points as sets: x and y sorted per pair
                    kept_torch = [o[:, :KEPT].sort(dim=1)[0] for o in out]
                else:
                    same = [bool(torch.equal(a, o[:, :KEPT].sort(dim=1)[0])) for a, o in zip(kept_torch, out)]
                del out
                criterion.point_select = mode
                torch.manual_seed(300 + it)
                ms, value = timed(lambda: loss_pass(criterion, preds, targets, indices))
                if it:
                    loss_ms[mode].append(ms)
                loss_value[mode] = value
        row = torch.empty(K, POINTS, 2, device=dev)
        reps = 50
        kernel_ms, _ = timed(lambda: [point_loss.select_uncertain_points(preds[i % PREDICTIONS].detach(), srcs[i % PREDICTIONS],
                                                                          cands[i % PREDICTIONS], KEPT, out=row, with_index=False)
                                      for i in range(reps)])
        kernel_us = kernel_ms / reps * 1e3
        moved = K * (CANDIDATES * 8 + KEPT * 16)                # candidates read once, the kept ones read again and written
        entry = dict(geo, pairs=K, stage_torch_ms=stage_ms["torch"], stage_hip_ms=stage_ms["hip"],
                     stage_speedup_of_medians=median(stage_ms["torch"]) / median(stage_ms["hip"]),
                     loss_masks_torch_ms=loss_ms["torch"], loss_masks_hip_ms=loss_ms["hip"],
                     loss_masks_speedup_of_medians=median(loss_ms["torch"]) / median(loss_ms["hip"]),
                     loss_torch=loss_value["torch"], loss_hip=loss_value["hip"],
                     kernel_us_per_call_back_to_back=kernel_us, kernel_bytes_moved=moved,
                     kernel_bytes_per_s=moved / (kernel_us * 1e-6),
                     kernel_fraction_of_hbm_peak=moved / (kernel_us * 1e-6) / HBM_BYTES_PER_S,
                     workgroups=K, kept_points_equal_torch_per_call=same)
        record["geometries"].append(entry)
        print(json.dumps(entry), flush=True)
        del preds, targets, cands
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Times the point-sampled part of a training step on inputs resident in HBM: the ten matcher calls (Point_HungarianMatcher
.forward_many: point samples, costs, one assignment launch) and the ten SetCriterion.loss_masks calls of a step, forward and
backward, once with the torch formulation and once with the device kernels (pctrans_amd/point_loss.py: point_sample /
point_loss = "hip").  The two alternate in one process, three timed runs each after one warm-up, HIP events around each pass
and around its three phases.  Geometries: configs[2] (2 x 100 queries at 224^2, 20 targets per image at 448^2) and configs[3]
(2 x 300 at 256^2, 60 targets at 512^2) of BASELINE.json, 12 544 points.

    python tools/bench_point_loss.py [--out profiles/point_loss.json] [--quick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd.loss.maskformer_criterion import SetCriterion          # noqa: E402
from pctrans_amd.loss.matcher import Point_HungarianMatcher             # noqa: E402

GEOMETRIES = [dict(name="configs[2]", B=2, Q=100, size=224, G=20), dict(name="configs[3]", B=2, Q=300, size=256, G=60)]
POINTS = 12544
PREDICTIONS = 10


def make_case(B, Q, size, G, dev, seed=0):
    """Disc targets at twice the predictions' resolution; predictions: a third of the queries soft-edged discs near a target,
    the rest noise around a negative offset."""
    g = torch.Generator(device=dev).manual_seed(seed)
    T = 2 * size
    yy = torch.arange(T, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(T, device=dev, dtype=torch.float32)[None, :]
    targets, centres = [], []
    for b in range(B):
        c = torch.rand(G, 3, generator=g, device=dev)
        cy, cx, r = 20 + c[:, 0] * (T - 40), 20 + c[:, 1] * (T - 40), 6 + c[:, 2] * 10
        masks = (((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2) <= r[:, None, None] ** 2).float()
        targets.append({"masks": masks, "labels": torch.ones(G, dtype=torch.long, device=dev)})
        centres.append(torch.stack([cy, cx, r], 1).tolist())
    preds = []
    ys = torch.arange(size, device=dev, dtype=torch.float32)[:, None] * 2 + 0.5
    xs = torch.arange(size, device=dev, dtype=torch.float32)[None, :] * 2 + 0.5
    for _ in range(PREDICTIONS):
        p = torch.randn(B, Q, size, size, generator=g, device=dev) - 4.0
        for b in range(B):
            for q in range(0, Q, 3):
                cy, cx, r = centres[b][(q // 3) % G]
                p[b, q] += 4.0 + (r * 1.1 - torch.sqrt((ys - cy) ** 2 + (xs - cx) ** 2)) * 0.8
        preds.append(p.requires_grad_(True))
    return preds, targets


def one_pass(criterion, preds, targets):
    """-> (total ms, [matcher, loss forward, loss backward] ms, summed loss)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for p in preds:
        p.grad = None
    torch.cuda.synchronize()
    ev[0].record()
    indices = criterion.matcher.forward_many([{"pred_masks": p} for p in preds], targets)
    ev[1].record()
    total = 0
    for p, ind in zip(preds, indices):
        losses = criterion.loss_masks({"pred_masks": p}, targets, ind, 1.0 * sum(len(t["labels"]) for t in targets))
        total = total + 5.0 * losses["loss_mask"] + 5.0 * losses["loss_dice"]
    ev[2].record()
    total.backward()
    ev[3].record()
    torch.cuda.synchronize()
    criterion.matcher.check()
    return ev[0].elapsed_time(ev[3]), [ev[i].elapsed_time(ev[i + 1]) for i in range(3)], float(total.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the smaller geometry only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_loss.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "points": POINTS, "predictions_per_step": PREDICTIONS,
              "phases": ["matcher", "loss forward", "loss backward"], "geometries": []}
    for geo in (GEOMETRIES[:1] if args.quick else GEOMETRIES):
        preds, targets = make_case(geo["B"], geo["Q"], geo["size"], geo["G"], dev)
        criterion = SetCriterion(1, Point_HungarianMatcher(cost_mask=5.0, cost_dice=5.0, num_points=POINTS), {}, 0.1, ["masks"],
                                 POINTS, 3.0, 0.75)
        runs = {"torch": [], "hip": []}
        phases = {"torch": [], "hip": []}
        loss, grads = {}, {}
        for it in range(4):                                    # the first round warms both paths up
            for mode in ("torch", "hip"):
                criterion.point_loss = criterion.matcher.point_sample = mode
                torch.manual_seed(100 + it)
                ms, parts, value = one_pass(criterion, preds, targets)
                if it:
                    runs[mode].append(ms)
                    phases[mode].append(parts)
                loss[mode] = value
                grads[mode] = [p.grad.clone() for p in preds]
        scale = max(float(g.abs().max()) for g in grads["torch"])
        entry = dict(geo, torch_ms=runs["torch"], hip_ms=runs["hip"], torch_phase_ms=phases["torch"], hip_phase_ms=phases["hip"],
                     speedup_of_medians=sorted(runs["torch"])[1] / sorted(runs["hip"])[1],
                     loss_torch=loss["torch"], loss_hip=loss["hip"],
                     grad_max_difference_over_max=max(float((a - b).abs().max()) for a, b in zip(grads["torch"], grads["hip"])) / scale)
        record["geometries"].append(entry)
        print(json.dumps(entry), flush=True)
        del preds, targets, grads
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Times the validation metrics of a batch of label maps resident in HBM (pctrans_amd/metrics.py), two paths alternating in one
process:

  hip     pct_label_overlap + pct_label_metrics, results left on the device ("hip": status unread; "hip_checked": with the one
          small device -> host copy of the status words the metric functions make by default)
  host    what a user of the package has today: the device -> host copy of both maps, then the table-based numpy formulation
          (tests/metrics_reference.py: from_table -- np.unique, one bincount, the O(G * P) rules), image by image

and, for orientation only and outside the rounds, ONE image through the literal per-mask loops of the definitions (`literal`
there; `--no-literal` skips it), wall clock.

Shapes: CVPPP 530 x 500 with about 20 labels, BBBC 520 x 696 with about 200 labels; N = 1 and N = 20.  One warm-up round, then
`--repeats` timed rounds with the paths alternating; HIP events around each call (an event pair around host work measures that
work too: the second event is recorded when the host gets there) and the wall clock beside them; median, minimum and maximum.
Also reported per shape: the table pass's atomics per pixel (run heads of equal (g, p) pairs inside 64-pixel wave spans, counted
on the host from the maps), and that both paths give the same numbers.

    python tools/bench_metrics.py [--out profiles/metrics.json] [--repeats 9] [--no-literal]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_reference as R                                              # noqa: E402
from pctrans_amd import metrics as M                                       # noqa: E402

SHAPES = [
    dict(name="CVPPP", dataset="CVPPP", size=(530, 500), labels=20, radius=(40, 90)),
    dict(name="BBBC", dataset="BBBC", size=(520, 696), labels=200, radius=(8, 16)),
]
BATCHES = (1, 20)
KEYS = {"CVPPP": ("best_dice_pred", "best_dice_gt", "sbd", "abs_diff_fg"), "BBBC": ("aji", "dice", "dq", "sq", "pq")}


def make_case(s, N):
    gts = [R.random_instances(s["size"][0], s["size"][1], s["labels"], seed=100 + n, radius=s["radius"]) for n in range(N)]
    preds = [R.perturbed(g, seed=200 + n) for n, g in enumerate(gts)]
    return np.stack(preds), np.stack(gts)


def atomics_per_pixel(pred, gt):
    """Run heads of the table pass: a lane adds where it is lane 0 of its wave or its (g, p) pair differs from the lane before."""
    key = (gt.astype(np.int64) * 65536 + pred.astype(np.int64)).reshape(gt.shape[0], -1)
    head = np.ones_like(key, dtype=bool)
    head[:, 1:] = key[:, 1:] != key[:, :-1]
    head[:, ::64] = True
    return float(head.sum()) / key.size


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-literal", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "shapes": []}
    for s in SHAPES:
        for N in BATCHES:
            pred_np, gt_np = make_case(s, N)
            pred, gt = torch.from_numpy(pred_np).to(torch.int16).to(dev), torch.from_numpy(gt_np).to(torch.int16).to(dev)
            keys = KEYS[s["dataset"]]

            def hip(check=False):
                return M.instance_metrics(pred, gt, s["dataset"], mode="hip", check=check)

            def hip_checked():
                return hip(True)

            def host():
                p, g = pred.cpu().numpy(), gt.cpu().numpy()
                return [R.from_table(p[n], g[n]) for n in range(N)]

            paths = {"hip": hip, "hip_checked": hip_checked, "host": host}
            ms, wall, out = {p: [] for p in paths}, {p: [] for p in paths}, {}
            for it in range(args.repeats + 1):                 # the first round warms every path up
                for name, fn in paths.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    out[name] = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if it:
                        ms[name].append(e0.elapsed_time(e1))
                        wall[name].append(1e3 * (t1 - t0))
            entry = dict(name=s["name"], N=N, height=s["size"][0], width=s["size"][1],
                         labels_gt=[int(len(np.unique(g))) for g in gt_np][:4], labels_pred=[int(len(np.unique(p))) for p in pred_np][:4],
                         atomics_per_pixel=atomics_per_pixel(pred_np, gt_np), status=out["hip"].status.cpu().tolist()[:4])
            for name in paths:
                entry[name] = dict(median_ms=median(ms[name]), min_ms=min(ms[name]), max_ms=max(ms[name]),
                                   wall_median_ms=median(wall[name]), ms=ms[name])
            entry["host_over_hip"] = entry["host"]["median_ms"] / entry["hip"]["median_ms"]
            entry["host_over_hip_checked"] = entry["host"]["median_ms"] / entry["hip_checked"]["median_ms"]
            got = {k: out["hip"][k].cpu().tolist() for k in keys}
            entry["max_abs_difference"] = max(abs(got[k][n] - out["host"][n][k]) for k in keys for n in range(N))
            entry["first_image"] = {k: got[k][0] for k in keys}
            if N == 1 and not args.no_literal:
                t0 = time.perf_counter()
                lit = R.literal(pred_np[0], gt_np[0])
                entry["literal_loops_one_image_wall_ms"] = 1e3 * (time.perf_counter() - t0)
                entry["max_abs_difference_to_literal"] = max(abs(got[k][0] - lit[k]) for k in keys)
            record["shapes"].append(entry)
            print(json.dumps({k: v for k, v in entry.items() if k not in paths}
                             | {p: entry[p]["median_ms"] for p in paths}), flush=True)
            del pred, gt
    M.clear_workspaces()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

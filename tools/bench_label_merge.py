"""Times the small-object merging of a batch of label maps resident in HBM (pctrans_amd/label_merge.py), the paths alternating in
one process:

  hip          pct_label_merge_small, results left on the device, status unread
  hip_again    the same call once more: the same-against-same control (what two timings of one path differ by here)
  hip_checked  with the one small device -> host copy of the status words that merge_small_objects makes by default
  host         what a user of the package had before: the device -> host copy of the maps, then the table-based numpy formulation
               (tests/label_merge_reference.py: merge -- np.unique, three bincounts, the table procedure), image by image
  host_torch   the same copy, then the package's own torch mode on the CPU tensors

Shapes: the reference's two test sets, 33 x 530 x 500 (CVPPP) and 50 x 520 x 696, each image with about 20 instances and a few
dozen fragments of 1 - 50 pixels (tests/label_merge_cases.py: random_map).  One warm-up round, then `--repeats` timed rounds with
the paths alternating; HIP events around each call (an event pair around host work measures that work too: the second event is
recorded when the host gets there) and the wall clock beside them; median, minimum and maximum.  Also reported per shape: merges
per pass, images with a tie, and that all paths give the same maps.

    python tools/bench_label_merge.py [--out profiles/label_merge.json] [--repeats 5]
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
import label_merge_cases as C                                              # noqa: E402
import label_merge_reference as R                                          # noqa: E402
from pctrans_amd import label_merge as LM                                  # noqa: E402

SHAPES = [dict(name="CVPPP_test", N=33, size=(530, 500)), dict(name="wide", N=50, size=(520, 696))]


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_merge.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "passes": list(LM.PASSES), "shapes": []}
    for s in SHAPES:
        N, (H, W) = s["N"], s["size"]
        rng = np.random.default_rng(7)
        maps = np.stack([C.random_map(rng, H, W, fragments=48, rectangles=(18, 23)) for _ in range(N)])
        labels = torch.from_numpy(maps).to(torch.int16).to(dev)

        def hip(check=False):
            return LM.merge_small_objects(labels, mode="hip", check=check)

        def host():
            m = labels.cpu().numpy()
            return np.stack([R.merge(m[n]).out for n in range(N)])

        paths = {"hip": hip, "hip_again": hip, "hip_checked": lambda: hip(True), "host": host,
                 "host_torch": lambda: LM.merge_small_objects(labels.cpu(), mode="torch")}
        ms, wall, out = {p: [] for p in paths}, {p: [] for p in paths}, {}
        for it in range(args.repeats + 1):                     # the first round warms every path up
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
        got = out["hip"].cpu().numpy()
        entry = dict(name=s["name"], N=N, height=H, width=W, distinct_values=out["hip"].num.cpu().tolist()[:4],
                     merges_per_pass=out["hip"].merges.sum(0).cpu().tolist()[:len(LM.PASSES)],
                     images_with_a_tie=int((out["hip"].status & LM.STATUS_TIE).ne(0).sum()),
                     images_with_another_status=int((out["hip"].status & ~LM.STATUS_TIE).ne(0).sum()),
                     pixels_changed=int((got != maps).sum()),
                     same_maps=bool(np.array_equal(got, out["host"]) and np.array_equal(got, out["host_torch"].numpy())
                                    and np.array_equal(got, out["hip_checked"].cpu().numpy())))
        for name in paths:
            entry[name] = dict(median_ms=median(ms[name]), min_ms=min(ms[name]), max_ms=max(ms[name]),
                               wall_median_ms=median(wall[name]), ms=ms[name])
        entry["hip_again_over_hip"] = entry["hip_again"]["median_ms"] / entry["hip"]["median_ms"]
        entry["host_over_hip"] = entry["host"]["median_ms"] / entry["hip"]["median_ms"]
        entry["host_over_hip_checked"] = entry["host"]["median_ms"] / entry["hip_checked"]["median_ms"]
        entry["host_torch_over_hip_checked"] = entry["host_torch"]["median_ms"] / entry["hip_checked"]["median_ms"]
        record["shapes"].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k not in paths} | {p: entry[p]["median_ms"] for p in paths}), flush=True)
        del labels
    LM.clear_workspaces()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

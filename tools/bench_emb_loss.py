"""Times SetCriterion.loss_embedding, forward + backward into the embedding, on inputs resident in HBM at the training shapes,
two paths alternating in one process:

  torch   the torch formulation: resized mask stack, argmax, torch.unique, one-hot membership matrix   (emb_loss = "torch")
  hip     pct_instance_label_map_f32 + pct_discriminative_loss_forward_f32 / _backward_f32           (emb_loss = "hip")

Shapes: configs[2] (B = 2, E = 16, 128 x 128, 24 targets of 512 x 512) and configs[3] (B = 2, E = 16, 130 x 174, 60 and 300
targets of 520 x 696).  Per path and shape: HIP-event time of one forward + backward (the host waits inside it where the path
synchronises), kernel launches and device->host copies of one extra profiled call, peak allocated bytes above the inputs.
One warm-up round, then `--repeats` timed rounds with the paths alternating; median, minimum and maximum are reported.

    python tools/bench_emb_loss.py [--out profiles/emb_loss.json] [--repeats 7] [--quick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd.loss import maskformer_criterion as crit                  # noqa: E402
from pctrans_amd.loss.matcher import Point_HungarianMatcher               # noqa: E402

SHAPES = [
    dict(name="configs[2]", B=2, E=16, size=(128, 128), mask_size=(512, 512), G=24),
    dict(name="configs[3], 60 targets", B=2, E=16, size=(130, 174), mask_size=(520, 696), G=60),
    dict(name="configs[3], 300 targets", B=2, E=16, size=(130, 174), mask_size=(520, 696), G=300),
]
PATHS = ("torch", "hip")


def make_case(s, dev):
    """Discs of radius 6 .. 15 (scaled with the mask's side) at random centres: instance masks as tools/record_train_configs.py
    draws them."""
    g = torch.Generator().manual_seed(1)
    H, W = s["mask_size"]
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    targets = []
    for _ in range(s["B"]):
        cy, cx = torch.randint(20, H - 20, (s["G"],), generator=g), torch.randint(20, W - 20, (s["G"],), generator=g)
        r = torch.randint(6, 16, (s["G"],), generator=g)
        targets.append({"masks": torch.stack([(((yy - int(y)) ** 2 + (xx - int(x)) ** 2) <= int(q) ** 2).float()
                                              for y, x, q in zip(cy, cx, r)])})
    emb = torch.randn(s["B"], s["E"], *s["size"], generator=g).to(dev)
    return emb, targets


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the first shape only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_emb_loss.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "shapes": []}
    for s in (SHAPES[:1] if args.quick else SHAPES):
        emb, targets = make_case(s, dev)
        crits = {}
        for path in PATHS:
            c = crit.SetCriterion(1, Point_HungarianMatcher(num_points=16), {}, 0.1, ["embedding"], 16, 3.0, 0.75)
            c.emb_loss = path
            crits[path] = c

        def call(path):
            x = emb.detach().requires_grad_(True)
            loss = crits[path].loss_embedding(x, targets)["loss_emb"]
            loss.backward()
            return loss.detach(), x.grad

        ms = {p: [] for p in PATHS}
        out = {}
        for it in range(args.repeats + 1):                     # the first round warms every path up
            for path in PATHS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                out[path] = call(path)
                e1.record()
                torch.cuda.synchronize()
                if it:
                    ms[path].append(e0.elapsed_time(e1))
        entry = dict(s)
        for path in PATHS:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            call(path)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                call(path)
                torch.cuda.synchronize()
            launches = d2h = 0
            for e in prof.events():
                if e.device_type == torch.autograd.DeviceType.CUDA:
                    launches += 1
                    d2h += "DtoH" in e.name
            entry[path] = dict(ms=ms[path], median_ms=median(ms[path]), min_ms=min(ms[path]), max_ms=max(ms[path]),
                               launches=launches, device_to_host_copies=d2h, peak_allocated_bytes=int(peak))
        entry["torch_over_hip"] = entry["torch"]["median_ms"] / entry["hip"]["median_ms"]
        entry["loss"] = {p: float(out[p][0]) for p in PATHS}
        entry["max_abs_gradient_difference"] = float((out["torch"][1] - out["hip"][1]).abs().max())
        record["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del emb, targets, crits, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

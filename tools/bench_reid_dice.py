"""Times the mask side of the query-contrast loss -- query_contrast.select_pos_neg_mask plus SetCriterion.loss_reid_mask on its
items, forward + backward into the mask logits -- on inputs resident in HBM at the two training shapes, two paths alternating in
one process:

  torch   sigmoid of all logits, the [N, Q, Q] matrix by bmm, the items' rows gathered; autograd's backward  (mask_dice = "torch")
  hip     pct_reid_dice_rows_forward_f32 / _backward_f32: the items' rows alone                              (mask_dice = "hip")

Shapes: configs[2] (N = 2, Q = 100, 224 x 224, 20 rows per image) and configs[3] (N = 2, Q = 300, 256 x 256, 60 rows per image).
The plan (which query is whose positive) is built once per shape and handed to both paths, so the timed stage holds no
device->host copy of its own.  Per path and shape: HIP-event time of one forward + backward, the kernels' own time where the
path records it (pctrans_amd/_timing.py), kernel launches of one extra profiled call, peak allocated bytes above the inputs.
One warm-up round, then `--repeats` timed rounds with the paths alternating; median, minimum and maximum are reported.

    python tools/bench_reid_dice.py [--out profiles/reid_dice.json] [--repeats 9] [--quick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import _timing                                            # noqa: E402
from pctrans_amd.loss import maskformer_criterion as crit                  # noqa: E402
from pctrans_amd.transformer_decoder import query_contrast as qc           # noqa: E402

SHAPES = [
    dict(name="configs[2]", N=2, Q=100, size=(224, 224), rows=20),
    dict(name="configs[3]", N=2, Q=300, size=(256, 256), rows=60),
]
PATHS = ("torch", "hip")


def make_case(s, dev):
    """Logits N(0, 3); `rows` matched queries per image, every other query assigned to a matched one round-robin (every cluster
    is non-empty: `rows` items per image, as a training step of the config has when every target is matched)."""
    g = torch.Generator().manual_seed(1)
    N, Q, R = s["N"], s["Q"], s["rows"]
    logits = (3 * torch.randn(N, Q, *s["size"], generator=g)).to(dev)
    plan = []
    for n in range(N):
        perm = torch.randperm(Q, generator=g).tolist()
        pos, rest = perm[:R], sorted(perm[R:])
        for j, p in enumerate(pos):
            cluster = rest[j::R]
            members = set(cluster) | {p}
            plan.append((n, p, cluster, [i for i in range(Q) if i not in members]))
    return logits, plan


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="the first shape only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reid_dice.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    c = crit.SetCriterion(1, None, {}, 0.1, [], 16, 3.0, 0.75)
    record = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "shapes": []}
    for s in (SHAPES[:1] if args.quick else SHAPES):
        logits, plan = make_case(s, dev)

        def call(path):
            z = logits.detach().requires_grad_(True)
            items = qc.select_pos_neg_mask(z, None, None, _plan_cache=plan, mask_dice=path)
            loss = c.loss_reid_mask({"pred_qd_mask": items}, None, None, 1.0)["loss_reid_mask"]
            loss.backward()
            return loss.detach(), z.grad

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
        entry = dict(s, logits_bytes=int(logits.numel() * 4))
        for path in PATHS:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            call(path)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            _timing.kernel_timing(True)
            call(path)
            torch.cuda.synchronize()
            kernels = {}
            for rec in _timing.kernel_timing(False):
                kernels[rec[0]] = kernels.get(rec[0], 0.0) + rec[1]
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                call(path)
                torch.cuda.synchronize()
            launches, dev_us = 0, 0.0
            for e in prof.events():
                if e.device_type == torch.autograd.DeviceType.CUDA:
                    launches += 1
                    dev_us += e.device_time if hasattr(e, "device_time") else e.cuda_time
            entry[path] = dict(ms=ms[path], median_ms=median(ms[path]), min_ms=min(ms[path]), max_ms=max(ms[path]),
                               launches=launches, device_ms_sum_of_kernels=dev_us / 1e3, timed_launches_ms=kernels,
                               peak_allocated_bytes=int(peak))
        entry["torch_over_hip"] = entry["torch"]["median_ms"] / entry["hip"]["median_ms"]
        entry["loss"] = {p: float(out[p][0]) for p in PATHS}
        entry["max_abs_gradient_difference"] = float((out["torch"][1] - out["hip"][1]).abs().max())
        entry["max_abs_gradient"] = float(out["torch"][1].abs().max())
        record["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del logits, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Times the query-contrast ("re-id") stage of a training step -- query_contrast.query_contrast_items plus
SetCriterion.loss_reid_query and loss_reid_mask on its items, forward + backward into the queries and the mask logits -- on inputs
resident in HBM at the two training shapes, three paths alternating in one process:

  torch   the [N, Q, Q] cosine table, the gathers / einsum / F.normalize, dice_for by bmm, _contrast_softplus     (every switch off)
  dice    the same with the mask side's rows from pct_reid_dice_rows_*                                            (reid_dice = "hip")
  hip     pct_reid_nearest_positive_f32, pct_reid_query_rows_*, pct_reid_dice_rows_* and pct_contrast_loss_rows_f32
                                                                       (reid_query = reid_dice = contrast_loss = "hip")

Shapes: configs[2] (N = 2, Q = 100, C = 256, 224 x 224 mask logits, 20 matched queries per image) and configs[3] (N = 2, Q = 300,
C = 256, 256 x 256, 60 per image), those of profiles/reid_dice_step.json.  The stage holds its one device->host copy (the
nearest-positive table) in every path.  Per path and shape: HIP-event time of one forward + backward, kernel launches of the
three parts of one extra profiled call (items, losses, backward), the kernels' own time where the path records it
(pctrans_amd/_timing.py), peak allocated bytes above the inputs.  One warm-up round, then `--repeats` timed rounds with the paths
alternating; median, minimum and maximum are reported.

    python tools/bench_reid_query.py [--out profiles/reid_query.json] [--repeats 9] [--quick]
"""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import _timing                                            # noqa: E402
from pctrans_amd.loss import maskformer_criterion as crit                  # noqa: E402
from pctrans_amd.transformer_decoder import query_contrast as qc           # noqa: E402

SHAPES = [
    dict(name="configs[2]", N=2, Q=100, C=256, size=(224, 224), G=20),
    dict(name="configs[3]", N=2, Q=300, C=256, size=(256, 256), G=60),
]
PATHS = {"torch": dict(reid_query="torch", mask_dice="torch", contrast_loss="torch"),
         "dice": dict(reid_query="torch", mask_dice="hip", contrast_loss="torch"),
         "hip": dict(reid_query="hip", mask_dice="hip", contrast_loss="hip")}


def make_case(s, dev):
    """Queries N(0, 1), mask logits N(0, 3), G matched queries per image drawn without replacement."""
    g = torch.Generator().manual_seed(1)
    N, Q, C, G = s["N"], s["Q"], s["C"], s["G"]
    query = torch.randn(Q, N, C, generator=g).to(dev)
    logits = (3 * torch.randn(N, Q, *s["size"], generator=g)).to(dev)
    indices = [(torch.randperm(Q, generator=g)[:G], torch.arange(G)) for _ in range(N)]
    return query, logits, indices


def median(v):
    return sorted(v)[len(v) // 2]


def launches_of(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="the first shape only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reid_query.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    c = crit.SetCriterion(1, None, {}, 0.1, [], 16, 3.0, 0.75)
    record = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "shapes": []}
    for s in (SHAPES[:1] if args.quick else SHAPES):
        query, logits, indices = make_case(s, dev)

        def parts(path):
            """The three parts of the stage as closures over one call's tensors."""
            sw = PATHS[path]
            x, z = query.detach().requires_grad_(True), logits.detach().requires_grad_(True)
            c.contrast_loss = sw["contrast_loss"]
            state = {}

            def items():
                random.seed(7)
                state["items"] = qc.query_contrast_items(x, z, indices, mask_dice=sw["mask_dice"], reid_query=sw["reid_query"])

            def losses():
                got = {**c.loss_reid_query({"pred_qd_query": state["items"][0]}, None, None, 1.0),
                       **c.loss_reid_mask({"pred_qd_mask": state["items"][1]}, None, None, 1.0)}
                state["losses"] = got
                state["total"] = got["loss_reid_query"] + 1.5 * got["loss_reid_query_aux"] + got["loss_reid_mask"]

            def backward():
                state["total"].backward()

            return x, z, state, (items, losses, backward)

        def call(path):
            x, z, state, fns = parts(path)
            for fn in fns:
                fn()
            return {k: float(v) for k, v in state["losses"].items()}, x.grad, z.grad, len(state["items"][0])

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
        entry = dict(s, items=out["torch"][3], query_bytes=int(query.numel() * 4), logits_bytes=int(logits.numel() * 4))
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
            _, _, _, fns = parts(path)
            launches = {fn.__name__: launches_of(fn)[1] for fn in fns}
            entry[path] = dict(ms=ms[path], median_ms=median(ms[path]), min_ms=min(ms[path]), max_ms=max(ms[path]),
                               launches=launches, launches_total=sum(launches.values()), timed_launches_ms=kernels,
                               peak_allocated_bytes=int(peak))
        entry["torch_over_hip"] = entry["torch"]["median_ms"] / entry["hip"]["median_ms"]
        entry["dice_over_hip"] = entry["dice"]["median_ms"] / entry["hip"]["median_ms"]
        entry["losses"] = {p: out[p][0] for p in PATHS}
        entry["same_items"] = out["torch"][3] == out["dice"][3] == out["hip"][3]
        for name, at in (("query", 1), ("logits", 2)):
            entry["max_abs_%s_gradient_difference" % name] = float((out["torch"][at] - out["hip"][at]).abs().max())
            entry["max_abs_%s_gradient" % name] = float(out["torch"][at].abs().max())
        record["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del query, logits, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

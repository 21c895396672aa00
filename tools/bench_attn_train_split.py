"""Forward + backward of ONE cross-attention of a training step at the key counts of the largest decoder level: the split-key HIP
training path (split_key_attention_train.cross_attention_train at 2 / 4 / 8 / 16 splits and at `plan`'s count) against the torch
chain it would replace (timed twice: the second arm is the control that shows what two runs of the same code differ by) and
against the unsplit kernels (attention_train.cross_attention_train), on fp32 operands with a mask of the decoder's kind (half the
entries dead, row_open = mask.all(-1)), 8 heads.  Geometries: (100 queries, 3 136 keys) and (300, 4 096) at 1, 2 and 4 images --
what the unsplit route leaves to torch -- and (100, 784), (300, 1 024) at 2 images, which it takes.  HIP events around `--iters`
repetitions after a warm-up, twice per arm: launched from Python per iteration and as replays of a HIP graph of one forward +
backward (the device's share; the routing rule reads these).  The arms alternate `--rounds` times in one process.

    python tools/bench_attn_train_split.py [--iters 50] [--rounds 3] [--out profiles/attn_train_split.json]

Per-kernel times come from a separate run under the profiler, one geometry and split count per process so that a kernel name
means one launch shape:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_attn_train_split.py --kernels 100,3136,2,8
    python tools/bench_attn_train_split.py --kernel-stats Q100-S3136-N2-x8=DIR --out profiles/attn_train_split.json

The second command needs no GPU: it adds the attention kernels' rows of DIR's *kernel_stats.csv to the record under that label.
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import attention_train as at, split_key_attention_train as sk  # noqa: E402

GEOMETRIES = [("largest level", Q, S, N) for Q, S in ((100, 3136), (300, 4096)) for N in (1, 2, 4)]
GEOMETRIES += [("middle level", 100, 784, 2), ("middle level", 300, 1024, 2)]
SPLITS = (2, 4, 8, 16)
HEADS, C = 8, 128


def torch_chain(q_c, q_s, k_c, k_p, v, mask, row_open):
    """CrossAttentionLayer.forward_post + attention_core between the projections and out_proj, as the parent runs them."""
    (Q, N, _), S, hd = q_c.shape, k_c.shape[0], C // HEADS
    mask = mask & ~row_open
    q = torch.cat([q_c.view(Q, N, HEADS, hd), q_s.view(Q, N, HEADS, hd)], dim=3).view(Q, N, 2 * C)
    k = torch.cat([k_c.view(S, N, HEADS, hd), k_p.view(S, N, HEADS, hd)], dim=3).view(S, N, 2 * C)
    qh = (q * float(2 * hd) ** -0.5).reshape(Q, N, HEADS, 2 * hd).permute(1, 2, 0, 3)
    kh = k.reshape(S, N, HEADS, 2 * hd).permute(1, 2, 3, 0)
    vh = v.reshape(S, N, HEADS, hd).permute(1, 2, 0, 3)
    p = torch.softmax(torch.matmul(qh, kh).masked_fill(mask, float("-inf")), dim=-1)
    return torch.matmul(p, vh).permute(2, 0, 1, 3).reshape(Q, N, C)


def operands(Q, S, N):
    torch.manual_seed(0)
    ops = [torch.randn(T, N, C, device="cuda", requires_grad=True) for T in (Q, Q, S, S, S)]
    mask = torch.rand(N, 1, Q, S, device="cuda") < 0.5
    mask[N - 1, 0, Q // 2] = True
    row_open = mask.all(-1, keepdim=True)
    assert sk.covered(*ops, HEADS, mask, row_open)
    return ops, mask, row_open, torch.randn(Q, N, C, device="cuda")


def runner(ops, mask, row_open, u):
    def run(arm):
        if arm.startswith("torch"):
            out = torch_chain(*ops, mask, row_open)
        elif arm == "unsplit":
            out = at.cross_attention_train(*ops, HEADS, mask, row_open)
        else:
            out = sk.cross_attention_train(*ops, HEADS, mask, row_open, splits=int(arm.split("x")[1]))
        out.backward(u)
        for t in ops:
            t.grad = None
    return run


def merge_kernel_stats(specs, out):
    rec = json.load(open(out)) if os.path.exists(out) else {}
    stats = rec.setdefault("kernel_stats", {})
    for spec in specs:
        label, root = spec.split("=", 1)
        files = sorted(glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True))
        if not files:
            raise SystemExit("no *kernel_stats.csv under " + root)
        rows = []
        for row in csv.DictReader(open(files[-1])):
            kernel = re.search(r"\bxats?_\w+", row.get("Name", ""))
            if kernel:
                rows.append({"kernel": kernel.group(0), "calls": int(row["Calls"]),
                             "average_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                             "max_us": round(float(row["MaxNs"]) / 1e3, 2)})
        stats[label] = sorted(rows, key=lambda r: r["kernel"])
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", default=None, metavar="Q,S,N,SPLITS",
                    help="run the unsplit and the split kernels of one geometry a few times and exit (for the profiler)")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="LABEL=DIR",
                    help="add the attention kernels' rows of DIR's *kernel_stats.csv to --out and exit (no GPU)")
    a = ap.parse_args()
    if a.kernel_stats:
        return merge_kernel_stats(a.kernel_stats, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_train_split.py needs the GPU: a CPU run times nothing")
    if a.kernels:
        Q, S, N, splits = (int(x) for x in a.kernels.split(","))
        run = runner(*operands(Q, S, N))
        for _ in range(20):
            run("unsplit")
            run("x%d" % splits)
        torch.cuda.synchronize()
        return
    records = []
    for name, Q, S, N in GEOMETRIES:
        ops, mask, row_open, u = operands(Q, S, N)
        run = runner(ops, mask, row_open, u)
        planned = max(1, sk.plan(Q, N, HEADS, S))
        arms = ["torch", "torch_control", "unsplit"] + ["x%d" % s for s in SPLITS]
        if planned not in SPLITS and planned >= 2:
            arms.append("x%d" % planned)

        def captured(arm):
            """One forward + backward of `arm` as a HIP graph: its replays are timed without the host's launch cost."""
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    run(arm)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(arm)
            return g

        def timed(fn):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.iters

        graphs = {arm: captured(arm) for arm in arms}
        for rnd in range(a.rounds):
            for arm in arms:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                eager = timed(lambda: run(arm))
                peak = torch.cuda.max_memory_allocated() - base
                replay = timed(graphs[arm].replay)
                rec = dict(level=name, N=N, heads=HEADS, Q=Q, S=S, round=rnd, arm=arm, plan=planned, iters=a.iters,
                           fwd_bwd_ms=round(eager, 4), graph_replay_ms=round(replay, 4),
                           peak_mib_above_operands=round(peak / 2 ** 20, 2))
                records.append(rec)
                print("N=%d Q=%d S=%d round %d %-13s fwd+bwd eager %.4f ms  graph replay %.4f ms  peak above operands %.2f MiB" % (
                    N, Q, S, rnd, arm, eager, replay, rec["peak_mib_above_operands"]), flush=True)
        del graphs
    if a.out:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        rec.update({"note": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0),
                    "plan_constants": dict(MAX_SPLITS=sk.MAX_SPLITS, MIN_CHUNKS=sk.MIN_CHUNKS, TARGET_WORKGROUPS=sk.TARGET_WORKGROUPS,
                                           MIN_KEYS=sk.MIN_KEYS),
                    "records": records})
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

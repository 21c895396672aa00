"""Times MaskFormer's eval-mode post-processing (everything after the head) on inputs resident in HBM: the torch formulation
(F.interpolate + instance_inference per image, as MaskFormer.forward runs it) against the device path
(pctrans_amd/postprocess.py, MaskFormer.postprocess = "hip").  The two alternate in one process, three timed runs each after
one warm-up, with HIP events around the whole post-processing.  Per geometry: both times, peak allocated memory, and for the
threshold kernel its algorithmic bytes (logits read once + 1 bit per output pixel + areas) over its own time against 8 TB/s.

    python tools/bench_postprocess.py [--out profiles/postprocess.json] [--dataset CVPPP] [--quick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import postprocess as post            # noqa: E402
from pctrans_amd.arch import maskformer as mfm         # noqa: E402

GEOMETRIES = [((512, 512), 100, 8), ((512, 512), 100, 32), ((512, 512), 100, 128), ((520, 696), 300, 8)]
HBM_BYTES_PER_S = 8e12


class _Head(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.masks = None

    def forward(self, features):
        return {"pred_masks": self.masks}, None


def make_logits(N, Q, h, w, device, seed=0):
    """bf16 query logits at the head's resolution (half the input's), built on the device: soft-edged discs, a third of the
    queries near-duplicates of their neighbour (merged), a third empty."""
    g = torch.Generator(device=device).manual_seed(seed)
    yy = torch.arange(h, device=device, dtype=torch.float32)[:, None]
    xx = torch.arange(w, device=device, dtype=torch.float32)[None, :]
    out = torch.full((N, Q, h, w), -9.0, device=device, dtype=torch.bfloat16)
    for n in range(N):
        c = torch.rand(Q, 3, generator=g, device=device)
        for q in range(0, Q, 3):
            cy, cx, r = float(c[q, 0]) * h, float(c[q, 1]) * w, 3.0 + float(c[q, 2]) * min(h, w) / 8
            d = torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            out[n, q] = ((r - d) * 0.9).bfloat16()
            if q + 1 < Q:
                out[n, q + 1] = ((r * 1.03 - d) * 0.9).bfloat16()
    return out


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dataset", default="CVPPP", choices=sorted(post.DATASETS))
    ap.add_argument("--quick", action="store_true", help="the smallest geometry only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_postprocess.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    record = {"dataset": args.dataset, "device": torch.cuda.get_device_name(0), "geometries": []}
    for (H, W), Q, N in (GEOMETRIES[:1] if args.quick else GEOMETRIES):
        head = _Head()
        net = mfm.MaskFormer(backbone=torch.nn.Identity(), sem_seg_head=head, criterion=torch.nn.Identity(), num_queries=Q,
                             dataset_name=args.dataset).eval()
        head.masks = make_logits(N, Q, H // 2, W // 2, dev)
        volume = torch.zeros(N, 1, H, W, device=dev)
        runs = {"torch": [], "hip": []}
        peak = {"torch": 0, "hip": 0}
        outs = {}
        for it in range(4):                                    # the first round warms both paths up
            for mode in ("torch", "hip"):
                net.postprocess = mode
                ms, mem, out = timed(lambda: net(volume)[0])
                if it:
                    runs[mode].append(ms)
                    peak[mode] = max(peak[mode], mem)
                outs[mode] = out
        thr = [timed(lambda: post.instance_masks(head.masks, (H, W), args.dataset))[0] for _ in range(4)][1:]
        algo = head.masks.numel() * 2 + N * Q * (H * W // 8 + 4)
        entry = {"size": [H, W], "queries": Q, "batch": N,
                 "torch_ms": runs["torch"], "hip_ms": runs["hip"],
                 "torch_peak_bytes": peak["torch"], "hip_peak_bytes": peak["hip"],
                 "hip_workspace_bytes_cached": post.workspace_bytes(N, Q, H, W),      # allocated once, outside the timed window
                 "speedup_of_medians": sorted(runs["torch"])[1] / sorted(runs["hip"])[1],
                 "labels_differ_share": float((outs["torch"] != outs["hip"]).float().mean()),
                 "threshold_kernel_ms": thr, "threshold_algorithmic_bytes": algo,
                 "threshold_share_of_8TBps": algo / (sorted(thr)[1] * 1e-3) / HBM_BYTES_PER_S}
        record["geometries"].append(entry)
        print(json.dumps(entry), flush=True)
        del head.masks, outs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Forward + backward of ONE cross-attention of a training step, the HIP training path (attention_train.cross_attention_train)
against the torch chain it replaces (the two per-head concatenations, q * scale, matmul, masked_fill, softmax, matmul and
their autograd backward), on fp32 operands at the key counts of configs[2] (448^2 crops: 196, 784, 3 136 keys; 100 queries)
and configs[3] (512^2 crops: 256, 1 024, 4 096 keys; 300 queries), 2 images, 8 heads, with a mask of the decoder's kind (half
the entries dead, row_open = mask.all(-1)).  HIP events around `--iters` repetitions after a warm-up, twice per arm: launched
from Python per iteration (what an eager step pays; both arms are host-bound at these sizes: the torch arm takes the same time at
196 and at 4 096 keys) and as replays of a HIP graph of one forward + backward (the device's share).  The two paths alternate
`--rounds` times in one process so that the spread between alternations can be read beside the difference.  Prints one line
per (geometry, round, path) and writes every figure to `--out` as JSON.

    python tools/bench_attn_train.py [--iters 50] [--rounds 3] [--out profiles/attn_train.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import attention_train as at  # noqa: E402

GEOMETRIES = [("configs[2]", 100, 196), ("configs[2]", 100, 784), ("configs[2]", 100, 3136),
              ("configs[3]", 300, 256), ("configs[3]", 300, 1024), ("configs[3]", 300, 4096)]
N, HEADS, C = 2, 8, 128


def torch_chain(q_c, q_s, k_c, k_p, v, mask, row_open):
    """CrossAttentionLayer.forward_post + attention_core between the projections and out_proj, as the parent runs them."""
    Q, S, hd = q_c.shape[0], k_c.shape[0], C // HEADS
    mask = mask & ~row_open
    q = torch.cat([q_c.view(Q, N, HEADS, hd), q_s.view(Q, N, HEADS, hd)], dim=3).view(Q, N, 2 * C)
    k = torch.cat([k_c.view(S, N, HEADS, hd), k_p.view(S, N, HEADS, hd)], dim=3).view(S, N, 2 * C)
    qh = (q * float(2 * hd) ** -0.5).reshape(Q, N, HEADS, 2 * hd).permute(1, 2, 0, 3)
    kh = k.reshape(S, N, HEADS, 2 * hd).permute(1, 2, 3, 0)
    vh = v.reshape(S, N, HEADS, hd).permute(1, 2, 0, 3)
    p = torch.softmax(torch.matmul(qh, kh).masked_fill(mask, float("-inf")), dim=-1)
    return torch.matmul(p, vh).permute(2, 0, 1, 3).reshape(Q, N, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_train.py needs the GPU: a CPU run times nothing")
    records = []
    for name, Q, S in GEOMETRIES:
        torch.manual_seed(0)
        ops = [torch.randn(T, N, C, device="cuda", requires_grad=True) for T in (Q, Q, S, S, S)]
        mask = torch.rand(N, 1, Q, S, device="cuda") < 0.5
        mask[N - 1, 0, Q // 2] = True
        row_open = mask.all(-1, keepdim=True)
        u = torch.randn(Q, N, C, device="cuda")
        assert at.covered(*ops, HEADS, mask, row_open)       # (the caller's speed rule, `supported`, is what this tool measures)

        def run(mode):
            out = at.cross_attention_train(*ops, HEADS, mask, row_open) if mode == "hip" else torch_chain(*ops, mask, row_open)
            out.backward(u)
            for t in ops:
                t.grad = None

        def captured(mode):
            """One forward + backward of `mode` as a HIP graph: its replays are timed without the host's launch cost."""
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    run(mode)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(mode)
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

        graphs = {mode: captured(mode) for mode in ("torch", "hip")}
        for rnd in range(a.rounds):
            for mode in ("torch", "hip"):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                eager = timed(lambda: run(mode))
                peak = torch.cuda.max_memory_allocated() - base
                replay = timed(graphs[mode].replay)
                rec = dict(config=name, N=N, heads=HEADS, Q=Q, S=S, round=rnd, path=mode, iters=a.iters,
                           fwd_bwd_ms=round(eager, 4), graph_replay_ms=round(replay, 4),
                           peak_mib_above_operands=round(peak / 2 ** 20, 2))
                records.append(rec)
                print("%s N=%d Q=%d S=%d round %d %-5s fwd+bwd eager %.4f ms  graph replay %.4f ms  peak above operands %.2f MiB" % (
                    name, N, Q, S, rnd, mode, eager, replay, rec["peak_mib_above_operands"]), flush=True)
        del graphs
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"note": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "records": records}, f, indent=1)


if __name__ == "__main__":
    main()

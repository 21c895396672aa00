"""Forward + backward of ONE self-attention of a training step, the HIP training path (self_attention_train.self_attention_train)
against the torch chain it replaces (the two operand adds, q * scale, matmul, softmax, matmul, the permutes and their autograd
backward), on fp32 operands: 2 images, 8 heads, 100 queries (configs[2]), 300 (configs[3]) and 512 (the kernels' limit).  Two
subjects per query count: the attention core on the five projections' outputs, and one whole SelfAttentionLayer (five
projections, core, out_proj, residual, LayerNorm) with its switch at "torch" and at "hip".  HIP events around `--iters`
repetitions after a warm-up, twice per arm: launched from Python per iteration (what an eager step pays) and as replays of a HIP
graph of one forward + backward (the device's share).  The two paths alternate `--rounds` times in one process so that the
spread between alternations can be read beside the difference; `summary` holds lowest - highest per arm.  One extra profiled
call per arm counts the kernel launches of a forward + backward; the peak of allocated memory above the operands is read from
the eager runs.  Prints one line per (subject, Q, round, path) and writes every figure to `--out` as JSON.

    python tools/bench_self_attn_train.py [--iters 50] [--rounds 3] [--out profiles/self_attn_train.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import self_attention_train as st  # noqa: E402
from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import SelfAttentionLayer  # noqa: E402

QUERIES = [("configs[2]", 100), ("configs[3]", 300), ("limit", 512)]
N, HEADS, C = 2, 8, 128


def torch_chain(q_c, q_p, k_c, k_p, v):
    """SelfAttentionLayer.forward_post + attention_core between the projections and out_proj, as the parent runs them."""
    Q, hd = q_c.shape[0], C // HEADS
    q = q_c + q_p
    k = k_c + k_p
    qh = (q * float(hd) ** -0.5).reshape(Q, N, HEADS, hd).permute(1, 2, 0, 3)
    kh = k.reshape(Q, N, HEADS, hd).permute(1, 2, 3, 0)
    vh = v.reshape(Q, N, HEADS, hd).permute(1, 2, 0, 3)
    p = torch.softmax(torch.matmul(qh, kh), dim=-1)
    return torch.matmul(p, vh).permute(2, 0, 1, 3).reshape(Q, N, C)


def launches_of(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_self_attn_train.py needs the GPU: a CPU run times nothing")
    records, summary = [], []

    def captured(run, mode):
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

    for name, Q in QUERIES:
        torch.manual_seed(0)
        ops = [torch.randn(Q, N, C, device="cuda", requires_grad=True) for _ in range(5)]
        u = torch.randn(Q, N, C, device="cuda")
        assert st.covered(*ops, HEADS)
        layer = SelfAttentionLayer(C, HEADS).cuda().train()
        tgt, qpos = torch.randn(Q, N, C, device="cuda", requires_grad=True), torch.randn(Q, N, C, device="cuda")

        def run_core(mode):
            out = st.self_attention_train(*ops, HEADS) if mode == "hip" else torch_chain(*ops)
            out.backward(u)
            for t in ops:
                t.grad = None

        def run_layer(mode):
            layer.self_attn_train = mode
            layer(tgt, query_pos=qpos).backward(u)
            tgt.grad = None
            layer.zero_grad(set_to_none=True)

        for subject, run in (("core", run_core), ("layer", run_layer)):
            graphs = {mode: captured(run, mode) for mode in ("torch", "hip")}
            launches = {mode: launches_of(lambda: run(mode)) for mode in ("torch", "hip")}
            for rnd in range(a.rounds):
                for mode in ("torch", "hip"):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    eager = timed(lambda: run(mode))
                    peak = torch.cuda.max_memory_allocated() - base
                    replay = timed(graphs[mode].replay)
                    rec = dict(config=name, subject=subject, N=N, heads=HEADS, Q=Q, round=rnd, path=mode, iters=a.iters,
                               fwd_bwd_ms=round(eager, 4), graph_replay_ms=round(replay, 4), launches=launches[mode],
                               peak_mib_above_operands=round(peak / 2 ** 20, 2))
                    records.append(rec)
                    print("%s %-5s N=%d Q=%d round %d %-5s fwd+bwd eager %.4f ms  graph replay %.4f ms  launches %d  "
                          "peak above operands %.2f MiB" % (name, subject, N, Q, rnd, mode, eager, replay, launches[mode],
                                                            rec["peak_mib_above_operands"]), flush=True)
            del graphs
            mine = [r for r in records if r["Q"] == Q and r["subject"] == subject]
            entry = dict(config=name, subject=subject, Q=Q)
            for mode in ("torch", "hip"):
                rs = [r for r in mine if r["path"] == mode]
                entry[mode] = {k: [min(r[k] for r in rs), max(r[k] for r in rs)] for k in ("fwd_bwd_ms", "graph_replay_ms")}
                entry[mode]["launches"] = launches[mode]
                entry[mode]["peak_mib_above_operands"] = max(r["peak_mib_above_operands"] for r in rs)
            summary.append(entry)
            print(json.dumps(entry), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"note": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "summary": summary,
                       "records": records}, f, indent=1)


if __name__ == "__main__":
    main()

"""ONE attention core of an fp32 evaluation forward, the forward-only HIP kernels (attention_eval.cross_attention /
self_attention) against the torch chain they replace as the parent commit runs it (cross: mask & ~row_open, the two per-head
concatenations, q * scale, matmul, masked_fill, softmax, matmul; self: the two adds, q * scale, matmul, softmax, matmul), under
no_grad on fp32 operands, 8 heads.  Cross: 100 queries at 256 / 1 024 / 4 096 keys and 300 queries at 374 / 1 452 / 5 655 keys
(the three levels of a 512^2 crop and of BBBC's 520 x 696), with a mask of the decoder's kind (half the entries dead, row_open =
mask.all(-1)); self: 100, 300 and 600 queries; batches of 1, 8 and 32 images.  Arms, alternating `--rounds` times in one process:
    torch, torch2   the chain twice -- the second is the control: what two runs of the same code differ by
    hip             the evaluation kernel (loads one key step ahead, no lse)
    train           the training forward (pct_*_attention_forward_f32): the same arithmetic, each step waiting for its own loads,
                    and lse written -- the evaluation kernel without its prefetch.  Self: up to its 512 queries
HIP events around `--iters` repetitions after a warm-up, launched from Python per iteration (eager) and as replays of a HIP graph
of one call (the device's share).  Peak memory above the operands is read per arm.  Prints one line per (shape, round, arm),
then per shape the medians and whether the kernel wins: its slowest round faster than the fastest round of torch and torch2.
Writes every figure to `--out` as JSON.

    python tools/bench_attention_eval.py [--iters 20] [--rounds 3] [--out profiles/attention_eval.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import attention_eval as ae  # noqa: E402
from pctrans_amd import attention_train as at  # noqa: E402
from pctrans_amd import self_attention_train as st  # noqa: E402

CROSS = [(100, 256), (100, 1024), (100, 4096), (300, 374), (300, 1452), (300, 5655)]
SELF = [100, 300, 600]
BATCHES = [1, 8, 32]
HEADS, C = 8, 128
# -Rpass-analysis=kernel-resource-usage of csrc/attention_eval.hip for gfx950 (hipcc of ROCm 7.0, the Makefile's flags)
RESOURCES = {"xat_eval_kernel": dict(vgprs=90, agprs=16, sgprs=46, scratch_bytes_per_lane=0, lds_bytes_per_block=5120,
                                     occupancy_waves_per_simd=4),
             "sat_eval_kernel": dict(vgprs=68, agprs=8, sgprs=34, scratch_bytes_per_lane=0, lds_bytes_per_block=5120,
                                     occupancy_waves_per_simd=6)}


def torch_cross(q_c, q_s, k_c, k_p, v, mask, row_open):
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


def torch_self(q_c, q_p, k_c, k_p, v):
    """SelfAttentionLayer.forward_post + attention_core between the projections and out_proj, as the parent runs them."""
    (Q, N, _), hd = q_c.shape, C // HEADS
    q, k = q_c + q_p, k_c + k_p
    qh = (q * float(hd) ** -0.5).reshape(Q, N, HEADS, hd).permute(1, 2, 0, 3)
    kh = k.reshape(Q, N, HEADS, hd).permute(1, 2, 3, 0)
    vh = v.reshape(Q, N, HEADS, hd).permute(1, 2, 0, 3)
    return torch.matmul(torch.softmax(torch.matmul(qh, kh), dim=-1), vh).permute(2, 0, 1, 3).reshape(Q, N, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_eval.py needs the GPU: a CPU run times nothing")
    torch.set_grad_enabled(False)
    records, summary = [], []

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

    def captured(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g

    shapes = [("cross", Q, S, N) for Q, S in CROSS for N in BATCHES] + [("self", Q, Q, N) for Q in SELF for N in BATCHES]
    for kind, Q, S, N in shapes:
        torch.manual_seed(0)
        ops = [torch.randn(T, N, C, device="cuda") for T in (Q, Q, S, S, S)]
        if kind == "cross":
            mask = torch.rand(N, 1, Q, S, device="cuda") < 0.5
            mask[N - 1, 0, Q // 2] = True
            row_open = mask.all(-1, keepdim=True)
            assert ae.covered(*ops, HEADS, mask, row_open)   # (the caller's speed rule, `supported`, is what this tool measures)
            arms = {"torch": lambda: torch_cross(*ops, mask, row_open), "torch2": lambda: torch_cross(*ops, mask, row_open),
                    "hip": lambda: ae.cross_attention(*ops, HEADS, mask, row_open),
                    "train": lambda: at.cross_attention_forward(*ops, HEADS, mask, row_open)}
            assert torch.equal(arms["hip"](), arms["train"]()[0])
        else:
            assert ae.covered(*ops, HEADS)
            arms = {"torch": lambda: torch_self(*ops), "torch2": lambda: torch_self(*ops),
                    "hip": lambda: ae.self_attention(*ops, HEADS)}
            if Q <= st.MAX_QUERIES:
                arms["train"] = lambda: st.self_attention_forward(*ops, HEADS)
                assert torch.equal(arms["hip"](), arms["train"]()[0])
        graphs = {name: captured(fn) for name, fn in arms.items()}
        replay = {name: [] for name in arms}
        eager = {name: [] for name in arms}
        peak = {}
        for rnd in range(a.rounds):
            for name, fn in arms.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                e = timed(fn)
                peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
                r = timed(graphs[name].replay)
                eager[name].append(e)
                replay[name].append(r)
                records.append(dict(kind=kind, N=N, heads=HEADS, Q=Q, S=S, round=rnd, path=name, iters=a.iters, eager_ms=round(e, 4),
                                    graph_replay_ms=round(r, 4), peak_mib_above_operands=peak[name]))
                print("%-5s N=%-2d Q=%-3d S=%-4d round %d %-6s eager %.4f ms  graph replay %.4f ms  peak above operands %.2f MiB" % (
                    kind, N, Q, S, rnd, name, e, r, peak[name]), flush=True)
        del graphs
        med = {name: statistics.median(v) for name, v in replay.items()}
        chain = replay["torch"] + replay["torch2"]
        row = dict(kind=kind, N=N, Q=Q, S=S, replay_ms_median={k: round(v, 4) for k, v in med.items()},
                   eager_ms_median={k: round(statistics.median(v), 4) for k, v in eager.items()},
                   hip_over_torch=round(med["hip"] / med["torch"], 3),
                   control_spread=round((max(chain) - min(chain)) / med["torch"], 3),
                   hip_over_train=round(med["hip"] / med["train"], 3) if "train" in med else None,
                   hip_wins=max(replay["hip"]) < min(chain), peak_mib_above_operands=peak)
        summary.append(row)
        print("== %-5s N=%-2d Q=%-3d S=%-4d  replay: hip / torch %.3f (control spread %.3f)  hip / train %s  wins %s  eager: hip %.4f torch %.4f"
              % (kind, N, Q, S, row["hip_over_torch"], row["control_spread"], row["hip_over_train"], row["hip_wins"],
                 row["eager_ms_median"]["hip"], row["eager_ms_median"]["torch"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"note": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "kernel_resources": RESOURCES,
                       "speed_rule": dict(max_keys=ae.MAX_KEYS, max_queries=ae.MAX_QUERIES, max_batch=ae.MAX_BATCH,
                                          long_keys=ae.LONG_KEYS, min_long_grid=ae.MIN_LONG_GRID,
                                          text="supported = covered, keys <= max_keys, queries <= max_queries, batch <= "
                                               "max_batch, and keys <= long_keys or ceil(Q / 16) * heads * batch >= min_long_grid"),
                       "prefetch": "hip_over_train of the summary: the evaluation kernel against the training forward, the same "
                                   "arithmetic with each key step waiting for its own loads (and lse written)",
                       "tile_skip": "not built", "summary": summary,
                       "records": records}, f, indent=1)


if __name__ == "__main__":
    main()

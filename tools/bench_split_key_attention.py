"""One CrossAttentionLayer forward in eval under bf16 autocast on the small grids of evaluation (batch 1 / 2 / 8, 100 and 300
queries, 8 heads; 1 024 and 4 096 keys of padded 512 x 512 images, 1 452 / 1 936 / 4 221 / 5 655 keys of unpadded ones): today's
route -- `split_keys = "torch"` with `ragged_keys` as it is by default, i.e. the aligned split-operand kernel on multiples of 64
keys and two concatenations, V^T by baddbmm and the generic kernel elsewhere -- against the split-key route (`split_keys = "hip"`),
with a mask of the decoder's kind (half the entries dead, two fully masked rows, memory_row_open = mask.all(-1)).  HIP events
around a window of repetitions after a warm-up.  Three things per shape, each with the arms today / split keys / today again
alternating `--rounds` times in one process (the second "today" is the control: the spread of one route against itself):
  core   the cores alone between the projections and out_proj, the split-key core at every candidate split count (`--splits`);
  layer  the eager layer, with the plan forced to the candidate whose median core time is lowest (host-bound at these sizes);
  graph  the same two layer forwards replayed from a HIP graph, where device time is what counts.
Prints one line per (shape, round) and writes every figure to `--out` as JSON with, per shape and measure, the control's spread
and whether the split-key arm is faster by more than it (`summarise`).  `plan`: what split_key_attention.plan gives the shape with
the shipped constants.

    python tools/bench_split_key_attention.py [--rounds 5] [--window-ms 100] [--out profiles/split_key_attention.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import fused_ops, ragged_attention, split_key_attention  # noqa: E402
from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer  # noqa: E402

KEYS = (1024, 4096, 1452, 1936, 4221, 5655)
QUERIES = (100, 300)
BATCHES = (1, 2, 8)
SPLITS = (2, 4, 8, 16)
HEADS, C = 8, 128


def cat_heads(a, b):
    T, N, _ = a.shape
    return torch.cat([a.view(T, N, HEADS, 16), b.view(T, N, HEADS, 16)], dim=3).view(T, N, 2 * C)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def summarise(today, arm):
    """The control's spread = max - min over every window of today's route (both arms, all rounds); `faster` = today's median
    minus the arm's median exceeds that spread."""
    spread = max(today) - min(today)
    return dict(control_spread_ms=round(spread, 4), median_ms=dict(today=round(median(today), 4), split=round(median(arm), 4)),
                ratio_of_medians=round(median(arm) / median(today), 3), faster=bool(median(today) - median(arm) > spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--keys", type=int, nargs="*", default=list(KEYS))
    ap.add_argument("--queries", type=int, nargs="*", default=list(QUERIES))
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--splits", type=int, nargs="*", default=list(SPLITS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_split_key_attention.py needs the GPU: a CPU run times nothing")

    def timed(fn):
        """ms per call over a window of at least --window-ms (at least 10, at most 20 000 calls), after a warm-up."""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        iters = int(min(20000, max(10, a.window_ms / max(e0.elapsed_time(e1) / 5, 1e-3))))
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def graphed(fn):
        """fn captured once in a HIP graph -> the replay."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return graph.replay

    torch.manual_seed(0)
    layer = CrossAttentionLayer(C, HEADS).cuda().eval()
    assert layer.ragged_keys == "torch", "today's route is measured with ragged_keys at its default"
    shipped_plan = split_key_attention.plan
    records = []
    for N in a.batches:
        for Q in a.queries:
            for S in a.keys:
                g = torch.Generator(device="cuda").manual_seed(S + Q + N)
                rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
                mask = torch.rand(N, 1, Q, S, device="cuda", generator=g) < 0.5
                mask[0, 0, Q // 2] = True
                mask[N - 1, 0, Q - 1] = True
                row_open = mask.all(-1, keepdim=True)
                kw = dict(tgt=rnd(Q, N, C), memory=rnd(S, N, C), memory_mask=mask, pos=rnd(S, N, C), query_pos=rnd(Q, N, C),
                          query_sine_embed=rnd(Q, N, 2 * C), is_first=False, memory_row_open=row_open)
                qc, qp, kc, kp = (rnd(T, N, C).bfloat16() for T in (Q, Q, S, S))
                mem16 = kw["memory"].bfloat16()
                w16, b16 = layer.ca_v_proj.weight.detach().bfloat16(), layer.ca_v_proj.bias.detach().bfloat16()
                assert split_key_attention.covered(qc, kc, kp, HEADS, mask)
                aligned = bool(fused_ops.cross_attention_supported(qc, kc, kp, HEADS, mask))
                candidates = [s for s in a.splits if 2 <= s <= min(16, split_key_attention.chunks(S))]

                def run_layer(switch):
                    layer.split_keys = switch
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                        return layer(**kw)

                def core_today():
                    if aligned:
                        return fused_ops.cross_attention(qc, qp, kc, kp, F.linear(mem16, w16, b16), HEADS, mask, row_open=row_open)
                    m = mask & ~row_open
                    v_t = torch.baddbmm(b16.view(1, C, 1), w16.unsqueeze(0).expand(N, C, C), mem16.permute(1, 2, 0))
                    return fused_ops.masked_attention(cat_heads(qc, qp), cat_heads(kc, kp), None, HEADS, m, v_t=v_t)

                def core_split(splits):
                    return split_key_attention.cross_attention(qc, qp, kc, kp, F.linear(mem16, w16, b16), HEADS, mask,
                                                               row_open=row_open, splits=splits)

                for s in candidates:               # the cores compute the same thing (V from different GEMMs: bf16 tolerance)
                    d = (core_today().float() - core_split(s).float()).abs()
                    assert torch.isfinite(d).all() and float(d.max()) < 0.1, (s, float(d.max()))
                # ---- cores
                core = dict(today=[], today_again=[], split={s: [] for s in candidates})
                for r in range(a.rounds):
                    core["today"].append(round(timed(core_today), 5))
                    for s in candidates:
                        core["split"][s].append(round(timed(lambda: core_split(s)), 5))
                    core["today_again"].append(round(timed(core_today), 5))
                    print("N=%d Q=%3d S=%4d round %d core ms today %.4f | %s | today again %.4f" % (
                        N, Q, S, r, core["today"][-1], " ".join("x%d %.4f" % (s, core["split"][s][-1]) for s in candidates),
                        core["today_again"][-1]), flush=True)
                today = core["today"] + core["today_again"]
                best = min(candidates, key=lambda s: median(core["split"][s]))
                rec = dict(N=N, Q=Q, S=S, heads=HEADS, chunks=split_key_attention.chunks(S), today="aligned" if aligned else "generic",
                           workgroups=ragged_attention.workgroups(Q, N, HEADS), rounds=a.rounds, plan=shipped_plan(Q, N, HEADS, S),
                           core_ms=core, core={s: summarise(today, core["split"][s]) for s in candidates}, best_splits=best)
                # ---- the layer, eager and replayed, with the plan forced to the best candidate
                split_key_attention.plan = lambda *_: best
                try:
                    assert split_key_attention.supported(qc, kc, kp, HEADS, mask)
                    replay = {sw: graphed(lambda sw=sw: run_layer(sw)) for sw in ("torch", "hip")}
                    arms = (("today", lambda: run_layer("torch"), replay["torch"]), ("split", lambda: run_layer("hip"), replay["hip"]),
                            ("today_again", lambda: run_layer("torch"), replay["torch"]))
                    t = {name: dict(layer=[], graph=[]) for name, _, _ in arms}
                    for r in range(a.rounds):
                        for name, eager, rep in arms:
                            t[name]["layer"].append(round(timed(eager), 5))
                            t[name]["graph"].append(round(timed(rep), 5))
                        print("N=%d Q=%3d S=%4d round %d x%d  layer ms today %.4f split %.4f today again %.4f | graph ms %.4f %.4f %.4f" % (
                            N, Q, S, r, best, t["today"]["layer"][-1], t["split"]["layer"][-1], t["today_again"]["layer"][-1],
                            t["today"]["graph"][-1], t["split"]["graph"][-1], t["today_again"]["graph"][-1]), flush=True)
                finally:
                    split_key_attention.plan = shipped_plan
                    layer.split_keys = "torch"
                rec["layer_ms"] = t
                for what in ("layer", "graph"):
                    rec[what] = summarise(t["today"][what] + t["today_again"][what], t["split"][what])
                records.append(rec)
                del kw, mask, row_open, qc, qp, kc, kp, mem16, replay, arms
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"note": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "window_ms": a.window_ms,
                       "constants": dict(MAX_SPLITS=split_key_attention.MAX_SPLITS, MIN_CHUNKS=split_key_attention.MIN_CHUNKS,
                                         TARGET_WORKGROUPS=split_key_attention.TARGET_WORKGROUPS),
                       "records": records}, f, indent=1)


if __name__ == "__main__":
    main()

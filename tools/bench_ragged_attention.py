"""One CrossAttentionLayer forward in eval under bf16 autocast at the key counts of the unpadded evaluation images (520 x 696:
374 / 1 452 / 5 655; 530 x 500: 272 / 4 221; 704 x 704: 484 / 1 936), today's route (two per-head concatenations, V^T by baddbmm,
the generic kernel) against the ragged split-operand kernel (`ragged_keys = "hip"`), 100 and 300 queries, batch 2 / 8 / 128, with
a mask of the decoder's kind (half the entries dead, two fully masked rows, memory_row_open = mask.all(-1)).  HIP events around a
window of repetitions after a warm-up.  Three arms alternate `--rounds` times in one process: parent, ragged, and the parent
again -- the control: the spread of one route against itself, to read beside the difference.  Separately the cores alone between
the projections and out_proj: V projection + mask pad + ragged kernel, against cat + cat + mask & ~row_open + V^T baddbmm +
generic kernel.  Prints one line per (shape, round) and writes every figure to `--out` as JSON with, per shape and measure, the
control's spread and whether the ragged arm is faster by more than it (`summarise`).  `routed`: whether
ragged_attention.supported sends the shape to the kernel -- where it does not, the layer's "ragged" arm runs today's route and
only the core shows the kernel.

    python tools/bench_ragged_attention.py [--rounds 3] [--window-ms 60] [--out profiles/ragged_attention.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import fused_ops, ragged_attention  # noqa: E402
from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer  # noqa: E402

KEYS = (374, 1452, 5655, 272, 4221, 484, 1936)
QUERIES = (100, 300)
BATCHES = (2, 8, 128)
HEADS, C = 8, 128


def cat_heads(a, b):
    T, N, _ = a.shape
    return torch.cat([a.view(T, N, HEADS, 16), b.view(T, N, HEADS, 16)], dim=3).view(T, N, 2 * C)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def summarise(rec):
    """Per measure (layer, core): the control's spread = max - min over every window of the parent route (both arms, all rounds);
    `faster` = the parent's median minus the ragged route's median exceeds that spread; `faster_every_window` = even the parent's
    best window minus the ragged route's worst does (one disturbed window of either arm undoes this one)."""
    for what in ("layer", "core"):
        par = rec["ms"]["parent"][what] + rec["ms"]["parent_again"][what]
        rag = rec["ms"]["ragged"][what]
        spread = max(par) - min(par)
        rec[what + "_control_spread_ms"] = round(spread, 4)
        rec[what + "_median_ms"] = dict(parent=round(median(par), 4), ragged=round(median(rag), 4))
        rec[what + "_ratio_of_medians"] = round(median(rag) / median(par), 3)
        rec[what + "_faster"] = bool(median(par) - median(rag) > spread)
        rec[what + "_faster_every_window"] = bool(min(par) - max(rag) > spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=60.0)
    ap.add_argument("--keys", type=int, nargs="*", default=list(KEYS))
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_attention.py needs the GPU: a CPU run times nothing")

    def timed(fn):
        """ms per call over a window of at least --window-ms (at least 10, at most 400 calls), after a warm-up."""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        iters = int(min(400, max(10, a.window_ms / max(e0.elapsed_time(e1), 1e-3))))
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    torch.manual_seed(0)
    layer = CrossAttentionLayer(C, HEADS).cuda().eval()
    records = []
    for N in a.batches:
        for Q in QUERIES:
            for S in a.keys:
                g = torch.Generator(device="cuda").manual_seed(S + Q + N)
                rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
                try:
                    mask = torch.rand(N, 1, Q, S, device="cuda", generator=g) < 0.5
                    mask[0, 0, Q // 2] = True
                    mask[N - 1, 0, Q - 1] = True
                    row_open = mask.all(-1, keepdim=True)
                    kw = dict(tgt=rnd(Q, N, C), memory=rnd(S, N, C), memory_mask=mask, pos=rnd(S, N, C), query_pos=rnd(Q, N, C),
                              query_sine_embed=rnd(Q, N, 2 * C), is_first=False, memory_row_open=row_open)
                    qc, qp, kc, kp = (rnd(T, N, C).bfloat16() for T in (Q, Q, S, S))
                except torch.OutOfMemoryError:
                    print("N=%d Q=%d S=%d does not fit: dropped" % (N, Q, S), flush=True)
                    continue
                mem16 = kw["memory"].bfloat16()
                w16, b16 = layer.ca_v_proj.weight.detach().bfloat16(), layer.ca_v_proj.bias.detach().bfloat16()
                assert ragged_attention.covered(qc, kc, kp, HEADS, mask)       # (the caller's speed rule, `supported`, is what this tool measures)

                def run_layer(switch):
                    layer.ragged_keys = switch
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                        return layer(**kw)

                def core_parent():
                    m = mask & ~row_open
                    v_t = torch.baddbmm(b16.view(1, C, 1), w16.unsqueeze(0).expand(N, C, C), mem16.permute(1, 2, 0))
                    return fused_ops.masked_attention(cat_heads(qc, qp), cat_heads(kc, kp), None, HEADS, m, v_t=v_t)

                def core_ragged():
                    return ragged_attention.cross_attention(qc, qp, kc, kp, F.linear(mem16, w16, b16), HEADS, mask, row_open=row_open)

                # the two cores compute the same thing (V from different GEMMs: bf16 tolerance, not bits)
                d = (core_parent().float() - core_ragged().float()).abs()
                assert torch.isfinite(d).all() and float(d.max()) < 0.1, float(d.max())
                arms = (("parent", lambda: run_layer("torch"), core_parent), ("ragged", lambda: run_layer("hip"), core_ragged),
                        ("parent_again", lambda: run_layer("torch"), core_parent))
                t = {name: dict(layer=[], core=[]) for name, _, _ in arms}
                for r in range(a.rounds):
                    for name, lay, core in arms:
                        t[name]["layer"].append(round(timed(lay), 4))
                        t[name]["core"].append(round(timed(core), 4))
                    print("N=%3d Q=%3d S=%4d round %d  layer ms parent %.4f ragged %.4f parent again %.4f | core ms %.4f %.4f %.4f" % (
                        N, Q, S, r, t["parent"]["layer"][-1], t["ragged"]["layer"][-1], t["parent_again"]["layer"][-1],
                        t["parent"]["core"][-1], t["ragged"]["core"][-1], t["parent_again"]["core"][-1]), flush=True)
                rec = dict(N=N, Q=Q, S=S, heads=HEADS, workgroups=ragged_attention.workgroups(Q, N, HEADS), rounds=a.rounds,
                           routed=bool(ragged_attention.supported(qc, kc, kp, HEADS, mask)), ms=t)
                summarise(rec)
                records.append(rec)
                del kw, mask, row_open, qc, qp, kc, kp, mem16
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"note": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "window_ms": a.window_ms,
                       "records": records}, f, indent=1)


if __name__ == "__main__":
    main()

"""Forward + backward of the pixel decoder's MSDeformAttn in a training step, `train_front = "hip"` (the fused forward with the device
backward of pctrans_amd/msda_train.py) against `train_front = "torch"` (the parent path: softmax, location arithmetic,
MSDeformAttnFunction and torch's backward of each), on ONE MSDeformAttn module and on the six-layer encoder (dropout 0, train mode)
at the encoder geometries of configs[2] (448^2 crops: 56^2 + 28^2 + 14^2 = 4 116 tokens) and configs[3] (512^2 crops: 64^2 + 32^2 +
16^2 = 5 376 tokens), 2 images, 128 channels, 8 heads, 4 points.  HIP events around `--iters` repetitions after a warm-up, twice per
arm: launched from Python per iteration (what an eager step pays) and as replays of a HIP graph of one forward + backward (the
device's share).  The two paths alternate `--rounds` times in one process so that the spread between alternations can be read beside
the difference.  Also per arm: kernel launches of one forward + backward (torch.profiler, divided by the layer count) and the peak
of allocated memory above the operands.  Prints one line per (geometry, subject, round, path) and writes every figure to `--out`.

    python tools/bench_msda_train.py [--iters 30] [--rounds 3] [--out profiles/msda_train.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import _lib  # noqa: E402
from pctrans_amd.pixel_decoder.msdeformattn import (MSDeformAttnTransformerEncoder,  # noqa: E402
                                                    MSDeformAttnTransformerEncoderLayer)
from pctrans_amd.pixel_decoder.ops.modules import MSDeformAttn  # noqa: E402

GEOMETRIES = [("configs[2]", [(56, 56), (28, 28), (14, 14)]), ("configs[3]", [(64, 64), (32, 32), (16, 16)])]
N, C, HEADS, POINTS, FFN, LAYERS = 2, 128, 8, 4, 1024, 6


def set_front(model, front):
    for m in model.modules():
        if isinstance(m, MSDeformAttn):
            m.train_front = front


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_msda_train.py needs the GPU: a CPU run times nothing")
    _lib.prepare_device(torch.device("cuda", torch.cuda.current_device()))
    records = []
    for name, shapes in GEOMETRIES:
        L, S = len(shapes), sum(h * w for h, w in shapes)
        torch.manual_seed(0)
        ss = torch.as_tensor(shapes, dtype=torch.long, device="cuda")
        starts = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
        ones = torch.ones((N, L, 2), device="cuda")
        ref = MSDeformAttnTransformerEncoder.get_reference_points(shapes, ones[:1], "cuda").expand(N, -1, -1, -1)
        src = torch.randn(N, S, C, device="cuda", requires_grad=True)
        pos = torch.randn(1, S, C, device="cuda")
        u = torch.randn(N, S, C, device="cuda")
        module = MSDeformAttn(C, L, HEADS, POINTS)
        encoder = MSDeformAttnTransformerEncoder(MSDeformAttnTransformerEncoderLayer(C, FFN, 0.0, "relu", L, HEADS, POINTS), LAYERS)
        with torch.no_grad():                  # offsets and weights as a trained model has them, not the all-zero initial Linears
            for m in [module] + [layer.self_attn for layer in encoder.layers]:
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.1)
        module, encoder = module.cuda().train(), encoder.cuda().train()
        subjects = {
            "module": (module, 1, lambda: module(src + pos, ref, src, ss, starts)),
            "encoder6": (encoder, LAYERS, lambda: encoder(src, ss, starts, ones, pos, None, reference_points=ref)),
        }
        for subject, (model, layers, fwd) in subjects.items():
            def run():
                fwd().backward(u)
                src.grad = None
                for p in model.parameters():
                    p.grad = None

            def captured():
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(3):
                        run()
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    run()
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

            def launches():
                """device activities (kernels, and the copies and fills among them) of one forward + backward"""
                run()
                torch.cuda.synchronize()
                with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                    run()
                    torch.cuda.synchronize()
                return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)

            graphs, counts = {}, {}
            for mode in ("torch", "hip"):
                set_front(model, mode)
                counts[mode] = launches()
                graphs[mode] = captured()
            for rnd in range(a.rounds):
                for mode in ("torch", "hip"):
                    set_front(model, mode)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    eager = timed(run)
                    peak = torch.cuda.max_memory_allocated() - base
                    replay = timed(graphs[mode].replay)
                    rec = dict(config=name, subject=subject, N=N, S=S, levels=L, heads=HEADS, points=POINTS, round=rnd, path=mode,
                               iters=a.iters, fwd_bwd_ms=round(eager, 4), graph_replay_ms=round(replay, 4),
                               launches_per_layer=round(counts[mode] / layers, 1),
                               peak_mib_above_operands=round(peak / 2 ** 20, 2))
                    records.append(rec)
                    print("%s %-8s round %d %-5s fwd+bwd eager %.4f ms  graph replay %.4f ms  launches / layer %.1f  peak above "
                          "operands %.2f MiB" % (name, subject, rnd, mode, eager, replay, rec["launches_per_layer"],
                                                 rec["peak_mib_above_operands"]), flush=True)
            del graphs
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"note": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "records": records}, f, indent=1)


if __name__ == "__main__":
    main()

"""Forward + backward of ONE dynamic mask head, the HIP training path (dynamic_mask_head_train) against the module's torch
formulation, at the geometry of configs[2] (2 x 100 queries, 112 x 112 mask features) and configs[3] (2 x 300 queries,
128 x 128).  HIP events around `--iters` repetitions after a warm-up; the two paths alternate `--rounds` times in one process
so that the spread between alternations can be read beside the difference.  Prints one line per (geometry, round, path).

    python tools/bench_dmh_train.py [--iters 20] [--rounds 3]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec  # noqa: E402

GEOMETRIES = {"configs[2]": (2, 100, 112, 112, (28, 28)), "configs[3]": (2, 300, 128, 128, (32, 32))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    for name, (N, Q, H, W, target) in GEOMETRIES.items():
        torch.manual_seed(0)
        d = dec.MultiScaleMaskedTransformerDecoder(
            128, True, hidden_dim=128, num_queries=Q, nheads=8, dim_feedforward=256, dec_layers=1, pre_norm=False,
            mask_dim=16, enforce_input_project=False, points_num=1, sem_loss_on=True, norm="BN", rel_coord=True).cuda()
        mf = torch.randn(N, 16, H, W, device="cuda", requires_grad=True)
        ref = torch.rand(Q, N, 2, device="cuda", requires_grad=True)
        prm = (torch.randn(Q, N, 233, device="cuda") * 0.1).requires_grad_(True)
        u = torch.randn(N, Q, 2 * H, 2 * W, device="cuda")

        def run(mode):
            d.dmh_train = mode
            up, _ = d.dynamic_mask_with_coords(mf, ref, prm, 4, True, target)
            up.backward(u)
            mf.grad = ref.grad = prm.grad = None

        for rnd in range(a.rounds):
            for mode in ("torch", "hip"):
                for _ in range(3):
                    run(mode)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    run(mode)
                e1.record()
                torch.cuda.synchronize()
                print("%s N=%d Q=%d %dx%d round %d %-5s fwd+bwd %.3f ms  peak %.0f MiB" % (
                    name, N, Q, H, W, rnd, mode, e0.elapsed_time(e1) / a.iters, torch.cuda.max_memory_allocated() / 2 ** 20),
                    flush=True)


if __name__ == "__main__":
    main()

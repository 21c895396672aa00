"""One FPN level of the pixel decoder (pixel_decoder/msdeformattn.py, the loop behind the encoder) as the torch statements and
as the device path (fused_ops.fpn_stage, csrc/fpn_stage.hip), alternating in one process: three rounds of each, the median of
the rounds' mean time per call.  enc is the channels-last view of token rows, as in the decoder.  Prints one JSON line.

    python tools/bench_fpn.py [--batch 128] [--cin 256] [--size 64] [--norm BN] [--iters 20]"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--cin", type=int, default=256)
    ap.add_argument("--size", type=int, default=64, help="height = width of the output map")
    ap.add_argument("--norm", default="BN", choices=["", "BN", "FrozenBN"])
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from pctrans_amd import fused_ops
    from pctrans_amd.layers import Conv2d, get_norm
    torch.manual_seed(0)
    n, h = a.batch, a.size
    lat = Conv2d(a.cin, 128, kernel_size=1, bias=a.norm == "", norm=get_norm(a.norm, 128)).cuda().eval()
    outc = Conv2d(128, 128, kernel_size=3, stride=1, padding=1, bias=a.norm == "", norm=get_norm(a.norm, 128),
                  activation=F.relu).cuda().eval()
    x = torch.randn(n, a.cin, 2 * h, 2 * h, device="cuda")
    rows = h * h // 4 + h * h // 16                                   # the two coarser levels in front, as with res3 .. res5
    tokens = torch.randn(n, rows + h * h, 128, device="cuda")
    enc = tokens[:, rows:].transpose(1, 2).reshape(n, 128, h, h)

    def torch_chain():
        cur_fpn = lat(x)
        y = enc + F.interpolate(cur_fpn, size=enc.shape[-2:], mode="bilinear", align_corners=False)
        return outc(y)

    def hip():
        return fused_ops.fpn_stage(x, enc, lat, outc)

    def time_of(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    with torch.no_grad():
        assert fused_ops.fpn_stage_supported(x, enc, lat, outc)
        for fn in (torch_chain, hip):                                # warm-up: solver search, workspaces, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        err = float((hip() - torch_chain()).abs().max())
        ms = {"torch": [], "hip": []}
        for _ in range(3):
            ms["torch"].append(time_of(torch_chain))
            ms["hip"].append(time_of(hip))
    print(json.dumps({"batch": n, "cin": a.cin, "size": h, "norm": a.norm, "iters": a.iters,
                      "torch_ms": ms["torch"], "hip_ms": ms["hip"], "torch_ms_median": statistics.median(ms["torch"]),
                      "hip_ms_median": statistics.median(ms["hip"]), "max_abs_diff": err}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Kept measurement of the two TRAINING configurations of BASELINE.json on one MI355X (a record for profiles/, not the judged
metric): one optimiser step of the whole model -- ResNet-50 backbone, pixel decoder, transformer decoder with query contrast,
matcher on the device, criterion with deep supervision, backward, AdamW -- at the reference's per-GPU batch.

    configs[2]  configs/CVPPP/CVPPP-PCTrans.yaml: 2 x 448^2 crops (dataset_CVPPP.py:106), 3 encoder levels, 100 queries
    configs[3]  configs/BBBC/BBBC-PCTrans.yaml:   2 x 512^2 crops (dataset_BBBC.py:111), 3 encoder levels, 300 queries

Reported per configuration: wall time per step without any profiler (HIP events around whole steps + host clock), kernel
launches and device->host copies per step (torch profiler on ONE extra step, its own timing discarded), summed device time
of that step's kernels.  MIOpen's naive solvers are excluded from the search as in bench.py.  Synthetic data."""
import json
import os
import sys
import time

os.environ.setdefault("MIOPEN_FIND_MODE", "1")
os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", "0")
os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_BWD", "0")
os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_WRW", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pctrans_amd.arch import maskformer as mfm  # noqa: E402
from pctrans_amd.arch.resnet import ResNet  # noqa: E402
from pctrans_amd.config import get_cfg  # noqa: E402
import train_switches  # noqa: E402  (tests/)

CONFIGS = {
    "configs[2] CVPPP-PCTrans.yaml": dict(dataset="CVPPP", N=2, H=448, W=448, Q=100, G=20),
    "configs[3] BBBC-PCTrans.yaml": dict(dataset="BBBC", N=2, H=512, W=512, Q=300, G=60),
}


def build(c):
    import random
    random.seed(0)
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=c["Q"], norm="BN", sem_norm="BN", dataset=c["dataset"])
    model = mfm.MaskFormer(**mfm.MaskFormer.from_config(cfg, ResNet(50, 3, norm="BN"))).cuda().train()
    N, H, W, G = c["N"], c["H"], c["W"], c["G"]
    vol = torch.randn(N, 3, H, W, device="cuda")
    g = torch.Generator().manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    targets = []
    for b in range(N):
        cy, cx = torch.randint(20, H - 20, (G,), generator=g), torch.randint(20, W - 20, (G,), generator=g)
        r = torch.randint(6, 16, (G,), generator=g)
        masks = torch.stack([(((yy - int(y)) ** 2 + (xx - int(x)) ** 2) <= int(q) ** 2).float() for y, x, q in zip(cy, cx, r)])
        centers = torch.stack([cx.float() / W, cy.float() / H], -1).view(G, 1, 2).cuda()
        targets.append({"masks": masks, "labels": torch.ones(G, dtype=torch.long, device="cuda"),
                        "fg_masks": (masks.sum(0) > 0).float(), "center_points": centers})
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.05)
    for s in train_switches.SWITCHES:             # the switches' table of the tests: one place says how each is set
        if s["config_key"] is not None and c.get(s["config_key"]):
            train_switches.set_switch(model, s["name"], True)
    if c.get("hip_msda_train"):                   # hand-written like the graph flags: not (yet) in the tests' table
        from pctrans_amd.pixel_decoder.ops.modules import MSDeformAttn
        for m in model.modules():
            if isinstance(m, MSDeformAttn):
                m.train_front = "hip"
    if c.get("graph_decoder"):
        from pctrans_amd.graph import graph_training_decoder
        graph_training_decoder(model, vol)
    if c.get("graph_front"):
        from pctrans_amd.graph import graph_training_front
        graph_training_front(model, vol)

    def step():
        losses = model(vol, targets, True)
        total = sum(v for v in losses.values() if torch.is_tensor(v))
        opt.zero_grad(set_to_none=True)
        total.backward()
        opt.step()
        return total
    return model, step


def selected_configs(argv):
    configs = dict(CONFIGS)
    if "--graph-front" in argv:
        configs.update({k + " + graphed backbone / pixel decoder": dict(v, graph_front=True) for k, v in CONFIGS.items()})
    if "--graph-decoder" in argv:
        configs.update({k + " + graphed decoder core": dict(v, graph_decoder=True) for k, v in CONFIGS.items()})
    if "--hip-msda-train" in argv:          # every selected config again with the encoder's fused MSDeformAttn front-end and its backward
        configs.update({k + " + HIP MSDeformAttn front": dict(v, hip_msda_train=True) for k, v in list(configs.items())})
    if "--hip-mask-head" in argv:           # every selected config again with the mask head's HIP training path
        configs.update({k + " + HIP mask head": dict(v, hip_mask_head=True) for k, v in list(configs.items())})
    if "--hip-point-loss" in argv:          # and again with the point-sampled losses and the matcher's gather on the device
        configs.update({k + " + HIP point loss": dict(v, hip_point_loss=True) for k, v in list(configs.items())})
    if "--hip-point-select" in argv:        # and the point-loss configs again with the uncertain points chosen by the kernel
        configs.update({k + " + HIP point select": dict(v, hip_point_select=True) for k, v in list(configs.items())
                        if v.get("hip_point_loss")})
    if "--hip-match-cost" in argv:          # and every selected config again with the matcher's cost matrices from the fused kernel
        configs.update({k + " + HIP match cost": dict(v, hip_match_cost=True) for k, v in list(configs.items())})
    if "--batched-heads" in argv:           # and the configs with all three on the device again with every head in one launch
        configs.update({k + " + batched heads": dict(v, batched_heads=True) for k, v in list(configs.items())
                        if v.get("hip_point_loss") and v.get("hip_point_select") and v.get("hip_match_cost")})
    if "--hip-emb-loss" in argv:            # and every selected config again with the pixel-embedding loss on the device
        configs.update({k + " + HIP embedding loss": dict(v, hip_emb_loss=True) for k, v in list(configs.items())})
    if "--hip-attn-train" in argv:          # and every selected config again with the cross-attention's HIP training path
        configs.update({k + " + HIP attention": dict(v, hip_attn_train=True) for k, v in list(configs.items())})
    if "--hip-reid-dice" in argv:           # and every selected config again with the re-id mask dice rows from the HIP kernels
        configs.update({k + " + HIP re-id dice": dict(v, hip_reid_dice=True) for k, v in list(configs.items())})
    return configs


def record_one(name, c):
    model, step = build(c)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    steps = 10
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        total = step()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    ev = e0.elapsed_time(e1) / steps
    peak_mib = round(torch.cuda.max_memory_allocated() / 2 ** 20)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    launches, dev_us, d2h = 0, 0.0, 0
    top = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            launches += 1
            dev_us += e.device_time if hasattr(e, "device_time") else e.cuda_time
            key = e.name[:60]
            top[key] = top.get(key, 0.0) + (e.device_time if hasattr(e, "device_time") else e.cuda_time)
            if "Memcpy DtoH" in e.name or "DtoH" in e.name:
                d2h += 1
    rec = dict(c, max_memory_allocated_mib=peak_mib, step_ms_wall=round(wall, 2), step_ms_hip_events=round(ev, 2), kernel_launches_per_step=launches,
               device_to_host_copies_per_step=d2h, device_ms_sum_of_kernels=round(dev_us / 1e3, 2),
               loss=float(total.detach()), samples_per_s_per_gpu=round(c["N"] / (wall / 1e3), 1),
               top_device_time_ms={k: round(v / 1e3, 2) for k, v in sorted(top.items(), key=lambda kv: -kv[1])[:12]})
    if c.get("graph_front") or c.get("graph_decoder"):
        from pctrans_amd.graph import release_training_graphs
        release_training_graphs(model)                # graphs destroyed now, not by a later collector pass inside a replay
    return rec


def main():
    """Every configuration is recorded in a child process of its own: a step's peak memory and the HIP runtime's graph
    bookkeeping then owe nothing to the configurations recorded before it (one process that captured, released and captured
    again across configurations ended in a segmentation fault at its third capture; graph.release_training_graphs documents
    the same fragility).  `--rounds R` repeats the whole list R times, so that flag-off and flag-on steps alternate on one
    machine; a child that fails ends the recording there with its exit status."""
    import subprocess
    known = ["--graph-front", "--graph-decoder", "--hip-msda-train"] + [s["flag"] for s in train_switches.SWITCHES if s["flag"] is not None]
    flags = [a for a in sys.argv[1:] if a in known]
    configs = selected_configs(flags)
    if "--only" in sys.argv:
        name = sys.argv[sys.argv.index("--only") + 1]
        rec = record_one(name, configs[name])
        rec["device"] = torch.cuda.get_device_name(0)
        print("REC " + json.dumps(rec), flush=True)
        return 0
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 1
    out = {"note": __doc__.split("\n\n")[0], "rounds": rounds, "configs": {name: [] for name in configs}}
    for rnd in range(rounds):
        for name in configs:
            child = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), "--only", name] + flags,
                                   stdout=subprocess.PIPE, text=True, timeout=600)
            recs = [ln[4:] for ln in child.stdout.splitlines() if ln.startswith("REC ")]
            if child.returncode != 0 or not recs:
                print("round %d, %s: child ended with status %d" % (rnd, name, child.returncode), flush=True)
                print("JSON " + json.dumps(out))
                return child.returncode or 1
            out["configs"][name].append(json.loads(recs[-1]))
            print(rnd, name, recs[-1], flush=True)
    print("JSON " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Times the preparation of the instance targets -- pctrans_amd.targets.prepare_instance_targets, what the reference trainer runs
before every training and validation step -- at the two training shapes, two modes alternating in one process:

  torch   the trainer's host loop as the trainer runs it: CPU label map in, torch.unique / `==` / nonzero / mean per instance on
          the host, the [G, H, W] bool stack copied to the device from pageable memory                        (mode = "torch")
  hip     the CPU label map copied to the device once, pct_instance_targets_census, one small device -> host copy,
          pct_instance_targets_planes                                                                         (mode = "hip")

Shapes: configs[2] (N = 2, 448 x 448, 20 instances per image) and configs[3] (N = 2, 512 x 512, 60 instances per image), int64
label maps as the loader delivers them.  Both modes are timed with the host's wall clock around a call that ends in a device
synchronise; the device mode also with HIP events, and its two kernel sequences with the events of pctrans_amd/_timing.py, from
which the planes kernel's write rate follows (sum G * H * W * (1 + 4) bytes of masks and planes plus N * H * W of foreground).
Per shape it also times the first Point_HungarianMatcher._match_target_planes + SetCriterion._hip_target_planes pair of a step
-- the consumers' torch.cat(masks).float() -- on a plain list, and on a TargetList that hands its planes over.
One warm-up round, then `--rounds` rounds of `--repeats` calls with the modes alternating; per round the median, and over the
rounds lowest - highest.

    python tools/bench_targets.py [--out profiles/targets.json] [--rounds 3] [--repeats 5] [--only 0|1]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pctrans_amd import _timing, targets                                   # noqa: E402
from pctrans_amd.loss import maskformer_criterion as crit                  # noqa: E402
from pctrans_amd.loss.matcher import Point_HungarianMatcher                # noqa: E402

SHAPES = [
    dict(name="configs[2]", N=2, size=(448, 448), instances=20),
    dict(name="configs[3]", N=2, size=(512, 512), instances=60),
]
MODES = ("torch", "hip")


def make_maps(s):
    """`instances` discs per image on a jittered grid (ids with gaps, background 0): blobs, as leaves and nuclei are."""
    g = torch.Generator().manual_seed(1)
    H, W = s["size"]
    cols = int(s["instances"] ** 0.5 + 0.999)
    rows = -(-s["instances"] // cols)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    maps = torch.zeros((s["N"], H, W), dtype=torch.int64)
    for n in range(s["N"]):
        for k in range(s["instances"]):
            cy = (k // cols + 0.5) * H / rows + float(torch.randn((), generator=g)) * 4
            cx = (k % cols + 0.5) * W / cols + float(torch.randn((), generator=g)) * 4
            r = 0.38 * min(H / rows, W / cols) * (0.8 + 0.4 * float(torch.rand((), generator=g)))
            maps[n][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 3 * k + 1
    return maps


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return dict(rounds=v, lowest=min(v), highest=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_targets.py needs a GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "repeats": args.repeats,
              "cpu_threads": torch.get_num_threads(), "shapes": []}
    for s in (SHAPES if args.only is None else [SHAPES[args.only]]):
        maps = make_maps(s)
        kw = dict(points_num=1, semantic_loss_on=True, device=dev)

        def call(mode):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = targets.prepare_instance_targets(maps, mode=mode, **kw)
            e1.record()
            torch.cuda.synchronize()
            return out, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

        def consumers(tg):
            """The first plane requests of a step: the matcher's, then the criterion's (fresh objects: nothing cached)."""
            m = Point_HungarianMatcher(num_points=16)
            c = crit.SetCriterion(1, m, {}, 0.1, [], 16, 3.0, 0.75)
            like = tg[0]["masks"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a = m._match_target_planes(tg, like)
            b = c._hip_target_planes(tg, like)
            torch.cuda.synchronize()
            assert a is not None and b is not None
            return (time.perf_counter() - t0) * 1e3

        out = {mode: call(mode)[0] for mode in MODES}                                       # warm-up
        assert out["hip"].planes is not None
        for a, b in zip(out["hip"], out["torch"]):
            for k in b:
                assert k == "center_points" or torch.equal(a[k], b[k]), k
        plain = [dict(t) for t in out["hip"]]
        consumers(plain), consumers(out["hip"])
        wall = {mode: [] for mode in MODES}
        events, handed, unhanded = [], [], []
        for _ in range(args.rounds):
            w = {mode: [] for mode in MODES}
            ev, h, u = [], [], []
            for _ in range(args.repeats):
                for mode in MODES:
                    _, ms, ems = call(mode)
                    w[mode].append(ms)
                    if mode == "hip":
                        ev.append(ems)
                u.append(consumers(plain))
                h.append(consumers(out["hip"]))
            for mode in MODES:
                wall[mode].append(median(w[mode]))
            events.append(median(ev))
            handed.append(median(h))
            unhanded.append(median(u))
        _timing.kernel_timing(True)
        for _ in range(args.repeats):
            targets.prepare_instance_targets(maps, mode="hip", **kw)
        kernels = {}
        for rec in _timing.kernel_timing(False):
            kernels.setdefault(rec[0], []).append(rec[1])
        kernels = {k: median(v) for k, v in kernels.items()}
        H, W = s["size"]
        total = sum(out["hip"].counts_host)
        written = total * H * W * 5 + s["N"] * H * W
        entry = dict(s, label_map_bytes=int(maps.numel() * maps.element_size()), mask_bytes=total * H * W,
                     planes_bytes_written=written,
                     torch=dict(wall_ms=spread(wall["torch"])), hip=dict(wall_ms=spread(wall["hip"]), event_ms=spread(events),
                                                                        kernel_ms=kernels),
                     planes_write_TBps=written / (kernels["instance_targets planes"] * 1e-3) / 1e12,
                     torch_over_hip=median(wall["torch"]) / median(wall["hip"]),
                     consumers_first_planes_ms=dict(plain_list=spread(unhanded), handed_over=spread(handed)),
                     max_abs_centre_difference=float(max((a["center_points"] - b["center_points"]).abs().max()
                                                         for a, b in zip(out["hip"], out["torch"]))))
        record["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""bench.py -- MSDeformAttn pixel decoder + PCTrans transformer decoder forward throughput on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does what its headline figure needs and no more: set-up, the untimed warm-up (pre-warm, settle blocks, W
steps), the K timed steps, --dump-outputs, the JSON line.  --full adds the measurements that take runs of their own
(cpu_baseline below, ~25 s on the host); the timed steps and every other field of the line are the same either way.

N > 1: one rank per GPU over RCCL.  Started bare (`python bench.py --gpus N`, no WORLD_SIZE in the environment) this
process never touches a GPU: it starts `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child
and exits with its code; started by torch.distributed.run itself (the driver's form) it is one of the N ranks.

One "step" = one forward of MaskFormerHead (pixel decoder with 6 MSDeformAttn encoder layers + 9-layer position-
guided masked-attention decoder + per-query dynamic mask head) over one batch of synthetic ResNet-50-shaped feature
maps of 512x512 images, 100 queries, eval mode, weights random-initialised by the reference's init recipes.
Images are independent, so ranks shard them with no data-path collective (weak scaling, DDP-style launch); the only
collectives are the barriers bracketing the timed region.

The JSON line carries, besides the throughput:
  roofline_mask_head / roofline_attn   the two MFMA kernels north_star names -- the per-query dynamic mask head (one-pass kernel,
                csrc/dyn_mask_head_fused.hip) and the masked cross-attention at the decoder's largest level
                (csrc/cross_attention.hip) -- timed the same way: useful and executed flops against the dense bf16 MFMA peak,
                algorithmic bytes against the HBM peak, "bound" = the nearer of the two.
  roofline      the MSDeformAttn forward kernel (the hot kernel north_star names), timed live with HIP events on its
                launch stream inside the timed steps; achieved = algorithmic bytes per launch / mean launch time,
                algorithmic bytes = N * S * (2*M*D*e + 3*M*L*P*4)  (SURVEY.md 8d), peak = 8 TB/s HBM3E.
  cpu_baseline  --full only: the C/OpenMP oracle (oracle/msda_oracle.c, kind "port") timed on this host for the same
                MSDeformAttn layer shape, and configs[0]'s whole head on the CPU; rank 0 / N=1 only, bounded to ~25 s.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# With 4 encoder levels every convolution of the head is 1x1 and runs as a strided-batched GEMM (layers.Conv2d); with the
# shipped 3-level yaml the FPN's 3x3 convolutions stay on MIOpen (north_star).  On a fresh box MIOpen's default hybrid
# find mode can settle on slow solvers (measured: 110.8 ms/step against 87.3 ms/step with the measured-best ones when
# the 1x1 convolutions still went through it), so ask for a full find: it runs once per shape in the untimed pre-warm.
os.environ.setdefault("MIOPEN_FIND_MODE", "1")
# ... but keep MIOpen's naive reference solver out of that find: it is timed like every other candidate, 24 launches of
# 0.38 s each at this batch (rocprofv3: naive_conv_ab_nonpacked_fwd_nhwc, 9 s of a 15 s run), and never wins
os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", "0")



def per_rank_miopen_dirs(environ=os.environ):
    """Several ranks on one node: every rank gets its OWN MIOpen user database and kernel cache directory (set before the
    first convolution).  With the shared default (~/.config/miopen, ~/.cache/miopen) eight ranks running a full find
    (MIOPEN_FIND_MODE=1) at once serialise on one database file's lock and compile the same kernels into one cache.
    Directories an operator has already set are left alone.  Returns what it set (for the JSON line / tests)."""
    if int(environ.get("WORLD_SIZE", "1")) <= 1 or "LOCAL_RANK" not in environ:
        return {}
    base = os.path.join(environ.get("PCT_BENCH_MIOPEN_BASE", os.path.join("/tmp", "pct_bench_miopen_%d" % os.getuid())),
                        "rank%s" % environ["LOCAL_RANK"])
    made = {}
    for var, sub in (("MIOPEN_USER_DB_PATH", "db"), ("MIOPEN_CUSTOM_CACHE_DIR", "cache")):
        if var not in environ:
            d = os.path.join(base, sub)
            os.makedirs(d, exist_ok=True)
            environ[var] = d
            made[var] = d
    return made


MIOPEN_DIRS = per_rank_miopen_dirs()

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s peak (6.3 TB/s achievable)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128, help="images per GPU per step")
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--levels", type=int, default=4, choices=[3, 4],
                    help="encoder feature levels: 4 = res2..res5 (north-star shape), 3 = res3..res5 (shipped yaml)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"],
                    help="autocast dtype of the transformer decoder; the pixel decoder is fp32 as in the reference")
    ap.add_argument("--loc-dist", default="M", choices=["M", "I"],
                    help="statistics of the encoder's sampling offsets (BASELINE.md 3 / SURVEY 8d): M = model-like, "
                         "sampling_offsets.weight ~ N(0, s) scaled per layer so that offsets are N(0, 2 px) on the sampled "
                         "level; I = the reference's initialisation (zero weight, head-directional bias of 1..4 px: what an "
                         "untrained network gives)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the CPU baseline (cpu_baseline)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0's predictions and mask "
                         "features) as DIR/<name>.npy, float32 / float64; large arrays as a fixed, seeded sample")
    return ap.parse_args()


def build_head(args, device):
    from pctrans_amd.config import get_cfg, resnet_output_shape
    from pctrans_amd.meta_arch.mask_former_head import MaskFormerHead
    feats = ("res2", "res3", "res4", "res5") if args.levels == 4 else ("res3", "res4", "res5")
    cfg = get_cfg(num_queries=args.queries, enc_in_features=feats)
    shapes = resnet_output_shape(50)
    torch.manual_seed(0)
    head = MaskFormerHead(**MaskFormerHead.from_config(cfg, shapes)).to(device).eval()
    return head, shapes


def model_like_offsets(head, feats, sigma_px=2.0):
    """Distribution M: give every encoder layer's sampling_offsets Linear a random weight and zero bias, then scale the
    weight so that the offsets it produces on these features have standard deviation `sigma_px` (measured by running the
    pixel decoder once with the layer's input captured).  Returns the realised per-layer standard deviations."""
    import torch.nn.functional as F
    layers = list(head.pixel_decoder.transformer.encoder.layers)
    g = torch.Generator(device="cpu").manual_seed(4321)
    for lyr in layers:
        so = lyr.self_attn.sampling_offsets
        with torch.no_grad():
            so.weight.copy_(torch.randn(so.weight.shape, generator=g).to(so.weight.device) * 0.1443)   # ~2 px on unit-variance rows
            so.bias.zero_()
    small = {k: v[:2] for k, v in feats.items()}
    stds = []
    # (the calibration passes run on the quad-owner kernel, so that the kernel the bench line reports on is launched by the
    # bench steps only and per-kernel profiler averages are not diluted by these 2-image launches)
    from pctrans_amd import _lib
    _lib.lib().pct_msda_set_kernel_choice(3)
    try:
        for i, lyr in enumerate(layers):          # layer by layer: rescaling layer i changes what layers > i see
            cap = {}
            attn = lyr.self_attn
            orig = attn.forward

            def spy(query, *a, _orig=orig, _cap=cap, **kw):
                qp = kw.get("_query_pos")
                _cap["x"] = (query if qp is None else query + qp).detach()
                return _orig(query, *a, **kw)
            attn.forward = spy
            try:
                with torch.no_grad():
                    head.pixel_decoder.forward_features(small)
            finally:
                attn.forward = orig
            off = F.linear(cap["x"].float(), attn.sampling_offsets.weight, attn.sampling_offsets.bias)
            s = float(off.detach().std())
            with torch.no_grad():
                attn.sampling_offsets.weight.mul_(sigma_px / s)
            stds.append(float(F.linear(cap["x"].float(), attn.sampling_offsets.weight).detach().std()))
    finally:
        _lib.lib().pct_msda_set_kernel_choice(-1)      # the process-wide override never outlives the calibration
    return stds


def synth_features(shapes, batch, image, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return {k: torch.randn(batch, s.channels, image // s.stride, image // s.stride, device=device, generator=g)
            for k, s in shapes.items()}


DUMP_BUDGET_BYTES = 60 * 10**6    # the arrays' data; with the .npy headers the directory stays under 64 MB


def flatten_outputs(obj, prefix, out):
    """The tensors of a (nested) dict / list / tuple output, keyed by their path joined with '.'.  Insertion order is
    the structure's own, so two runs list the same names in the same order."""
    if torch.is_tensor(obj):
        out[prefix] = obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            flatten_outputs(v, "%s.%s" % (prefix, k) if prefix else str(k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            flatten_outputs(v, "%s.%d" % (prefix, i) if prefix else str(i), out)
    return out


def dump_outputs(outputs, dirname, budget=DUMP_BUDGET_BYTES):
    """Write every tensor of `outputs` as <dirname>/<name>.npy: float64 stays float64, everything else becomes float32.
    The budget is shared out smallest array first, each taking at most an equal part of what is left: an array that
    does not fit its part is written as the elements at that many flat indices, drawn (sorted, without replacement) by a
    generator seeded from the array's name and shape, so that two runs with the same arguments sample the same positions.
    Returns {name: {"shape", "sampled"}} where "sampled" is the number of elements written, or None for the whole array."""
    import zlib
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    tensors = flatten_outputs(outputs, "", {})
    item = {k: 8 if t.dtype == torch.float64 else 4 for k, t in tensors.items()}
    order = sorted(tensors, key=lambda k: (tensors[k].numel() * item[k], k))
    take, left = {}, budget
    for i, k in enumerate(order):
        take[k] = min(tensors[k].numel(), left // (len(order) - i) // item[k])
        left -= take[k] * item[k]
    manifest = {}
    for name, t in tensors.items():
        t = t.detach()
        flat = t.reshape(-1)
        sampled = take[name] < flat.numel()
        if sampled:
            seed = zlib.crc32(("%s %s" % (name, list(t.shape))).encode())
            idx = np.sort(np.random.default_rng(seed).choice(flat.numel(), take[name], replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        a = flat.to(torch.float64 if item[name] == 8 else torch.float32).cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), a if sampled else a.reshape(tuple(t.shape)))
        manifest[name] = {"shape": list(t.shape), "sampled": take[name] if sampled else None}
    return manifest


def host_cpu():
    """(model name, physical cores, logical CPUs) of this host, from /proc/cpuinfo."""
    model, cores, logical = "unknown", set(), 0
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("processor"):
                    logical += 1
                elif line.startswith("model name") and model == "unknown":
                    model = line.split(":", 1)[1].strip()
                elif line.startswith("physical id"):
                    phys = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":", 1)[1].strip()
                    cores.add((phys, core))
    except OSError:
        pass
    return model, (len(cores) or logical or 1), (logical or 1)


def wants_cpu_baseline(args, world):
    """The CPU baseline is an extra of --full (unless --no-cpu-baseline), and only a 1-rank run takes it: a plain run does
    what its headline figure needs and no more."""
    return args.full and not args.no_cpu_baseline and world == 1


def cpu_baseline(args, levels_hw):
    """The CPU side of the comparison, rank 0 / N = 1 only, bounded to ~25 s in all:
      * headline: the C/OpenMP oracle's MSDeformAttn forward (one encoder layer, one image of the bench geometry,
        model-like locations) on all PHYSICAL cores, plus the same on 1 thread;
      * table: P1 / P2 / P4 x {U, M} on all physical cores, ~1 s each;
      * head: BASELINE.json configs[0] -- the whole head (pixel decoder + transformer decoder) on a 256 x 256 tile,
        ResNet-18 channels, 50 queries, batch 1, on the CPU through the dense PyTorch formulation of the op (what the
        reference falls back to when ops/ is not built, ops/modules/ms_deform_attn.py:119-121)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from msda_cases import make_case
    from oracle import msda_oracle as orc
    model, phys, logical = host_cpu()
    threads_max = orc.max_threads()
    threads = max(1, min(phys, threads_max))

    def timed(case, seconds, nthreads, warm_seconds=0.0):
        orc.set_threads(nthreads)
        a = (case["value"], case["shapes"], case["starts"], case["loc"], case["attn"])
        orc.forward(*a)                                                         # warm-up
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < warm_seconds:      # (the first second of a fresh OpenMP team runs ~8x slower)
            orc.forward(*a)
        reps, t0 = 0, time.perf_counter()
        while True:
            orc.forward(*a)
            reps += 1
            el = time.perf_counter() - t0
            if el >= seconds or reps >= 20000:
                return reps, el

    def alg_bytes(shapes, P=4):
        S_ = sum(h * w for h, w in shapes)
        return S_ * (2 * 128 * 4 + 3 * 8 * len(shapes) * P * 4)

    S = sum(h * w for h, w in levels_hw)
    c = make_case(seed=0, N=1, M=8, D=16, Lq=S, P=4, shapes=levels_hw, model_like=True)
    reps, el = timed(c, args.cpu_seconds, threads, warm_seconds=1.5)
    reps1, el1 = timed(c, min(3.0, args.cpu_seconds), 1)
    table = {}
    shapes_tbl = {"P1": [(16, 16), (32, 32), (64, 64)], "P2": [(16, 16), (32, 32), (64, 64), (128, 128)],
                  "P4": [(17, 22), (33, 44), (65, 87)]}
    for name, shp in shapes_tbl.items():
        St = sum(h * w for h, w in shp)
        for dist in ("U", "M"):
            ct = make_case(seed=0, N=1, M=8, D=16, Lq=St, P=4, shapes=shp, model_like=(dist == "M"))
            r, e = timed(ct, 1.0, threads)
            table["%s_%s" % (name, dist)] = {"ms_per_image_layer": 1e3 * e / r, "algorithmic_GBps": alg_bytes(shp) * r / e / 1e9}
    orc.set_threads(threads_max)
    out = {"value": reps / el, "unit": "MSDeformAttn-forward image-layers/s", "cores": threads, "kind": "port",
           "cpu_model": model, "physical_cores": phys, "logical_cpus": logical, "threads_used": threads,
           "sample": "oracle/msda_oracle.c (C + OpenMP, %d threads = physical cores) forward, 1 image x %d reps, levels %s, "
                     "S=%d, M=8 D=16 P=4 fp32, model-like locations" % (threads, reps, list(levels_hw), S),
           "ms_per_image_layer": 1e3 * el / reps, "algorithmic_GBps": alg_bytes(levels_hw) * reps / el / 1e9,
           "one_thread": {"value": reps1 / el1, "ms_per_image_layer": 1e3 * el1 / reps1,
                          "algorithmic_GBps": alg_bytes(levels_hw) * reps1 / el1 / 1e9},
           "table_all_cores": table}
    try:
        out["head_config1_cpu"] = cpu_head_config1(threads)
    except Exception as e:      # the CPU head is an extra; never lose the bench line over it
        out["head_config1_cpu"] = {"error": repr(e)}
    return out


def cpu_head_config1(threads, seconds=5.0):
    """BASELINE.json configs[0]: single 256 x 256 tile, ResNet-18 feature shapes, 50 queries, batch 1, CPU, fp32."""
    from pctrans_amd.config import get_cfg, resnet_output_shape
    from pctrans_amd.meta_arch.mask_former_head import MaskFormerHead
    from pctrans_amd.pixel_decoder.ops.modules import ms_deform_attn as msda_mod
    prev_threads = torch.get_num_threads()
    torch.set_num_threads(threads)
    prev = msda_mod.allow_cpu_reference(True)          # the dense formulation of the op, for CPU tensors only
    try:
        cfg = get_cfg(num_queries=50, enc_in_features=("res3", "res4", "res5"))
        shapes = resnet_output_shape(18)
        torch.manual_seed(0)
        head = MaskFormerHead(**MaskFormerHead.from_config(cfg, shapes)).eval()
        g = torch.Generator().manual_seed(1)
        feats = {k: torch.randn(1, s.channels, 256 // s.stride, 256 // s.stride, generator=g) for k, s in shapes.items()}
        with torch.no_grad():
            head(feats)
            reps, t0 = 0, time.perf_counter()
            while True:
                head(feats)
                reps += 1
                el = time.perf_counter() - t0
                if el >= seconds:
                    break
        return {"value": reps / el, "unit": "samples/s", "ms_per_sample": 1e3 * el / reps, "threads": threads,
                "workload": "configs[0]: 256x256 tile, ResNet-18 feature shapes, 3 encoder levels (8^2, 16^2, 32^2), "
                            "50 queries, batch 1, fp32, PyTorch CPU kernels + dense MSDeformAttn formulation"}
    finally:
        msda_mod.allow_cpu_reference(prev)
        torch.set_num_threads(prev_threads)


def traffic_from_profile(args):
    """HBM bytes per launch of the MSDeformAttn kernel from the PMC passes committed under profiles/ (collected with
    `rocprofv3 --pmc TCC_EA0_RDREQ_{32B,64B,128B}_sum` and `--pmc TCC_EA0_WRREQ_*` in separate passes around this very
    script, tools/pmc_bench_traffic.sh; bench.py cannot read counters itself).  Only reported when the committed
    measurement is for this workload."""
    path = os.path.join(ROOT, "profiles", "r04_msda_traffic_batch%d_dist%s.json" % (args.batch, args.loc_dist))
    if not os.path.exists(path):          # (an older record of the same kernel family: still per launch of this workload)
        path = os.path.join(ROOT, "profiles", "r03_msda_traffic_batch%d_dist%s.json" % (args.batch, args.loc_dist))
    try:
        with open(path) as f:
            t = json.load(f)
        if t.get("batch") == args.batch and t.get("levels") == args.levels and args.image == 512:
            if "hbm_bytes" in t:      # memory-side requests by size (32/64/128 B): no FETCH_SIZE calibration needed
                return {"bytes": t["hbm_bytes"], "read_bytes": t["hbm_read_bytes"], "write_bytes": t["hbm_write_bytes"],
                        "source": os.path.relpath(path, ROOT)}
            return {"bytes": t["hbm_bytes_raw"], "bytes_if_fetch_doubled": t["hbm_bytes_fetch_doubled"],
                    "source": os.path.relpath(path, ROOT)}
    except (OSError, ValueError, KeyError):
        pass
    return None


def issue_from_profile(args, prefix):
    """Issue-side SQ counters of one kernel family from the committed PMC passes over this script (tools/pmc_bench_issue.sh ->
    profiles/r04_bench_issue.json): the share of SIMD cycles the matrix pipe is busy, a vector instruction is issuing, an LDS
    instruction is issuing.  The unit a kernel keeps busiest is the bound it is nearest to; only for the judged workload."""
    if not (args.batch == 128 and args.levels == 4 and args.image == 512 and args.loc_dist == "M"):
        return None
    try:
        with open(os.path.join(ROOT, "profiles", "r04_bench_issue.json")) as f:
            t = json.load(f)
        recs = [v for k, v in t["kernels"].items() if k.startswith(prefix)]
        if not recs:
            return None
        n = sum(r["launches"] for r in recs)
        out = {k: sum(r[k] * r["launches"] for r in recs) / n for k in ("mfma_busy", "valu_issue", "lds_issue", "wait_any")}
        out["nearest_bound"] = max(("mfma_busy", "valu_issue", "lds_issue"), key=lambda k: out[k])
        out["source"] = "profiles/r04_bench_issue.json"
        return out
    except (OSError, ValueError, KeyError):
        return None


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a child `torch.distributed.run` (the
    reference's launch, README.md:30-33, in its current spelling) and return its exit code.  Nothing in this process
    has touched the GPU (device_count() does not initialise it), and it never replaces itself with another program."""
    import socket
    import subprocess
    share = os.environ.get("PCT_BENCH_SHARE_GPU") == "1"
    ndev = torch.cuda.device_count()
    if not share and args.gpus > ndev:
        print("bench.py: --gpus %d but %d GPU(s) visible (PCT_BENCH_SHARE_GPU=1 rehearses several ranks on one card "
              "over gloo)" % (args.gpus, ndev), file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    # only the JSON line goes to this process's stdout; anything else a rank or a library prints there (gloo announces its
    # peers on stdout, for instance) is passed on to stderr
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:
        if line.startswith("{") and '"metric"' in line:
            sys.stdout.write(line)
            sys.stdout.flush()
        else:
            sys.stderr.write(line)
    return proc.wait()


def main():
    args = parse()
    if args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr)
        sys.exit(2)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)
    assert torch.cuda.is_available(), "bench.py needs an MI355X; there is no CPU path"
    # PCT_BENCH_SHARE_GPU=1 (rehearsal only): several ranks on one card over gloo, to exercise the multi-rank code path
    # on a 1-GPU box; the judged runs use one GPU per rank over RCCL ('nccl' == RCCL on ROCm).
    share = os.environ.get("PCT_BENCH_SHARE_GPU") == "1"
    from pctrans_amd.parallel import init_devices
    device, rank, local_rank, world = init_devices(distributed=world > 1, backend="nccl", manual_seed=0,
                                                   share_gpu=share)
    torch.cuda.set_device(device)

    from pctrans_amd import MultiScaleDeformableAttention as MSDA
    from pctrans_amd import _lib
    _lib.lib()      # fail loudly if the HIP library is missing

    head, shapes = build_head(args, device)
    feats = synth_features(shapes, args.batch, args.image, device, seed=1234 + rank)
    offset_std = model_like_offsets(head, feats) if args.loc_dist == "M" else None
    amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=(args.dtype == "bf16"))

    def step():
        with torch.no_grad(), amp:
            return head(feats)

    for _ in range(2):          # untimed pre-warm: MIOpen's first-call kernel search for the 3x3 convolutions
        step()
    # ... and until the SUSTAINED step time has settled.  Measured on this pool (round 4, tools/diag_fresh_box.py and the
    # step_ms list below): in three of five first runs on a fresh box two steps about one second into the back-to-back load
    # took 325 ms instead of 106 (a one-off stall of ~440 ms, the same kernels, gone in the next process on that box) while
    # single steps bracketed by synchronisations had already settled at 106 ms -- so the settling is judged on BLOCKS of 5
    # back-to-back steps, the way the timed region runs: at least 8 blocks, until two consecutive blocks agree within 1.5 %,
    # at most 12 (60 untimed steps, ~5.5 s).  With several ranks the count is FIXED (8 blocks): a data-dependent exit would let
    # ranks enter the timed region after different numbers of steps.  Blocks taken and their per-step times go into the JSON
    # line (settle_steps / settle_ms); no collective inside.
    # (Python's cyclic garbage collector stays off from here to the end of the timed region: a generation-2 pass over the module
    # trees pauses the launching thread for 100-200 ms -- a step of 289 ms among steps of 101.7 in round 4 -- and with the host
    # only ~30 % ahead of the device that is a hole in the stream.  Collected once here; reference counting still frees the
    # step's tensors.)
    import gc
    gc.collect()
    gc.disable()
    # (End of round 4: twice in ~15 runs ONE step of 380-450 ms appeared among steps of 90, both times as the second step of
    # the timed region -- 2.0-2.3 s into the sustained load with 4 settle blocks, and 1-2 steps after the per-launch timing
    # events start being recorded; its hook-timed kernels took their usual time, the hole was between kernels.  Cause not
    # established (tools/diag_events.py does not reproduce it).  Both candidates are now put in front of the timed region: the
    # settle blocks run exactly as the timed steps do -- per-launch events recorded -- and there are at least 8 of them (40
    # steps, ~3.6 s; at most 12; fixed 8 with several ranks).)
    SETTLE_BLOCK = 5
    prev = None
    settle_ms = []
    # (PCT_BENCH_SETTLE_BLOCKS: fewer blocks for counter-collection runs -- `rocprofv3 --pmc` around this script ends in a
    # segmentation fault inside the profiler once a run passes ~30 000 dispatches with four counters, tools/pmc_bench_*.sh set 2;
    # the count taken is in the JSON line)
    settle_min = max(1, int(os.environ.get("PCT_BENCH_SETTLE_BLOCKS", "8")))
    for i_blk in range(settle_min + 4 if world == 1 else settle_min):
        MSDA.kernel_timing(True)
        torch.cuda.synchronize(device)
        t_s = time.perf_counter()
        for _ in range(SETTLE_BLOCK):
            step()
        torch.cuda.synchronize(device)
        dt = (time.perf_counter() - t_s) / SETTLE_BLOCK
        # (the block's records are dropped, its events reused by the next block: the number of live timing events stays that
        # of one block)
        MSDA.kernel_timing(False, recycle=True)
        settle_ms.append(1e3 * dt)
        if world == 1 and i_blk >= settle_min - 1 and prev is not None and abs(dt - prev) <= 0.015 * prev:
            break
        prev = dt
    MSDA.kernel_timing(True)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(device)
    MSDA.kernel_timing(False, recycle=True)

    def fence():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    # Every event the timed region will record is created and recorded once BEFORE it (pctrans_amd/_timing.reserve: the runtime
    # allocates an event's profiling signal at its first record, in pools that grow in steps): count one warm-up step's
    # hook-timed launches, then reserve two events per launch for all timed steps.
    from pctrans_amd import _timing as _kt
    MSDA.kernel_timing(True)
    step()
    per_step = _kt.count()
    MSDA.kernel_timing(False)
    _kt.reserve(2 * per_step * (args.steps + 1) + 16, device)
    step_marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    for e in step_marks:
        e.record()
    MSDA.kernel_timing(True)           # HIP events around every hook-timed launch, on the launch stream
    fence()
    t0 = time.perf_counter()
    step_marks[0].record()
    rec_marks = [_kt.count()]
    for i_step in range(args.steps):
        pred, mask_features = step()
        step_marks[i_step + 1].record()       # one event per step: a straggler step shows in the JSON (step_ms)
        rec_marks.append(_kt.count())         # ... and which of the hook-timed launches belong to it
        if i_step + 1 < args.steps:
            del mask_features                 # (only the last step's is kept, for --dump-outputs)
    fence()
    elapsed = time.perf_counter() - t0
    gc.enable()
    step_ms = [step_marks[i].elapsed_time(step_marks[i + 1]) for i in range(args.steps)]
    launches = MSDA.kernel_timing(False)
    # per step: the sum of the hook-timed launches (MSDeformAttn, fused FFN, mask head, attention: ~70 % of a step) and the longest
    # one -- a straggler step whose timed kernels took their usual time stalled BETWEEN kernels (host, runtime, an untimed kernel)
    step_timed = [round(sum(r[1] for r in launches[rec_marks[i]:rec_marks[i + 1]]), 2) for i in range(args.steps)]
    step_longest = [max(((r[1], r[0]) for r in launches[rec_marks[i]:rec_marks[i + 1]]), default=(0.0, ""))
                    for i in range(args.steps)]

    t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if share else device)
    per_rank = [elapsed]
    if world > 1:
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)                       # each rank's own wall time: a straggler shows in the JSON
        per_rank = [float(x.item()) for x in every]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    assert torch.isfinite(pred["pred_masks"].float()).all(), "non-finite output"
    dumped = None
    if args.dump_outputs and rank == 0:
        # what a caller of MaskFormerHead.forward receives (predictions dict, mask features), from the last timed step
        dumped = dump_outputs(dict(pred, mask_features=mask_features), args.dump_outputs)

    rc = 0
    if rank == 0:
        enc_feats = ["res2", "res3", "res4", "res5"][4 - args.levels:]
        levels_hw = [(args.image // shapes[k].stride,) * 2 for k in reversed(enc_feats)]     # coarse -> fine
        S = sum(h * w for h, w in levels_hw)
        L, M, D, P = len(levels_hw), 8, 16, 4
        alg_bytes = args.batch * S * (2 * M * D * 4 + 3 * M * L * P * 4)
        fwd = [rec[1] for rec in launches if rec[0] == "forward"]
        kernels_run = sorted({rec[2] for rec in launches if rec[0] == "forward" and len(rec) > 2})
        # the roofline record names ONE kernel: every timed MSDeformAttn launch must have run the same family, and at the
        # judged workload (batch >= 8 images of 512^2) that family is the pyramid-column kernel.  A violation is REPORTED in
        # the line (roofline.kernel_check) and turns the exit code non-zero after the line is printed.
        kernel_check = "ok"
        if len(kernels_run) != 1:
            kernel_check = "timed MSDeformAttn launches ran %d kernel families: %s" % (
                len(kernels_run), [MSDA.KERNEL_NAMES.get(k, k) for k in kernels_run])
        elif kernels_run != [4] and args.batch * args.image * args.image >= 8 * 512 * 512:
            kernel_check = "expected the pyramid-column kernel, ran %s" % MSDA.KERNEL_NAMES.get(kernels_run[0], kernels_run[0])
        k0 = kernels_run[0] if kernels_run else -1
        mean_ms = sum(fwd) / max(1, len(fwd))
        achieved = alg_bytes / (mean_ms * 1e-3) / 1e9 if fwd else None
        out = {
            "metric": "MSDeformAttn+decoder fwd samples/sec at 512x512, 100 queries",
            "value": world * args.batch * args.steps / elapsed,
            "unit": "samples/s",
            "n_gpus": world,
            "world_size_observed": dist.get_world_size() if world > 1 else 1,
            "backend": dist.get_backend() if world > 1 else None,
            "steps": args.steps,
            "warmup": args.warmup,
            "settle_steps": SETTLE_BLOCK * len(settle_ms), "settle_ms": [round(x, 2) for x in settle_ms],
            "step_ms": [round(x, 2) for x in step_ms],
            "step_timed_kernels_ms": step_timed,
            "step_longest_timed_kernel": ["%.2f %s" % sl for sl in step_longest],
            "ms_per_step": 1e3 * elapsed / args.steps,
            "miopen_dirs_rank0": MIOPEN_DIRS or None,
            "dumped_outputs": {"dir": args.dump_outputs, "arrays": dumped} if dumped is not None else None,
            "ms_per_step_per_rank": {"min": 1e3 * min(per_rank) / args.steps, "max": 1e3 * max(per_rank) / args.steps,
                                     "ranks": [1e3 * x / args.steps for x in per_rank]},
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16 decoder (autocast) / f32 MSDeformAttn pixel decoder" if args.dtype == "bf16" else "f32",
            "data": "synthetic",
            "full": args.full,
            "config": {
                "workload": "configs[1]: %dx%d synthetic, ResNet-50 feature shapes (backbone not in the timed path), "
                            "MSDeformAttn pixel decoder over %d levels %s + 9-layer masked-attention decoder, "
                            "%d queries, eval" % (args.image, args.image, L, levels_hw, args.queries),
                "per_gpu_batch": args.batch, "global_batch": world * args.batch, "levels": L,
                "queries": args.queries, "parallelism": "dp%d (images sharded, no data-path collective)" % world,
            },
            "roofline": {
                "kernel": ("%s%s (MSDeformAttn forward incl. softmax + location math); id reported by "
                           "pct_msda_last_kernel() after every timed launch" % (
                               MSDA.KERNEL_NAMES.get(k0, "none"),
                               ": pct::msda_forward_col_kernel<L=%d, fused front-end, 256 threads>, LDS gather, one lane per "
                               "(query, head)" % L if k0 == 4 else "")),
                "kernel_check": kernel_check,
                "location_dist": ({"name": "M", "definition": "sampling_offsets.weight ~ N(0, s), zero bias, s scaled per "
                                   "encoder layer so that offsets are N(0, 2 px) on the sampled level",
                                   "offset_std_px_per_layer": offset_std} if args.loc_dist == "M" else
                                  {"name": "I", "definition": "reference initialisation: zero sampling_offsets.weight, "
                                   "head-directional bias of 1..4 px"}),
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic_from_profile(args),
                "algorithmic_bytes_per_launch": alg_bytes, "mean_launch_ms": mean_ms, "launches_timed": len(fwd),
                "share_of_step": (sum(fwd) / (1e3 * elapsed)) if fwd else None,
                "issue": issue_from_profile(args, "pct::msda_forward_col_kernel"),
            },
        }
        # second hand-written kernel on the path, MFMA-bound: the encoder's whole feed-forward block in one kernel
        # (ffn_fused_split.hip); the two-kernel path (linear_k128_split + linear_ln_split) when that one does not apply
        ffn = [rec[1] for rec in launches if rec[0] == "ffn f=1024"]
        ffn1 = [rec[1] for rec in launches if rec[0] == "linear_k128 n=1024 relu"]
        rows = args.batch * S
        if ffn:
            msf = sum(ffn) / len(ffn)
            gemm_tf = 2.0 * 2.0 * rows * 128 * 1024 / (msf * 1e-3) / 1e12        # both products
            out["roofline_mfma"] = {
                "kernel": "pct::ffn_fused_split_kernel (encoder FFN: LayerNorm(x + W2 relu(W1 x + b1) + b2), x [%d,128], hidden 1024 "
                          "kept in registers; fp32 operands as exact 3-way bf16 splits, 6 x v_mfma_f32_32x32x16_bf16 per fp32 "
                          "MFMA-equivalent) + ffn_split_weights_kernel" % rows,
                "bound": "mfma", "achieved": 6.0 * gemm_tf, "peak": 2500.0, "unit": "TFLOP/s", "frac": 6.0 * gemm_tf / 2500.0,
                "gemm_fp32_equiv_tflops": gemm_tf, "mean_launch_ms": msf, "launches_timed": len(ffn),
                "share_of_step": sum(ffn) / (1e3 * elapsed), "issue": issue_from_profile(args, "pct::ffn_fused_split_kernel"),
                "note": "achieved = bf16 MFMA flops executed (6 x the two GEMMs' 2*rows*128*1024 each) / launch time; peak = "
                        "dense bf16 MFMA rate at 2.4 GHz (the kernel runs at ~1.85 GHz under the power limit); the same GEMMs "
                        "counted once are gemm_fp32_equiv_tflops (the fp32 MFMA peak is 157.3)",
            }
        elif ffn1:
            ms1 = sum(ffn1) / len(ffn1)
            gemm_tf = 2.0 * rows * 128 * 1024 / (ms1 * 1e-3) / 1e12
            out["roofline_mfma"] = {
                "kernel": "pct::linear_k128_split_kernel<bias+ReLU> (encoder FFN linear1: [%d,128] x [1024,128]^T)" % rows,
                "bound": "mfma", "achieved": 6.0 * gemm_tf, "peak": 2500.0, "unit": "TFLOP/s", "frac": 6.0 * gemm_tf / 2500.0,
                "gemm_fp32_equiv_tflops": gemm_tf, "mean_launch_ms": ms1, "launches_timed": len(ffn1),
                "share_of_step": sum(ffn1) / (1e3 * elapsed),
                "note": "achieved = bf16 MFMA flops executed (6 x the GEMM's) / launch time",
            }
        MFMA_PEAK_TF = 2500.0      # dense bf16 (MI355X_MICROARCH.md); HBM peak as above
        # ---- the per-query dynamic mask head (dec.py:647-719): 10 calls per step on the stride-4 mask features -------------
        for tag in ("mask_head one-pass", "mask_head two-launch"):
            mh = [rec[1] for rec in launches if rec[0] == tag]
            if not mh:
                continue
            Hm = Wm = args.image // 4 if args.levels == 4 else args.image // 8
            NQ, HWm = args.batch * args.queries, Hm * Wm
            ms_mh = sum(mh) / len(mh)
            useful = 2.0 * 216 * NQ * HWm                                # 8x18 + 8x8 + 8 MACs per (query, pixel)
            executed = (16 * 16 * 32 + 16 * 16 * 16) * 2.0 * (NQ / 2) * (HWm / 16) * (1.25 if tag.endswith("one-pass") else 1.0)
            alg = 4.0 * args.batch * 16 * HWm + 2.0 * NQ * 4 * HWm + 0.1 * NQ * HWm + 4.0 * NQ * 233   # features, x2 logits, mask (mean over the
            # 10 calls: 4 x 1/64 + 3 x 1/16 + 3 x 1/4 of the map), generated parameters
            if tag.endswith("two-launch"):
                alg_note = "algorithmic bytes as for the one-pass kernel; this path also writes and re-reads the %d MB logits plane" % (2 * NQ * HWm // 10**6)
            else:
                alg_note = "algorithmic bytes: fp32 features once, bf16 x2-upsampled logits once, mask bytes, generated parameters"
            f_m, f_h = executed / (ms_mh * 1e-3) / 1e12 / MFMA_PEAK_TF, alg / (ms_mh * 1e-3) / 1e9 / HBM_PEAK_GBS
            out["roofline_mask_head"] = {
                "kernel": "pct::dmh_fused_kernel (+ dmh_prepare_kernel)" if tag.endswith("one-pass") else
                          "pct::dmh_logits_mfma_kernel + pct::dmh_resize_kernel",
                "bound": "hbm" if f_h >= f_m else "mfma", "frac": max(f_h, f_m), "frac_hbm": f_h, "frac_mfma_executed": f_m,
                "achieved_GBps": alg / (ms_mh * 1e-3) / 1e9, "peak_GBps": HBM_PEAK_GBS,
                "useful_TFLOPs": useful / (ms_mh * 1e-3) / 1e12, "executed_mfma_TFLOPs": executed / (ms_mh * 1e-3) / 1e12,
                "peak_TFLOPs": MFMA_PEAK_TF, "algorithmic_bytes_per_call": alg, "mean_call_ms": ms_mh,
                "calls_timed": len(mh), "share_of_step": sum(mh) / (1e3 * elapsed), "note": alg_note,
                "issue": issue_from_profile(args, "pct::dmh_fused_kernel"),
            }
        # ---- masked cross-attention (attention.py:271-387) at the decoder's finest level (most keys) --------------------------
        xa = {}
        for rec in launches:
            if rec[0].startswith("cross_attention S=") or rec[0].startswith("masked_attention S="):
                xa.setdefault((rec[0].split(" ")[0], int(rec[0].split("=")[1])), []).append(rec[1])
        if xa:
            (kname, S_a), tl = max(xa.items(), key=lambda kv: kv[0][1])
            ms_a = sum(tl) / len(tl)
            Nn, Qq, Hh = args.batch, args.queries, 8
            useful = 2.0 * Nn * Hh * Qq * S_a * (32 + 16)
            executed = 2.0 * Nn * Hh * (-(-Qq // 16) * 16) * S_a * (32 + 16)       # padded query tiles
            alg = 2.0 * (3 * S_a * Nn * 128 + 3 * Qq * Nn * 128) + Nn * Qq * S_a
            f_m, f_h = executed / (ms_a * 1e-3) / 1e12 / MFMA_PEAK_TF, alg / (ms_a * 1e-3) / 1e9 / HBM_PEAK_GBS
            out["roofline_attn"] = {
                "kernel": "pct::cross_attention_kernel (split operands, LDS-staged)" if kname == "cross_attention" else
                          "pct::masked_attention_kernel (generic operands)",
                "keys": S_a, "bound": "hbm" if f_h >= f_m else "mfma", "frac": max(f_h, f_m), "frac_hbm": f_h,
                "frac_mfma_executed": f_m, "achieved_GBps": alg / (ms_a * 1e-3) / 1e9, "peak_GBps": HBM_PEAK_GBS,
                "useful_TFLOPs": useful / (ms_a * 1e-3) / 1e12, "peak_TFLOPs": MFMA_PEAK_TF,
                "algorithmic_bytes_per_call": alg, "mean_call_ms": ms_a, "calls_timed": len(tl),
                "all_levels_ms": {"%s S=%d" % k: sum(v) / len(v) for k, v in sorted(xa.items())},
                "share_of_step": sum(sum(v) for v in xa.values()) / (1e3 * elapsed),
                "issue": issue_from_profile(args, "pct::cross_attention_kernel"),
                "note": "algorithmic bytes: K-content, K-position, V, the query halves and the output once (bf16), mask bytes once",
            }
        if wants_cpu_baseline(args, world):
            out["cpu_baseline"] = cpu_baseline(args, levels_hw)
            out["cpu_baseline"]["gpu_same_unit"] = args.batch / (mean_ms * 1e-3) if fwd else None
        print(json.dumps(out), flush=True)
        if kernel_check != "ok":
            print("bench.py: " + kernel_check, file=sys.stderr)
            rc = 3

    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and rc:
        sys.exit(rc)


if __name__ == "__main__":
    main()

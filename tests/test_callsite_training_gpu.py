"""GPU: one training step of the whole model (forward in train mode, losses, backward) with every HIP call it makes
checked against float64 on the operands it actually received (tests/callsite_capture.py with TRAINING_ENTRIES;
tests/callsite_reference.py).  Under autograd the encoder takes the unfused MSDeformAttn forward and its backward, and the
matcher assigns all prediction heads' problems in one LSAP launch; the forward-only fused kernels must not run at all.

Configurations, built as tools/record_train_configs.py builds them (BN, synthetic disc targets, fp32, TF32 off):
BASELINE configs[2] (ResNet-50, 2 x 448^2, 100 queries, 20 targets), configs[3] (ResNet-50, 2 x 512^2, 300 queries, 60
targets) and a small non-square run (ResNet-18, 1 x 256 x 320, 50 queries, 8 targets: the training crops are square, so a
W / H swap in grad_loc would pass both others; it also routes the backward to the generic kernel).  Each in two states:
`init` (reference points at pixel centres, whole-pixel offsets: every sample on its own query's level sits on a texel) and
`M` (bench.model_like_offsets on the backbone's features).

Bounds:
  * unfused forward, and the generic entries that fall back to torch under autograd: test_callsite_parity_gpu's bounds;
  * backward, per level slice (grad_value rows of level l; grad_attn and grad_loc at [..., l, ...]): max|err| <=
    max(2 x the fp32 yardstick's error, 5e-6 x s), s = max|float64 slice| (no floor of 1: the gradients reaching the
    encoder are far below 1) -- 2e-5 x s for the column kernel's grad_value, the resolution of its fixed-point sums; an
    all-zero float64 slice must come out exactly zero.  grad_loc is scored against the
    nearer of the two one-sided float64 candidates (callsite_reference.msda_backward), the yardstick likewise; nothing
    is masked;
  * LSAP: status 0, every assignment an injection, identical to scipy's linear_sum_assignment on the costs widened to
    float64, or else of exactly the same float64 total (a tie).

Observed on the MI355X, largest error / yardstick-error over the six runs (run with -rP to print them per test): backward
grad_attn col 1.90 / generic 1.10, grad_loc col 2.11 / generic 1.10 (above 2 only where the 5e-6 x s floor is the bound),
grad_value generic 2.06 and col 10-47 (at most 6.8e-6 x s: the fixed-point resolution, see COL_GRAD_VALUE_FLOOR); unfused
forward 1.17; the torch fall-backs linear 1.00, conv1x1_nchw 3.73 (floor-bound).  Families: forward quad-owner everywhere,
backward column for configs[2] / [3] and generic for the small run.  Two-candidate grad_loc coordinates: 31.4 % at init for
configs[2] / [3], 30.0 % for the small run, 0.02 % with model-like offsets.  LSAP: one launch of 10 problems per image,
every assignment identical to scipy's, no ties.  The file takes about 26 s, half of it the first ResNet-50 step (MIOpen's
first-call search for its convolutions)."""
import math
import time

import numpy as np
import pytest
import torch

import callsite_reference as ref
from callsite_capture import ENTRY_POINTS, TRAINING_ENTRIES, CallsiteCapture
from callsite_check import K_DPP, Report
from callsite_check import check as _check

pytestmark = pytest.mark.gpu

B_GENERIC, B_COL = 2, 3


@pytest.fixture
def no_tf32(monkeypatch):
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)

# name -> (ResNet depth, batch, H, W, queries, targets per image, dataset)
CONFIGS = {
    "cfg2_cvppp_448_q100": (50, 2, 448, 448, 100, 20, "CVPPP"),
    "cfg3_bbbc_512_q300": (50, 2, 512, 512, 300, 60, "BBBC"),
    "r18_256x320_q50": (18, 1, 256, 320, 50, 8, "CVPPP"),
}

# MSDeformAttn families `auto` takes.  Forward: 3 levels stay below the column threshold (N*S*M 65 856 / 86 016 /
# 13 440 < 450 000) and fill fewer than 3 x 768 windowed items -> quad-owner.  Backward: the column kernel from
# N*S*M >= 32 768 (msda_backward_col.hip), below that the windowed kernel declines too -> generic.
FWD_FAMILY = {name: K_DPP for name in CONFIGS}
BWD_FAMILY = {"cfg2_cvppp_448_q100": B_COL, "cfg3_bbbc_512_q300": B_COL, "r18_256x320_q50": B_GENERIC}


def _expected():
    """Calls per entry point of one training step: 6 encoder layers, each one unfused forward, one backward and one
    `fused_ops.linear` (value_proj, which falls back to the module under autograd); the input projection's three
    `conv1x1_nchw` (falling back to the module likewise); the matcher's one LSAP launch for all prediction heads.  Every
    forward-only fused entry: none."""
    e = dict.fromkeys(ENTRY_POINTS + TRAINING_ENTRIES, 0)
    e.update({"MSDA.ms_deform_attn_forward": 6, "MSDA.ms_deform_attn_backward": 6, "fused_ops.lsap": 1,
              "fused_ops.linear": 6, "fused_ops.conv1x1_nchw": 3})
    return e


def _build(name, state):
    from pctrans_amd.arch import maskformer as mfm
    from pctrans_amd.arch.resnet import ResNet
    from pctrans_amd.config import get_cfg
    depth, N, H, W, Q, G, dataset = CONFIGS[name]
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=Q, norm="BN", sem_norm="BN", dataset=dataset)
    model = mfm.MaskFormer(**mfm.MaskFormer.from_config(cfg, ResNet(depth, 3, norm="BN"))).cuda().train()
    vol = torch.randn(N, 3, H, W, device="cuda")
    g = torch.Generator().manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    targets = []
    for _ in range(N):
        cy, cx = torch.randint(20, H - 20, (G,), generator=g), torch.randint(20, W - 20, (G,), generator=g)
        r = torch.randint(6, 16, (G,), generator=g)
        masks = torch.stack([(((yy - int(y)) ** 2 + (xx - int(x)) ** 2) <= int(q) ** 2).float() for y, x, q in zip(cy, cx, r)])
        centers = torch.stack([cx.float() / W, cy.float() / H], -1).view(G, 1, 2).cuda()
        targets.append({"masks": masks, "labels": torch.ones(G, dtype=torch.long, device="cuda"),
                        "fg_masks": (masks.sum(0) > 0).float(), "center_points": centers})
    if state == "M":
        import bench
        with torch.no_grad():
            feats = model.backbone(vol)
        bench.model_like_offsets(model.sem_seg_head, feats)
        del feats
    return model, vol, targets


# ---------------------------------------------------------------- backward
class Tally:
    """Failures (collected, so that one run shows all of them), two-candidate coordinates, LSAP outcomes."""

    def __init__(self):
        self.failures, self.two, self.coords, self.identical, self.ties = [], 0, 0, 0, 0


# the column kernel sums grad_value in integers: every contribution is rounded to 2^-21..2^-20 of the item's bound
# max|grad_out| * max|attn| (msda_backward_col.hip), documented as 2e-5 of the gradient's own magnitude
# (test_msda_bwd_col_gpu.py).  Observed here: 11-42x the fp32 yardstick, up to 6.8e-6 x s -- above the 5e-6 x s floor.
COL_GRAD_VALUE_FLOOR = 2e-5


def _grad_bound(got, cands, yard, what, report, kind, tally, floor=5e-6):
    """`cands` [..., K]: the float64 candidates of every element (K = 1: continuous)."""
    got, yard = got.double(), yard.double()
    s = float(cands.abs().max())
    if s == 0.0:
        if bool((got != 0).any()):
            tally.failures.append("%s: float64 slice is zero, output max|.| %.3g" % (what, float(got.abs().max())))
        return
    if not bool(torch.isfinite(got).all()):
        tally.failures.append("%s: non-finite output" % what)
        return
    err = float((got[..., None] - cands).abs().min(-1).values.max())
    err32 = float((yard[..., None] - cands).abs().min(-1).values.max())
    bound = max(2.0 * err32, floor * s)
    report.note("backward", kind, err / max(err32, 1e-300))
    if err > bound:
        tally.failures.append("%s: max|err| %.3g > %.3g (fp32 yardstick %.3g, scale %.3g)" % (what, err, bound, err32, s))


def _check_backward(call, report, tally):
    a = call.args
    ops = (a["value"], a["spatial_shapes"], a["level_start_index"], a["sampling_loc"], a["attn_weight"], a["grad_output"])
    gv64, gl64, ga64 = ref.msda_backward(*ops)
    gv32, gl32, ga32 = ref.msda_backward(*ops, dtype=torch.float32, delta=0)
    gv, gl, ga = call.out
    assert gv.shape == gv64.shape and gl.shape == gl64.shape[:-1] and ga.shape == ga64.shape
    tally.two += int((gl64[..., 0] != gl64[..., 1]).sum())
    tally.coords += gl.numel()
    fam = {B_COL: "col", B_GENERIC: "generic"}.get(call.kernel, str(call.kernel))
    starts = a["level_start_index"].tolist()
    for l, (H, W) in enumerate(a["spatial_shapes"].tolist()):
        rows = slice(starts[l], starts[l] + H * W)
        what = "backward level %d (%dx%d)" % (l, H, W)
        _grad_bound(gv[:, rows], gv64[:, rows, ..., None], gv32[:, rows], what + " grad_value", report,
                    "grad_value/" + fam, tally, COL_GRAD_VALUE_FLOOR if call.kernel == B_COL else 5e-6)
        _grad_bound(ga[:, :, :, l], ga64[:, :, :, l, :, None], ga32[:, :, :, l], what + " grad_attn", report,
                    "grad_attn/" + fam, tally)
        _grad_bound(gl[:, :, :, l], gl64[:, :, :, l], gl32[:, :, :, l, ..., 0], what + " grad_loc", report,
                    "grad_loc/" + fam, tally)


# ---------------------------------------------------------------- LSAP
def _check_lsap(call, tally):
    from scipy.optimize import linear_sum_assignment
    cost = call.args["cost"].double().cpu().numpy()
    counts = call.args["num_target"].cpu().numpy()
    rows, status = (t.cpu().numpy() for t in call.out)
    B, Q, _ = cost.shape
    assert (status == 0).all(), status
    for b in range(B):
        g, r = int(counts[b]), rows[b]
        assert (r[g:] == -1).all() and ((r[:g] >= 0) & (r[:g] < Q)).all() and len(set(r[:g].tolist())) == g, (b, r)
        ri, ci = linear_sum_assignment(cost[b, :, :g])
        want = np.full(g, -1)
        want[ci] = ri
        if np.array_equal(r[:g], want):
            tally.identical += 1
        else:
            got_total = math.fsum(cost[b, r[:g], np.arange(g)])
            want_total = math.fsum(cost[b, want, np.arange(g)])
            if got_total != want_total:
                tally.failures.append("lsap problem %d: total %.17g, scipy %.17g" % (b, got_total, want_total))
            tally.ties += 1


# ---------------------------------------------------------------- the step
@pytest.mark.parametrize("state", ["init", "M"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_training_kernel_call_matches_float64(monkeypatch, no_tf32, name, state):
    t0 = time.perf_counter()
    model, vol, targets = _build(name, state)
    cap = CallsiteCapture(entries=ENTRY_POINTS + TRAINING_ENTRIES).install(monkeypatch)
    losses = model(vol, targets, True)
    total = sum(v for v in losses.values() if torch.is_tensor(v))
    total.backward()
    torch.cuda.synchronize()
    t_step = time.perf_counter() - t0
    counts = cap.counts()
    assert counts == _expected(), {k: v for k, v in counts.items() if v != _expected()[k]}
    report, tally = Report("%s %s" % (name, state)), Tally()
    fams = {}
    for e, calls in cap.calls.items():
        for c in calls:
            if e == "MSDA.ms_deform_attn_backward":
                fams.setdefault("bwd", set()).add(c.kernel)
                assert c.kernel == BWD_FAMILY[name], "backward ran family %d, expected %d" % (c.kernel, BWD_FAMILY[name])
                _check_backward(c, report, tally)
            elif e == "fused_ops.lsap":
                assert c.args["cost"].shape[0] % CONFIGS[name][1] == 0
                _check_lsap(c, tally)
            else:
                if c.kernel is not None:
                    fams.setdefault("fwd", set()).add(c.kernel)
                    assert c.kernel == FWD_FAMILY[name], "%s ran family %d, expected %d" % (e, c.kernel, FWD_FAMILY[name])
                _check(c, report)
            del c.args, c.out
    torch.cuda.synchronize()
    report.show()
    print("[training] %s %s: families %s, two-candidate grad_loc coordinates %d / %d (%.2f %%), lsap identical %d, "
          "ties %d, step + capture %.1f s, checks %.1f s" % (
              name, state, {k: sorted(v) for k, v in fams.items()}, tally.two, tally.coords,
              100.0 * tally.two / max(1, tally.coords), tally.identical, tally.ties, t_step, time.perf_counter() - t0 - t_step))
    assert not tally.failures, "\n".join(tally.failures[:40])

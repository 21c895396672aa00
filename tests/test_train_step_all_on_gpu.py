"""GPU: one training step of the whole model with EVERY device path of the loss side and the decoder side on at once
(tests/train_switches.py: dmh_train, attn_train, reid_dice, point_loss / matcher.point_sample, point_select, match_cost, emb_loss,
loss_heads / cost_heads = "batched", targets from label maps in "hip" mode), against the same step on the torch chain and a
float64 arbiter.  Each switch has a test of its own on hand-built operands; here the paths hand tensors to each other: the
TargetList's planes and index vectors go to the matcher's and the criterion's caches and to the embedding loss, the HIP mask
head's logits feed the batched costs, the selection kernel, the batched loss and the re-id dice rows, the batched costs decide the
pairs all of them use, draw_head_coords draws behind the matcher, and autograd sums four HIP backwards into the same mask
features and query embeddings.

Model: get_cfg(num_queries=12, norm="BN", sem_norm="BN", enc_layers=2, dec_layers=4, train_num_points=512, dataset="BBBC") on a
ResNet-18, 2 x 3 x 128 x 128, TF32 off.  DEC_LAYERS counts the query-feature prediction, so the decoder has dec_layers - 1 = 3
layers and dec_layers = 4 prediction heads; every count below is derived from the decoder, none is a literal.  Targets come from
MaskFormer.prepare_instance_targets on int64 label maps; the second image's labels are not ascending in raster order.

Runs of one step (forward, losses, backward; no graph capture), each seeded with torch.manual_seed and random.seed:
    off   fp32, train_switches.all_off, targets in "torch" mode
    on    fp32, train_switches.all_on, targets in "hip" mode
    f64   copy.deepcopy(model).double(), all_off, targets in "torch" mode: the arbiter.  torch.rand draws fp32 and widens, so
          the random numbers are those of the fp32 runs.  The position encodings of both decoders and gen_sineembed_for_position
          build fp32 constants: their outputs are widened (the hooks of test_dmh_train_gpu.py).  The model calls `.float()` in
          many places (the pixel decoder runs "in fp32" on purpose, the reference-point update, the matcher's costs, the
          contrast items' cosines): for this run alone Tensor.float leaves a float64 tensor as it is, so nothing of the arbiter is
          rounded to fp32.  Its matcher assigns with scipy on the float64 costs (device_lsap = False: the LSAP kernel is fp32).

Assertions (all failures of a step are collected and shown together):
  * the paths ran: with everything on every wrapper of train_switches.SWITCHES is entered and no torch-side counterpart is, with
    everything off the other way round; heads mask-head backwards, layers cross-attention forwards and backwards, one *_many call
    each for selection, loss and cost, one embedding-loss forward and backward, one device target build, no per-head wrapper;
  * discrete decisions: indices_list of every head and image, the sampled points of every head (the uncertain ones as a set per
    pair, the random tail bit for bit), the query-contrast plan, Python's random state and torch's generator state are the same in
    all three runs.  off == f64 is a precondition on the inputs -- the run seed is the first of 0, 1, 2, ... for which it holds --
    and on == off is the finding under test.  The float64 margins that make the seed safe are printed: per LSAP problem the gap
    between the best and the second-best assignment total (all injections enumerated), per pair the gap between the last admitted
    and the first rejected uncertainty key;
  * values, for every entry of the loss dict, every parameter gradient and the input volume's gradient:
    |on - off| <= max(2 |off - f64|, 5e-6 max|f64|) (test_dmh_train_gpu.py, test_callsite_training_gpu.py); a gradient that is
    zero in exact arithmetic (a key-projection bias, recognised as test_dmh_train_gpu.py recognises it) |on - off| <= 4 |off - f64|;
    the same parameters have a gradient.
Three steps with changing targets: three models from the same weights (off, on, f64), a fresh target list per step from (3, 3),
(2, 4) and (4, 1) instances -- the previous list dropped first, so the allocator may reuse its addresses under the caches keyed on
data_ptr / _version -- and all of the above per step.  After each step every model takes a plain SGD update (lr 1e-3, no momentum)
of its own gradients and the value bound is applied to every parameter; then all three models go back to the initial weights and
buffers, in place, so each parameter's _version moves twice per step under the weight-keyed caches.  The steps do not continue
from the updated weights: on this untrained model the first gradient has norm 2.7e3 and the updated weights sit on decision
thresholds.  Measured with all models re-synchronised to the off model's updated weights after each step and one seed for the
sequence: seeds 0 .. 4 break the precondition off == f64 (0 at the second step, in the query-contrast positives, for every seed of
that step as well; 1 .. 4 at the third, 6-15 uncertain points of a pair); seed 5 is the first that meets it at all three steps,
and there one gradient of the third step (the last decoder FFN's norm.weight) has |on - off| 6.26e-6 against a bound of 5.11e-6,
with the torch chain's own run-to-run rounding (below) of that order.  That sequence is not in the suite.  A last step has an image without instances and runs under bf16 autocast, where
the predictions are bf16 and the paths give way as its test lists.

Settings of every run: TF32 off, torch.backends.cudnn.deterministic and torch.use_deterministic_algorithms(warn_only), all put
back afterwards.  Without the second the torch chain does not repeat its own forward on the MI355X (other loss bits, under
autocast other assignments).  With them the losses and every discrete decision repeat bit for bit.  The gradients do not: torch
has no deterministic backward for grid_sample and bilinear upsampling (warn_only lets them run), so two off runs differ by
rounding in 239 of 251 gradients and two on runs in 91.  The value bound is measured against one off run.

Found by this file: emb_loss = "hip" never reached its kernels in a whole model.  The pixel embedding the model hands to the
criterion is the pixel decoder's mask_features: CONVS_DIM = 128 channels (both shipped yamls) where the kernels covered 32, and
channels-last where they read [B, E, h, w] planes -- for either reason SetCriterion._loss_embedding_hip gave way to the torch chain
without a word.  The kernels now take the channels in tiles of 32 up to 128 and the criterion copies a channels-last embedding
once, inside autograd (tests/test_embedding_loss_gpu.py: test_more_than_32_channels_against_float64,
test_guard_bands_of_the_wide_layouts, test_set_criterion_copies_a_channels_last_embedding).

Run with -rP for the figures; PCT_TRAIN_ALL_ON_REPORT=<file> writes the worst |on - off| / |off - f64| per loss, gradient and
parameter and the margins as JSON.

Observed on the MI355X (run seed 0 everywhere: the first that meets the precondition):
  * float64 margins, smallest over the problems / pairs of a step: assignment totals (of ~27-37) best to second-best 2.6e-2
    (3, 3), 1.7e-2 (2, 4), 6.4e-2 (4, 1); uncertainty keys 5.0e-5, 7.5e-5, 6.2e-5 (logits of order 1: 500 fp32 ulps); no
    attention-mask bit differs between any two runs of a step;
  * worst |on - off| / |off - f64|: losses 3-7 on the (3, 3) step (loss_reid_mask, loss_dice_2), 43 (loss_reid_query_aux at
    (2, 4)) and 25 (loss_reid_query at (4, 1)), each where |off - f64| is a few 1e-8 and 5e-6 max|f64| is the bound; gradients
    1.8-2.5 per step, above 2 for at most 19 of the 251 tensors (the floor, or the zero rule of the key-projection biases, is
    the bound there); the autocast step 0.22 / 2.25.
Breaking a seam on a scratch copy (the per-switch tests of the loss side run beside it):
  * `tgt` off by one plane in _loss_masks_batched: test_one_step_values and test_three_steps_values fail ("loss loss_mask:
    |on - off| 1.784e-01 > 3.990e-05", every mask loss and every gradient); of the per-switch tests
    test_loss_heads_gpu.py::test_criterion_batched_against_each fails too;
  * one torch.rand of draw_head_coords not drawn: the *_paths_and_decisions tests fail ("head 1: the random tail of the sampled
    points differs", "head 2 pair 0: 384 uncertain points differ", the generator's final state); the same per-switch test fails too;
  * _hip_target_planes returning its cached planes for a changed key: test_three_steps_values fails at the second step ("loss
    loss_mask_1: |on - off| 0.176 > 1.56e-05", 60 entries, up to 1e4 x the bound); all 149 per-switch tests pass.
"""
import atexit
import contextlib
import copy
import itertools
import json
import os
import random
import warnings

import numpy as np
import pytest
import torch

import train_switches as TS

pytestmark = pytest.mark.gpu

H = W = 128
SEED_ONE = 0          # single step, (3, 3) instances
SEEDS_STEPS = [0, 0, 0]   # three steps with changing targets: per step the first seed for which off == f64
SEED_EMPTY = 0        # the step with an empty image under autocast (its float64 run is no precondition: see the test)
STEP_COUNTS = [(3, 3), (2, 4), (4, 1)]

_FIGURES = {}


def _report():
    path = os.environ.get("PCT_TRAIN_ALL_ON_REPORT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump(_FIGURES, f, indent=1, sort_keys=True)


atexit.register(_report)


# ---------------------------------------------------------------- model, inputs
def build_model(dev="cuda"):
    from pctrans_amd.arch import maskformer as mfm
    from pctrans_amd.arch.resnet import ResNet
    from pctrans_amd.config import get_cfg
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=12, norm="BN", sem_norm="BN", enc_layers=2, dec_layers=4, train_num_points=512, dataset="BBBC")
    model = mfm.MaskFormer(**mfm.MaskFormer.from_config(cfg, ResNet(18, 3, norm="BN"))).to(dev).train()
    assert TS._heads(model) == cfg.MODEL.MASK_FORMER.DEC_LAYERS and TS._layers(model) == cfg.MODEL.MASK_FORMER.DEC_LAYERS - 1
    vol = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    return model, vol


def make64(model):
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    m64 = TS.all_off(copy.deepcopy(model).double())
    for m in m64.modules():
        if isinstance(m, dec.PositionEmbeddingSine):
            m.register_forward_hook(lambda mod, i, o: o.double())
    m64.criterion.matcher.device_lsap = False
    return m64


BOXES = [(10, 40, 12, 44), (20, 52, 70, 110), (70, 110, 16, 50), (76, 120, 66, 100)]     # y0, y1, x0, x1
LABELS = [[1, 2, 3, 4], [9, 4, 6, 2]]          # image 1: not ascending in raster order; the masks come in ascending label order


def label_maps(counts):
    """The loader's CPU label maps [2, H, W] int64 with counts[b] rectangular instances in image b (0: none at all)."""
    maps = torch.zeros((2, H, W), dtype=torch.int64)
    for b, n in enumerate(counts):
        for k in range(n):
            y0, y1, x0, x1 = BOXES[k]
            maps[b, y0 + 3 * b:y1 - 2 * b, x0 + 5 * b:x1 + 4 * b] = LABELS[b][k]
    return maps


# ---------------------------------------------------------------- one run
@contextlib.contextmanager
def _patched(owner, attr, new):
    had, before = attr in vars(owner), vars(owner).get(attr)
    setattr(owner, attr, new)
    try:
        yield
    finally:
        if had:
            setattr(owner, attr, before)
        else:
            delattr(owner, attr)


def _rng_state(dev):
    return torch.cuda.get_rng_state() if torch.device(dev).type == "cuda" else torch.get_rng_state()


def run_step(model, vol, maps, mode, seed, autocast=False):
    """One step of `model` in `mode` ("off", "on", "f64") -> a record of everything the tests compare.  The model's switches are
    set here; the targets are built here from `maps` and dropped before returning."""
    from pctrans_amd import point_loss
    from pctrans_amd.loss import maskformer_criterion as crit
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    from pctrans_amd.transformer_decoder import query_contrast as qc
    on, f64 = mode == "on", mode == "f64"
    (TS.all_on if on else TS.all_off)(model)
    decoder = model.sem_seg_head.predictor
    rec = {"mode": mode, "coords": [], "plans": [], "attn": [], "costs": [], "keys": []}
    real = {"many": point_loss.point_mask_losses_many, "each": point_loss.point_mask_losses,
            "torch": crit.get_uncertain_point_coords_with_randomness, "plan": qc._plan, "rand": torch.rand,
            "float": torch.Tensor.float, "sine": dec.gen_sineembed_for_position, "unc": crit.calculate_uncertainty,
            "head": decoder.dynamic_mask_with_coords, "criterion": model.criterion.forward,
            "costs": model.criterion.matcher._batched_costs}

    def many(preds, src, planes, tgt, coords, num_masks):
        rec["coords"] += [c.detach().double().cpu() for c in coords]
        return real["many"](preds, src, planes, tgt, coords, num_masks)

    def each(pred, src, planes, tgt, coords, num_masks):
        rec["coords"].append(coords.detach().double().cpu())
        return real["each"](pred, src, planes, tgt, coords, num_masks)

    def chain(*a, **k):
        coords = real["torch"](*a, **k)
        rec["coords"].append(coords.detach().double().cpu())
        return coords

    def plan(*a, **k):
        got = real["plan"](*a, **k)
        rec["plans"].append(copy.deepcopy(got))
        return got

    def head(*a, **k):
        out = real["head"](*a, **k)
        rec["attn"].append(out[1].detach().cpu())
        return out

    def criterion(outputs, targets, *a, **k):
        rec["indices"] = [[(s.tolist(), t.tolist()) for s, t in ind] for ind in outputs["indices_list"]]
        rec["pred_dtypes"] = [outputs["pred_masks"].dtype] + [o["pred_masks"].dtype for o in outputs["aux_outputs"]]
        rec["contrast_items"] = (len(outputs["pred_qd_query"]), len(outputs["pred_qd_mask"]))
        return real["criterion"](outputs, targets, *a, **k)

    def costs(outputs, targets):
        got = real["costs"](outputs, targets)
        rec["costs"].append((got[0].detach().double().cpu(), list(got[1])))
        return got

    def uncertainty(logits):
        out = real["unc"](logits)
        rec["keys"].append(out.detach()[:, 0].double().cpu())
        return out

    with contextlib.ExitStack() as stack:
        stack.enter_context(_patched(point_loss, "point_mask_losses_many", many))
        stack.enter_context(_patched(point_loss, "point_mask_losses", each))
        stack.enter_context(_patched(crit, "get_uncertain_point_coords_with_randomness", chain))
        stack.enter_context(_patched(qc, "_plan", plan))
        stack.enter_context(_patched(decoder, "dynamic_mask_with_coords", head))
        stack.enter_context(_patched(model.criterion, "forward", criterion))
        if f64:
            stack.enter_context(_patched(torch, "rand", lambda *a, **k: real["rand"](*a, **k).double()))
            stack.enter_context(_patched(torch.Tensor, "float", lambda t, *a, **k: t if t.dtype == torch.float64
                                         else real["float"](t, *a, **k)))
            stack.enter_context(_patched(dec, "gen_sineembed_for_position",
                                         lambda p, *a, **k: real["sine"](p, *a, **k).to(p.dtype)))
            stack.enter_context(_patched(model.criterion.matcher, "_batched_costs", costs))
            stack.enter_context(_patched(crit, "calculate_uncertainty", uncertainty))
        before = os.environ.get("PCT_TARGETS")
        os.environ["PCT_TARGETS"] = TS.targets_mode(on)
        stack.callback(lambda: os.environ.pop("PCT_TARGETS") if before is None else os.environ.__setitem__("PCT_TARGETS", before))
        watch = stack.enter_context(TS.Watch(model))         # (last: it counts calls from the model, not from the spies above)
        random.seed(seed)
        torch.manual_seed(seed)
        targets = model.prepare_instance_targets(maps)
        rec["handed"] = getattr(targets, "planes", None) is not None
        x = (vol.double() if f64 else vol).detach().clone().requires_grad_(True)
        with torch.autocast(torch.device(vol.device).type, dtype=torch.bfloat16, enabled=autocast and not f64):
            losses = model(x, targets, True)
        total = sum(v for v in losses.values() if torch.is_tensor(v))
        model.zero_grad(set_to_none=True)
        total.backward()
        if vol.is_cuda:
            torch.cuda.synchronize()
        rec["counts"] = dict(watch.counts)
    rec["losses"] = {k: v.detach().double().cpu() for k, v in losses.items() if torch.is_tensor(v)}
    rec["grads"] = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
    rec["grads"]["input volume"] = x.grad.detach().double().cpu()
    rec["rng"], rec["random"] = _rng_state(vol.device), random.getstate()
    rec["num_uncertain"] = int(model.criterion.importance_sample_ratio * model.criterion.num_points)
    del targets, losses, total
    return rec


# ---------------------------------------------------------------- the checks
def check_paths(model, rec, fails, only=None, skip=()):
    """Which functions of train_switches.SWITCHES a run entered: a device path that silently falls back shows here."""
    c, what = rec["counts"], "[%s] " % rec["mode"]
    if rec["mode"] == "on":
        wrappers, torch_side = TS.labels("wrappers", only, skip), TS.labels("torch_side", only, skip)
        fails += [what + "torch-side %s ran %d times with every switch on" % (k, c[k]) for k in torch_side if c[k]]
        fails += [what + "wrapper %s was never entered" % k for k in wrappers if not c[k]]
        fails += [what + "per-head wrapper %s ran %d times beside the batched path" % (k, c[k])
                  for k in TS.labels("superseded", only, skip) if c[k]]
        for k, n in TS.expected_counts(model, only, skip).items():
            if c[k] != n:
                fails.append(what + "%s entered %d times, the model's structure gives %d" % (k, c[k], n))
        if not rec["handed"]:
            fails.append(what + "the target list carries no planes")
    else:
        wrappers, torch_side = TS.labels("wrappers") + TS.labels("superseded"), TS.labels("torch_side")
        fails += [what + "wrapper %s ran %d times with every switch off" % (k, c[k]) for k in wrappers if c[k]]
        fails += [what + "torch-side %s was never entered" % k for k in torch_side if not c[k]]
        if rec["handed"]:
            fails.append(what + "a torch-mode target list carries planes")


def check_discrete(a, b, fails, rng=True):
    """Everything a step decides discretely, run `a` against run `b`."""
    what = "[%s vs %s] " % (a["mode"], b["mode"])
    if a["indices"] != b["indices"]:
        differ = [h for h, (x, y) in enumerate(zip(a["indices"], b["indices"])) if x != y]
        fails.append(what + "indices_list differs at heads %s: %s / %s" % (differ, a["indices"][differ[0]], b["indices"][differ[0]]))
    if len(a["coords"]) != len(b["coords"]) or any(x.shape != y.shape for x, y in zip(a["coords"], b["coords"])):
        fails.append(what + "sampled points: %s / %s" % ([tuple(x.shape) for x in a["coords"]], [tuple(x.shape) for x in b["coords"]]))
    else:
        nu = a["num_uncertain"]
        for h, (x, y) in enumerate(zip(a["coords"], b["coords"])):
            if not torch.equal(x[:, nu:], y[:, nu:]):
                fails.append(what + "head %d: the random tail of the sampled points differs" % h)
            for k in range(x.shape[0]):
                sx, sy = set(map(tuple, x[k, :nu].tolist())), set(map(tuple, y[k, :nu].tolist()))
                if sx != sy:
                    fails.append(what + "head %d pair %d: %d uncertain points differ" % (h, k, len(sx - sy)))
    if a["plans"] != b["plans"] or a["contrast_items"] != b["contrast_items"]:
        fails.append(what + "query-contrast items differ: %s / %s" % (a["plans"], b["plans"]))
    if a["random"] != b["random"]:
        fails.append(what + "Python's random was consumed differently")
    if rng and not torch.equal(a["rng"], b["rng"]):
        fails.append(what + "the generator's final state differs")
    flips = sum(int((x != y).sum()) for x, y in zip(a["attn"], b["attn"]))
    print("%sattention-mask bits that differ: %d of %d" % (what, flips, sum(x.numel() for x in a["attn"])))


_INJECTIONS = {}


def lsap_margins(rec):
    """Per LSAP problem of the float64 run: (second-best - best assignment total, best total), all injections enumerated."""
    out = []
    for cost, counts in rec["costs"]:
        cost = cost.numpy()
        for b, g in enumerate(counts):
            Q = cost.shape[1]
            if (Q, g) not in _INJECTIONS:
                _INJECTIONS[(Q, g)] = np.array(list(itertools.permutations(range(Q), g)))
            totals = np.sort(cost[b][_INJECTIONS[(Q, g)], np.arange(g)].sum(1))
            out.append((float(totals[1] - totals[0]), float(totals[0])))
    return out


def key_margins(rec):
    """Per pair of the float64 run: the gap between the last admitted and the first rejected uncertainty key -|logit|."""
    nu = rec["num_uncertain"]
    out = []
    for keys in rec["keys"]:
        top = torch.sort(keys, dim=1, descending=True).values
        out += (top[:, nu - 1] - top[:, nu]).tolist()
    return out


def print_margins(rec64, tag):
    lm, km = lsap_margins(rec64), key_margins(rec64)
    print("[%s] float64 margins: LSAP best-to-second gap min %.3e (of totals ~%.3g, %d problems); uncertainty-key gap min %.3e "
          "(%d pairs)" % (tag, min(m for m, _ in lm), float(np.mean([t for _, t in lm])), len(lm), min(km), len(km)))
    _FIGURES.setdefault(tag, {})["margins"] = {"lsap_gap_min": min(m for m, _ in lm), "key_gap_min": min(km)}
    return lm, km


def _bound(name, x_on, x_off, x_64, fails, worst, tag, zero_rule=False):
    err = float((x_on - x_off).abs().max())
    yerr = float((x_off - x_64).abs().max())
    top = float(x_64.abs().max())
    if not (bool(torch.isfinite(x_on).all()) and bool(torch.isfinite(x_off).all()) and bool(torch.isfinite(x_64).all())):
        fails.append("[%s] %s: non-finite values" % (tag, name))
        return
    ratio = 0.0 if err == 0.0 else (err / yerr if yerr > 0 else float("inf"))
    worst[name] = ratio
    bound = 4.0 * yerr if zero_rule else max(2.0 * yerr, 5e-6 * top)
    if err > bound:
        fails.append("[%s] %s%s: |on - off| %.3e > %.3e (|off - f64| %.3e, max|f64| %.3e)" % (
            tag, name, " (zero in exact arithmetic)" if zero_rule else "", err, bound, yerr, top))


def check_values(on, off, f64, fails, tag):
    """The value bound on every loss, every parameter gradient and the input's gradient; prints the worst ratios."""
    if not (on["losses"].keys() == off["losses"].keys() == f64["losses"].keys()):
        fails.append("[%s] loss dicts differ: %s / %s / %s" % (tag, sorted(on["losses"]), sorted(off["losses"]), sorted(f64["losses"])))
        return
    worst_loss, worst_grad = {}, {}
    for k in off["losses"]:
        _bound("loss " + k, on["losses"][k], off["losses"][k], f64["losses"][k], fails, worst_loss, tag)
    if on["grads"].keys() != off["grads"].keys():
        fails.append("[%s] parameters with a gradient differ: %s" % (tag, sorted(on["grads"].keys() ^ off["grads"].keys())))
    g64 = f64["grads"]
    for n in off["grads"]:
        if n not in on["grads"] or n not in g64:
            if n not in g64:
                fails.append("[%s] grad %s: the float64 run has none" % (tag, n))
            continue
        sib = n[:-len("bias")] + "weight"
        zero = n.endswith(".bias") and sib in g64 and float(g64[n].abs().max()) < 1e-12 * float(g64[sib].abs().max())
        _bound("grad " + n, on["grads"][n], off["grads"][n], g64[n], fails, worst_grad, tag, zero_rule=zero)
    show(tag, "loss", worst_loss)
    show(tag, "grad", worst_grad)


def sgd_and_resync(models, optimizers, state=None):
    """Each model takes its own SGD update -> {mode: its parameters afterwards}.  Then all of them take the weights and buffers of
    `state` (default: those of "off" after its update), so that the next step compares one step and not three histories.
    load_state_dict copies in place: with the update, every parameter's _version moves twice under the weight-keyed caches."""
    after = {}
    for k, m in models.items():
        optimizers[k].step()
        after[k] = {n: p.detach().double().cpu() for n, p in m.named_parameters()}
    state = models["off"].state_dict() if state is None else state
    for m in models.values():
        m.load_state_dict(state)
    return after


def check_params(after, f64_grads, fails, tag):
    """The value bound on every parameter after the update (the zero rule where the gradient is zero in exact arithmetic)."""
    worst = {}
    if not (after["on"].keys() == after["off"].keys() == after["f64"].keys()):
        fails.append("[%s] parameter names differ" % tag)
        return
    for n in after["off"]:
        sib = n[:-len("bias")] + "weight"
        zero = (n.endswith(".bias") and n in f64_grads and sib in f64_grads
                and float(f64_grads[n].abs().max()) < 1e-12 * float(f64_grads[sib].abs().max())
                and float(after["f64"][n].abs().max()) < 1e-12 * float(after["f64"][sib].abs().max()))
        _bound("param " + n, after["on"][n], after["off"][n], after["f64"][n], fails, worst, tag, zero_rule=zero)
    show(tag, "param", worst)


def show(tag, kind, worst):
    _FIGURES.setdefault(tag, {})[kind] = worst
    top = sorted(worst.items(), key=lambda kv: -kv[1])
    print("[%s] worst |on - off| / |off - f64| per %s: %s%s" % (
        tag, kind, ", ".join("%s %.3g" % (k.split(" ", 1)[1], v) for k, v in top[:8]), " ..." if len(top) > 8 else ""))


def check_decisions(model, on, off, f64, tag, precondition=True):
    """The paths each run took and everything it decided discretely -> the failures of on against off."""
    fails = []
    check_paths(model, on, fails)
    check_paths(model, off, fails)
    check_paths(model, f64, fails)
    if precondition:
        pre = []
        check_discrete(off, f64, pre)
        print_margins(f64, tag)
        assert not pre, "[%s] precondition off == f64 does not hold at this seed:\n" % tag + "\n".join(pre[:20])
    check_discrete(on, off, fails)
    return fails


# ---------------------------------------------------------------- the steps, run once per module
@contextlib.contextmanager
def _settings():
    """TF32 off; MIOpen's deterministic convolution algorithms, without which the torch chain does not repeat its own forward
    (module text)."""
    before = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32, torch.backends.cudnn.deterministic
    algos = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    torch.backends.cudnn.deterministic = True
    # torch's own deterministic kernels wherever it has one (index and scatter adds, the embedding's backward); warn_only because
    # grid_sample's and the bilinear upsampling's backward have none and would raise
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message=".*does not have a deterministic implementation.*")
            yield
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32, torch.backends.cudnn.deterministic = before
        torch.use_deterministic_algorithms(algos[0], warn_only=algos[1])


@pytest.fixture(scope="module")
def one_step():
    """off, on and f64 of one step on the same weights and inputs, (3, 3) instances."""
    with _settings():
        model, vol = build_model()
        m64 = make64(model)
        maps = label_maps((3, 3))
        return model, {"off": run_step(model, vol, maps, "off", SEED_ONE), "on": run_step(model, vol, maps, "on", SEED_ONE),
                       "f64": run_step(m64, vol, maps, "f64", SEED_ONE)}


LR = 1e-3


def sgd(model):
    return torch.optim.SGD(model.parameters(), lr=LR, momentum=0.0)


@pytest.fixture(scope="module")
def three_steps():
    """Three models from the same weights (off, on, f64), three steps, a fresh target list per step from (3, 3), (2, 4) and (4, 1)
    instances -- the previous list is dropped before the next is built, so the allocator may reuse its addresses under the
    matcher's and the criterion's caches keyed on data_ptr / _version.  After each step every model takes a plain SGD update (lr
    1e-3, no momentum) of its own gradients, its parameters are kept for the value bound, and all three go back to the initial
    weights and buffers in place (module text: what continuing from the updated weights gave)."""
    with _settings():
        base, vol = build_model()
        initial = copy.deepcopy(base.state_dict())       # (with its _metadata: the model renames keys of old versions)
        models = {"off": base, "on": copy.deepcopy(base), "f64": make64(base)}
        optimizers = {k: sgd(m) for k, m in models.items()}
        steps = []
        for s, counts in enumerate(STEP_COUNTS):
            r = {k: run_step(models[k], vol, label_maps(counts), k, SEEDS_STEPS[s]) for k in ("off", "on", "f64")}
            r["params"] = sgd_and_resync(models, optimizers, initial)
            steps.append(r)
        return models["on"], steps


@pytest.fixture(scope="module")
def empty_step():
    """One image without any instance, the fp32 runs under bf16 autocast."""
    with _settings():
        model, vol = build_model()
        m64 = make64(model)
        maps = label_maps((3, 0))
        return model, {"off": run_step(model, vol, maps, "off", SEED_EMPTY, autocast=True),
                       "on": run_step(model, vol, maps, "on", SEED_EMPTY, autocast=True),
                       "f64": run_step(m64, vol, maps, "f64", SEED_EMPTY)}


# ---------------------------------------------------------------- the tests
def test_one_step_paths_and_decisions(one_step):
    model, r = one_step
    on, heads = r["on"], TS._heads(model)
    assert len(on["indices"]) == heads and len(on["coords"]) == heads and on["coords"][0].shape == (6, model.criterion.num_points, 2)
    assert all(len(s) == 3 for ind in on["indices"] for s, _ in ind)
    fails = check_decisions(model, on, r["off"], r["f64"], "one step")
    assert not fails, "\n".join(fails[:60])


def test_one_step_values(one_step):
    model, r = one_step
    fails = []
    check_values(r["on"], r["off"], r["f64"], fails, "one step")
    assert not fails, "\n".join(fails[:60])


def test_three_steps_paths_and_decisions(three_steps):
    model, steps = three_steps
    fails = []
    for s, (counts, r) in enumerate(zip(STEP_COUNTS, steps)):
        # (2, 4) and (4, 1) keep the pair count equal across the heads (6, 6, 5 pairs): the batched path is still the one taken
        # (check_paths asserts one *_many call each and no per-head wrapper)
        assert all([len(t) for _, t in ind] == list(counts) for ind in r["on"]["indices"])
        fails += check_decisions(model, r["on"], r["off"], r["f64"], "step %d %s" % (s, counts))
    assert not fails, "\n".join(fails[:60])


def test_three_steps_values(three_steps):
    model, steps = three_steps
    fails = []
    for s, (counts, r) in enumerate(zip(STEP_COUNTS, steps)):
        check_values(r["on"], r["off"], r["f64"], fails, "step %d %s" % (s, counts))
        check_params(r["params"], r["f64"]["grads"], fails, "step %d %s, after the update" % (s, counts))
    assert not fails, "\n".join(fails[:60])


def test_empty_image_under_autocast_paths_and_decisions(empty_step):
    """One image without any instance (its target is one all-zero plane, matched to one query: 3 + 1 pairs, num_masks 3) in a
    step under bf16 autocast.  The predictions of every head are bf16 there (the mask head's last two matmuls run under autocast),
    and the documented fall-backs are what a whole step takes:
      * the HIP mask head and the HIP cross-attention refuse autocast: mask_heads_forward_batched per head, the torch attention
        core per layer;
      * `loss_heads = "batched"` gives way head by head where SetCriterion._loss_masks_batched says -- a prediction that is not
        fp32: no *_many call, nothing drawn ahead, one loss_masks per head; the per-head device loss and selection take fp32
        predictions too, so each head runs get_uncertain_point_coords_with_randomness with its torch.topk;
      * the matcher's device costs, batched or per head, give way to its point_sample (predictions and targets: two per head);
      * the re-id dice rows take the torch bmm.
    The targets from label maps and the embedding loss stay on the device: the pixel embedding is fp32 under autocast.  Nothing
    raises and every decision is the off step's.  (The float64 run, without autocast, only measures the yardstick |off - f64| of
    the values test: a bf16 step and a float64 step may decide differently, so off == f64 is no precondition here.)"""
    model, r = empty_step
    on, off = r["on"], r["off"]
    heads, layers = TS._heads(model), TS._layers(model)
    assert on["pred_dtypes"] == off["pred_dtypes"] == [torch.bfloat16] * heads
    assert all([len(t) for _, t in ind] == [3, 1] for ind in on["indices"])
    c = on["counts"]
    PL, CR, DEC = TS._PL, TS._CRIT, TS._DEC
    fails = []
    assert c["pctrans_amd.dynamic_mask_head:dynamic_mask_head_backward"] == 0
    assert c[DEC + ":MultiScaleMaskedTransformerDecoder:mask_heads_forward_batched"] == heads
    assert c["pctrans_amd.attention_train:cross_attention_forward"] == 0 == c["pctrans_amd.attention_train:cross_attention_backward"]
    assert c["cross_attention_cores:forward"] == layers
    device_point_paths = [k for kind in ("wrappers", "superseded")
                          for k in TS.labels(kind, only=("point_loss", "point_select", "match_cost", "loss_heads"))]
    assert len(device_point_paths) == 10 and all(c[k] == 0 for k in device_point_paths), {k: c[k] for k in device_point_paths}
    assert c[CR + ":get_uncertain_point_coords_with_randomness"] == heads and c["torch:topk"] == heads
    assert c[TS._MATCHER + ":point_sample"] == 2 * heads
    assert c["pctrans_amd.reid_dice:dice_rows_forward"] == 0 == c["pctrans_amd.reid_dice:dice_rows_backward"] and c["torch:bmm"] > 0
    check_paths(model, on, fails, only=("emb_loss", "targets"))
    check_paths(model, off, fails)
    check_discrete(on, off, fails)
    assert not fails, "\n".join(fails[:60])


def test_empty_image_under_autocast_values(empty_step):
    model, r = empty_step
    fails = []
    check_values(r["on"], r["off"], r["f64"], fails, "empty image, autocast")
    assert not fails, "\n".join(fails[:60])

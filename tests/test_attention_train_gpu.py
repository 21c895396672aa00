"""GPU: the differentiable fp32 cross-attention (pct_cross_attention_forward_f32 / pct_cross_attention_backward_f32,
pctrans_amd/attention_train.py) against the float64 reference of attention_train_reference.py (pinned on the CPU against
autograd of the float64 torch chain by test_attention_train_cpu.py).

Accuracy rule, for `out` and each of the five gradients:  e_hip <= 2 * e_torch + 2^-22 * max|ref|,  where
e_torch is the error of the unchanged fp32 torch chain on the same operands on the same device.  Torch's chain is NaN on a row
with nothing attendable (and spreads it over the key gradients): where a case has such rows, the yardstick runs with those rows'
mask rows cleared and their grad_out rows zeroed, which removes exactly their terms, and the kernel's rows are asserted to be 0.
PCT_ATTN_TRAIN_REPORT=<file> writes the measured pairs of every case there as JSON (profiles/attn_train_parity.json).

Measured on an MI355X (profiles/attn_train_parity.json): all 181 cases meet the rule; the kernel's error is 0.30 x (out) to
0.46 x (key gradients) the torch chain's in the median.  A first version with fp32 score chains and D from rowsum(grad_out * out)
missed it in 5 cases (ratios 2.2 - 7); csrc/cross_attention_train.hip says what was changed and why."""
import atexit
import json
import os

import pytest
import torch

import attention_train_reference as R

pytestmark = pytest.mark.gpu

NAMES = ("out", "grad_q_c", "grad_q_s", "grad_k_c", "grad_k_p", "grad_v")
CASES = [(f, Q, S, 8) for f in R.FAMILIES for Q in R.QS for S in R.SS]
CASES += [(f, Q, S, 4) for f in ("noise", "noise_open", "window_masks") for Q, S in ((17, 65), (100, 196), (16, 1), (1, 784))]
CASES += [("noise_open", R.BIG[0], R.BIG[1], 8)]
_FIGURES = {}


def _report():
    path = os.environ.get("PCT_ATTN_TRAIN_REPORT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump(_FIGURES, f, indent=1, sort_keys=True)


atexit.register(_report)


def _cuda(t):
    return None if t is None else t.cuda()


def _kernel(c, ops=None):
    """(out, lse, five gradients) of the device path on the case's operands."""
    from pctrans_amd import attention_train as at
    ops = [t.cuda() for t in c["ops"]] if ops is None else ops
    mask, ro, go = _cuda(c["mask"]), _cuda(c["row_open"]), c["grad_out"].cuda()
    assert at.supported(*ops, c["heads"], mask, ro)
    out, lse = at.cross_attention_forward(*ops, c["heads"], mask, ro)
    grads = at.cross_attention_backward(*ops, c["heads"], mask, ro, out, lse, go)
    return out, lse, grads


def _yardstick(c):
    """(out, five gradients) of the fp32 torch chain on the device, the dead rows taken out of it."""
    mask, go = c["mask"], c["grad_out"].clone()
    if c["dead_rows"]:
        mask = mask.clone()
        for n, q in c["dead_rows"]:
            mask[n, 0, q] = False
            go[q, n] = 0
    out, grads = R.torch_chain_grads([t.cuda() for t in c["ops"]], c["heads"], _cuda(mask), _cuda(c["row_open"]), go.cuda())
    return out, grads


@pytest.mark.parametrize("family,Q,S,heads", CASES, ids=lambda v: str(v))
def test_forward_and_backward_against_float64(family, Q, S, heads):
    c = R.case(family, Q, S, heads)
    out, lse, grads = _kernel(c)
    y_out, y_grads = _yardstick(c)
    live = torch.ones(Q, R.N, dtype=torch.bool)
    for n, q in c["dead_rows"]:                                         # a dead row: out, lse and its own gradients exactly 0
        live[q, n] = False
        assert float(out[q, n].abs().max()) == 0.0 and float(lse[:, n, :, q].abs().max()) == 0.0
        assert float(grads[0][q, n].abs().max()) == 0.0 and float(grads[1][q, n].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in (out, lse) + tuple(grads))
    if c["blocked_key"] is not None:                                    # masked for every query: exactly zero gradient rows
        for g in grads[2:]:
            assert float(g[c["blocked_key"]].abs().max()) == 0.0
    lse_err = float((lse.double().sum(0).cpu() - c["lse"]).abs().max())         # the two planes: value + low-order word
    assert lse_err <= 2.0 ** -20 * max(1.0, float(c["lse"].abs().max())), lse_err
    fig = {}
    failed = []
    for name, g, y, w in zip(NAMES, (out,) + tuple(grads), (y_out,) + tuple(y_grads), (c["out"],) + tuple(c["grads"])):
        g, y = g.double().cpu(), y.double().cpu()
        if name == "out":
            g, y, w = g[live], y[live], w[live]
        top = float(w.abs().max()) if w.numel() else 0.0
        e_hip, e_torch = (float((t - w).abs().max()) if w.numel() else 0.0 for t in (g, y))
        bound = 2 * e_torch + 2.0 ** -22 * top
        fig[name] = {"e_hip": e_hip, "e_torch": e_torch, "max_ref": top, "bound": bound}
        print("%s: max|ref| %.3e  e_hip %.3e  e_torch %.3e  bound %.3e" % (name, top, e_hip, e_torch, bound))
        if not e_hip <= bound:
            failed.append((name, e_hip, bound))
    _FIGURES["%s-Q%d-S%d-h%d" % (family, Q, S, heads)] = fig
    assert not failed, failed


def test_speed_rule_leaves_long_key_sets_to_torch():
    """`supported` = `covered` up to MAX_KEYS keys (measured: profiles/attn_train.json); the kernels themselves run beyond it."""
    from pctrans_amd import attention_train as at
    assert at.MAX_KEYS == 1024
    for S, want in ((at.MAX_KEYS, True), (at.MAX_KEYS + 1, False)):
        ops = [torch.randn(T, 1, 128, device="cuda") for T in (3, 3, S, S, S)]
        assert at.covered(*ops, 8) and at.supported(*ops, 8) is want
    out = at.cross_attention_train(*[t.requires_grad_(True) for t in ops], 8)
    want = R.torch_chain(*ops, 8)
    assert float((out - want).abs().max()) <= 1e-5 * float(want.abs().max())
    out.sum().backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in ops)


def test_two_calls_are_bit_identical():
    c = R.case("noise_open", R.BIG[0], R.BIG[1], 8)
    a, b = _kernel(c), _kernel(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


def test_operands_at_a_16_byte_offset():
    """Every operand a view that starts 16 bytes into its allocation: the same bits as from aligned copies."""
    c = R.case("noise", 17, 65, 8)
    want = _kernel(c)
    ops = []
    for t in c["ops"]:
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
        v = buf[4:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 32 == 16
        ops.append(v)
    got = _kernel(c, ops)
    assert torch.equal(got[0], want[0]) and all(torch.equal(x, y) for x, y in zip(got[2], want[2]))


def test_status_codes_on_device_pointers():
    from pctrans_amd import _lib
    L = _lib.lib()
    c = R.case("noise_nomask", 16, 64, 8)
    ops = [t.cuda() for t in c["ops"]]
    out, lse = torch.empty(16, 2, 128, device="cuda"), torch.empty(2, 2, 8, 16, device="cuda")
    p = [t.data_ptr() for t in ops]
    call = lambda ptrs, N=2, h=8, Q=16, S=64, o=out.data_ptr(): L.pct_cross_attention_forward_f32(
        *ptrs, None, None, N, h, Q, S, R.SCALE, o, lse.data_ptr(), None)
    assert call(p) == 0
    torch.cuda.synchronize()
    assert float((out.double().cpu() - c["out"]).abs().max()) < 1e-4
    assert call([p[0] + 4] + p[1:]) == -3 and call(p, o=out.data_ptr() + 8) == -3
    assert call(p, h=5) == -4 and call(p, N=-1) == -1 and call([None] + p[1:]) == -1
    before = out.clone()
    assert call(p, Q=0) == 0 and call(p, S=0) == 0 and call(p, N=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)


def test_function_keeps_the_seven_tensors_only():
    """Saved for the backward: the five operands, out and lse.  What one forward leaves allocated is out + lse + 1 MiB of
    slack, where the torch chain keeps the [N, heads, Q, S] probabilities (and more)."""
    from pctrans_amd import attention_train as at
    c = R.case("noise_open", R.BIG[0], R.BIG[1], 8)
    Q, S = R.BIG
    ops = [t.cuda().requires_grad_(True) for t in c["ops"]]
    mask, ro = c["mask"].cuda(), c["row_open"].cuda()
    nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    out = at.cross_attention_train(*ops, 8, mask, ro)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - base
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 7 and [tuple(t.shape) for t in saved[:5]] == [tuple(t.shape) for t in ops]
    assert tuple(saved[5].shape) == (Q, 2, 128) and tuple(saved[6].shape) == (2, 2, 8, Q)
    assert grown <= nbytes(out) + 2 * 4 * 2 * 8 * Q + (1 << 20), grown
    g = torch.autograd.grad(out, ops, c["grad_out"].cuda())
    assert all(x.shape == t.shape for x, t in zip(g, ops))
    del out, g, saved
    base = torch.cuda.memory_allocated()
    out = R.torch_chain(*ops, 8, mask, ro)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - base > 2 * 8 * Q * S * 4


def _decoder_run(d, mf, xs, mode):
    from pctrans_amd import attention_train as at
    for m in d.modules():
        if hasattr(m, "attn_train"):
            m.attn_train = mode
    d.zero_grad(set_to_none=True)
    calls = [0]
    inner = at.cross_attention_backward

    def spy(*a, **k):
        calls[0] += 1
        return inner(*a, **k)

    at.cross_attention_backward = spy
    try:
        outs = d._forward_core(mf, *xs)
        sum(o.square().mean() for o in outs[2:]).backward()
    finally:
        at.cross_attention_backward = inner
    grads = {n: p.grad.detach().clone() for n, p in d.named_parameters() if p.grad is not None}
    preds = [o.detach() for o in outs[2:]]
    # the losses of the step, evaluated in float64 from the predictions: an fp32 mean over 15 360 squares of size 265 rounds by
    # about 5e-5 on its own, the size of the differences compared below
    return preds, [o.double().square().mean() for o in preds], grads, calls[0]


def test_decoder_with_the_switch_on_is_the_decoder_with_it_off(golden, monkeypatch):
    """The decoder of the smallest golden case (6 queries, levels of 6, 20 and 80 keys, 3 layers) in train mode: the per-layer
    mask predictions, the losses formed from them (mean square, evaluated in float64) and every parameter gradient with the switch on against float64, under the
    accuracy rule with the switch-off decoder as the yardstick.  A key-projection bias has a mathematically zero gradient (the
    softmax does not see a shift of every key): what an fp32 run holds there is the rounding of terms of its weight's size that
    cancel, so the rule's floor takes its scale from the sibling weight's gradient there."""
    import copy
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    from test_decoder_golden import _full_decoder, _t
    g = golden("dec_full_decoder")
    d = _full_decoder("cuda").train()
    xs = [_t(g["x%d" % i]).cuda() for i in range(3)]
    mf = _t(g["mask_features"]).cuda()
    d64 = copy.deepcopy(d).double()
    d64.pe_layer.register_forward_hook(lambda m, i, o: o.double())
    sine = dec.gen_sineembed_for_position
    monkeypatch.setattr(dec, "gen_sineembed_for_position",
                        lambda p, *a, **k: sine(p, *a, **k).to(torch.float64 if p.dtype == torch.float64 else torch.float32))
    p_off, l_off, g_off, c_off = _decoder_run(d, mf, xs, "torch")
    p_on, l_on, g_on, c_on = _decoder_run(d, mf, xs, "hip")
    p_64, l_64, g_64, _ = _decoder_run(d64, mf.double(), [x.double() for x in xs], "torch")
    assert c_off == 0 and c_on == 3 and g_on.keys() == g_off.keys() == g_64.keys()

    def close(on, off, ref, what, floor_scale=None):
        e_on, e_off = float((on.double() - ref).abs().max()), float((off.double() - ref).abs().max())
        top = float(ref.abs().max()) if floor_scale is None else floor_scale
        print("%s: scale %.3e  e_on %.3e  e_off %.3e" % (what, top, e_on, e_off))
        assert e_on <= 2 * e_off + 2.0 ** -22 * top, (what, e_on, e_off, top)

    for i in range(len(l_64)):
        close(p_on[i], p_off[i], p_64[i], "mask prediction %d" % i)
    # the step's losses as one tensor [layers + 1] under the rule, like every other tensor (largest error over its elements, floor
    # from its largest element); every prediction they are formed from is held elementwise above
    close(torch.stack(l_on), torch.stack(l_off), torch.stack(l_64), "losses")
    for n in g_64:
        sib = n[:-len("bias")] + "weight"
        zero = n.endswith(".bias") and sib in g_64 and float(g_64[n].abs().max()) < 1e-12 * float(g_64[sib].abs().max())
        close(g_on[n], g_off[n], g_64[n], "grad " + n, float(g_64[sib].abs().max()) if zero else None)


def test_graphed_training_decoder_with_the_switch_on():
    """graph.graph_training_decoder with the HIP attention training path: the replayed step is the eager step with the switch
    on, over three replays (tolerances of test_dmh_train_gpu.py::test_graphed_training_decoder_with_the_switch_on)."""
    import copy
    import random
    from pctrans_amd import attention_train as at, graph
    from pctrans_amd.arch import maskformer as mfm
    from pctrans_amd.arch.resnet import ResNet
    from pctrans_amd.config import get_cfg
    from test_arch_cpu import _blob
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=12, norm="BN", sem_norm="BN", enc_layers=2, dec_layers=4, train_num_points=512, dataset="BBBC")
    eager = mfm.MaskFormer(**mfm.MaskFormer.from_config(cfg, ResNet(18, 3, norm="BN"))).cuda().train()
    switched = [m for m in eager.modules() if hasattr(m, "attn_train")]
    assert len(switched) >= 3
    for m in switched:
        m.attn_train = "hip"
    dec_only = copy.deepcopy(eager)
    assert [m.attn_train for m in dec_only.modules() if hasattr(m, "attn_train")] == ["hip"] * len(switched)
    H = W = 128
    vol = torch.randn(2, 3, H, W, device="cuda")
    targets = []
    for b in range(2):
        masks = torch.stack([_blob(H, W, 30, 30, 14), _blob(H, W, 90, 80, 20), _blob(H, W, 40, 100 - 9 * b, 10)]).cuda()
        centers = torch.tensor([[30 / W, 30 / H], [80 / W, 90 / H], [(100 - 9 * b) / W, 40 / H]], device="cuda").view(3, 1, 2)
        targets.append({"masks": masks, "labels": torch.ones(3, dtype=torch.long, device="cuda"),
                        "fg_masks": (masks.sum(0) > 0).float(), "center_points": centers})
    calls = [0]
    inner = at.cross_attention_backward

    def spy(*a, **k):
        calls[0] += 1
        return inner(*a, **k)

    at.cross_attention_backward = spy
    try:
        graph.graph_training_decoder(dec_only, vol)
        assert graph.has_graphed_decoder(dec_only) and calls[0] > 0          # the capture went through the HIP backward

        def step(model):
            random.seed(3)
            torch.manual_seed(3)
            losses = model(vol, targets, True)
            total = sum(v for v in losses.values() if torch.is_tensor(v))
            model.zero_grad(set_to_none=True)
            total.backward()
            return ({k: float(v.detach()) for k, v in losses.items() if torch.is_tensor(v)},
                    {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})

        before = calls[0]
        le, ge = step(eager)
        assert calls[0] > before                                              # the eager step runs the HIP backward too
        for _ in range(3):
            lg, gg = step(dec_only)
            assert lg.keys() == le.keys()
            for k in le:
                assert abs(le[k] - lg[k]) <= 2e-4 * max(1.0, abs(le[k])), (k, le[k], lg[k])
            assert ge.keys() <= gg.keys()
            for n in ge:
                scale = float(ge[n].abs().max())
                tol = 5e-3 * scale + 1e-6 if scale > 1e-5 else 1e-5
                assert float((ge[n] - gg[n]).abs().max()) <= tol, n
            for n in gg.keys() - ge.keys():                                   # (parameters the losses do not reach)
                assert float(gg[n].abs().max()) == 0.0, n
    finally:
        at.cross_attention_backward = inner
        if graph.has_graphed_decoder(dec_only):
            graph.release_training_graphs(dec_only)

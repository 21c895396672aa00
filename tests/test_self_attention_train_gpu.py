"""GPU: the differentiable fp32 self-attention (pct_self_attention_forward_f32 / pct_self_attention_backward_f32,
pctrans_amd/self_attention_train.py) against the float64 reference of self_attention_train_reference.py (pinned on the CPU
against autograd of the float64 torch chain by test_self_attention_train_cpu.py).

Accuracy rule, for `out`, grad_q, grad_k and grad_v:  e_hip <= 2 * e_torch + 2^-22 * max|ref|,  where e_torch is
the error of the unchanged fp32 torch chain on the same operands on the same device (its gradients of q_c and q_p are one tensor,
as are those of k_c and k_p; the first of each is taken).  PCT_SELF_ATTN_TRAIN_REPORT=<file> writes the measured pairs of every
case there as JSON (profiles/self_attn_train_parity.json).

The kernels' tiles are 16 queries by 16 keys with four waves over interleaved key steps, which is what the query counts of
self_attention_train_reference.QS straddle; the LDS image of the backward's query pass has no seam below its limit of 512.

Measured on an MI355X (profiles/self_attn_train_parity.json): all 37 cases meet the rule, the largest e_hip / bound is 0.56; the
kernels' error is 0.41 x (out), 0.60 x (grad_q), 0.79 x (grad_k) and 0.75 x (grad_v) the torch chain's in the median."""
import atexit
import json
import os

import pytest
import torch

import self_attention_train_reference as R

pytestmark = pytest.mark.gpu

NAMES = ("out", "grad_q", "grad_k", "grad_v")
CASES = R.CASES
_FIGURES = {}


def _report():
    path = os.environ.get("PCT_SELF_ATTN_TRAIN_REPORT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump(_FIGURES, f, indent=1, sort_keys=True)


atexit.register(_report)


def _kernel(c, ops=None):
    """(out, lse, three gradients) of the device path on the case's operands."""
    from pctrans_amd import self_attention_train as st
    ops = [t.cuda() for t in c["ops"]] if ops is None else ops
    assert st.supported(*ops, c["heads"])
    out, lse = st.self_attention_forward(*ops, c["heads"])
    grads = st.self_attention_backward(*ops, c["heads"], out, lse, c["grad_out"].cuda())
    return out, lse, grads


def _close(got, yard, ref, what, floor_scale=None):
    """The rule; -> the figures.  Prints before it asserts."""
    got, yard, ref = got.double().cpu(), yard.double().cpu(), ref.double().cpu()
    e_hip, e_torch = float((got - ref).abs().max()), float((yard - ref).abs().max())
    top = float(ref.abs().max()) if floor_scale is None else floor_scale
    bound = 2 * e_torch + 2.0 ** -22 * top
    print("%s: scale %.3e  e_hip %.3e  e_torch %.3e  bound %.3e" % (what, top, e_hip, e_torch, bound))
    return {"e_hip": e_hip, "e_torch": e_torch, "max_ref": top, "bound": bound}


@pytest.mark.parametrize("family,Q,heads", CASES, ids=lambda v: str(v))
def test_forward_and_backward_against_float64(family, Q, heads):
    c = R.case(family, Q, heads)
    out, lse, grads = _kernel(c)
    y_out, y = R.torch_chain_grads([t.cuda() for t in c["ops"]], heads, c["grad_out"].cuda())
    assert torch.equal(y[0], y[1]) and torch.equal(y[2], y[3])          # the add's backward is the identity
    assert all(bool(torch.isfinite(t).all()) for t in (out, lse) + tuple(grads))
    lse_err = float((lse.double().sum(0).cpu() - c["lse"]).abs().max())         # the two planes: value + low-order word
    assert lse_err <= 2.0 ** -20 * max(1.0, float(c["lse"].abs().max())), lse_err
    fig = {name: _close(g, w, ref, name) for name, g, w, ref in
           zip(NAMES, (out,) + tuple(grads), (y_out, y[0], y[2], y[4]), (c["out"],) + tuple(c["grads"]))}
    _FIGURES["%s-Q%d-h%d" % (family, Q, heads)] = fig
    failed = [(n, f["e_hip"], f["bound"]) for n, f in fig.items() if not f["e_hip"] <= f["bound"]]
    assert not failed, failed


def test_two_calls_are_bit_identical():
    c = R.case("noise", R.BIG, 8)
    a, b = _kernel(c), _kernel(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


def test_operands_at_a_16_byte_offset():
    """Every operand a view that starts 16 bytes into its allocation: the same bits as from aligned copies."""
    c = R.case("noise", 17, 8)
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
    c = R.case("noise", 16, 8)
    ops = [t.cuda() for t in c["ops"]]
    out, lse = torch.empty(16, 2, 128, device="cuda"), torch.empty(2, 2, 8, 16, device="cuda")
    p = [t.data_ptr() for t in ops]
    call = lambda ptrs, N=2, h=8, Q=16, o=out.data_ptr(): L.pct_self_attention_forward_f32(
        *ptrs, N, h, Q, R.SCALE, o, lse.data_ptr(), None)
    assert call(p) == 0
    torch.cuda.synchronize()
    assert float((out.double().cpu() - c["out"]).abs().max()) < 1e-4
    assert call([p[0] + 4] + p[1:]) == -3 and call(p, o=out.data_ptr() + 8) == -3
    assert call(p, h=5) == -4 and call(p, Q=513) == -4 and call(p, N=-1) == -1 and call([None] + p[1:]) == -1
    before = out.clone()
    assert call(p, Q=0) == 0 and call(p, N=0) == 0
    ws, g = torch.empty(2 * 8 * 16, device="cuda"), [torch.full((16, 2, 128), 7.0, device="cuda") for _ in range(3)]
    go = c["grad_out"].cuda()
    back = lambda N=2, Q=16, h=8: L.pct_self_attention_backward_f32(
        *p, out.data_ptr(), lse.data_ptr(), go.data_ptr(), N, h, Q, R.SCALE, ws.data_ptr(), *[t.data_ptr() for t in g], None)
    assert back(Q=0) == 0 and back(N=0) == 0 and back(h=5) == -4 and back(Q=513) == -4
    torch.cuda.synchronize()
    assert torch.equal(out, before) and all(float(t.min()) == 7.0 == float(t.max()) for t in g)
    assert back() == 0
    torch.cuda.synchronize()
    for t, ref in zip(g, c["grads"]):
        assert float((t.double().cpu() - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max()))


def test_function_keeps_the_seven_tensors_only():
    """Saved for the backward: the five operands, out and lse.  What one forward leaves allocated is out + lse + 1 MiB of
    slack, where the torch chain keeps the [N, heads, Q, Q] probabilities (and more)."""
    from pctrans_amd import self_attention_train as st
    Q = R.BIG
    c = R.case("noise", Q, 8)
    ops = [t.cuda().requires_grad_(True) for t in c["ops"]]
    nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    out = st.self_attention_train(*ops, 8)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - base
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 7 and [tuple(t.shape) for t in saved[:5]] == [tuple(t.shape) for t in ops]
    assert tuple(saved[5].shape) == (Q, 2, 128) and tuple(saved[6].shape) == (2, 2, 8, Q)
    assert grown <= nbytes(out) + 2 * 4 * 2 * 8 * Q + (1 << 20), grown
    g = torch.autograd.grad(out, ops, c["grad_out"].cuda())
    assert all(x.shape == t.shape for x, t in zip(g, ops))
    assert torch.equal(g[0], g[1]) and torch.equal(g[2], g[3])
    part = torch.autograd.grad(st.self_attention_train(*ops, 8), [ops[1], ops[4]], c["grad_out"].cuda())
    assert torch.equal(part[0], g[1]) and torch.equal(part[1], g[4])       # filtered by needs_input_grad, same bits
    del out, g, saved, part
    base = torch.cuda.memory_allocated()
    out = R.torch_chain(*ops, 8)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - base > 2 * 8 * Q * Q * 4


class _Spy:
    """Counts the entries into self_attention_train.self_attention_backward (and into the forward wrapper)."""

    def __enter__(self):
        from pctrans_amd import self_attention_train as st
        self.st, self.bwd, self.fwd = st, st.self_attention_backward, st.self_attention_forward
        self.backward = self.forward = 0

        def spy_b(*a, **k):
            self.backward += 1
            return self.bwd(*a, **k)

        def spy_f(*a, **k):
            self.forward += 1
            return self.fwd(*a, **k)

        st.self_attention_backward, st.self_attention_forward = spy_b, spy_f
        return self

    def __exit__(self, *exc):
        self.st.self_attention_backward, self.st.self_attention_forward = self.bwd, self.fwd


def _layer_run(layer, tgt, qpos, mode, grad, **kw):
    layer.self_attn_train = mode
    layer.zero_grad(set_to_none=True)
    t = tgt.detach().clone().requires_grad_(True)
    out = layer(t, query_pos=qpos, **kw)
    out.backward(grad)
    return out.detach(), dict({n: p.grad.detach().clone() for n, p in layer.named_parameters()}, tgt=t.grad.detach().clone())


def test_layer_with_the_switch_on_is_the_layer_with_it_off():
    """SelfAttentionLayer (128 channels, 8 heads, 65 queries, 2 images) with the switch on against the same weights with it
    off and a float64 copy: the output, the gradient of tgt and every parameter gradient under the rule.  The two key
    projections' biases have a mathematically zero gradient (a shift of every key leaves the softmax unchanged): the floor
    takes its scale from the sibling weight's gradient there."""
    import copy
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import SelfAttentionLayer
    torch.manual_seed(11)
    layer = SelfAttentionLayer(128, 8).cuda().train()
    with torch.no_grad():
        for p in layer.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    layer64 = copy.deepcopy(layer).double()
    tgt, qpos, grad = (torch.randn(65, 2, 128, device="cuda") for _ in range(3))
    with _Spy() as spy:
        o_off, g_off = _layer_run(layer, tgt, qpos, "torch", grad)
        assert spy.forward == 0 and spy.backward == 0
        o_on, g_on = _layer_run(layer, tgt, qpos, "hip", grad)
        assert spy.forward == 1 and spy.backward == 1                     # the backward wrapper is entered exactly once
        o_64, g_64 = _layer_run(layer64, tgt.double(), qpos.double(), "hip", grad.double())
        assert spy.forward == 1 and spy.backward == 1                     # float64 operands keep the torch chain
    assert g_on.keys() == g_off.keys() == g_64.keys()
    figs = {"out": _close(o_on, o_off, o_64, "out")}
    for n in g_64:
        sib = n[:-len("bias")] + "weight"
        zero = n in ("sa_kcontent_proj.bias", "sa_kpos_proj.bias")
        if zero:
            assert float(g_64[n].abs().max()) < 1e-12 * float(g_64[sib].abs().max())
        figs[n] = _close(g_on[n], g_off[n], g_64[n], "grad " + n, float(g_64[sib].abs().max()) if zero else None)
    failed = [(n, f["e_hip"], f["bound"]) for n, f in figs.items() if not f["e_hip"] <= f["bound"]]
    assert not failed, failed


def test_layer_keeps_the_torch_chain_where_the_kernels_do_not_apply():
    """Not entered under torch.no_grad(), under bf16 autocast, with a tgt_mask, or with the switch at "torch"."""
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import SelfAttentionLayer
    torch.manual_seed(12)
    layer = SelfAttentionLayer(128, 8).cuda().train()
    tgt, qpos = torch.randn(17, 2, 128, device="cuda", requires_grad=True), torch.randn(17, 2, 128, device="cuda")
    with _Spy() as spy:
        layer.self_attn_train = "hip"
        with torch.no_grad():
            layer(tgt, query_pos=qpos)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            layer(tgt, query_pos=qpos).float().sum().backward()
        layer(tgt, query_pos=qpos, tgt_mask=torch.zeros(17, 17, dtype=torch.bool, device="cuda")).sum().backward()
        layer.self_attn_train = "torch"
        layer(tgt, query_pos=qpos).sum().backward()
        assert spy.forward == 0 and spy.backward == 0
        layer.self_attn_train = "hip"
        layer(tgt, query_pos=qpos).sum().backward()
        assert spy.forward == 1 and spy.backward == 1


def _decoder_run(d, mf, xs, mode):
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import SelfAttentionLayer
    for m in d.modules():
        if isinstance(m, SelfAttentionLayer):
            m.self_attn_train = mode
        assert getattr(m, "attn_train", "torch") == "torch"                # the self-attention layers only
    d.zero_grad(set_to_none=True)
    with _Spy() as spy:
        outs = d._forward_core(mf, *xs)
        sum(o.square().mean() for o in outs[2:]).backward()
    grads = {n: p.grad.detach().clone() for n, p in d.named_parameters() if p.grad is not None}
    preds = [o.detach() for o in outs[2:]]
    # the losses of the step, evaluated in float64 from the predictions (test_attention_train_gpu.py says why)
    return preds, [o.double().square().mean() for o in preds], grads, spy.backward


def test_decoder_with_the_switch_on_is_the_decoder_with_it_off(golden, monkeypatch):
    """The decoder of the smallest golden case (6 queries, 3 layers) in train mode, the switch set on its self-attention layers
    only: the per-layer mask predictions, the losses formed from them (mean square, evaluated in float64) as one tensor and
    every parameter gradient with the switch on against float64, under the accuracy rule with the switch-off decoder as the
    yardstick; a bias whose float64 gradient is zero against its weight's takes the floor's scale from that weight
    (test_attention_train_gpu.py::test_decoder_with_the_switch_on_is_the_decoder_with_it_off)."""
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
    assert c_off == 0 and c_on == d.num_layers == 3 and g_on.keys() == g_off.keys() == g_64.keys()
    figs = {}
    for i in range(len(l_64)):
        figs["mask prediction %d" % i] = _close(p_on[i], p_off[i], p_64[i], "mask prediction %d" % i)
    figs["losses"] = _close(torch.stack(l_on), torch.stack(l_off), torch.stack(l_64), "losses")
    for n in g_64:
        sib = n[:-len("bias")] + "weight"
        zero = n.endswith(".bias") and sib in g_64 and float(g_64[n].abs().max()) < 1e-12 * float(g_64[sib].abs().max())
        figs["grad " + n] = _close(g_on[n], g_off[n], g_64[n], "grad " + n, float(g_64[sib].abs().max()) if zero else None)
    failed = [(n, f["e_hip"], f["bound"]) for n, f in figs.items() if not f["e_hip"] <= f["bound"]]
    assert not failed, failed


def test_graphed_training_decoder_with_the_switch_on():
    """graph.graph_training_decoder with the HIP self-attention training path: the replayed step is the eager step with the
    switch on, over three replays (tolerances and structure of
    test_attention_train_gpu.py::test_graphed_training_decoder_with_the_switch_on)."""
    import copy
    import random
    from pctrans_amd import graph
    from pctrans_amd.arch import maskformer as mfm
    from pctrans_amd.arch.resnet import ResNet
    from pctrans_amd.config import get_cfg
    from test_arch_cpu import _blob
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=12, norm="BN", sem_norm="BN", enc_layers=2, dec_layers=4, train_num_points=512, dataset="BBBC")
    eager = mfm.MaskFormer(**mfm.MaskFormer.from_config(cfg, ResNet(18, 3, norm="BN"))).cuda().train()
    switched = [m for m in eager.modules() if hasattr(m, "self_attn_train")]
    assert len(switched) >= 3
    for m in switched:
        m.self_attn_train = "hip"
    dec_only = copy.deepcopy(eager)
    assert [m.self_attn_train for m in dec_only.modules() if hasattr(m, "self_attn_train")] == ["hip"] * len(switched)
    H = W = 128
    vol = torch.randn(2, 3, H, W, device="cuda")
    targets = []
    for b in range(2):
        masks = torch.stack([_blob(H, W, 30, 30, 14), _blob(H, W, 90, 80, 20), _blob(H, W, 40, 100 - 9 * b, 10)]).cuda()
        centers = torch.tensor([[30 / W, 30 / H], [80 / W, 90 / H], [(100 - 9 * b) / W, 40 / H]], device="cuda").view(3, 1, 2)
        targets.append({"masks": masks, "labels": torch.ones(3, dtype=torch.long, device="cuda"),
                        "fg_masks": (masks.sum(0) > 0).float(), "center_points": centers})
    with _Spy() as spy:
        try:
            graph.graph_training_decoder(dec_only, vol)
            assert graph.has_graphed_decoder(dec_only) and spy.backward > 0      # the capture went through the HIP backward

            def step(model):
                random.seed(3)
                torch.manual_seed(3)
                losses = model(vol, targets, True)
                total = sum(v for v in losses.values() if torch.is_tensor(v))
                model.zero_grad(set_to_none=True)
                total.backward()
                return ({k: float(v.detach()) for k, v in losses.items() if torch.is_tensor(v)},
                        {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})

            before = spy.backward
            le, ge = step(eager)
            assert spy.backward > before                                          # the eager step runs the HIP backward too
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
            if graph.has_graphed_decoder(dec_only):
                graph.release_training_graphs(dec_only)

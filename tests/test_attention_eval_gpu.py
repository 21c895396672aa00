"""GPU: the decoder's attention in fp32 evaluation (pct_cross_attention_eval_f32 / pct_self_attention_eval_f32,
pctrans_amd/attention_eval.py; kernels csrc/attention_eval.hip).

  * `out` is, bit for bit, that of the training forwards (pct_cross_attention_forward_f32 / pct_self_attention_forward_f32), which
    test_attention_train_gpu.py and test_self_attention_train_gpu.py hold to float64 at the training geometries;
  * at the evaluation geometries no other test reaches -- (Q, S) = (100, 374), (300, 4 096), (300, 5 655 = 88 * 64 + 23) and a
    self-attention of 600 queries -- against the float64 references (attention_train_reference.py,
    self_attention_train_reference.py) under the project's rule:  e_hip <= 2 * e_torch + 2^-22 * max|ref|,  where
    e_torch is the error of the fp32 torch chain on the same operands on the same device (a dead row taken out of the
    yardstick, which is NaN there, and asserted to be exactly 0 in the kernel's output);
  * the layers and the whole decoder with the switch on against the switch off, beside float64."""
import copy

import numpy as np
import pytest
import torch

import attention_train_reference as R
import self_attention_train_reference as SR

pytestmark = pytest.mark.gpu

IDENTITY_GROUPS = [(f, h) for h in (8, 4) for f in R.FAMILIES]
EVAL_CROSS = [(f, Q, S, 8) for Q, S in ((100, 374), (300, 4096), (300, 5655)) for f in ("noise", "underflow", "window_masks")]
EVAL_SELF_Q = 600
EVAL_SELF_FAMILIES = ("noise", "underflow")


def _cuda(t):
    return None if t is None else t.cuda()


def _cross(c, ops=None):
    from pctrans_amd import attention_eval as ae
    ops = [t.cuda() for t in c["ops"]] if ops is None else ops
    mask, ro = _cuda(c["mask"]), _cuda(c["row_open"])
    assert ae.covered(*ops, c["heads"], mask, ro)
    return ae.cross_attention(*ops, c["heads"], mask, ro)


@pytest.mark.parametrize("family,heads", IDENTITY_GROUPS, ids=lambda v: str(v))
def test_cross_output_is_the_training_forwards_bit_for_bit(family, heads):
    from pctrans_amd import attention_train as at
    for Q in R.QS:
        for S in R.SS:
            c = R.case(family, Q, S, heads)
            ops = [t.cuda() for t in c["ops"]]
            mask, ro = _cuda(c["mask"]), _cuda(c["row_open"])
            want = at.cross_attention_forward(*ops, heads, mask, ro)[0]
            got = _cross(c, ops)
            assert torch.equal(got, want), (family, Q, S, heads, float((got - want).abs().max()))
            for n, q in c["dead_rows"]:
                assert float(got[q, n].abs().max()) == 0.0


def test_self_output_is_the_training_forwards_bit_for_bit():
    from pctrans_amd import attention_eval as ae, self_attention_train as st
    for family, Q, heads in SR.CASES:
        ops = [t.cuda() for t in SR.case(family, Q, heads)["ops"]]
        assert ae.covered(*ops, heads)
        got, want = ae.self_attention(*ops, heads), st.self_attention_forward(*ops, heads)[0]
        assert torch.equal(got, want), (family, Q, heads, float((got - want).abs().max()))


def _rule(name, got, yard, ref):
    got, yard = got.double().cpu(), yard.double().cpu()
    top = float(ref.abs().max())
    e_hip, e_torch = float((got - ref).abs().max()), float((yard - ref).abs().max())
    bound = 2 * e_torch + 2.0 ** -22 * top
    print("%s: max|ref| %.3e  e_hip %.3e  e_torch %.3e  bound %.3e" % (name, top, e_hip, e_torch, bound))
    assert bool(torch.isfinite(got).all()) and e_hip <= bound, (name, e_hip, e_torch, bound)


@pytest.mark.parametrize("family,Q,S,heads", EVAL_CROSS, ids=lambda v: str(v))
def test_cross_at_evaluation_geometries_against_float64(family, Q, S, heads):
    c = R.case(family, Q, S, heads)
    out = _cross(c)
    mask = c["mask"]
    live = torch.ones(Q, R.N, dtype=torch.bool)
    if c["dead_rows"]:                                                    # the yardstick without its NaN rows
        mask = mask.clone()
        for n, q in c["dead_rows"]:
            mask[n, 0, q] = False
            live[q, n] = False
            assert float(out[q, n].abs().max()) == 0.0
    yard = R.torch_chain(*[t.cuda() for t in c["ops"]], heads, _cuda(mask), _cuda(c["row_open"]))
    _rule("%s Q %d S %d" % (family, Q, S), out.cpu()[live], yard.cpu()[live], c["out"][live])


@pytest.mark.parametrize("family", EVAL_SELF_FAMILIES)
def test_self_beyond_the_training_kernels_query_limit_against_float64(family):
    from pctrans_amd import attention_eval as ae, self_attention_train as st
    c = SR.case(family, EVAL_SELF_Q, 8)
    ops = [t.cuda() for t in c["ops"]]
    assert EVAL_SELF_Q > st.MAX_QUERIES and not st.covered(*ops, 8) and ae.covered(*ops, 8)
    _rule("self %s Q %d" % (family, EVAL_SELF_Q), ae.self_attention(*ops, 8), SR.torch_chain(*ops, 8), c["out"])


def test_two_calls_are_bit_identical():
    from pctrans_amd import attention_eval as ae
    c = R.case("window_masks", 300, 5655, 8)
    assert torch.equal(_cross(c), _cross(c))
    ops = [t.cuda() for t in SR.case("noise", EVAL_SELF_Q, 8)["ops"]]
    assert torch.equal(ae.self_attention(*ops, 8), ae.self_attention(*ops, 8))


def _offset_copies(ops):
    res = []
    for t in ops:
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
        v = buf[4:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 32 == 16
        res.append(v)
    return res


def test_operands_at_a_16_byte_offset():
    """Every operand a view that starts 16 bytes into its allocation: the same bits as from aligned copies."""
    from pctrans_amd import attention_eval as ae
    c = R.case("noise", 17, 65, 8)
    assert torch.equal(_cross(c, _offset_copies(c["ops"])), _cross(c))
    s = SR.case("noise", 17, 8)
    assert torch.equal(ae.self_attention(*_offset_copies(s["ops"]), 8), ae.self_attention(*[t.cuda() for t in s["ops"]], 8))


def _node_types(g):
    """hipGraphNodeType of every node of a captured graph (kept: keep_graph=True), asked of the HIP runtime this process has
    loaded.  hipGraphNodeTypeKernel is 0."""
    import ctypes
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    graph, n = ctypes.c_void_p(g.raw_cuda_graph()), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    types = []
    for node in nodes:
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(t)) == 0
        types.append(t.value)
    return types


def test_a_captured_call_is_one_kernel_node_and_replays_the_eager_bits():
    from pctrans_amd import attention_eval as ae
    c = R.case("noise_open", 100, 196, 8)
    ops = [t.cuda() for t in c["ops"]]
    mask, ro = c["mask"].cuda(), c["row_open"].cuda()
    s = [t.cuda() for t in SR.case("noise", 100, 8)["ops"]]
    eager = (ae.cross_attention(*ops, 8, mask, ro), ae.self_attention(*s, 8))
    torch.cuda.synchronize()
    for fn, want in ((lambda: ae.cross_attention(*ops, 8, mask, ro), eager[0]), (lambda: ae.self_attention(*s, 8), eager[1])):
        g = torch.cuda.CUDAGraph(keep_graph=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()                                                          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(g):
            out = fn()
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        assert _node_types(g) == [0]                                       # one node, and it is a kernel


def test_status_codes_on_device_pointers():
    from pctrans_amd import _lib
    L = _lib.lib()
    c = R.case("noise_nomask", 16, 64, 8)
    ops = [t.cuda() for t in c["ops"]]
    out = torch.empty(16, 2, 128, device="cuda")
    p = [t.data_ptr() for t in ops]
    cross = lambda ptrs, N=2, h=8, Q=16, S=64, o=out.data_ptr(): L.pct_cross_attention_eval_f32(
        *ptrs, None, None, N, h, Q, S, R.SCALE, o, None)                 # NULL mask and NULL row_open
    assert cross(p) == 0
    torch.cuda.synchronize()
    assert float((out.double().cpu() - c["out"]).abs().max()) < 1e-4
    assert cross(p, h=3) == -4 and cross([p[0] + 4] + p[1:]) == -3 and cross(p, N=-1) == -1 and cross([None] + p[1:]) == -1
    before = out.clone()
    assert cross(p, Q=0) == 0 and cross(p, S=0) == 0 and cross(p, N=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    s = SR.case("noise", 16, 8)
    sp = [t.cuda() for t in s["ops"]]
    self_ = lambda N=2, h=8, Q=16: L.pct_self_attention_eval_f32(*[t.data_ptr() for t in sp], N, h, Q, SR.SCALE, out.data_ptr(), None)
    assert self_() == 0
    torch.cuda.synchronize()
    assert float((out.double().cpu() - s["out"]).abs().max()) < 1e-4
    before = out.clone()
    assert self_(h=3) == -4 and self_(Q=0) == 0 and self_(N=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # a mask without row_open, and row_open without a mask (ignored)
    m = R.case("noise", 16, 64, 8)
    mops = [t.cuda() for t in m["ops"]]
    mask = m["mask"].cuda().view(torch.uint8)
    ro = torch.ones(2, 16, dtype=torch.uint8, device="cuda")
    call = lambda mk, r: L.pct_cross_attention_eval_f32(*[t.data_ptr() for t in mops], mk, r, 2, 8, 16, 64, R.SCALE, out.data_ptr(), None)
    assert call(mask.data_ptr(), None) == 0
    torch.cuda.synchronize()
    live = torch.ones(16, 2, dtype=torch.bool)
    for n, q in m["dead_rows"]:
        live[q, n] = False
    assert float((out.double().cpu() - m["out"])[live].abs().max()) < 1e-4
    assert call(None, ro.data_ptr()) == 0
    torch.cuda.synchronize()
    nomask = R.forward64(*m["ops"], 8)[0]
    assert float((out.double().cpu() - nomask).abs().max()) < 1e-4


def test_speed_rule_keeps_what_was_not_timed_faster_with_torch():
    """`supported` = `covered` inside the region timed faster than the torch chain (profiles/attention_eval.json; the rule is
    stated in pctrans_amd/attention_eval.py); the kernels themselves run beyond it."""
    from pctrans_amd import attention_eval as ae
    assert (ae.MAX_KEYS, ae.MAX_QUERIES, ae.MAX_BATCH, ae.LONG_KEYS, ae.MIN_LONG_GRID) == (5655, 600, 32, 1452, 152)
    for Q, S, N, want in ((300, 5655, 1, True), (100, 4096, 1, False), (100, 4096, 8, True), (100, 1452, 1, True),
                          (300, 5656, 8, False), (601, 601, 1, False), (100, 256, 33, False), (1, 1, 1, True)):
        ops = [torch.empty(T, N, 128, device="cuda") for T in (Q, Q, S, S, S)]
        assert ae.covered(*ops, 8) and ae.supported(*ops, 8) is want, (Q, S, N)
    ops = [torch.randn(T, 1, 128, device="cuda") for T in (100, 100, 4096, 4096, 4096)]
    want = R.torch_chain(*ops, 8)
    assert float((ae.cross_attention(*ops, 8) - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_operands_that_require_a_gradient_raise():
    from pctrans_amd import attention_eval as ae
    ops = [torch.randn(T, 1, 128, device="cuda") for T in (3, 3, 5, 5, 5)]
    ops[2].requires_grad_(True)
    with pytest.raises(RuntimeError, match="no backward"):
        ae.cross_attention(*ops, 8)
    with torch.no_grad():
        assert ae.cross_attention(*ops, 8).shape == (3, 1, 128)
    sops = [torch.randn(3, 1, 128, device="cuda").requires_grad_(i == 4) for i in range(5)]
    with pytest.raises(RuntimeError, match="no backward"):
        ae.self_attention(*sops, 8)


# ---- layers ---------------------------------------------------------------------------------------------------------------------
class _Spies:
    """Counts the entries into the two wrappers and into attention_core's torch chain (the statements behind its fused branch)."""

    def __init__(self, monkeypatch):
        from pctrans_amd import attention_eval as ae
        from pctrans_amd.transformer_decoder import attention
        self.cross = self.self_ = self.core = 0
        cross, self_, core = ae.cross_attention, ae.self_attention, attention.attention_core

        def spy_cross(*a, **k):
            self.cross += 1
            return cross(*a, **k)

        def spy_self(*a, **k):
            self.self_ += 1
            return self_(*a, **k)

        def spy_core(*a, **k):
            self.core += 1
            return core(*a, **k)

        monkeypatch.setattr(ae, "cross_attention", spy_cross)
        monkeypatch.setattr(ae, "self_attention", spy_self)
        monkeypatch.setattr(attention, "attention_core", spy_core)

    def take(self):
        got = (self.cross, self.self_, self.core)
        self.cross = self.self_ = self.core = 0
        return got


def _layer_inputs(dtype=torch.float32, Q=37, bs=2, hw=150):
    g = torch.Generator().manual_seed(11)
    tgt, memory, pos = torch.randn(Q, bs, 128, generator=g), torch.randn(hw, bs, 128, generator=g), torch.randn(hw, bs, 128, generator=g)
    query_pos, sine = torch.randn(Q, bs, 128, generator=g), torch.randn(Q, bs, 256, generator=g)
    mask = torch.rand(bs, 1, Q, hw, generator=g) < 0.6
    mask[1, 0, 2] = True
    mask[0, 0, Q - 1] = True
    row_open = mask.all(-1, keepdim=True)
    f = lambda t: t.to(dtype).cuda()
    return dict(tgt=f(tgt), memory=f(memory), pos=f(pos), query_pos=f(query_pos), sine=f(sine), mask=mask.cuda(),
                row_open=row_open.cuda())


def _run_cross(layer, x, is_first, mask="mask", row_open="row_open", **kw):
    return layer(x["tgt"], x["memory"], memory_mask=None if mask is None else x[mask], pos=x["pos"], query_pos=x["query_pos"],
                 query_sine_embed=x["sine"], is_first=is_first, memory_row_open=None if row_open is None else x[row_open], **kw)


def _on_off_f64(on, off, ref, what):
    e_on, e_off = float((on.double() - ref).abs().max()), float((off.double() - ref).abs().max())
    top = float(ref.abs().max())
    print("%s: max|f64| %.3e  |on - f64| %.3e  |off - f64| %.3e" % (what, top, e_on, e_off))
    assert bool(torch.isfinite(on).all()) and e_on <= max(2 * e_off, 5e-6 * top), (what, e_on, e_off, top)


def test_layers_with_the_switch_on_against_the_switch_off_beside_float64(monkeypatch):
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    torch.manual_seed(7)
    ca, sa = dec.CrossAttentionLayer(128, 8).cuda().eval(), dec.SelfAttentionLayer(128, 8).cuda().eval()
    ca64, sa64 = copy.deepcopy(ca).double(), copy.deepcopy(sa).double()
    x, x64 = _layer_inputs(), _layer_inputs(torch.float64)
    spies = _Spies(monkeypatch)
    with torch.no_grad():
        for what, run in (("cross, first layer", lambda l, i: _run_cross(l, i, True)),
                          ("cross, later layer", lambda l, i: _run_cross(l, i, False)),
                          ("cross, no mask", lambda l, i: _run_cross(l, i, False, None, None)),
                          ("self", lambda l, i: l(i["tgt"], query_pos=i["query_pos"]))):
            layer, layer64 = (sa, sa64) if what == "self" else (ca, ca64)
            layer.attn_eval = "torch"
            off = run(layer, x)
            assert spies.take() == (0, 0, 1), what
            layer.attn_eval = "hip"
            on = run(layer, x)
            assert spies.take() == ((0, 1, 0) if what == "self" else (1, 0, 0)), what
            ref = run(layer64, x64)
            spies.take()
            _on_off_f64(on, off, ref, what)


def test_calls_the_kernels_do_not_take_keep_their_bits(monkeypatch):
    """Where a gradient is required, under autocast, with a key-padding mask, with a float mask, and in train mode with
    dropout, the switch changes nothing: the same branch, the same bits, the wrappers not entered."""
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    torch.manual_seed(8)
    ca, sa = dec.CrossAttentionLayer(128, 8).cuda().eval(), dec.SelfAttentionLayer(128, 8).cuda().eval()
    x = _layer_inputs()
    x["float_mask"] = torch.zeros(2, 1, 37, 150, device="cuda").masked_fill(x["mask"] & ~x["row_open"], -1e4)
    kpm = torch.zeros(2, 150, dtype=torch.bool, device="cuda")
    kpm[:, -7:] = True
    skpm = torch.zeros(2, 37, dtype=torch.bool, device="cuda")
    skpm[:, -3:] = True

    def with_grad(l, i):
        with torch.enable_grad():
            return _run_cross(l, dict(i, tgt=i["tgt"].clone().requires_grad_(True)), False).detach()

    def weights_with_grad(l, i):
        with torch.enable_grad():
            return (l(i["tgt"], query_pos=i["query_pos"]) if l is sa else _run_cross(l, i, True)).detach()

    def autocast(l, i):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return l(i["tgt"], query_pos=i["query_pos"]) if l is sa else _run_cross(l, i, False)

    runs = [("cross, gradient on tgt", ca, with_grad), ("cross, weights require a gradient", ca, weights_with_grad),
            ("self, weights require a gradient", sa, weights_with_grad),
            ("cross, autocast", ca, autocast), ("self, autocast", sa, autocast),
            ("cross, key-padding mask", ca, lambda l, i: _run_cross(l, i, False, memory_key_padding_mask=kpm)),
            ("self, key-padding mask", sa, lambda l, i: l(i["tgt"], query_pos=i["query_pos"], tgt_key_padding_mask=skpm)),
            ("cross, float mask", ca, lambda l, i: _run_cross(l, i, False, "float_mask", None)),
            ("self, mask", sa, lambda l, i: l(i["tgt"], query_pos=i["query_pos"], tgt_mask=torch.zeros(37, 37, device="cuda")))]
    spies = _Spies(monkeypatch)
    with torch.no_grad():
        for what, layer, run in runs:
            res = []
            for mode in ("torch", "hip"):
                layer.attn_eval = mode
                res.append(run(layer, x))
                assert spies.take()[:2] == (0, 0), what
            assert torch.equal(res[0], res[1]) and bool(torch.isfinite(res[0]).all()), what
    drop = dec.CrossAttentionLayer(128, 8, dropout=0.1).cuda()
    with torch.no_grad():
        drop.train()
        drop.attn_eval = "hip"
        _run_cross(drop, x, False)
        assert spies.take() == (0, 0, 1)                                  # dropout is live: the torch chain
        drop.eval()
        _run_cross(drop, x, False)
        assert spies.take() == (1, 0, 0)                                  # eval mode: dropout does nothing


def test_the_bf16_fused_branch_keeps_its_bits_with_the_switch_on(monkeypatch):
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    torch.manual_seed(9)
    ca = dec.CrossAttentionLayer(128, 8).cuda().eval().bfloat16()
    x = _layer_inputs(torch.bfloat16, hw=128)
    spies = _Spies(monkeypatch)
    res = []
    with torch.no_grad():
        for mode in ("torch", "hip"):
            ca.attn_eval = mode
            res.append(_run_cross(ca, x, False))
            assert spies.take()[:2] == (0, 0)                             # a bf16 kernel of fused_ops, not these wrappers
    assert torch.equal(res[0], res[1]) and bool(torch.isfinite(res[0].float()).all())


def test_whole_decoder_in_fp32_with_both_switches_on(golden, monkeypatch):
    """The dec_full_decoder fixture under no_grad on the device: every attention of the forward goes through the two wrappers
    (num_layers entries each), none through the torch chain; tolerances of
    test_decoder_golden.py::test_whole_decoder_on_the_fused_kernels_matches_the_reference_class."""
    from test_decoder_golden import _full_decoder, _t
    g = golden("dec_full_decoder")
    d = _full_decoder("cuda")
    switched = [m for m in d.modules() if hasattr(m, "attn_eval")]
    assert len(switched) == 2 * d.num_layers
    for m in switched:
        m.attn_eval = "hip"
    xs = [_t(g["x%d" % i]).cuda() for i in range(3)]
    spies = _Spies(monkeypatch)
    with torch.no_grad():
        out = d(xs, None, _t(g["mask_features"]).cuda())
    assert spies.take() == (d.num_layers, d.num_layers, 0)
    scale = max(1.0, float(np.abs(g["pred_masks"]).max()))
    np.testing.assert_allclose(out["pred_masks"].cpu().numpy(), g["pred_masks"], rtol=0, atol=5e-4 * scale)
    np.testing.assert_allclose(out["reference_points"].cpu().numpy(), g["reference_points"], rtol=0, atol=5e-5)
    assert len(out["aux_outputs"]) == int(g["n_aux"])
    for i, a in enumerate(out["aux_outputs"]):
        np.testing.assert_allclose(a["pred_masks"].cpu().numpy(), g["aux%d_pred_masks" % i], rtol=0, atol=5e-4 * scale)
    for i, a in enumerate(out["aux_reference_points"]):
        np.testing.assert_allclose(a["reference_points"].cpu().numpy(), g["aux%d_reference_points" % i], rtol=0, atol=5e-5)

"""GPU: the differentiable fp32 cross-attention with the keys divided over several workgroups
(pct_cross_attention_split_forward_f32 / pct_cross_attention_split_backward_f32, pctrans_amd/split_key_attention_train.py) against
the unsplit kernels of pctrans_amd/attention_train.py, bit for bit where the construction promises it, and against the float64
reference of attention_train_reference.py everywhere else.

Property (a): with one split all seven results (out, both lse planes, five gradients) are the unsplit kernels' bits.
Property (b): with any split count, a call whose queries each see the keys of one split only has the unsplit kernels' bits, too.
Accuracy: the rule of tests/test_attention_train_gpu.py, unchanged -- for `out` and each gradient
e_hip <= 2 * e_torch + 2^-22 * max|ref| with the fp32 torch chain on the same device as the yardstick; lse within 2^-20; dead
rows and blocked keys exactly zero.  tests/test_split_key_attention_train_cpu.py shows that three wrong combines miss these bounds
by more than 100 x on cases of this file."""
import copy

import pytest
import torch

import attention_train_reference as R
import split_key_attention_train_cases as K

pytestmark = pytest.mark.gpu


def _cuda(t):
    return None if t is None else t.cuda()


def _split(c, splits, ops=None):
    from pctrans_amd import split_key_attention_train as sk
    ops = [t.cuda() for t in c["ops"]] if ops is None else ops
    mask, ro, go = _cuda(c["mask"]), _cuda(c["row_open"]), c["grad_out"].cuda()
    assert sk.covered(*ops, c["heads"], mask, ro)
    out, lse = sk.cross_attention_forward(*ops, c["heads"], mask, ro, splits=splits)
    grads = sk.cross_attention_backward(*ops, c["heads"], mask, ro, out, lse, go, splits=splits)
    return (out, lse) + tuple(grads)


def _unsplit(c, ops=None):
    from pctrans_amd import attention_train as at
    ops = [t.cuda() for t in c["ops"]] if ops is None else ops
    mask, ro, go = _cuda(c["mask"]), _cuda(c["row_open"]), c["grad_out"].cuda()
    out, lse = at.cross_attention_forward(*ops, c["heads"], mask, ro)
    grads = at.cross_attention_backward(*ops, c["heads"], mask, ro, out, lse, go)
    return (out, lse) + tuple(grads)


def _same_bits(got, want):
    bad = [n for n, g, w in zip(("out", "lse") + K.NAMES[1:], got, want) if not torch.equal(g, w)]
    assert not bad, bad


# ---------------------------------------------------------------- (a) one split
@pytest.mark.parametrize("family,Q,S,heads", K.ONE_SPLIT, ids=lambda v: str(v))
def test_one_split_is_the_unsplit_kernels_bit_for_bit(family, Q, S, heads):
    c = R.case(family, Q, S, heads)
    _same_bits(_split(c, 1), _unsplit(c))


def test_two_splits_of_one_chunk_are_one_split():
    """S = 64 is one chunk: the entry uses min(splits, chunks)."""
    c = R.case("noise", 17, 64, 8)
    _same_bits(_split(c, 2), _unsplit(c))


# ---------------------------------------------------------------- (b) every query inside one split
@pytest.mark.parametrize("heads", (8, 4))
def test_queries_that_see_one_split_only_get_the_unsplit_bits(heads):
    c = K.window_case(heads)
    _same_bits(_split(c, K.WINDOW["splits"]), _unsplit(c))


# ---------------------------------------------------------------- accuracy against float64
def _accuracy(c, key, splits):
    Q = c["ops"][0].shape[0]
    got = _split(c, splits)
    out, lse, grads = got[0], got[1], got[2:]
    for n, q in c["dead_rows"]:                                         # a dead row: out, lse and its own gradients exactly 0
        assert float(out[q, n].abs().max()) == 0.0 and float(lse[:, n, :, q].abs().max()) == 0.0
        assert float(grads[0][q, n].abs().max()) == 0.0 and float(grads[1][q, n].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in got)
    if c["blocked_key"] is not None:                                    # masked for every query: exactly zero gradient rows
        for g in grads[2:]:
            assert float(g[c["blocked_key"]].abs().max()) == 0.0
    lse_err = float((lse.double().sum(0).cpu() - c["lse"]).abs().max())
    print("lse: error %.3e  bound %.3e" % (lse_err, K.lse_bound(c)))
    assert lse_err <= K.lse_bound(c), lse_err
    fig = K.rule(c, tuple(t.double().cpu() for t in (out,) + tuple(grads)), K.yardstick(c, key, "cuda"))
    for name, (e, b) in fig.items():
        print("%s: e_hip %.3e  bound %.3e" % (name, e, b))
    failed = [(n, e, b) for n, (e, b) in fig.items() if not e <= b]
    assert not failed, failed
    assert Q == out.shape[0]


@pytest.mark.parametrize("family,Q,S,heads,splits", K.ACCURACY, ids=lambda v: str(v))
def test_forward_and_backward_against_float64(family, Q, S, heads, splits):
    _accuracy(R.case(family, Q, S, heads), (family, Q, S, heads), splits)


def _big_splits():
    """`plan`'s count for the largest level; 7 (49 chunks in equal parts) as well, whatever the shipped constants route."""
    from pctrans_amd import split_key_attention_train as sk
    return sorted({max(1, sk.plan(K.BIG[0], R.N, 8, K.BIG[1])), 7})


def test_the_largest_level_at_the_plans_count_against_float64():
    c = R.case("noise_open", K.BIG[0], K.BIG[1], 8)
    for splits in _big_splits():
        _accuracy(c, ("noise_open",) + K.BIG + (8,), splits)


# ---------------------------------------------------------------- other properties of the entries
def test_two_calls_are_bit_identical():
    c = R.case("noise_open", K.BIG[0], K.BIG[1], 8)
    for splits in _big_splits():
        _same_bits(_split(c, splits), _split(c, splits))


def test_operands_at_a_16_byte_offset():
    """Every operand a view that starts 16 bytes into its allocation: the same bits as from aligned copies."""
    c = R.case("noise", 17, 129, 8)
    want = _split(c, 3)
    ops = []
    for t in c["ops"]:
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
        v = buf[4:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 32 == 16
        ops.append(v)
    _same_bits(_split(c, 3, ops), want)


def test_status_codes_on_device_pointers():
    """A workspace one byte short, a misaligned one and splits = 0 return their status and launch nothing: the outputs keep what
    they held.  An empty call returns 0."""
    from pctrans_amd import _lib, split_key_attention_train as sk
    L = _lib.lib()
    Q, S, N, heads, splits = 16, 129, 2, 8, 3
    c = R.case("noise_nomask", Q, S, heads)
    ops = [t.cuda() for t in c["ops"]]
    need = sk.workspace_bytes(N, heads, Q, splits)
    ws = torch.zeros(need // 8 + 2, dtype=torch.float64, device="cuda")
    out, lse = torch.full((Q, N, 128), 7.0, device="cuda"), torch.full((2, N, heads, Q), 7.0, device="cuda")
    grads = [torch.full_like(t, 7.0) for t in ops]
    go = c["grad_out"].cuda()
    p = [t.data_ptr() for t in ops]

    def fwd(splits=splits, w=ws.data_ptr(), nbytes=need, Q=Q):
        return L.pct_cross_attention_split_forward_f32(*p, None, None, N, heads, Q, S, R.SCALE, splits, w, nbytes, out.data_ptr(),
                                                       lse.data_ptr(), None)

    def bwd(splits=splits, w=ws.data_ptr(), nbytes=need, Q=Q):
        return L.pct_cross_attention_split_backward_f32(*p, None, None, None, lse.data_ptr(), go.data_ptr(), N, heads, Q, S, R.SCALE,
                                                        splits, w, nbytes, *[g.data_ptr() for g in grads], None)

    for call in (fwd, bwd):
        assert call(nbytes=need - 1) == -1 and call(w=ws.data_ptr() + 8) == -3 and call(splits=0) == -1 and call(splits=17) == -1
        assert call(w=None) == -1 and call(Q=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in [out, lse] + grads) and bool((ws == 0).all())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert float((out.double().cpu() - c["out"]).abs().max()) < 1e-4
    assert all(bool(torch.isfinite(g).all()) and not bool((g == 7.0).all()) for g in grads)
    assert bool((ws[need // 8:] == 0).all())                           # nothing behind the workspace is written


def test_supported_follows_the_plan_and_refuses_autocast(monkeypatch):
    from pctrans_amd import split_key_attention_train as sk
    monkeypatch.setattr(sk, "MIN_CHUNKS", 1)
    monkeypatch.setattr(sk, "TARGET_WORKGROUPS", 1 << 20)
    monkeypatch.setattr(sk, "MIN_KEYS", 1025)
    for S, want in ((1024, False), (1025, True)):
        ops = [torch.randn(T, 1, 128, device="cuda") for T in (3, 3, S, S, S)]
        assert sk.covered(*ops, 8) and sk.supported(*ops, 8) is want
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not sk.covered(*ops, 8) and not sk.supported(*ops, 8)
    assert not sk.supported(*[t.cpu() for t in ops], 8) and not sk.supported(*[t.half() for t in ops], 8)


def test_function_keeps_the_seven_tensors_and_the_split_count():
    from pctrans_amd import split_key_attention_train as sk
    c = R.case("noise_open", 100, 196, 8)
    ops = [t.cuda().requires_grad_(True) for t in c["ops"]]
    mask, ro = c["mask"].cuda(), c["row_open"].cuda()
    out = sk.cross_attention_train(*ops, 8, mask, ro, splits=2)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 7 and [tuple(t.shape) for t in saved[:5]] == [tuple(t.shape) for t in ops]
    assert tuple(saved[5].shape) == (100, 2, 128) and tuple(saved[6].shape) == (2, 2, 8, 100)
    g = torch.autograd.grad(out, ops, c["grad_out"].cuda())
    want = _split(c, 2)
    _same_bits((out.detach(), saved[6]) + tuple(g), want)


# ---------------------------------------------------------------- the layer
def _layer_inputs(dtype, Q, bs, hw):
    g = torch.Generator().manual_seed(23)
    tgt, memory, pos = torch.randn(Q, bs, 128, generator=g), torch.randn(hw, bs, 128, generator=g), torch.randn(hw, bs, 128, generator=g)
    query_pos, sine = torch.randn(Q, bs, 128, generator=g), torch.randn(Q, bs, 256, generator=g)
    mask = torch.rand(bs, 1, Q, hw, generator=g) < 0.6
    mask[1, 0, 2] = True                                               # fully masked rows, opened as the decoder opens them
    mask[0, 0, Q - 1] = True
    row_open = mask.all(-1, keepdim=True)
    grad = torch.randn(Q, bs, 128, generator=g)
    f = lambda t: t.to(dtype).cuda()
    x = dict(tgt=f(tgt), memory=f(memory), pos=f(pos), query_pos=f(query_pos), sine=f(sine), grad=f(grad))
    for k in ("tgt", "memory", "pos", "query_pos", "sine"):
        x[k].requires_grad_(True)
    x.update(mask=mask.cuda(), row_open=row_open.cuda())
    return x


def _layer_step(layer, x):
    """-> {name: tensor}: the layer's output and every parameter and input gradient of one forward + backward."""
    layer.zero_grad(set_to_none=True)
    leaves = [x[k] for k in ("tgt", "memory", "pos", "query_pos", "sine")]
    for t in leaves:
        t.grad = None
    out = layer(x["tgt"], x["memory"], memory_mask=x["mask"], pos=x["pos"], query_pos=x["query_pos"], query_sine_embed=x["sine"],
                is_first=True, memory_row_open=x["row_open"])
    out.backward(x["grad"])
    got = {"out": out.detach().clone()}
    got.update({"grad " + n: p.grad.detach().clone() for n, p in layer.named_parameters() if p.grad is not None})
    got.update({"grad input " + k: x[k].grad.detach().clone() for k in ("tgt", "memory", "pos", "query_pos", "sine")})
    return got


class _Spies:
    def __init__(self, monkeypatch):
        from pctrans_amd import attention_train as at, split_key_attention_train as sk
        from pctrans_amd.transformer_decoder import attention
        self.counts = dict(split_fwd=0, split_bwd=0, unsplit_fwd=0, unsplit_bwd=0, core=0)
        for owner, attr, key in ((sk, "cross_attention_forward", "split_fwd"), (sk, "cross_attention_backward", "split_bwd"),
                                 (at, "cross_attention_forward", "unsplit_fwd"), (at, "cross_attention_backward", "unsplit_bwd"),
                                 (attention, "attention_core", "core")):
            monkeypatch.setattr(owner, attr, self._spy(getattr(owner, attr), key))

    def _spy(self, real, key):
        def spy(*a, **k):
            self.counts[key] += 1
            return real(*a, **k)
        return spy

    def take(self):
        got = dict(self.counts)
        for k in self.counts:
            self.counts[k] = 0
        return got


def test_layer_with_the_switch_on_against_the_switch_off_beside_float64(monkeypatch):
    """S = 1 040 keys (17 chunks, the last of 16 keys), Q = 17, N = 2, the decoder's mask and row_open, the plan forced to route
    it.  "hip": the split wrappers are entered once each and the torch core is not; "torch": the reverse.  Output and every
    parameter and input gradient within max(2 |torch - f64|, 5e-6 max|f64|) of a float64 copy of the layer."""
    from pctrans_amd import split_key_attention_train as sk
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    monkeypatch.setattr(sk, "MIN_CHUNKS", 1)
    monkeypatch.setattr(sk, "TARGET_WORKGROUPS", 1 << 20)
    monkeypatch.setattr(sk, "MIN_KEYS", 1025)
    Q, bs, hw = 17, 2, 1040
    assert sk.plan(Q, bs, 8, hw) >= 2
    torch.manual_seed(7)
    ca = dec.CrossAttentionLayer(128, 8).cuda().train()
    ca64 = copy.deepcopy(ca).double()
    x, x64 = _layer_inputs(torch.float32, Q, bs, hw), _layer_inputs(torch.float64, Q, bs, hw)
    spies = _Spies(monkeypatch)
    assert ca.attn_train == "torch" and ca.attn_train_split == "torch"
    off = _layer_step(ca, x)
    assert spies.take() == dict(split_fwd=0, split_bwd=0, unsplit_fwd=0, unsplit_bwd=0, core=1)
    ca.attn_train_split = "hip"
    on = _layer_step(ca, x)
    assert spies.take() == dict(split_fwd=1, split_bwd=1, unsplit_fwd=0, unsplit_bwd=0, core=0)
    ref = _layer_step(ca64, x64)
    assert on.keys() == off.keys() == ref.keys() and len(on) >= 20
    failed = []
    for name in ref:
        e_on, e_off = (float((t[name].double() - ref[name]).abs().max()) for t in (on, off))
        top = float(ref[name].abs().max())
        print("%s: max|f64| %.3e  |on - f64| %.3e  |off - f64| %.3e" % (name, top, e_on, e_off))
        if not (bool(torch.isfinite(on[name]).all()) and e_on <= max(2 * e_off, 5e-6 * top)):
            failed.append((name, e_on, e_off, top))
    assert not failed, failed


def test_the_unsplit_route_keeps_what_it_takes(monkeypatch):
    """S = 1 024 with both switches "hip": attention_train.supported comes first and keeps the call; without it the call goes
    to the torch chain, not to the split kernels (the shipped MIN_KEYS)."""
    from pctrans_amd import split_key_attention_train as sk
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    monkeypatch.setattr(sk, "MIN_CHUNKS", 1)
    monkeypatch.setattr(sk, "TARGET_WORKGROUPS", 1 << 20)
    monkeypatch.setattr(sk, "MIN_KEYS", 1)                             # even a plan that would route 1 024 keys
    Q, bs, hw = 17, 2, 1024
    assert sk.plan(Q, bs, 8, hw) >= 2
    torch.manual_seed(7)
    ca = dec.CrossAttentionLayer(128, 8).cuda().train()
    x = _layer_inputs(torch.float32, Q, bs, hw)
    spies = _Spies(monkeypatch)
    ca.attn_train = ca.attn_train_split = "hip"
    _layer_step(ca, x)
    assert spies.take() == dict(split_fwd=0, split_bwd=0, unsplit_fwd=1, unsplit_bwd=1, core=0)
    monkeypatch.setattr(sk, "MIN_KEYS", 1025)
    ca.attn_train = "torch"
    _layer_step(ca, x)
    assert spies.take() == dict(split_fwd=0, split_bwd=0, unsplit_fwd=0, unsplit_bwd=0, core=1)

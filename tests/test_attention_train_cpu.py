"""CPU: the C ABI entries of the differentiable cross-attention (header, library, binding, status codes that need no device);
the `attn_train` switch and its fallback on CPU tensors; the float64 reference of test_attention_train_gpu.py
(attention_train_reference.py) against torch autograd on the float64 torch chain, and the conditions the GPU tests place on
their inputs, checked on the reference alone."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import attention_train_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pct_cross_attention_forward_f32", "pct_cross_attention_backward_f32")


def test_abi_declares_exports_and_binds_the_entries():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_attn_train.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_attn_train.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_lib.ATTN_TRAIN_SYMBOLS) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.SEG_SYMBOLS, _lib.FPN_SYMBOLS):
            assert name not in other
        argtypes, restype, checked_by = _lib.ATTN_TRAIN_SYMBOLS[name]
        assert name in open(os.path.join(ROOT, checked_by)).read()
        assert re.search(r"\bT %s\b" % name, out)
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == argtypes and fn.restype is restype
        # the argument count of the declaration is the table's
        decl = re.search(r"PCT_API int %s\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == len(argtypes), name
    assert len(_lib.ATTN_TRAIN_SYMBOLS[NAMES[0]][0]) == 15 and len(_lib.ATTN_TRAIN_SYMBOLS[NAMES[1]][0]) == 22
    assert _lib.lib().pct_abi_version() == 1 and _lib.ABI_VERSION == 1


def test_status_codes_need_no_device():
    """Arguments are checked on the host before any launch: host pointers stand in and are never dereferenced."""
    from pctrans_amd import _lib
    L = _lib.lib()
    OK, BAD, ALIGN, UNSUP = 0, -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    fwd = lambda a=p, N=2, h=8, Q=5, S=7, out=p, lse=p, q_c=p: L.pct_cross_attention_forward_f32(
        q_c, a, p, p, p, None, None, N, h, Q, S, 0.1, out, lse, None)
    bwd = lambda N=2, h=8, Q=5, S=7, ws=p, go=p, gv=p: L.pct_cross_attention_backward_f32(
        p, p, p, p, p, None, None, p, p, go, N, h, Q, S, 0.1, ws, p, p, p, p, gv, None)
    for f in (fwd, bwd):
        assert f(N=-1) == BAD and f(Q=-1) == BAD and f(S=-1) == BAD and f(h=0) == BAD
        assert f(N=0) == OK and f(Q=0) == OK and f(S=0) == OK
        assert f(h=3) == UNSUP and f(h=16) == UNSUP and f(N=70000) == UNSUP and f(Q=1 << 24) == UNSUP
    assert fwd(q_c=None) == BAD and fwd(out=None) == BAD and fwd(lse=None) == BAD
    assert bwd(ws=None) == BAD and bwd(go=None) == BAD and bwd(gv=None) == BAD
    assert fwd(a=p + 4) == ALIGN and fwd(out=p + 8) == ALIGN
    assert bwd(go=p + 4) == ALIGN and bwd(gv=p + 8) == ALIGN and bwd(ws=p + 4) == ALIGN
    assert fwd(N=0, q_c=None) == OK                                      # an empty call is not asked for pointers


def test_switch_default_follows_the_environment(monkeypatch):
    from pctrans_amd import attention_train
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    monkeypatch.delenv("PCT_ATTN_TRAIN", raising=False)
    assert attention_train.default() == "torch" and CrossAttentionLayer(128, 8).attn_train == "torch"
    monkeypatch.setenv("PCT_ATTN_TRAIN", "hip")
    assert attention_train.default() == "hip" and CrossAttentionLayer(128, 8).attn_train == "hip"
    monkeypatch.setenv("PCT_ATTN_TRAIN", "")
    assert attention_train.default() == "torch"
    monkeypatch.setenv("PCT_ATTN_TRAIN", "triton")
    with pytest.raises(RuntimeError):
        attention_train.default()


def test_cpu_tensors_are_not_supported_and_workspace_formula():
    from pctrans_amd import attention_train
    c = R.case("noise_open", 17, 65, 8)
    assert not attention_train.supported(*c["ops"], 8, c["mask"], c["row_open"])
    assert not attention_train.supported(*c["ops"], 8)
    assert not attention_train.covered(*c["ops"], 8, c["mask"], c["row_open"]) and attention_train.MAX_KEYS == 1024
    with pytest.raises(RuntimeError):
        attention_train.cross_attention_train(*c["ops"], 8, c["mask"], c["row_open"])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        attention_train.cross_attention_forward(*c["ops"], 8)
    assert attention_train.workspace_bytes(2, 8, 300) == 4 * 2 * 8 * 300


def test_cpu_layer_with_the_switch_on_is_the_layer_with_it_off(monkeypatch):
    """On CPU tensors the switch changes nothing: outputs and gradients are bit-equal, and the device path is not entered."""
    from pctrans_amd import attention_train
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    monkeypatch.setattr(attention_train, "cross_attention_train", lambda *a, **k: (_ for _ in ()).throw(AssertionError()))
    torch.manual_seed(5)
    layer = CrossAttentionLayer(128, 8)
    Q, bs, hw = 6, 2, 20
    g = torch.Generator().manual_seed(6)
    tgt, memory, pos = torch.randn(Q, bs, 128, generator=g), torch.randn(hw, bs, 128, generator=g), torch.randn(hw, bs, 128, generator=g)
    query_pos, sine = torch.randn(Q, bs, 128, generator=g), torch.randn(Q, bs, 256, generator=g)
    mask = torch.rand(bs, 1, Q, hw, generator=g) < 0.5
    mask[1, 0, 2] = True
    row_open = mask.all(-1, keepdim=True)
    res = []
    for mode in ("torch", "hip"):
        layer.attn_train = mode
        layer.zero_grad(set_to_none=True)
        t = tgt.clone().requires_grad_(True)
        out = layer(t, memory, memory_mask=mask, pos=pos, query_pos=query_pos, query_sine_embed=sine, is_first=True,
                    memory_row_open=row_open)
        out.square().sum().backward()
        res.append((out.detach(), t.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2].keys() == res[1][2].keys() and all(torch.equal(res[0][2][n], res[1][2][n]) for n in res[0][2])
    assert torch.isfinite(res[0][0]).all()


@pytest.mark.parametrize("family,Q,S,heads", [("noise_open", 17, 65, 8), ("noise_nomask", 16, 63, 4), ("noise", 5, 9, 8),
                                              ("peaked", 17, 64, 8), ("window_masks", 16, 65, 4), ("noise_open", 1, 63, 8)])
def test_reference_gradients_are_autograd_of_the_float64_torch_chain(family, Q, S, heads):
    """1e-12 relative on every live row.  Torch's masked softmax is NaN on a dead row and autograd spreads that NaN over the
    key gradients, so the chain runs with the dead rows' mask rows cleared and their grad_out rows zeroed -- which gives those
    rows no gradient and leaves every other row's terms as they were; the reference must match that with the dead rows in."""
    c = R.case(family, Q, S, heads)
    ops = [t.double() for t in c["ops"]]
    mask, go = c["mask"], c["grad_out"].double().clone()
    if c["dead_rows"]:
        mask = mask.clone()
        for n, q in c["dead_rows"]:
            mask[n, 0, q] = False
            go[q, n] = 0
    out, grads = R.torch_chain_grads(ops, heads, mask, c["row_open"], go)
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    live = torch.ones(Q, R.N, dtype=torch.bool)
    for n, q in c["dead_rows"]:
        live[q, n] = False
        assert float(c["out"][q, n].abs().max()) == 0.0 and float(c["lse"][n, :, q].abs().max()) == 0.0
        assert float(c["grads"][0][q, n].abs().max()) == 0.0 and float(c["grads"][1][q, n].abs().max()) == 0.0
    assert rel(c["out"][live], out[live]) <= 1e-12
    for name, g, w in zip(("grad_q_c", "grad_q_s", "grad_k_c", "grad_k_p", "grad_v"), c["grads"], grads):
        assert g.shape == w.shape and rel(g, w) <= 1e-12, name


def test_reference_meets_the_conditions_of_the_gpu_tests():
    """Every case the GPU tests run: each row has an attendable key or is a declared dead row, nothing of the reference is
    non-finite, no lse comes near the fp32 range, a blocked key has exactly zero gradient rows, and the case is cached."""
    import test_attention_train_gpu as G
    assert len(G.CASES) > 150
    for family, Q, S, heads in G.CASES:
        c = R.case(family, Q, S, heads)
        assert c is R.case(family, Q, S, heads)
        m = R.effective_mask(c["mask"], c["row_open"], R.N, Q, S)
        dead = set(c["dead_rows"])
        if m is None:
            assert not dead
        else:
            assert dead == {(int(n), int(q)) for n, q in m.all(-1).reshape(R.N, Q).nonzero().tolist()}
        if family in ("noise", "window_masks") and Q > 2 and m is not None:
            assert dead, (family, Q, S)
        for t in (c["out"], c["lse"]) + tuple(c["grads"]):
            assert torch.isfinite(t).all(), (family, Q, S)
        assert float(c["lse"].abs().max()) < 1e6
        if c["blocked_key"] is not None:
            assert c["row_open"] is None and bool(c["mask"][:, :, :, c["blocked_key"]].all())
            for g in c["grads"][2:]:
                assert float(g[c["blocked_key"]].abs().max()) == 0.0
    assert any(R.case(*k)["row_open"] is not None and bool(R.case(*k)["row_open"].any()) for k in G.CASES)

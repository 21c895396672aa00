"""CPU: the C ABI entries of the differentiable self-attention (header, library, binding, status codes that need no device);
the `self_attn_train` switch and its fallback on CPU tensors; the float64 reference of test_self_attention_train_gpu.py
(self_attention_train_reference.py) against torch autograd on the float64 torch chain, and the conditions the GPU tests place
on their inputs, checked on the reference alone."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import self_attention_train_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pct_self_attention_forward_f32", "pct_self_attention_backward_f32")


def test_abi_declares_exports_and_binds_the_entries():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_self_attn_train.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_self_attn_train.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_lib.SELF_ATTN_TRAIN_SYMBOLS) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.SEG_SYMBOLS, _lib.FPN_SYMBOLS,
                      _lib.ATTN_TRAIN_SYMBOLS):
            assert name not in other
        argtypes, restype, checked_by = _lib.SELF_ATTN_TRAIN_SYMBOLS[name]
        assert name in open(os.path.join(ROOT, checked_by)).read()
        assert re.search(r"\bT %s\b" % name, out)
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == argtypes and fn.restype is restype
        # the argument count of the declaration is the table's
        decl = re.search(r"PCT_API int %s\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == len(argtypes), name
    assert len(_lib.SELF_ATTN_TRAIN_SYMBOLS[NAMES[0]][0]) == 12 and len(_lib.SELF_ATTN_TRAIN_SYMBOLS[NAMES[1]][0]) == 17
    assert _lib.lib().pct_abi_version() == 1 and _lib.ABI_VERSION == 1


def test_status_codes_need_no_device():
    """Arguments are checked on the host before any launch: host pointers stand in and are never dereferenced."""
    from pctrans_amd import _lib
    L = _lib.lib()
    OK, BAD, ALIGN, UNSUP = 0, -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    fwd = lambda a=p, N=2, h=8, Q=5, out=p, lse=p, q_c=p: L.pct_self_attention_forward_f32(
        q_c, a, p, p, p, N, h, Q, 0.25, out, lse, None)
    bwd = lambda N=2, h=8, Q=5, ws=p, go=p, gv=p, o=p: L.pct_self_attention_backward_f32(
        p, p, p, p, p, o, p, go, N, h, Q, 0.25, ws, p, p, gv, None)
    for f in (fwd, bwd):
        assert f(N=-1) == BAD and f(Q=-1) == BAD and f(h=0) == BAD and f(h=-8) == BAD
        assert f(N=0) == OK and f(Q=0) == OK
        assert f(h=5) == UNSUP and f(h=3) == UNSUP and f(h=16) == UNSUP and f(N=70000) == UNSUP
        assert f(Q=513) == UNSUP and f(Q=1 << 24) == UNSUP              # beyond the LDS image of the backward
    assert fwd(q_c=None) == BAD and fwd(out=None) == BAD and fwd(lse=None) == BAD
    assert bwd(ws=None) == BAD and bwd(go=None) == BAD and bwd(gv=None) == BAD
    assert fwd(a=p + 4) == ALIGN and fwd(out=p + 8) == ALIGN and fwd(q_c=p + 4) == ALIGN
    assert bwd(go=p + 4) == ALIGN and bwd(gv=p + 8) == ALIGN and bwd(ws=p + 4) == ALIGN
    assert fwd(N=0, q_c=None) == OK                                      # an empty call is not asked for pointers
    assert bwd(N=0, o=None) == OK


def test_switch_default_follows_the_environment(monkeypatch):
    from pctrans_amd import self_attention_train
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import SelfAttentionLayer
    monkeypatch.delenv("PCT_SELF_ATTN_TRAIN", raising=False)
    assert self_attention_train.default() == "torch" and SelfAttentionLayer(128, 8).self_attn_train == "torch"
    assert not hasattr(SelfAttentionLayer(128, 8), "attn_train")
    monkeypatch.setenv("PCT_SELF_ATTN_TRAIN", "hip")
    assert self_attention_train.default() == "hip" and SelfAttentionLayer(128, 8).self_attn_train == "hip"
    monkeypatch.setenv("PCT_SELF_ATTN_TRAIN", "")
    assert self_attention_train.default() == "torch"
    monkeypatch.setenv("PCT_SELF_ATTN_TRAIN", "triton")
    with pytest.raises(RuntimeError, match="PCT_SELF_ATTN_TRAIN must be 'hip' or 'torch', got 'triton'"):
        self_attention_train.default()


def test_cpu_tensors_are_not_covered_and_workspace_formula():
    from pctrans_amd import self_attention_train
    c = R.case("noise", 17, 8)
    assert not self_attention_train.covered(*c["ops"], 8) and not self_attention_train.supported(*c["ops"], 8)
    assert self_attention_train.MAX_QUERIES == 512
    with pytest.raises(RuntimeError):
        self_attention_train.self_attention_train(*c["ops"], 8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        self_attention_train.self_attention_forward(*c["ops"], 8)
    assert self_attention_train.workspace_bytes(2, 8, 300) == 4 * 2 * 8 * 300


def test_cpu_layer_with_the_switch_on_is_the_layer_with_it_off(monkeypatch):
    """On CPU tensors the switch changes nothing: outputs and gradients are bit-equal, the device path is not entered, and the
    state-dict keys are the layer's."""
    from pctrans_amd import self_attention_train
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import SelfAttentionLayer
    monkeypatch.setattr(self_attention_train, "self_attention_train", lambda *a, **k: (_ for _ in ()).throw(AssertionError()))
    torch.manual_seed(5)
    layer = SelfAttentionLayer(128, 8)
    assert sorted(layer.state_dict()) == sorted(
        "%s.%s" % (m, w) for m in ("sa_qcontent_proj", "sa_qpos_proj", "sa_kcontent_proj", "sa_kpos_proj", "sa_v_proj",
                                   "self_attn.out_proj", "norm1") for w in ("weight", "bias"))
    g = torch.Generator().manual_seed(6)
    tgt, query_pos = torch.randn(6, 2, 128, generator=g), torch.randn(6, 2, 128, generator=g)
    res = []
    for mode in ("torch", "hip"):
        layer.self_attn_train = mode
        layer.zero_grad(set_to_none=True)
        t = tgt.clone().requires_grad_(True)
        out = layer(t, query_pos=query_pos)
        out.square().sum().backward()
        res.append((out.detach(), t.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2].keys() == res[1][2].keys() and all(torch.equal(res[0][2][n], res[1][2][n]) for n in res[0][2])
    assert torch.isfinite(res[0][0]).all()


@pytest.mark.parametrize("family,Q,heads", R.CASES, ids=lambda v: str(v))
def test_reference_gradients_are_autograd_of_the_float64_torch_chain(family, Q, heads):
    """1e-12 relative, on every case of the GPU test.  The float64 chain gets the parts' fp32 sums (q and k as the kernels and
    the fp32 chain see them) with a zero second part, so its adds are exact; the gradients of the two parts of q are one tensor,
    and so are those of k."""
    c = R.case(family, Q, heads)
    q_c, q_p, k_c, k_p, v = c["ops"]
    ops = [(q_c + q_p).double(), torch.zeros_like(q_p).double(), (k_c + k_p).double(), torch.zeros_like(k_p).double(), v.double()]
    out, grads = R.torch_chain_grads(ops, heads, c["grad_out"].double())
    rel = lambda a, b, floor=1e-300: float((a - b).abs().max()) / max(float(b.abs().max()), floor)
    assert rel(c["out"], out) <= 1e-12
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[2], grads[3])
    # a row with one key of weight 1 (Q = 1, one_hot) has dS = dP - D = 0 mathematically, and two evaluation orders leave
    # different roundings of it: the error is taken against the size of the terms that cancel, |dP| |operand| scale
    term = float(c["grad_out"].abs().max()) * float(v.abs().max()) * R.SCALE
    floors = (term * float(ops[2].abs().max()), term * float(ops[0].abs().max()), 1e-300)
    for name, g, w, floor in zip(("grad_q", "grad_k", "grad_v"), c["grads"], (grads[0], grads[2], grads[4]), floors):
        assert g.shape == w.shape and rel(g, w, floor) <= 1e-12, name
    assert abs(float(c["p"].sum(-1).min()) - 1) < 1e-12 and abs(float(c["p"].sum(-1).max()) - 1) < 1e-12


def test_split_operands_sum_exactly():
    """Content + position part in fp32 is the family's q (and k) bit for bit, and neither part is trivial."""
    for family, Q, heads in R.CASES:
        c = R.case(family, Q, heads)
        assert c is R.case(family, Q, heads)
        if family == "noise":
            assert c["q"] is None
            continue
        q_c, q_p, k_c, k_p, _ = c["ops"]
        assert torch.equal(q_c + q_p, c["q"]) and torch.equal(k_c + k_p, c["k"])
        assert torch.equal((q_c.double() + q_p.double()).float(), c["q"])
        nz = c["k"] != 0
        assert bool((k_c[nz] != 0).all()) and bool((k_p[nz] != 0).all())


def test_reference_meets_the_conditions_of_the_gpu_tests():
    """The hard families are as hard as the GPU test assumes, asserted from the reference alone: the largest |score| and the
    smallest winning probability of a row per family; everything finite; no lse near the fp32 range."""
    import test_self_attention_train_gpu as G
    assert G.CASES == R.CASES and len(R.CASES) == 37
    top, win = {}, {}
    for family, Q, heads in R.CASES:
        c = R.case(family, Q, heads)
        for t in (c["out"], c["lse"], c["p"]) + tuple(c["grads"]):
            assert torch.isfinite(t).all(), (family, Q)
        assert float(c["lse"].abs().max()) < 1e6
        q, k = R._summed(*c["ops"][:4])
        s = R._heads_first(q, heads) @ R._heads_first(k, heads).transpose(2, 3) * R.SCALE
        top[family] = max(top.get(family, 0.0), float(s.abs().max()))
        if Q >= 63:
            win[family] = min(win.get(family, 1.0), float(c["p"].amax(-1).min()))
    assert top["noise"] < 20
    assert 40 < top["peaked"] < 120
    assert 400 < top["underflow"] < 1000
    assert 30000 < top["one_hot"] < 70000
    assert win["one_hot"] == 1.0                                          # every other key is at least 64 below the winner
    assert win["noise"] < 0.2 and win["peaked"] < 0.9                     # rows with several live keys exist
    big = R.case("underflow", 100, 8)["p"]
    assert float((big < 2.0 ** -126).double().mean()) > 0.5               # most probabilities are below fp32's normal range

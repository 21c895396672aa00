"""CPU: the C ABI entries of the decoder's attention in fp32 evaluation (header, library, binding, status codes that need no
device); the `attn_eval` switch and what it does on CPU tensors (nothing); and, on the float64 references of
test_attention_eval_gpu.py alone, the conditions that file places on its inputs and the claim a skip of fully masked tiles would
rest on: such a tile leaves the online-softmax state of every query as it was."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attention_train_reference as R
import self_attention_train_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pct_cross_attention_eval_f32", "pct_self_attention_eval_f32")


def test_abi_declares_exports_and_binds_the_entries():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_attn_eval.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_attn_eval.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_lib.ATTN_EVAL_SYMBOLS) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.ATTN_TRAIN_SYMBOLS, _lib.SELF_ATTN_TRAIN_SYMBOLS):
            assert name not in other
        argtypes, restype, checked_by = _lib.ATTN_EVAL_SYMBOLS[name]
        assert name in open(os.path.join(ROOT, checked_by)).read()
        assert re.search(r"\bT %s\b" % name, out)
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == argtypes and fn.restype is restype
        decl = re.search(r"PCT_API int %s\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == len(argtypes), name
    assert len(_lib.ATTN_EVAL_SYMBOLS[NAMES[0]][0]) == 14 and len(_lib.ATTN_EVAL_SYMBOLS[NAMES[1]][0]) == 11


def test_status_codes_need_no_device():
    """Arguments are checked on the host before any launch: host pointers stand in and are never dereferenced."""
    from pctrans_amd import _lib
    L = _lib.lib()
    OK, BAD, ALIGN, UNSUP = 0, -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    cross = lambda a=p, N=2, h=8, Q=5, S=7, out=p, q_c=p: L.pct_cross_attention_eval_f32(
        q_c, a, p, p, p, None, None, N, h, Q, S, 0.1, out, None)
    self_ = lambda a=p, N=2, h=8, Q=5, S=None, out=p, q_c=p: L.pct_self_attention_eval_f32(q_c, a, p, p, p, N, h, Q, 0.1, out, None)
    for f in (cross, self_):
        assert f(N=-1) == BAD and f(Q=-1) == BAD and f(h=0) == BAD
        assert f(N=0) == OK and f(Q=0) == OK
        assert f(h=3) == UNSUP and f(h=16) == UNSUP and f(N=70000) == UNSUP and f(Q=1 << 24) == UNSUP
        assert f(q_c=None) == BAD and f(out=None) == BAD
        assert f(a=p + 4) == ALIGN and f(out=p + 8) == ALIGN
        assert f(N=0, q_c=None) == OK                                    # an empty call is not asked for pointers
    assert cross(S=-1) == BAD and cross(S=0) == OK and cross(S=1 << 24) == UNSUP


def test_switch_default_follows_the_environment(monkeypatch):
    from pctrans_amd import attention_eval
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer, SelfAttentionLayer
    for value, want in ((None, "torch"), ("", "torch"), ("hip", "hip"), ("torch", "torch")):
        monkeypatch.delenv("PCT_ATTN_EVAL", raising=False) if value is None else monkeypatch.setenv("PCT_ATTN_EVAL", value)
        assert attention_eval.default() == want
        assert CrossAttentionLayer(128, 8).attn_eval == want and SelfAttentionLayer(128, 8).attn_eval == want
    monkeypatch.setenv("PCT_ATTN_EVAL", "triton")
    with pytest.raises(RuntimeError, match=re.escape("PCT_ATTN_EVAL must be 'hip' or 'torch', got 'triton'")):
        attention_eval.default()


def test_cpu_bf16_and_mis_shaped_tensors_are_not_covered():
    from pctrans_amd import attention_eval as ae
    c = R.case("noise_open", 17, 65, 8)
    for pred in (ae.covered, ae.supported):
        assert not pred(*c["ops"], 8, c["mask"], c["row_open"]) and not pred(*c["ops"], 8)
        assert not pred(*[t.bfloat16() for t in c["ops"]], 8)
        assert not pred(*c["ops"][:4], c["ops"][4][:-1], 8) and not pred(*c["ops"], 4)
        s = SR.case("noise", 17, 8)
        assert not pred(*s["ops"], 8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ae.cross_attention(*c["ops"], 8, c["mask"], c["row_open"])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ae.self_attention(*SR.case("noise", 17, 8)["ops"], 8)


def test_a_switch_value_other_than_torch_or_hip_raises():
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer, SelfAttentionLayer
    g = torch.Generator().manual_seed(2)
    t, mem = torch.randn(3, 1, 128, generator=g), torch.randn(5, 1, 128, generator=g)
    sa, ca = SelfAttentionLayer(128, 8).eval(), CrossAttentionLayer(128, 8).eval()
    sa.attn_eval = ca.attn_eval = "triton"
    with torch.no_grad():
        with pytest.raises(ValueError, match="SelfAttentionLayer.attn_eval"):
            sa(t, query_pos=t)
        with pytest.raises(ValueError, match="CrossAttentionLayer.attn_eval"):
            ca(t, mem, pos=mem, query_pos=t, query_sine_embed=torch.randn(3, 1, 256, generator=g), is_first=True)


def test_cpu_layers_with_the_switch_on_are_the_layers_with_it_off(monkeypatch):
    """On CPU tensors the switch changes nothing: the outputs are bit-equal and the device path is not entered."""
    from pctrans_amd import attention_eval as ae
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer, SelfAttentionLayer
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError())
    monkeypatch.setattr(ae, "cross_attention", boom)
    monkeypatch.setattr(ae, "self_attention", boom)
    torch.manual_seed(5)
    ca, sa = CrossAttentionLayer(128, 8).eval(), SelfAttentionLayer(128, 8).eval()
    Q, bs, hw = 6, 2, 20
    g = torch.Generator().manual_seed(6)
    tgt, memory, pos = torch.randn(Q, bs, 128, generator=g), torch.randn(hw, bs, 128, generator=g), torch.randn(hw, bs, 128, generator=g)
    query_pos, sine = torch.randn(Q, bs, 128, generator=g), torch.randn(Q, bs, 256, generator=g)
    mask = torch.rand(bs, 1, Q, hw, generator=g) < 0.5
    mask[1, 0, 2] = True
    row_open = mask.all(-1, keepdim=True)
    res = []
    with torch.no_grad():
        for mode in ("torch", "hip"):
            ca.attn_eval = sa.attn_eval = mode
            res.append((ca(tgt, memory, memory_mask=mask, pos=pos, query_pos=query_pos, query_sine_embed=sine, is_first=True,
                           memory_row_open=row_open),
                        ca(tgt, memory, memory_mask=mask, pos=pos, query_pos=query_pos, query_sine_embed=sine, is_first=False,
                           memory_row_open=row_open),
                        sa(tgt, query_pos=query_pos)))
    for a, b in zip(*res):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---- on the references alone ----------------------------------------------------------------------------------------------------
def _online_softmax_over_masked_steps(c, Q, S):
    """The forward's online softmax in numpy float64 on the case's float64 scores, per (image, head, query), wave w walking
    the 16-key steps w, w + 4, ... (csrc/attn_train_common.hpp: fwd_step).  -> (steps that were fully masked for a query, how
    many of those met a state that already held a key, 16 x 16 tiles fully masked for all their queries); asserts on every
    fully masked step that each p is exactly 0 and that the state (m, l, O) is left bit for bit as it was, with the factor
    exp(0) = 1 where the state holds a key and on the untouched state (-inf, 0, 0) otherwise."""
    heads = c["heads"]
    hf = lambda t: R._heads_first(t.double(), heads).numpy()
    qc, qs, kc, kp, vh = (hf(t) for t in c["ops"])
    x = (qc @ kc.transpose(0, 1, 3, 2) + qs @ kp.transpose(0, 1, 3, 2)) * R.SCALE          # [N, h, Q, S]
    m = R.effective_mask(c["mask"], c["row_open"], R.N, Q, S)
    dead = np.zeros((R.N, 1, Q, S), dtype=bool) if m is None else m.numpy()
    T = -(-S // 16)
    pad = 16 * T - S
    x = np.pad(x, ((0, 0),) * 3 + ((0, pad),))
    dead = np.broadcast_to(np.pad(dead, ((0, 0),) * 3 + ((0, pad),), constant_values=True), x.shape)
    vh = np.pad(vh, ((0, 0), (0, 0), (0, pad), (0, 0)))
    masked_steps = on_live_state = 0
    with np.errstate(invalid="ignore"):
        for w in range(4):
            m_run = np.full(x.shape[:3], -np.inf)
            l_run = np.zeros(x.shape[:3])
            o = np.zeros(x.shape[:3] + (16,))
            for t in range(w, T, 4):
                sl = slice(16 * t, 16 * t + 16)
                d = dead[..., sl]
                mx = np.where(d, -np.inf, x[..., sl]).max(-1)
                m_new = np.maximum(m_run, mx)
                m_safe = np.where(np.isneginf(m_new), 0.0, m_new)
                alpha = np.exp(m_run - m_safe)
                p = np.where(d, 0.0, np.exp(x[..., sl] - m_safe[..., None]))
                l_new = l_run * alpha + p.sum(-1)
                o_new = o * alpha[..., None] + p @ vh[:, :, sl]
                full = d.all(-1)                                          # this step holds no key for the query
                assert (p[full] == 0.0).all()
                held = full & ~np.isneginf(m_run)
                assert (alpha[held] == 1.0).all() and (alpha[full & ~held] == 0.0).all()
                assert (l_run[full & ~held] == 0.0).all() and (o[full & ~held] == 0.0).all()
                for new, old in ((m_new, m_run), (l_new, l_run), (o_new, o)):
                    assert np.array_equal(new[full].view(np.int64), old[full].view(np.int64))
                masked_steps += int(full.sum())
                on_live_state += int(held.sum())
                m_run, l_run, o = m_new, l_new, o_new
    tiles = dead.reshape(R.N, -1, Q, T, 16).all(-1)[:, 0]                 # [N, Q, T]
    qpad = -Q % 16
    tiles = np.pad(tiles, ((0, 0), (0, qpad), (0, 0)), mode="edge").reshape(R.N, -1, 16, T).all(2)
    return masked_steps, on_live_state, int(tiles.sum())


@pytest.mark.parametrize("family,Q,S", [("window_masks", 100, 374), ("window_masks", 300, 4096), ("noise", 100, 374),
                                        ("noise", 17, 65)])
def test_a_fully_masked_step_leaves_the_online_softmax_state_as_it_was(family, Q, S):
    c = R.case(family, Q, S, 8)
    assert c["dead_rows"]
    steps, on_live, tiles = _online_softmax_over_masked_steps(c, Q, S)
    print("%s Q %d S %d: %d fully masked (query, step) pairs, %d of them behind a live key, %d whole 16 x 16 tiles"
          % (family, Q, S, steps, on_live, tiles))
    assert steps > 0
    if family == "window_masks":
        assert on_live > 0 and tiles > 0


def test_reference_meets_the_conditions_of_the_gpu_tests():
    """Every case test_attention_eval_gpu.py runs: finite operands and a finite reference, every row with an attendable key or
    a declared dead row, the case cached; and the evaluation geometries are those no training test reaches."""
    import test_attention_eval_gpu as G
    assert len(G.IDENTITY_GROUPS) == 2 * len(R.FAMILIES) and G.EVAL_SELF_Q == 600 > 512
    assert sorted(set((Q, S) for _, Q, S, _ in G.EVAL_CROSS)) == [(100, 374), (300, 4096), (300, 5655)] and 5655 == 88 * 64 + 23
    assert sorted(set(f for f, _, _, _ in G.EVAL_CROSS)) == ["noise", "underflow", "window_masks"]
    cases = list(G.EVAL_CROSS) + [(f, Q, S, h) for f, h in G.IDENTITY_GROUPS for Q in R.QS for S in R.SS]
    for family, Q, S, heads in cases:
        c = R.case(family, Q, S, heads)
        assert c is R.case(family, Q, S, heads)
        assert all(bool(torch.isfinite(t).all()) for t in c["ops"]) and bool(torch.isfinite(c["out"]).all())
        m = R.effective_mask(c["mask"], c["row_open"], R.N, Q, S)
        dead = set(c["dead_rows"])
        assert dead == (set() if m is None else {(int(n), int(q)) for n, q in m.all(-1).reshape(R.N, Q).nonzero().tolist()})
        for n, q in dead:
            assert float(c["out"][q, n].abs().max()) == 0.0
    for family, Q, heads in list(SR.CASES) + [(f, G.EVAL_SELF_Q, 8) for f in G.EVAL_SELF_FAMILIES]:
        c = SR.case(family, Q, heads)
        assert all(bool(torch.isfinite(t).all()) for t in c["ops"]) and bool(torch.isfinite(c["out"]).all())

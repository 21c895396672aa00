"""CPU: the ragged cross-attention entry's header, ctypes table and exports agree; its switch keeps the rule of the others; the
layer attribute is checked; `supported` refuses what the kernel does not take and CPU tensors keep the torch chain; the entry's
argument errors come back as status codes in the ABI's order without a launch; and the inputs of tests/test_ragged_attention_gpu.py
hold what that file relies on."""
import ctypes
import os
import re

import pytest
import torch

import hard_inputs as hi
import ragged_attention_cases as cases

NAME = "pct_cross_attention_ragged_bf16"
BAD, ALIGN, UNSUP = -1, -3, -4


# ---------------------------------------------------------------- header, table, exports
def test_header_table_and_exports_agree():
    """Parameter by parameter: a pointer is c_void_p, `float` c_float, `int` c_int (a pointer bound as c_int reaches the entry
    truncated to 32 bits)."""
    from conftest import ROOT
    from pctrans_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pctrans_hip_xattn.h")).read()
    protos = dict(re.findall(r"PCT_API\s+int\s+(pct_\w+)\s*\(([^)]*)\)\s*;", hdr))
    assert sorted(protos) == sorted(_lib.XATTN_SYMBOLS) == [NAME]
    assert '#include "pctrans_hip_xattn.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()

    def ctype(param):
        if "*" in param:
            return ctypes.c_void_p
        return {"float": ctypes.c_float, "int": ctypes.c_int}[" ".join(param.split()[:-1])]

    argtypes, restype, checked_by = _lib.XATTN_SYMBOLS[NAME]
    params = [p.strip() for p in protos[NAME].split(",")]
    assert [ctype(p) for p in params] == argtypes and restype == ctypes.c_int
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "q_content", "q_pos", "k_content", "k_pos", "v", "mask", "mask_pitch", "row_open", "batch", "heads", "num_query",
        "num_key", "scale", "out", "stream"]
    assert checked_by == "tests/test_ragged_attention_gpu.py" and os.path.exists(os.path.join(ROOT, checked_by))
    fn = getattr(_lib.lib(), NAME)                                   # exported, and bound by lib()
    assert fn.argtypes == argtypes and fn.restype == restype


def test_makefile_lists_the_header():
    from conftest import ROOT
    assert "../../include/pctrans_hip_xattn.h" in open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------- the switch and the layer attribute
def test_switch_default_and_its_message(monkeypatch):
    from pctrans_amd import ragged_attention
    for value, want in ((None, "torch"), ("", "torch"), ("hip", "hip"), ("torch", "torch")):
        monkeypatch.delenv("PCT_XATTN_RAGGED", raising=False) if value is None else monkeypatch.setenv("PCT_XATTN_RAGGED", value)
        assert ragged_attention.default() == want
    monkeypatch.setenv("PCT_XATTN_RAGGED", "triton")
    with pytest.raises(RuntimeError, match=re.escape("PCT_XATTN_RAGGED must be 'hip' or 'torch', got 'triton'")):
        ragged_attention.default()


def _layer_and_inputs(Q=5, S=13, N=2, C=64, heads=4):
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    torch.manual_seed(0)
    layer = CrossAttentionLayer(C, heads).eval()
    kw = dict(tgt=torch.randn(Q, N, C), memory=torch.randn(S, N, C), pos=torch.randn(S, N, C), query_pos=torch.randn(Q, N, C),
              query_sine_embed=torch.randn(Q, N, 2 * C), is_first=True)
    return layer, kw


def test_layer_attribute_defaults_to_torch_is_no_state_and_rejects_other_values(monkeypatch):
    monkeypatch.delenv("PCT_XATTN_RAGGED", raising=False)
    layer, kw = _layer_and_inputs()
    assert layer.ragged_keys == "torch"
    assert not any("ragged" in k for k in layer.state_dict())
    layer.ragged_keys = "triton"
    with pytest.raises(ValueError, match=re.escape("CrossAttentionLayer.ragged_keys must be 'torch' or 'hip', got 'triton'")):
        layer(**kw)


def test_cpu_tensors_keep_the_torch_chain_with_the_switch_on(monkeypatch):
    from pctrans_amd import ragged_attention
    layer, kw = _layer_and_inputs()
    calls = []

    def entered(*a, **k):
        calls.append(a)
        raise AssertionError("the kernel path was entered on CPU tensors")

    monkeypatch.setattr(ragged_attention, "cross_attention", entered)
    real = layer.cross_attn.forward
    chain = []
    monkeypatch.setattr(layer.cross_attn, "forward", lambda *a, **k: chain.append(1) or real(*a, **k))
    with torch.no_grad():
        want = layer(**kw)
        layer.ragged_keys = "hip"
        got = layer(**kw)
    assert calls == [] and len(chain) == 2
    assert torch.equal(got, want)


def test_supported_refuses_cpu_fp32_six_heads_and_a_2d_mask():
    from pctrans_amd import ragged_attention
    L, S, N = 10, 33, 2
    q, _, k, _, v = cases.operands(L, S, N, 8, seed=0, device="cpu")
    assert not ragged_attention.supported(q, k, v, 8, None)                                   # CPU tensors
    assert not ragged_attention.supported(q.float(), k.float(), v.float(), 8, None)           # fp32
    q6, _, k6, _, v6 = cases.operands(L, S, N, 6, seed=0, device="cpu")
    assert not ragged_attention.supported(q6, k6, v6, 6, None)                                # 6 heads
    assert not ragged_attention.supported(q, k, v, 8, torch.zeros(L, S, dtype=torch.bool))    # [L, S] mask
    assert not ragged_attention.supported(q, k[:0], v[:0], 8, None)                           # no key


# ---------------------------------------------------------------- argument errors, host only
def test_argument_errors_are_status_codes_in_the_abi_order_without_a_launch():
    """Aligned host pointers that are never dereferenced (tests/test_abi.py does the same for the encoder's entries).  Every
    BAD_ARG condition wins over every ALIGNMENT condition, and ALIGNMENT over UNSUPPORTED."""
    from pctrans_amd import _lib
    fn = getattr(_lib.lib(), NAME)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0

    def call(ptrs=None, mask=p, pitch=48, row_open=None, N=2, heads=8, Q=10, S=33, out=p):
        qc, qp, kc, kp, v = ptrs or (p,) * 5
        return fn(qc, qp, kc, kp, v, mask, pitch, row_open, N, heads, Q, S, 32.0 ** -0.5, out, None)

    bad_args = [dict(S=0), dict(S=-5), dict(heads=0), dict(heads=-4), dict(N=-1), dict(Q=-1), dict(pitch=32), dict(pitch=40),
                dict(pitch=-16), dict(ptrs=(None, p, p, p, p)), dict(ptrs=(p, p, p, p, None)), dict(out=None)]
    misaligned = [dict(ptrs=tuple(p + 8 * (i == j) for i in range(5))) for j in range(5)] + [dict(mask=p + 8), dict(out=p + 4)]
    unsupported = [dict(heads=6), dict(heads=12 * 4 + 2), dict(N=1 << 20, S=1 << 12, pitch=1 << 12)]
    for kw in bad_args:
        assert call(**kw) == BAD, kw
    for kw in misaligned:
        assert call(**kw) == ALIGN, kw
    for kw in unsupported:
        assert call(**kw) == UNSUP, kw
    for b in bad_args:
        for m in misaligned + unsupported:
            if not (set(b) & set(m)):
                assert call(**b, **m) == BAD, (b, m)
    for m in misaligned:
        for u in unsupported:
            assert call(**m, **u) == ALIGN, (m, u)
    # the mask's pitch is ignored without a mask; an out on 8 bytes is enough; empty calls return 0 before any pointer is looked at
    assert call(mask=None, pitch=0, N=0) == 0 and call(mask=None, pitch=-3, Q=0) == 0
    assert call(ptrs=(None,) * 5, out=None, N=0) == 0 and call(ptrs=(p + 2,) * 5, Q=0) == 0
    assert call(N=0, S=0) == BAD and call(Q=0, pitch=32) == BAD and call(N=0, heads=0) == BAD


# ---------------------------------------------------------------- the GPU file's inputs hold what it relies on
@pytest.mark.parametrize("S", cases.KEYS + cases.ALIGNED_KEYS)
def test_bit_identity_masks_hold_the_four_rows(S):
    for L in cases.QUERIES:
        for N in cases.BATCHES:
            m = cases.bit_mask(L, S, N, seed=S + L)[:, 0]
            live = ~m
            assert live[0, 1].nonzero().flatten().tolist() == [S - 1]               # only key S - 1
            assert live[0, 2].nonzero().flatten().tolist() == [0]                   # only key 0
            first = cases.last_step_start(S)
            assert 0 <= first < S <= first + 32 and first % 32 == 0
            assert not live[0, 3, :first].any() and live[0, 3, first:].all()        # only the last 32-key step
            dead = m.all(-1)
            assert dead.nonzero().tolist() == [[N - 1, L - 1]]                      # one fully masked row


def test_hard_geometries_are_the_issues():
    assert sorted(g[1] for g in cases.HARD_GEOMETRIES) == [22, 50, 97, 374]
    assert all(g[4] == 32 and g[3] % 4 == 0 for g in cases.HARD_GEOMETRIES)
    assert all(g[1] % 64 for g in cases.HARD_GEOMETRIES)                           # none reaches the 64-key kernel
    own = list(hi.ATTN_GEOMETRIES)
    cases.hard_case("peaked", (16, 22, 1, 4, 32))
    assert hi.ATTN_GEOMETRIES == own                                               # the builder's table is as it was


@pytest.mark.parametrize("geometry", cases.HARD_GEOMETRIES, ids=lambda g: "L%d-S%d-N%d-h%d-d%d" % g)
def test_hard_cases_hold_the_builders_own_claims(geometry):
    L, S, N, heads, hd = geometry
    # one_hot: the planted keys of _one_hot_keys are there, and every query's other keys weigh less than 2^-12 in float64
    c = cases.hard_case("one_hot", geometry)
    hot = torch.from_numpy(c["hot"])
    planted = [p for p in (0, 31, 32, S - 33, S - 1, 32 * (S // 32), 32 * (S // 32) + (S % 32) // 2) if 0 <= p < S]
    assert set(planted) <= set(hot.flatten().tolist()) and S - 1 in planted
    assert set(range(min(S, 32))) <= set((hot % 32).flatten().tolist()) or hot.numel() < 39      # every residue, where the queries allow
    rest = 1.0 - c["p"].gather(-1, hot[..., None])[..., 0]
    assert bool((rest < 2.0 ** -12).all())
    assert tuple(c["q"].shape) == (L, N, heads * hd) and tuple(c["v"].shape) == (S, N, heads * 16)
    # window_masks: the fully masked rows the GPU test expects NaN on exist, are NaN in float64, and no other row is;
    # some window lies wholly inside the ragged tail
    c = cases.hard_case("window_masks", geometry)
    mask = c["mask"][:, 0]
    assert len(c["dead_rows"]) >= 2
    for n, l in c["dead_rows"]:
        assert bool(mask[n, l].all()) and bool(torch.isnan(c["want"][l, n]).all())
    assert int(mask.all(-1).sum()) == len(c["dead_rows"]) == int(torch.isnan(c["want"]).all(-1).sum())
    tail = 32 * (S // 32) if S % 32 else max(0, S - 32)
    win = torch.from_numpy(c["windows"])
    assert bool(((win[..., 0] >= tail) & (win[..., 1] > win[..., 0])).any())
    # every family: a finite float64 reference off the dead rows, and a positive bound
    for family in hi.ATTN_FAMILIES:
        c = cases.hard_case(family, geometry)
        live = ~torch.isnan(c["want"])
        assert bool(torch.isfinite(c["want"][live]).all()) and bool((c["A"][live] > 0).all())
        if family != "window_masks":
            assert bool(live.all())

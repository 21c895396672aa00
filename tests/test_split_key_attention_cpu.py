"""CPU: the split-key cross-attention entries' header, ctypes table and exports agree; the switch keeps the rule of the others;
the layer attribute is checked and CPU tensors keep the torch chain; `chunk_ranges` and `plan` hold their rules; the entry's
argument errors come back as status codes in the documented order without a launch; the masks of
tests/test_split_key_attention_gpu.py hold what that file relies on; and a float64 restatement of partials + combine equals plain
softmax attention, while three wrong combines leave the GPU test's bound by far."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hard_inputs as hi
import ragged_attention_cases as rcases
import split_key_attention_cases as cases

WORKSPACE, ENTRY = "pct_cross_attention_split_keys_workspace", "pct_cross_attention_split_keys_bf16"
BAD, ALIGN, UNSUP = -1, -3, -4
EPS = 2.0 ** -9


# ---------------------------------------------------------------- header, table, exports
def test_header_table_and_exports_agree():
    """Parameter by parameter: a pointer is c_void_p, `float` c_float, `int` c_int, `long long` c_longlong."""
    from conftest import ROOT
    from pctrans_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pctrans_hip_xattn_split.h")).read()
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"PCT_API\s+(int|long long)\s+(pct_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert sorted(protos) == sorted(_lib.XATTN_SPLIT_SYMBOLS) == sorted([WORKSPACE, ENTRY])
    assert '#include "pctrans_hip_xattn_split.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    assert not set(_lib.XATTN_SPLIT_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.XATTN_SYMBOLS))

    def ctype(param):
        if "*" in param:
            return ctypes.c_void_p
        return {"float": ctypes.c_float, "int": ctypes.c_int, "long long": ctypes.c_longlong}[" ".join(param.split()[:-1])]

    names = {}
    for name, (ret, params) in protos.items():
        argtypes, restype, checked_by = _lib.XATTN_SPLIT_SYMBOLS[name]
        params = [p.strip() for p in params.split(",")]
        assert [ctype(p) for p in params] == argtypes, name
        assert restype == {"int": ctypes.c_int, "long long": ctypes.c_longlong}[ret], name
        assert checked_by == "tests/test_split_key_attention_gpu.py" and os.path.exists(os.path.join(ROOT, checked_by))
        fn = getattr(_lib.lib(), name)                                # exported, and bound by lib()
        assert fn.argtypes == argtypes and fn.restype == restype
        names[name] = [p.split()[-1].lstrip("*") for p in params]
    assert names[WORKSPACE] == ["batch", "heads", "num_query", "splits"]
    # the ragged entry's operands in its order, then splits, workspace, workspace_bytes, then out, stream
    assert names[ENTRY] == ["q_content", "q_pos", "k_content", "k_pos", "v", "mask", "mask_pitch", "row_open", "batch", "heads",
                            "num_query", "num_key", "scale", "splits", "workspace", "workspace_bytes", "out", "stream"]


def test_makefile_lists_the_header():
    from conftest import ROOT
    assert "../../include/pctrans_hip_xattn_split.h" in open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------- the switch and the layer attribute
def test_switch_default_and_its_message(monkeypatch):
    from pctrans_amd import split_key_attention
    for value, want in ((None, "torch"), ("", "torch"), ("hip", "hip"), ("torch", "torch")):
        monkeypatch.delenv("PCT_XATTN_SPLIT_KEYS", raising=False) if value is None \
            else monkeypatch.setenv("PCT_XATTN_SPLIT_KEYS", value)
        assert split_key_attention.default() == want
    monkeypatch.setenv("PCT_XATTN_SPLIT_KEYS", "triton")
    with pytest.raises(RuntimeError, match=re.escape("PCT_XATTN_SPLIT_KEYS must be 'hip' or 'torch', got 'triton'")):
        split_key_attention.default()


def _layer_and_inputs(Q=5, S=13, N=2, C=64, heads=4):
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    torch.manual_seed(0)
    layer = CrossAttentionLayer(C, heads).eval()
    kw = dict(tgt=torch.randn(Q, N, C), memory=torch.randn(S, N, C), pos=torch.randn(S, N, C), query_pos=torch.randn(Q, N, C),
              query_sine_embed=torch.randn(Q, N, 2 * C), is_first=True)
    return layer, kw


def test_layer_attribute_defaults_to_torch_is_no_state_and_rejects_other_values(monkeypatch):
    monkeypatch.delenv("PCT_XATTN_SPLIT_KEYS", raising=False)
    layer, kw = _layer_and_inputs()
    assert layer.split_keys == "torch"
    assert not any("split" in k for k in layer.state_dict())
    layer.split_keys = "triton"
    with pytest.raises(ValueError, match=re.escape("CrossAttentionLayer.split_keys must be 'torch' or 'hip', got 'triton'")):
        layer(**kw)


def test_cpu_tensors_keep_the_torch_chain_with_the_switch_on(monkeypatch):
    from pctrans_amd import split_key_attention
    layer, kw = _layer_and_inputs(S=300)
    monkeypatch.setattr(split_key_attention, "MIN_CHUNKS", 1)
    monkeypatch.setattr(split_key_attention, "MIN_KEYS", 1)
    assert split_key_attention.plan(5, 2, 4, 300) >= 2              # the plan would route this shape
    calls = []

    def entered(*a, **k):
        calls.append(a)
        raise AssertionError("the kernel path was entered on CPU tensors")

    monkeypatch.setattr(split_key_attention, "cross_attention", entered)
    real = layer.cross_attn.forward
    chain = []
    monkeypatch.setattr(layer.cross_attn, "forward", lambda *a, **k: chain.append(1) or real(*a, **k))
    with torch.no_grad():
        want = layer(**kw)
        layer.split_keys = "hip"
        got = layer(**kw)
    assert calls == [] and len(chain) == 2
    assert torch.equal(got, want)


def test_supported_refuses_what_the_ragged_kernel_refuses():
    from pctrans_amd import split_key_attention
    L, S, N = 10, 1024, 1
    q, _, k, _, v = rcases.operands(L, S, N, 8, seed=0, device="cpu")
    assert split_key_attention.plan(L, N, 8, S) >= 2
    assert not split_key_attention.covered(q, k, v, 8, None) and not split_key_attention.supported(q, k, v, 8, None)
    assert not split_key_attention.supported(q.float(), k.float(), v.float(), 8, None)


# ---------------------------------------------------------------- chunk_ranges and plan
@pytest.mark.parametrize("S", cases.KEYS + tuple(g[1] for g in cases.HARD_GEOMETRIES) + (cases.LAYER_SHAPE["S"], 1024, 4096, 5655))
def test_chunk_ranges_partition_the_chunks(S):
    from pctrans_amd import split_key_attention
    nch = split_key_attention.chunks(S)
    assert nch == cases.chunks(S) == -(-S // 64)
    for splits in range(1, min(16, nch) + 1):
        r = split_key_attention.chunk_ranges(S, splits)
        assert len(r) == splits and r[0][0] == 0 and r[-1][1] == nch
        assert all(c0 < c1 for c0, c1 in r)                                        # non-empty
        assert all(a[1] == b[0] for a, b in zip(r, r[1:]))                         # ascending, no gap, no overlap
        assert r == [(j * nch // splits, (j + 1) * nch // splits) for j in range(splits)]
        assert max(c1 - c0 for c0, c1 in r) - min(c1 - c0 for c0, c1 in r) <= 1    # balanced
        k = cases.key_ranges(S, splits)
        assert k[0][0] == 0 and k[-1][1] == S and all(lo < hi for lo, hi in k)
    assert set(cases.split_counts(S)) <= set(range(2, nch + 1))


def test_the_c_rule_is_the_python_rule():
    """One statement of the rule in C, and it reads as chunk_ranges does."""
    from conftest import ROOT
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "cross_attention.hip")).read()
    assert len(re.findall(r"\(long long\)j \* nch / splits", src)) == 1
    assert len(re.findall(r"int xa_split_begin\(", src)) == 1


def test_plan_follows_its_rule_and_never_exceeds_the_entrys_limits(monkeypatch):
    from pctrans_amd import ragged_attention, split_key_attention as sk
    assert (sk.MAX_SPLITS, sk.CHUNK) == (16, 64) and sk.MIN_CHUNKS >= 1 and sk.TARGET_WORKGROUPS >= 1 and sk.MIN_KEYS >= 1

    def rule(L, N, heads, S):
        nch = -(-S // 64)
        if S < sk.MIN_KEYS:                                      # the measured key-count floor: not routed
            return 1
        return min(sk.MAX_SPLITS, nch // sk.MIN_CHUNKS, -(-sk.TARGET_WORKGROUPS // ragged_attention.workgroups(L, N, heads)))

    shapes = [(L, N, 8, S) for L in (10, 100, 300) for N in (1, 2, 8, 128) for S in (1, 63, 65, 221, 374, 1024, 1452, 4096, 5655, 65536)]
    for forced in (None, dict(MIN_CHUNKS=1, TARGET_WORKGROUPS=1 << 20, MIN_KEYS=1),
                   dict(MIN_CHUNKS=1, TARGET_WORKGROUPS=1 << 20, MIN_KEYS=1, MAX_SPLITS=64)):
        for name, value in (forced or {}).items():
            monkeypatch.setattr(sk, name, value)
        for L, N, heads, S in shapes:
            p = sk.plan(L, N, heads, S)
            assert 0 <= p <= min(16, -(-S // 64)), (L, N, S, p)
            if sk.MAX_SPLITS <= 16:
                assert p == rule(L, N, heads, S), (L, N, S)
            if forced is None and S < 1024:
                assert p < 2, (L, N, S)                          # shipped constants: below 1 024 keys today's route is faster
    assert sk.plan(37, 2, 8, 221) == 4 and sk.plan(20, 1, 8, 63) == 1 and sk.plan(20, 1, 8, 20) == 1   # forced: the layer tests


# ---------------------------------------------------------------- argument errors, host only
def test_workspace_bytes_and_its_refusals():
    from pctrans_amd import _lib
    fn = getattr(_lib.lib(), WORKSPACE)
    assert fn(2, 8, 37, 4) == 4 * 2 * 8 * 37 * 18 * 4
    assert fn(2, 8, 37, 1) == 0 and fn(0, 8, 37, 4) == 0 and fn(2, 8, 0, 4) == 0
    assert fn(1 << 20, 1 << 10, 1 << 10, 16) == 16 * (1 << 40) * 72                # no 32-bit product on the way
    for kw in (dict(batch=-1), dict(heads=0), dict(heads=-4), dict(num_query=-1), dict(splits=0), dict(splits=17), dict(splits=-2)):
        a = dict(batch=2, heads=8, num_query=37, splits=4)
        a.update(kw)
        assert fn(a["batch"], a["heads"], a["num_query"], a["splits"]) == BAD, kw
    assert fn(2, 6, 37, 4) == UNSUP and fn(2, 6, 37, 0) == BAD


def test_argument_errors_are_status_codes_in_the_documented_order_without_a_launch():
    """Aligned host pointers that are never dereferenced.  The ragged entry's answers come first, in its order (BAD_ARG, the
    empty call, a null operand, ALIGNMENT, UNSUPPORTED); then BAD_ARG for `splits` and the workspace's presence and size; then
    ALIGNMENT for the workspace."""
    from pctrans_amd import _lib
    fn = getattr(_lib.lib(), ENTRY)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    N, heads, Q, S = 2, 8, 10, 200                                                # 4 chunks
    need = getattr(_lib.lib(), WORKSPACE)(N, heads, Q, 4)

    def call(ptrs=None, mask=p, pitch=208, row_open=None, N=N, heads=heads, Q=Q, S=S, splits=4, ws=p, ws_bytes=need, out=p):
        qc, qp, kc, kp, v = ptrs or (p,) * 5
        return fn(qc, qp, kc, kp, v, mask, pitch, row_open, N, heads, Q, S, 32.0 ** -0.5, splits, ws, ws_bytes, out, None)

    ragged_bad = [dict(S=0), dict(heads=0), dict(N=-1), dict(Q=-1), dict(pitch=192), dict(pitch=204),
                  dict(ptrs=(None, p, p, p, p)), dict(out=None)]
    ragged_misaligned = [dict(ptrs=(p, p, p + 8, p, p)), dict(mask=p + 8), dict(out=p + 4)]
    ragged_unsupported = [dict(heads=6), dict(N=1 << 20, S=1 << 12, pitch=1 << 12)]
    split_bad = [dict(splits=0), dict(splits=-1), dict(splits=5), dict(splits=17), dict(ws=None), dict(ws_bytes=need - 1),
                 dict(ws_bytes=0), dict(ws_bytes=-8)]
    ws_misaligned = [dict(ws=p + 8), dict(ws=p + 4)]
    for group, code in ((ragged_bad, BAD), (ragged_misaligned, ALIGN), (ragged_unsupported, UNSUP), (split_bad, BAD),
                        (ws_misaligned, ALIGN)):
        for kw in group:
            assert call(**kw) == code, kw
    # the order: every earlier group wins over every later one
    ordered = [(ragged_bad, BAD), (ragged_misaligned, ALIGN), (ragged_unsupported, UNSUP), (split_bad, BAD), (ws_misaligned, ALIGN)]
    for i, (first, code) in enumerate(ordered):
        for later, _ in ordered[i + 1:]:
            for a in first:
                for b in later:
                    if not (set(a) & set(b)):
                        assert call(**a, **b) == code, (a, b)
    # the limit is min(16, chunks)  (no call here passes every check: that one would launch)
    assert call(S=1023, pitch=1024, splits=17, ws_bytes=1 << 30) == BAD
    assert call(S=960, pitch=960, splits=16, ws_bytes=1 << 30) == BAD              # 15 chunks
    # empty calls return 0 before `splits` or the workspace are looked at
    assert call(N=0, splits=0, ws=None, ws_bytes=0) == 0 and call(Q=0, splits=99, ws=p + 4) == 0
    assert call(N=0, S=0) == BAD


# ---------------------------------------------------------------- the GPU file's masks hold what it relies on
@pytest.mark.parametrize("S", cases.KEYS)
def test_exact_masks_hold_the_builders_claims(S):
    for splits in cases.split_counts(S):
        ranges = cases.key_ranges(S, splits)
        for L in cases.QUERIES:
            for N in cases.BATCHES:
                c = cases.exact_mask(L, S, N, splits, seed=S + L + splits)
                live, js = ~c["mask"][:, 0], c["live_split"]
                assert tuple(live.shape) == (N, L, S) and tuple(c["row_open"].shape) == (N, 1, L, 1)
                special = {c["opened"], c["dead"]}
                for n in range(N):
                    for l in range(L):
                        keys = live[n, l].nonzero().flatten().tolist()
                        if (n, l) in special:
                            assert keys == [] and int(js[n, l]) == -1
                            continue
                        lo, hi = ranges[int(js[n, l])]
                        assert keys and lo <= keys[0] and keys[-1] < hi, (n, l)      # inside one split's chunk range
                # every split is the live one for some row; its first and its last key are live in some row
                assert set(js[js >= 0].tolist()) == set(range(splits))
                for j, (lo, hi) in enumerate(ranges):
                    assert bool(live[:, :, lo].any()) and bool(live[:, :, hi - 1].any()), j
                n, l = c["key_s_minus_1"]
                assert live[n, l].nonzero().flatten().tolist() == [S - 1] and int(js[n, l]) == splits - 1
                n, l = c["key_0"]
                assert live[n, l].nonzero().flatten().tolist() == [0] and int(js[n, l]) == 0
                # one fully masked row, one fully masked row that row_open opens, and no other of either kind
                assert sorted((~live.any(-1)).nonzero().tolist()) == sorted([list(c["opened"]), list(c["dead"])])
                assert c["row_open"][:, 0, :, 0].nonzero().tolist() == [list(c["opened"])]


def test_hard_geometries_are_the_issues():
    assert cases.HARD_GEOMETRIES == [(37, 200, 2, 8, 32), (100, 374, 2, 8, 32), (16, 129, 1, 4, 32)]
    assert [cases.split_counts(g[1]) for g in cases.HARD_GEOMETRIES] == [[2, 3, 4], [2, 3, 4, 5, 6], [2, 3]]
    assert [cases.split_counts(S) for S in cases.KEYS] == [[2], [2, 3], [2, 3, 4], [2, 3, 4], [2, 3, 4], [2, 3, 4, 5, 6]]


# ---------------------------------------------------------------- partials + combine, restated in float64
def _restated(c, splits, **variant):
    """The case's output [L, N, heads*16] from partials_f64 + combine_f64 on its float64 scores."""
    L, S, N, heads, _ = c["geometry"]
    ranges = cases.key_ranges(S, splits)
    scores = c["scores"].numpy()
    v = c["v"].double().numpy().reshape(S, N, heads, 16)
    out = np.empty((L, N, heads, 16))
    for n in range(N):
        for h in range(heads):
            out[:, n, h] = cases.combine_f64(*cases.partials_f64(scores[n, h], v[:, n, h], ranges), **variant)
    return torch.from_numpy(out.reshape(L, N, heads * 16))


def _ratio(got, want, A):
    dead = torch.isnan(want)
    tol = 2.0 * (EPS * A + EPS * want.abs())
    return float(((got - want).abs()[~dead] / tol[~dead]).max())


@pytest.mark.parametrize("geometry", cases.HARD_GEOMETRIES, ids=lambda g: "L%d-S%d-N%d-h%d-d%d" % g)
def test_partials_and_combine_in_float64_are_plain_softmax_attention(geometry):
    S = geometry[1]
    for family in ("peaked", "window_masks", "underflow"):
        c = rcases.hard_case(family, geometry)
        want = c["want"]
        dead = torch.isnan(want)
        for splits in cases.split_counts(S):
            got = _restated(c, splits)
            assert torch.equal(torch.isnan(got), dead), (family, splits)             # NaN exactly on the fully masked rows
            assert float((got - want)[~dead].abs().max()) <= 1e-12, (family, splits)


@pytest.mark.parametrize("geometry", cases.HARD_GEOMETRIES, ids=lambda g: "L%d-S%d-N%d-h%d-d%d" % g)
def test_three_wrong_combines_leave_the_bound_by_far(geometry):
    """Without the exp(m_j - M) weights; every split normalised before the sum; the last split dropped (asserted where that
    split holds at least 32 keys: a last split of one or eight keys need not weigh enough in any of a small case's rows)."""
    S = geometry[1]
    c = rcases.hard_case("peaked", geometry)
    for splits in cases.split_counts(S):
        assert _ratio(_restated(c, splits), c["want"], c["A"]) < 1e-6
        lo, hi = cases.key_ranges(S, splits)[-1]
        for variant in (dict(weights=False), dict(normalise_first=True), dict(drop_last=True)):
            r = _ratio(_restated(c, splits, **variant), c["want"], c["A"])
            print(geometry, splits, variant, "worst |err| / bound %.3g" % r)
            if "drop_last" not in variant or hi - lo >= 32:
                assert r > 10.0, (splits, variant, r)

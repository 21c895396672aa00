"""CPU: the split-key differentiable cross-attention's header, ctypes table and exports agree; `chunk_ranges` and `plan` hold their
rules; the switch keeps the rule of the others; CPU tensors and autocast are refused; the layer checks its attribute; the window
case of tests/test_split_key_attention_train_gpu.py holds what that file relies on; and a float64 restatement of the split algebra
(split_key_attention_train_cases.split_algebra) equals the float64 reference on that file's cases, while three wrong combines
leave its bounds by far."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attention_train_reference as R
import split_key_attention_train_cases as K

NAMES = ("pct_cross_attention_split_train_workspace", "pct_cross_attention_split_forward_f32",
         "pct_cross_attention_split_backward_f32")


# ---------------------------------------------------------------- header, table, exports
def test_header_table_and_exports_agree():
    from conftest import ROOT
    from pctrans_amd import _lib
    top = open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    assert '#include "pctrans_hip_attn_train_split.h"' in top and "pct_cross_attention_split_forward_f32" not in top
    hdr = open(os.path.join(ROOT, "include", "pctrans_hip_attn_train_split.h")).read()
    protos = {name: (ret, params) for ret, name, params in re.findall(r"PCT_API\s+(int|long long)\s+(pct_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert sorted(protos) == sorted(_lib.ATTN_TRAIN_SPLIT_SYMBOLS) == sorted(NAMES)
    assert not set(_lib.ATTN_TRAIN_SPLIT_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.ATTN_TRAIN_SYMBOLS))

    def ctype(param):
        if "*" in param:
            return ctypes.c_void_p
        return {"float": ctypes.c_float, "int": ctypes.c_int, "long long": ctypes.c_longlong}[" ".join(param.split()[:-1])]

    names = {}
    for name, (ret, params) in protos.items():
        argtypes, restype, checked_by = _lib.ATTN_TRAIN_SPLIT_SYMBOLS[name]
        params = [p.strip() for p in params.split(",")]
        assert [ctype(p) for p in params] == argtypes, name
        assert restype == {"int": ctypes.c_int, "long long": ctypes.c_longlong}[ret], name
        assert checked_by == "tests/test_split_key_attention_train_gpu.py" and os.path.exists(os.path.join(ROOT, checked_by))
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == argtypes and fn.restype == restype
        names[name] = [p.split()[-1].lstrip("*") for p in params]
    # the unsplit entries' arguments with splits, workspace, workspace_bytes behind `scale`
    unsplit = open(os.path.join(ROOT, "include", "pctrans_hip_attn_train.h")).read()
    for split_name, name in ((NAMES[1], "pct_cross_attention_forward_f32"), (NAMES[2], "pct_cross_attention_backward_f32")):
        params = re.search(r"PCT_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, unsplit).group(1)
        want = [p.split()[-1].lstrip("*") for p in params.split(",")]
        at = want.index("scale") + 1
        if name.endswith("backward_f32"):
            assert want[at] == "workspace"
            want = want[:at] + want[at + 1:]
        assert names[split_name] == want[:at] + ["splits", "workspace", "workspace_bytes"] + want[at:], split_name
    makefile = open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()
    assert "cross_attention_train_split.hip" in makefile and "../../include/pctrans_hip_attn_train_split.h" in makefile


def test_workspace_bytes_and_argument_errors_without_a_launch():
    """Aligned host pointers that are never dereferenced; no call here passes every check (that one would launch)."""
    from pctrans_amd import _lib
    L = _lib.lib()
    BAD, ALIGN, UNSUP = -1, -3, -4
    ws_fn = L.pct_cross_attention_split_train_workspace
    rows = 2 * 8 * 37
    assert ws_fn(2, 8, 37, 4) == 8 * 4 * rows + 4 * rows + 128 * 4 * rows and ws_fn(2, 8, 37, 4) % 16 == 0
    assert ws_fn(1, 4, 1, 1) == 32 + 16 + 512                                        # 4 rows: D padded from 16 to 16 bytes ...
    assert ws_fn(1, 4, 3, 1) == 96 + 48 + 1536 and ws_fn(1, 4, 1, 2) == 64 + 16 + 1024
    assert ws_fn(0, 8, 37, 4) == 0 and ws_fn(2, 8, 0, 4) == 0
    assert ws_fn(65535, 8, 4096, 16) == 65535 * 8 * 4096 * (136 * 16 + 4)             # no 32-bit product on the way
    assert ws_fn(2, 8, 37, 16) >= 76 * 16 * rows                                      # the forward's part fits
    for args in ((-1, 8, 37, 4), (2, 0, 37, 4), (2, 8, -1, 4), (2, 8, 37, 0), (2, 8, 37, 17), (2, 6, 37, 0)):
        assert ws_fn(*args) == BAD, args
    assert ws_fn(2, 6, 37, 4) == UNSUP
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    need = ws_fn(2, 8, 10, 4)

    def fwd(N=2, heads=8, Q=10, S=200, splits=4, ws=p, ws_bytes=need, q_c=p):
        return L.pct_cross_attention_split_forward_f32(q_c, p, p, p, p, None, None, N, heads, Q, S, R.SCALE, splits, ws, ws_bytes, p,
                                                       p, None)

    def bwd(N=2, heads=8, Q=10, S=200, splits=4, ws=p, ws_bytes=need, go=p):
        return L.pct_cross_attention_split_backward_f32(p, p, p, p, p, None, None, None, p, go, N, heads, Q, S, R.SCALE, splits, ws,
                                                        ws_bytes, p, p, p, p, p, None)

    for call in (fwd, bwd):
        for kw in (dict(splits=0), dict(splits=-1), dict(splits=17), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                   dict(N=-1), dict(heads=0)):
            assert call(**kw) == BAD, (call.__name__, kw)
        for kw in (dict(ws=p + 8), dict(ws=p + 4)):
            assert call(**kw) == ALIGN, (call.__name__, kw)
        assert call(heads=5) == UNSUP and call(heads=5, splits=0) == UNSUP           # the unsplit entries' geometry first
        assert call(N=0, splits=0, ws=None) == 0 and call(Q=0) == 0 and call(S=0, ws_bytes=0) == 0     # empty: nothing is looked at
    assert fwd(q_c=None) == BAD and fwd(q_c=p + 4) == ALIGN and bwd(go=None) == BAD


# ---------------------------------------------------------------- chunk_ranges and plan
@pytest.mark.parametrize("S", (1, 63, 64, 65, 129, 196, 330, 784, 1024, 1025, 1040, 3136, 4096, 5655))
def test_chunk_ranges_partition_the_chunks(S):
    from pctrans_amd import split_key_attention_train as sk
    nch = sk.chunks(S)
    assert nch == -(-S // 64) == K.chunks(S) and sk.CHUNK == K.CHUNK == 64
    for splits in range(1, min(16, nch) + 1):
        r = sk.chunk_ranges(S, splits)
        assert len(r) == splits and r[0][0] == 0 and r[-1][1] == nch
        assert all(c0 < c1 for c0, c1 in r)                                        # non-empty
        assert all(a[1] == b[0] for a, b in zip(r, r[1:]))                         # ascending, no gap, no overlap
        assert K.key_ranges(S, splits) == [(c0 * 64, min(c1 * 64, S)) for c0, c1 in r]
    assert K.key_ranges(S, 16) == K.key_ranges(S, min(16, nch))                    # the entry's clamp


def test_the_c_rule_is_the_python_rule():
    from conftest import ROOT
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "cross_attention_train_split.hip")).read()
    assert len(re.findall(r"\{j \* nch / splits \* XS_CHUNK, min\(\(j \+ 1\) \* nch / splits \* XS_CHUNK, S\)\}", src)) == 1
    assert re.search(r"constexpr int XS_CHUNK = 16 \* AT_WAVES;", src) and re.search(r"constexpr int XS_MAX_SPLITS = 16;", src)


def test_plan_follows_its_rule_and_never_exceeds_the_entrys_limits(monkeypatch):
    from pctrans_amd import attention_train, split_key_attention_train as sk
    assert (sk.MAX_SPLITS, sk.CHUNK) == (16, 64) and sk.MIN_CHUNKS >= 1 and sk.TARGET_WORKGROUPS >= 1
    assert sk.MIN_KEYS >= attention_train.MAX_KEYS + 1                # only what the unsplit route leaves to torch

    def rule(Q, N, heads, S):
        nch = -(-S // 64)
        if S < sk.MIN_KEYS:
            return 1
        return max(0, min(sk.MAX_SPLITS, nch // sk.MIN_CHUNKS, -(-sk.TARGET_WORKGROUPS // (-(-Q // 16) * heads * N))))

    shapes = [(Q, N, h, S) for Q in (1, 17, 100, 300) for N in (1, 2, 4, 64) for h in (4, 8)
              for S in (1, 63, 65, 196, 784, 1024, 1025, 1040, 3136, 4096, 65536)]
    for forced in (None, dict(MIN_CHUNKS=1, TARGET_WORKGROUPS=1 << 20, MIN_KEYS=1),
                   dict(MIN_CHUNKS=1, TARGET_WORKGROUPS=1 << 20, MIN_KEYS=1, MAX_SPLITS=64)):
        for name, value in (forced or {}).items():
            monkeypatch.setattr(sk, name, value)
        for Q, N, h, S in shapes:
            p = sk.plan(Q, N, h, S)
            assert 0 <= p <= min(16, -(-S // 64)), (Q, N, S, p)
            if sk.MAX_SPLITS <= 16:
                assert p == rule(Q, N, h, S), (Q, N, S)
            if forced is None and S < sk.MIN_KEYS:
                assert p == 1, (Q, N, S)
    assert sk.plan(17, 2, 8, 1040) == 16 and sk.plan(17, 2, 8, 64) == 1              # forced: the layer test's shape


# ---------------------------------------------------------------- the switch, `supported`, the layer attribute
def test_switch_default_and_its_message(monkeypatch):
    from pctrans_amd import split_key_attention_train as sk
    for value, want in ((None, "torch"), ("", "torch"), ("hip", "hip"), ("torch", "torch")):
        monkeypatch.delenv("PCT_ATTN_TRAIN_SPLIT", raising=False) if value is None else monkeypatch.setenv("PCT_ATTN_TRAIN_SPLIT", value)
        assert sk.default() == want
    monkeypatch.setenv("PCT_ATTN_TRAIN_SPLIT", "triton")
    with pytest.raises(RuntimeError, match=re.escape("PCT_ATTN_TRAIN_SPLIT must be 'hip' or 'torch', got 'triton'")):
        sk.default()


def test_supported_is_false_for_cpu_tensors_and_under_autocast(monkeypatch):
    from pctrans_amd import attention_train, split_key_attention_train as sk
    monkeypatch.setattr(sk, "MIN_KEYS", 1)
    monkeypatch.setattr(sk, "MIN_CHUNKS", 1)
    monkeypatch.setattr(sk, "TARGET_WORKGROUPS", 1 << 20)
    ops = [torch.randn(T, 2, 128) for T in (5, 5, 300, 300, 300)]
    assert sk.plan(5, 2, 8, 300) >= 2
    assert not sk.covered(*ops, 8) and not sk.supported(*ops, 8)
    with pytest.raises(RuntimeError, match="outside what the kernels cover"):
        sk.cross_attention_train(*ops, 8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        sk.cross_attention_forward(*ops, 8, splits=2)
    # (device tensors under autocast: tests/test_split_key_attention_train_gpu.py; here the rule is the unsplit route's, by identity)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert not sk.supported(*ops, 8)
    seen = []
    monkeypatch.setattr(attention_train, "covered", lambda *a: seen.append(a) or False)
    assert not sk.covered(*ops, 8, None, None) and len(seen) == 1 and seen[0][:5] == tuple(ops)


def _layer_and_inputs(Q=5, S=300, N=2, C=64, heads=4):
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    torch.manual_seed(0)
    layer = CrossAttentionLayer(C, heads)
    kw = dict(tgt=torch.randn(Q, N, C), memory=torch.randn(S, N, C), pos=torch.randn(S, N, C), query_pos=torch.randn(Q, N, C),
              query_sine_embed=torch.randn(Q, N, 2 * C), is_first=True)
    return layer, kw


def test_layer_attribute_defaults_to_torch_is_no_state_and_rejects_other_values(monkeypatch):
    monkeypatch.delenv("PCT_ATTN_TRAIN_SPLIT", raising=False)
    layer, kw = _layer_and_inputs()
    assert layer.attn_train_split == "torch"
    assert not any("split" in k for k in layer.state_dict())
    layer.attn_train_split = "triton"
    with pytest.raises(ValueError, match=re.escape("CrossAttentionLayer.attn_train_split must be 'torch' or 'hip', got 'triton'")):
        layer(**kw)


def test_cpu_tensors_keep_the_torch_chain_with_the_switch_on(monkeypatch):
    from pctrans_amd import split_key_attention_train as sk
    layer, kw = _layer_and_inputs()
    monkeypatch.setattr(sk, "MIN_KEYS", 1)
    monkeypatch.setattr(sk, "MIN_CHUNKS", 1)
    monkeypatch.setattr(sk, "TARGET_WORKGROUPS", 1 << 20)
    assert sk.plan(5, 2, 4, 300) >= 2

    def entered(*a, **k):
        raise AssertionError("the kernel path was entered on CPU tensors")

    monkeypatch.setattr(sk, "cross_attention_train", entered)
    want = layer(**kw)
    layer.attn_train_split = "hip"
    got = layer(**kw)
    assert got.requires_grad and torch.equal(got, want)


# ---------------------------------------------------------------- the window case of property (b)
@pytest.mark.parametrize("heads", (8, 4))
def test_window_case_holds_what_the_gpu_test_relies_on(heads):
    from pctrans_amd import split_key_attention_train as sk
    Q, S, splits = K.WINDOW["Q"], K.WINDOW["S"], K.WINDOW["splits"]
    assert (Q, S, splits) == (17, 330, 3) and S % 64 != 0 and Q % 16 == 1
    ranges = [(c0 * 64, min(c1 * 64, S)) for c0, c1 in sk.chunk_ranges(S, splits)]
    assert ranges == [(0, 128), (128, 256), (256, 330)]
    c = K.window_case(heads)
    live, js = ~c["mask"][:, 0], c["live_split"]
    assert tuple(live.shape) == (R.N, Q, S) and c["row_open"] is None and c["dead_rows"] == []
    for n in range(R.N):
        for q in range(Q):
            keys = live[n, q].nonzero().flatten().tolist()
            lo, hi = ranges[int(js[n, q])]
            assert keys and lo <= keys[0] and keys[-1] < hi, (n, q)                # every live key inside one split's range
    assert set(js.flatten().tolist()) == set(range(splits))                        # every split is the live one for some query
    assert set(js[:, 16].tolist()) <= set(range(splits))                           # ... the lone query of the second tile included
    for lo, hi in ranges:                                                          # a range's first and last key are live somewhere
        assert bool(live[:, :, lo].any()) and bool(live[:, :, hi - 1].any())


# ---------------------------------------------------------------- the split algebra in float64
def _close(got, want):
    return float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def _algebra_cases():
    seen = set()
    for f, Q, S, heads, s in K.ACCURACY:
        if (f, Q, S, heads, K.used_splits(S, s)) not in seen:                       # 16 splits of 2 chunks are 2 splits
            seen.add((f, Q, S, heads, K.used_splits(S, s)))
            yield f, Q, S, heads, s


@pytest.mark.parametrize("family,Q,S,heads,splits", list(_algebra_cases()), ids=lambda v: str(v))
def test_split_algebra_in_float64_is_the_reference(family, Q, S, heads, splits):
    """Dead rows (noise, window_masks) and rows without a live key in some split (every masked family: the last split of
    (17, 129) is one key) included."""
    c = R.case(family, Q, S, heads)
    out, lse, grads = K.split_algebra(c, splits)
    assert _close(out, c["out"]) and _close(lse, c["lse"])
    for g, w in zip(grads, c["grads"]):
        assert _close(g, w)
    for n, q in c["dead_rows"]:
        assert float(out[q, n].abs().max()) == 0.0 and float(lse[n, :, q].abs().max()) == 0.0
    if c["mask"] is not None and (family == "window_masks" and K.used_splits(S, splits) >= 2 and Q >= 4 or (S, splits) == (129, 3)):
        m = K.split_maxima(c, splits)                                              # (129, 3): the last split is one key
        assert bool((np.isinf(m).any(0) & ~np.isinf(m).all(0)).any())              # a live row with an empty split


def test_split_algebra_on_the_window_and_big_cases():
    for c, splits in ((K.window_case(8), K.WINDOW["splits"]), (K.window_case(4), K.WINDOW["splits"]),
                      (R.case("noise_open", K.BIG[0], K.BIG[1], 8), 7)):
        out, lse, grads = K.split_algebra(c, splits)
        assert _close(out, c["out"]) and _close(lse, c["lse"]) and all(_close(g, w) for g, w in zip(grads, c["grads"]))


# the case of each family on which the wrong combines are judged: (Q, S, splits) of the GPU file's accuracy list.  Three splits of
# (100, 196) are 64 + 64 + 68 keys; the window masks leave few rows with live keys in three splits, so theirs has two
WRONG = {f: (100, 196, 2 if f == "window_masks" else 3) for f in R.FAMILIES}


@pytest.mark.parametrize("family", R.FAMILIES)
def test_three_wrong_combines_leave_the_bound_by_far(family):
    """The factor exp(m_j - M) dropped; lse from the last split's maximum; D from split 0 alone.  Each misses the GPU test's
    bound (the rule on `out` / the 2^-20 bound on lse / the rule on the gradients, the fp32 torch chain on this device as the
    yardstick) by more than 100 x.  From the reference alone: the case has live rows whose maximum lies outside split 0, with the
    splits' maxima at least 1 apart -- without them the first two would be right by accident."""
    Q, S, splits = WRONG[family]
    assert (family, Q, S, 8, splits) in K.ACCURACY
    c = R.case(family, Q, S, 8)
    m = K.split_maxima(c, splits)                                                  # [splits, N, heads, Q]
    assert m.shape[0] == splits >= 2
    live = np.isfinite(m)
    ranked = np.sort(np.where(live, m, -np.inf), axis=0)
    with np.errstate(invalid="ignore"):
        apart = (live.sum(0) >= 2) & (ranked[-1] - ranked[-2] >= 1.0)              # the two largest split maxima of the row
    outside_first, outside_last = apart & (m.argmax(0) != 0), apart & (m.argmax(0) != splits - 1)
    print(family, "rows with maxima 1 apart: %d, maximum outside split 0: %d, outside the last split: %d"
          % (apart.sum(), outside_first.sum(), outside_last.sum()))
    assert int(outside_first.sum()) >= 4 and int(outside_last.sum()) >= 4          # (the lse variant needs the second kind)
    yard = K.yardstick(c, (family, Q, S, 8), "cpu")
    right = K.split_algebra(c, splits)
    fig = K.rule(c, (right[0],) + right[2], yard)
    assert all(e <= b for e, b in fig.values()), fig
    assert float((right[1] - c["lse"]).abs().max()) <= K.lse_bound(c)

    out, lse, grads = K.split_algebra(c, splits, "no_factor")
    e, b = K.rule(c, (out,) + grads, yard)["out"]
    print(family, "no_factor: out error / bound %.3g" % (e / b))
    assert e > 100 * b, (e, b)

    out, lse, grads = K.split_algebra(c, splits, "lse_last_max")
    with np.errstate(invalid="ignore"):
        e = float(np.nanmax(np.where(np.isfinite(lse.numpy()), (lse - c["lse"]).abs().numpy(), np.inf)))
    print(family, "lse_last_max: lse error / bound %.3g" % (e / K.lse_bound(c)))
    assert e > 100 * K.lse_bound(c), e

    out, lse, grads = K.split_algebra(c, splits, "delta_split0")
    fig = K.rule(c, (out,) + grads, yard)
    worst = max(fig[n][0] / fig[n][1] for n in K.NAMES[1:])
    print(family, "delta_split0: worst gradient error / bound %.3g" % worst)
    assert fig["out"][0] <= fig["out"][1] and worst > 100, fig

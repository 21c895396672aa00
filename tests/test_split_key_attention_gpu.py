"""GPU: the split-operand cross-attention with the keys divided over several workgroups (csrc/cross_attention.hip PARTIAL + the
combine, C ABI pct_cross_attention_split_keys_bf16, pctrans_amd/split_key_attention.py):
  * BIT-IDENTICAL to the unsplit kernel on every row whose live keys lie inside one split's chunk range (the combine is exact
    there: weights 1 and 0, the dead splits' partial results are zeros), for every split count, tails in the last split only;
  * the hard operand families of tests/hard_inputs.py under the bound derived in tests/test_attention_hard_inputs_gpu.py;
  * splits = 1 is the ragged entry (and, on multiples of 64 keys, the aligned kernel);
  * nothing behind the last key, the mask rows' first S bytes, the output or the workspace is used, and nothing the workspace
    held before the call matters;
  * refused arguments give their status in the documented order and leave the output alone;
and at its call sites: one CrossAttentionLayer, and the whole head on an unpadded 104 x 136 image, eager and replayed from a graph."""
import pytest
import torch

import callsite_check as chk
import hard_inputs as hi
import ragged_attention_cases as rcases
import split_key_attention_cases as cases

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -9
BAD, ALIGN, UNSUP = -1, -3, -4


def _cat_heads(a, b, heads):
    T, N, C = a.shape
    return torch.cat([a.view(T, N, heads, 16), b.view(T, N, heads, 16)], dim=3).reshape(T, N, 2 * C)


def _split_heads(t, heads):
    """[T, N, heads*32] -> the content / positional halves [T, N, heads*16] whose per-head concatenation is t."""
    T, N, _ = t.shape
    t = t.reshape(T, N, heads, 32)
    return t[..., :16].reshape(T, N, heads * 16).contiguous(), t[..., 16:].reshape(T, N, heads * 16).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_same_bits(got, want, what=""):
    """NaN by position, every other element by its 16 bits."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (what, float((got.float() - want.float())[~nan].abs().max()))


def _worst_ratio(got, want, A):
    """max over the finite rows of |got - want| / (2 (2^-9 A + 2^-9 |want|)); NaN exactly on the fully masked rows."""
    dead = torch.isnan(want)
    assert torch.equal(torch.isnan(got), dead) and bool(torch.isfinite(got[~dead]).all())
    tol = 2.0 * (EPS * A + EPS * want.abs())
    err = (got.double() - want).abs()
    assert bool((tol[~dead] > 0).all())
    return float((err[~dead] / tol[~dead]).max())


def _f64(qc, qp, kc, kp, v, heads, mask):
    """hard_inputs.attention_f64 on the per-head concatenations of device operands -> (want, A) on the CPU."""
    want, A, _, _ = hi.attention_f64(_cat_heads(qc, qp, heads).cpu(), _cat_heads(kc, kp, heads).cpu(), v.cpu(),
                                     None if mask is None else mask.cpu(), heads)
    return want, A


# ---------------------------------------------------------------- 1. bits where the combine is exact
@pytest.mark.parametrize("S", cases.KEYS)
def test_rows_with_one_live_split_have_the_unsplit_kernels_bits(S):
    from pctrans_amd import ragged_attention, split_key_attention
    for splits in cases.split_counts(S):
        for L in cases.QUERIES:
            for heads in cases.HEADS:
                for N in cases.BATCHES:
                    what = "S=%d splits=%d L=%d heads=%d N=%d" % (S, splits, L, heads, N)
                    qc, qp, kc, kp, v = rcases.operands(L, S, N, heads, seed=L + S + splits)
                    c = cases.exact_mask(L, S, N, splits, seed=S + L + splits)
                    mask, row_open = c["mask"].cuda(), c["row_open"].cuda()
                    assert split_key_attention.covered(qc, kc, v, heads, mask), what
                    got = split_key_attention.cross_attention(qc, qp, kc, kp, v, heads, mask, row_open=row_open, splits=splits)
                    want = ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask, row_open=row_open)
                    assert got.shape == (L, N, heads * 16) and got.dtype == torch.bfloat16
                    # NaN in all 16 * heads channels of the masked row and nowhere else
                    dead = torch.zeros(L, N, dtype=torch.bool, device="cuda")
                    dead[c["dead"][1], c["dead"][0]] = True
                    nan = torch.isnan(got.float())
                    assert torch.equal(nan.all(-1), dead) and torch.equal(nan.any(-1), dead), what
                    one = (c["live_split"] >= 0).t().cuda()                              # [L, N]
                    assert int(one.sum()) == L * N - 2
                    assert torch.equal(_bits(got)[one], _bits(want)[one]), \
                        (what, float((got.float() - want.float())[one].abs().max()))
                    # a row whose only live key is S - 1 / 0 is that key's value row, exactly
                    for (n, l), key in ((c["key_s_minus_1"], S - 1), (c["key_0"], 0)):
                        assert torch.equal(_bits(got[l, n]), _bits(v[key, n])), (what, key)
                    # the opened row attends to every key of every split: the derived bound
                    n, l = c["opened"]
                    ops = [t[:, n:n + 1] for t in (qc[l:l + 1], qp[l:l + 1], kc, kp, v)]
                    w64, A = _f64(*ops, heads, None)
                    assert _worst_ratio(got[l:l + 1, n:n + 1].float().cpu(), w64, A) <= 1.0, what


@pytest.mark.parametrize("S", cases.KEYS)
def test_unmasked_calls_stay_inside_the_derived_bound(S):
    """Without a mask every split is live in every row: the combine's weights are all in play."""
    from pctrans_amd import ragged_attention, split_key_attention
    for L in cases.QUERIES:
        for heads in cases.HEADS:
            for N in cases.BATCHES:
                qc, qp, kc, kp, v = rcases.operands(L, S, N, heads, seed=L + S)
                want, A = _f64(qc, qp, kc, kp, v, heads, None)
                base = _worst_ratio(ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, None).float().cpu(), want, A)
                for splits in cases.split_counts(S):
                    got = split_key_attention.cross_attention(qc, qp, kc, kp, v, heads, None, splits=splits)
                    ratio = _worst_ratio(got.float().cpu(), want, A)
                    print("S=%d L=%d heads=%d N=%d splits=%d: worst |err| / bound %.3g (unsplit %.3g)"
                          % (S, L, heads, N, splits, ratio, base))
                    assert ratio <= 1.0, (S, L, heads, N, splits, ratio)


# ---------------------------------------------------------------- 2. hard inputs
@pytest.mark.parametrize("geometry", cases.HARD_GEOMETRIES, ids=lambda g: "L%d-S%d-N%d-h%d-d%d" % g)
@pytest.mark.parametrize("family", hi.ATTN_FAMILIES)
def test_hard_inputs_stay_inside_the_derived_bound(family, geometry):
    from pctrans_amd import ragged_attention, split_key_attention
    L, S, N, heads, hd = geometry
    c = rcases.hard_case(family, geometry)
    q, k, v = c["q"].cuda(), c["k"].cuda(), c["v"].cuda()
    mask = c["mask"].cuda() if c["mask"] is not None else None
    want, A = c["want"], c["A"]
    (qc, qp), (kc, kp) = _split_heads(q, heads), _split_heads(k, heads)
    assert split_key_attention.covered(qc, kc, v, heads, mask)
    base = _worst_ratio(ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask).float().cpu(), want, A)
    assert cases.split_counts(S) == list(range(2, min(6, cases.chunks(S)) + 1))
    for splits in cases.split_counts(S):
        out = split_key_attention.cross_attention(qc, qp, kc, kp, v, heads, mask, splits=splits)
        assert out.shape == (L, N, heads * 16) and out.dtype == torch.bfloat16
        ratio = _worst_ratio(out.float().cpu(), want, A)
        print("%s %s splits=%d: worst |err| / bound %.3g (unsplit kernel %.3g)" % (family, geometry, splits, ratio, base))
        assert ratio <= 1.0, (splits, ratio)
        if family == "window_masks":
            assert int(torch.isnan(out.float()).all(-1).sum()) == len(c["dead_rows"])
        if family == "one_hot":
            # out = bf16(v[p]) exactly wherever the float64 weight of all other keys is below 2^-12
            hot = torch.from_numpy(c["hot"])                                                # [N, heads, L]
            rest = 1.0 - c["p"].gather(-1, hot[..., None])[..., 0]
            sure = (rest < 2.0 ** -12).permute(2, 0, 1)                                     # [L, N, heads]
            assert bool(sure.all())
            vh = c["v"].reshape(S, N, heads, 16).permute(1, 2, 0, 3)                        # [N, heads, S, 16]
            picked = vh.gather(2, hot[..., None].expand(-1, -1, -1, 16)).permute(2, 0, 1, 3)   # [L, N, heads, 16]
            got = out.cpu().reshape(L, N, heads, 16)
            assert torch.equal(got[sure].view(torch.int16), picked[sure].view(torch.int16)), splits


# ---------------------------------------------------------------- 3. splits = 1
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("S", [33, 129, 192])
def test_one_split_is_the_existing_kernel(S, masked):
    from pctrans_amd import fused_ops, ragged_attention, split_key_attention
    for L, N, heads in ((37, 3, 8), (65, 1, 4)):
        qc, qp, kc, kp, v = rcases.operands(L, S, N, heads, seed=L + S)
        mask = rcases.bit_mask(L, S, N, seed=S + L, device="cuda") if masked else None
        got = split_key_attention.cross_attention(qc, qp, kc, kp, v, heads, mask, splits=1)     # no workspace at all
        _assert_same_bits(got, ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask), "ragged entry")
        if S % 64 == 0:
            _assert_same_bits(got, fused_ops.cross_attention(qc, qp, kc, kp, v, heads, mask), "aligned kernel")


# ---------------------------------------------------------------- 4. nothing outside is used
def _entry(qc, qp, kc, kp, v, mask, pitch, row_open, N, heads, L, S, splits, ws, ws_bytes, out, check=True):
    from pctrans_amd import _lib
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = _lib.lib().pct_cross_attention_split_keys_bf16(
        ptr(qc), ptr(qp), ptr(kc), ptr(kp), ptr(v), ptr(mask), pitch, ptr(row_open), N, heads, L, S, 32.0 ** -0.5, splits,
        ws if isinstance(ws, int) or ws is None else ws.data_ptr(), ws_bytes, ptr(out), torch.cuda.current_stream().cuda_stream)
    if check:
        _lib.check(rc, "cross_attention_split_keys")
    return rc


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("S,splits", [(65, 2), (129, 3), (200, 4), (256, 3), (374, 6)])
def test_nothing_behind_the_last_key_the_mask_row_the_output_or_the_workspace_is_used(S, splits, masked):
    """Every byte the call could wrongly touch is allocated: the operands are the first S rows of buffers of S + 64 rows whose
    other rows hold 3e38; the mask rows sit in a buffer of pitch 16 ceil(S / 16) + 64 whose bytes from S on say "may attend";
    the output is the first L rows of a buffer filled with a sentinel; the workspace is the first `need` bytes of a buffer
    filled with NaN, with a sentinel behind them."""
    from pctrans_amd import split_key_attention
    L, N, heads = 37, 2, 8
    C = heads * 16
    qc, qp, kc, kp, v = rcases.operands(L, S, N, heads, seed=11 + S)

    def behind(t):
        buf = torch.full((S + 64, N, C), 3e38, dtype=torch.bfloat16, device="cuda")
        buf[:S] = t
        return buf

    bkc, bkp, bv = behind(kc), behind(kp), behind(v)
    mask = pm = row_open = None
    pitch = 16 * ((S + 15) // 16) + 64
    if masked:
        mask = rcases.bit_mask(L, S, N, seed=S, device="cuda")
        pm = torch.zeros(N, L, pitch, dtype=torch.bool, device="cuda")
        pm[:, :, :S] = mask[:, 0]
        row_open = torch.zeros(N, L, dtype=torch.bool, device="cuda")
        row_open[0, 5] = True
    need = split_key_attention.workspace_bytes(N, heads, L, splits)
    assert need == splits * N * heads * L * 18 * 4
    sentinel, guard = -1.75, 12345.0
    outs = []
    for fill in (float("nan"), float("inf"), -3e38):
        ws = torch.full((need // 4 + 64,), fill, dtype=torch.float32, device="cuda")
        ws[need // 4:] = guard
        out = torch.full((L + 8, N, C), sentinel, dtype=torch.bfloat16, device="cuda")
        _entry(qc, qp, bkc[:S], bkp[:S], bv[:S], pm, pitch, row_open, N, heads, L, S, splits, ws, need, out)
        assert bool((out[L:] == sentinel).all()) and bool((ws[need // 4:] == guard).all())
        outs.append(out[:L])
    want = split_key_attention.cross_attention(qc.clone(), qp.clone(), kc.clone(), kp.clone(), v.clone(), heads, mask,
                                               row_open=row_open, splits=splits)
    for out in outs:                               # a clean run's bits, whatever the workspace held before
        _assert_same_bits(out, want)
    live = ~torch.isnan(want)
    assert bool(torch.isfinite(want[live].float()).all()) and int((~live).all(-1).sum()) == (1 if masked else 0)


# ---------------------------------------------------------------- 5. status codes
def test_refused_arguments_give_their_status_in_order_and_leave_the_output_alone():
    from pctrans_amd import split_key_attention
    L, S, N, heads, splits = 10, 200, 2, 8, 4
    qc, qp, kc, kp, v = rcases.operands(L, S, N, heads, seed=1)
    mask = torch.zeros(N, L, 208, dtype=torch.bool, device="cuda")
    need = split_key_attention.workspace_bytes(N, heads, L, splits)
    ws = torch.zeros(need // 4 + 4, dtype=torch.float32, device="cuda")
    sentinel = -1.75
    out = torch.full((L, N, heads * 16), sentinel, dtype=torch.bfloat16, device="cuda")

    def call(mask=mask, pitch=208, heads=heads, S=S, splits=splits, ws=ws.data_ptr(), ws_bytes=need, kc=kc):
        rc = _entry(qc, qp, kc, kp, v, mask, pitch, None, N, heads, L, S, splits, ws, ws_bytes, out, check=False)
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())
        return rc

    odd = torch.zeros(S * N * heads * 16 + 8, dtype=torch.bfloat16, device="cuda")[4:4 + S * N * heads * 16]     # 8 bytes off
    ragged = [(dict(pitch=192), BAD), (dict(kc=None), BAD), (dict(kc=odd), ALIGN), (dict(heads=6), UNSUP)]
    split_bad = [dict(splits=0), dict(splits=5), dict(splits=17), dict(ws=None), dict(ws_bytes=need - 1)]
    for kw, code in ragged:
        assert call(**kw) == code, kw
        for b in split_bad + [dict(ws=ws.data_ptr() + 8)]:
            assert call(**kw, **b) == code, (kw, b)                       # the ragged entry's answer comes first
    for b in split_bad:
        assert call(**b) == BAD, b
        if "ws" not in b:
            assert call(ws=ws.data_ptr() + 8, **b) == BAD, b              # BAD_ARG before the workspace's alignment
    assert call(ws=ws.data_ptr() + 8) == ALIGN and call(ws=ws.data_ptr() + 4) == ALIGN
    assert split_key_attention.workspace_bytes(N, heads, L, 1) == 0
    with pytest.raises(RuntimeError):
        split_key_attention.workspace_bytes(N, heads, L, 17)
    with pytest.raises(RuntimeError):
        split_key_attention.cross_attention(qc, qp, kc, kp, v, heads, None, splits=5)
    # and the accepted call writes
    assert _entry(qc, qp, kc, kp, v, mask, 208, None, N, heads, L, S, splits, ws, need, out) == 0
    assert bool(torch.isfinite(out.float()).all()) and not bool((out == sentinel).all())


# ---------------------------------------------------------------- 6. and 7. the call sites
class _Recorder:
    """Keeps the calls of split_key_attention.cross_attention and of ragged_attention.cross_attention, counts
    fused_ops.masked_attention by its key count and the layer's V^T products (torch.baddbmm on a token-major operand)."""

    def __init__(self, monkeypatch):
        from pctrans_amd import fused_ops, ragged_attention, split_key_attention
        self.split, self.ragged, self.generic_keys, self.vt = [], [], [], 0
        real_split, real_ragged = split_key_attention.cross_attention, ragged_attention.cross_attention
        real_generic, real_baddbmm = fused_ops.masked_attention, torch.baddbmm

        def keep(calls, out, qc, qp, kc, kp, v, heads, attn_mask, row_open, splits=None):
            calls.append(dict(ops=[t.clone() for t in (qc, qp, kc, kp, v)], heads=heads, splits=splits,
                              mask=None if attn_mask is None else attn_mask.clone(),
                              row_open=None if row_open is None else row_open.clone(), out=out.clone()))

        def split(qc, qp, kc, kp, v, heads, attn_mask=None, row_open=None, splits=None):
            used = splits if splits is not None else split_key_attention.plan(qc.shape[0], qc.shape[1], heads, kc.shape[0])
            out = real_split(qc, qp, kc, kp, v, heads, attn_mask, row_open=row_open, splits=splits)
            if not torch.cuda.is_current_stream_capturing():
                keep(self.split, out, qc, qp, kc, kp, v, heads, attn_mask, row_open, used)
            return out

        def ragged(qc, qp, kc, kp, v, heads, attn_mask=None, row_open=None):
            out = real_ragged(qc, qp, kc, kp, v, heads, attn_mask, row_open=row_open)
            if not torch.cuda.is_current_stream_capturing():
                keep(self.ragged, out, qc, qp, kc, kp, v, heads, attn_mask, row_open)
            return out

        def generic(q, k, v, heads, attn_mask=None, v_t=None):
            self.generic_keys.append(k.shape[0])
            return real_generic(q, k, v, heads, attn_mask, v_t=v_t)

        def baddbmm(*a, **kw):
            x = a[2]
            self.vt += int(x.dim() == 3 and x.shape[1] > 1 and x.stride(1) == 1 and x.stride(2) != 1)
            return real_baddbmm(*a, **kw)

        monkeypatch.setattr(split_key_attention, "cross_attention", split)
        monkeypatch.setattr(ragged_attention, "cross_attention", ragged)
        monkeypatch.setattr(fused_ops, "masked_attention", generic)
        monkeypatch.setattr(torch, "baddbmm", baddbmm)

    @staticmethod
    def check_bound(c):
        """A kept call against hard_inputs.attention_f64 on its own operands: the derived bound, NaN nowhere."""
        qc, qp, kc, kp, v = c["ops"]
        h, mask = c["heads"], c["mask"]
        if mask is not None and c["row_open"] is not None:
            mask = mask & ~c["row_open"].reshape(mask.shape[0], 1, mask.shape[2], 1)
        want, A = _f64(qc, qp, kc, kp, v, h, mask)
        assert bool(torch.isfinite(want).all())
        ratio = _worst_ratio(c["out"].float().cpu(), want, A)
        print("S=%d splits=%s: worst |err| / bound %.3g" % (kc.shape[0], c["splits"], ratio))
        assert ratio <= 1.0, (kc.shape[0], ratio)


def _force_plan(monkeypatch):
    from pctrans_amd import split_key_attention
    monkeypatch.setattr(split_key_attention, "MIN_CHUNKS", 1)
    monkeypatch.setattr(split_key_attention, "TARGET_WORKGROUPS", 1 << 20)
    monkeypatch.setattr(split_key_attention, "MIN_KEYS", 1)                 # (the measured key-count floor is above 221 keys)


def test_layer_takes_the_split_key_route_behind_its_switch(monkeypatch):
    from pctrans_amd import split_key_attention
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    Q, S, N, C, heads = (cases.LAYER_SHAPE[k] for k in ("Q", "S", "N", "C", "heads"))
    assert (Q, S, N) == (37, 221, 2)
    _force_plan(monkeypatch)
    assert split_key_attention.plan(Q, N, heads, S) == 4
    torch.manual_seed(0)
    layer = CrossAttentionLayer(C, heads).cuda().eval()
    assert layer.split_keys == "torch"
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    mask = torch.rand(N, 1, Q, S, device="cuda", generator=g) < 0.6
    mask[0, 0, 4, :] = True
    mask[N - 1, 0, Q - 1, :] = True
    kw = dict(tgt=rnd(Q, N, C), memory=rnd(S, N, C), memory_mask=mask, pos=rnd(S, N, C), query_pos=rnd(Q, N, C),
              query_sine_embed=rnd(Q, N, 2 * C), is_first=True, memory_row_open=mask.all(-1, keepdim=True))
    rec = _Recorder(monkeypatch)

    def run(switch, ragged="torch"):
        layer.split_keys, layer.ragged_keys = switch, ragged
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return layer(**kw)

    want = run("torch")
    assert (len(rec.split), len(rec.ragged), rec.generic_keys, rec.vt) == (0, 0, [S], 1)       # today's route
    got = run("hip")
    assert (len(rec.split), len(rec.ragged), rec.generic_keys, rec.vt) == (1, 0, [S], 1)       # entered once; no V^T product
    c = rec.split[0]
    assert c["row_open"] is not None and int(c["row_open"].sum()) == 2 and c["splits"] >= 2
    assert tuple(c["ops"][2].shape) == (S, N, C)
    rec.check_bound(c)
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert float((got.float() - want.float()).abs().max()) < 0.1          # the two routes form V with different GEMMs
    run("hip", ragged="hip")                                              # decided before the ragged route
    assert (len(rec.split), len(rec.ragged), rec.generic_keys, rec.vt) == (2, 0, [S], 1)
    run("torch", ragged="hip")                                            # "torch": every line as today, whatever ragged_keys says
    assert (len(rec.split), len(rec.ragged), rec.generic_keys, rec.vt) == (2, 1, [S], 1)


def test_whole_head_on_an_unpadded_image_splits_the_long_level_eager_and_replayed(monkeypatch):
    """ResNet-18 features of a 104 x 136 image (26 x 34, 13 x 17, 7 x 9, 4 x 5): the decoder's levels have 20, 63 and 221 keys.
    With the plan forced, the three 221-key layers (4 chunks) enter the new entry, the one-chunk layers go on entering the
    ragged one.  The same forward replayed from a graph gives the eager bits: the workspace allocation survives capture."""
    from pctrans_amd.graph import GraphedForward
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    H, W, Q = 104, 136, 20
    head, feats = chk.build_head(18, H, W, Q, 3, 1, None)
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = {k: torch.randn(1, f.shape[1], -(-H // s), -(-W // s), device="cuda", generator=g)
             for (k, f), s in zip(sorted(feats.items()), (4, 8, 16, 32))}
    layers = [m for m in head.modules() if isinstance(m, CrossAttentionLayer)]
    assert len(layers) == 9 and all(m.split_keys == "torch" and m.ragged_keys == "torch" for m in layers)
    for m in layers:
        m.split_keys = m.ragged_keys = "hip"
    _force_plan(monkeypatch)
    rec = _Recorder(monkeypatch)
    out = chk.forward(head, feats, "bf16")
    assert [c["ops"][2].shape[0] for c in rec.split] == [221] * 3 and all(c["splits"] == 4 for c in rec.split)
    assert [c["ops"][2].shape[0] for c in rec.ragged] == [20, 63] * 3
    assert len(rec.generic_keys) == 9 and set(rec.generic_keys) == {Q}             # the self-attentions alone
    assert rec.vt == 0
    assert all(c["mask"] is not None and c["row_open"] is not None for c in rec.split + rec.ragged)
    for c in rec.split + rec.ragged:
        rec.check_bound(c)
    assert torch.isfinite(out["pred_masks"].float()).all()
    fwd = GraphedForward(head, feats, autocast_dtype=torch.bfloat16)
    got, _ = fwd(feats)
    torch.cuda.synchronize()
    assert torch.equal(got["pred_masks"], out["pred_masks"])
    assert torch.equal(got["reference_points"], out["reference_points"])
    for a, b in zip(got["aux_outputs"], out["aux_outputs"]):
        assert torch.equal(a["pred_masks"], b["pred_masks"])

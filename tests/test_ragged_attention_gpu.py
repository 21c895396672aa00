"""GPU: the split-operand cross-attention for any key count (csrc/cross_attention.hip RAGGED, C ABI
pct_cross_attention_ragged_bf16, pctrans_amd/ragged_attention.py) against
  * pct_masked_attention_bf16 on the per-head concatenations: BIT-IDENTICAL outputs for key counts on both sides of every
    32-key step and 64-key chunk boundary, below one step, below one chunk, many chunks; rows whose only live key is the
    first / the last one, rows live only inside the last partial step, a fully masked row (NaN);
  * pct_cross_attention_bf16 where that covers the call;
  * row_open on a tail: an opened row attends to every real key and to nothing else;
  * poison behind the last key, behind the mask rows' first S bytes and behind the output, all in allocated memory;
  * the hard operand families of tests/hard_inputs.py under the bound derived in tests/test_attention_hard_inputs_gpu.py;
  * the float formulation at bf16 tolerance;
and at its call sites: one CrossAttentionLayer, and the whole head on an unpadded 104 x 136 image (221 / 63 / 20 keys)."""
import pytest
import torch

import callsite_check as chk
import hard_inputs as hi
import ragged_attention_cases as cases
from test_fused_ops_gpu import _attn_reference

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -9


def _cat_heads(a, b, heads):
    T, N, C = a.shape
    return torch.cat([a.view(T, N, heads, 16), b.view(T, N, heads, 16)], dim=3).reshape(T, N, 2 * C)


def _split_heads(t, heads):
    """[T, N, heads*32] -> the content / positional halves [T, N, heads*16] whose per-head concatenation is t."""
    T, N, _ = t.shape
    t = t.reshape(T, N, heads, 32)
    return t[..., :16].reshape(T, N, heads * 16).contiguous(), t[..., 16:].reshape(T, N, heads * 16).contiguous()


def _assert_same_bits(got, want, what=""):
    """NaN by position, every other element by its 16 bits."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]), \
        (what, float((got.float() - want.float())[~nan].abs().max()))


def _generic(qc, qp, kc, kp, v, heads, mask):
    """The oracle of tests/test_cross_attention_gpu.py: the generic kernel on the per-head concatenations."""
    from pctrans_amd import fused_ops
    return fused_ops.masked_attention(_cat_heads(qc, qp, heads), _cat_heads(kc, kp, heads), v, heads, mask)


# ---------------------------------------------------------------- 1. bit identity with the generic kernel
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("S", cases.KEYS)
def test_bit_identical_to_the_generic_kernel_on_concatenated_operands(S, masked):
    from pctrans_amd import ragged_attention
    for L in cases.QUERIES:
        for heads in cases.HEADS:
            for N in cases.BATCHES:
                what = "L=%d S=%d N=%d heads=%d" % (L, S, N, heads)
                qc, qp, kc, kp, v = cases.operands(L, S, N, heads, seed=L + S)
                mask = cases.bit_mask(L, S, N, seed=S + L, device="cuda") if masked else None
                assert ragged_attention.supported(qc, kc, v, heads, mask), what
                got = ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask)
                want = _generic(qc, qp, kc, kp, v, heads, mask)
                assert got.shape == (L, N, heads * 16) and got.dtype == torch.bfloat16
                dead = torch.zeros(L, N, dtype=torch.bool, device="cuda")
                if masked:
                    dead[L - 1, N - 1] = True                       # the fully masked row, and no other
                assert torch.equal(torch.isnan(got.float()).all(-1), dead) and torch.equal(torch.isnan(got.float()).any(-1), dead), what
                _assert_same_bits(got, want, what)
                if masked:
                    # the row whose only live key is S - 1 / 0 is that key's value row, exactly
                    hv = v.view(S, N, heads * 16)
                    assert torch.equal(got[1, 0].view(torch.int16), hv[S - 1, 0].view(torch.int16)), what
                    assert torch.equal(got[2, 0].view(torch.int16), hv[0, 0].view(torch.int16)), what


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("S", cases.ALIGNED_KEYS)
def test_multiples_of_64_keys_give_the_bits_of_both_existing_kernels(S, masked):
    from pctrans_amd import fused_ops, ragged_attention
    for L, N, heads in ((37, 3, 8), (65, 1, 12), (10, 1, 4)):
        qc, qp, kc, kp, v = cases.operands(L, S, N, heads, seed=L + S)
        mask = cases.bit_mask(L, S, N, seed=S + L, device="cuda") if masked else None
        got = ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask)
        _assert_same_bits(got, fused_ops.cross_attention(qc, qp, kc, kp, v, heads, mask), "split kernel")
        _assert_same_bits(got, _generic(qc, qp, kc, kp, v, heads, mask), "generic kernel")


def test_supported_on_the_device():
    from pctrans_amd import ragged_attention
    L, S, N, heads = 10, 33, 2, 8
    qc, qp, kc, kp, v = cases.operands(L, S, N, heads, seed=0)
    mask = torch.zeros(N, 1, L, S, dtype=torch.bool, device="cuda")
    assert ragged_attention.supported(qc, kc, v, heads, None) and ragged_attention.supported(qc, kc, v, heads, mask)
    assert not ragged_attention.supported(qc.float(), kc.float(), v.float(), heads, None)
    assert not ragged_attention.supported(qc, kc, v, heads, mask[0, 0])                         # [L, S]
    assert not ragged_attention.supported(qc, kc, v, heads, mask.to(torch.uint8))
    q6, _, k6, _, v6 = cases.operands(L, S, N, 6, seed=0)
    assert not ragged_attention.supported(q6, k6, v6, 6, None)
    # a contiguous view that starts 2 bytes off a 16-byte boundary: False, no exception
    flat = torch.zeros(S * N * heads * 16 + 1, dtype=torch.bfloat16, device="cuda")
    off = flat[1:].view(S, N, heads * 16)
    assert off.is_contiguous() and off.data_ptr() % 16 == 2
    assert not ragged_attention.supported(qc, off, v, heads, None) and not ragged_attention.supported(qc, kc, off, heads, None)


def test_supported_leaves_the_small_grids_at_middle_key_counts_to_the_generic_route():
    """The measured rule (profiles/ragged_attention.json): fewer than 80 workgroups and 485 .. 4 220 keys keep today's route,
    although the kernel covers them."""
    from pctrans_amd import ragged_attention
    assert [ragged_attention.workgroups(L, N, 8) for L, N in ((100, 2), (300, 2), (100, 8), (300, 8), (100, 128))] == [8, 20, 32, 80, 512]
    for L, N, S, want in ((100, 2, 1452, False), (300, 2, 1936, False), (100, 8, 1452, False), (100, 8, 485, False),
                          (100, 8, 4220, False), (100, 8, 484, True), (100, 8, 4221, True), (300, 8, 1452, True),
                          (100, 2, 5655, True), (100, 2, 374, True)):
        qc, _, kc, _, v = cases.operands(L, S, N, 8, seed=0)
        assert ragged_attention.covered(qc, kc, v, 8, None)
        assert ragged_attention.supported(qc, kc, v, 8, None) == want, (L, N, S)


# ---------------------------------------------------------------- 2. row_open with a tail
@pytest.mark.parametrize("L,S,N,heads", [(37, 33, 2, 8), (65, 97, 1, 4), (20, 22, 1, 8), (37, 374, 2, 8), (37, 65, 1, 12)])
def test_row_open_with_a_tail_equals_clearing_those_rows(L, S, N, heads):
    """Fully masked opened rows in the first and in the last (partial) query tile: finite, the unmasked call's rows, and the
    whole result the bits of the call on the mask with those rows cleared.  (A tail whose dead bytes were ANDed with the
    opened row's `keep` would let these rows attend to the zero rows behind key S - 1.)"""
    from pctrans_amd import ragged_attention
    qc, qp, kc, kp, v = cases.operands(L, S, N, heads, seed=7 + L + S)
    gm = torch.Generator(device="cuda").manual_seed(L * S)
    mask = torch.rand(N, 1, L, S, device="cuda", generator=gm) < 0.6
    mask[..., min(3, S - 1)] = False
    mask[0, 0, 4, :] = True
    mask[N - 1, 0, L - 1, :] = True
    row_open = mask.all(dim=-1, keepdim=True)
    row_open[0, 0, 9, 0] = True                                     # a partly masked row opened as well
    assert int(row_open.sum()) == 3
    got = ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask, row_open=row_open)
    want = ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask & ~row_open)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(got.view(torch.int16), _generic(qc, qp, kc, kp, v, heads, mask & ~row_open).view(torch.int16))
    free = ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, None)
    for n, l in ((0, 4), (N - 1, L - 1), (0, 9)):
        assert torch.equal(got[l, n].view(torch.int16), free[l, n].view(torch.int16)), (n, l)
    with pytest.raises(RuntimeError, match="bool"):
        ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask, row_open=row_open.to(torch.uint8))


# ---------------------------------------------------------------- 3. poison behind the tail, in bounds
def _entry(qc, qp, kc, kp, v, mask, pitch, row_open, N, heads, L, S, out):
    from pctrans_amd import _lib
    rc = _lib.lib().pct_cross_attention_ragged_bf16(
        qc.data_ptr(), qp.data_ptr(), kc.data_ptr(), kp.data_ptr(), v.data_ptr(), mask.data_ptr() if mask is not None else None,
        pitch, row_open.data_ptr() if row_open is not None else None, N, heads, L, S, 32.0 ** -0.5, out.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cross_attention_ragged")


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("S", [1, 33, 97, 374])
def test_nothing_behind_the_last_key_the_mask_row_or_the_output_is_used(S, masked):
    """Every byte the call could wrongly touch is allocated: the operands are the first S rows of buffers of S + 64 rows whose
    other rows hold NaN, +-inf and 3e38; the mask rows sit in a buffer of pitch 16 ceil(S / 16) + 64 whose bytes from S on say
    "may attend"; the output is the first L rows of a buffer filled with a sentinel."""
    from pctrans_amd import ragged_attention
    L, N, heads = 37, 2, 8
    C = heads * 16
    qc, qp, kc, kp, v = cases.operands(L, S, N, heads, seed=11 + S)
    poison = torch.tensor([float("nan"), float("inf"), float("-inf"), 3e38], device="cuda").bfloat16()

    def behind(t):
        buf = poison.repeat((S + 64) * N * C // 4).view(S + 64, N, C).clone()
        buf[:S] = t
        return buf

    bkc, bkp, bv = behind(kc), behind(kp), behind(v)
    mask = pm = None
    pitch = 16 * ((S + 15) // 16) + 64
    if masked:
        mask = cases.bit_mask(L, S, N, seed=S, device="cuda")
        pm = torch.zeros(N, L, pitch, dtype=torch.bool, device="cuda")
        pm[:, :, :S] = mask[:, 0]
    row_open = None
    if masked:
        row_open = torch.zeros(N, L, dtype=torch.bool, device="cuda")
        row_open[0, 5] = True
    sentinel = -1.75
    out = torch.full((L + 8, N, C), sentinel, dtype=torch.bfloat16, device="cuda")
    _entry(qc, qp, bkc[:S], bkp[:S], bv[:S], pm, pitch, row_open, N, heads, L, S, out)
    want = ragged_attention.cross_attention(qc.clone(), qp.clone(), kc.clone(), kp.clone(), v.clone(), heads, mask,
                                            row_open=row_open)
    _assert_same_bits(out[:L], want)
    assert bool((out[L:] == sentinel).all())
    live = ~torch.isnan(want)
    assert bool(torch.isfinite(out[:L][live].float()).all()) and int((~live).all(-1).sum()) == (1 if masked else 0)
    _assert_same_bits(want, _generic(qc, qp, kc, kp, v, heads, mask & ~row_open[:, None, :, None] if masked else None))


# ---------------------------------------------------------------- 4. hard inputs
def _worst_ratio(got, want, A):
    """max over the finite rows of |got - want| / (2 (2^-9 A + 2^-9 |want|)); NaN exactly on the fully masked rows."""
    dead = torch.isnan(want)
    assert torch.equal(torch.isnan(got), dead) and bool(torch.isfinite(got[~dead]).all())
    tol = 2.0 * (EPS * A + EPS * want.abs())
    err = (got.double() - want).abs()
    assert bool((tol[~dead] > 0).all())
    return float((err[~dead] / tol[~dead]).max())


@pytest.mark.parametrize("geometry", cases.HARD_GEOMETRIES, ids=lambda g: "L%d-S%d-N%d-h%d-d%d" % g)
@pytest.mark.parametrize("family", hi.ATTN_FAMILIES)
def test_hard_inputs_stay_inside_the_derived_bound(family, geometry):
    from pctrans_amd import fused_ops, ragged_attention
    L, S, N, heads, hd = geometry
    c = cases.hard_case(family, geometry)
    q, k, v = c["q"].cuda(), c["k"].cuda(), c["v"].cuda()
    mask = c["mask"].cuda() if c["mask"] is not None else None
    want, A = c["want"], c["A"]
    (qc, qp), (kc, kp) = _split_heads(q, heads), _split_heads(k, heads)
    assert ragged_attention.supported(qc, kc, v, heads, mask)
    out = ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask)
    assert out.shape == (L, N, heads * 16) and out.dtype == torch.bfloat16
    ratio = _worst_ratio(out.float().cpu(), want, A)
    print("%s %s: worst |err| / bound %.3g" % (family, geometry, ratio))
    assert ratio <= 1.0, ratio
    if family == "window_masks":
        assert int(torch.isnan(out.float()).all(-1).sum()) == len(c["dead_rows"])
    _assert_same_bits(out, fused_ops.masked_attention(q, k, v, heads, mask))
    if family == "one_hot":
        # out = bf16(v[p]) exactly wherever the float64 weight of all other keys is below 2^-12
        hot = torch.from_numpy(c["hot"])                                                # [N, heads, L]
        rest = 1.0 - c["p"].gather(-1, hot[..., None])[..., 0]
        sure = (rest < 2.0 ** -12).permute(2, 0, 1)                                     # [L, N, heads]
        assert bool(sure.all())
        vh = c["v"].reshape(S, N, heads, 16).permute(1, 2, 0, 3)                        # [N, heads, S, 16]
        picked = vh.gather(2, hot[..., None].expand(-1, -1, -1, 16)).permute(2, 0, 1, 3)   # [L, N, heads, 16]
        got = out.cpu().reshape(L, N, heads, 16)
        assert torch.equal(got[sure].view(torch.int16), picked[sure].view(torch.int16))


# ---------------------------------------------------------------- 5. the float formulation
@pytest.mark.parametrize("L,S,N,heads,masked", [(37, 33, 2, 8, True), (65, 97, 3, 4, True), (100, 374, 2, 8, True),
                                                (10, 22, 1, 12, False), (300, 1452, 1, 8, True)])
def test_float_formulation_at_bf16_tolerance(L, S, N, heads, masked):
    from pctrans_amd import ragged_attention
    qc, qp, kc, kp, v = cases.operands(L, S, N, heads, seed=L + S)
    mask = None
    if masked:
        gm = torch.Generator(device="cuda").manual_seed(1000 + L + S)
        mask = torch.rand(N, 1, L, S, device="cuda", generator=gm) < 0.7
        mask[..., 0] = False                                       # no fully masked row
    got = ragged_attention.cross_attention(qc, qp, kc, kp, v, heads, mask)
    want = _attn_reference(_cat_heads(qc, qp, heads), _cat_heads(kc, kp, heads), v, heads, mask)
    assert torch.isfinite(got.float()).all()
    err = (got.float() - want).abs()
    assert float(err.max()) < 3e-2 and float(err.mean()) < 3e-3, (float(err.max()), float(err.mean()))


# ---------------------------------------------------------------- 6. and 7. the call sites
class _Recorder:
    """Counts and keeps the calls of ragged_attention.cross_attention, counts fused_ops.masked_attention by its key count and
    the layer's V^T products (torch.baddbmm on a token-major operand)."""

    def __init__(self, monkeypatch):
        from pctrans_amd import fused_ops, ragged_attention
        self.ragged, self.generic_keys, self.vt = [], [], 0
        self.masked_attention = real_generic = fused_ops.masked_attention
        real_ragged, real_baddbmm = ragged_attention.cross_attention, torch.baddbmm

        def ragged(qc, qp, kc, kp, v, heads, attn_mask=None, row_open=None):
            out = real_ragged(qc, qp, kc, kp, v, heads, attn_mask, row_open=row_open)
            self.ragged.append(dict(ops=[t.clone() for t in (qc, qp, kc, kp, v)], heads=heads,
                                    mask=None if attn_mask is None else attn_mask.clone(),
                                    row_open=None if row_open is None else row_open.clone(), out=out.clone()))
            return out

        def generic(q, k, v, heads, attn_mask=None, v_t=None):
            self.generic_keys.append(k.shape[0])
            return real_generic(q, k, v, heads, attn_mask, v_t=v_t)

        def baddbmm(*a, **kw):
            # the layer's V^T product reads `memory.permute(1, 2, 0)`: channels at stride 1, tokens strided (the head's other
            # baddbmm calls read channel-major maps)
            x = a[2]
            self.vt += int(x.dim() == 3 and x.shape[1] > 1 and x.stride(1) == 1 and x.stride(2) != 1)
            return real_baddbmm(*a, **kw)

        monkeypatch.setattr(ragged_attention, "cross_attention", ragged)
        monkeypatch.setattr(fused_ops, "masked_attention", generic)
        monkeypatch.setattr(torch, "baddbmm", baddbmm)

    def check_calls(self):
        """Every kept call, re-run through the generic kernel on its own concatenated operands: the same bits."""
        for c in self.ragged:
            qc, qp, kc, kp, v = c["ops"]
            h, mask = c["heads"], c["mask"]
            if mask is not None and c["row_open"] is not None:
                mask = mask & ~c["row_open"].reshape(mask.shape[0], 1, mask.shape[2], 1)
            want = self.masked_attention(_cat_heads(qc, qp, h), _cat_heads(kc, kp, h), v, h, mask)
            _assert_same_bits(c["out"], want, "S=%d" % kc.shape[0])


def test_layer_takes_the_ragged_route_behind_its_switch(monkeypatch):
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    Q, S, N, C, heads = 37, 13 * 17, 2, 128, 8
    torch.manual_seed(0)
    layer = CrossAttentionLayer(C, heads).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    mask = torch.rand(N, 1, Q, S, device="cuda", generator=g) < 0.6
    mask[0, 0, 4, :] = True
    mask[N - 1, 0, Q - 1, :] = True
    kw = dict(tgt=rnd(Q, N, C), memory=rnd(S, N, C), memory_mask=mask, pos=rnd(S, N, C), query_pos=rnd(Q, N, C),
              query_sine_embed=rnd(Q, N, 2 * C), is_first=True, memory_row_open=mask.all(-1, keepdim=True))
    rec = _Recorder(monkeypatch)

    def run(switch):
        layer.ragged_keys = switch
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return layer(**kw)

    want = run("torch")
    assert (len(rec.ragged), rec.generic_keys, rec.vt) == (0, [S], 1)              # today's route, untouched by the switch
    got = run("hip")
    assert (len(rec.ragged), rec.generic_keys, rec.vt) == (1, [S], 1)              # entered once; nothing added to the others
    assert rec.ragged[0]["row_open"] is not None and int(rec.ragged[0]["row_open"].sum()) == 2
    assert tuple(rec.ragged[0]["ops"][2].shape) == (S, N, C)
    rec.check_calls()
    assert got.shape == want.shape and torch.isfinite(got).all()
    # the two routes form V with different GEMMs: close, not equal
    assert float((got.float() - want.float()).abs().max()) < 0.1


def test_whole_head_on_an_unpadded_image_runs_all_nine_layers_on_the_ragged_kernel(monkeypatch):
    """ResNet-18 features of a 104 x 136 image as a ResNet gives them (sizes round up: 26 x 34, 13 x 17, 7 x 9, 4 x 5): the
    decoder's levels have 20, 63 and 221 keys.  The final masks are not compared across the routes: V comes from different
    GEMMs, and thresholds of a random-init head flip."""
    from pctrans_amd.transformer_decoder.mask2former_transformer_decoder import CrossAttentionLayer
    H, W, Q = 104, 136, 20
    head, feats = chk.build_head(18, H, W, Q, 3, 1, None)
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = {k: torch.randn(1, f.shape[1], -(-H // s), -(-W // s), device="cuda", generator=g)
             for (k, f), s in zip(sorted(feats.items()), (4, 8, 16, 32))}
    assert [tuple(feats[k].shape[2:]) for k in ("res2", "res3", "res4", "res5")] == [(26, 34), (13, 17), (7, 9), (4, 5)]
    layers = [m for m in head.modules() if isinstance(m, CrossAttentionLayer)]
    assert len(layers) == 9 and all(m.ragged_keys == "torch" for m in layers)
    for m in layers:
        m.ragged_keys = "hip"
    rec = _Recorder(monkeypatch)
    out = chk.forward(head, feats, "bf16")
    assert [c["ops"][2].shape[0] for c in rec.ragged] == [20, 63, 221] * 3
    assert len(rec.generic_keys) == 9 and set(rec.generic_keys) == {Q}             # the self-attentions alone
    assert rec.vt == 0
    assert all(c["mask"] is not None and c["row_open"] is not None for c in rec.ragged)
    rec.check_calls()
    assert torch.isfinite(out["pred_masks"].float()).all()

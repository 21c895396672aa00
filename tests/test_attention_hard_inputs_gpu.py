"""GPU: the online-softmax step shared by the two bf16 MFMA attention kernels (csrc/attn_common.hpp) on the operand families
of tests/hard_inputs.py -- peaked scores as a trained decoder produces them, scores monotone in the key index (the running
maximum moves at every 32-key step / never after the first key), one live key per query at every position of the step layout,
small mask windows (ragged tail, dead leading steps, fully masked rows), value outliers on keys without weight, underflow --
through three routes: masked_attention with `v`, with `v_t`, and cross_attention on split operands where S % 64 == 0.

The bound comes from what the kernel does, not from torch under autocast.  With p the float64 probabilities of the exact bf16
operands, A = sum_i p_i |v_i| and `want` the float64 output:
  * P is rounded to bf16 before P.V: at most 2^-9 relative per term, 2^-9 A in total;
  * the output is rounded to bf16: at most 2^-9 |out|;
  * __expf and the fp32 accumulation sit orders of magnitude below both.
Per element |got - want| <= 2 (2^-9 A + 2^-9 |want|), the factor 2 being the margin.  The worst ratio to that bound is
printed per case, and next to it the ratio of the bf16-autocast formulation (the yardstick of the call-site checks), for
information only."""
import pytest
import torch

import hard_inputs as hi

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -9


def _split_heads(t, heads):
    """[T, N, heads*32] -> the content / positional halves [T, N, heads*16] whose per-head concatenation is t."""
    T, N, _ = t.shape
    t = t.reshape(T, N, heads, 32)
    return t[..., :16].reshape(T, N, heads * 16).contiguous(), t[..., 16:].reshape(T, N, heads * 16).contiguous()


def _autocast_formulation(q, k, v, mask, heads):
    """The torch path of attention_core as bf16 autocast evaluates it: q * scale, the scores and P in bf16, softmax in fp32."""
    L, N, E = q.shape
    S, hd = k.shape[0], E // heads
    qh = (q * (float(hd) ** -0.5)).reshape(L, N, heads, hd).permute(1, 2, 0, 3)
    kh = k.reshape(S, N, heads, hd).permute(1, 2, 3, 0)
    vh = v.reshape(S, N, heads, 16).permute(1, 2, 0, 3)
    s = torch.matmul(qh, kh)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s.float(), -1).bfloat16()
    return torch.matmul(p, vh).permute(2, 0, 1, 3).reshape(L, N, heads * 16)


def _worst_ratio(got, want, A):
    """max over the finite rows of |got - want| / (2 (2^-9 A + 2^-9 |want|)); NaN exactly on the fully masked rows."""
    dead = torch.isnan(want)
    assert torch.equal(torch.isnan(got), dead) and bool(torch.isfinite(got[~dead]).all())
    tol = 2.0 * (EPS * A + EPS * want.abs())
    err = (got.double() - want).abs()
    assert bool((tol[~dead] > 0).all())
    return float((err[~dead] / tol[~dead]).max())


@pytest.mark.parametrize("geometry", hi.ATTN_GEOMETRIES, ids=lambda g: "L%d-S%d-N%d-h%d-d%d" % g)
@pytest.mark.parametrize("family", hi.ATTN_FAMILIES)
def test_attention_routes_stay_inside_the_derived_bound(family, geometry):
    from pctrans_amd import fused_ops
    L, S, N, heads, hd = geometry
    c = hi.attention_case(family, geometry)
    q, k, v = c["q"].cuda(), c["k"].cuda(), c["v"].cuda()
    mask = c["mask"].cuda() if c["mask"] is not None else None
    want, A = c["want"], c["A"]
    assert fused_ops.masked_attention_supported(q, k, v, heads, mask, None, 0.0, False, False)
    routes = {"v": fused_ops.masked_attention(q, k, v, heads, mask),
              "v_t": fused_ops.masked_attention(q, k, None, heads, mask, v_t=v.permute(1, 2, 0).contiguous())}
    if hd == 32 and S % 64 == 0:
        (qc, qp), (kc, kp) = _split_heads(q, heads), _split_heads(k, heads)
        assert fused_ops.cross_attention_supported(qc, kc, v, heads, mask)
        routes["cross"] = fused_ops.cross_attention(qc, qp, kc, kp, v, heads, mask)
    ratios = {}
    for name, out in routes.items():
        assert out.shape == (L, N, heads * 16) and out.dtype == torch.bfloat16
        ratios[name] = _worst_ratio(out.float().cpu(), want, A)
    yard = _autocast_formulation(q, k, v, mask, heads).float().cpu()
    live = ~torch.isnan(want)
    yard_ratio = float(((yard.double() - want).abs()[live] / (2.0 * (EPS * A + EPS * want.abs()))[live]).max())
    print("%s %s: worst |err| / bound %s; bf16-autocast formulation %.3g"
          % (family, geometry, ", ".join("%s %.3g" % kv for kv in ratios.items()), yard_ratio))
    assert max(ratios.values()) <= 1.0, ratios
    # one accumulation order for all three routes: the same bits (off the NaN rows, which were compared above)
    for name in ("v_t", "cross"):
        if name in routes:
            assert torch.equal(routes[name].view(torch.int16).cpu()[live], routes["v"].view(torch.int16).cpu()[live]), name
    if family == "one_hot":
        # out = bf16(v[p]) exactly wherever the float64 weight of all other keys is below 2^-12
        hot = torch.from_numpy(c["hot"])                                                # [N, heads, L]
        rest = 1.0 - c["p"].gather(-1, hot[..., None])[..., 0]                          # [N, heads, L]
        sure = (rest < 2.0 ** -12).permute(2, 0, 1)                                     # [L, N, heads]
        assert bool(sure.all())
        vh = c["v"].reshape(S, N, heads, 16).permute(1, 2, 0, 3)                        # [N, heads, S, 16]
        picked = vh.gather(2, hot[..., None].expand(-1, -1, -1, 16)).permute(2, 0, 1, 3)   # [L, N, heads, 16]
        for name, out in routes.items():
            got = out.cpu().reshape(L, N, heads, 16)
            assert torch.equal(got[sure].view(torch.int16), picked[sure].view(torch.int16)), name

"""GPU: every HIP entry point of the head checked against float64 on the operands it actually received, at the BASELINE
head shapes and at the bench geometry (tests/callsite_capture.py records the calls, tests/callsite_reference.py defines
the operations).  Each call is compared on its own inputs, so a threshold decision that flips in one decoder layer cannot
cascade into the next one's comparison, and every element of every call is held to the bound:
  * fp32 kernels: error vs float64 at most twice that of the same operation done by torch in fp32 on the same inputs
    (TF32 off), with a floor of 5e-6 x scale (scale = max(1, |reference|)); MSDeformAttn also within 1e-4 absolute;
  * bf16 kernels: the yardstick is torch under bf16 autocast on the same inputs (attention: P rounded to bf16 before P.V;
    mask head: the bf16 chain of test_dyn_mask_head_gpu with its third layer's operands rounded as well, see
    callsite_reference.mask_head_autocast): maximum error at most 2x, mean error at most 1.5x the yardstick's;
  * attention-mask bits: may differ from float64 only where the float64 resized logit is within the logit bound of 0,
    and in fewer than 1e-3 of the bits (or twice the yardstick's own share, where that is larger);
  * attention rows that are NaN in float64 (fully masked) are NaN in the output, and no others.
Each configuration must hit the expected number of calls per entry point, and every MSDeformAttn call the kernel family
`auto` is pinned to (test_msda_col_gpu.py::test_auto_kernel_choice_per_baseline_config).

Observed on the MI355X, largest error / yardstick-error over all geometries (run with -rP to print them per test):
bf16 masked_attention max 1.27 / mean 1.00, cross_attention 1.08 / 1.00, mask head 1.00 / 1.00; fp32 MSDeformAttn 1.11,
linear_k128_multi 0.43, linear_add_layer_norm 1.07, ffn_layer_norm 0.65, conv1x1_groupnorm_tokens_into 0.97,
groupnorm_flatten_into 1.64, conv1x1_from_token_rows 0.90; conv1x1_nchw (2.89) and the fp32 mask head (3.40) exceed 2 only
where the 5e-6 x scale floor is the bound."""
import types

import pytest
import torch

import callsite_reference as ref
from callsite_capture import CallsiteCapture

pytestmark = pytest.mark.gpu

K_DPP, K_COL = 3, 4

# name -> (ResNet depth, H, W, queries, pixel-decoder levels, batch): test_head_gpu's BASELINE head shapes
CONFIGS = {
    "cfg1_cvppp_tile_r18_q50": (18, 256, 256, 50, 3, 1),
    "cfg3_cvppp_val_530x500": (50, 544, 512, 100, 3, 2),
    "cfg4_bbbc_520x696_q300": (50, 544, 704, 300, 3, 2),
    "cfg2_north_star_l4": (50, 512, 512, 100, 4, 2),
}

# the MSDeformAttn family `auto` launches.  cfg1 / cfg2 / bench as pinned in test_auto_kernel_choice_per_baseline_config
# (cfg1_256_b1; cfg2_512_b1 / _b8 bracket batch 2; cfg2_512_b128_fused).  Not in that table, stated here: cfg3 at 544 x 512
# (N*S*M = 91 392) and cfg4 at 544 x 704 (125 664) stay below the 3-level column threshold (450 000) and fill fewer than
# 3 x 768 windowed work items -> the quad-owner kernel.
MSDA_FAMILY = {"cfg1_cvppp_tile_r18_q50": K_DPP, "cfg3_cvppp_val_530x500": K_DPP, "cfg4_bbbc_520x696_q300": K_DPP,
               "cfg2_north_star_l4": K_COL, "bench": K_COL}

_ZERO = dict.fromkeys([
    "fused_ops.linear", "fused_ops.linear_k128_multi", "fused_ops.linear_add_layer_norm", "fused_ops.linear_layer_norm",
    "fused_ops.ffn_layer_norm", "fused_ops.conv1x1_nchw", "fused_ops.conv1x1_groupnorm_tokens_into",
    "fused_ops.groupnorm_flatten_into", "fused_ops.conv1x1_from_token_rows", "fused_ops.masked_attention",
    "fused_ops.cross_attention", "MSDA.ms_deform_attn_fused_forward", "MSDA.ms_deform_attn_forward",
    "dynamic_mask_head.dynamic_mask_head_forward"], 0)


def _expected(name, precision):
    """Calls per entry point of one forward.  Encoder: 6 layers, each the three input projections (one merged launch from
    4 096 token rows on, else three `linear`s), the fused MSDeformAttn, output_proj + residual + LayerNorm and the FFN.
    Input projections: one conv + GroupNorm + flatten per level where every level has H*W % 128 == 0, else a conv and a
    GroupNorm-flatten per level.  Decoder: 10 mask-head calls; under bf16 9 self-attentions on masked_attention and 9
    cross-attentions, on cross_attention where the level has a multiple of 64 keys, else on masked_attention with V^T.
    The 16-channel mask projection reads the encoder's token rows at batch <= 4 from 4 096 pixels on (not cfg1's 32 x 32
    map, not the bench's batch 128); the mask head then runs on fp32 features (fp32 logits) under autocast as well."""
    e = dict(_ZERO)
    e.update({"MSDA.ms_deform_attn_fused_forward": 6, "fused_ops.linear_add_layer_norm": 6,
              "fused_ops.ffn_layer_norm": 6, "dynamic_mask_head.dynamic_mask_head_forward": 10})
    if name == "cfg1_cvppp_tile_r18_q50":                       # 1 344 token rows: three `linear`s per layer
        e["fused_ops.linear"] = 18
    else:
        e["fused_ops.linear_k128_multi"] = 6
    if name in ("cfg2_north_star_l4", "bench"):
        e["fused_ops.conv1x1_groupnorm_tokens_into"] = 4
    else:                                                       # a level with H*W % 128 != 0 (8x8, 17x16, 17x22)
        e["fused_ops.conv1x1_nchw"] = e["fused_ops.groupnorm_flatten_into"] = 3
    if name != "cfg1_cvppp_tile_r18_q50" and name != "bench":  # batch <= 4 and a mask-feature map of >= 4 096 pixels
        e["fused_ops.conv1x1_from_token_rows"] = 1
    if precision == "bf16":
        # keys per cross-attention level: cfg1 64 / 256 / 1024, cfg3 272 / 1088 / 4352, cfg4 374 / 1496 / 5984,
        # cfg2 and bench 256 / 1024 / 4096; layer i reads level i % 3
        split = {"cfg1_cvppp_tile_r18_q50": 9, "cfg3_cvppp_val_530x500": 6, "cfg4_bbbc_520x696_q300": 0}.get(name, 9)
        e["fused_ops.cross_attention"] = split
        e["fused_ops.masked_attention"] = 9 + (9 - split)
    return e


@pytest.fixture
def no_tf32(monkeypatch):
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)


# ---------------------------------------------------------------- bounds
class Report:
    """Largest error / yardstick-error ratio per entry point (max and, for bf16, mean), printed at the end of a test."""

    def __init__(self, label):
        self.label, self.worst = label, {}

    def note(self, entry, kind, ratio):
        key = (entry.split(".")[-1], kind)
        self.worst[key] = max(self.worst.get(key, 0.0), ratio)

    def show(self):
        items = ", ".join("%s %s %.2f" % (e, k, r) for (e, k), r in sorted(self.worst.items()))
        print("\n[callsite ratios] %s: %s" % (self.label, items))


def _fp32_bound(got, want, yard, what, report, entry, abs_cap=None):
    """-> the logit bound applied (for the mask-bit check)."""
    got, want, yard = got.double(), want.double(), yard.double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all(), what
    scale = max(1.0, float(want.abs().max()))
    err, err32 = float((got - want).abs().max()), float((yard - want).abs().max())
    bound = max(2.0 * err32, 5e-6 * scale)
    report.note(entry, "max", err / max(err32, 1e-30))
    assert err <= bound, "%s: max|err| %.3g > %.3g (fp32 torch %.3g, scale %.3g)" % (what, err, bound, err32, scale)
    if abs_cap is not None:
        assert err <= abs_cap, "%s: max|err| %.3g above %.0e" % (what, err, abs_cap)
    return bound


def _bf16_bound(got, want, yard, what, report, entry, rows_dim=None):
    """bf16 rule on every element; with `rows_dim`, NaN rows (fully masked attention rows) are checked for agreement and
    left out of the error statistics."""
    got, want, yard = got.double(), want.double(), yard.double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    live = torch.ones_like(want, dtype=torch.bool)
    if rows_dim is not None:
        nan_w, nan_g = torch.isnan(want), torch.isnan(got)
        assert torch.equal(nan_w.all(rows_dim), nan_w.any(rows_dim)), what      # a NaN reference row is NaN throughout
        assert torch.equal(nan_g.all(rows_dim), nan_w.all(rows_dim)), \
            "%s: NaN rows differ (%d in the output, %d in float64)" % (what, int(nan_g.all(rows_dim).sum()),
                                                                        int(nan_w.all(rows_dim).sum()))
        live = ~nan_w
    assert torch.isfinite(got[live]).all(), what
    e, ey = (got - want)[live].abs(), (yard - want)[live].abs()
    if e.numel() == 0:
        return 0.0
    mx, mxy, mn, mny = float(e.max()), float(ey.max()), float(e.mean()), float(ey.mean())
    report.note(entry, "max", mx / max(mxy, 1e-30))
    report.note(entry, "mean", mn / max(mny, 1e-30))
    assert mx <= 2.0 * mxy, "%s: max|err| %.3g > 2 x autocast torch %.3g" % (what, mx, mxy)
    assert mn <= 1.5 * mny, "%s: mean|err| %.3g > 1.5 x autocast torch %.3g" % (what, mn, mny)
    return 2.0 * mxy


def _mask_bits(got, resized64, resized_yard, tol, what):
    """Bits may differ only within `tol` of the threshold, and rarely: in fewer than 1e-3 of them, or -- where the
    yardstick's own rounding already flips more (bf16 logits of magnitude ~30 carry a rounding of 0.1) -- in at most
    twice the yardstick's share."""
    want = resized64 < 0                                        # sigmoid(x) < 0.5
    differ = got != want
    if bool(differ.any()):
        near = float(resized64[differ].abs().max())
        assert near <= tol, "%s: a mask bit differs where the float64 logit is %.3g from 0 (bound %.3g)" % (what, near, tol)
    share, share_y = float(differ.float().mean()), float(((resized_yard < 0) != want).float().mean())
    assert share < max(1e-3, 2.0 * share_y), (what, share, share_y)


# ---------------------------------------------------------------- one check per entry point
def _check(call, report):
    a, e = call.args, call.entry
    what = "%s%s" % (e, "" if call.images is None else " images %s" % call.images)
    if e == "fused_ops.linear":
        want = ref.linear(a["x"], a["lin"], a["relu"], a["x_add"])
        yard = ref.linear(a["x"], a["lin"], a["relu"], a["x_add"], dtype=torch.float32)
        _fp32_bound(call.out, want, yard, what, report, e)
    elif e == "fused_ops.linear_k128_multi":
        wants = ref.linear_k128_multi(a["x"], a["layers"], a["x_add"])
        yards = ref.linear_k128_multi(a["x"], a["layers"], a["x_add"], dtype=torch.float32)
        assert len(call.out) == len(wants)
        for i, (g, w, y) in enumerate(zip(call.out, wants, yards)):
            _fp32_bound(g, w, y, "%s output %d" % (what, i), report, e)
    elif e in ("fused_ops.linear_add_layer_norm", "fused_ops.linear_layer_norm"):
        want = ref.linear_add_layer_norm(a["x"], a["linear"], a["residual"], a["norm"])
        yard = ref.linear_add_layer_norm(a["x"], a["linear"], a["residual"], a["norm"], dtype=torch.float32)
        _fp32_bound(call.out, want, yard, what, report, e)
    elif e == "fused_ops.ffn_layer_norm":
        want = ref.ffn_layer_norm(a["x"], a["linear1"], a["linear2"], a["norm"])
        yard = ref.ffn_layer_norm(a["x"], a["linear1"], a["linear2"], a["norm"], dtype=torch.float32)
        _fp32_bound(call.out, want, yard, what, report, e)
    elif e in ("fused_ops.conv1x1_nchw", "fused_ops.conv1x1_from_token_rows"):
        _fp32_bound(call.out, ref.conv1x1(a["x"], a["conv"]), ref.conv1x1(a["x"], a["conv"], torch.float32), what, report, e)
    elif e == "fused_ops.conv1x1_groupnorm_tokens_into":
        want = ref.conv1x1_groupnorm_tokens(a["x"], a["conv"], a["gn"])
        yard = ref.conv1x1_groupnorm_tokens(a["x"], a["conv"], a["gn"], torch.float32)
        _fp32_bound(call.out, want, yard, "%s at row %d" % (what, a["row_offset"]), report, e)
    elif e == "fused_ops.groupnorm_flatten_into":
        want = ref.groupnorm_flatten(a["x"], a["gn"])
        yard = ref.groupnorm_flatten(a["x"], a["gn"], torch.float32)
        _fp32_bound(call.out, want, yard, "%s at row %d" % (what, a["row_offset"]), report, e)
    elif e == "MSDA.ms_deform_attn_fused_forward":
        args = (a["value"], a["spatial_shapes"], a["reference_points"], a["sampling_offsets"], a["attention_logits"])
        _fp32_bound(call.out, ref.msda_fused(*args), ref.msda_fused(*args, dtype=torch.float32), what, report, e,
                    abs_cap=1e-4)
    elif e == "MSDA.ms_deform_attn_forward":
        args = (a["value"], a["spatial_shapes"], a["sampling_loc"], a["attn_weight"])
        _fp32_bound(call.out, ref.msda(*args), ref.msda(*args, dtype=torch.float32), what, report, e, abs_cap=1e-4)
    elif e == "fused_ops.masked_attention":
        v = a["v"] if a["v"] is not None else a["v_t"].permute(2, 0, 1)
        want = ref.attention(a["q"], a["k"], v, a["num_heads"], a["attn_mask"])
        yard = ref.attention_autocast(a["q"], a["k"], v, a["num_heads"], a["attn_mask"])
        _bf16_bound(call.out, want, yard, what + (" (V^T)" if a["v"] is None else ""), report, e, rows_dim=-1)
    elif e == "fused_ops.cross_attention":
        q, k, m = ref.cross_operands(a["q_content"], a["q_pos"], a["k_content"], a["k_pos"], a["num_heads"],
                                     a["attn_mask"], a["row_open"])
        want = ref.attention(q, k, a["v"], a["num_heads"], m)
        yard = ref.attention_autocast(q, k, a["v"], a["num_heads"], m)
        _bf16_bound(call.out, want, yard, "%s S=%d" % (what, k.shape[0]), report, e, rows_dim=-1)
    elif e == "dynamic_mask_head.dynamic_mask_head_forward":
        up, amask = call.out
        feats, stride, target = a["feats_f32"], a["stride"], a["target_size"]
        up64, rs64 = ref.mask_head(feats, a["ref_xy"], a["params"], stride, a["rel_coord"], target)
        what = "%s %dx%d -> %s" % (what, feats.shape[2], feats.shape[3], tuple(target))
        if a["out_dtype"] == torch.float32:
            up32, rs32 = ref.mask_head(feats, a["ref_xy"], a["params"], stride, a["rel_coord"], target, torch.float32)
            bound = _fp32_bound(up, up64, up32, what, report, e)
            tol = max(bound, 2.0 * float((rs32.double() - rs64).abs().max()))
            rsy = rs32
        else:
            assert up.dtype == torch.bfloat16 and a["rel_coord"]
            upy, rsy = ref.mask_head_autocast(feats, a["ref_xy"], a["params"], stride, target)
            bound = _bf16_bound(up, up64, upy, what, report, e)
            tol = max(bound, 2.0 * float((rsy.double() - rs64).abs().max()))
        _mask_bits(amask, rs64, rsy.double(), tol, what)
    else:
        raise AssertionError("no reference for " + e)


def _check_all(cap, family, report):
    for e, calls in cap.calls.items():
        for c in calls:
            if c.kernel is not None:
                assert c.kernel == family, "%s ran kernel family %d, expected %d" % (e, c.kernel, family)
            _check(c, report)
            del c.args, c.out                                   # free the copies as the check goes
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the head at the BASELINE shapes
def _head(name, offsets):
    from pctrans_amd.config import get_cfg, resnet_output_shape
    from pctrans_amd.meta_arch.mask_former_head import MaskFormerHead
    depth, H, W, Q, levels, N = CONFIGS[name]
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=Q, enc_in_features=("res2", "res3", "res4", "res5")[4 - levels:], norm="BN", sem_norm="BN")
    shapes = resnet_output_shape(depth)
    head = MaskFormerHead(**MaskFormerHead.from_config(cfg, shapes)).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = {k: torch.randn(N, s.channels, H // s.stride, W // s.stride, device="cuda", generator=g)
             for k, s in shapes.items()}
    if offsets == "M":
        import bench
        bench.model_like_offsets(head, feats)
    return head, feats


def _forward(head, feats, precision):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
        out, _ = head(feats)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("offsets", ["init", "M"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_head_kernel_call_matches_float64(monkeypatch, no_tf32, name, offsets, precision):
    head, feats = _head(name, offsets)
    cap = CallsiteCapture().install(monkeypatch)
    _forward(head, feats, precision)
    assert cap.counts() == _expected(name, precision)
    report = Report("%s %s %s" % (name, offsets, precision))
    _check_all(cap, MSDA_FAMILY[name], report)
    report.show()


# ---------------------------------------------------------------- the bench geometry
def test_every_head_kernel_call_matches_float64_at_bench_geometry(monkeypatch, no_tf32):
    """bench.py's workload: batch 128, 512^2, 4 levels, 100 queries, bf16 autocast, distribution-M offsets.  The first, a
    middle and the last image of every call are checked (the last ones are the persistent grids' late items)."""
    import bench
    head, shapes = bench.build_head(types.SimpleNamespace(levels=4, queries=100), torch.device("cuda"))
    feats = bench.synth_features(shapes, 128, 512, "cuda", seed=1234)
    bench.model_like_offsets(head, feats)
    cap = CallsiteCapture(select=[0, 63, 127]).install(monkeypatch)
    _forward(head, feats, "bf16")
    del feats
    assert cap.counts() == _expected("bench", "bf16")
    for calls in cap.calls.values():
        for c in calls:
            assert c.images == [0, 63, 127], c
    report = Report("bench b128 M bf16")
    _check_all(cap, MSDA_FAMILY["bench"], report)
    report.show()

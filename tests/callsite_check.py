"""The per-call float64 check of the head's HIP entry points and the routing rules that say which calls a forward makes
(a plain helper module, like msda_cases.py).  test_callsite_parity_gpu.py runs the check at the BASELINE head shapes and
the bench geometry, test_callsite_geometry_gpu.py at GEOMETRIES, which sit on both sides of every routing threshold.

Bounds, per element of every kept image of every call:
  * fp32 kernels: error vs float64 at most twice that of the same operation done by torch in fp32 on the same inputs
    (TF32 off), with a floor of 5e-6 x scale (scale = max(1, |reference|)); MSDeformAttn also within 1e-4 absolute;
  * bf16 kernels: the yardstick is torch under bf16 autocast on the same inputs (attention: P rounded to bf16 before P.V;
    mask head: the bf16 chain of test_dyn_mask_head_gpu with its third layer's operands rounded as well, see
    callsite_reference.mask_head_autocast): maximum error at most 2x, mean error at most 1.5x the yardstick's;
  * attention-mask bits: may differ from float64 only where the float64 resized logit is within the logit bound of 0,
    and in fewer than 1e-3 of the bits (or twice the yardstick's own share, where that is larger);
  * attention rows that are NaN in float64 (fully masked) are NaN in the output, and no others.

The routing rules (`expected_calls`, `expected_msda_family`, `routes`) restate, from the geometry alone, the decisions
the product makes from tensor shapes; they deliberately do not call the product's `*_supported` predicates, so a moved
threshold shows up as a count mismatch on the GPU instead of moving the expectation with it."""
import math

import torch

import callsite_reference as ref

K_WIN, K_DPP, K_COL = 1, 3, 4                       # pct_msda_last_kernel(): windowed, quad-owner, pyramid column
FAMILY_NAME = {K_WIN: "windowed", K_DPP: "quad-owner", K_COL: "column"}

ENTRIES = (
    "fused_ops.linear", "fused_ops.linear_k128_multi", "fused_ops.linear_add_layer_norm", "fused_ops.linear_layer_norm",
    "fused_ops.ffn_layer_norm", "fused_ops.conv1x1_nchw", "fused_ops.conv1x1_groupnorm_tokens_into",
    "fused_ops.groupnorm_flatten_into", "fused_ops.conv1x1_from_token_rows", "fused_ops.masked_attention",
    "fused_ops.cross_attention", "MSDA.ms_deform_attn_fused_forward", "MSDA.ms_deform_attn_forward",
    "dynamic_mask_head.dynamic_mask_head_forward")


# ---------------------------------------------------------------- routing rules, from the geometry alone
HEADS, POINTS, ENC_LAYERS, DEC_LAYERS = 8, 4, 6, 9  # get_cfg: NHEADS 8, 4 encoder points, 6 encoder / 10 - 1 decoder layers


def level_shapes(levels, H, W):
    """Encoder levels coarse -> fine (res5 first, pixel_decoder/msdeformattn.py `xs`): strides 32, 16, 8 (and 4 with
    four levels).  H and W are image sizes, multiples of 32 as the trainer pads them."""
    assert H % 32 == 0 and W % 32 == 0, (H, W)
    return [(H // s, W // s) for s in (32, 16, 8, 4)[:levels]]


def mask_feature_shape(levels, H, W):
    """The mask features are the finest encoder level (stride 8 with three levels: the FPN adds res2 at that level's size,
    pixel_decoder/msdeformattn.py `F.interpolate(cur_fpn, size=out[-1].shape[-2:])`; stride 4 with four)."""
    return level_shapes(levels, H, W)[-1]


def decoder_keys(levels, H, W):
    """Keys of the decoder's cross-attention layers: layer i reads multi-scale level i % 3 (strides 32, 16, 8)."""
    lv = level_shapes(levels, H, W)[:3]
    return [lv[i % 3][0] * lv[i % 3][1] for i in range(DEC_LAYERS)]


def merged_projections(levels, H, W, N):
    """The encoder's three input projections in one `linear_k128_multi` launch:
    fused_ops.linear_k128_supported (`x.numel() >= 128 * 4096`: at least 4 096 token rows over the batch) and
    fused_ops._x_add_ok for the shared [1, S, 128] position table (`x.numel() // x.shape[0] // 128 >= 32`: 32 rows per
    image).  Else three `fused_ops.linear`s.  The same 4 096-row rule picks linear_add_layer_norm's K = 128 kernel; below
    it that entry runs the `linear` fallback and pct_add_layernorm_f32."""
    S = sum(h * w for h, w in level_shapes(levels, H, W))
    return N * S >= 4096 and S >= 32


def fused_input_projection(levels, H, W):
    """`conv1x1_groupnorm_tokens_into` per level where EVERY level has H*W % 128 == 0 (fused_ops.conv1x1_nchw_supported;
    ResNet channel counts are multiples of 16), else `conv1x1_nchw` + `groupnorm_flatten_into` per level."""
    return all((h * w) % 128 == 0 for h, w in level_shapes(levels, H, W))


def mask_projection_from_token_rows(levels, H, W, N):
    """fused_ops.conv1x1_from_token_rows_supported: batch <= 4 and a mask-feature map of >= 4 096 pixels.  The map is a
    channels-last view of the encoder's token rows (four levels) or the FPN output (three levels), which is channels-last
    from batch 2 on and NCHW-contiguous at batch 1; the predicate takes both layouts."""
    h, w = mask_feature_shape(levels, H, W)
    return N <= 4 and h * w >= 4096


def cross_attention_split(S):
    """fused_ops.cross_attention_supported: `S % 64 == 0` keys (heads % 4 == 0 and 16 channels per head always hold);
    else the cross-attention runs on masked_attention with V^T."""
    return S % 64 == 0


def _dmh_fused(H, W, th, tw):
    """dynamic_mask_head.fused_geometry: a 128-pixel-wide map of a multiple of 8 rows, the attention-mask target an exact
    1/2, 1/4 or 1/8 of it."""
    return (W == 128 and H >= 8 and H % 8 == 0 and H % th == 0 and W % tw == 0 and H // th == W // tw
            and H // th in (2, 4, 8))


def mask_head_kernels(levels, H, W, N, precision):
    """Kernel of each of the 10 mask-head calls: "valu" (fp32 features: the fp32 run, or the token-row projection's fp32
    output under autocast too), else under bf16 "fused" (the one-launch kernel, dynamic_mask_head.fused_geometry) or
    "mfma" (two launches).  Call 0 targets level 0, call i + 1 level (i + 1) % 3 (decoder `attn_mask_target_size`)."""
    if precision == "fp32" or mask_projection_from_token_rows(levels, H, W, N):
        return ["valu"] * (DEC_LAYERS + 1)
    mh, mw = mask_feature_shape(levels, H, W)
    lv = level_shapes(levels, H, W)[:3]
    return ["fused" if _dmh_fused(mh, mw, *lv[i % 3]) else "mfma" for i in range(DEC_LAYERS + 1)]


def expected_msda_family(levels, H, W, N):
    """The MSDeformAttn kernel `auto` launches for the encoder's fused forward (Lq == S, fp32, 4 points), restating
    launch_msda_forward_special in csrc/msda_forward.hip: the column kernel from N*S*M >= 160 000 (>= 4 levels) or
    450 000 (3 levels); else the windowed kernel once N * ceil(S / 256) * M >= 3 * 768 work items fill its grid (and
    N*S*M >= 32 768, msda_forward_win.hip); else the quad-owner kernel."""
    S = sum(h * w for h, w in level_shapes(levels, H, W))
    if N * S * HEADS >= (160000 if levels >= 4 else 450000):
        return K_COL
    if N * math.ceil(S / 256) * HEADS >= 3 * 768 and N * S * HEADS >= 32768:
        return K_WIN
    return K_DPP


def expected_calls(levels, H, W, N, Q, precision):
    """Calls per entry point of one forward.  Encoder: 6 layers, each the three input projections (merged_projections),
    the fused MSDeformAttn, output_proj + residual + LayerNorm and the FFN.  Input projections: fused_input_projection.
    Decoder: 10 mask-head calls; under bf16 9 self-attentions on masked_attention and 9 cross-attentions, on
    cross_attention where the level has a multiple of 64 keys, else on masked_attention with V^T.  The mask projection:
    mask_projection_from_token_rows.  (Q changes no count; it is part of the geometry all the same.)"""
    e = dict.fromkeys(ENTRIES, 0)
    e.update({"MSDA.ms_deform_attn_fused_forward": ENC_LAYERS, "fused_ops.linear_add_layer_norm": ENC_LAYERS,
              "fused_ops.ffn_layer_norm": ENC_LAYERS, "dynamic_mask_head.dynamic_mask_head_forward": DEC_LAYERS + 1})
    if merged_projections(levels, H, W, N):
        e["fused_ops.linear_k128_multi"] = ENC_LAYERS
    else:
        e["fused_ops.linear"] = 3 * ENC_LAYERS
    if fused_input_projection(levels, H, W):
        e["fused_ops.conv1x1_groupnorm_tokens_into"] = levels
    else:
        e["fused_ops.conv1x1_nchw"] = e["fused_ops.groupnorm_flatten_into"] = levels
    if mask_projection_from_token_rows(levels, H, W, N):
        e["fused_ops.conv1x1_from_token_rows"] = 1
    if precision == "bf16":
        split = sum(cross_attention_split(S) for S in decoder_keys(levels, H, W))
        e["fused_ops.cross_attention"] = split
        e["fused_ops.masked_attention"] = DEC_LAYERS + (DEC_LAYERS - split)
    return e


def routes(levels, H, W, N, Q):
    """{(rule, side)} a geometry exercises, over its fp32 and bf16 runs (tests/test_callsite_routes_cpu.py requires both
    sides of every rule)."""
    lv = level_shapes(levels, H, W)
    keys = decoder_keys(levels, H, W)
    out = {("msda L=%d" % levels, FAMILY_NAME[expected_msda_family(levels, H, W, N)]),
           ("input projections", "merged" if merged_projections(levels, H, W, N) else "three linears"),
           ("input_proj L=%d" % levels, "conv+GN fused" if fused_input_projection(levels, H, W) else "conv, GN-flatten"),
           ("mask projection", "token rows" if mask_projection_from_token_rows(levels, H, W, N) else "library conv"),
           ("coarsest level", "< 32 keys" if lv[0][0] * lv[0][1] < 32 else ">= 32 keys"),
           ("queries", str(Q)), ("query tile", "partial" if Q % 16 else "full"),
           ("batch", "odd" if N % 2 else "even")}
    for S in keys:
        side = "cross_attention" if cross_attention_split(S) else "V^T"
        out.add(("cross-attention", side))
        if Q == 300:
            out.add(("cross-attention, 300 queries", side))
    for k in set(mask_head_kernels(levels, H, W, N, "bf16")):
        out.add(("mask head bf16 run", k))
        if k == "fused":
            mh, mw = mask_feature_shape(levels, H, W)
            out.add(("fused mask head queries", "odd" if Q % 2 else "even"))
            out.add(("fused mask head queries", str(Q)))
            out.add(("fused mask head map", "square" if mh == mw else "non-square"))
    return out


class Geometry:
    def __init__(self, levels, depth, H, W, N, Q, select=None):
        self.levels, self.depth, self.H, self.W, self.N, self.Q, self.select = levels, depth, H, W, N, Q, select

    @property
    def key(self):
        return (self.levels, self.H, self.W, self.N, self.Q)

    def __repr__(self):
        return "Geometry(%d levels, r%d, %dx%d, batch %d, %d queries)" % (self.levels, self.depth, self.H, self.W, self.N,
                                                                          self.Q)


# name -> the head's input geometry: encoder levels, ResNet depth, image H x W, batch, queries, images kept (`select`,
# None = all; batches above 4 keep the first and the last).  Each sits next to the threshold(s) named in its comment;
# none repeats a BASELINE config.  S = encoder tokens per image, N*S*M with M = 8 heads.
GEOMETRIES = {
    # coarsest level 5 x 5 = 25 keys (< one 32-key step, odd); 1 575 rows; every decoder level on V^T (25, 100, 400)
    "l3_160x160_b3_q50": Geometry(3, 18, 160, 160, 3, 50),
    # 4 032 token rows: one image below the 4 096-row merged-projection / add_layernorm threshold
    "l3_256_b3_q100": Geometry(3, 50, 256, 256, 3, 100),
    # ... and 5 376 rows: one image above it
    "l3_256_b4_q100": Geometry(3, 18, 256, 256, 4, 100),
    # mask features 64 x 64 = 4 096 pixels: exactly on the token-row projection's pixel threshold; every 3-level input
    # projection a multiple of 128 pixels (256, 1 024, 4 096: conv1x1_groupnorm_tokens_into); 300 queries on
    # cross_attention at every level
    "l3_512_b1_q300": Geometry(3, 50, 512, 512, 1, 300),
    # ... and 60 x 64 = 3 840 pixels, one 32-pixel step of the image below it; 15 x 16 = 240 pixels breaks the fused
    # input projection; 75 queries on cross_attention (960, 3 840 keys) and V^T (240)
    "l3_480x512_b1_q75": Geometry(3, 18, 480, 512, 1, 75),
    # N*S*M = 403 200: one image below the 3-level column threshold (450 000) -> quad-owner
    "l3_640_b6_q100": Geometry(3, 50, 640, 640, 6, 100, select=[0, -1]),
    # N*S*M = 470 400: one image above it -> column kernel at L = 3
    "l3_640_b7_q50": Geometry(3, 50, 640, 640, 7, 50, select=[0, -1]),
    # N*S*M = 97 920: below the 4-level column threshold (160 000) -> quad-owner at L = 4
    "l4_384_b1_q100": Geometry(4, 50, 384, 384, 1, 100),
    # N*S*M = 195 840: one image above it -> column; 300 queries on cross_attention (576, 2 304 keys) and V^T (144)
    "l4_384_b2_q300": Geometry(4, 50, 384, 384, 2, 300),
    # batch 4: the last batch the token-row mask projection takes (mask features 192 x 128 = 24 576 pixels) -> the fp32
    # mask head under autocast too; every level a multiple of 128 pixels (4-level conv1x1_groupnorm_tokens_into)
    "l4_768x512_b4_q100": Geometry(4, 50, 768, 512, 4, 100, select=[0, -1]),
    # ... batch 5, one image over it -> the bf16 one-launch mask head on a non-square 192 x 128 map with 300 queries
    "l4_768x512_b5_q300": Geometry(4, 50, 768, 512, 5, 300, select=[0, -1]),
    # 4 080 token rows: 16 rows below the 4 096-row threshold; mask features 24 x 128 = 3 072 pixels (< 4 096) -> the
    # one-launch bf16 mask head with an odd query count (its last query pair is half empty)
    "l4_96x512_b1_q75": Geometry(4, 18, 96, 512, 1, 75),
}

# geometries with one side of an MSDeformAttn kernel threshold: also run with model-like sampling offsets
MSDA_THRESHOLD_GEOMETRIES = ("l3_640_b6_q100", "l3_640_b7_q50", "l4_384_b1_q100", "l4_384_b2_q300")

# (rule, side) pairs the geometry table must exercise (tests/test_callsite_routes_cpu.py)
REQUIRED_ROUTES = {
    ("msda L=3", "column"), ("msda L=3", "quad-owner"), ("msda L=4", "column"), ("msda L=4", "quad-owner"),
    ("input projections", "merged"), ("input projections", "three linears"),
    ("input_proj L=3", "conv+GN fused"), ("input_proj L=3", "conv, GN-flatten"),
    ("input_proj L=4", "conv+GN fused"), ("input_proj L=4", "conv, GN-flatten"),
    ("cross-attention", "cross_attention"), ("cross-attention", "V^T"),
    ("cross-attention, 300 queries", "cross_attention"), ("cross-attention, 300 queries", "V^T"),
    ("mask projection", "token rows"), ("mask projection", "library conv"),
    ("mask head bf16 run", "valu"), ("mask head bf16 run", "fused"), ("mask head bf16 run", "mfma"),
    ("fused mask head queries", "odd"), ("fused mask head queries", "300"), ("fused mask head map", "non-square"),
    ("coarsest level", "< 32 keys"), ("coarsest level", ">= 32 keys"),
    ("queries", "50"), ("queries", "100"), ("queries", "300"), ("queries", "75"), ("query tile", "partial"),
    ("batch", "odd"), ("batch", "even"),
}


def missing_routes(geometries):
    """REQUIRED_ROUTES that no geometry of `geometries` (name -> Geometry) exercises."""
    seen = set()
    for g in geometries.values():
        seen |= routes(g.levels, g.H, g.W, g.N, g.Q)
    return REQUIRED_ROUTES - seen


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


def fp32_bound(got, want, yard, what, report, entry, abs_cap=None):
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


def bf16_bound(got, want, yard, what, report, entry, rows_dim=None):
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


def mask_bits(got, resized64, resized_yard, tol, what):
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
def check(call, report):
    a, e = call.args, call.entry
    what = "%s%s" % (e, "" if call.images is None else " images %s" % call.images)
    if e == "fused_ops.linear":
        want = ref.linear(a["x"], a["lin"], a["relu"], a["x_add"])
        yard = ref.linear(a["x"], a["lin"], a["relu"], a["x_add"], dtype=torch.float32)
        fp32_bound(call.out, want, yard, what, report, e)
    elif e == "fused_ops.linear_k128_multi":
        wants = ref.linear_k128_multi(a["x"], a["layers"], a["x_add"])
        yards = ref.linear_k128_multi(a["x"], a["layers"], a["x_add"], dtype=torch.float32)
        assert len(call.out) == len(wants)
        for i, (g, w, y) in enumerate(zip(call.out, wants, yards)):
            fp32_bound(g, w, y, "%s output %d" % (what, i), report, e)
    elif e in ("fused_ops.linear_add_layer_norm", "fused_ops.linear_layer_norm"):
        want = ref.linear_add_layer_norm(a["x"], a["linear"], a["residual"], a["norm"])
        yard = ref.linear_add_layer_norm(a["x"], a["linear"], a["residual"], a["norm"], dtype=torch.float32)
        fp32_bound(call.out, want, yard, what, report, e)
    elif e == "fused_ops.ffn_layer_norm":
        want = ref.ffn_layer_norm(a["x"], a["linear1"], a["linear2"], a["norm"])
        yard = ref.ffn_layer_norm(a["x"], a["linear1"], a["linear2"], a["norm"], dtype=torch.float32)
        fp32_bound(call.out, want, yard, what, report, e)
    elif e in ("fused_ops.conv1x1_nchw", "fused_ops.conv1x1_from_token_rows"):
        fp32_bound(call.out, ref.conv1x1(a["x"], a["conv"]), ref.conv1x1(a["x"], a["conv"], torch.float32), what, report, e)
    elif e == "fused_ops.conv1x1_groupnorm_tokens_into":
        want = ref.conv1x1_groupnorm_tokens(a["x"], a["conv"], a["gn"])
        yard = ref.conv1x1_groupnorm_tokens(a["x"], a["conv"], a["gn"], torch.float32)
        fp32_bound(call.out, want, yard, "%s at row %d" % (what, a["row_offset"]), report, e)
    elif e == "fused_ops.groupnorm_flatten_into":
        want = ref.groupnorm_flatten(a["x"], a["gn"])
        yard = ref.groupnorm_flatten(a["x"], a["gn"], torch.float32)
        fp32_bound(call.out, want, yard, "%s at row %d" % (what, a["row_offset"]), report, e)
    elif e == "MSDA.ms_deform_attn_fused_forward":
        args = (a["value"], a["spatial_shapes"], a["reference_points"], a["sampling_offsets"], a["attention_logits"])
        fp32_bound(call.out, ref.msda_fused(*args), ref.msda_fused(*args, dtype=torch.float32), what, report, e,
                   abs_cap=1e-4)
    elif e == "MSDA.ms_deform_attn_forward":
        args = (a["value"], a["spatial_shapes"], a["sampling_loc"], a["attn_weight"])
        fp32_bound(call.out, ref.msda(*args), ref.msda(*args, dtype=torch.float32), what, report, e, abs_cap=1e-4)
    elif e == "fused_ops.masked_attention":
        v = a["v"] if a["v"] is not None else a["v_t"].permute(2, 0, 1)
        want = ref.attention(a["q"], a["k"], v, a["num_heads"], a["attn_mask"])
        yard = ref.attention_autocast(a["q"], a["k"], v, a["num_heads"], a["attn_mask"])
        bf16_bound(call.out, want, yard, what + (" (V^T)" if a["v"] is None else ""), report, e, rows_dim=-1)
    elif e == "fused_ops.cross_attention":
        q, k, m = ref.cross_operands(a["q_content"], a["q_pos"], a["k_content"], a["k_pos"], a["num_heads"],
                                     a["attn_mask"], a["row_open"])
        want = ref.attention(q, k, a["v"], a["num_heads"], m)
        yard = ref.attention_autocast(q, k, a["v"], a["num_heads"], m)
        bf16_bound(call.out, want, yard, "%s S=%d" % (what, k.shape[0]), report, e, rows_dim=-1)
    elif e == "dynamic_mask_head.dynamic_mask_head_forward":
        up, amask = call.out
        feats, stride, target = a["feats_f32"], a["stride"], a["target_size"]
        up64, rs64 = ref.mask_head(feats, a["ref_xy"], a["params"], stride, a["rel_coord"], target)
        what = "%s %dx%d -> %s" % (what, feats.shape[2], feats.shape[3], tuple(target))
        if a["out_dtype"] == torch.float32:
            up32, rs32 = ref.mask_head(feats, a["ref_xy"], a["params"], stride, a["rel_coord"], target, torch.float32)
            bound = fp32_bound(up, up64, up32, what, report, e)
            tol = max(bound, 2.0 * float((rs32.double() - rs64).abs().max()))
            rsy = rs32
        else:
            assert up.dtype == torch.bfloat16 and a["rel_coord"]
            upy, rsy = ref.mask_head_autocast(feats, a["ref_xy"], a["params"], stride, target)
            bound = bf16_bound(up, up64, upy, what, report, e)
            tol = max(bound, 2.0 * float((rsy.double() - rs64).abs().max()))
        mask_bits(amask, rs64, rsy.double(), tol, what)
    else:
        raise AssertionError("no reference for " + e)


def check_all(cap, family, report):
    """Check every recorded call.  `family`: the MSDeformAttn kernel family every MSDeformAttn call must have run
    (expected_msda_family), or a list of them, one per MSDeformAttn call in call order."""
    msda_calls = 0
    for e, calls in cap.calls.items():
        for c in calls:
            if c.kernel is not None:
                want = family if isinstance(family, int) else family[msda_calls]
                msda_calls += 1
                assert c.kernel == want, "%s ran kernel family %d, expected %d" % (e, c.kernel, want)
            check(c, report)
            del c.args, c.out                                   # free the copies as the check goes
    if not isinstance(family, int):
        assert msda_calls == len(family), (msda_calls, len(family))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the head
def build_head(depth, H, W, Q, levels, N, offsets, feature_seed=3):
    """MaskFormerHead of the shipped config at `levels` encoder levels and Q queries, seeded random init, on random
    ResNet-`depth` features of an H x W image batch of N.  `offsets` "M": bench.model_like_offsets (distribution M)."""
    from pctrans_amd.config import get_cfg, resnet_output_shape
    from pctrans_amd.meta_arch.mask_former_head import MaskFormerHead
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=Q, enc_in_features=("res2", "res3", "res4", "res5")[4 - levels:], norm="BN", sem_norm="BN")
    shapes = resnet_output_shape(depth)
    head = MaskFormerHead(**MaskFormerHead.from_config(cfg, shapes)).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(feature_seed)
    feats = {k: torch.randn(N, s.channels, H // s.stride, W // s.stride, device="cuda", generator=g)
             for k, s in shapes.items()}
    if offsets == "M":
        import bench
        bench.model_like_offsets(head, feats)
    return head, feats


def forward(head, feats, precision):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
        out, _ = head(feats)
    torch.cuda.synchronize()
    return out

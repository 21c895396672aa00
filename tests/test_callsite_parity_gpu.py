"""GPU: every HIP entry point of the head checked against float64 on the operands it actually received, at the BASELINE
head shapes and at the bench geometry (tests/callsite_capture.py records the calls, tests/callsite_reference.py defines
the operations).  Each call is compared on its own inputs, so a threshold decision that flips in one decoder layer cannot
cascade into the next one's comparison, and every element of every call is held to the bound (tests/callsite_check.py
holds the check):
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

import callsite_check as chk
from callsite_capture import CallsiteCapture

pytestmark = pytest.mark.gpu

K_DPP, K_COL = chk.K_DPP, chk.K_COL

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

_ZERO = dict.fromkeys(chk.ENTRIES, 0)


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


# ---------------------------------------------------------------- the head at the BASELINE shapes
def _head(name, offsets):
    depth, H, W, Q, levels, N = CONFIGS[name]
    return chk.build_head(depth, H, W, Q, levels, N, offsets)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("offsets", ["init", "M"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_head_kernel_call_matches_float64(monkeypatch, no_tf32, name, offsets, precision):
    head, feats = _head(name, offsets)
    cap = CallsiteCapture().install(monkeypatch)
    chk.forward(head, feats, precision)
    assert cap.counts() == _expected(name, precision)
    report = chk.Report("%s %s %s" % (name, offsets, precision))
    chk.check_all(cap, MSDA_FAMILY[name], report)
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
    chk.forward(head, feats, "bf16")
    del feats
    assert cap.counts() == _expected("bench", "bf16")
    for calls in cap.calls.values():
        for c in calls:
            assert c.images == [0, 63, 127], c
    report = chk.Report("bench b128 M bf16")
    chk.check_all(cap, MSDA_FAMILY["bench"], report)
    report.show()

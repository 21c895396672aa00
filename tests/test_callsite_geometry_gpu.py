"""GPU: every HIP entry point of the head checked against float64 at the call sites of a forward, at the geometries of
tests/callsite_check.py (GEOMETRIES): each sits next to one of the thresholds by which image size, batch and query count
move a call to another kernel, and the table puts every such rule on both sides.  Bounds and the per-call check are those
of test_callsite_parity_gpu.py (callsite_check.check_all).  Each geometry runs from random init in fp32 and under bf16
autocast; the four next to an MSDeformAttn kernel threshold also run with model-like sampling offsets (in fp32: the
encoder, where MSDeformAttn runs, is fp32 under autocast as well).  Every run must make exactly the calls
callsite_check.expected_calls states, every MSDeformAttn call must run expected_msda_family, every mask-head call must
produce the dtype of its expected kernel, and the decoder's cross-attention levels must go to cross_attention or to
masked_attention with V^T as cross_attention_split says.

Observed on the MI355X, largest error / yardstick-error over all geometries (run with -rP to print them per test):
bf16 masked_attention max 1.27 / mean 1.00, cross_attention 1.22 / 1.00, mask head 1.00 / 1.00; fp32 MSDeformAttn 1.12,
linear 1.00, linear_k128_multi 0.46, linear_add_layer_norm 1.13, ffn_layer_norm 0.67, conv1x1_groupnorm_tokens_into 1.51,
groupnorm_flatten_into 1.60, conv1x1_from_token_rows 0.94; conv1x1_nchw (3.54) and the fp32 mask head (2.67) exceed 2 only
where the 5e-6 x scale floor is the bound.  The 28 runs take about 16 s."""
import pytest
import torch

import callsite_check as chk
from callsite_capture import CallsiteCapture

pytestmark = pytest.mark.gpu

RUNS = [(name, "init", p) for name in chk.GEOMETRIES for p in ("fp32", "bf16")] + \
       [(name, "M", "fp32") for name in chk.MSDA_THRESHOLD_GEOMETRIES]


@pytest.fixture
def no_tf32(monkeypatch):
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)


def _check_routes(cap, g, precision):
    """The per-call side of the rules that the counts alone do not pin."""
    kernels = chk.mask_head_kernels(g.levels, g.H, g.W, g.N, precision)
    calls = cap.calls["dynamic_mask_head.dynamic_mask_head_forward"]
    assert len(calls) == len(kernels)
    for i, (c, k) in enumerate(zip(calls, kernels)):
        want = torch.float32 if k == "valu" else torch.bfloat16
        assert c.args["out_dtype"] == want and c.out[0].dtype == want, (i, k, c.args["out_dtype"])
    if precision == "bf16":
        keys = chk.decoder_keys(g.levels, g.H, g.W)
        split = [c.args["k_content"].shape[0] for c in cap.calls["fused_ops.cross_attention"]]
        v_t = [c.args["k"].shape[0] for c in cap.calls["fused_ops.masked_attention"] if c.args["v"] is None]
        assert split == [S for S in keys if chk.cross_attention_split(S)], split
        assert v_t == [S for S in keys if not chk.cross_attention_split(S)], v_t
        for c in cap.calls["fused_ops.masked_attention"]:
            if c.args["v"] is not None:                             # self-attention over the queries
                assert c.args["k"].shape[0] == g.Q


@pytest.mark.parametrize("name,offsets,precision", RUNS)
def test_every_head_kernel_call_matches_float64_across_geometries(monkeypatch, no_tf32, name, offsets, precision):
    g = chk.GEOMETRIES[name]
    head, feats = chk.build_head(g.depth, g.H, g.W, g.Q, g.levels, g.N, offsets)
    cap = CallsiteCapture(select=g.select).install(monkeypatch)
    chk.forward(head, feats, precision)
    del feats
    assert cap.counts() == chk.expected_calls(g.levels, g.H, g.W, g.N, g.Q, precision)
    if g.select is not None:
        kept = sorted(i % g.N for i in g.select)
        for calls in cap.calls.values():
            for c in calls:
                assert c.images == kept, c
    _check_routes(cap, g, precision)
    report = chk.Report("%s %s %s" % (name, offsets, precision))
    chk.check_all(cap, chk.expected_msda_family(g.levels, g.H, g.W, g.N), report)
    report.show()

"""GPU: the fused dynamic-mask-head kernel (through the C ABI) against the literal restatement of the reference's
formulation (materialised per-query inputs + grouped convs, mask2former_transformer_decoder.py:647-719) built from
torch ops in float64 on the host, at the reference's shapes: 128x128 / 64x64 feature maps, Q = 100 / 300, the three
attention-mask target sizes, non-square BBBC maps.  Tolerance 1e-4 absolute on O(1..10) logits in fp32 (north_star);
mask bits may differ only where the resized logit is within 1e-4 of the threshold."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from test_head_cpu import _reference_formulation, _small_decoder

pytestmark = pytest.mark.gpu


def _case(N, Q, H, W, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    mf = torch.randn(N, 16, H, W, generator=g, dtype=torch.float64)
    ref = torch.rand(Q, N, 2, generator=g, dtype=torch.float64)
    prm = torch.randn(Q, N, 233, generator=g, dtype=torch.float64) * scale
    w0 = prm[..., :144].view(Q, N, 8, 18)
    w0[..., :2] *= 0.02           # rel-coord weights see inputs up to +-512
    return mf, ref, prm


@pytest.mark.parametrize("N,Q,H,W,target", [
    (2, 100, 128, 128, (16, 16)), (2, 100, 128, 128, (32, 32)), (1, 100, 128, 128, (64, 64)),
    (2, 300, 65, 87, (17, 22)), (1, 50, 32, 32, (8, 8)), (3, 7, 9, 6, (5, 4)), (1, 10, 200, 128, (25, 16)),
])
def test_fused_mask_head_fp32(N, Q, H, W, target):
    from pctrans_amd import dynamic_mask_head as dmh
    d = _small_decoder(Q=Q).double()
    mf, ref, prm = _case(N, Q, H, W, seed=N * 1000 + Q)
    want = _reference_formulation(d, mf, ref, prm)                                   # [N, Q, H, W] float64
    want_up = F.interpolate(want, size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
    want_rs = F.interpolate(want, size=target, mode="bilinear", align_corners=False).flatten(2)
    up, amask = dmh.dynamic_mask_head_forward(mf.float().cuda(), ref.transpose(0, 1).float().cuda(),
                                              prm.transpose(0, 1).float().cuda(), 4, True, target)
    assert up.shape == (N, Q, 2 * H, 2 * W) and up.dtype == torch.float32
    scale = max(1.0, float(want_up.abs().max()))
    err = float((up.cpu().double() - want_up).abs().max())
    assert err <= 1e-4 * scale, (err, scale)
    got_m = amask.cpu()
    want_m = want_rs.sigmoid() < 0.5
    differ = got_m != want_m
    assert float(want_rs[differ].abs().max() if differ.any() else 0.0) < 1e-4 * scale
    assert differ.float().mean() < 1e-3


def _bf16_chain_reference(mf, ref, prm, stride=4):
    """The autocast pipeline the bf16 kernels implement, from torch ops: features / generated weights / hidden
    activations rounded to bf16 (what bf16 convolutions see), fp32 accumulation, rel-coord term and biases in fp32."""
    N, C, H, W = mf.shape
    Q = ref.shape[0]
    r = lambda t: t.bfloat16().float()
    p = prm.transpose(0, 1).float()                                       # [N, Q, 233]
    w0 = p[..., :144].reshape(N, Q, 8, 18)
    w1, w2 = p[..., 144:208].reshape(N, Q, 8, 8), p[..., 208:216].reshape(N, Q, 1, 8)
    b0, b1, b2 = p[..., 216:224], p[..., 224:232], p[..., 232:233]
    f = r(mf.float()).reshape(N, 1, C, H * W)
    inst = ref.transpose(0, 1).float() * torch.tensor([W * stride, H * stride], dtype=torch.float32, device=mf.device)
    ys, xs = torch.meshgrid(torch.arange(H, device=mf.device), torch.arange(W, device=mf.device), indexing="ij")
    loc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).float() * stride + stride // 2
    rel = inst[:, :, None, :] - loc[None, None]                           # [N, Q, HW, 2]
    x = r(w0[..., 2:]) @ f + w0[..., 0:1] * rel[:, :, None, :, 0] + w0[..., 1:2] * rel[:, :, None, :, 1] + b0[..., None]
    x = r(torch.relu(x))
    x = torch.relu(r(w1) @ x + b1[..., None])
    return ((w2 @ x) + b2[..., None]).reshape(N, Q, H, W)


@pytest.mark.parametrize("kernel", ["mfma", "valu"])
@pytest.mark.parametrize("N,Q,H,W,target", [(2, 100, 64, 64, (16, 16)), (1, 101, 128, 128, (64, 64)),
                                            (2, 7, 33, 20, (9, 5))])
def test_fused_mask_head_bf16_output_matches_autocast_semantics(monkeypatch, kernel, N, Q, H, W, target):
    """bf16 mode: MFMA kernels (bf16 operands, default) and the fp32-VALU kernel (logits rounded to bf16 afterwards)
    against the torch emulation of the autocast pipeline; resized with fp32 math, stored as bf16."""
    from pctrans_amd import dynamic_mask_head as dmh
    monkeypatch.setenv("PCT_DMH_KERNEL", kernel)
    mf, ref, prm = _case(N, Q, H, W, seed=5)
    mf, ref, prm = mf.float().cuda(), ref.float().cuda(), prm.float().cuda()
    want = _bf16_chain_reference(mf, ref, prm)
    up, amask = dmh.dynamic_mask_head_forward(mf, ref.transpose(0, 1), prm.transpose(0, 1), 4, True, target,
                                              out_dtype=torch.bfloat16)
    assert up.dtype == torch.bfloat16 and up.shape == (N, Q, 2 * H, 2 * W)
    lb = want.bfloat16()
    want_up = F.interpolate(lb, size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
    # hidden activations near a bf16 rounding boundary may round differently: a few bf16 ulps on a small fraction
    diff = (up.float() - want_up.float()).abs()
    tol = want_up.float().abs() * 2.0 ** -6 + 3e-2
    assert (diff <= tol).float().mean() > 0.995, float((diff <= tol).float().mean())
    want_m = F.interpolate(lb, size=target, mode="bilinear", align_corners=False).sigmoid().flatten(2) < 0.5
    assert (amask != want_m).float().mean() < 1e-2


def test_decoder_uses_fused_kernel_and_matches_batched_formulation():
    """End to end inside the decoder: eval forward on the GPU (fused kernel) == the differentiable batched torch
    formulation run on the same device (grad enabled -> torch path)."""
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    torch.manual_seed(0)
    d = dec.MultiScaleMaskedTransformerDecoder(
        128, True, hidden_dim=128, num_queries=20, nheads=8, dim_feedforward=256, dec_layers=3, pre_norm=False,
        mask_dim=16, enforce_input_project=False, points_num=1, sem_loss_on=True, norm="BN", rel_coord=True
    ).cuda().eval()
    mf = torch.randn(2, 16, 32, 40, device="cuda")
    ref = torch.rand(20, 2, 2, device="cuda")
    prm = torch.randn(20, 2, 233, device="cuda") * 0.2
    with torch.no_grad():
        up_f, m_f = d.dynamic_mask_with_coords(mf, ref, prm, 4, True, (8, 10))
    up_t, m_t = d.dynamic_mask_with_coords(mf, ref, prm.requires_grad_(), 4, True, (8, 10))
    assert m_f.shape == m_t.shape == (2, 1, 20, 80)
    assert float((up_f - up_t).abs().max()) <= 1e-4 * max(1.0, float(up_t.abs().max()))
    assert (m_f != m_t).float().mean() < 1e-3


def test_resize_kernel_exact_x2_path_is_bitwise_torch_bf16_interpolate():
    """The streaming resize kernel on its own (through the MFMA entry point with an identity-like setup is not possible,
    so compare end to end): for even widths the x2 fast path must reproduce torch's bf16 bilinear upsample of the
    bf16 logits exactly wherever the logits themselves agree bit for bit."""
    from pctrans_amd import dynamic_mask_head as dmh
    N, Q, H, W = 1, 6, 40, 36
    mf, ref, prm = _case(N, Q, H, W, seed=9)
    mf, ref, prm = mf.float().cuda(), ref.float().cuda(), prm.float().cuda()
    up, _ = dmh.dynamic_mask_head_forward(mf, ref.transpose(0, 1), prm.transpose(0, 1), 4, True, (10, 9),
                                          out_dtype=torch.bfloat16)
    # the bit-for-bit check of this path, borders and seams included, is tests/test_dmh_exact_gpu.py (geometry 40 x 36)
    want =F.interpolate(_bf16_chain_reference(mf, ref, prm).bfloat16(), size=(2 * H, 2 * W), mode="bilinear",
                         align_corners=False)
    close = ((up.float() - want.float()).abs() <= want.float().abs() * 2.0 ** -6 + 3e-2).float().mean()
    assert float(close) > 0.995
    # borders use lambda = 0 / replicated indices: corners must equal their source logit's neighbourhood mix, finite
    assert torch.isfinite(up.float()).all()


@pytest.mark.parametrize("tag", ["rel", "norel", "rel_up"])
def test_fused_mask_head_kernel_matches_the_reference_method_fixture(golden, tag):
    """The HIP kernel (through the C ABI) against vectors produced by the reference's own dynamic_mask_with_coords /
    mask_heads_forward / parse_dynamic_params (tests/golden/make_golden_decoder.py)."""
    import numpy as np
    from pctrans_amd import dynamic_mask_head as dmh
    g = golden("dec_dynamic_mask_head_" + tag)
    feats = torch.from_numpy(g["feats"]).cuda()
    ref_xy = torch.from_numpy(g["refpts"]).transpose(0, 1).contiguous().cuda()         # [N, Q, 2]
    params = torch.from_numpy(g["params"]).transpose(0, 1).contiguous().cuda()         # [N, Q, G]
    rel, stride, tgt, heads = bool(g["rel_coord"]), int(g["stride"]), tuple(int(v) for v in g["target"]), int(g["heads"])
    up, amask = dmh.dynamic_mask_head_forward(feats, ref_xy, params, stride, rel, tgt)
    scale = max(1.0, float(np.abs(g["logits_x2"]).max()))
    np.testing.assert_allclose(up.cpu().numpy(), g["logits_x2"], rtol=0, atol=1e-4 * scale)
    N, Q = feats.shape[0], ref_xy.shape[1]
    want = g["attn_mask"].reshape(N, heads, Q, -1)[:, 0]
    assert (amask.cpu().numpy() != want).mean() < 1e-3            # logits at the sigmoid threshold may fall either side

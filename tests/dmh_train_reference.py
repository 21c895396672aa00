"""Float64 restatement, in plain torch without autograd, of the backward of the dynamic mask head (what
pctrans_amd/csrc/dyn_mask_head_bwd.hip computes), plus the helpers the training-path tests share: the input recipe, the
ReLU-gate ambiguity set, and the autograd yardstick on the module's own formulation.  test_dmh_train_cpu.py pins
`backward64` against torch.autograd.grad of that formulation in float64; the GPU bounds are taken against `backward64`."""
import torch
from torch.nn import functional as F


def case(N, Q, H, W, seed, scale=0.3, rel_coord=True):
    """Inputs as test_dyn_mask_head_gpu._case, [N, Q, ...] layout, float64, plus grad_up ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    cin = 18 if rel_coord else 16
    G = cin * 8 + 64 + 8 + 8 + 8 + 1
    mf = torch.randn(N, 16, H, W, generator=g, dtype=torch.float64)
    ref = torch.rand(Q, N, 2, generator=g, dtype=torch.float64)
    prm = torch.randn(Q, N, G, generator=g, dtype=torch.float64) * scale
    if rel_coord:
        prm[..., :144].view(Q, N, 8, 18)[..., :2] *= 0.02          # rel-coord weights see inputs up to +-512
    gup = torch.randn(N, Q, 2 * H, 2 * W, generator=g, dtype=torch.float64)
    return mf, ref.transpose(0, 1).contiguous(), prm.transpose(0, 1).contiguous(), gup


def upsample_matrix(n, dtype=torch.float64, device="cpu"):
    """[2n, n]: torch's upsample_bilinear2d along one axis, scale 2, align_corners = False (src = (o + 0.5) / 2 - 0.5
    clamped at 0, second tap clamped at the last element)."""
    U = torch.zeros(2 * n, n, dtype=dtype, device=device)
    for o in range(2 * n):
        src = max(0.5 * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(src), n - 1)
        i1 = i0 + (1 if i0 < n - 1 else 0)
        lam = src - i0
        U[o, i0] += 1.0 - lam
        U[o, i1] += lam
    return U


def _split(prm, rel_coord):
    N, Q, _ = prm.shape
    cin = 18 if rel_coord else 16
    w0, w1, w2, b0, b1, b2 = torch.split_with_sizes(prm, [cin * 8, 64, 8, 8, 8, 1], dim=2)
    return w0.reshape(N, Q, 8, cin), w1.reshape(N, Q, 8, 8), w2, b0, b1, b2


def _inputs(mf, ref, stride, rel_coord):
    """in [N, Q or 1, cin, HW]: rel_x, rel_y (ref * (W, H) * stride - pixel centre), then the 16 features."""
    N, C, H, W = mf.shape
    feats = mf.reshape(N, 1, C, H * W)
    if not rel_coord:
        return feats
    Q = ref.shape[1]
    ys, xs = torch.meshgrid(torch.arange(H, device=mf.device), torch.arange(W, device=mf.device), indexing="ij")
    cx = (xs.reshape(-1) * stride + stride // 2).to(mf.dtype)
    cy = (ys.reshape(-1) * stride + stride // 2).to(mf.dtype)
    relx = ref[..., 0:1] * (W * stride) - cx                      # [N, Q, HW]
    rely = ref[..., 1:2] * (H * stride) - cy
    return torch.cat((relx[:, :, None], rely[:, :, None], feats.expand(N, Q, C, H * W)), dim=2)


def backward64(mf, ref, prm, gup, stride=4, rel_coord=True, chunk=64):
    """mf [N,16,H,W], ref [N,Q,2], prm [N,Q,G], gup [N,Q,2H,2W] (any float dtype; computed in float64)
    -> grad_feat [N,16,H,W], grad_ref [N,Q,2] (zeros without rel_coord), grad_params [N,Q,G]."""
    mf, ref, prm, gup = (t.double() for t in (mf, ref, prm, gup))
    N, C, H, W = mf.shape
    Q = prm.shape[1]
    Uy, Ux = upsample_matrix(H, device=mf.device), upsample_matrix(W, device=mf.device)
    grad_feat = torch.zeros_like(mf).reshape(N, C, H * W)
    grad_ref = torch.zeros(N, Q, 2, dtype=torch.float64, device=mf.device)
    gp = []
    for q0 in range(0, Q, chunk):
        sl = slice(q0, min(q0 + chunk, Q))
        w0, w1, w2, b0, b1, b2 = _split(prm[:, sl], rel_coord)
        inp = _inputs(mf, ref[:, sl], stride, rel_coord)                             # [N, q, cin, HW]
        g = torch.einsum("oy,nqop,px->nqyx", Uy, gup[:, sl], Ux).reshape(N, -1, 1, H * W)
        a0 = torch.matmul(w0, inp) + b0[..., None]
        x0 = a0.clamp(min=0)
        a1 = torch.matmul(w1, x0) + b1[..., None]
        x1 = a1.clamp(min=0)
        db2 = g.sum(-1)                                                              # [N, q, 1]
        dw2 = (g * x1).sum(-1)
        dx1 = g * w2[..., None] * (a1 > 0)
        db1 = dx1.sum(-1)
        dW1 = torch.matmul(dx1, x0.transpose(-1, -2))
        dx0 = torch.matmul(w1.transpose(-1, -2), dx1) * (a0 > 0)
        db0 = dx0.sum(-1)
        dW0 = torch.matmul(dx0, inp.expand(N, dx0.shape[1], inp.shape[2], H * W).transpose(-1, -2))
        off = 2 if rel_coord else 0
        grad_feat += torch.matmul(w0[..., off:].transpose(-1, -2), dx0).sum(1)
        if rel_coord:
            scale = torch.tensor([W * stride, H * stride], dtype=torch.float64, device=mf.device)
            grad_ref[:, sl] = scale * (w0[..., 0:2] * db0[..., None]).sum(2)
        gp.append(torch.cat((dW0.flatten(2), dW1.flatten(2), dw2, db0, db1, db2), dim=2))
    return grad_feat.reshape(N, C, H, W), grad_ref, torch.cat(gp, dim=1)


def ambiguous_pixels(mf, ref, prm, stride=4, rel_coord=True, chunk=64):
    """bool [N, Q, H, W]: a ReLU pre-activation of the pixel is zero to rounding -- some unit has
    |a| < 64 * 2^-24 * (sum |w * in| + |b|), for layer 1 plus the largest such sum of layer 0 -- so its one-sided
    derivative cannot be pinned by any fp32 evaluation."""
    mf, ref, prm = (t.double() for t in (mf, ref, prm))
    N, C, H, W = mf.shape
    eps = 64.0 * 2.0 ** -24
    out = []
    for q0 in range(0, prm.shape[1], chunk):
        sl = slice(q0, min(q0 + chunk, prm.shape[1]))
        w0, w1, w2, b0, b1, b2 = _split(prm[:, sl], rel_coord)
        inp = _inputs(mf, ref[:, sl], stride, rel_coord)
        a0 = torch.matmul(w0, inp) + b0[..., None]
        s0 = torch.matmul(w0.abs(), inp.abs()) + b0.abs()[..., None]
        x0 = a0.clamp(min=0)
        a1 = torch.matmul(w1, x0) + b1[..., None]
        s1 = torch.matmul(w1.abs(), x0) + b1.abs()[..., None] + s0.max(dim=2, keepdim=True).values
        amb = (a0.abs() < eps * s0).any(2) | (a1.abs() < eps * s1).any(2)
        out.append(amb.reshape(N, -1, H, W))
    return torch.cat(out, dim=1)


def mask_grad_up(gup, amb):
    """grad_up with zeros on every output pixel that draws (with a non-zero weight) from an ambiguous pixel."""
    N, Q, H, W = amb.shape
    Sy = (upsample_matrix(H, device=amb.device) > 0).double()
    Sx = (upsample_matrix(W, device=amb.device) > 0).double()
    hit = torch.einsum("oy,nqyx,px->nqop", Sy, amb.double(), Sx) > 0
    return gup.masked_fill(hit, 0.0)


def autograd_formulation(decoder, mf, ref, prm, gup, stride=4, rel_coord=True):
    """The module's differentiable formulation (mask_heads_forward_batched + F.interpolate) under torch.autograd.grad, in the
    dtype of the operands -> (grad_feat, grad_ref, grad_params)."""
    mf, ref, prm = (t.detach().clone().requires_grad_(True) for t in (mf, ref, prm))
    N, C, H, W = mf.shape
    logits = decoder.mask_heads_forward_batched(mf, ref, prm, stride, rel_coord)
    up = F.interpolate(logits, size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
    wanted = (mf, ref, prm) if rel_coord else (mf, prm)
    grads = torch.autograd.grad((up * gup).sum(), wanted)
    if rel_coord:
        return grads
    return grads[0], torch.zeros_like(ref), grads[1]

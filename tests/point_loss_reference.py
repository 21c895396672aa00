"""Float64 reference of the point-sampled mask losses (pctrans_amd/point_loss.py): F.grid_sample in float64 on the CPU plus the
criterion's own sigmoid_ce_loss and dice_loss formulas, gradients from autograd.  Inputs are the fp32 tensors the kernels get,
cast to float64 exactly; nothing here depends on the code under test.  Also the error bounds the GPU tests hold the kernels to,
each derived from the kernel's arithmetic (u = 2^-24, the unit roundoff of fp32)."""
import torch
import torch.nn.functional as F

from pctrans_amd.loss.maskformer_criterion import dice_loss, sigmoid_ce_loss

U = 2.0 ** -24


def _d(t):
    return t.detach().cpu().double()


def sample64(planes, plane_index, coords, planes_per_coord_row=1):
    """[K, P] float64: plane plane_index[k] (None: k) of planes [n, H, W] at coords[k // planes_per_coord_row]."""
    planes, coords = (p if p.dtype == torch.float64 and not p.is_cuda else _d(p) for p in (planes, coords))
    K = planes.shape[0] if plane_index is None else len(plane_index)
    if K == 0:
        return planes.new_zeros((0, coords.shape[1]))
    picked = planes if plane_index is None else planes[torch.as_tensor(plane_index).cpu().long()]
    rows = torch.arange(K) // planes_per_coord_row
    grid = 2.0 * coords[rows][:, :, None, :] - 1.0
    return F.grid_sample(picked[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0, :, 0]


def sums64(x, t):
    """[K, 4] float64: sum_p bce_with_logits(x, t), sigma(x) t, sigma(x), t."""
    x, t = _d(x), _d(t)
    s = x.sigmoid()
    return torch.stack([F.binary_cross_entropy_with_logits(x, t, reduction="none").sum(1), (s * t).sum(1), s.sum(1), t.sum(1)], 1)


def losses64(pred, src_index, tgt, tgt_index, coords, num_masks):
    """-> (loss_mask, loss_dice, grad of (g_m loss_mask + g_d loss_dice) w.r.t. pred as a function of (g_m, g_d)).
    pred [B, Q, H, W] (any float dtype), indices into its / tgt's flattened planes."""
    pred64 = _d(pred).requires_grad_(True)
    x = sample64(pred64.flatten(0, 1), src_index, _d(coords))
    t = sample64(_d(tgt), tgt_index, _d(coords))
    lm, ld = sigmoid_ce_loss(x, t, num_masks), dice_loss(x, t, num_masks)

    def grad(g_m=1.0, g_d=1.0):
        return torch.autograd.grad(g_m * lm + g_d * ld, pred64, retain_graph=True)[0]
    return lm.detach(), ld.detach(), grad


def grad_x_closed_form(x, t, alpha, beta, gamma):
    """The backward kernel's formula in float64: alpha (sigma - t) + sigma (1 - sigma) (beta - gamma t), coefficients [K]."""
    x, t = _d(x), _d(t)
    a, b, g = (_d(c)[:, None] for c in (alpha, beta, gamma))
    s = x.sigmoid()
    return a * (s - t) + s * (1 - s) * (b - g * t)


def coefficients64(sums, P, num_masks, g_m=1.0, g_d=1.0):
    """alpha, beta, gamma [K] float64 of the two losses' gradient (include/pctrans_hip_train.h)."""
    sums = _d(sums)
    num, den = 2 * sums[:, 1] + 1, sums[:, 2] + sums[:, 3] + 1
    return (torch.full_like(num, g_m / (P * num_masks)), g_d * num / (den * den) / num_masks, 2 * g_d / den / num_masks)


def scatter64(grad_x, coords, H, W):
    """[K, H, W] float64: grad_x [K, P] scattered to the four taps of each point (autograd of grid_sample); and the number of
    taps that land on each pixel, [K, H, W]."""
    grad_x, coords = _d(grad_x), _d(coords)
    K = grad_x.shape[0]
    planes = torch.zeros(K, H, W, dtype=torch.float64, requires_grad=True)
    (sample64(planes, None, coords) * grad_x).sum().backward()
    x = coords[..., 0] * W - 0.5
    y = coords[..., 1] * H - 0.5
    x0, y0 = x.floor().long(), y.floor().long()
    count = torch.zeros(K, H + 2, W + 2, dtype=torch.float64)
    k = torch.arange(K)[:, None].expand_as(x0)
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = (y0 + dy).clamp(-1, H) + 1, (x0 + dx).clamp(-1, W) + 1
            count.index_put_((k, yy, xx), torch.ones_like(x), accumulate=True)
    # a position within u W of a pixel boundary may floor to the other side in fp32 and touch the next pixel with a weight of
    # that size: a pixel's bound counts the taps on its 3 x 3 neighbourhood
    near = F.avg_pool2d(count[:, None], 3, stride=1, padding=1, divisor_override=1)[:, 0]
    return planes.grad, near[:, 1:-1, 1:-1]


def flip_candidates(logits64, num_uncertain, e_s):
    """How many of the oversampled candidates [K, S] could enter or leave the num_uncertain most uncertain (smallest |logit|)
    when every logit moves by up to e_s: the selected ones within 2 e_s of the first one left out, and the left-out ones
    within 2 e_s of the last one selected."""
    unc = -logits64.abs()
    top = torch.sort(unc, dim=1, descending=True)[0]
    if num_uncertain == 0 or num_uncertain >= unc.shape[1]:
        return 0
    kth, nxt = top[:, num_uncertain - 1:num_uncertain], top[:, num_uncertain:num_uncertain + 1]
    selected = unc >= kth
    return int(((selected & (unc - nxt <= 2 * e_s)) | (~selected & (kth - unc <= 2 * e_s))).sum())


def module_case(seed=5, device="cpu"):
    """A small criterion problem: 2 images x 6 queries at 40 x 24, 3 targets each at 80 x 48 (another resolution), 70 points
    from 210 candidates.  -> (pred [2, 6, 40, 24] fp32, targets, indices)."""
    g = torch.Generator().manual_seed(seed)
    pred = (torch.randn(2, 6, 40, 24, generator=g) * 3).to(device)
    targets = [{"masks": (torch.rand(3, 80, 48, generator=g) > 0.5).float().to(device),
                "labels": torch.ones(3, dtype=torch.long, device=device)} for _ in range(2)]
    indices = [(torch.tensor([4, 0, 3]), torch.tensor([2, 0, 1])), (torch.tensor([1, 5, 2]), torch.tensor([0, 2, 1]))]
    return pred, targets, indices


# ---- bounds --------------------------------------------------------------------------------------------------------------
def sample_bound(vmax, H, W):
    """|fp32 sample - float64 sample| for plane values up to vmax in magnitude.  x = fma(c, W, -0.5) is off by at most
    u W (half an ulp of a number below W), y by u H; the sample is piecewise linear in x and y with slopes of at most 2 vmax
    (two neighbouring values, or a value and the zero outside), so the positions cost 2 vmax u (W + H).  The weights: tx =
    x - floor(x) is exact or one rounding, 1 - tx one rounding, each product one, each weight within 4 u; four weight-value
    products and three additions of terms whose magnitudes sum to at most vmax: 4 u + 4 u + 3 u of vmax.  Rounded up to 16."""
    return vmax * U * (2 * (W + H) + 16)


def term_bounds(x, t, e_x, e_t):
    """Per-point bounds [K, P] on the four summands evaluated in fp32 from samples within e_x, e_t of the true ones.  bce is
    1-Lipschitz in x and |x|-Lipschitz in t; sigma is 1/4-Lipschitz; expf, log1pf and the division are good to 2 ulp each
    and the few additions and products add one u each: 8 u of the magnitudes involved."""
    x, t = _d(x), _d(t)
    s = x.sigmoid()
    mag = x.clamp(min=0) + (x * t).abs() + F.softplus(-x.abs())
    bce = e_x * (1 + t.abs()) + e_t * x.abs() + 8 * U * mag
    sg = e_x / 4 + 8 * U * s
    return torch.stack([bce, sg * t.abs() + e_t * s + 8 * U * s * t.abs(), sg, torch.full_like(x, e_t)], 2)


def sums_bound(x, t, e_x, e_t):
    """[K, 4]: the per-point bounds summed, plus the P fp32 additions: each partial sum is rounded once, at most P roundings
    of a sum no larger than the sum of the magnitudes (the kernel's tree has fewer; P is the bound the order cannot beat)."""
    x, t = _d(x), _d(t)
    P = x.shape[1]
    mags = sums64(x, t).abs()
    mags[:, 0] = (x.clamp(min=0) + (x * t).abs() + F.softplus(-x.abs())).sum(1)
    mags[:, 3] = t.abs().sum(1)
    return term_bounds(x, t, e_x, e_t).sum(1) + P * U * mags


def grad_planes_bound(count, alpha, beta, gamma, H, W):
    """[K, H, W]: a pixel that receives n taps, each |w grad_x| <= bound_k = |alpha| + (|beta| + |gamma|) / 4.  grad_x from
    given x, t in fp32: 8 u bound_k (as above); the weight w within u (W + H) + 4 u of the float64 one (position, then the
    products); the product one more u; the fixed-point quantum bound_k 2^-30 per contribution (the header's statement); the
    final conversion one u of a sum no larger than n bound_k.  Where the scale's exponent is clamped (bound_k below 2^-96) the
    half quantum is 2^-127 instead, and an fp32 product that small is subnormal, rounded to a multiple of 2^-149: 2^-126 per
    contribution covers both."""
    b = (_d(alpha).abs() + (_d(beta).abs() + _d(gamma).abs()) / 4)[:, None, None]
    return count * (b * (U * (W + H + 4 + 8 + 1 + 1) + 2.0 ** -30) + 2.0 ** -126)

"""Float64 reference of the matcher's cost matrices (pctrans_amd/point_loss.py: match_costs, pct_point_match_cost_f32) and the
bounds the GPU tests hold the kernel to.  The reference is point_loss_reference.sample64 for both sample sets and the formulas
of matcher.batch_sigmoid_ce_loss / batch_dice_loss in float64; nothing here depends on the code under test.

Bounds, from the kernel's arithmetic (csrc/point_loss.hip), u = 2^-24:

* per factor.  e = expf(-|x|) and log1pf(e) are good to 2 ulp each, and an error of e moves log1p(e) by at most that error,
  e <= log1p(e) / ln 2: log1p(e) within (2 + 2.9 + 1) u, the addition of max(-+x, 0) one more: softplus(-+x) within 8 u of
  itself (both summands are non-negative, relative errors do not grow).  sigma = 1 / (1 + e) or e / (1 + e): 2 u for e, one
  addition, one division, one product: within 8 u as well.  1 - t is one rounding.  FACTOR = 8 + 1 covers a product's factors.
* summation.  A (q, g) accumulator of the cross-entropy receives two products per point (softplus(-x) t, then
  softplus(x) (1 - t)) over the L = 128 * passes points of its chunk, each product rounded at most once and each addition once;
  the `chunks` partial sums are then added in ascending order.  Every term is non-negative, so the error is at most
  (2 L + chunks + 1) u times the sum itself.  sigma t: one product per point, (L + chunks + 1) u.  sum sigma and sum t: a lane adds
  every second point, L / 2 additions, one addition joins the two halves, then the chunks: (L / 2 + chunks + 1) u.
  L and chunks follow from the split stated in include/pctrans_hip_train.h (`plan`).
* a product whose value is below 2^-120 may lose its subnormal part in fp32 (flushed, or rounded to a multiple of 2^-149):
  2^-126 for each such product, nothing for the others (`tiny`).
* the quotients.  ce = sum / P: one rounding.  dice = 1 - N / D, N = 2 st + 1, D = sg + t + 1: N within e_N = 2 e_st + 2 u N,
  D within e_D = e_sg + e_t + 2 u D, the quotient within e_N / D' + N e_D / (D D') + u N / D with D' = D - e_D, the subtraction
  one rounding of a number of at most 1 + N / D.  cost = cost_mask ce + cost_dice dice: two products and an addition, 3 u of the
  magnitudes.
* sampling (end to end).  The samples are within e_x, e_t (point_loss_reference.sample_bound) of the float64 ones.
  softplus(-x) moves by at most e_x sigma(-x + e_x) (its slope, largest at the near end), softplus(x) by e_x sigma(x + e_x),
  sigma by e_x / 4, t and 1 - t by e_t.
The cross-entropy bound is relative to the non-negative sum  sum pos t + sum neg (1 - t); sum |x| does not enter."""
import torch
import torch.nn.functional as F

import point_loss_reference as R

U = R.U
FACTOR = 9
TINY = 2.0 ** -120
FLUSH = 2.0 ** -126


def plan(B, Q, Gmax, P):
    """-> (points per chunk, chunks): the split of include/pctrans_hip_train.h."""
    qg, gg = -(-Q // 128), -(-Gmax // 64)
    subs = -(-P // 128)
    want = max(1, min(32, subs, -(-512 // (B * qg * gg))))
    passes = -(-subs // want)
    return 128 * passes, -(-subs // passes)


def samples64(pred, tgt, counts, coords):
    """x [B, Q, P], t [B, Gmax, P] float64 (zero rows past an image's count): pred [B, Q, H, W], tgt [sum G, Ht, Wt]."""
    B, Q = pred.shape[:2]
    gmax = max(counts)
    x = R.sample64(pred.flatten(0, 1), None, coords, Q).view(B, Q, -1)
    t = torch.zeros(B, gmax, coords.shape[1], dtype=torch.float64)
    at = 0
    for b, g in enumerate(counts):
        if g:
            t[b, :g] = R.sample64(tgt[at:at + g], None, coords[b:b + 1], g)
        at += g
    return x, t


def parts64(x, t):
    """The five sums from samples x [B, Q, P], t [B, G, P] (any dtype, cast exactly): ce_sum [B, Q, G] = sum pos t + sum neg (1 - t),
    st [B, Q, G], sg [B, Q], tt [B, G], and the number of tiny products per (q, g)."""
    x, t = x.detach().cpu().double(), t.detach().cpu().double()
    pos, neg, s = F.softplus(-x), F.softplus(x), x.sigmoid()
    a, b = torch.einsum("bnc,bmc->bnm", pos, t), torch.einsum("bnc,bmc->bnm", neg, 1 - t)
    tiny = torch.zeros_like(a)
    for lhs, rhs in ((pos, t), (neg, 1 - t), (s, t)):
        for q0 in range(0, x.shape[1], 32):                                  # counted exactly, 32 queries at a time
            prod = (lhs[:, q0:q0 + 32, None, :] * rhs[:, None, :, :]).abs()
            tiny[:, q0:q0 + 32] += ((prod > 0) & (prod < TINY)).sum(-1)
    return a + b, torch.einsum("bnc,bmc->bnm", s, t), s.sum(-1), t.sum(-1), tiny


def cost_from_parts(ce_sum, st, sg, tt, P, cost_mask, cost_dice, counts):
    ce = ce_sum / P
    dice = 1 - (2 * st + 1) / (sg[:, :, None] + tt[:, None, :] + 1)
    C = cost_mask * ce + cost_dice * dice
    for b, g in enumerate(counts):
        C[b, :, g:] = 0
    return C, ce, dice


def cost64(pred, tgt, counts, coords, cost_mask, cost_dice):
    """-> cost [B, Q, Gmax] float64 as Point_HungarianMatcher._batched_costs forms it, zero past an image's count."""
    x, t = samples64(pred, tgt, counts, coords)
    ce_sum, st, sg, tt, _ = parts64(x, t)
    return cost_from_parts(ce_sum, st, sg, tt, coords.shape[1], cost_mask, cost_dice, counts)[0]


def cost_bound(x, t, counts, cost_mask, cost_dice, e_x=0.0, e_t=0.0, B=None):
    """[B, Q, Gmax] float64: the bound on |kernel cost - float64 cost from the samples x, t| when the kernel's fp32 samples are
    within e_x, e_t of x, t (0, 0: the kernel's own samples, the contraction alone)."""
    x, t = x.detach().cpu().double(), t.detach().cpu().double()
    nb, Q, P = x.shape
    G = t.shape[1]
    L, chunks = plan(nb if B is None else B, Q, G, P)
    ce_sum, st, sg, tt, tiny = parts64(x, t)
    pos, neg, s = F.softplus(-x), F.softplus(x), x.sigmoid()
    # sampling: the slopes at the near end of the interval, the factors at the far end
    d_pos, d_neg = e_x * torch.sigmoid(-x + e_x), e_x * torch.sigmoid(x + e_x)
    one_t = (1 - t).abs()
    e_ce = (torch.einsum("bnc,bmc->bnm", d_pos, t.abs() + e_t) + torch.einsum("bnc,bmc->bnm", d_neg, one_t + e_t)
            + e_t * (pos.sum(-1) + neg.sum(-1))[:, :, None])
    e_st = torch.einsum("bnc,bmc->bnm", torch.full_like(x, e_x / 4), t.abs() + e_t) + e_t * s.sum(-1)[:, :, None]
    e_sg = torch.full_like(sg, P * e_x / 4)
    e_tt = torch.full_like(tt, P * e_t)
    # arithmetic, relative to the sums (grown by what sampling may add to them)
    e_ce = e_ce + (2 * L + chunks + 1 + FACTOR) * U * (ce_sum + e_ce) + FLUSH * tiny
    e_st = e_st + (L + chunks + 1 + FACTOR) * U * (st + e_st) + FLUSH * tiny
    e_sg = e_sg + (L // 2 + chunks + 1 + FACTOR) * U * (sg + e_sg)
    e_tt = e_tt + (L // 2 + chunks + 1) * U * (tt.abs() + e_tt)
    ce = ce_sum / P
    e_c = e_ce / P + U * ce + FLUSH * (ce < TINY)
    N, D = 2 * st + 1, sg[:, :, None] + tt[:, None, :] + 1
    e_N = 2 * e_st + 2 * U * N
    e_D = e_sg[:, :, None] + e_tt[:, None, :] + 2 * U * D
    Dl = (D - e_D).clamp(min=1e-300)
    e_dice = e_N / Dl + N * e_D / (D * Dl) + U * N / D + U * (1 + N / D)
    dice = 1 - N / D
    bound = abs(cost_mask) * e_c + abs(cost_dice) * e_dice + 3 * U * (abs(cost_mask) * ce + abs(cost_dice) * dice.abs())
    for b, g in enumerate(counts):
        bound[b, :, g:] = 0                                                  # exactly zero there
    return bound


def sample_errors(pred, tgt):
    """(e_x, e_t): the gather's bound for the two plane sets."""
    return (R.sample_bound(float(pred.abs().nan_to_num(0).max()), *pred.shape[-2:]),
            R.sample_bound(float(tgt.abs().max()) if tgt.numel() else 0.0, *tgt.shape[-2:]))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def random_case(B, Q, counts, P, hw=(7, 9), thw=(14, 18), seed=0, scale=3.0):
    """pred [B, Q, H, W], tgt [sum G, Ht, Wt] binary, coords [B, P, 2] in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, Q, *hw, generator=g) * scale
    tgt = (torch.rand(sum(counts), *thw, generator=g) > 0.5).float()
    coords = torch.rand(B, P, 2, generator=g)
    return pred, tgt, coords


def centre_coords(B, P, H, W, seed=0):
    """Pixel centres of a plane whose sides are powers of two: (i + 0.5) / W is exact in fp32, the sample IS the pixel."""
    g = torch.Generator().manual_seed(seed)
    ix, iy = torch.randint(0, W, (B, P), generator=g), torch.randint(0, H, (B, P), generator=g)
    return torch.stack([(ix + 0.5) / W, (iy + 0.5) / H], -1).float()


def case_perfect_match(P=777, Q=33, G=5, side=32, seed=1):
    """Binary targets, query q < G the logits +-80 with the sign of target q, the other queries random; points at pixel centres:
    ce[q, q] = softplus(-80) ~ 1.8e-35 for q < G."""
    g = torch.Generator().manual_seed(seed)
    tgt = (torch.rand(G, side, side, generator=g) > 0.5).float()
    pred = torch.randn(1, Q, side, side, generator=g) * 3
    pred[0, :G] = 160 * tgt - 80
    return pred, tgt, centre_coords(1, P, side, side, seed), [G]


def case_constant_logits(value, P=777, Q=5, G=3, seed=2):
    pred, tgt, coords = random_case(1, Q, [G], P, seed=seed)
    return torch.full_like(pred, value), tgt, coords, [G]


def case_constant_targets(P=777, Q=5, seed=3):
    """An all-zero and an all-one target plane (and a random one)."""
    pred, tgt, coords = random_case(1, Q, [3], P, seed=seed)
    tgt[0], tgt[1] = 0, 1
    return pred, tgt, coords, [3]


def case_edge_coordinates(P=777, Q=5, G=3, seed=4):
    """Coordinates exactly 0, at pixel centres, 1 - 2^-24 and slightly outside [0, 1], mixed with random ones."""
    pred, tgt, coords = random_case(1, Q, [G], P, hw=(8, 16), thw=(14, 18), seed=seed)
    special = torch.tensor([0.0, 1 - 2.0 ** -24, -1e-3, 1 + 1e-3, -0.07, 1.07, 0.5 / 16, 7.5 / 16, 15.5 / 16, 0.5])
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(special), (1, P, 2), generator=g)
    coords = torch.where(torch.rand(1, P, 2, generator=g) < 0.7, special[pick], coords)
    return pred, tgt, coords, [G]


def case_one_pixel(P=777, Q=5, G=3, seed=5):
    """All P points on one pixel."""
    pred, tgt, coords = random_case(1, Q, [G], P, seed=seed)
    coords[:] = torch.tensor([0.4321, 0.6789])
    return pred, tgt, coords, [G]


HARD_CASES = {
    "perfect match at +-80": case_perfect_match,
    "logits all 0": lambda: case_constant_logits(0.0),
    "logits 1e4": lambda: case_constant_logits(1e4),
    "all-zero and all-one targets": case_constant_targets,
    "edge coordinates": case_edge_coordinates,
    "all points on one pixel": case_one_pixel,
}

"""Reference of the uncertain-point selection (pct_point_select_uncertain_f32, pctrans_amd/point_loss.py:
select_uncertain_points) and the hard inputs of its tests.  The reference is integer arithmetic on the CPU on the fp32 logits it
is given: key = bit pattern of |x| (0 for a NaN), a stable sort of the keys, the first n candidate numbers in ascending order.
Nothing here depends on the code under test.

The hard inputs use 8 x 16 planes and candidates on pixel centres: (j + 0.5) / 16 and (i + 0.5) / 8 are exact in fp32, so
x = c W - 0.5 is the integer j, the weights are 1, 0, 0, 0 and the sample is the pixel (i, j) -- its `ideal` logit -- as long as
the three neighbours that enter with weight 0 are finite."""
import torch

H8, W16 = 8, 16
NUM_PLANES = 8
INDEX = [6, 1, 4]                       # K = 3 of 8 planes through a non-identity index (tests/test_point_loss_gpu.py: INDEX)


def keys(logits):
    """[K, S] int64: the bit pattern of |x| as an unsigned integer, 0 for a NaN."""
    x = logits.detach().cpu().to(torch.float32).contiguous()
    bits = x.view(torch.int32).to(torch.int64) & 0x7FFFFFFF
    return torch.where(bits > 0x7F800000, torch.zeros_like(bits), bits)


def select_reference(logits, n):
    """logits [K, S] fp32 -> [K, n] int64: the n candidates with the smallest keys, ties to the lowest candidate numbers
    (a stable sort), in ascending candidate number."""
    order = torch.sort(keys(logits), dim=1, stable=True)[1]
    return torch.sort(order[:, :n], dim=1)[0]


def threshold_population(logits, n):
    """Per row: (the n-th smallest key, how many candidates hold it, how many of them are admitted)."""
    k = keys(logits)
    kth = torch.sort(k, dim=1)[0][:, n - 1]
    held = (k == kth[:, None]).sum(1)
    admitted = n - (k < kth[:, None]).sum(1)
    return kth, held, admitted


def planes_with_extremes(H, W, seed=1, scale=3.0):
    """[8, H, W]: N(0, 3) with logits of +80 on the upper half of plane 6 and -80 on the left half of plane 1."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(NUM_PLANES, H, W, generator=g) * scale
    p[INDEX[0], : H // 2] = 80.0
    p[INDEX[1], :, : W // 2] = -80.0
    return p


def random_candidates(K, S, seed=2):
    return torch.rand(K, S, 2, generator=torch.Generator().manual_seed(seed))


def centres(pix):
    """Pixel numbers [K, S] of an 8 x 16 plane -> coordinates [K, S, 2] (x, y) of the pixel centres, exact in fp32."""
    pix = torch.as_tensor(pix)
    return torch.stack([((pix % W16).float() + 0.5) / W16, ((pix // W16).float() + 0.5) / H8], -1)


def ideal_logits(planes, index, pix):
    """[K, S]: the pixels themselves, what a sample on a pixel centre is."""
    return planes.flatten(1)[torch.as_tensor(index)[:, None], torch.as_tensor(pix)]


def _signs(shape, seed):
    return torch.where(torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < 0.5, -1.0, 1.0)


def _random_pixels(K, S, seed, count=H8 * W16):
    return torch.randint(0, count, (K, S), generator=torch.Generator().manual_seed(seed))


def case_zero_plane(S):
    """Every key is 0: the answer is candidates 0 .. n - 1.  Uniform candidates (any weights: the sample of zeros is zero)."""
    return dict(planes=torch.zeros(NUM_PLANES, H8, W16), index=INDEX, coords=random_candidates(3, S, 21))


def case_one_magnitude(S, c=2.5):
    """Every pixel is +c or -c: one key, signs mixed."""
    planes = c * _signs((NUM_PLANES, H8, W16), 22)
    pix = _random_pixels(3, S, 23)
    return dict(planes=planes, index=INDEX, coords=centres(pix), pix=pix)


def case_threshold_ties(S, last_admitted):
    """Three magnitudes dealt by candidate number: s % 4 == 0 -> 0.5 (below the threshold), 1 -> 2.0 (above), 2 and 3 -> 1.0
    (the threshold key), signs mixed through the choice of pixel.  n is set so that the admitted threshold candidates end at
    candidate `last_admitted` while more of them follow.  -> the case and n."""
    assert last_admitted % 4 in (2, 3) and last_admitted + 4 < S
    planes = torch.zeros(NUM_PLANES, H8, W16)
    flat = planes.flatten(1)
    slot = torch.arange(H8 * W16) % 8                  # pixel p: magnitude number (p % 8) // 2, sign (-1) ** p
    flat[:] = torch.tensor([0.5, 2.0, 1.0, 4.0])[slot // 2] * torch.where(slot % 2 == 0, 1.0, -1.0)
    s = torch.arange(S)
    which = torch.tensor([0, 1, 2, 2])[s % 4]          # 0.5, 2.0, 1.0, 1.0
    g = torch.Generator().manual_seed(24)
    pix = torch.stack([(torch.randint(0, H8 * W16 // 8, (S,), generator=g) * 8 + 2 * which
                        + torch.randint(0, 2, (S,), generator=g)) for _ in range(3)])
    n = int((s % 4 == 0).sum()) + int(((s % 4 >= 2) & (s <= last_admitted)).sum())
    return dict(planes=planes, index=INDEX, coords=centres(pix), pix=pix), n


def case_low_mantissa_bits(S):
    """Pixel p holds +-(1 + p 2^-23): the keys differ in their lowest byte only (p < 128 keeps bit 7 clear: no carry)."""
    vals = (1.0 + torch.arange(H8 * W16, dtype=torch.float64) * 2.0 ** -23).float()
    planes = vals.view(1, H8, W16) * _signs((NUM_PLANES, H8, W16), 25)
    pix = _random_pixels(3, S, 26)
    return dict(planes=planes, index=INDEX, coords=centres(pix), pix=pix)


def case_every_exponent(S):
    """Pixel p holds +-2^e, e from -149 (the smallest denormal) to 80 in 128 steps."""
    e = (-149 + torch.arange(H8 * W16, dtype=torch.float64) * (229.0 / 127.0)).round()
    vals = (2.0 ** e).float()
    planes = vals.view(1, H8, W16) * _signs((NUM_PLANES, H8, W16), 27)
    pix = _random_pixels(3, S, 28)
    return dict(planes=planes, index=INDEX, coords=centres(pix), pix=pix)


def case_signed_zeros(S):
    """Columns 0 .. 7 hold -0, columns 8 .. 15 +0, the last row -1 and +1.  A centre sample keeps the pixel's sign when the
    three neighbours that enter with weight 0 carry it too (0 * -0 = -0, but -0 + +0 = +0): candidates stay off column 7, whose
    right neighbour is positive; those on the last row are +-1, above every zero."""
    planes = torch.zeros(NUM_PLANES, H8, W16)
    planes[:, :, :8] = -0.0
    planes[:, H8 - 1, :8] = -1.0
    planes[:, H8 - 1, 8:] = 1.0
    g = torch.Generator().manual_seed(29)
    cols = torch.tensor([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15])
    pix = torch.randint(0, H8, (3, S), generator=g) * W16 + cols[torch.randint(0, len(cols), (3, S), generator=g)]
    return dict(planes=planes, index=INDEX, coords=centres(pix), pix=pix)


def case_nan_pixels(S):
    """N(0, 3) planes with five NaN pixels each; a candidate on a NaN pixel, or with one among its weight-0 neighbours, is NaN."""
    g = torch.Generator().manual_seed(30)
    planes = torch.randn(NUM_PLANES, H8, W16, generator=g) * 3
    for p in range(NUM_PLANES):
        planes[p].view(-1)[torch.randperm(H8 * W16, generator=g)[:5]] = float("nan")
    pix = _random_pixels(3, S, 31)
    return dict(planes=planes, index=INDEX, coords=centres(pix), pix=pix)


def case_edge_coordinates(S, H=5, W=7):
    """Uniform candidates on the +-80 planes with coordinates of exactly 0 and the largest fp32 below 1 in front."""
    below1 = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    coords = random_candidates(3, S, 32)
    special = torch.tensor([(0.0, 0.0), (below1, below1), (0.0, below1), (below1, 0.0), (0.0, 0.5), (0.5, below1)])
    for k in range(3):
        coords[k, :len(special)] = special[torch.arange(len(special)).roll(k)]
    return dict(planes=planes_with_extremes(H, W), index=INDEX, coords=coords)

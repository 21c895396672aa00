"""Shapes and inputs the two ragged cross-attention test files share (a plain helper module, like hard_inputs.py).

KEYS x QUERIES x HEADS x BATCHES, masked and unmasked: the bit-identity test's whole product (L: one partial tile, three tiles,
a second tile group of one tile).
HARD_GEOMETRIES: hard_inputs.attention_case geometries at head_dim 32 with S in {50, 97, 374} and one S < 32."""
import torch

import hard_inputs as hi

KEYS = (1, 4, 22, 31, 32, 33, 63, 65, 96, 97, 127, 129, 374)
QUERIES, HEADS, BATCHES = (10, 37, 65), (4, 8, 12), (1, 3)
ALIGNED_KEYS = (64, 192)                            # on these the new entry must also give fused_ops.cross_attention's bits

HARD_GEOMETRIES = [(37, 50, 2, 8, 32), (37, 97, 2, 8, 32), (100, 374, 2, 8, 32), (16, 22, 1, 4, 32)]


def hard_case(family, geometry):
    """hard_inputs.attention_case for a geometry that need not be one of hi.ATTN_GEOMETRIES: the builder seeds itself from the
    geometry's position in that list, so a geometry outside it is looked up in a list one entry longer for the time of the
    call (the module's own list is put back, never mutated)."""
    if geometry in hi.ATTN_GEOMETRIES:
        return hi.attention_case(family, geometry)
    own = hi.ATTN_GEOMETRIES
    hi.ATTN_GEOMETRIES = own + [geometry]
    try:
        return hi.attention_case(family, geometry)
    finally:
        hi.ATTN_GEOMETRIES = own


def last_step_start(S):
    """First key of the last (partial or full) 32-key step."""
    return 32 * ((S - 1) // 32)


def bit_mask(L, S, N, seed, device="cpu"):
    """bool [N, 1, L, S], True = dead: random at 70 %, then row 1 of image 0 live at key S - 1 only, row 2 at key 0 only, row 3
    only inside the last 32-key step (all of it), and the last row of the last image fully masked.  Every other row keeps key 0."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(N, 1, L, S, generator=g) < 0.7
    mask[..., 0] = False
    mask[0, 0, 1, :] = True
    mask[0, 0, 1, S - 1] = False
    mask[0, 0, 2, 1:] = True
    mask[0, 0, 3, :] = True
    mask[0, 0, 3, last_step_start(S):] = False
    mask[N - 1, 0, L - 1, :] = True
    return mask.to(device)


def operands(L, S, N, heads, seed, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    C = heads * 16
    mk = lambda *s: torch.randn(*s, generator=g).bfloat16().to(device)
    return mk(L, N, C), mk(L, N, C), mk(S, N, C), mk(S, N, C), mk(S, N, C)

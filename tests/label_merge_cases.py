"""Inputs of the small-object merging tests: hand-built maps at the smallest sizes that reach each branch of the rules
(tests/label_merge_reference.py), and random maps drawn and then filtered to those on which no decision met a tie -- only there
is the reference's result independent of numpy's sort.

A case is (labels [H, W] int64, fg [H, W] uint8 or None, passes).  `hand()` -> name -> case; every hand-built case is asserted
tie-free by the tests except those of TIED, which are built to tie, and those of UNCOVERED, which hold values the kernels do not
cover."""
import functools

import numpy as np

import label_merge_reference as R

PASSES = R.PASSES
TIED = ("tie_two_objects", "tie_zero_and_visited")
UNCOVERED = {"count_513": R.STATUS_COUNT, "negative_value": R.STATUS_VALUE, "fractional_value": R.STATUS_VALUE}
SIDE = 24                                         # the canvas of most hand-built cases


def _canvas(h=SIDE, w=SIDE):
    return np.zeros((h, w), dtype=np.int64)


def _strips(extra=None):
    """512 distinct values with gaps up to 65 408 as 2 x 26 cells (52 pixels: never visited) on 64 x 416; the cell of value
    128 * 83 keeps three pixels and gives the others to its right neighbour, so it is a fragment between three cells."""
    m = np.zeros((64, 416), dtype=np.int64)
    for i in range(32):
        for j in range(16):
            m[2 * i:2 * i + 2, 26 * j:26 * j + 26] = 128 * (16 * i + j)
    i, j = 5, 3
    m[2 * i:2 * i + 2, 26 * j:26 * j + 26] = 128 * (16 * i + j + 1)
    m[2 * i, 26 * j + 10:26 * j + 13] = 128 * (16 * i + j)
    if extra is not None:
        m[40, 200] = extra
    return m


@functools.lru_cache(maxsize=None)
def hand():
    cases = {}

    def add(name, m, fg=None, passes=PASSES):
        cases[name] = (m, None if fg is None else fg.astype(np.uint8), tuple(passes))

    m = _canvas()                                  # a fragment inside a large object, at its rim: the first value is not 0
    m[2:18, 2:18] = 3
    m[9, 2:4] = 7
    add("inside_object", m)

    m = _canvas()                                  # in background beside an object: 0 first, the fragment second
    m[4:9, 13:18] = 3
    m[10, 10:13] = 7
    add("beside_object", m)

    m = _canvas()                                  # 0 first, another object second
    m[2:9, 8:14] = 3
    m[10, 10:12] = 7
    m[12:20, 13:20] = 9
    add("beside_two_objects", m)

    m = _canvas()                                  # deep inside an object: two distinct values in every crop, stays
    m[2:18, 2:18] = 3
    m[9, 9:11] = 7
    add("deep_inside_object", m)

    m = _canvas()                                  # exactly `threshold` pixels: visited
    m[2:9, 8:14] = 3
    m[10, 8:13] = 7
    add("exact_threshold", m, passes=((5, 5),))

    m = _canvas()                                  # the mean position is (10.5, 10.5): floor sees 3, ceil and round see 9
    m[2:9, 2:20] = 3
    m[9:21, 13:21] = 9
    m[10, 10] = m[11, 11] = 7
    add("half_centroid", m, passes=((5, 5),))

    m = _canvas()                                  # two distinct values in the crop: stays
    m[2:9, 2:9] = 3
    m[15, 15:17] = 7
    add("isolated", m)

    m = _canvas()                                  # the fragment is the first value of its own 3 x 3 crop: stays
    m[8:16, 4:10] = 3
    m[9:12, 10] = 7
    m[10, 11:13] = 7
    m[14:22, 12:20] = 9
    add("dominates_crop", m, passes=((5, 3),))

    m = _canvas()                                  # centroid near the top / left border: empty crop; near the bottom / right: clipped
    m[0:6, 2:10] = 4
    m[1, 0:2] = 8
    m[SIDE - 8:SIDE, SIDE - 12:SIDE - 2] = 3
    m[SIDE - 2, SIDE - 2:SIDE] = 7
    add("borders", m)

    m = _canvas()                                  # 5 joins the larger-numbered 6, which is then visited at its grown centroid
    m[2:10, 2:9] = 3
    m[10, 10:13] = 6
    m[12, 8:10] = 5
    add("chain_up", m, passes=((5, 5),))

    m = _canvas()                                  # 6 joins the smaller-numbered 5, which was visited before (and stayed)
    m[10, 10:15] = 5
    m[10, 8:10] = 6
    add("chain_down", m, passes=((5, 5),))

    m = _canvas()                                  # 5 and 6 see each other: whichever is visited first joins the other
    m[10, 8:10] = 5
    m[10, 10:13] = 6
    add("pair_order", m, passes=((5, 5),))

    m = _canvas()                                  # 5 (3 pixels) joins 6 (4 pixels): 7 pixels live, 4 in the snapshot -> still visited
    m[2:10, 2:9] = 3
    m[10, 10:14] = 6
    m[12, 8:11] = 5
    add("chain_grows_past_threshold", m, passes=((5, 5),))

    m = _canvas()                                  # a two-part fragment whose centroid lies in an object that it does not touch
    m[3:8, 8:12] = 3
    m[0:3, 8:12] = 3
    m[7:15, 12:20] = 9
    m[5, 5] = m[5, 15] = 7
    add("two_parts", m)

    m = _canvas()                                  # 8 pixels: survives pass 1 (5 x 5: too large), goes in pass 2 (11 x 11)
    m[2:14, 2:12] = 3
    m[6:10, 12:14] = 7
    add("second_pass", m)

    m = _canvas(32, 32)                            # 45 + 10 pixels after pass 2: skipped by the snapshot of pass 3
    m[2:30, 2:12] = 3
    m[10:19, 12:17] = 8
    m[12:17, 17:19] = 6
    add("grows_past_fifty", m)

    m = _canvas(12, 12)                            # a map so full that 0 itself is small and is visited
    m[:, :7] = 1
    m[:, 7:] = 2
    m[5, 5:8] = 0
    add("small_background", m)

    m = _canvas()                                  # the gate makes a fragment of a large object; and removes another fragment
    m[2:12, 2:12] = 3
    m[4:10, 12:22] = 4
    m[14, 4:6] = 7
    fg = np.ones_like(m)
    fg[4:10, 14:22] = 0
    fg[4:8, 12:14] = 0
    fg[14, 4:6] = 0
    add("gate", m, fg)

    m = _canvas(9, 7)                              # smaller than the 11 x 11 window in both directions
    m[7:9, :] = 3
    m[4:6, 3:7] = 3
    m[6, 3] = 3
    m[6, 6] = 9
    m[1, 1:3] = m[2, 1] = 7
    add("tiny_9x7", m, passes=((20, 11),))

    m = _canvas(6, 40)                             # smaller than the window in one direction: the wrapped crop is one or two rows
    m[0:3, 10:30] = 9
    m[5, 15:21] = 3
    m[5, 25] = 9
    m[0:6, 32:40] = 3
    m[3:5, 18:22] = 7
    add("tiny_6x40", m)

    m = _canvas()                                  # gaps up to 65 535
    m[2:12, 2:12] = 700
    m[4:6, 12:14] = 65535
    m[14:22, 10:20] = 3
    m[13, 12:14] = 40000
    add("gaps", m)

    add("count_512", _strips())
    add("count_513", _strips(65535))

    m = _canvas()
    m[2:12, 2:12] = 3
    m[4:6, 12:14] = -2
    add("negative_value", m)

    m = _canvas().astype(np.float64)
    m[2:12, 2:12] = 3
    m[4:6, 12:14] = 2.5
    add("fractional_value", m)

    add("all_zero", _canvas())

    m = _canvas()                                  # two objects with the same count in the crop: the lower value wins here
    m[2:12, 2:10] = 3
    m[2:12, 13:20] = 9
    m[6, 10:13] = 7
    add("tie_two_objects", m)

    m = _canvas()                                  # 0 and the visited value share the top count of a clipped 3 x 3 crop
    m[SIDE - 8:SIDE - 2, SIDE - 6:SIDE - 2] = 3
    m[SIDE - 2:SIDE, SIDE - 2:SIDE] = 7
    m[SIDE - 3, SIDE - 3] = 3
    m[SIDE - 3, SIDE - 2:SIDE] = 0
    add("tie_zero_and_visited", m, passes=((5, 3),))
    return cases


def tie_free_hand():
    return {k: v for k, v in hand().items() if k not in TIED and k not in UNCOVERED}


def random_map(rng, H, W, fragments=25, rectangles=(3, 8)):
    """A few rectangles (`rectangles`: at least, fewer than) plus up to `fragments` scattered fragments of 1 - 50 pixels."""
    m = np.zeros((H, W), dtype=np.int64)
    label, boxes = 0, []
    for _ in range(int(rng.integers(*rectangles))):
        label += int(rng.integers(1, 4))
        h, w = int(rng.integers(H // 6 + 1, H // 2 + 1)), int(rng.integers(W // 6 + 1, W // 2 + 1))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        m[y:y + h, x:x + w] = label
        boxes.append((y, x, h, w))
    for k in range(int(rng.integers(fragments // 2, fragments + 1))):
        label += int(rng.integers(1, 4))
        h, w = int(rng.integers(1, 6)), int(rng.integers(1, 11))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        if k % 4:                                   # three of four at the rim of a rectangle, where a crop sees three values
            by, bx, bh, bw = boxes[int(rng.integers(0, len(boxes)))]
            if rng.integers(0, 2):
                y, x = by + int(rng.integers(-h, bh + 1)), bx + (bw - 1 if rng.integers(0, 2) else -w + 1) + int(rng.integers(-2, 3))
            else:
                y, x = by + (bh - 1 if rng.integers(0, 2) else -h + 1) + int(rng.integers(-2, 3)), bx + int(rng.integers(-w, bw + 1))
            y, x = min(max(y, 0), H - h), min(max(x, 0), W - w)
        m[y:y + h, x:x + w] = label
    return m


@functools.lru_cache(maxsize=None)
def random_tie_free(H, W, want, seed, fragments=25):
    """-> (`want` tie-free maps [want, H, W], the number of draws it took)."""
    rng = np.random.default_rng(seed)
    kept, draws = [], 0
    while len(kept) < want:
        m = random_map(rng, H, W, fragments)
        draws += 1
        if R.merge(m).ties == 0:
            kept.append(m)
        assert draws <= 20 * want
    return np.stack(kept), draws

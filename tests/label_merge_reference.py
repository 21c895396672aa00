"""The table-based restatement of the reference's merge_func / merge_small_object (connectomics/engine/trainer.py:744-777) that
pctrans_amd/label_merge.py and csrc/label_merge.hip are checked against, in numpy.

`seg[seg == ids] = max_ids` moves ALL pixels of one current label to another, so the current map is cur[original value] and a
label's pixel count, row sum and column sum are additive under a merge: one census of the image, a sequential procedure over
the table rows that reads at most window^2 pixels per visit, one relabel.

One pass (threshold, window):
  snapshot   the values present in the current map, ascending, with their counts at the start of the pass (np.unique)
  visit      every value whose SNAPSHOT count is <= threshold, ascending; value 0 like any other
  centroid   from the LIVE sums: r = sum_row // count - window // 2, c likewise
  crop       seg[r:r+window, c:c+window] with numpy's slices: a negative start wraps (lo = max(start + n, 0)), hi = min(start +
             window, n), empty when lo >= hi
  decision   fewer than three distinct current values in the crop: nothing.  Ordered by count descending, then value ascending
             (the library's tie order; the reference's is numpy's unstable sort): 0 first -> the best value other than 0 and
             the visited one; otherwise the first value, and nothing if that is the visited one
  tie        a decision met one when 0 and the visited value share the top count, or when more than one eligible value (all
             but 0 and the visited one when 0 is first, else all) has the best count
  merge      the visited value's three sums go to the target, every original value mapped to it is redirected

`variant` names one wrong reading of the rules, for the test that shows the listed cases tell them apart."""
import numpy as np

PASSES = ((5, 5), (20, 11), (50, 11))
MAX_VALUES = 512
STATUS_VALUE, STATUS_COUNT, STATUS_TIE = 1, 2, 4
VARIANTS = ("ceil_centroid", "round_centroid", "clamp_crop", "live_sizes", "snapshot_centroid", "stale_sums", "descending",
            "ge2_distinct", "lt_threshold", "gate_after")


def crop_range(start, window, n, clamp=False):
    """numpy's seg[start:start + window] on an axis of n: -> (lo, hi), empty when lo >= hi."""
    assert start + window > 0                       # (the centroid is >= 0: the stop never wraps)
    if clamp:
        lo = max(start, 0)
    else:
        lo = max(start + n, 0) if start < 0 else min(start, n)
    return lo, min(start + window, n)


class Merged:
    """out: the merged map; values: the distinct gated values, ascending; final: the value each of them ends as; before, after:
    pixel counts; merges: per pass; ties: decisions that met a tie; events: (pass, visited value, target value)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def status(self):
        v = self.values.astype(np.float64)
        bad = bool(((v < 0) | (v > 65535) | (v != np.trunc(v))).any())
        return (STATUS_VALUE if bad else 0) | (STATUS_COUNT if len(v) > MAX_VALUES else 0) | (STATUS_TIE if self.ties else 0)


def merge(seg, passes=PASSES, fg=None, variant=None):
    seg = np.asarray(seg)
    assert seg.ndim == 2 and variant in (None,) + VARIANTS
    if fg is not None and variant != "gate_after":
        seg = np.where(np.asarray(fg) != 0, seg, np.zeros((), dtype=seg.dtype))
    H, W = seg.shape
    values, inv = np.unique(seg, return_inverse=True)
    inv = inv.reshape(H, W)
    K = len(values)
    flat = inv.ravel()
    ys, xs = np.divmod(np.arange(H * W, dtype=np.int64), W)
    cnt = np.bincount(flat, minlength=K).astype(np.int64)
    sr = np.rint(np.bincount(flat, weights=ys.astype(np.float64), minlength=K)).astype(np.int64)      # (exact: far below 2^53)
    sc = np.rint(np.bincount(flat, weights=xs.astype(np.float64), minlength=K)).astype(np.int64)
    before = cnt.copy()
    cur = np.arange(K)
    zero = int(np.searchsorted(values, 0)) if (values == 0).any() else -1
    merges, ties, events = [0] * len(passes), 0, []
    for p, (threshold, window) in enumerate(passes):
        snap, snap_r, snap_c = cnt.copy(), sr.copy(), sc.copy()
        order = range(K - 1, -1, -1) if variant == "descending" else range(K)
        for k in order:
            size = cnt[k] if variant == "live_sizes" else snap[k]
            if size == 0:
                continue                                        # not in the snapshot
            if size > threshold or (variant == "lt_threshold" and size == threshold):
                continue
            if variant is None:
                assert cnt[k] > 0, "a value is never visited after it vanished"
            elif cnt[k] == 0:
                continue
            n, a, b = (snap[k], snap_r[k], snap_c[k]) if variant == "snapshot_centroid" else (cnt[k], sr[k], sc[k])
            if variant == "ceil_centroid":
                r, c = -(-a // n), -(-b // n)
            elif variant == "round_centroid":
                r, c = (2 * a + n) // (2 * n), (2 * b + n) // (2 * n)
            else:
                r, c = a // n, b // n
            r0, r1 = crop_range(int(r) - window // 2, window, H, variant == "clamp_crop")
            c0, c1 = crop_range(int(c) - window // 2, window, W, variant == "clamp_crop")
            if r0 >= r1 or c0 >= c1:
                continue
            hist = np.bincount(cur[inv[r0:r1, c0:c1]].ravel(), minlength=K)
            present = np.nonzero(hist)[0]
            if len(present) < (2 if variant == "ge2_distinct" else 3):
                continue
            top = hist.max()
            zero_first = zero >= 0 and hist[zero] == top
            if zero_first:
                eligible = [v for v in present if v != zero and v != k]
                if not eligible:
                    continue                                    # (only with ge2_distinct)
                tie = k != zero and hist[k] == top
            else:
                eligible, tie = list(present), False
            best = max(hist[v] for v in eligible)
            winners = [v for v in eligible if hist[v] == best]
            ties += int(tie or len(winners) > 1)
            target = winners[0]                                 # count descending, then value ascending
            if target == k:
                continue
            cnt[target] += cnt[k]
            if variant != "stale_sums":
                sr[target] += sr[k]
                sc[target] += sc[k]
            cnt[k] = sr[k] = sc[k] = 0
            cur[cur == k] = target
            merges[p] += 1
            events.append((p, values[k], values[target]))
    out = values[cur][inv]
    if fg is not None and variant == "gate_after":
        out = np.where(np.asarray(fg) != 0, out, np.zeros((), dtype=out.dtype))
    return Merged(out=out.astype(seg.dtype), values=values, final=values[cur], before=before, after=cnt, merges=merges, ties=ties,
                  events=events)

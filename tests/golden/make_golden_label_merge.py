#!/usr/bin/env python3
"""Golden vectors for the small-object merging, from the reference's own code.  RUN IN THE DEV CONTAINER ONLY.

`connectomics/engine/trainer.py` of the reference cannot be imported here (its header needs the whole data pipeline), but
`merge_func` and `merge_small_object` (:744-777) touch nothing but numpy.  As make_golden_targets.py does, this script reads the
file as text, takes exactly those two functions out of its AST, executes them unmodified in a namespace holding numpy, feeds them
the maps of tests/label_merge_cases.py and stores inputs and outputs in label_merge_small.npz next to this file.  Nothing of the
reference's source is copied into the repository; only data is written.

Stored: the three single passes (5, 5), (20, 11), (50, 11) each on its own, the whole merge_func on the hand-built and on random
tie-free maps, and one run on float32 maps, as test_cvppp has them.  The reference orders equal counts by numpy's unstable
sort, so before writing the script asserts with the restatement (tests/label_merge_reference.py) that no stored case met a tie:
otherwise the fixture would pin one numpy build's sort.

    python tests/golden/make_golden_label_merge.py [--ref /root/reference]
"""
import argparse
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
TRAINER = "connectomics/engine/trainer.py"
SEED = 20240


def load_reference(ref_root):
    path = os.path.join(ref_root, TRAINER)
    tree = ast.parse(open(path).read(), filename=path)
    picked = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in ("merge_func", "merge_small_object")]
    assert len(picked) == 2
    ns = {"np": np}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return ns["merge_func"], ns["merge_small_object"]


def main():
    import label_merge_cases as C
    import label_merge_reference as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    merge_func, merge_small_object = load_reference(args.ref)
    out = {}

    def store(name, seg, passes, dtype=np.int32):
        assert R.merge(seg, passes).ties == 0, name
        got = seg.astype(dtype)
        if tuple(passes) == R.PASSES:
            got = merge_func(got)
        else:
            for threshold, window in passes:
                got = merge_small_object(got, threshold=threshold, window=window)
        out[name + ".in"], out[name + ".out"], out[name + ".passes"] = seg.astype(dtype), got, np.asarray(passes, dtype=np.int32)

    for name, (seg, fg, passes) in sorted(C.tie_free_hand().items()):
        if name == "count_512":
            continue                                # (64 x 416: the largest hand-built map adds nothing the others lack here)
        gated = seg if fg is None else seg * fg     # the trainer's `seg_outputs * fg`
        store("hand." + name, gated, passes, np.uint16 if gated.max() > 32767 else np.int32)
    maps, _ = C.random_tie_free(37, 53, 6, SEED)
    for n, seg in enumerate(maps):
        store("random.%d" % n, seg, R.PASSES)
        store("float.%d" % n, seg, R.PASSES, np.float32)
    for p, single in enumerate(R.PASSES):
        kept = 0
        for seg in C.random_tie_free(37, 53, 12, SEED + 1)[0]:
            if R.merge(seg, (single,)).ties == 0 and kept < 3:
                store("pass%d.%d" % (p, kept), seg, (single,))
                kept += 1
        assert kept == 3
    path = os.path.join(HERE, "label_merge_small.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for the instance targets, from the reference's own code.  RUN IN THE DEV CONTAINER ONLY.

`connectomics/engine/trainer.py` of the reference cannot be imported here (its header needs GPUtil, h5py, waterz and the
whole data pipeline), but `Trainer.prepare_intance_targets` (:231-319) touches nothing but torch, `random` and three
configuration values.  As make_golden_decoder.py does, this script reads the file as text, takes exactly that method out of
its AST, executes it unmodified in a namespace holding torch and random, with a bare namespace as `self`, feeds it the
small label maps below and stores inputs and outputs in targets_small.npz next to this file.  Nothing of the reference's
source is copied into the repository; only data is written.

The maps (37 x 53: odd width, not square, neither dimension a multiple of 16) are built from rectangles, a one-pixel instance,
a border ring that touches all four borders and a pair of equal rectangles, with gaps between the label values
{0, 3, 7, 200, 65535} and a different number of instances per image.  Every such instance has a mean position that is a
multiple of 1/4 -- exact in fp32 -- and coordinate sums far below 2^24, so the reference's float mean is exact and its
`mean / W` is the exact rational centre rounded to fp32 ONCE: the device path (exact integer sums, one rounding) must
reproduce these centre points bit for bit.  The script asserts that property of its own output before writing it.

    python tests/golden/make_golden_targets.py [--ref /root/reference]
"""
import argparse
import ast
import os
import random
import types
from fractions import Fraction

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TRAINER = "connectomics/engine/trainer.py"
H, W = 37, 53
SEED = 1234


def load_reference_method(ref_root):
    path = os.path.join(ref_root, TRAINER)
    tree = ast.parse(open(path).read(), filename=path)
    picked = [fn for node in tree.body if isinstance(node, ast.ClassDef) and node.name == "Trainer"
              for fn in node.body if isinstance(fn, ast.FunctionDef) and fn.name == "prepare_intance_targets"]
    assert len(picked) == 1
    ns = {"torch": torch, "random": random}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return ns["prepare_intance_targets"]


def bag(ignore_label, points_num, semantic_loss_on):
    NS = types.SimpleNamespace
    model = NS(SEM_SEG_HEAD=NS(IGNORE_VALUE=ignore_label),
               MASK_FORMER=NS(POSITION_POINTS_NUM=points_num, SEMANTIC_LOSS_ON=semantic_loss_on))
    return NS(cfg=NS(MODEL=model), device=torch.device("cpu"))


def label_maps():
    a = np.zeros((H, W), dtype=np.int64)
    a[0, :] = a[H - 1, :] = 65535                       # a ring on all four borders
    a[:, 0] = a[:, W - 1] = 65535
    a[2:10, 3:21] = 3
    a[12:31, 5:26] = 200
    a[20, 31] = 7                                       # one pixel
    b = np.zeros((H, W), dtype=np.int64)
    b[3:9, 2:12] = 3                                    # two equal rectangles, one instance
    b[20:26, 30:40] = 3
    b[10:18, 12:29] = 200
    b[30:36, 44:52] = 65535
    return np.stack([a, b])


def exact_centres(gt, ids):
    out = []
    for v in ids:
        ys, xs = np.nonzero(gt == v)
        n = len(xs)
        out.append([np.float32(float(Fraction(int(xs.sum()), n * W))), np.float32(float(Fraction(int(ys.sum()), n * W)))])
    return np.asarray(out, dtype=np.float32).reshape(-1, 2)


def store(out, case, got):
    for n, item in enumerate(got):
        for k, v in item.items():
            out["%s.%d.%s" % (case, n, k)] = v.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    prepare = load_reference_method(args.ref)
    maps = label_maps()
    out = {"maps": maps.astype(np.int32), "empty": np.zeros((1, H, W), dtype=np.int32), "seed": np.asarray(SEED)}
    for ignore in (0, -1):
        for disc in (False, True):
            got = prepare(bag(ignore, 1, True), [torch.from_numpy(maps)], disc)
            case = "i%d_d%d" % (ignore, int(disc))
            store(out, case, got)
            for n, item in enumerate(got):               # the property the module text states
                ids = np.unique(maps[n])
                want = exact_centres(maps[n], ids[ids != ignore])
                assert np.array_equal(item["center_points"].numpy(), want), (case, n)
    store(out, "empty", prepare(bag(0, 1, True), [torch.zeros((1, H, W), dtype=torch.int64)], False))
    random.seed(SEED)
    store(out, "p3", prepare(bag(0, 3, True), [torch.from_numpy(maps)], True))
    path = os.path.join(HERE, "targets_small.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()

"""CPU: the validation metrics' torch formulation (pctrans_amd/metrics.py, mode="torch") and the table-based numpy reference
against the literal per-mask definitions (tests/metrics_reference.py), the discrimination of the test inputs, the ABI
bookkeeping of the two entries (include/pctrans_hip_metrics.h) and the argument validation."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import metrics_reference as R
from conftest import ROOT

NAMES = ["pct_label_overlap", "pct_label_metrics"]
SIZES = [(64, 64), (37, 53)]


@functools.lru_cache(maxsize=None)
def _cases(H, W):
    return R.small_builders(H, W)


@functools.lru_cache(maxsize=None)
def _literal(H, W, name, variant=None):
    pred, gt = _cases(H, W)[name]
    return R.literal(pred, gt, variant)


def _rows(result):
    """Metrics of a batch -> one dict of Python numbers per image."""
    cols = {k: v.cpu().tolist() for k, v in result.items()}
    return [{k: cols[k][n] for k in cols} for n in range(len(next(iter(cols.values()))))]


def _torch_rows(pred, gt, fg=None):
    from pctrans_amd import metrics as M
    p, g = torch.from_numpy(np.stack(pred)), torch.from_numpy(np.stack(gt))
    cv, bb = M.cvppp_metrics(p, g, fg, mode="torch"), M.bbbc_metrics(p, g, fg, mode="torch")
    assert cv.mode == bb.mode == "torch" and cv.status.dtype == torch.int32
    return [dict(a, **b) for a, b in zip(_rows(cv), _rows(bb))], cv.status.tolist()


def test_abi_bookkeeping():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_metrics.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_metrics.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_lib.METRICS_SYMBOLS) == sorted(NAMES)
    for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.SEG_SYMBOLS, _lib.FPN_SYMBOLS, _lib.ATTN_TRAIN_SYMBOLS,
                  _lib.REID_SYMBOLS, _lib.TARGETS_SYMBOLS, _lib.MSDA_TRAIN_SYMBOLS, _lib.REID_QUERY_SYMBOLS):
        assert not set(NAMES) & set(other)
    for name in NAMES:
        argtypes, restype, checked_by = _lib.METRICS_SYMBOLS[name]
        assert restype is ctypes.c_int and os.path.exists(os.path.join(ROOT, checked_by))
        decl = re.search(r"PCT_API int %s\(([^)]*)\)" % name, header).group(1)
        assert len(argtypes) == len(decl.split(",")), name
        assert hasattr(_lib.lib(), name)
    makefile = open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()
    assert " label_metrics.hip " in makefile and "pctrans_hip_metrics.h" in makefile
    launchers = open(os.path.join(ROOT, "pctrans_amd", "csrc", "launchers.hpp")).read()
    assert "launch_label_overlap(" in launchers and "launch_label_metrics(" in launchers
    from pctrans_amd import metrics as M
    for macro, value in (("PCT_METRICS_MAX_VALUES", M.MAX_VALUES), ("PCT_METRICS_WORKSPACE_PER_IMAGE", M.WORKSPACE_PER_IMAGE),
                         ("PCT_METRICS_COLUMNS", M.COLUMNS), ("PCT_METRICS_STATUS_PRED_VALUE", M.STATUS_PRED_VALUE),
                         ("PCT_METRICS_STATUS_PRED_COUNT", M.STATUS_PRED_COUNT), ("PCT_METRICS_STATUS_GT_VALUE", M.STATUS_GT_VALUE),
                         ("PCT_METRICS_STATUS_GT_COUNT", M.STATUS_GT_COUNT), ("PCT_METRICS_STATUS_EMPTY_PRED", M.STATUS_EMPTY_PRED),
                         ("PCT_METRICS_STATUS_EMPTY_GT", M.STATUS_EMPTY_GT)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro


def test_geometry_outside_the_limits_is_refused_before_any_launch():
    """No launch, so this runs without a GPU: the pointers are host memory that is never dereferenced."""
    from pctrans_amd import _lib
    L = _lib.lib()
    UNSUP, BAD = -4, -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    args = lambda N, H, W, dp=1, dg=1: (p, dp, p, dg, None, N, H, W, p, p, p, p, p, p, p, None)
    assert L.pct_label_overlap(*args(0, 8, 8)) == UNSUP
    assert L.pct_label_overlap(*args(65536, 8, 8)) == UNSUP
    assert L.pct_label_overlap(*args(1, 4096, 4096)) == UNSUP              # height * width = 2^24
    assert L.pct_label_overlap(*args(1, 8, 8, dp=5)) == UNSUP
    assert L.pct_label_overlap(*args(1, 8, 8, dg=-1)) == UNSUP
    assert L.pct_label_overlap(*args(1, 0, 8)) == BAD
    assert L.pct_label_metrics(p, p, p, p, p, 0, p, p, None) == UNSUP
    assert L.pct_label_metrics(p, p, p, p, p, 65536, p, p, None) == UNSUP
    assert L.pct_label_metrics(p, p, p, p, None, 1, p, p, None) == BAD


@pytest.mark.parametrize("size", SIZES)
def test_torch_mode_against_the_literal_definitions(size):
    H, W = size
    cases = _cases(H, W)
    names = sorted(cases)
    rows, status = _torch_rows([cases[k][0] for k in names], [cases[k][1] for k in names])
    from pctrans_amd import metrics as M
    for name, row, st in zip(names, rows, status):
        want = _literal(H, W, name)
        assert not R.mismatches(row, want), (name, R.mismatches(row, want))
        pred, gt = cases[name]
        assert bool(st & M.STATUS_EMPTY_PRED) == (not pred.any()) and bool(st & M.STATUS_EMPTY_GT) == (not gt.any()), name
        assert not st & M.STATUS_FALLBACK
    empty = rows[names.index("empty_both")]
    assert all(empty[k] == 0 for k in R.FLOAT_KEYS + R.INT_KEYS)
    assert rows[names.index("empty_pred")]["aji"] == 0 and rows[names.index("empty_gt")]["aji"] == 0


@pytest.mark.parametrize("size", SIZES)
def test_torch_overlap_against_per_pair_masks(size):
    from pctrans_amd import metrics as M
    H, W = size
    cases = _cases(H, W)
    names = sorted(cases)
    ov = M.label_overlap(torch.from_numpy(np.stack([cases[k][0] for k in names])),
                         torch.from_numpy(np.stack([cases[k][1] for k in names])), mode="torch")
    assert ov.mode == "torch" and ov.table.shape[1:] == (M.MAX_VALUES, M.MAX_VALUES)
    for n, name in enumerate(names):
        vp, vg, ap, ag, T = R.literal_table(*cases[name])
        assert ov.num[n].tolist() == [len(vp), len(vg)], name
        assert ov.values[n, 0, :len(vp)].tolist() == vp.tolist() and ov.values[n, 1, :len(vg)].tolist() == vg.tolist()
        assert ov.areas[n, 0, :len(vp)].tolist() == ap.tolist() and ov.areas[n, 1, :len(vg)].tolist() == ag.tolist()
        assert ov.range[n].tolist() == [[vp[0], vp[-1]], [vg[0], vg[-1]]]
        assert np.array_equal(ov.table[n, :len(vg), :len(vp)].numpy(), T) and int(ov.table[n].sum()) == H * W
        assert not ov.values[n, 0, len(vp):].any() and not ov.areas[n, 1, len(vg):].any()


@pytest.mark.parametrize("size", SIZES)
def test_table_reference_against_the_literal_definitions(size):
    H, W = size
    for name, (pred, gt) in sorted(_cases(H, W).items()):
        want = _literal(H, W, name)
        got = R.from_table(pred, gt)
        assert not R.mismatches(got, want), (name, R.mismatches(got, want))
        assert (got["terms_pred"], got["terms_gt"]) == (want["terms_pred"], want["terms_gt"]), name
        vp, vg, ap, ag, T = R.literal_table(pred, gt)
        for a, b in zip(R.table(pred, gt), (vp, vg, ap, ag, T)):
            assert np.array_equal(a, b), name


def test_the_inputs_tell_the_known_wrong_variants_apart():
    """Each wrong reading of the definitions moves at least one metric of at least one builder by more than 1e-6."""
    H, W = SIZES[0]
    for variant in R.VARIANTS:
        moved = []
        for name in sorted(_cases(H, W)):
            want, wrong = _literal(H, W, name), _literal(H, W, name, variant)
            if any(abs(want[k] - wrong[k]) > 1e-6 for k in R.FLOAT_KEYS):
                moved.append(name)
        assert moved, variant
    expect = {"ge_half": "iou_half", "last_max": "iou_tie", "no_take_on_zero_row": "aji_zero_row",
              "bd_present_divisor": "gaps", "bg_zero_cvppp": "no_background"}
    for variant, name in expect.items():
        want, wrong = _literal(H, W, name), _literal(H, W, name, variant)
        assert any(abs(want[k] - wrong[k]) > 1e-6 for k in R.FLOAT_KEYS), (variant, name)


def test_foreground_map_and_values_the_kernels_do_not_cover_in_torch_mode():
    from pctrans_amd import metrics as M
    H, W = SIZES[1]
    pred, gt = _cases(H, W)["blocks_shifted"]
    fg = (np.arange(W)[None, :] % 3 != 0) & np.ones((H, 1), dtype=bool)
    rows, _ = _torch_rows([pred], [gt], torch.from_numpy(fg[None]))
    assert not R.mismatches(rows[0], R.literal(pred * fg, gt))
    # more than 512 distinct values, negative, large and non-integral values: the torch mode scores them all and says so
    many, few = R.many_values(513), R.many_values(512)
    rows, status = _torch_rows([many, few], [few, many])
    assert status == [M.STATUS_PRED_COUNT, M.STATUS_GT_COUNT]
    for row, (p, g) in zip(rows, ((many, few), (few, many))):
        assert not R.mismatches(row, R.from_table(p, g))
    odd = pred.astype(np.float32)
    for value, bit in ((-1.0, M.STATUS_PRED_VALUE), (70000.0, M.STATUS_PRED_VALUE), (2.5, M.STATUS_PRED_VALUE)):
        m = odd.copy()
        m[5, 7] = value
        res = M.cvppp_metrics(torch.from_numpy(m[None]), torch.from_numpy(gt[None]), mode="torch")
        assert res.status.tolist() == [bit], value
        res = M.cvppp_metrics(torch.from_numpy(gt[None]), torch.from_numpy(m[None]), mode="torch")
        assert res.status.tolist() == [M.STATUS_GT_VALUE], value


def test_modes_switch_and_supported(monkeypatch):
    from pctrans_amd import metrics as M
    H, W = 16, 12
    pred, gt = torch.zeros((2, H, W), dtype=torch.int16), torch.ones((2, H, W), dtype=torch.int64)
    with pytest.raises(ValueError, match="mode"):
        M.cvppp_metrics(pred, gt, mode="numpy")
    with pytest.raises(ValueError, match="mode"):
        M.label_overlap(pred, gt, mode="")
    with pytest.raises(ValueError, match="dataset"):
        M.instance_metrics(pred, gt, "COCO")
    with pytest.raises(ValueError):
        M.bbbc_metrics(pred, gt[:, :8])
    monkeypatch.delenv("PCT_METRICS", raising=False)
    assert M.default() == "hip"
    monkeypatch.setenv("PCT_METRICS", "torch")
    assert M.default() == "torch"
    monkeypatch.setenv("PCT_METRICS", "cuda")
    with pytest.raises(RuntimeError, match="PCT_METRICS"):
        M.default()
    monkeypatch.delenv("PCT_METRICS")
    assert not M.supported(pred, gt)                                       # CPU tensors: the default mode gives the torch result
    res = M.instance_metrics(pred, gt, "BBBC")
    assert res.mode == "torch" and set(res) == {"aji", "dice", "dq", "sq", "pq", "tp", "fp", "fn", "taken"}
    assert set(M.instance_metrics(pred, gt, "CVPPP")) == {"best_dice_pred", "best_dice_gt", "sbd", "abs_diff_fg"}
    # the limits, on stand-ins without storage (`supported` looks at shape, dtype and device only)
    class _Cuda:
        """What `supported` asks of a tensor, for a device this machine may not have."""
        def __init__(self, shape, dtype=torch.int16):
            self.shape, self.dtype, self.is_cuda, self.device = torch.Size(shape), dtype, True, torch.device("cuda", 0)
        def dim(self):
            return len(self.shape)
    monkeypatch.setattr(torch, "is_tensor", lambda x: isinstance(x, (torch.Tensor, _Cuda)))
    ok = lambda *shape, **kw: M.supported(_Cuda(shape, **kw), _Cuda(shape))
    assert ok(1, 520, 696) and ok(65535, 2, 2) and ok(1, 4095, 4096) and ok(1, 1, 2 ** 24 - 1)
    assert not ok(65536, 2, 2) and not ok(0, 4, 4) and not ok(1, 4096, 4096) and not ok(1, 0, 4)
    assert not ok(1, 8, 8, dtype=torch.float64) and not ok(1, 8, 8, dtype=torch.bool) and ok(1, 8, 8, dtype=torch.float32)
    assert not M.supported(_Cuda((1, 8, 8)), _Cuda((1, 8, 9))) and not M.supported(_Cuda((8, 8)), _Cuda((8, 8)))
    assert not M.supported(_Cuda((1, 8, 8)), _Cuda((1, 8, 8)), fg=_Cuda((1, 8, 8), torch.float32))
    assert M.supported(_Cuda((1, 8, 8)), _Cuda((1, 8, 8)), fg=_Cuda((1, 8, 8), torch.uint8))


def test_source_rules_of_the_kernel_file():
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "label_metrics.hip")).read()
    assert "asm" not in src and "__builtin_amdgcn" not in src                  # vector stores and plain C++ only
    assert "float atomic" not in src and "atomicAdd(&T[key], len)" in src      # integer adds: one per run
    assert not re.search(r"\b(malloc|hipMalloc|hipStreamSynchronize|hipDeviceSynchronize|hipMemcpy)\b", src)

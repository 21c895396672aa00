"""CPU: the C ABI entries of the point-sampled mask losses (header, binding table, exports, argument validation without a
launch), the PCT_POINT_LOSS switch and its routing on CPU tensors, and the float64 reference of test_point_loss_gpu.py
(point_loss_reference.py) against the criterion's existing formulation and against autograd."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import point_loss_reference as R
from pctrans_amd import _lib, point_loss
from pctrans_amd.loss import maskformer_criterion as crit
from pctrans_amd.loss import point_features
from pctrans_amd.loss.matcher import Point_HungarianMatcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pct_point_sample_f32", "pct_point_mask_loss_forward_f32", "pct_point_mask_loss_backward_f32")


def _criterion(num_points=70, mode=None):
    c = crit.SetCriterion(1, Point_HungarianMatcher(num_points=num_points), {}, 0.1, ["masks"], num_points, 3.0, 0.75)
    if mode is not None:
        c.point_loss = c.matcher.point_sample = mode
    return c


def test_header_table_and_exports_agree_on_the_three_entries():
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    declared = set(re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    gpu_tests = open(os.path.join(ROOT, "tests", "test_point_loss_gpu.py")).read()
    for name, nargs in zip(NAMES, (12, 17, 12)):
        assert name in declared and name in _lib.OPT_IN_SYMBOLS and name not in _lib.SYMBOLS
        argtypes, restype, checked_by = _lib.OPT_IN_SYMBOLS[name]
        assert len(argtypes) == nargs and restype is ctypes.c_int and checked_by == "tests/test_point_loss_gpu.py"
        assert name in gpu_tests
        assert re.search(r"\bT %s\b" % name, out)
        assert getattr(_lib.lib(), name).argtypes == argtypes
        # the declaration's parameter count is the table's
        decl = re.search(r"PCT_API int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == nargs
    assert declared == set(_lib.OPT_IN_SYMBOLS) and _lib.ABI_VERSION == 1 and _lib.lib().pct_abi_version() == 1


def test_band_rows_and_width_constants_are_the_kernel_s():
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "point_loss.hip")).read()
    assert int(re.search(r"PL_BAND_ROWS = (\d+);", src).group(1)) == point_loss.BAND_ROWS
    assert int(re.search(r"PL_MAX_WIDTH = (\d+);", src).group(1)) == point_loss.MAX_WIDTH
    assert point_loss.BAND_ROWS * point_loss.MAX_WIDTH * 8 <= 64 * 1024          # a band of 64-bit accumulators in 64 KiB


def test_argument_validation_returns_status_codes_without_a_launch():
    L = _lib.lib()
    BAD, ALIGN, UNSUP = -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # host pointer, never dereferenced
    assert p % 16 == 0
    # gather: (planes, index, coords, num_planes, H, W, K, P, coord_rows, per_row, out, stream)
    assert L.pct_point_sample_f32(p, None, p, 4, 5, 7, -1, 8, 4, 1, p, None) == BAD
    assert L.pct_point_sample_f32(p, None, p, 4, 0, 7, 4, 8, 4, 1, p, None) == BAD
    assert L.pct_point_sample_f32(p, None, p, 4, 5, 7, 4, 8, 4, 0, p, None) == BAD          # planes_per_coord_row < 1
    assert L.pct_point_sample_f32(p, None, p, 4, 5, 7, 4, 8, 1, 2, p, None) == BAD          # 4 outputs at 2 per row, 1 row
    assert L.pct_point_sample_f32(p, None, p, 4, 5, 7, 6, 8, 6, 1, p, None) == BAD          # identity past the planes
    assert L.pct_point_sample_f32(None, None, p, 4, 5, 7, 4, 8, 4, 1, p, None) == BAD
    assert L.pct_point_sample_f32(p + 2, None, p, 4, 5, 7, 4, 8, 4, 1, p, None) == ALIGN
    assert L.pct_point_sample_f32(p, None, p + 4, 4, 5, 7, 4, 8, 4, 1, p, None) == ALIGN      # coords: 8-byte pairs
    assert L.pct_point_sample_f32(p, None, p, 4, 65536, 65536, 4, 8, 4, 1, p, None) == UNSUP
    assert L.pct_point_sample_f32(p, None, p, 4, 5, 7, 0, 8, 0, 1, p, None) == 0
    assert L.pct_point_sample_f32(p, None, p, 4, 5, 7, 4, 0, 4, 1, p, None) == 0
    # forward: (pred, src, n_pred, H, W, tgt, tgt_index, n_tgt, Ht, Wt, coords, K, P, x, t, sums, stream)
    fwd = L.pct_point_mask_loss_forward_f32
    assert fwd(p, p, 8, 5, 7, p, p, 3, 9, 9, p, -1, 8, p, p, p, None) == BAD
    assert fwd(p, p, 8, 5, 7, p, p, 3, 9, 0, p, 3, 8, p, p, p, None) == BAD
    assert fwd(p, p, 8, 5, 7, p, p, 3, 9, 9, p, 3, 8, p, None, p, None) == BAD
    assert fwd(p, None, 2, 5, 7, p, p, 3, 9, 9, p, 3, 8, p, p, p, None) == BAD                # identity past the planes
    assert fwd(p, p, 8, 5, 7, p, p + 1, 3, 9, 9, p, 3, 8, p, p, p, None) == ALIGN
    assert fwd(p, p, 8, 5, 7, p, p, 3, 9, 9, p + 4, 3, 8, p, p, p, None) == ALIGN
    assert fwd(p, p, 8, 5, point_loss.MAX_WIDTH + 1, p, p, 3, 9, 9, p, 3, 8, p, p, p, None) == UNSUP
    assert fwd(p, p, 8, 5, 7, p, p, 3, 9, 9, p, 0, 8, p, p, p, None) == 0
    assert fwd(p, p, 8, 5, 7, p, p, 3, 9, 9, p, 3, 0, p, p, p, None) == 0
    # backward: (x, t, coords, alpha, beta, gamma, K, P, H, W, grad_planes, stream)
    bwd = L.pct_point_mask_loss_backward_f32
    assert bwd(p, p, p, p, p, p, 3, -1, 5, 7, p, None) == BAD
    assert bwd(p, p, p, p, p, p, 3, 8, 5, 0, p, None) == BAD
    assert bwd(p, p, p, p, None, p, 3, 8, 5, 7, p, None) == BAD
    assert bwd(p, p, p, p, p, p, 3, 8, 5, 7, p + 2, None) == ALIGN
    assert bwd(p, p, p + 4, p, p, p, 3, 8, 5, 7, p, None) == ALIGN
    assert bwd(p, p, p, p, p, p, 3, 8, 5, point_loss.MAX_WIDTH + 1, p, None) == UNSUP
    assert bwd(p, p, p, p, p, p, 0, 8, 5, 7, p, None) == 0
    assert bwd(p, p, p, p, p, p, 3, 0, 5, 7, p, None) == 0


def test_switch_default_follows_the_environment(monkeypatch):
    monkeypatch.delenv("PCT_POINT_LOSS", raising=False)
    assert point_loss.default() == "torch"
    c = _criterion()
    assert c.point_loss == "torch" and c.matcher.point_sample == "torch"
    monkeypatch.setenv("PCT_POINT_LOSS", "hip")
    c = _criterion()
    assert c.point_loss == "hip" and c.matcher.point_sample == "hip"
    monkeypatch.setenv("PCT_POINT_LOSS", "bogus")
    with pytest.raises(RuntimeError, match="PCT_POINT_LOSS"):
        point_loss.default()
    with pytest.raises(RuntimeError):
        _criterion()


def test_cpu_tensors_keep_the_torch_path(monkeypatch):
    pred, targets, indices = R.module_case()
    for name in ("point_sample_planes", "point_mask_losses"):
        monkeypatch.setattr(point_loss, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("device path on CPU tensors")))
    got = {}
    for mode in ("torch", "hip"):
        c = _criterion(mode=mode)
        torch.manual_seed(3)
        p = pred.clone().requires_grad_(True)
        losses = c.loss_masks({"pred_masks": p}, targets, indices, 6.0)
        (losses["loss_mask"] + losses["loss_dice"]).backward()
        torch.manual_seed(4)
        match = c.matcher({"pred_masks": pred}, targets)
        got[mode] = (losses["loss_mask"].detach(), losses["loss_dice"].detach(), p.grad, match)
    for a, b in zip(got["torch"][:3], got["hip"][:3]):
        assert torch.equal(a, b)
    for (i0, j0), (i1, j1) in zip(got["torch"][3], got["hip"][3]):
        assert torch.equal(i0, i1) and torch.equal(j0, j1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        point_loss.point_mask_loss_forward(pred, None, targets[0]["masks"], None, torch.zeros(3, 4, 2))


def test_reference_is_the_criterion_s_current_formulation(monkeypatch):
    """The yardstick against the existing code alone: loss_masks (torch path, float64, CPU) on a seeded case, and the reference
    on the coordinates that call drew, agree to float64 rounding, values and gradient."""
    pred, targets, indices = R.module_case()
    c = _criterion(mode="torch")
    seen = []
    real = point_features.point_sample
    monkeypatch.setattr(crit, "point_sample", lambda inp, pc, **kw: seen.append(pc) or real(inp, pc, **kw))
    p = pred.double().requires_grad_(True)
    torch.manual_seed(3)
    torch.set_default_dtype(torch.float64)           # torch.rand then draws float64 coordinates, which grid_sample needs here
    try:
        losses = c.loss_masks({"pred_masks": p}, targets, indices, 6.0)
    finally:
        torch.set_default_dtype(torch.float32)
    (2.0 * losses["loss_mask"] + 0.5 * losses["loss_dice"]).backward()
    coords = seen[-1]
    assert coords.shape == (6, 70, 2)
    src = torch.cat([s + b * 6 for b, (s, _) in enumerate(indices)])
    tgt = torch.cat([t + b * 3 for b, (_, t) in enumerate(indices)])
    lm, ld, grad = R.losses64(pred.double(), src, torch.cat([t["masks"] for t in targets]), tgt, coords, 6.0)
    assert abs(float(lm - losses["loss_mask"].detach())) <= 1e-12 and abs(float(ld - losses["loss_dice"].detach())) <= 1e-12
    assert float((grad(2.0, 0.5) - p.grad).abs().max()) <= 1e-12
    unmatched = torch.ones(12, dtype=torch.bool)
    unmatched[src] = False
    assert float(p.grad.flatten(0, 1)[unmatched].abs().max()) == 0.0


def test_closed_form_gradient_is_autograd_of_the_reference():
    """grad_x = alpha (sigma - t) + sigma (1 - sigma) (beta - gamma t) with the header's coefficients, against autograd of
    sigmoid_ce_loss and dice_loss in float64; scattered, against autograd through grid_sample."""
    g = torch.Generator().manual_seed(2)
    K, P, H, W = 3, 70, 5, 7
    x = (torch.randn(K, P, generator=g, dtype=torch.float64) * 4).requires_grad_(True)
    t = torch.rand(K, P, generator=g, dtype=torch.float64)
    for g_m, g_d in ((1.0, 1.0), (0.0, 2.5), (-3.0, 0.0)):
        loss = g_m * crit.sigmoid_ce_loss(x, t, 6.0) + g_d * crit.dice_loss(x, t, 6.0)
        want = torch.autograd.grad(loss, x)[0]
        a, b, c = R.coefficients64(R.sums64(x, t), P, 6.0, g_m, g_d)
        got = R.grad_x_closed_form(x, t, a, b, c)
        assert float((got - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))
    pred, targets, indices = R.module_case()
    src = torch.cat([s + b * 6 for b, (s, _) in enumerate(indices)])
    tgt = torch.cat([tt + b * 3 for b, (_, tt) in enumerate(indices)])
    coords = torch.rand(6, P, 2, generator=g)
    planes = torch.cat([tt["masks"] for tt in targets])
    _, _, grad = R.losses64(pred, src, planes, tgt, coords, 6.0)
    xs, ts = R.sample64(pred.flatten(0, 1), src, coords), R.sample64(planes, tgt, coords)
    a, b, c = R.coefficients64(R.sums64(xs, ts), P, 6.0, 1.0, 1.0)
    scattered, count = R.scatter64(R.grad_x_closed_form(xs, ts, a, b, c), coords, 40, 24)
    assert float((scattered - grad(1.0, 1.0).flatten(0, 1)[src]).abs().max()) <= 1e-14
    assert float(count.sum()) >= 4 * 6 * P - 1e-9 and bool((count[scattered != 0] > 0).all())


def test_seeded_case_has_few_candidates_that_can_flip():
    """The module-level GPU test compares the coordinates the two paths select; it allows a difference only among the
    candidates this counts, and caps them at 1 % of the selected points.  The seeded case itself stays under the cap."""
    pred, targets, indices = R.module_case()
    src = torch.cat([s + b * 6 for b, (s, _) in enumerate(indices)])
    torch.manual_seed(3)
    cand = torch.rand(6, 210, 2)
    logits = R.sample64(pred.flatten(0, 1), src, cand)
    e_s = R.sample_bound(float(pred.abs().max()), 40, 24)
    selected = 6 * int(0.75 * 70)
    assert R.flip_candidates(logits, int(0.75 * 70), e_s) <= 0.01 * selected
    # and the count does count: a bound as wide as the logits' spread makes every candidate one
    assert R.flip_candidates(logits, int(0.75 * 70), 100.0) == 6 * 210

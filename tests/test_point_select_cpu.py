"""CPU: the C ABI entry of the uncertain-point selection (header, binding table, export, argument validation without a launch),
the PCT_POINT_SELECT switch and its routing on CPU tensors, the reference of test_point_select_gpu.py
(point_select_reference.py) against torch.topk and against hand-written rows, and the hard-input builders against what the GPU
test assumes of them, on their ideal logits."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import point_loss_reference as R
import point_select_reference as SR
from pctrans_amd import _lib, point_loss
from pctrans_amd.loss import maskformer_criterion as crit
from pctrans_amd.loss.matcher import Point_HungarianMatcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pct_point_select_uncertain_f32"


def _criterion(num_points=70):
    return crit.SetCriterion(1, Point_HungarianMatcher(num_points=num_points), {}, 0.1, ["masks"], num_points, 3.0, 0.75)


def test_header_table_and_export_agree():
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in _lib.OPT_IN_SYMBOLS and NAME not in _lib.SYMBOLS
    argtypes, restype, checked_by = _lib.OPT_IN_SYMBOLS[NAME]
    assert len(argtypes) == 13 and restype is ctypes.c_int and checked_by == "tests/test_point_select_gpu.py"
    assert NAME in open(os.path.join(ROOT, checked_by)).read()
    assert re.search(r"\bT %s\b" % NAME, out)
    assert getattr(_lib.lib(), NAME).argtypes == argtypes
    decl = re.search(r"PCT_API int %s\((.*?)\);" % NAME, header, re.S).group(1)
    assert len(decl.split(",")) == 13
    assert _lib.ABI_VERSION == 1 and _lib.lib().pct_abi_version() == 1


def test_candidate_limit_is_the_kernel_s_and_the_header_s():
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "point_loss.hip")).read()
    assert int(re.search(r"PL_SELECT_MAX_CAND = (\d+);", src).group(1)) == point_loss.MAX_CANDIDATES >= 65536
    assert int(re.search(r"PL_SELECT_BLOCK = (\d+);", src).group(1)) * 64 == point_loss.MAX_CANDIDATES   # 64 keys per thread
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    assert "num_cand <= %d" % point_loss.MAX_CANDIDATES in header


def test_argument_validation_returns_status_codes_without_a_launch():
    fn = _lib.lib().pct_point_select_uncertain_f32
    BAD, ALIGN, UNSUP = -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # host pointer, never dereferenced
    assert fn(p, p, 8, 5, 7, p, 3, 8, 9, p, 9, p, None) == BAD                # num_keep > num_cand
    assert fn(p, p, 8, 5, 7, p, 3, 8, 4, p, 3, p, None) == BAD                # a row shorter than num_keep
    assert fn(p, p, 8, 5, 7, p + 4, 3, 8, 4, p, 4, p, None) == ALIGN
    assert fn(p, p, 8, 5, 7, p, 3, point_loss.MAX_CANDIDATES + 1, 4, p, 4, p, None) == UNSUP
    assert fn(p, p, 8, 5, 7, p, 0, 8, 4, p, 4, p, None) == 0
    assert fn(p, p, 8, 5, 7, p, 3, 8, 0, p, 0, None, None) == 0


def test_switch_default_follows_the_environment(monkeypatch):
    monkeypatch.delenv("PCT_POINT_SELECT", raising=False)
    assert point_loss.select_default() == "torch" and _criterion().point_select == "torch"
    monkeypatch.setenv("PCT_POINT_SELECT", "hip")
    c = _criterion()
    assert point_loss.select_default() == "hip" and c.point_select == "hip" and c.point_loss == "torch"
    monkeypatch.setenv("PCT_POINT_SELECT", "topk")
    with pytest.raises(RuntimeError, match="PCT_POINT_SELECT"):
        point_loss.select_default()
    with pytest.raises(RuntimeError):
        _criterion()


def test_cpu_tensors_raise_and_keep_the_torch_path(monkeypatch):
    pred, targets, indices = R.module_case()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        point_loss.select_uncertain_points(pred, None, torch.zeros(12, 8, 2), 4)
    assert not point_loss.select_supported(pred, torch.zeros(12, 8, 2), 4)
    monkeypatch.setattr(point_loss, "select_uncertain_points",
                        lambda *a, **k: (_ for _ in ()).throw(AssertionError("device path on CPU tensors")))
    got = {}
    for loss, select in (("torch", "torch"), ("hip", "hip"), ("torch", "hip")):
        c = _criterion()
        c.point_loss, c.point_select = loss, select
        torch.manual_seed(3)
        p = pred.clone().requires_grad_(True)
        losses = c.loss_masks({"pred_masks": p}, targets, indices, 6.0)
        (losses["loss_mask"] + losses["loss_dice"]).backward()
        got[loss, select] = (losses["loss_mask"].detach(), losses["loss_dice"].detach(), p.grad)
    for other in (("hip", "hip"), ("torch", "hip")):
        assert all(torch.equal(a, b) for a, b in zip(got["torch", "torch"], got[other]))


def test_reference_agrees_with_topk_on_tie_free_rows():
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(5, 2065, generator=g) * 3
    assert all(len(row.abs().unique()) == 2065 for row in logits)
    for n in (1, 516, 2064, 2065):
        want = torch.topk(-logits.abs(), n, dim=1)[1]
        got = SR.select_reference(logits, n)
        assert got.shape == (5, n) and bool((got[:, 1:] > got[:, :-1]).all())
        assert all(set(got[k].tolist()) == set(want[k].tolist()) for k in range(5))


def test_reference_follows_the_tie_and_nan_rules():
    nan, inf = float("nan"), float("inf")
    row = torch.tensor([[2.0, -1.0, 1.0, 0.5, -1.0, nan, 1.0, -0.0, 0.0, -inf, 3.0, nan]])
    #  keys by candidate:  2     1     1    .5    1     0    1     0    0    inf   3    0
    assert SR.keys(row).tolist()[0][5] == 0 and SR.keys(row).tolist()[0][7] == 0 and SR.keys(row).tolist()[0][9] == 0x7F800000
    assert SR.select_reference(row, 1).tolist() == [[5]]                       # a NaN first, the lowest number of the key-0 ties
    assert SR.select_reference(row, 3).tolist() == [[5, 7, 8]]                  # NaN, -0 and +0 tie: candidate order
    assert SR.select_reference(row, 4).tolist() == [[5, 7, 8, 11]]
    assert SR.select_reference(row, 5).tolist() == [[3, 5, 7, 8, 11]]
    assert SR.select_reference(row, 7).tolist() == [[1, 2, 3, 5, 7, 8, 11]]      # two of the four with |x| = 1: the lowest numbers
    assert SR.select_reference(row, 9).tolist() == [[1, 2, 3, 4, 5, 6, 7, 8, 11]]
    assert SR.select_reference(row, 12).tolist() == [list(range(12))]
    kth, held, admitted = SR.threshold_population(row, 7)
    assert (int(kth), int(held), int(admitted)) == (0x3F800000, 4, 2)


def test_hard_input_builders_are_as_hard_as_the_gpu_test_assumes():
    """On ideal logits (the pixel under each centre candidate): what each family is built for."""
    case = SR.case_one_magnitude(2065)
    x = SR.ideal_logits(case["planes"], case["index"], case["pix"])
    assert len(SR.keys(x).unique()) == 1 and bool((x < 0).any()) and bool((x > 0).any())
    # pixel centres are exact: c W - 0.5 is the column, c H - 0.5 the row
    c = SR.centres(case["pix"]).double()
    assert torch.equal(c[..., 0] * SR.W16 - 0.5, (case["pix"] % SR.W16).double())
    assert torch.equal(c[..., 1] * SR.H8 - 0.5, (case["pix"] // SR.W16).double())
    for S, last in ((2065, 1024 + 5 * 64 + 38), (2065, 1024 + 5 * 64 + 63), (2065, 1023), (37632, 20 * 1024 + 1023)):
        case, n = SR.case_threshold_ties(S, last)
        x = SR.ideal_logits(case["planes"], case["index"], case["pix"])
        kth, held, admitted = SR.threshold_population(x, n)
        assert bool((kth == 0x3F800000).all()) and bool((0 < admitted).all()) and bool((admitted < held).all())
        want = SR.select_reference(x, n)
        ones = SR.keys(x) == 0x3F800000
        for k in range(3):
            assert int(want[k][ones[k][want[k]]].max()) == last and bool(ones[k, last + 1:].any())
        assert bool((x < 0).any()) and bool((x > 0).any())
    case = SR.case_low_mantissa_bits(2065)
    k = SR.keys(SR.ideal_logits(case["planes"], case["index"], case["pix"]))
    assert len((k >> 8).unique()) == 1 and len(k.unique()) > 100
    case = SR.case_every_exponent(2065)
    k = SR.keys(SR.ideal_logits(case["planes"], case["index"], case["pix"]))
    assert int((k >> 23).min()) == 0 and int(k.min()) == 1 and int((k >> 23).max()) == 127 + 80 and len((k >> 23).unique()) > 100
    case = SR.case_signed_zeros(2065)
    x = SR.ideal_logits(case["planes"], case["index"], case["pix"])
    zero = x == 0
    assert bool((zero & torch.signbit(x)).any(1).all()) and bool((zero & ~torch.signbit(x)).any(1).all())
    assert int(zero.sum(1).min()) > 140 and bool((~zero).any(1).all()) and not bool((case["pix"] % SR.W16 == 7).any())
    case = SR.case_nan_pixels(2065)
    x = SR.ideal_logits(case["planes"], case["index"], case["pix"])
    assert 60 < int(x.isnan().sum(1).min()) and bool((case["planes"].isnan().sum((1, 2)) == 5).all())
    case = SR.case_edge_coordinates(210)
    assert float(case["coords"].min()) == 0.0 and float(case["coords"].max()) < 1.0
    assert float(case["coords"].max()) == float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))


def test_random_inputs_have_few_candidates_that_can_flip():
    """The GPU test's condition flip_candidates <= 0.01 K n, on the CPU, for the smaller sizes of each geometry."""
    for H, W in ((5, 7), (67, 24), (8, 16)):
        planes = SR.planes_with_extremes(H, W)
        for S in (210, 1000, 2065):
            x64 = R.sample64(planes, SR.INDEX, SR.random_candidates(3, S))
            n = S // 4
            assert R.flip_candidates(x64, n, R.sample_bound(float(planes.abs().max()), H, W)) <= 0.01 * 3 * n

"""No GPU: the PCT_MATCH_COST switch and its routing on CPU tensors, the binding of pct_point_match_cost_f32, and the reference
and bounds of test_match_cost_gpu.py (match_cost_reference.py): the reference against the matcher's own fp32 chain, and every hard
input shown to pose a finite assignment problem whose bound is far below the scale of its costs."""
import ctypes
import os
import re

import pytest
import torch
from scipy.optimize import linear_sum_assignment

import match_cost_reference as M
from pctrans_amd import _lib, point_loss
from pctrans_amd.loss import matcher as matcher_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pct_point_match_cost_f32"


def test_abi_declares_and_binds_the_entry():
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    assert re.search(r"PCT_API int %s\(" % NAME, header)
    assert NAME in _lib.OPT_IN_SYMBOLS and NAME not in _lib.SYMBOLS
    argtypes, restype, checked_by = _lib.OPT_IN_SYMBOLS[NAME]
    assert len(argtypes) == 19 and restype is ctypes.c_int and checked_by == "tests/test_match_cost_gpu.py"
    assert argtypes[14] is ctypes.c_float and argtypes[15] is ctypes.c_float
    assert NAME in open(os.path.join(ROOT, checked_by)).read()
    assert getattr(_lib.lib(), NAME).argtypes == argtypes


def test_status_codes_need_no_device():
    fn = getattr(_lib.lib(), NAME)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert fn(p, 2, 5, 7, 9, p, 3, 14, 18, p, p, 3, p, -1, 1.0, 1.0, p, p, None) == -1
    assert fn(p, 2, 5, 7, 9, p, 3, 14, 18, p, p, 3, p + 4, 70, 1.0, 1.0, p, p, None) == -3
    assert fn(p, 2, 5, 65536, 65536, p, 3, 14, 18, p, p, 3, p, 70, 1.0, 1.0, p, p, None) == -4
    assert fn(p, 2, 5, 7, 9, p, 3, 14, 18, p, p, 0, p, 70, 1.0, 1.0, p, p, None) == 0


def test_default_and_env_parsing(monkeypatch):
    monkeypatch.delenv("PCT_MATCH_COST", raising=False)
    assert point_loss.match_cost_default() == "torch" and matcher_mod.Point_HungarianMatcher(num_points=4).match_cost == "torch"
    monkeypatch.setenv("PCT_MATCH_COST", "hip")
    m = matcher_mod.Point_HungarianMatcher(num_points=4)
    assert point_loss.match_cost_default() == "hip" and m.match_cost == "hip" and m.point_sample == "torch"
    monkeypatch.setenv("PCT_MATCH_COST", "mfma")
    with pytest.raises(RuntimeError, match="PCT_MATCH_COST"):
        point_loss.match_cost_default()


def test_supported_rejects_cpu_non_fp32_and_non_contiguous():
    pred, tgt = torch.zeros(2, 5, 7, 9), torch.zeros(3, 14, 18)
    assert not point_loss.match_cost_supported(pred, tgt, 70, 3)                       # CPU
    with pytest.raises(RuntimeError, match="CPU"):
        point_loss.match_costs(pred, tgt, torch.zeros(2), torch.zeros(2), torch.zeros(2, 70, 2), 1.0, 1.0, 3)
    meta = "meta"                                                                      # the checks that need no device memory
    if hasattr(torch.zeros(1, device=meta), "is_cuda"):
        assert not point_loss.match_cost_supported(pred.to(meta), tgt.to(meta), 70, 3)
    assert not point_loss.match_cost_supported(pred.double(), tgt, 70, 3)
    assert not point_loss.match_cost_supported(pred.transpose(2, 3), tgt, 70, 3)
    assert not point_loss.match_cost_supported(pred, tgt, 0, 3) and not point_loss.match_cost_supported(pred, tgt, 70, 0)


def test_workspace_formula_follows_the_header():
    # configs[3]: 2 x 300 queries, 60 targets, 12 544 points: 3 query groups, 1 target group, 98 passes -> 32 chunks at most
    assert point_loss.match_cost_workspace_bytes(2, 300, 60, 12544) == 4 * 2 * 32 * (2 * 384 * 64 + 384 + 64)
    assert point_loss.match_cost_workspace_bytes(1, 1, 1, 1) == 4 * (2 * 128 * 64 + 128 + 64)
    assert point_loss.match_cost_workspace_bytes(1, 1024, 512, 12544) == 4 * 8 * (2 * 1024 * 512 + 1024 + 512)
    for B, Q, G, P in ((2, 300, 60, 12544), (1, 33, 5, 777), (3, 100, 37, 129), (1, 1024, 512, 65)):
        L, chunks = M.plan(B, Q, G, P)
        qg, gg = -(-Q // 128), -(-G // 64)
        assert chunks * L >= P and 4 * B * chunks * (2 * qg * 128 * gg * 64 + qg * 128 + gg * 64) <= \
            point_loss.match_cost_workspace_bytes(B, Q, G, P)


def _targets(tgt, counts):
    out, at = [], 0
    for g in counts:
        out.append({"masks": tgt[at:at + g]})
        at += g
    return out


def test_matcher_on_cpu_tensors_takes_todays_path(monkeypatch):
    pred, tgt, _ = M.random_case(2, 12, [3, 5], 70, hw=(20, 12), thw=(40, 24), seed=3)
    called = []
    monkeypatch.setattr(point_loss, "match_costs", lambda *a, **k: called.append(1))
    got = {}
    for mode in ("torch", "hip"):
        m = matcher_mod.Point_HungarianMatcher(5.0, 2.0, num_points=70)
        m.match_cost = mode
        torch.manual_seed(7)
        got[mode] = m.forward({"pred_masks": pred}, _targets(tgt, [3, 5]))
    assert not called
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got["torch"], got["hip"]))


def test_reference_reproduces_batched_costs_within_fp32_roundoff():
    counts = [3, 5]
    pred, tgt, _ = M.random_case(2, 12, counts, 70, hw=(20, 12), thw=(40, 24), seed=4)
    m = matcher_mod.Point_HungarianMatcher(5.0, 2.0, num_points=70)
    torch.manual_seed(9)
    C, got_counts = m._batched_costs({"pred_masks": pred}, _targets(tgt, counts))
    torch.manual_seed(9)
    coords = torch.cat([torch.rand(1, 70, 2) for _ in range(2)])
    want = M.cost64(pred, tgt, counts, coords, 5.0, 2.0)
    assert got_counts == counts and C.shape == want.shape
    for b, g in enumerate(counts):                        # (past a count the chain holds the cost of a zero mask: never read)
        assert float((C[b, :, :g].double() - want[b, :, :g]).abs().max()) <= 1e-5 * float(want.abs().max())
    assert bool((want[0, :, 3:] == 0).all())


@pytest.mark.parametrize("name", sorted(M.HARD_CASES))
def test_hard_inputs_pose_a_finite_problem_and_the_bound_is_below_the_cost_scale(name):
    pred, tgt, coords, counts = M.HARD_CASES[name]()
    x, t = M.samples64(pred, tgt, counts, coords)
    C = M.cost64(pred, tgt, counts, coords, 5.0, 2.0)
    assert bool(C.isfinite().all())
    ri, ci = linear_sum_assignment(C[0, :, :counts[0]].numpy())
    total = float(C[0, ri, ci].sum())
    assert total == total and abs(total) < float("inf")
    for e in ((0.0, 0.0), M.sample_errors(pred, tgt)):
        bound = M.cost_bound(x, t, counts, 5.0, 2.0, *e)
        assert bool(bound.isfinite().all()) and float(bound.max()) < 1e-2 * float(C.abs().max()), (name, float(bound.max()))
    # the cross-entropy's contraction bound is relative to the non-negative sum
    ce = M.parts64(x, t)[0] / coords.shape[1]
    b_ce = M.cost_bound(x, t, counts, 1.0, 0.0)
    assert bool((b_ce <= 1e-4 * ce + 1e-36).all()), name

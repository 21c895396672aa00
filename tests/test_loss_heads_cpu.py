"""CPU: the head dimension of the point-sampled losses and matcher costs (pct_point_select_uncertain_many_f32,
pct_point_mask_loss_forward_many_f32, pct_point_match_cost_many_f32; pctrans_amd/point_loss.py: *_many): the PCT_LOSS_HEADS switch,
header / binding table / export, the argument checks that return before a launch, the pre-drawn random numbers against the
per-head sequence of torch.rand calls, and the criterion and matcher on CPU tensors, where "batched" must be "each"."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import point_loss_reference as R
from pctrans_amd import _lib, point_loss
from pctrans_amd.loss import maskformer_criterion as crit
from pctrans_amd.loss.matcher import Point_HungarianMatcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pct_point_select_uncertain_many_f32", "pct_point_mask_loss_forward_many_f32", "pct_point_match_cost_many_f32")
BAD, ALIGN, UNSUP = -1, -3, -4


def _criterion(num_points=70):
    return crit.SetCriterion(1, Point_HungarianMatcher(num_points=num_points), {}, 0.1, ["masks"], num_points, 3.0, 0.75)


def test_switch_default_follows_the_environment(monkeypatch):
    monkeypatch.delenv("PCT_LOSS_HEADS", raising=False)
    c = _criterion()
    assert point_loss.heads_default() == "each" and c.loss_heads == "each" and c.matcher.cost_heads == "each"
    monkeypatch.setenv("PCT_LOSS_HEADS", "batched")
    c = _criterion()
    assert point_loss.heads_default() == "batched" and c.loss_heads == "batched" and c.matcher.cost_heads == "batched"
    assert c.point_loss == "torch" and c.point_select == "torch" and c.matcher.match_cost == "torch"     # the others stay theirs
    monkeypatch.setenv("PCT_LOSS_HEADS", "all")
    with pytest.raises(RuntimeError, match="PCT_LOSS_HEADS"):
        point_loss.heads_default()
    with pytest.raises(RuntimeError):
        _criterion()
    with pytest.raises(RuntimeError):
        Point_HungarianMatcher(num_points=4)


def test_header_table_and_exports_agree_on_the_three_entries():
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    declared = set(re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    gpu_tests = open(os.path.join(ROOT, "tests", "test_loss_heads_gpu.py")).read()
    for name, nargs in zip(NAMES, (14, 18, 20)):
        assert name in declared and name in _lib.OPT_IN_SYMBOLS and name not in _lib.SYMBOLS
        argtypes, restype, checked_by = _lib.OPT_IN_SYMBOLS[name]
        assert len(argtypes) == nargs and restype is ctypes.c_int and checked_by == "tests/test_loss_heads_gpu.py"
        assert name in gpu_tests
        assert re.search(r"\bT %s\b" % name, out)
        assert getattr(_lib.lib(), name).argtypes == argtypes
        decl = re.search(r"PCT_API int %s\((.*?)\);" % name, header, re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == nargs and params[0] == "const float *const *preds" and params[1] == "int num_heads"
        for p, t in zip(params, argtypes):                          # pointers, ints and floats in the declaration's order
            want = ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float") else ctypes.c_int
            assert t is want, (name, p)
        # the single-head sibling's parameters follow the head table
        single = re.search(r"PCT_API int %s\((.*?)\);" % name.replace("_many", ""), header, re.S).group(1)
        assert [" ".join(p.split()) for p in params[2:]] == [" ".join(p.split()) for p in single.split(",")][1:]
    assert declared == set(_lib.OPT_IN_SYMBOLS) and _lib.ABI_VERSION == 1 and _lib.lib().pct_abi_version() == 1


def test_head_limit_is_the_header_s_and_the_kernel_s():
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "point_loss.hip")).read()
    assert int(re.search(r"#define PCT_POINT_MAX_HEADS (\d+)", header).group(1)) == point_loss.MAX_HEADS == 16
    assert int(re.search(r"PL_MAX_HEADS = (\d+);", src).group(1)) == point_loss.MAX_HEADS
    # both kernels of a stage call one body
    for body in ("point_select_body", "point_loss_forward_body", "match_cost_partial_body", "match_cost_finish_body"):
        assert len(re.findall(r"\b%s\b" % body, src)) == 3, body    # the definition and the two kernels
    assert point_loss._head_groups(17) == [(0, 16), (16, 17)] and point_loss._head_groups(16) == [(0, 16)]
    assert point_loss._head_groups(1) == [(0, 1)] and point_loss._head_groups(33) == [(0, 16), (16, 32), (32, 33)]


def _table(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def test_argument_validation_returns_status_codes_without_a_launch():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # host pointer, never dereferenced
    assert p % 16 == 0
    three, seventeen = _table(p, p, p), _table(*[p] * 17)
    hole, odd = _table(p, None, p), _table(p, p + 2, p)

    def select(t, n, cand=p, keep=4, row=4):
        return L.pct_point_select_uncertain_many_f32(t, n, p, 8, 5, 7, cand, 3, 8, keep, p, row, p, None)

    def forward(t, n, coords=p, pairs=3):
        return L.pct_point_mask_loss_forward_many_f32(t, n, p, 8, 5, 7, p, p, 6, 9, 11, coords, pairs, 12, p, p, p, None)

    def cost(t, n, coords=p, points=70, ws=p, h=7, w=9):
        return L.pct_point_match_cost_many_f32(t, n, 2, 5, h, w, p, 3, 14, 18, p, p, 3, coords, points, 1.0, 1.0, ws, p, None)

    for fn in (select, forward, cost):
        assert fn(three, 0) == 0 and fn(None, 0) == 0               # no head: OK, nothing launched
        assert fn(seventeen, 17) == BAD and fn(three, -1) == BAD
        assert fn(None, 3) == BAD and fn(hole, 3) == BAD            # a missing table, a missing entry
        assert fn(odd, 3) == ALIGN                                  # every entry's alignment
        assert fn(three, 3, p + 4) == ALIGN                         # coordinates: 8 bytes
    # the single-head rules hold behind the head table
    assert select(three, 3, keep=9, row=9) == BAD and select(three, 3, keep=4, row=3) == BAD
    assert select(three, 3, keep=0, row=0) == 0 and forward(three, 3, pairs=0) == 0 and cost(three, 3, points=0) == 0
    assert L.pct_point_select_uncertain_many_f32(three, 3, p, 8, 5, 7, p, 3, point_loss.MAX_CANDIDATES + 1, 4, p, 4, p, None) == UNSUP
    assert L.pct_point_mask_loss_forward_many_f32(three, 3, p, 8, 5, 257, p, p, 6, 9, 11, p, 3, 12, p, p, p, None) == UNSUP
    assert cost(three, 3, ws=p + 8) == ALIGN and cost(three, 3, points=-1) == BAD and cost(three, 3, h=65536, w=65536) == UNSUP
    # (head, image) is one grid dimension: 16 heads x 4096 images is past it
    sixteen = _table(*[p] * 16)
    assert L.pct_point_match_cost_many_f32(sixteen, 16, 4096, 5, 7, 9, p, 3, 14, 18, p, p, 3, p, 70, 1.0, 1.0, p, p, None) == UNSUP


def test_workspace_is_the_single_head_size_per_head():
    one = point_loss.match_cost_workspace_bytes(2, 300, 60, 12544)
    assert point_loss.match_cost_many_workspace_bytes(10, 2, 300, 60, 12544) == 10 * one
    # planned for the real batch: a plan for 20 images would split the points into fewer chunks
    assert point_loss.match_cost_workspace_bytes(20, 300, 60, 12544) != 10 * one
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    assert "num_heads * (4 * batch * chunks * (2 Qp Gp + Qp + Gp)) bytes" in header


@pytest.mark.parametrize("heads,K,S,N", [(1, 6, 144, 12), (4, 6, 210, 18), (10, 3, 37632, 3136), (3, 5, 9, 0)])
def test_pre_drawn_coordinates_are_the_per_head_sequence(heads, K, S, N):
    torch.manual_seed(11)
    want = []
    for _ in range(heads):
        want.append((torch.rand(K, S, 2), torch.rand(K, N, 2) if N > 0 else torch.empty(K, 0, 2)))
    state = torch.get_rng_state()
    torch.manual_seed(11)
    cand, fresh = point_loss.draw_head_coords(heads, K, S, N, torch.device("cpu"))
    assert torch.equal(torch.get_rng_state(), state)
    assert cand.shape == (heads, K, S, 2) and fresh.shape == (heads, K, N, 2) and cand.is_contiguous() and fresh.is_contiguous()
    for h in range(heads):
        assert torch.equal(cand[h], want[h][0]) and torch.equal(fresh[h], want[h][1])


def test_cpu_tensors_raise_and_are_not_supported():
    preds = [torch.zeros(2, 5, 33, 20) for _ in range(3)]
    tgt = torch.zeros(7, 41, 27)
    cand = torch.zeros(3, 6, 144, 2)
    assert not point_loss.select_many_supported(preds, cand, 36) and not point_loss.loss_many_supported(preds, tgt)
    assert not point_loss.match_costs_many_supported(preds, tgt, 70, 3)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        point_loss.select_uncertain_points_many(preds, None, cand, 36)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        point_loss.match_costs_many(preds, tgt, torch.zeros(2), torch.zeros(2), torch.zeros(3, 2, 70, 2), 1.0, 1.0, 3)
    with pytest.raises(RuntimeError):
        point_loss.point_mask_losses_many(preds, torch.zeros(3, 6), tgt, torch.zeros(3, 6), torch.zeros(3, 6, 48, 2), 6.0)
    # heads must be alike
    assert not point_loss._heads_alike([]) and not point_loss._heads_alike(preds + [torch.zeros(2, 5, 33, 21)])
    assert not point_loss._heads_alike(preds + [preds[0].double()]) and point_loss._heads_alike(preds)


def _outputs(seed, heads, dtype_of=None, short_head=None):
    """final + (heads - 1) auxiliary predictions of R.module_case's geometry, each with its own matching."""
    _, targets, _ = R.module_case()
    g = torch.Generator().manual_seed(seed)
    preds = [(torch.randn(2, 6, 40, 24, generator=g) * 3).requires_grad_(True) for _ in range(heads)]
    if dtype_of is not None:
        preds[dtype_of] = preds[dtype_of].detach().bfloat16().requires_grad_(True)       # (runs under autocast)
    indices = []
    for h in range(heads):
        ind = []
        for _ in range(2):
            n = 2 if h == short_head else 3
            ind.append((torch.randperm(6, generator=g)[:n], torch.randperm(3, generator=g)[:n]))
        indices.append(ind)
    for t in targets:                                              # forward's loops also form loss_refpoints of the later heads
        t["center_points"] = torch.rand(3, 2, generator=g)
    outputs = {"pred_masks": preds[-1], "aux_outputs": [{"pred_masks": p} for p in preds[:-1]], "indices_list": indices,
               "aux_reference_points": [{"reference_points": torch.rand(2, 6, 2, generator=g)} for _ in range(heads - 2)]}
    return outputs, targets, preds


@pytest.mark.parametrize("variant", ["alike", "one head bfloat16", "one head with fewer pairs"])
@pytest.mark.parametrize("loss,select", [("torch", "torch"), ("hip", "hip")])
def test_criterion_on_cpu_tensors_batched_is_each(monkeypatch, variant, loss, select):
    for name in ("select_uncertain_points_many", "point_mask_losses_many", "draw_head_coords"):
        monkeypatch.setattr(point_loss, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("batched path on CPU tensors")))
    kw = {"one head bfloat16": {"dtype_of": 1}, "one head with fewer pairs": {"short_head": 2}}.get(variant, {})
    got = {}
    for mode in ("each", "batched"):
        outputs, targets, preds = _outputs(21, 4, **kw)
        c = _criterion()
        c.point_loss, c.point_select, c.loss_heads = loss, select, mode
        torch.manual_seed(3)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=variant == "one head bfloat16"):
            losses = c(outputs, targets)
        assert set(losses) >= set(["loss_mask", "loss_dice"] + ["%s_%d" % (n, i) for n in ("loss_mask", "loss_dice")
                                                               for i in range(3)])
        sum(v.double() * (1 + 0.25 * i) for i, v in enumerate(losses[k] for k in sorted(losses))).backward()
        got[mode] = ({k: v.detach() for k, v in losses.items()}, [p.grad for p in preds], torch.get_rng_state())
    assert all(torch.equal(got["each"][0][k], got["batched"][0][k]) for k in got["each"][0])
    assert all(torch.equal(a, b) for a, b in zip(got["each"][1], got["batched"][1]))
    assert torch.equal(got["each"][2], got["batched"][2])


def test_matcher_on_cpu_tensors_batched_is_each(monkeypatch):
    monkeypatch.setattr(point_loss, "match_costs_many", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device path")))
    _, targets, _ = R.module_case()
    g = torch.Generator().manual_seed(5)
    outs = [{"pred_masks": torch.randn(2, 6, 40, 24, generator=g) * 3} for _ in range(3)]
    got = {}
    for mode in ("each", "batched"):
        m = Point_HungarianMatcher(5.0, 2.0, num_points=70)
        m.match_cost, m.cost_heads = "hip", mode
        torch.manual_seed(7)
        got[mode] = (m.forward_many(outs, targets), torch.get_rng_state())
    assert torch.equal(got["each"][1], got["batched"][1])
    for a, b in zip(got["each"][0], got["batched"][0]):
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))

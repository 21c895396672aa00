"""GPU: every MSDeformAttn kernel on samples that sit ON the pixel lattice and ON the gate (tests/msda_lattice_cases.py), where
grad_sampling_loc is one-sided: at an integer pixel coordinate k the cell [k, k + 1] counts (floor), and a sample is gated out
exactly on -1 and on W / H (cuh:290-296).  The other MSDA files leave samples within 1e-3 px of an integer out of their
grad_sampling_loc comparison; here nothing is masked but the samples the case builder records as undecided (the fp32 coordinate
depends on whether loc * W - 0.5 is rounded once or twice; none on power-of-two maps, under 10 % on the others).
tests/test_msda_lattice_cpu.py shows that a kernel with a left-cell, truncating, `>= -1` or `<= W` rule misses these bounds by
more than a factor of 100.

  backward   generic, column and windowed kernel (forced with pct_msda_set_bwd_kernel_choice, asserted with
             pct_msda_last_bwd_kernel) against orc.backward on the same fp32 operands, 2e-5 * max(1, max|ref|) per gradient as
             tests/test_msda_bwd_col_gpu.py; a gated-out sample's grad_sampling_loc and grad_attn_weight are exactly 0.0
  forward    generic, quad-owner, windowed and column kernel against orc.forward at 1e-4; with one level's value all +inf and
             all of that level's samples gated out on the lattice the output stays finite (a `>=` gate gives 0 * inf = NaN)
  fused      the training entry (pctrans_amd/msda_train.py) on pixel-centre reference points with whole-pixel offsets and with
             the module's real initial grid, against float64 at the fp32 location the entry forms, bounds() of
             tests/test_msda_fused_train_gpu.py without its edge mask
The windowed kernels decline calls of fewer than 32 768 records: they run the cases of 43 008 records and more.
"""
import numpy as np
import pytest
import torch

import msda_lattice_cases as LC
from oracle import msda_oracle as orc

pytestmark = pytest.mark.gpu

B_WIN, B_GENERIC, B_COL = 1, 2, 3
K_WIN, K_GENERIC, K_DPP, K_COL = 1, 2, 3, 4
BWD = {B_WIN: "windowed", B_GENERIC: "generic", B_COL: "column"}
FWD = {K_WIN: "windowed", K_GENERIC: "generic", K_DPP: "quad", K_COL: "column"}
WIN_MIN_RECORDS = 32768
GRAD_TOL, FWD_TOL = 2e-5, 1e-4

BWD_RUNS = [(cid, k) for cid in LC.CASE_IDS for k in (B_GENERIC, B_COL, B_WIN)
            if k != B_WIN or LC.records_of(cid) >= WIN_MIN_RECORDS]
FWD_RUNS = [(cid, k) for cid in LC.CASE_IDS for k in (K_GENERIC, K_DPP, K_COL, K_WIN)
            if k != K_WIN or LC.records_of(cid) >= WIN_MIN_RECORDS]


@pytest.fixture(scope="module")
def MSDA():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pctrans_amd import MultiScaleDeformableAttention as m
    return m


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pctrans_amd import _lib
    _lib.prepare_device(torch.device("cuda", torch.cuda.current_device()))
    return _lib.lib()


@pytest.fixture(scope="module")
def T():
    from pctrans_amd import msda_train
    return msda_train


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_want = {}


def reference(cid, what):
    """orc.forward / orc.backward on the case's fp32 operands, computed once per case."""
    if (cid, what) not in _want:
        c = LC.make(cid)
        args = (c["value"], c["shapes"], c["starts"], c["loc"], c["attn"])
        _want[cid, what] = orc.forward(*args) if what == "forward" else orc.backward(*args, LC.grad_out_for(c))
    return _want[cid, what]


def run_bwd(MSDA, lib, c, kernel):
    lib.pct_msda_set_bwd_kernel_choice(kernel)
    try:
        g = MSDA.ms_deform_attn_backward(dev(c["value"]), dev(c["shapes"]), dev(c["starts"]), dev(c["loc"]), dev(c["attn"]),
                                         dev(LC.grad_out_for(c)), 64)
        torch.cuda.synchronize()
        ran = lib.pct_msda_last_bwd_kernel()
    finally:
        lib.pct_msda_set_bwd_kernel_choice(-1)
    assert ran == kernel, "%s ran, not %s" % (BWD.get(ran, ran), BWD[kernel])
    return [t.cpu().numpy() for t in g]


def run_fwd(MSDA, lib, c, kernel):
    lib.pct_msda_set_kernel_choice(kernel)
    try:
        out = MSDA.ms_deform_attn_forward(dev(c["value"]), dev(c["shapes"]), dev(c["starts"]), dev(c["loc"]), dev(c["attn"]), 64)
        torch.cuda.synchronize()
        ran = lib.pct_msda_last_kernel()
    finally:
        lib.pct_msda_set_kernel_choice(-1)
    assert ran == kernel, "%s ran, not %s" % (FWD.get(ran, ran), FWD[kernel])
    return out.cpu().numpy()


# ---------------------------------------------------------------- backward, unfused op
@pytest.mark.parametrize("cid,kernel", BWD_RUNS, ids=["%s-%s" % (c, BWD[k]) for c, k in BWD_RUNS])
def test_backward_on_the_lattice_vs_oracle(MSDA, lib, cid, kernel):
    c = LC.make(cid)
    want = reference(cid, "backward")
    got = run_bwd(MSDA, lib, c, kernel)
    decided = c["decided"]
    keep = {"grad_value": True, "grad_loc": decided[..., None], "grad_attn": decided}
    ratios = {}
    for g, w, name in zip(got, want, ("grad_value", "grad_loc", "grad_attn")):
        assert np.isfinite(g).all(), name
        bound = GRAD_TOL * max(1.0, float(np.abs(w).max()))
        ratios[name] = float(np.where(keep[name], np.abs(g - w), 0.0).max()) / bound
    print("%s %s: error / tolerance  grad_value %.3f  grad_loc %.3f  grad_attn %.3f  (%.4f of the samples undecided)" % (
        cid, BWD[kernel], ratios["grad_value"], ratios["grad_loc"], ratios["grad_attn"], 1.0 - decided.mean()))
    gated = LC.gated_out(c) & decided
    assert gated.any()
    assert np.all(got[1][gated] == 0.0), "grad_loc of %d gated-out samples" % int((got[1][gated] != 0).any(-1).sum())
    assert np.all(got[2][gated] == 0.0), "grad_attn of %d gated-out samples" % int((got[2][gated] != 0).sum())
    assert all(r <= 1.0 for r in ratios.values()), ratios


def test_every_backward_kernel_runs_every_family():
    for k in (B_GENERIC, B_COL, B_WIN):
        families = {LC.make(cid)["family"] for cid, kk in BWD_RUNS if kk == k}
        assert families >= {"lattice", "gate_neighbours", "init_exact", "lattice_nonpow2", "init_nonpow2"}, (BWD[k], families)


@pytest.mark.parametrize("kernel", [B_COL, B_WIN], ids=["column", "windowed"])
def test_backward_on_the_lattice_is_bitwise_repeatable(MSDA, lib, kernel):
    """grad_sampling_loc and grad_attn_weight carry no float atomics in either kernel (tests/test_msda_bwd_col_gpu.py,
    tests/test_msda_fused_train_gpu.py): two calls give the same bits, on the lattice as elsewhere.  (grad_value is flushed by
    float atomics and is not claimed to repeat.)"""
    c = LC.make("lattice-win")
    a, b = run_bwd(MSDA, lib, c, kernel), run_bwd(MSDA, lib, c, kernel)
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("cid,kernel", FWD_RUNS, ids=["%s-%s" % (c, FWD[k]) for c, k in FWD_RUNS])
def test_forward_on_the_lattice_vs_oracle(MSDA, lib, cid, kernel):
    """(The forward is continuous across cells and the gate, so the undecided samples need no mask.)"""
    c = LC.make(cid)
    want = reference(cid, "forward")
    got = run_fwd(MSDA, lib, c, kernel)
    err = float(np.abs(got - want).max())
    print("%s %s: forward error %.2e" % (cid, FWD[kernel], err))
    assert np.isfinite(got).all() and err <= FWD_TOL


@pytest.fixture(scope="module")
def inf_case():
    c = LC.inf_level()
    want = orc.forward(c["value"], c["shapes"], c["starts"], c["loc"], c["attn"])
    assert np.isfinite(want).all()
    return c, want


@pytest.mark.parametrize("kernel", [K_GENERIC, K_DPP, K_COL, K_WIN], ids=[FWD[k] for k in (K_GENERIC, K_DPP, K_COL, K_WIN)])
def test_forward_gate_keeps_an_infinite_level_out(MSDA, lib, inf_case, kernel):
    c, want = inf_case
    got = run_fwd(MSDA, lib, c, kernel)
    assert np.isfinite(got).all(), "%d non-finite outputs: a gated-out sample read the +inf level" % int((~np.isfinite(got)).sum())
    np.testing.assert_allclose(got, want, rtol=0, atol=FWD_TOL)


# ---------------------------------------------------------------- the fused training entry
FUSED_RUNS = [(name, k) for name in LC.FUSED_CASES for k in (B_COL, B_WIN, B_GENERIC)
              if k != B_WIN or LC.FUSED_CASES[name][1] * LC.n_px(LC.FUSED_CASES[name][0]) * LC.M >= WIN_MIN_RECORDS]


def run_entry(T, lib, c, kernel):
    from test_msda_fused_train_gpu import operands
    value, shapes, starts, ref, offsets, logits = operands(c)
    lib.pct_msda_set_bwd_kernel_choice(kernel)
    try:
        gv, goff, glog = T.fused_backward(value, shapes, starts, ref, offsets, logits, dev(c["grad_out"]))
        torch.cuda.synchronize()
        ran = lib.pct_msda_last_bwd_kernel()
    finally:
        lib.pct_msda_set_bwd_kernel_choice(-1)
    assert ran == kernel, "%s ran, not %s" % (BWD.get(ran, ran), BWD[kernel])
    return {"grad_value": gv.cpu().numpy(), "grad_offsets": goff.cpu().numpy(), "grad_logits": glog.cpu().numpy()}


@pytest.mark.parametrize("name,kernel", FUSED_RUNS, ids=["%s-%s" % (n, BWD[k]) for n, k in FUSED_RUNS])
def test_fused_entry_on_the_lattice_vs_float64(T, lib, name, kernel):
    """The reference takes the fp32 location fl(ref + fl(offsets / W)) the entry's expand kernel forms (one rounding of the exact
    sum: asserted by the builder), widened; every sample is decided, and all but the few whose fp32 pixel coordinate is not the
    exact one (`exact`: float64 would see another) are compared."""
    from test_msda_fused_train_gpu import bounds
    c = LC.fused(name)
    want = LC.fused_reference(c)
    got = run_entry(T, lib, c, kernel)
    assert c["decided"].all() and float(c["exact"].mean()) > 0.98
    keep = {"grad_value": True, "grad_offsets": c["exact"][..., None], "grad_logits": True}
    tol, ratios = bounds(c, want), {}
    for key in ("grad_value", "grad_offsets", "grad_logits"):
        g = got[key].astype(np.float64).reshape(want[key].shape)
        assert np.isfinite(g).all(), key
        ratios[key] = float((np.where(keep[key], np.abs(g - want[key]), 0.0) / tol[key]).max())
    print("%s %s fused: error / bound  grad_value %.3f  grad_offsets %.3f  grad_logits %.3f  (%.5f of the samples inexact)" % (
        name, BWD[kernel], ratios["grad_value"], ratios["grad_offsets"], ratios["grad_logits"], 1.0 - c["exact"].mean()))
    gated = LC.gated_out(c)
    assert gated.any() and np.all(got["grad_offsets"][gated] == 0.0)
    assert all(r <= 1.0 for r in ratios.values()), ratios


def test_every_backward_kernel_serves_the_fused_lattice_cases():
    assert {k for _, k in FUSED_RUNS} == {B_COL, B_WIN, B_GENERIC}
    assert {n for n, k in FUSED_RUNS if k == B_WIN} == {"int-win", "init-win"}


@pytest.mark.parametrize("kernel", [B_COL, B_WIN], ids=["column", "windowed"])
def test_fused_entry_on_the_lattice_is_bitwise_repeatable(T, lib, kernel):
    c = LC.fused("int-win")
    a, b = run_entry(T, lib, c, kernel), run_entry(T, lib, c, kernel)
    np.testing.assert_array_equal(a["grad_offsets"], b["grad_offsets"])
    np.testing.assert_array_equal(a["grad_logits"], b["grad_logits"])

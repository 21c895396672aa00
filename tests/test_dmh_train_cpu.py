"""CPU: the float64 restatement of the mask head's backward (dmh_train_reference.backward64, the reference of
test_dmh_train_gpu.py) against torch.autograd.grad of the module's own formulation in float64; the C ABI entry of the HIP
backward (header, library, binding); the decoder's routing of the training path on CPU tensors."""
import os
import re
import subprocess

import pytest
import torch
from torch.nn import functional as F

import dmh_train_reference as R
from test_head_cpu import _small_decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_autograd(mf, ref, prm, gup, stride, rel_coord):
    """The same head written out with differentiable float64 ops and no cast on the way (the module's float64 path rounds the
    relative coordinates to fp32 as the reference does, forward and therefore backward)."""
    mf, ref, prm = (t.detach().clone().requires_grad_(True) for t in (mf, ref, prm))
    N, C, H, W = mf.shape
    w0, w1, w2, b0, b1, b2 = R._split(prm, rel_coord)
    x = torch.relu(torch.matmul(w0, R._inputs(mf, ref, stride, rel_coord)) + b0[..., None])
    x = torch.relu(torch.matmul(w1, x) + b1[..., None])
    logits = (torch.matmul(w2[:, :, None], x) + b2[..., None]).reshape(N, -1, H, W)
    up = F.interpolate(logits, size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
    return torch.autograd.grad((up * gup).sum(), (mf, ref, prm), allow_unused=True)


@pytest.mark.parametrize("rel_coord,N,Q,H,W", [(True, 2, 5, 9, 7), (False, 2, 5, 9, 7), (True, 1, 3, 6, 11), (True, 1, 2, 1, 1)])
def test_backward64_is_autograd_of_the_module_formulation(rel_coord, N, Q, H, W):
    """1e-10 * scale against autograd of the module's formulation.  That formulation casts the relative coordinates to fp32
    in float64 too (`.float()`, as the reference): the reference points here are multiples of 2^-10, so the cast is exact
    on the way in; on the way back it rounds the gradient of the reference points to fp32, so grad_ref is held to 1e-10
    against the same head written without the cast and to 2^-22 against the module."""
    d = _small_decoder(Q=Q, rel_coord=rel_coord).double()
    mf, ref, prm, gup = R.case(N, Q, H, W, seed=11, rel_coord=rel_coord)
    ref = (ref * 1024).round() / 1024
    want = R.autograd_formulation(d, mf, ref, prm, gup, 4, rel_coord)
    plain = _plain_autograd(mf, ref, prm, gup, 4, rel_coord)
    got = R.backward64(mf, ref, prm, gup, 4, rel_coord, chunk=2)
    for name, g, w in zip(("grad_feat", "grad_ref", "grad_params"), got, want):
        assert g.shape == w.shape, name
        scale = max(1.0, float(w.abs().max()))
        tol = 2.0 ** -22 if name == "grad_ref" else 1e-10
        assert float((g - w).abs().max()) <= tol * scale, name
    if rel_coord:
        assert float((got[1] - plain[1]).abs().max()) <= 1e-10 * max(1.0, float(plain[1].abs().max()))
    assert float((got[0] - plain[0]).abs().max()) <= 1e-10 * max(1.0, float(plain[0].abs().max()))
    assert float((got[2] - plain[2]).abs().max()) <= 1e-10 * max(1.0, float(plain[2].abs().max()))


def test_ambiguity_set_and_its_footprint():
    mf, ref, prm, gup = R.case(1, 4, 6, 5, seed=3)
    amb = R.ambiguous_pixels(mf, ref, prm)
    assert amb.shape == (1, 4, 6, 5) and amb.dtype == torch.bool and amb.float().mean() < 0.01
    amb = torch.zeros(1, 1, 6, 5, dtype=torch.bool)
    amb[0, 0, 0, 0] = amb[0, 0, 3, 2] = True
    kept = R.mask_grad_up(torch.ones(1, 1, 12, 10, dtype=torch.float64), amb)[0, 0] == 0
    want = torch.zeros(12, 10, dtype=torch.bool)
    want[0:3, 0:3] = True              # the corner pixel feeds outputs 0, 1 (itself) and 2 (as the lower tap)
    want[5:9, 3:7] = True              # an inner pixel feeds 2x-1 .. 2x+2
    assert torch.equal(kept, want)


def test_abi_declares_exports_and_binds_the_backward():
    from pctrans_amd import _lib
    name = "pct_dynamic_mask_head_backward_f32"
    # pctrans_hip.h holds the entry points with a default call site; the opt-in ones are in the header it includes
    assert '#include "pctrans_hip_train.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    assert re.search(r"PCT_API int %s\(" % name, header)
    assert set(re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)) == set(_lib.OPT_IN_SYMBOLS)
    assert name in _lib.OPT_IN_SYMBOLS and name not in _lib.SYMBOLS and len(_lib.OPT_IN_SYMBOLS[name][0]) == 16
    for sym, (_, _, checked_by) in _lib.OPT_IN_SYMBOLS.items():          # every opt-in entry names the tests that hold it
        assert sym in open(os.path.join(ROOT, checked_by)).read() or "dynamic_mask_head_backward" in open(
            os.path.join(ROOT, checked_by)).read(), sym
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s\b" % name, out)
    fn = getattr(_lib.lib(), name)
    assert fn.argtypes == _lib.OPT_IN_SYMBOLS[name][0]
    assert _lib.lib().pct_abi_version() == 1


def test_cpu_tensors_keep_the_torch_formulation(monkeypatch):
    from pctrans_amd import dynamic_mask_head as dmh
    d = _small_decoder(Q=4)
    assert d.dmh_train == "torch"
    calls = []
    monkeypatch.setattr(dmh, "dynamic_mask_head_train", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError()))
    mf, ref, prm, _ = R.case(2, 4, 8, 8, seed=1)
    mf, ref, prm = mf.float().requires_grad_(True), ref.float().transpose(0, 1), prm.float().transpose(0, 1).requires_grad_(True)
    outs = []
    for mode in ("torch", "hip"):
        d.dmh_train = mode
        up, am = d.dynamic_mask_with_coords(mf, ref, prm, 4, True, (4, 4))
        assert up.requires_grad and up.shape == (2, 4, 16, 16) and am.shape == (2, 1, 4, 16)
        outs.append(up)
    assert not calls and torch.equal(outs[0], outs[1])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        dmh.dynamic_mask_head_backward(mf, ref.transpose(0, 1), prm.transpose(0, 1), torch.zeros(2, 4, 16, 16), 4, True)


def test_switch_default_follows_the_environment(monkeypatch):
    from pctrans_amd import dynamic_mask_head as dmh
    monkeypatch.delenv("PCT_DMH_TRAIN", raising=False)
    assert dmh.train_default() == "torch" and _small_decoder(Q=2).dmh_train == "torch"
    monkeypatch.setenv("PCT_DMH_TRAIN", "hip")
    assert _small_decoder(Q=2).dmh_train == "hip"
    monkeypatch.setenv("PCT_DMH_TRAIN", "triton")
    with pytest.raises(RuntimeError):
        dmh.train_default()

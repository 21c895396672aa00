"""CPU: the C ABI entries of the pixel-embedding loss (header, binding table, exports, argument validation without a launch),
the PCT_EMB_LOSS switch and its routing on CPU tensors, and the float64 reference and the bound of test_embedding_loss_gpu.py
(embedding_loss_reference.py) against the golden fixture and against the criterion's torch formulation in fp32."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import embedding_loss_reference as R
from pctrans_amd import _lib, embedding_loss
from pctrans_amd.loss import maskformer_criterion as crit
from pctrans_amd.loss.matcher import Point_HungarianMatcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pct_instance_label_map_f32", "pct_discriminative_loss_forward_f32", "pct_discriminative_loss_backward_f32")


def _criterion(mode=None):
    c = crit.SetCriterion(1, Point_HungarianMatcher(num_points=16), {}, 0.1, ["embedding"], 16, 3.0, 0.75)
    if mode is not None:
        c.emb_loss = mode
    return c


def _golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "loss_criterion.npz")) as z:
        return {k: z[k] for k in ("emb", "seg_gt", "loss_emb", "grad_emb", "loss_emb_params")}


def test_header_table_and_exports_agree_on_the_three_entries():
    header = open(os.path.join(ROOT, "include", "pctrans_hip_train.h")).read()
    declared = set(re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, nargs in zip(NAMES, (11, 17, 12)):
        assert name in declared and name in _lib.OPT_IN_SYMBOLS and name not in _lib.SYMBOLS
        argtypes, restype, checked_by = _lib.OPT_IN_SYMBOLS[name]
        assert len(argtypes) == nargs and restype is ctypes.c_int and checked_by == "tests/test_embedding_loss_gpu.py"
        assert re.search(r"\bT %s\b" % name, out)
        assert getattr(_lib.lib(), name).argtypes == argtypes
        decl = re.search(r"PCT_API int %s\((.*?)\);" % name, header, re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == nargs
        for p, t in zip(params, argtypes):                          # pointers, ints and floats in the declaration's order
            want = ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float") else ctypes.c_int
            assert t is want, (name, p)
    assert declared == set(_lib.OPT_IN_SYMBOLS) and _lib.ABI_VERSION == 1 and _lib.lib().pct_abi_version() == 1


def test_constants_are_the_kernel_s():
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "embedding_loss.hip")).read()
    for py, name in ((embedding_loss.PIXELS_PER_PASS, "EL_SUB"), (embedding_loss.MAX_CHUNKS, "EL_MAX_CHUNKS"),
                     (embedding_loss.MAX_CHANNELS, "EL_MAX_E"), (embedding_loss.MAX_LABELS, "EL_MAX_L"),
                     (embedding_loss.SLOT, "EL_SLOT"), (embedding_loss.TABLE_ROW, "EL_ROW")):
        assert int(re.search(r"%s = (\d+);" % name, src).group(1)) == py, name
    for pixels in (1, 143, 256, 257, 4087, 64 * 256, 64 * 256 + 1, 130 * 174, 2 ** 31 - 2):
        passes, chunks = embedding_loss.chunks(pixels)
        assert chunks == R.chunks(pixels) and 1 <= chunks <= 64 and passes * chunks * 256 >= pixels > (chunks - 1) * passes * 256


def test_argument_validation_returns_status_codes_without_a_launch():
    L = _lib.lib()
    BAD, ALIGN, UNSUP = -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # host pointer, never dereferenced
    assert p % 16 == 0
    # (planes, num_planes, Ht, Wt, start, count, batch, h, w, labels, stream)
    lm = L.pct_instance_label_map_f32
    assert lm(p, 3, 0, 8, p, p, 2, 4, 4, p, None) == BAD
    assert lm(p, 3, 8, 8, p, p, -1, 4, 4, p, None) == BAD
    assert lm(p, 3, 8, 8, None, p, 2, 4, 4, p, None) == BAD
    assert lm(p, 3, 8, 8, p, p, 2, 4, 4, p + 2, None) == ALIGN
    assert lm(p, 3, 8, 8, p, p, 2, 65536, 65536, p, None) == UNSUP
    assert lm(p, 3, 8, 8, p, p, 0, 4, 4, p, None) == 0
    # (emb, labels, B, E, h, w, L, delta_v, delta_d, alpha, beta, gama, workspace, table, loss, status, stream)
    fwd = L.pct_discriminative_loss_forward_f32
    assert fwd(p, p, 2, 8, 4, 4, 0, 0.5, 3.0, 1.0, 1.0, 0.001, p, p, p, p, None) == BAD
    assert fwd(p, p, 2, 0, 4, 4, 3, 0.5, 3.0, 1.0, 1.0, 0.001, p, p, p, p, None) == BAD
    assert fwd(p, p, 2, 8, 4, 4, 3, 0.5, 3.0, 1.0, 1.0, 0.001, p, None, p, p, None) == BAD
    assert fwd(p, p, 2, 8, 4, 4, 3, 0.5, 3.0, 1.0, 1.0, 0.001, p + 4, p, p, p, None) == ALIGN        # workspace: 16 bytes
    assert fwd(p, p, 2, 8, 4, 4, 3, 0.5, 3.0, 1.0, 1.0, 0.001, p, p, p + 2, p, None) == ALIGN
    assert fwd(p, p, 2, 129, 4, 4, 3, 0.5, 3.0, 1.0, 1.0, 0.001, p, p, p, p, None) == UNSUP
    assert fwd(p, p, 2, 8, 4, 4, 1025, 0.5, 3.0, 1.0, 1.0, 0.001, p, p, p, p, None) == UNSUP
    assert fwd(p, p, 2, 8, 65536, 65536, 3, 0.5, 3.0, 1.0, 1.0, 0.001, p, p, p, p, None) == UNSUP
    # (emb, labels, table, grad_out, B, E, h, w, L, delta_v, grad, stream)
    bwd = L.pct_discriminative_loss_backward_f32
    assert bwd(p, p, p, p, 2, 8, 4, 0, 3, 0.5, p, None) == BAD
    assert bwd(p, p, p, None, 2, 8, 4, 4, 3, 0.5, p, None) == BAD
    assert bwd(p, p, p, p, 2, 8, 4, 4, 3, 0.5, p + 1, None) == ALIGN
    assert bwd(p, p, p, p, 2, 129, 4, 4, 3, 0.5, p, None) == UNSUP
    assert bwd(p, p, p, p, 2, 8, 4, 4, 1025, 0.5, p, None) == UNSUP


def test_switch_default_follows_the_environment(monkeypatch):
    monkeypatch.delenv("PCT_EMB_LOSS", raising=False)
    assert embedding_loss.default() == "torch" and _criterion().emb_loss == "torch"
    monkeypatch.setenv("PCT_EMB_LOSS", "hip")
    assert _criterion().emb_loss == "hip"
    monkeypatch.setenv("PCT_EMB_LOSS", "bogus")
    with pytest.raises(RuntimeError, match="PCT_EMB_LOSS"):
        embedding_loss.default()
    with pytest.raises(RuntimeError):
        _criterion()


def test_cpu_tensors_keep_the_torch_path(monkeypatch):
    for name in ("instance_label_map", "discriminative_loss"):
        monkeypatch.setattr(embedding_loss, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("device path on CPU tensors")))
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(2, 8, 12, 16, generator=g)
    targets = [{"masks": torch.rand(n, 48, 64, generator=g) > 0.7} for n in (3, 5)]
    got = {}
    for mode in ("torch", "hip"):
        x = emb.clone().requires_grad_(True)
        loss = _criterion(mode).loss_embedding(x, targets)["loss_emb"]
        loss.backward()
        got[mode] = (loss.detach(), x.grad)
    assert torch.equal(got["torch"][0], got["hip"][0]) and torch.equal(got["torch"][1], got["hip"][1])
    assert not embedding_loss.supported(emb, 5)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        embedding_loss.discriminative_loss(emb, torch.zeros(2, 12, 16, dtype=torch.int32), 5)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        embedding_loss.instance_label_map(torch.zeros(3, 48, 64), torch.zeros(2, dtype=torch.int32),
                                          torch.zeros(2, dtype=torch.int32), (12, 16))


def test_reference_reproduces_the_golden_fixture():
    """Float64 against values the reference's own function returned in fp32: the tolerances tests/test_criterion_golden.py
    applies to the torch path."""
    g = _golden()
    emb, gt = torch.from_numpy(g["emb"]), torch.from_numpy(g["seg_gt"])
    assert tuple(emb.shape) == (3, 8, 12, 10) and int(gt.max()) == 9
    loss, grad = R.loss64(emb, gt, 9)
    assert abs(loss - float(g["loss_emb"])) <= 2e-5 * abs(float(g["loss_emb"])) + 1e-6
    want = torch.from_numpy(g["grad_emb"]).double()
    assert bool(((grad - want).abs() <= 2e-4 * want.abs() + 1e-7).all())
    other, _ = R.loss64(emb, gt, 9, **R.OTHER_PARAMS)
    assert abs(other - float(g["loss_emb_params"])) <= 2e-5 * abs(float(g["loss_emb_params"])) + 1e-6


def test_reference_is_autograd_of_the_criterion_s_formulation_in_float64():
    for name, E, h, w, L in (("identical instances", 16, 13, 11, 70), ("near and far centroids", 3, 13, 11, 70)):
        emb, lab = R.family(name, E, h, w, L)
        x = emb.double().requires_grad_(True)
        loss = crit.discriminative_loss(x, lab.long(), **R.OTHER_PARAMS)
        grad, = torch.autograd.grad(loss, x)
        want, wgrad = R.loss64(emb, lab, L, **R.OTHER_PARAMS)
        assert abs(float(loss.detach()) - want) <= 1e-12 * max(1.0, abs(want))
        assert float((grad - wgrad).abs().max()) <= 1e-12 * max(1.0, float(wgrad.abs().max()))


@pytest.mark.parametrize("name,E,h,w,L", R.cases())
def test_torch_fp32_stays_inside_the_bound(name, E, h, w, L):
    """The bound is not so tight that the existing fp32 formulation breaks it, on every input the GPU tests run."""
    emb, lab = R.family(name, E, h, w, L)
    want, wgrad, lb, gb = R.expected(name, E, h, w, L)
    loss, grad = R.torch_fp32(emb, lab)
    assert abs(float(loss) - want) <= lb, (float(loss), want, lb)
    excess = (grad.double() - wgrad).abs() - gb
    assert float(excess.max()) <= 0, float(excess.max())
    # and the bound says something: far below the values it guards, the forced cancellation aside
    if name != "offset 100 spread 0.01":
        assert lb <= 1e-3 * max(abs(want), 1e-3)


def test_label_map_reference_is_the_criterion_s():
    g = torch.Generator().manual_seed(2)
    masks = [torch.rand(n, 50, 70, generator=g) > 0.6 for n in (4, 0, 2)]
    got = R.label_map_reference(masks, (13, 18))
    emb = torch.zeros(3, 2, 13, 18)
    seen = []
    real = crit.discriminative_loss
    try:
        crit.discriminative_loss = lambda e, gt, **k: seen.append(gt) or real(e, gt, **k)
        _criterion("torch").loss_embedding(emb, [{"masks": m} for m in masks])
    finally:
        crit.discriminative_loss = real
    assert torch.equal(seen[0], got) and int(got[1].max()) == 0 and int(got.max()) == 4

"""CPU: the C ABI of the device post-processing (header, binding table, exported symbols, argument validation without a
launch), the MaskFormer switch and its default, and the float64 helper of the GPU tests (postprocess_reference.py) against the
literal restatement of the reference's instance_inference (test_arch_cpu._instance_inference_literal)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import postprocess_reference as R
from test_arch_cpu import _instance_inference_literal, instance_logits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pct_instance_masks_f32", "pct_instance_masks_bf16", "pct_instance_labels_from_bits", "pct_instance_labels_f32",
         "pct_instance_labels_bf16"}


def test_header_table_and_library_agree():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_post.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_post.h")).read()
    declared = set(re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header))
    assert declared == NAMES == set(_lib.POST_SYMBOLS)
    assert not NAMES & set(_lib.SYMBOLS) and not NAMES & set(_lib.OPT_IN_SYMBOLS)
    assert "maskformer.py:" in header                                   # the entries cite the reference lines they replace
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name
        assert getattr(_lib.lib(), name).argtypes == _lib.POST_SYMBOLS[name][0]
        assert os.path.exists(os.path.join(ROOT, _lib.POST_SYMBOLS[name][2])), name      # the tests that hold the entry
    assert _lib.lib().pct_abi_version() == 1
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()
    assert "instance_post.hip" in src and "pctrans_hip_post.h" in src


def test_argument_validation_returns_error_codes_without_touching_the_device():
    from pctrans_amd import _lib
    L = _lib.lib()
    BAD, ALIGN, UNSUP = -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # 16-byte aligned host pointer: never dereferenced
    assert p % 16 == 0
    for fn in (L.pct_instance_labels_f32, L.pct_instance_labels_bf16, L.pct_instance_masks_f32, L.pct_instance_masks_bf16):
        assert fn(p, 1, 513, 8, 8, 16, 16, 0, p, p, None) == UNSUP                 # more than 512 queries
        assert fn(p, 1, 100, 8, 8, 2048, 4096, 0, p, p, None) == UNSUP             # 2 H W + 1 >= 2^24
        assert fn(p, 1, 100, 8, 8, 7001, 1000, 0, p, p, None) == UNSUP             # H + W > 8000
        assert fn(p, 1, 100, 8, 8, 16, 16, 2, p, p, None) == BAD                   # unknown dataset
        assert fn(p, -1, 100, 8, 8, 16, 16, 0, p, p, None) == BAD
        assert fn(p, 1, 100, 0, 8, 16, 16, 0, p, p, None) == BAD
        assert fn(None, 1, 100, 8, 8, 16, 16, 0, p, p, None) == BAD
        assert fn(p, 1, 100, 8, 8, 16, 16, 0, p + 4, p, None) == ALIGN             # bits / workspace: 16 bytes
        assert fn(p + 1, 1, 100, 8, 8, 16, 16, 1, p, p, None) == ALIGN             # logits: their element size
        assert fn(p, 0, 100, 8, 8, 16, 16, 0, p, p, None) == 0                     # empty batch: OK, no launch
        assert fn(None, 0, 100, 8, 8, 16, 16, 1, None, None, None) == 0
    assert L.pct_instance_masks_f32(p, 1, 100, 8, 8, 16, 16, 0, p, p + 2, None) == ALIGN      # areas: 4 bytes
    assert L.pct_instance_labels_f32(p, 1, 100, 8, 8, 16, 16, 0, p, p + 1, None) == ALIGN     # labels: 2 bytes
    fb = L.pct_instance_labels_from_bits
    assert fb(p, p, 1, 513, 16, 16, 0, p, p, None) == UNSUP
    assert fb(p, p, 1, 100, 4096, 2048, 1, p, p, None) == UNSUP
    assert fb(p, p, 70000, 100, 16, 16, 1, p, p, None) == UNSUP
    assert fb(p + 4, p, 1, 100, 16, 16, 0, p, p, None) == ALIGN
    assert fb(p, p, 1, 100, 16, 16, 0, p + 8, p, None) == ALIGN
    assert fb(p, None, 1, 100, 16, 16, 0, p, p, None) == BAD
    assert fb(p, p, 0, 100, 16, 16, 0, p, p, None) == 0


def _net(dataset="CVPPP", head=None):
    from pctrans_amd.arch import maskformer as mfm
    return mfm.MaskFormer(backbone=torch.nn.Identity(), sem_seg_head=head or torch.nn.Identity(),
                          criterion=torch.nn.Identity(), num_queries=4, dataset_name=dataset)


def test_default_is_torch_and_follows_the_environment(monkeypatch):
    from pctrans_amd import postprocess as post
    monkeypatch.delenv("PCT_POSTPROCESS", raising=False)
    assert post.default() == "torch" and _net().postprocess == "torch"
    monkeypatch.setenv("PCT_POSTPROCESS", "hip")
    assert _net().postprocess == "hip"
    monkeypatch.setenv("PCT_POSTPROCESS", "triton")
    with pytest.raises(RuntimeError, match="PCT_POSTPROCESS"):
        post.default()
    with pytest.raises(RuntimeError, match="PCT_POSTPROCESS"):
        _net()


class _StubHead(torch.nn.Module):
    def __init__(self, masks):
        super().__init__()
        self.masks = masks

    def forward(self, features):
        return {"pred_masks": self.masks}, None


@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_cpu_tensors_keep_the_torch_path(dataset, monkeypatch):
    from pctrans_amd import postprocess as post
    monkeypatch.setattr(post, "instance_labels", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device path taken")))
    logits = instance_logits()[None]
    outs = []
    for mode in ("torch", "hip"):
        net = _net(dataset, _StubHead(logits)).eval()
        net.postprocess = mode
        out, bd = net(torch.zeros(1, 3, 96, 88))
        assert bd is None and out.dtype == torch.int16 and out.shape == (1, 96, 88)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    net.postprocess = "cuda"
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 96, 88))
    monkeypatch.undo()
    for fn in (post.instance_labels, post.instance_masks):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(logits, (96, 88), dataset)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        post.instance_labels_from_bits(torch.zeros(1, 14, 264, dtype=torch.int32), torch.zeros(1, 14, dtype=torch.int32),
                                       (96, 88), dataset)


def test_workspace_formula_and_bit_format():
    from pctrans_amd import postprocess as post
    assert post.plane_words(96, 88) == R.plane_words(96, 88) == 264 and post.plane_words(512, 512) == 8192
    nq, pw = 300, post.plane_words(520, 696)
    assert post.workspace_bytes(3, 100, 520, 696, with_masks=False) == 4 * (nq * pw + nq * 100 + nq * 4 + 5 * nq + 12)
    assert post.workspace_bytes(1, 14, 96, 88) == 4 * (2 * 14 * 264 + 196 + 16 + 6 * 16 + 4)
    g = torch.Generator().manual_seed(1)
    m = torch.rand(2, 3, 9, 7, generator=g) < 0.4
    bits = R.pack_bits(m)
    assert bits.shape == (2, 3, 4) and bits.dtype == torch.int32
    back, pad = R.unpack_bits(bits, 9, 7)
    assert torch.equal(back, m) and not pad.any()
    assert ((int(bits[1, 2, 1]) >> 3) & 1) == int(m[1, 2].flatten()[35])


@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_float64_helper_equals_the_literal_restatement(dataset):
    logits = instance_logits()
    want = _instance_inference_literal(logits, dataset)[0]
    x64 = R.resize64(logits, (96, 88))
    assert x64.dtype == torch.float64 and torch.equal(x64, logits.double())
    masks = R.threshold64(x64, dataset)
    assert torch.equal(masks, logits.sigmoid().float() > R.PARAMS[dataset]["t"])        # no pixel of this case sits on the threshold
    got, info = R.labels_from_masks(masks, dataset)
    assert got.dtype == torch.int16 and torch.equal(got, want)
    assert torch.equal(R.instance_labels64(logits, (96, 88), dataset), want)
    assert R.areas_distinct(info, dataset) and len(info["areas"]) == int(want.max())
    m = info["margins"]
    assert m["dice"] > 1e-4 and (dataset == "BBBC" or (m["mean"] > 1e-4 and m["nms"] > 1e-4))
    band = R.ambiguous_band(x64, dataset, logits.abs().max())
    assert band.shape == masks.shape and float(band.double().mean()) <= 1e-3


def test_resize64_is_bilinear_without_aligned_corners():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 12, 10, generator=g, dtype=torch.float64)
    for size in ((24, 20), (31, 17), (12, 10), (7, 9)):
        want = torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False)
        assert float((R.resize64(x, size) - want).abs().max()) < 1e-12, size
    assert abs(R.logit_threshold("CVPPP") - 0.8001193) < 1e-6 and abs(R.logit_threshold("BBBC") + 2.9444390) < 1e-6

"""CPU: the C ABI of the pixel decoder's FPN level on the device (header, binding table, exported symbol, argument validation
without a launch), what fused_ops.fpn_stage_supported refuses, the decoder's `fpn` switch and its default, and the identity
the first kernel rests on: at the exact ratio 2 the bilinear resize (align_corners=False) is the 2 x 2 mean."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pct_fpn_stage_f32"}


def test_header_table_and_library_agree():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_fpn.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_fpn.h")).read()
    declared = set(re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header))
    assert declared == NAMES == set(_lib.FPN_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.SEG_SYMBOLS):
        assert not NAMES & set(other)
    assert "msdeformattn.py:" in header                                 # the entry cites the lines it replaces
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name
        assert getattr(_lib.lib(), name).argtypes == _lib.FPN_SYMBOLS[name][0]
        assert len(_lib.FPN_SYMBOLS[name][0]) == 27 and getattr(_lib.lib(), name).restype is ctypes.c_int
        assert os.path.exists(os.path.join(ROOT, _lib.FPN_SYMBOLS[name][2])), name      # the tests that hold the entry
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()
    assert "fpn_stage.hip" in src and "pctrans_hip_fpn.h" in src


def test_argument_validation_returns_error_codes_without_touching_the_device():
    from pctrans_amd import _lib
    fn = _lib.lib().pct_fpn_stage_f32
    BAD, ALIGN, UNSUP = -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # 16-byte aligned host pointer: never dereferenced
    assert p % 16 == 0

    def call(x=p, enc=p, stride=128 * 8 * 8, cl=0, lat=None, outc=None, ws=p, y=p, n=1, k=64, c=128, h=8, w=8, out=p):
        lat = lat if lat is not None else [p, p, None, None, None, None, 0.0]
        outc = outc if outc is not None else [p, None, p, p, p, p, 1e-5]
        return fn(x, enc, stride, cl, *lat, *outc, ws, y, n, k, c, h, w, out, None)

    assert call(n=0) == 0                                            # empty batch: OK, no launch
    assert call(n=0, x=None, enc=None, ws=None, y=None, out=None) == 0
    assert call(n=-1) == BAD and call(h=0) == BAD and call(w=0) == BAD and call(k=0) == BAD and call(c=0) == BAD
    assert call(stride=128 * 8 * 8 - 1) == BAD                       # images of enc overlap
    for name in ("x", "enc", "ws", "y", "out"):
        assert call(**{name: None}) == BAD, name
    assert call(lat=[None, p, None, None, None, None, 0.0]) == BAD   # no weights
    assert call(outc=[p, None, p, None, p, p, 1e-5]) == BAD          # half a norm
    assert call(outc=[p, None, None, p, p, p, 1e-5]) == BAD
    assert call(lat=[p, p, p, p, p, None, 1e-5]) == BAD
    assert call(c=64, stride=64 * 8 * 8) == UNSUP                    # channels != 128
    assert call(k=24) == UNSUP                                       # in_channels % 16
    assert call(h=4096, w=4096, stride=128 * 4096 * 4096) == UNSUP   # 2^24 pixels
    assert call(x=p + 4) == ALIGN and call(ws=p + 8) == ALIGN and call(y=p + 4) == ALIGN and call(out=p + 2) == ALIGN
    assert call(enc=p + 2) == ALIGN and call(enc=p + 4, cl=1) == ALIGN and call(cl=1, stride=128 * 8 * 8 + 2) == ALIGN
    assert call(lat=[p + 2, p, None, None, None, None, 0.0]) == ALIGN
    assert call(outc=[p, None, p, p + 1, p, p, 1e-5]) == ALIGN
    assert b"" != _lib.lib().pct_error_string(UNSUP)


def _convs(norm, cin=16):
    from pctrans_amd.layers import Conv2d, get_norm
    lat = Conv2d(cin, 128, kernel_size=1, bias=norm == "", norm=get_norm(norm, 128))
    outc = Conv2d(128, 128, kernel_size=3, stride=1, padding=1, bias=norm == "", norm=get_norm(norm, 128), activation=F.relu)
    return lat.eval(), outc.eval()


def test_supported_refuses_what_the_kernels_do_not_cover(monkeypatch):
    """Evaluated with tensors that claim to be on the device (meta tensors cannot: the device checks come first, so the CPU cases
    are real and the rest patch nothing but `is_cuda`)."""
    from pctrans_amd import fused_ops
    x, enc = torch.randn(1, 16, 8, 12), torch.randn(1, 128, 4, 6)
    for norm in ("", "BN", "FrozenBN", "GN"):
        lat, outc = _convs(norm)
        with torch.no_grad():
            assert not fused_ops.fpn_stage_supported(x, enc, lat, outc)              # CPU tensors
    # the module-side conditions, on the objects alone
    assert fused_ops._fpn_norm_tensors(None) == ()
    lat, outc = _convs("GN")
    assert fused_ops._fpn_norm_tensors(lat.norm) is None                              # GroupNorm
    assert fused_ops._fpn_conv_tensors(lat, 16, 1, 0) is None
    lat, outc = _convs("LN")
    assert fused_ops._fpn_norm_tensors(outc.norm) is None                             # LayerNorm2d
    lat, outc = _convs("BN")
    assert len(fused_ops._fpn_conv_tensors(lat, 16, 1, 0)) == 5 and len(fused_ops._fpn_conv_tensors(outc, 128, 3, 1)) == 5
    outc.train()
    assert fused_ops._fpn_norm_tensors(outc.norm) is None                             # batch statistics
    assert fused_ops._fpn_conv_tensors(outc, 128, 3, 1) is None
    lat, outc = _convs("FrozenBN")
    assert len(fused_ops._fpn_conv_tensors(lat, 16, 1, 0)) == 5
    lat, outc = _convs("")
    assert len(fused_ops._fpn_conv_tensors(lat, 16, 1, 0)) == 2                        # weight and bias
    assert fused_ops._fpn_conv_tensors(lat, 32, 1, 0) is None                          # another channel count
    assert fused_ops._fpn_conv_tensors(lat, 16, 3, 1) is None                          # another kernel size
    lat.bias = None
    assert fused_ops._fpn_conv_tensors(lat, 16, 1, 0) is None                          # neither norm nor bias


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda with True: lets the shape, layout and autograd conditions of fpn_stage_supported be
    evaluated on a machine without a device (nothing is launched by that function)."""
    @property
    def is_cuda(self):
        return True


def _dev(t):
    return t.as_subclass(_OnDevice)


def _dev_convs(norm, cin=16):
    lat, outc = _convs(norm, cin)
    for m in (lat, outc):
        for name, p in list(m.named_parameters()):
            mod = m.norm if name.startswith("norm.") else m
            rg = p.requires_grad
            mod._parameters[name.split(".")[-1]] = _dev(p.detach()).requires_grad_(rg)
        for name, b in list(m.named_buffers()):
            if b.dtype == torch.float32:
                (m.norm)._buffers[name.split(".")[-1]] = _dev(b)
    return lat, outc


def test_supported_follows_shape_mode_and_autograd():
    from pctrans_amd import fused_ops
    x, enc = _dev(torch.randn(1, 16, 8, 12)), _dev(torch.randn(1, 128, 4, 6))
    for norm in ("", "BN", "FrozenBN"):
        lat, outc = _dev_convs(norm)
        with torch.no_grad():
            assert fused_ops.fpn_stage_supported(x, enc, lat, outc), norm
            assert not fused_ops.fpn_stage_supported(_dev(torch.randn(1, 16, 8, 13)), enc, lat, outc)       # not 2x
            assert not fused_ops.fpn_stage_supported(_dev(torch.randn(1, 16, 12, 18)), enc, lat, outc)      # 3x
            assert not fused_ops.fpn_stage_supported(_dev(torch.randn(1, 16, 4, 6)), enc, lat, outc)        # 1x
            assert not fused_ops.fpn_stage_supported(x.double(), enc, lat, outc)
            assert not fused_ops.fpn_stage_supported(x, _dev(torch.randn(1, 128, 6, 4)).transpose(2, 3), lat, outc)
        # gradients enabled: the parameters (or, without any, the inputs) require grad
        assert lat.weight.requires_grad and not fused_ops.fpn_stage_supported(x, enc, lat, outc)
        for p in list(lat.parameters()) + list(outc.parameters()):
            p.requires_grad_(False)
        assert fused_ops.fpn_stage_supported(x, enc, lat, outc)
        assert not fused_ops.fpn_stage_supported(_dev(x.detach().clone()).requires_grad_(), enc, lat, outc)
        assert not fused_ops.fpn_stage_supported(x, _dev(enc.detach().clone()).requires_grad_(), lat, outc)
    with torch.no_grad():
        lat, outc = _dev_convs("GN")
        assert not fused_ops.fpn_stage_supported(x, enc, lat, outc)
        lat, outc = _dev_convs("BN")
        outc.train()
        assert not fused_ops.fpn_stage_supported(x, enc, lat, outc)
        lat, outc = _dev_convs("BN")
        outc.activation = None
        assert not fused_ops.fpn_stage_supported(x, enc, lat, outc)
        lat, outc = _dev_convs("BN")
        lat.activation = F.relu
        assert not fused_ops.fpn_stage_supported(x, enc, lat, outc)
        # the channels-last view of token rows at a row offset, images further apart than H * W * 128
        lat, outc = _dev_convs("BN")
        tokens = torch.randn(2, 40, 128)
        view = _dev(tokens[:, 16:].transpose(1, 2).reshape(2, 128, 4, 6))
        assert view.stride() == (40 * 128, 1, 6 * 128, 128) and not view.is_contiguous()
        assert fused_ops.fpn_stage_supported(_dev(torch.randn(2, 16, 8, 12)), view, lat, outc)


def _pixel_decoder(norm="BN"):
    from pctrans_amd.layers import ShapeSpec
    from pctrans_amd.pixel_decoder.msdeformattn import MSDeformAttnPixelDecoder
    shapes = {k: ShapeSpec(channels=c, stride=s) for k, c, s in (("res2", 16, 4), ("res3", 24, 8), ("res4", 32, 16),
                                                                 ("res5", 40, 32))}
    return MSDeformAttnPixelDecoder(shapes, transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=64,
                                    transformer_enc_layers=1, conv_dim=128, mask_dim=16, norm=norm,
                                    transformer_in_features=["res3", "res4", "res5"], common_stride=4)


def test_default_is_torch_and_follows_the_environment(monkeypatch):
    from pctrans_amd import fused_ops
    monkeypatch.delenv("PCT_FPN", raising=False)
    assert fused_ops.fpn_default() == "torch" and _pixel_decoder().fpn == "torch"
    monkeypatch.setenv("PCT_FPN", "")
    assert _pixel_decoder().fpn == "torch"
    monkeypatch.setenv("PCT_FPN", "hip")
    pix = _pixel_decoder()
    assert pix.fpn == "hip" and "fpn" not in pix.state_dict() and "fpn" not in dict(pix.named_buffers())
    monkeypatch.setenv("PCT_FPN", "triton")
    with pytest.raises(RuntimeError, match="PCT_FPN"):
        _pixel_decoder()


def test_hip_switch_on_the_cpu_runs_the_torch_statements(monkeypatch):
    """fpn = "hip" with CPU tensors: nothing is supported, the loop's torch statements run and the library is not entered."""
    from pctrans_amd import fused_ops
    from pctrans_amd.pixel_decoder.ops.modules import ms_deform_attn as msda_mod
    monkeypatch.setattr(msda_mod, "_ALLOW_CPU_REFERENCE", True)      # the encoder's sampling in its torch formulation
    torch.manual_seed(3)
    pix = _pixel_decoder().eval()
    feats = {"res2": torch.randn(1, 16, 8, 12), "res3": torch.randn(1, 24, 4, 6), "res4": torch.randn(1, 32, 2, 3),
             "res5": torch.randn(1, 40, 1, 2)}
    with torch.no_grad():
        want = pix.forward_features(feats)
        pix.fpn = "hip"
        monkeypatch.setattr(fused_ops, "fpn_stage", lambda *a: (_ for _ in ()).throw(AssertionError("HIP path taken")))
        got = pix.forward_features(feats)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert all(torch.equal(a, b) for a, b in zip(got[2], want[2]))


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (17, 23), (64, 64), (65, 87)])
def test_bilinear_resize_by_two_is_the_2x2_mean(H, W):
    """The identity the first kernel rests on, in fp32 and fp64: F.interpolate(x, (H, W), bilinear, align_corners=False) of a
    2H x 2W map samples at the centre of each 2 x 2 block with weights 1/4 (exact in binary), i.e. avg_pool2d(x, 2)."""
    g = torch.Generator().manual_seed(H * 100 + W)
    for dtype in (torch.float32, torch.float64):
        x = torch.randn(2, 3, 2 * H, 2 * W, generator=g, dtype=dtype)
        a = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
        b = F.avg_pool2d(x, 2)
        assert float((a - b).abs().max()) <= 2.0 ** (-22 if dtype == torch.float32 else -50) * float(x.abs().max())
    x = torch.randint(-8, 9, (1, 2, 2 * H, 2 * W), generator=g).float()                 # exactly representable sums
    assert torch.equal(F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False), F.avg_pool2d(x, 2))

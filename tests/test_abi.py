"""CPU: the C-ABI library builds/loads and exports every symbol include/pctrans_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    return sorted(set(re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", hdr)))


def test_header_declares_expected_entry_points():
    syms = _declared_symbols()
    for s in ("pct_abi_version", "pct_error_string", "pct_ms_deform_attn_forward_f32",
              "pct_ms_deform_attn_forward_f64", "pct_ms_deform_attn_forward_f16", "pct_ms_deform_attn_forward_bf16",
              "pct_ms_deform_attn_backward_f32", "pct_ms_deform_attn_backward_f64"):
        assert s in syms


def test_library_exports_every_declared_symbol():
    from pctrans_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: make -C pctrans_amd/csrc"
    l = ctypes.CDLL(_lib.LIB_PATH)
    for s in _declared_symbols():
        assert hasattr(l, s), "libpctrans_hip.so does not export " + s
    assert set(_lib.SYMBOLS) == set(_declared_symbols()), "ctypes table and header disagree"
    assert _lib.lib().pct_abi_version() == _lib.ABI_VERSION
    assert b"im2col_step" in _lib.lib().pct_error_string(-2)


def test_kernel_sources_carry_no_build_switches_or_launch_overrides():
    """The shipped kernels are the only kernels: no compile-time switch can select another variant (the knock-out timing
    builds, which gave wrong results by design, are gone with them), and the environment selects nothing but the
    documented kernel choices and the two test hooks.  The glue between them is declared once: launchers.hpp alone holds the
    prototypes of the launch_* / prepare_* functions and the value of the internal "not covered" status."""
    csrc = os.path.join(ROOT, "pctrans_amd", "csrc")
    names = set()
    # a launch_* / prepare_* function declared at file scope and not defined (an explicit instantiation starts with `template`)
    proto = re.compile(r"^(?!template\b)(?=\S)[\w:<>\*&, ]*?\b((?:launch|prepare)_\w+)\s*\([^;{}]*\)\s*;", re.M)
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".hpp", ".h")):
            continue
        src = open(os.path.join(csrc, f)).read()
        assert "PCT_EXPERIMENT_BUILD" not in src, f
        assert not re.search(r"#\s*ifn?def\s+(PCT|FZ)_", src), f
        names.update(re.findall(r"getenv\(\s*\"(\w+)\"", src))
        if f == "launchers.hpp":
            assert len(proto.findall(src)) >= 25 and re.search(r"PCT_NOT_COVERED = -100;", src), f
            continue
        assert not re.search(r"-\s*100\b", src), f
        if f.endswith(".hip"):
            assert not proto.findall(src), (f, proto.findall(src))
            assert '#include "launchers.hpp"' in src, f
    assert names == {"PCT_MSDA_KERNEL", "PCT_MSDA_BWD_KERNEL", "PCT_WIN_QUEUE", "PCT_BCOL_FLAG_CAP", "PCT_LIN_KERNEL"}, names
    from pctrans_amd import _lib
    assert _lib.lib().pct_build_info() == b"target=gfx950"


def test_missing_library_fails_loudly(monkeypatch):
    from pctrans_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libpctrans_hip.so")
    with pytest.raises(_lib.PctransLibraryError):
        _lib.lib()


SWITCHES = [("point_loss", "default", "PCT_POINT_LOSS", "torch"), ("point_loss", "select_default", "PCT_POINT_SELECT", "torch"),
            ("point_loss", "match_cost_default", "PCT_MATCH_COST", "torch"), ("postprocess", "default", "PCT_POSTPROCESS", "torch"),
            ("msda_train", "default", "PCT_MSDA_TRAIN", "torch"), ("embedding_loss", "default", "PCT_EMB_LOSS", "torch"),
            ("attention_train", "default", "PCT_ATTN_TRAIN", "torch"), ("targets", "default", "PCT_TARGETS", "hip"),
            ("metrics", "default", "PCT_METRICS", "hip"), ("dynamic_mask_head", "train_default", "PCT_DMH_TRAIN", "torch"),
            ("reid_dice", "default", "PCT_REID_DICE", "torch"), ("reid_query", "default", "PCT_REID_QUERY", "torch"),
            ("reid_query", "contrast_default", "PCT_CONTRAST_LOSS", "torch"), ("fused_ops", "fpn_default", "PCT_FPN", "torch")]


@pytest.mark.parametrize("module,function,variable,unset", SWITCHES)
def test_every_hip_torch_switch_keeps_its_default_and_its_message(monkeypatch, module, function, variable, unset):
    """The process defaults of the opt-in device paths (one rule, pctrans_amd/_lib.py: env_switch): unset or empty gives the
    module's default, 'hip' and 'torch' are taken, anything else raises with the variable's name and the value."""
    import importlib
    default = getattr(importlib.import_module("pctrans_amd." + module), function)
    for value, want in ((None, unset), ("", unset), ("hip", "hip"), ("torch", "torch")):
        monkeypatch.delenv(variable, raising=False) if value is None else monkeypatch.setenv(variable, value)
        assert default() == want
    monkeypatch.setenv(variable, "triton")
    with pytest.raises(RuntimeError, match=re.escape("%s must be 'hip' or 'torch', got 'triton'" % variable)):
        default()


def test_cpu_tensors_raise_like_the_reference_extension():
    import torch
    from pctrans_amd import MultiScaleDeformableAttention as MSDA
    v = torch.zeros(1, 4, 1, 4)
    shapes = torch.tensor([[2, 2]])
    starts = torch.tensor([0])
    loc = torch.zeros(1, 1, 1, 1, 1, 2)
    w = torch.zeros(1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_forward(v, shapes, starts, loc, w, 64)
    with pytest.raises(RuntimeError, match="contiguous"):
        MSDA.ms_deform_attn_forward(v.expand(2, 4, 1, 4).transpose(0, 1), shapes, starts, loc, w, 64)


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under pctrans_amd/ may reference it."""
    bad = []
    for d, _, files in os.walk(os.path.join(ROOT, "pctrans_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")) or f == "Makefile":
                txt = open(os.path.join(d, f)).read()
                if re.search(r"\boracle\b", txt) and not f.endswith(".md"):
                    for line in txt.splitlines():
                        if re.search(r"(import|from|include|CDLL|-l).*\boracle", line):
                            bad.append((f, line.strip()))
    assert not bad, bad


def test_argument_validation_returns_error_codes_without_touching_the_device():
    """Bad arguments are rejected on the host (no launch, so this runs without a GPU): the C ABI reports errors through
    return codes, never by printing (the reference printf()s launch failures, cuh:953-957)."""
    from pctrans_amd import _lib
    L = _lib.lib()
    BAD, UNSUP, ALIGN = -1, -4, -3
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # 16-byte aligned host pointer: never dereferenced
    assert p % 16 == 0
    # linear_k128: negative rows, n not a multiple of 32, misaligned x, row stride below K
    assert L.pct_linear_k128_f32(p, 128, None, 0, 0, p, p, -1, 128, 0, p, 128, None) == BAD
    assert L.pct_linear_k128_f32(p, 128, None, 0, 0, p, p, 8, 100, 0, p, 100, None) == UNSUP
    assert L.pct_linear_k128_f32(p + 4, 128, None, 0, 0, p, p, 8, 128, 0, p, 128, None) == ALIGN
    assert L.pct_linear_k128_f32(p, 64, None, 0, 0, p, p, 8, 128, 0, p, 128, None) == BAD
    assert L.pct_linear_k128_f32(p, 128, p, 128, 8, p, p, 64, 128, 0, p, 128, None) == BAD      # add_period < 32
    assert L.pct_linear_k128_f32(p, 128, None, 0, 0, p, p, 0, 128, 0, p, 128, None) == 0        # empty: OK, no launch
    # fused output_proj + LayerNorm: missing residual
    assert L.pct_linear_k128_add_layernorm_f32(p, 128, p, p, None, 128, p, p, 1e-5, 8, p, 128, None) == BAD
    # GroupNorm + flatten: channels other than 128, groups that do not divide into multiples of 4 channels
    assert L.pct_groupnorm_flatten_f32(p, p, p, 1, 64, 16, 32, 1e-5, p, p, 2048, 0, None) == UNSUP
    assert L.pct_groupnorm_flatten_f32(p, p, p, 1, 128, 16, 64, 1e-5, p, p, 2048, 0, None) == UNSUP
    assert L.pct_groupnorm_flatten_f32(p, p, p, 0, 128, 16, 32, 1e-5, p, p, 2048, 0, None) == 0
    # add + LayerNorm: unsupported width
    assert L.pct_add_layernorm_f32(p, None, p, p, 1e-5, 4, 96, p, None) == UNSUP
    assert b"" != L.pct_error_string(UNSUP)

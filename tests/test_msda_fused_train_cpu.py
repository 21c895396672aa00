"""CPU: the float64 reference of the differentiable fused MSDeformAttn front-end (tests/msda_fused_reference.py) against torch
autograd, the properties of its cases that the GPU tests rely on, the ABI declaration of the entry, and the host logic of
pctrans_amd/msda_train.py and of MSDeformAttn.train_front (no device call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import msda_fused_reference as R
from conftest import ROOT

NAME = "pct_ms_deform_attn_fused_backward_f32"


def _torch_chain(c):
    """The module's torch chain in float64 with autograd through the dense formulation: out and the three gradients."""
    from pctrans_amd.pixel_decoder.ops.functions import ms_deform_attn_core_pytorch
    N, S, M, D, L, Lq, P = c["dims"]
    value = torch.from_numpy(c["value"]).double().requires_grad_()
    offsets = torch.from_numpy(c["offsets"]).double().requires_grad_()
    logits = torch.from_numpy(c["logits"]).double().requires_grad_()
    ref = torch.from_numpy(c["ref"]).double()
    shapes = torch.from_numpy(c["shapes"])
    w = torch.softmax(logits, -1).view(N, Lq, M, L, P)
    normalizer = torch.stack([shapes[..., 1], shapes[..., 0]], -1)
    loc = ref[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
    out = ms_deform_attn_core_pytorch(value, shapes, loc, w)
    out.backward(torch.from_numpy(c["grad_out"]).double())
    return [t.detach().numpy() for t in (out, value.grad, offsets.grad, logits.grad)]


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_equals_torch_autograd_in_float64(name):
    c = R.make(name)
    out, gv, goff, glog = _torch_chain(c)
    ref = R.backward(c)
    for got, want, what in ((out, R.forward(c), "out"), (gv, ref["grad_value"], "grad_value"),
                            (goff, ref["grad_offsets"], "grad_offsets"), (glog, ref["grad_logits"], "grad_logits")):
        err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
        print("%s %s: |torch - reference| %.2e of %.2e" % (name, what, err, top))
        assert top > 0 and err <= 1e-12 * top, (name, what, err, top)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_conditions_the_gpu_tests_rely_on(name):
    """Few samples sit on a cell boundary (they are left out of the grad_offsets comparison), and on the 2 px cases most samples
    are inside their map and have a location gradient to compare."""
    c = R.make(name)
    edge = float(R.edge_mask(c).mean())
    live = float((np.abs(R.backward(c)["gloc"]).max(-1) > 0).mean())
    gated = float(R.gated_out(c).mean())
    print("%s: edge share %.4f, samples with a location gradient %.3f, gated out %.3f" % (name, edge, live, gated))
    assert edge < 0.01
    assert np.all(R.backward(c)["gloc"][R.gated_out(c)] == 0)
    if name in R.TWO_PX_CASES:
        assert live >= 0.5
    if name == "far_offsets":
        assert gated > 0.5
    if name == "peaked":
        N, S, M, D, L, Lq, P = c["dims"]
        assert float((R.backward(c)["w"].reshape(-1, L * P).max(-1) > 0.9).mean()) > 0.5      # near-one-hot rows
    if name == "lq37_p8":
        N, S, M, D, L, Lq, P = c["dims"]
        assert Lq != S and (N * Lq * M) % 64 != 0 and N * Lq * M > 64


def test_header_table_and_library_agree():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_msda_train.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_msda_train.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert declared == [NAME] == list(_lib.MSDA_TRAIN_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.SEG_SYMBOLS, _lib.FPN_SYMBOLS, _lib.ATTN_TRAIN_SYMBOLS,
                  _lib.REID_SYMBOLS, _lib.TARGETS_SYMBOLS):
        assert NAME not in other
    argtypes, restype, checked_by = _lib.MSDA_TRAIN_SYMBOLS[NAME]
    assert os.path.exists(os.path.join(ROOT, checked_by)), checked_by
    # the declaration's parameter list and the table: 21 arguments, ref_batch_stride the one long long
    params = re.search(re.escape(NAME) + r"\s*\(([^)]*)\)", header).group(1).split(",")
    assert len(params) == len(argtypes) == 21
    assert [i for i, p in enumerate(params) if "long long" in p] == [i for i, a in enumerate(argtypes) if a is ctypes.c_longlong] == [4]
    assert [i for i, p in enumerate(params) if re.match(r"\s*int\s+\w+$", p)] == [i for i, a in enumerate(argtypes) if a is ctypes.c_int]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    fn = getattr(_lib.lib(), NAME)
    assert fn.argtypes == argtypes and fn.restype is ctypes.c_int and restype is ctypes.c_int
    assert _lib.ABI_VERSION == 1 and _lib.lib().pct_abi_version() == 1
    makefile = open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()
    assert " msda_fused_backward.hip " in makefile and "pctrans_hip_msda_train.h" in makefile


def test_entry_validates_its_arguments_without_touching_the_device():
    from pctrans_amd import _lib
    BAD, STEP, ALIGN, UNSUP = -1, -2, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                    # 16-byte aligned host pointer: never dereferenced
    assert p % 16 == 0
    fn = _lib.lib().pct_ms_deform_attn_fused_backward_f32

    def call(value=p, ref=p, stride=0, offsets=p, logits=p, go=p, N=2, S=21, M=8, D=16, L=3, Lq=21, P=4, step=128, ws=p, gv=p,
             goff=p, glog=p):
        return fn(value, p, p, ref, stride, offsets, logits, go, N, S, M, D, L, Lq, P, step, ws, gv, goff, glog, None)

    assert call(N=0) == 0 and call(Lq=0) == 0                                  # empty: PCT_OK, nothing launched
    assert call(L=17) == UNSUP and call(L=9, P=8) == UNSUP                      # L * P > 64
    assert call(L=3, P=2) == UNSUP and call(L=4, P=3) == UNSUP                  # L * P % 4, odd P
    assert call(S=2 ** 24, M=8, D=16) == UNSUP                                  # what the unfused backward refuses
    assert call(N=3, step=2) == STEP
    assert call(ws=None) == BAD and call(ref=None) == BAD and call(goff=None) == BAD and call(stride=-1) == BAD
    assert call(M=0) == BAD
    for k in ("offsets", "logits", "ws", "goff", "glog"):
        assert call(**{k: p + 4}) == ALIGN, k
    assert call(gv=p + 2) == ALIGN


def test_default_reads_the_environment(monkeypatch):
    from pctrans_amd import msda_train
    monkeypatch.delenv("PCT_MSDA_TRAIN", raising=False)
    assert msda_train.default() == "torch"
    for v in ("hip", "torch"):
        monkeypatch.setenv("PCT_MSDA_TRAIN", v)
        assert msda_train.default() == v
    monkeypatch.setenv("PCT_MSDA_TRAIN", "")
    assert msda_train.default() == "torch"
    monkeypatch.setenv("PCT_MSDA_TRAIN", "HIP")
    with pytest.raises(RuntimeError, match="PCT_MSDA_TRAIN"):
        msda_train.default()
    assert msda_train.workspace_bytes(2, 336, 8, 3, 4) == 12 * 2 * 336 * 8 * 12


def _module_inputs(c, d_model=128):
    N, S, M, D, L, Lq, P = c["dims"]
    rng = np.random.RandomState(7)
    src = torch.from_numpy(rng.standard_normal((N, S, d_model)).astype(np.float32))
    return src, torch.from_numpy(c["ref"]).expand(N, -1, -1, -1), torch.from_numpy(c["shapes"]), torch.from_numpy(c["starts"])


def _module(train_front):
    from pctrans_amd.pixel_decoder.ops.modules import MSDeformAttn
    torch.manual_seed(3)
    m = MSDeformAttn(128, 3, 8, 4)
    with torch.no_grad():                              # the initial offsets / weights Linears have zero weights: give them some
        m.sampling_offsets.weight.normal_(0, 0.05)
        m.attention_weights.weight.normal_(0, 0.05)
    m.train_front = train_front
    return m


def test_module_switch_default_and_bad_value(monkeypatch):
    from pctrans_amd.pixel_decoder.ops.modules import MSDeformAttn, ms_deform_attn
    monkeypatch.delenv("PCT_MSDA_TRAIN", raising=False)
    assert MSDeformAttn(128, 3, 8, 4).train_front == "torch"
    monkeypatch.setenv("PCT_MSDA_TRAIN", "hip")
    assert MSDeformAttn(128, 3, 8, 4).train_front == "hip"
    assert "train_front" not in MSDeformAttn(128, 3, 8, 4).state_dict()
    src, ref, shapes, starts = _module_inputs(R.make("pyr3_shared"))
    m = _module("rocm")
    prev = ms_deform_attn.allow_cpu_reference(True)
    try:
        with pytest.raises(ValueError, match="train_front"):
            m(src, ref, src, shapes, starts)
    finally:
        ms_deform_attn.allow_cpu_reference(prev)


def test_covered_refuses_what_the_kernels_do_not_take():
    """On this side of the device every tensor is a CPU tensor, which `covered` refuses first; the other refusals are checked on
    tensors that are otherwise well-formed, and again on the device by test_msda_fused_train_gpu.py."""
    from pctrans_amd import msda_train
    c = R.make("pyr3_shared")
    value, ref, off, lg = (torch.from_numpy(c[k]) for k in ("value", "ref", "offsets", "logits"))
    assert not msda_train.covered(value, ref, off, lg)                                       # CPU tensors
    assert not msda_train.covered(value.double(), ref.double(), off.double(), lg.double())   # fp64
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not msda_train.covered(value, ref, off, lg)
    assert not msda_train.covered(value, torch.cat([ref, ref], -1), off, lg)                 # 4-d reference points
    assert not msda_train.covered(value, ref.clone().requires_grad_(), off, lg)
    with pytest.raises(RuntimeError):
        msda_train.ms_deform_attn_fused_train(value, torch.from_numpy(c["shapes"]), torch.from_numpy(c["starts"]), ref, off, lg)
    with pytest.raises(RuntimeError, match="CPU"):
        msda_train.fused_backward(value, torch.from_numpy(c["shapes"]), torch.from_numpy(c["starts"]), ref, off, lg,
                                  torch.from_numpy(c["grad_out"]))


@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "padding_mask"])
def test_cpu_module_with_hip_front_gives_the_torch_chain(mask):
    """CPU tensors are outside `covered`: with train_front = "hip" and allow_cpu_reference the module runs the torch chain, bit
    for bit what train_front = "torch" gives, output and gradients."""
    from pctrans_amd.pixel_decoder.ops.modules import ms_deform_attn
    c = R.make("pyr3_shared")
    src, ref, shapes, starts = _module_inputs(c)
    pad = None
    if mask:
        pad = torch.zeros(src.shape[:2], dtype=torch.bool)
        pad[1, 300:] = True
    prev = ms_deform_attn.allow_cpu_reference(True)
    try:
        results = []
        for front in ("hip", "torch"):
            m = _module(front)
            x = src.clone().requires_grad_()
            out = m(x, ref, x, shapes, starts, pad)
            out.square().sum().backward()
            results.append([out.detach(), x.grad] + [p.grad for p in m.parameters()])
    finally:
        ms_deform_attn.allow_cpu_reference(prev)
    assert len(results[0]) == len(results[1]) == 10
    for a, b in zip(*results):
        assert a is not None and torch.equal(a, b)

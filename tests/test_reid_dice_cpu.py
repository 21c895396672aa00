"""CPU: the C ABI entries of the re-id mask dice (header, library, binding, status codes that need no device); the `reid_dice`
switch and its fallback on CPU tensors; the float64 reference of test_reid_dice_gpu.py (reid_dice_reference.py) against the
torch formulation and its autograd; the derived bounds, held by the fp32 torch chain and missed by known-wrong results."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import reid_dice_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pct_reid_dice_rows_forward_f32", "pct_reid_dice_rows_backward_f32")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_abi_declares_exports_and_binds_the_entries():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_reid.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_reid.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_lib.REID_SYMBOLS) == sorted(NAMES)
    assert "dec.py:917-927" in header and "dec.py:880-901" in header
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.SEG_SYMBOLS, _lib.FPN_SYMBOLS,
                      _lib.ATTN_TRAIN_SYMBOLS):
            assert name not in other
        argtypes, restype, checked_by = _lib.REID_SYMBOLS[name]
        assert name in open(os.path.join(ROOT, checked_by)).read()
        assert re.search(r"\bT %s\b" % name, out)
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == argtypes and fn.restype is restype
        decl = re.search(r"PCT_API int %s\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == len(argtypes), name
    assert len(_lib.REID_SYMBOLS[NAMES[0]][0]) == 13 and len(_lib.REID_SYMBOLS[NAMES[1]][0]) == 14
    assert _lib.lib().pct_abi_version() == 1 and _lib.ABI_VERSION == 1
    makefile = open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()
    assert " reid_dice.hip " in makefile and "pctrans_hip_reid.h" in makefile


def test_status_codes_need_no_device():
    """Arguments are checked on the host before any launch: host pointers stand in and are never dereferenced."""
    from pctrans_amd import _lib
    L = _lib.lib()
    OK, BAD, ALIGN, UNSUP = 0, -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    fwd = lambda z=p, st=p, key=p, N=2, Q=5, h=6, w=5, I=3, ws=p, s=p, D=p, status=p: L.pct_reid_dice_rows_forward_f32(
        z, st, key, N, Q, h, w, I, ws, s, D, status, None)
    bwd = lambda z=p, st=p, key=p, D=p, s=p, G=p, N=2, Q=5, h=6, w=5, I=3, ws=p, gz=p: L.pct_reid_dice_rows_backward_f32(
        z, st, key, D, s, G, N, Q, h, w, I, ws, gz, None)
    for f in (fwd, bwd):
        assert f(N=0) == BAD and f(N=-1) == BAD and f(Q=0) == BAD and f(h=0) == BAD and f(w=-3) == BAD and f(I=-1) == BAD
        assert f(Q=1025, I=3) == UNSUP and f(N=65536) == UNSUP and f(h=1 << 16, w=1 << 15) == UNSUP
        assert f(N=2, Q=5, I=11) == UNSUP                                # more than Q rows in some image
        assert f(z=None) == BAD and f(st=None) == BAD and f(key=None) == BAD and f(ws=None) == BAD
        assert f(z=p + 2) == ALIGN and f(key=p + 1) == ALIGN and f(ws=p + 4) == ALIGN and f(st=p + 2) == ALIGN
    assert fwd(s=None) == BAD and fwd(D=None) == BAD and fwd(status=None) == BAD and fwd(D=p + 2) == ALIGN
    assert bwd(D=None) == BAD and bwd(s=None) == BAD and bwd(G=None) == BAD and bwd(gz=None) == BAD and bwd(gz=p + 1) == ALIGN
    assert fwd(I=0, key=None, D=None) == OK                              # no row: nothing is launched or asked for


def test_switch_default_follows_the_environment(monkeypatch):
    from pctrans_amd import reid_dice
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    make = lambda: dec.MultiScaleMaskedTransformerDecoder(
        16, True, hidden_dim=16, num_queries=4, nheads=2, dim_feedforward=16, dec_layers=1, pre_norm=False, mask_dim=8,
        enforce_input_project=False, points_num=1, sem_loss_on=False, norm="BN", rel_coord=True)
    monkeypatch.delenv("PCT_REID_DICE", raising=False)
    assert reid_dice.default() == "torch" and make().reid_dice == "torch"
    monkeypatch.setenv("PCT_REID_DICE", "hip")
    assert reid_dice.default() == "hip" and make().reid_dice == "hip"
    monkeypatch.setenv("PCT_REID_DICE", "")
    assert reid_dice.default() == "torch"
    monkeypatch.setenv("PCT_REID_DICE", "triton")
    with pytest.raises(RuntimeError):
        reid_dice.default()


def test_constants_and_workspace_formulas_are_the_kernel_files():
    from pctrans_amd import reid_dice
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "reid_dice.hip")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert reid_dice.MAX_QUERIES == const("RD_MAX_Q") == 1024
    assert reid_dice.MAX_CHUNKS == const("RD_MAX_CHUNKS") == R.MAX_CHUNKS
    assert reid_dice.PIXELS_PER_PASS == const("RD_FWD_PIX") == R.PIXELS_PER_PASS
    assert "N > 65535" in src and reid_dice.MAX_BATCH == 65535 and "0x7fffffffLL" in src
    header = open(os.path.join(ROOT, "include", "pctrans_hip_reid.h")).read()
    assert "4 * chunks * (num_rows + batch) * num_query bytes" in header
    assert "subs = ceil(height * width / 64), passes = ceil(subs / 128), chunks = ceil(subs / passes)" in header
    assert "4 * (3 * num_rows * num_query + num_rows + batch * num_query) bytes" in header
    for P in (1, 30, 64, 65, 252, 8192, 8193, 8245, 50176, 65536, 2 ** 31 - 2):
        subs = -(-P // 64)
        passes = -(-subs // 128)
        ch = -(-subs // passes)
        assert reid_dice.chunks(P) == (passes, ch) == R.chunks(P) and ch <= 128 and passes * ch * 64 >= P
        assert reid_dice.chain_length(P) == passes * 64 + ch == R.chain_length(P)
        for N, Q, I in ((2, 300, 120), (1, 1024, 64), (3, 37, 4)):
            assert reid_dice.workspace_bytes(N, Q, P, I) == 4 * ch * (I + N) * Q
            assert reid_dice.workspace_bytes(N, Q, P, I, backward=True) == 4 * (3 * I * Q + I + N * Q)
    assert reid_dice.chunks(65536) == (8, 128) and reid_dice.chain_length(65536) == 640
    assert reid_dice.chunks(97 * 85) == (2, 65)                         # the two-pass shape of the GPU tests


def test_cpu_tensors_are_not_supported():
    from pctrans_amd import reid_dice
    z = R.family("normal", 5, 6, 5, (2, 1))
    st, key = R.rows_of(5, 6, 5, (2, 1))
    assert not reid_dice.supported(z, (2, 1))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        reid_dice.dice_rows(z, st, key)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        reid_dice.dice_rows_forward(z, st, key)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        reid_dice.dice_rows_backward(z, st, key, z, z, z)


def _golden_inputs(golden):
    g = golden("dec_query_contrast")
    query, emb_dist, masks = _t(g["query"]), _t(g["emb_dist"]), _t(g["masks"])
    pos = [(_t(g["pos_src_%d" % b]), _t(g["pos_tgt_%d" % b])) for b in range(query.shape[1])]
    return g, query, emb_dist, masks, pos


def test_cpu_items_with_the_keyword_are_the_torch_items(golden, monkeypatch):
    """On CPU tensors mask_dice="hip" changes nothing: the items are bit-equal and the device path is not entered."""
    from pctrans_amd import reid_dice
    from pctrans_amd.transformer_decoder import query_contrast as qc
    monkeypatch.setattr(reid_dice, "dice_rows", lambda *a, **k: (_ for _ in ()).throw(AssertionError()))
    g, query, emb_dist, masks, pos = _golden_inputs(golden)
    off = qc.select_pos_neg_mask(masks, emb_dist, pos)
    on = qc.select_pos_neg_mask(masks, emb_dist, pos, mask_dice="hip")
    assert len(on) == len(off) == int(g["n_items_m"]) and on.batched.keys() == off.batched.keys()
    for k in off.batched:
        assert torch.equal(on.batched[k], off.batched[k])
    for a, b in zip(on, off):
        assert torch.equal(a["contrast"], b["contrast"]) and torch.equal(a["label"], b["label"])
    # the golden fixture still passes through the keyword (tolerances of tests/test_decoder_golden.py)
    for i, it in enumerate(on):
        want_c, want_l = g["m%d_contrast" % i].ravel(), g["m%d_label" % i]
        got_c, got_l = it["contrast"].numpy().ravel(), it["label"].numpy()
        np.testing.assert_array_equal(got_l, want_l)
        for lab in (0, 1):
            np.testing.assert_allclose(np.sort(got_c[got_l == lab]), np.sort(want_c[want_l == lab]), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        qc.select_pos_neg_mask(masks, emb_dist, pos, mask_dice="triton")
    torch.manual_seed(0)
    both = qc.query_contrast_items(query, masks, pos, mask_dice="hip")
    assert len(both[1]) == len(qc.query_contrast_items(query, masks, pos)[1])


@pytest.mark.parametrize("name,Q,h,w,counts", R.cases())
def test_reference_is_dice_for_and_autograd_of_the_float64_torch_chain(name, Q, h, w, counts):
    """Every case, to 1e-12 absolute."""
    from pctrans_amd.transformer_decoder import query_contrast as qc
    e = R.expected(name, "random", Q, h, w, counts)
    assert e is R.expected(name, "random", Q, h, w, counts)
    st = e["image_start"].tolist()
    for n in range(len(counts)):
        full = qc.dice_for(e["z"][n].double())
        for i in range(st[n], st[n + 1]):
            assert float((e["D"][i] - full[int(e["key"][i])]).abs().max()) <= 1e-12
    D, dz = R.torch_chain(e["z"].double(), e["image_start"], e["key"], e["G"].double())
    assert float((D - e["D"]).abs().max()) <= 1e-12
    assert float((dz - e["dz"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("name,Q,h,w,counts", R.cases())
def test_fp32_torch_chain_stays_inside_the_bounds(name, Q, h, w, counts):
    """The parent's path in fp32 on the CPU, both incoming gradients."""
    for kind in R.GRADS:
        e = R.expected(name, kind, Q, h, w, counts)
        D, dz = R.torch_chain(e["z"], e["image_start"], e["key"], e["G"])
        derr, gerr = (D.double() - e["D"]).abs(), (dz.double() - e["dz"]).abs()
        print("%s %s Q=%d: D err/bound %.3f  grad err/bound %.3f" % (
            name, kind, Q, float((derr / e["dbound"]).max()), float((gerr / e["gbound"].clamp(min=1e-300)).max())))
        assert bool((derr <= e["dbound"]).all()) and bool((gerr <= e["gbound"]).all())
        if name == "all cold":
            assert float((e["D"] - 1).abs().max()) < 1e-8 and float(e["dz"].abs().max()) < 1e-8 * float(e["G"].abs().sum())


@pytest.mark.parametrize("name,Q,h,w,counts", R.cases())
def test_bounds_separate_known_wrong_results(name, Q, h, w, counts):
    """Three wrong float64 results -- the last pixel dropped from every sum, the last pixel chunk dropped, x (1 - x) replaced by
    x -- each miss the true one by more than 4 x the bound somewhere (in D or in the gradient).  The families are built for it:
    "normal" has every pixel carry weight; "sparse hot" puts a hot pixel at the first and last pixel of the map and of every
    chunk; "saturated" ends on a +40 block for every other query.  "all cold" cannot take part and is checked for the opposite:
    with x <= 1e-13 everywhere the dropped pixels move D by 1e-13 of itself and x differs from x (1 - x) by 1e-13 of itself,
    far below fp32's resolution, so every wrong result is EQUAL to the true one to fp32 and no fp32 bound may separate them;
    that family holds D = 1 and the near-zero gradients instead."""
    e = R.expected(name, "random", Q, h, w, counts)
    z, st, key, G = e["z"], e["image_start"], e["key"], e["G"]
    P = h * w
    tail = P - (R.chunks(P)[1] - 1) * R.chunk_pixels(P)                 # pixels of the last chunk
    assert 1 <= tail <= R.chunk_pixels(P)
    wrong = {}
    for what, drop in (("last pixel", 1), ("last chunk", tail)):
        # (a map of one chunk: dropping it leaves no pixel, every sum is 0 and D = 1)
        D, s = R.dice64(z, st, key, drop_pixels=drop)
        wrong[what] = (D, R.grad64(z, st, key, G, D, s)[0])
    wrong["x for x (1 - x)"] = (e["D"], R.grad64(z, st, key, G, e["D"], e["s"], w_is_x=True)[0])
    for what, (D, dz) in wrong.items():
        miss = max(float(((D - e["D"]).abs() / e["dbound"].clamp(min=1e-300)).max()),
                   float(((dz - e["dz"]).abs() / e["gbound"].clamp(min=1e-300)).max()))
        print("%s Q=%d %s: miss / bound %.3g" % (name, Q, what, miss))
        if name == "all cold":
            assert miss < 1.0, (what, miss)
        else:
            assert miss > 4.0, (what, miss)

"""CPU: the C ABI entries of the re-id query rows and the contrast reduction (header, library, binding, status codes that need no
device); the `reid_query` / `contrast_loss` switches and their fallback on CPU tensors; the float64 reference of
test_reid_query_gpu.py (reid_query_reference.py) against query_contrast.py, _contrast_softplus and torch autograd; the
preconditions of the GPU tests' inputs."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import reid_query_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pct_reid_nearest_positive_f32", "pct_reid_query_rows_forward_f32", "pct_reid_query_rows_backward_f32",
         "pct_contrast_loss_rows_f32")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_abi_declares_exports_and_binds_the_entries():
    from pctrans_amd import _lib
    assert '#include "pctrans_hip_reid_query.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_reid_query.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_lib.REID_QUERY_SYMBOLS) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.SEG_SYMBOLS, _lib.FPN_SYMBOLS,
                      _lib.ATTN_TRAIN_SYMBOLS, _lib.REID_SYMBOLS, _lib.TARGETS_SYMBOLS, _lib.MSDA_TRAIN_SYMBOLS):
            assert name not in other
        argtypes, restype, checked_by = _lib.REID_QUERY_SYMBOLS[name]
        assert name in open(os.path.join(ROOT, checked_by)).read()
        assert re.search(r"\bT %s\b" % name, out)
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == argtypes and fn.restype is restype
        decl = re.search(r"PCT_API int %s\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == len(argtypes), name
    assert [len(_lib.REID_QUERY_SYMBOLS[n][0]) for n in NAMES] == [8, 11, 14, 11]
    assert _lib.REID_QUERY_SYMBOLS[NAMES[3]][0][7] is ctypes.c_float                  # inv_temperature
    assert _lib.lib().pct_abi_version() == 1 and _lib.ABI_VERSION == 1
    makefile = open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()
    assert " reid_query.hip " in makefile and "pctrans_hip_reid_query.h" in makefile


def test_status_codes_need_no_device():
    """Arguments are checked on the host before any launch: host pointers stand in and are never dereferenced."""
    from pctrans_amd import _lib
    L = _lib.lib()
    OK, BAD, ALIGN, UNSUP = 0, -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    near = lambda x=p, pos=p, Q=37, N=3, C=24, P=5, out=p: L.pct_reid_nearest_positive_f32(x, pos, Q, N, C, P, out, None)
    fwd = lambda x=p, st=p, key=p, Q=37, N=3, C=24, I=6, m=p, S=p, Cs=p: L.pct_reid_query_rows_forward_f32(
        x, st, key, Q, N, C, I, m, S, Cs, None)
    bwd = lambda x=p, st=p, key=p, m=p, Cs=p, gS=p, gC=p, Q=37, N=3, C=24, I=6, ws=p, gx=p: L.pct_reid_query_rows_backward_f32(
        x, st, key, m, Cs, gS, gC, Q, N, C, I, ws, gx, None)
    loss = lambda rows=p, img=p, key=p, own=p, I=6, Q=37, N=3, inv_t=0.5, out=p, coef=p: L.pct_contrast_loss_rows_f32(
        rows, img, key, own, I, Q, N, inv_t, out, coef, None)
    for f in (near, fwd, bwd):
        assert f(Q=0) == BAD and f(N=0) == BAD and f(N=-1) == BAD and f(C=0) == BAD and f(x=None) == BAD
        assert f(Q=1025) == UNSUP and f(N=65536) == UNSUP and f(C=516) == UNSUP and f(C=514) == UNSUP and f(C=22) == UNSUP
        assert f(x=p + 4) == ALIGN and f(x=p + 8) == ALIGN
    assert near(P=0) == BAD and near(P=38) == UNSUP and near(pos=None) == BAD and near(out=None) == BAD and near(pos=p + 2) == ALIGN
    for f in (fwd, bwd):
        assert f(I=-1) == BAD and f(st=None) == BAD and f(key=None) == BAD and f(key=p + 1) == ALIGN and f(st=p + 2) == ALIGN
        assert f(Q=5, N=2, I=11) == UNSUP                                 # more than Q rows in some image
    assert fwd(m=None) == BAD and fwd(S=None) == BAD and fwd(Cs=None) == BAD and fwd(S=p + 2) == ALIGN
    assert fwd(I=0, key=None, S=None, Cs=None, m=None) == OK             # no row: nothing is launched or asked for
    assert bwd(ws=None) == BAD and bwd(gx=None) == BAD and bwd(gS=None) == BAD and bwd(gC=None) == BAD and bwd(m=None) == BAD
    assert bwd(ws=p + 4) == ALIGN and bwd(gx=p + 4) == ALIGN and bwd(gC=p + 2) == ALIGN
    assert loss(I=-1) == BAD and loss(Q=0) == BAD and loss(N=0) == BAD and loss(inv_t=0.0) == BAD and loss(inv_t=-1.0) == BAD
    assert loss(inv_t=float("nan")) == BAD
    assert loss(rows=None) == BAD and loss(img=None) == BAD and loss(key=None) == BAD and loss(own=None) == BAD
    assert loss(out=None) == BAD and loss(coef=None) == BAD and loss(rows=p + 2) == ALIGN and loss(coef=p + 1) == ALIGN
    assert loss(Q=1025) == UNSUP and loss(N=65536) == UNSUP
    assert loss(I=0, rows=None, out=None, coef=None) == OK


def _decoder():
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    return dec.MultiScaleMaskedTransformerDecoder(
        16, True, hidden_dim=16, num_queries=4, nheads=2, dim_feedforward=16, dec_layers=1, pre_norm=False, mask_dim=8,
        enforce_input_project=False, points_num=1, sem_loss_on=False, norm="BN", rel_coord=True)


def _criterion():
    from pctrans_amd.loss import maskformer_criterion as crit
    return crit.SetCriterion(1, None, {}, 0.1, [], 16, 3.0, 0.75)


def test_switch_defaults_follow_the_environment(monkeypatch):
    from pctrans_amd import reid_query
    for env, default, attr, make in (("PCT_REID_QUERY", reid_query.default, "reid_query", _decoder),
                                     ("PCT_CONTRAST_LOSS", reid_query.contrast_default, "contrast_loss", _criterion)):
        monkeypatch.delenv(env, raising=False)
        assert default() == "torch" and getattr(make(), attr) == "torch"
        monkeypatch.setenv(env, "hip")
        assert default() == "hip" and getattr(make(), attr) == "hip"
        monkeypatch.setenv(env, "")
        assert default() == "torch"
        monkeypatch.setenv(env, "triton")
        with pytest.raises(RuntimeError):
            default()
        monkeypatch.delenv(env, raising=False)


def test_limits_are_the_kernel_files_constants():
    from pctrans_amd import reid_query
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "reid_query.hip")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert reid_query.MAX_QUERIES == const("RQ_MAX_Q") == R.MAX_QUERIES == 1024
    assert reid_query.MAX_CHANNELS == const("RQ_MAX_C") == R.MAX_CHANNELS == 512
    assert reid_query.LANE_CHANNELS == const("RQ_LANE_CHANNELS") and reid_query.WAVE_STEPS == const("RQ_WAVE_STEPS")
    assert reid_query.CHAIN_LENGTH == const("RQ_LANE_CHANNELS") + const("RQ_WAVE_STEPS") == R.CHAIN_LENGTH == 14
    assert "N > 65535" in src and reid_query.MAX_BATCH == R.MAX_BATCH == 65535 and "(C & 3)" in src
    header = open(os.path.join(ROOT, "include", "pctrans_hip_reid_query.h")).read()
    assert "length L = 14 (8 + 6)" in header
    assert "4 * num_rows * (channels + 2 * num_query + 1) bytes" in header
    assert "num_query <= 1024, channels <= 512 with channels % 4 == 0, batch <= 65535" in header
    for Q, C, I in ((300, 256, 120), (37, 24, 4), (1024, 512, 0)):
        assert reid_query.workspace_bytes(Q, C, I) == 4 * I * (C + 2 * Q + 1)
    for C in (4, 24, 256, 512):                                            # L <= C + 8 is what the issue's bounds assume
        assert R.CHAIN_LENGTH <= max(C, 8) + 8


def test_cpu_tensors_are_not_supported():
    from pctrans_amd import reid_query
    e = R.expected(0)
    q = e["query"]
    assert not reid_query.supported(q, (1, 0, 1)) and not reid_query.contrast_supported(e["S"].float(), e["image_of"], e["key"],
                                                                                       e["owner"])
    calls = (lambda: reid_query.nearest_positive(q, e["pos_lists"]),
             lambda: reid_query.query_rows(q, e["image_start"], e["key"]),
             lambda: reid_query.query_rows_forward(q, e["image_start"], e["key"]),
             lambda: reid_query.query_rows_backward(q, e["image_start"], e["key"], q, q, q, q),
             lambda: reid_query.contrast_loss_rows(e["S"].float(), e["image_of"], e["key"], e["owner"], 2.0),
             lambda: reid_query.contrast_loss_rows_forward(e["S"].float(), e["image_of"], e["key"], e["owner"], 2.0))
    for call in calls:
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            call()


def _golden_inputs(golden):
    g = golden("dec_query_contrast")
    query, emb_dist, masks = _t(g["query"]), _t(g["emb_dist"]), _t(g["masks"])
    pos = [(_t(g["pos_src_%d" % b]), _t(g["pos_tgt_%d" % b])) for b in range(query.shape[1])]
    return g, query, emb_dist, masks, pos


def test_cpu_items_and_losses_with_the_switches_are_the_torch_ones(golden, monkeypatch):
    """On CPU tensors reid_query = "hip" and contrast_loss = "hip" change nothing: items and losses are bit-equal, the device
    path is not entered, and the split plan is the plan of the fixture."""
    from pctrans_amd import reid_query
    from pctrans_amd.transformer_decoder import query_contrast as qc
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError())
    for name in ("nearest_positive", "query_rows", "contrast_loss_rows"):
        monkeypatch.setattr(reid_query, name, boom)
    g, query, emb_dist, masks, pos = _golden_inputs(golden)
    random.seed(5)
    off = qc.query_contrast_items(query, masks, pos)
    random.seed(5)
    on = qc.query_contrast_items(query, masks, pos, mask_dice="hip", reid_query="hip")
    random.seed(5)
    direct = qc.select_pos_neg_query(query, emb_dist, pos, query_rows="hip")        # (the fixture's own table: its items)
    random.seed(5)
    direct_off = qc.select_pos_neg_query(query, emb_dist, pos)
    assert len(on[0]) == len(off[0]) > 0 and len(on[1]) == len(off[1]) > 0
    assert len(direct) == len(direct_off) == int(g["n_items_q"])
    for a, b in ((on[0], off[0]), (on[1], off[1]), (direct, direct_off)):
        assert a.batched.keys() == b.batched.keys() and "rows" not in a.batched
        for k in b.batched:
            assert torch.equal(a.batched[k], b.batched[k]), k
        for x, y in zip(a, b):
            assert x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in y)
    with pytest.raises(ValueError):
        qc.query_contrast_items(query, masks, pos, reid_query="triton")
    with pytest.raises(ValueError):
        qc.select_pos_neg_query(query, emb_dist, pos, query_rows="triton")
    c_off, c_on = _criterion(), _criterion()
    c_on.contrast_loss = "hip"
    for c in (c_off, c_on):
        c.got = {**c.loss_reid_query({"pred_qd_query": off[0]}, None, None, 1), **c.loss_reid_mask({"pred_qd_mask": off[1]}, None, None, 1)}
    assert c_on.got.keys() == c_off.got.keys() and all(torch.equal(c_on.got[k], c_off.got[k]) for k in c_off.got)
    c_on.contrast_loss = "triton"
    with pytest.raises(ValueError):
        c_on.loss_reid_mask({"pred_qd_mask": off[1]}, None, None, 1)


def test_reference_reproduces_query_contrast_and_the_softplus_on_the_golden_fixture(golden):
    from pctrans_amd.loss.maskformer_criterion import _contrast_softplus
    from pctrans_amd.transformer_decoder import query_contrast as qc
    g, query, emb_dist, masks, pos = _golden_inputs(golden)
    Q, N, _ = query.shape
    pos_lists = [p[0].tolist() for p in pos]
    # the fixture's emb_dist is a table of its own, not the cosines of its queries: the plan of the fixture's queries is the one
    # query_contrast_items builds, from F.cosine_similarity
    q = query.permute(1, 0, 2)
    emb_dist = torch.nn.functional.cosine_similarity(q.unsqueeze(2), q.unsqueeze(1), dim=-1)
    plan = qc._plan(emb_dist, pos)
    nearest, gap = R.nearest64(query, pos_lists)
    assert min(float(gp[[r for r in range(Q) if r not in pl]].min()) for gp, pl in zip(gap, pos_lists) if pl) > 1e-5
    assert [tuple(p) for p in R.plan_of(nearest, pos_lists, Q)] == [tuple(p) for p in plan] and len(plan) > 0
    assert plan == qc._plan_from_nearest(nearest, pos_lists, Q)
    for n, c in enumerate(R.cos64(query, pos_lists)):
        assert float((c - emb_dist[n][:, pos_lists[n]].double()).abs().max()) <= 1e-6
    random.seed(3)
    items = qc.select_pos_neg_query(query, emb_dist, pos, _plan_cache=plan)
    bt = items.batched
    image_start, key, image_of, owner = R.rows_of(plan, N, Q)
    norm, S, Cs, S_abs = R.rows64(query, image_start, key)
    order = torch.tensor([p[2] + p[3] for p in plan])
    assert float((S.gather(1, order) - bt["contrast"].double()).abs().max()) <= 1e-5 * float(S_abs.max())
    # the auxiliary cosines: the drawn (item, query) pairs are those of the same seed
    random.seed(3)
    at = 0
    for i, (b, _, cluster, neg) in enumerate(plan):
        k = len(neg) if len(cluster) * 10 >= len(neg) else len(cluster) * 10
        qs = cluster + [neg[s] for s in random.sample(list(range(len(neg))), k)]
        assert float((Cs[i, qs] - bt["aux_consin"][at:at + len(qs)].double()).abs().max()) <= 1e-6
        at += len(qs)
    assert at == bt["aux_consin"].shape[0]
    for temperature, scores in ((2.0, S), (0.5, Cs)):                      # (any rows serve the reduction; Cs stands for a dice)
        want = _contrast_softplus(scores.gather(1, order) / temperature, bt["n_pos"])
        loss, coef = R.contrast64(scores, image_of, key, owner, 1.0 / temperature)
        assert float((loss - want).abs().max()) <= 1e-12 * (1 + float(want.abs().max())) + 2.1e-9    # (F.softplus above 20)
        assert int((coef[torch.arange(len(plan)), key.long()] != 0).sum()) == 0


@pytest.mark.parametrize("shape", range(len(R.SHAPES)))
def test_reference_gradients_are_autograds_in_float64(shape):
    from pctrans_amd.loss.maskformer_criterion import _contrast_softplus
    e = R.expected(shape)
    N, Q, C, counts = R.SHAPES[shape]
    x = e["query"].double().requires_grad_(True)
    img, key = e["image_of"].long(), e["key"].long()
    xt = x.transpose(0, 1)
    S = torch.einsum("iqc,ic->iq", xt[img], xt[img, key])
    unit = torch.nn.functional.normalize(xt, dim=-1)
    Cs = torch.einsum("iqc,ic->iq", unit[img], unit[img, key])
    assert float((S.detach() - e["S"]).abs().max()) <= 1e-12 * float(e["S_abs"].max())
    assert float((Cs.detach() - e["Cs"]).abs().max()) <= 1e-13
    want, = torch.autograd.grad((S * e["gS"].double()).sum() + (Cs * e["gC"].double()).sum(), x)
    got, got_abs, T = R.grad64(e["query"], e["image_start"], e["key"], e["gS"], e["gC"], e["norm"], e["Cs"])
    assert float((got - want).abs().max()) <= 1e-12 * float(got_abs.max())
    assert bool((got_abs >= got.abs() * (1 - 1e-12)).all()) and float(T.max()) >= 3 * Q
    for n, c in enumerate(counts):
        if c == 0:
            assert int((got[:, n] != 0).sum()) == 0 and int((T[:, n] != 0).sum()) == 0
    # a clamped norm: the row's b terms are dropped, as F.normalize's clamp passes no gradient
    tiny = e["query"].clone()
    row = min(r for r in range(Q) if r not in e["pos_lists"][0])           # an unmatched query of image 0
    tiny[row, 0] = 1e-20
    x = tiny.double().requires_grad_(True)
    xt = x.transpose(0, 1)
    unit = torch.nn.functional.normalize(xt, dim=-1)
    Cs = torch.einsum("iqc,ic->iq", unit[img], unit[img, key])
    want, = torch.autograd.grad((Cs * e["gC"].double()).sum(), x)
    norm, _, Cs64, _ = R.rows64(tiny, e["image_start"], e["key"])
    assert float(norm[0, row]) == 1e-12
    got, got_abs, _ = R.grad64(tiny, e["image_start"], e["key"], torch.zeros_like(e["gS"]), e["gC"], norm, Cs64)
    assert float((got - want).abs().max()) <= 1e-12 * float(got_abs.max())
    # the reduction's coefficients
    order = torch.tensor([p[2] + p[3] for p in e["plan"]])
    n_pos = torch.tensor([len(p[2]) for p in e["plan"]])
    for temperature in (2.0, 0.5):
        rows = e["S"].clone().requires_grad_(True)
        loss = _contrast_softplus(rows.gather(1, order) / temperature, n_pos)
        want, = torch.autograd.grad(loss.sum(), rows)
        got_loss, coef = R.contrast64(e["S"], e["image_of"], e["key"], e["owner"], 1.0 / temperature)
        # F.softplus returns its argument above 20 and passes the gradient through unchanged there: e^-20 = 2.1e-9
        loss = loss.detach()
        assert float((got_loss - loss).abs().max()) <= 1e-12 * (1 + float(loss.abs().max())) + 2.1e-9
        assert float((coef - want).abs().max()) <= (1e-12 + 2.1e-9) / temperature
        low = loss < 20
        assert int(low.sum()) >= 2 and float((got_loss - loss)[low].abs().max()) <= 1e-12 * 21
        assert float((coef - want)[low].abs().max()) <= 1e-12 / temperature


def test_inputs_of_the_gpu_tests_meet_their_preconditions():
    """Shape 0: every unmatched row's top-two gap exceeds 2 (2 L + 6) u, so the kernel's table must equal the float64 one with no
    row left out; the single-instance image gives an item without negatives, the middle image none.  Shape 1: above one 256-channel
    pass, both images with items."""
    assert R.COS_BOUND == (2 * 14 + 6) * 2.0 ** -24 and R.GAP == 2 * R.COS_BOUND
    e = R.expected(0)
    N, Q, C, counts = R.SHAPES[0]
    assert (N, Q, C, counts) == (3, 37, 24, (5, 0, 1)) and R.SHAPES[1] == (2, 70, 256, (9, 33))
    for n in range(N):
        unmatched = [r for r in range(Q) if r not in e["pos_lists"][n]]
        assert float(e["gap"][n][unmatched].min()) > 100 * R.GAP
        print("image %d: minimum top-two gap %.3e against %.3e" % (n, float(e["gap"][n][unmatched].min()), R.GAP))
    assert e["image_start"].tolist()[1] == e["image_start"].tolist()[2]                  # the image without items
    last = e["plan"][-1]
    assert last[0] == 2 and len(last[2]) == Q - 1 and last[3] == []                      # the item without negatives
    assert float(R.contrast64(e["S"], e["image_of"], e["key"], e["owner"], 0.5)[0][-1]) == 0.0
    assert len(e["plan"]) >= 4 and any(len(p[3]) > 0 for p in e["plan"])
    e1 = R.expected(1)
    assert all(c > 0 for c in (e1["image_start"][1:] - e1["image_start"][:-1]).tolist())
    assert e1["key"].tolist()[:3] != sorted(e1["key"].tolist()[:3]) or e1["key"].tolist()[-3:] != sorted(e1["key"].tolist()[-3:])
    assert e["query"].dtype == torch.float32 and e["query"].is_contiguous() and R.expected(0) is e

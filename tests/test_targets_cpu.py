"""CPU: pctrans_amd/targets.py -- the torch mode of prepare_instance_targets against the reference trainer's own
prepare_intance_targets (tests/golden/targets_small.npz, written by tests/golden/make_golden_targets.py) exactly: values,
dtypes, shapes, every key; the random.sample draws of points_num = 3; TargetList as a list of plain dicts; what `supported`
refuses; the ABI table; and the criterion and matcher on a plain list against the same dicts in a TargetList without planes."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NAMES = ("pct_instance_targets_census", "pct_instance_targets_planes")
CASES = [("i0_d0", 0, False), ("i0_d1", 0, True), ("i-1_d0", -1, False), ("i-1_d1", -1, True)]


def _equal(item, g, case, n):
    keys = {k.split(".")[2] for k in g if k.startswith("%s.%d." % (case, n))}
    assert set(item) == keys and type(item) is dict, (case, n, sorted(item), sorted(keys))
    for k in keys:
        want = torch.from_numpy(g["%s.%d.%s" % (case, n, k)])
        got = item[k]
        assert got.dtype == want.dtype and got.shape == want.shape, (case, n, k, got.dtype, got.shape, want.dtype, want.shape)
        assert torch.equal(got.cpu(), want), (case, n, k)


@pytest.mark.parametrize("case,ignore,disc", CASES)
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.float32])
def test_torch_mode_equals_the_reference_exactly(golden, case, ignore, disc, dtype):
    from pctrans_amd import targets
    g = golden("targets_small")
    maps = torch.from_numpy(g["maps"]).to(dtype)
    got = targets.prepare_instance_targets(maps, points_num=1, semantic_loss_on=True, instance_discriminative=disc,
                                           ignore_label=ignore, mode="torch")
    assert isinstance(got, targets.TargetList) and isinstance(got, list) and len(got) == 2
    assert got.planes is None and got.starts is None and got.counts is None and got.counts_host is None
    for n, item in enumerate(got):
        _equal(item, g, case, n)
    assert got[0]["masks"].shape[0] != got[1]["masks"].shape[0]
    without = targets.prepare_instance_targets(maps, ignore_label=ignore, instance_discriminative=disc, mode="torch")
    assert all(set(t) == {"labels", "masks", "center_points"} for t in without)


def test_torch_mode_image_without_instances(golden):
    from pctrans_amd import targets
    g = golden("targets_small")
    got = targets.prepare_instance_targets(torch.from_numpy(g["empty"]).long(), semantic_loss_on=True, mode="torch")
    assert len(got) == 1
    _equal(got[0], g, "empty", 0)
    assert got[0]["masks"].dtype == torch.float32 and got[0]["labels"].numel() == 0


def test_torch_mode_three_points_reproduces_the_draws(golden):
    from pctrans_amd import targets
    g = golden("targets_small")
    random.seed(int(g["seed"]))
    got = targets.prepare_instance_targets(torch.from_numpy(g["maps"]).long(), points_num=3, semantic_loss_on=True,
                                           instance_discriminative=True, mode="torch")
    for n, item in enumerate(got):
        _equal(item, g, "p3", n)
    assert got[0]["labels"].shape[0] == 4 and got[0]["masks"].shape[0] == 3        # the one-pixel instance: label kept, mask dropped


def test_supported_refuses_what_the_kernels_do_not_cover(monkeypatch):
    from pctrans_amd import targets
    maps = torch.zeros((2, 8, 8), dtype=torch.int64)
    assert not targets.supported(maps, 1, torch.device("cpu"))
    assert not targets.supported(maps, 1, None)                                      # a CPU map and no device given
    assert not targets.supported(maps, 3, torch.device("cuda", 0))
    assert not targets.supported(maps.double(), 1, torch.device("cuda", 0))
    assert not targets.supported(maps[0], 1, torch.device("cuda", 0))
    assert targets.MAX_INSTANCES == 512
    # the default mode is "hip", PCT_TARGETS overrides it, and a CPU device always gets the torch mode
    monkeypatch.delenv("PCT_TARGETS", raising=False)
    assert targets.default() == "hip"
    monkeypatch.setenv("PCT_TARGETS", "torch")
    assert targets.default() == "torch"
    monkeypatch.setenv("PCT_TARGETS", "fast")
    with pytest.raises(RuntimeError):
        targets.default()
    monkeypatch.delenv("PCT_TARGETS")
    got = targets.prepare_instance_targets(maps, mode="hip")
    assert got.planes is None and len(got) == 2
    with pytest.raises(ValueError):
        targets.prepare_instance_targets(maps, mode="cuda")
    with pytest.raises(ValueError):
        targets.prepare_instance_targets(maps[0])


def test_abi_table_and_header_agree():
    from pctrans_amd import _lib
    header = open(os.path.join(ROOT, "include", "pctrans_hip_targets.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_lib.TARGETS_SYMBOLS) == sorted(NAMES)
    assert '#include "pctrans_hip_targets.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    for name in NAMES:
        for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.SEG_SYMBOLS, _lib.FPN_SYMBOLS,
                      _lib.ATTN_TRAIN_SYMBOLS, _lib.REID_SYMBOLS):
            assert name not in other
        argtypes, restype, checked_by = _lib.TARGETS_SYMBOLS[name]
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == argtypes and fn.restype is ctypes.c_int and restype is ctypes.c_int
        assert os.path.exists(os.path.join(ROOT, checked_by)), name
    assert len(_lib.TARGETS_SYMBOLS[NAMES[0]][0]) == 13 and len(_lib.TARGETS_SYMBOLS[NAMES[1]][0]) == 14
    from pctrans_amd import targets
    assert ("#define PCT_TARGETS_WORKSPACE_PER_IMAGE %d " % targets.WORKSPACE_PER_IMAGE) in header
    assert ("#define PCT_TARGETS_MAX_INSTANCES %d " % targets.MAX_INSTANCES) in header


def test_entry_points_reject_bad_arguments_without_a_launch():
    """Null pointers, sizes, dtype codes, alignment and the geometry limits are refused on the host: no GPU needed."""
    from pctrans_amd import _lib
    L = _lib.lib()
    BAD, ALIGN, UNSUP = -1, -3, -4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0
    census, planes = L.pct_instance_targets_census, L.pct_instance_targets_planes
    assert census(p, 2, 0, 8, 8, 0, p, p, p, p, p, p, None) == BAD
    assert census(None, 2, 1, 8, 8, 0, p, p, p, p, p, p, None) == BAD
    assert census(p, 5, 1, 8, 8, 0, p, p, p, p, p, p, None) == UNSUP
    assert census(p + 2, 2, 1, 8, 8, 0, p, p, p, p, p, p, None) == ALIGN
    assert census(p, 2, 1, 8, 8, 0, p + 4, p, p, p, p, p, None) == ALIGN
    assert census(p, 2, 65536, 8, 8, 0, p, p, p, p, p, p, None) == UNSUP
    assert census(p, 2, 1, 65536, 32768, 0, p, p, p, p, p, p, None) == UNSUP
    assert planes(p, 2, 1, 8, 8, p, p, 0, 1, p, p, p, p, None) == BAD
    assert planes(p, 2, 1, 8, 8, p, None, 1, 1, p, p, p, p, None) == BAD
    assert planes(p, 2, 1, 8, 8, p, p, 600, 513, p, p, p, p, None) == UNSUP
    assert planes(p, 2, 1, 8, 8, p, p, 1, 1, p, p + 4, p, p, None) == ALIGN
    assert planes(p, 2, 1, 8, 8, p, p, 1, 1, p, p, p + 8, None, None) == ALIGN


def _case():
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(2, 6, 16, 16, generator=g)
    maps = torch.zeros((2, 32, 32), dtype=torch.int64)
    maps[0, 2:12, 3:15], maps[0, 14:30, 10:28], maps[0, 20:24, 0:6] = 4, 9, 11
    maps[1, 1:9, 1:30], maps[1, 12:31, 5:16] = 2, 7
    emb = torch.randn(2, 8, 16, 16, generator=g)
    return pred, maps, emb


def test_criterion_and_matcher_treat_a_target_list_without_planes_as_a_plain_list():
    from pctrans_amd import targets
    from pctrans_amd.loss import maskformer_criterion as crit
    from pctrans_amd.loss.matcher import Point_HungarianMatcher
    pred, maps, emb = _case()
    wrapped = targets.prepare_instance_targets(maps, semantic_loss_on=True, mode="torch")
    plain = [dict(t) for t in wrapped]
    assert type(plain) is list and wrapped.planes is None
    out = {}
    for name, tg in (("plain", plain), ("wrapped", wrapped)):
        c = crit.SetCriterion(1, Point_HungarianMatcher(num_points=40), {}, 0.1, ["masks", "embedding"], 40, 3.0, 0.75)
        torch.manual_seed(3)
        indices = c.matcher.forward_many([{"pred_masks": pred}, {"pred_masks": pred * 0.5}], tg)
        torch.manual_seed(4)
        lm = c.loss_masks({"pred_masks": pred}, tg, indices[0], 5.0)
        le = c.loss_embedding(emb, tg)
        out[name] = (indices, lm, le)
    for a, b in zip(out["plain"][0], out["wrapped"][0]):
        for (sa, ta), (sb, tb) in zip(a, b):
            assert torch.equal(sa, sb) and torch.equal(ta, tb)
    for k in ("loss_mask", "loss_dice"):
        assert torch.equal(out["plain"][1][k], out["wrapped"][1][k])
    assert torch.equal(out["plain"][2]["loss_emb"], out["wrapped"][2]["loss_emb"])
    # planes that do not agree with the dicts' masks are not taken
    wrong = targets.TargetList(plain)
    wrong.planes = torch.zeros((4, 32, 32))
    wrong.counts_host, wrong.starts, wrong.counts = [2, 2], torch.tensor([0, 2]), torch.tensor([2, 2])
    assert targets.handed_planes(wrong, [t["masks"] for t in plain], pred) is None
    right = targets.TargetList(plain)
    right.planes = torch.cat([t["masks"] for t in plain]).float()
    right.counts_host, right.starts, right.counts = [3, 2], torch.tensor([0, 3]), torch.tensor([3, 2])
    assert targets.handed_planes(right, [t["masks"] for t in plain], pred) is right.planes
    assert targets.handed_planes(plain, [t["masks"] for t in plain], pred) is None


def test_model_method_fills_its_arguments_from_the_model(golden):
    from pctrans_amd.arch import maskformer as mfm
    from pctrans_amd.arch.resnet import ResNet
    from pctrans_amd.config import get_cfg
    g = golden("targets_small")
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=6, norm="BN", sem_norm="BN", enc_layers=1, dec_layers=2, train_num_points=64, dataset="BBBC")
    model = mfm.MaskFormer(**mfm.MaskFormer.from_config(cfg, ResNet(18, 3, norm="BN")))
    got = model.prepare_instance_targets(torch.from_numpy(g["maps"]).long())
    assert model.sem_seg_head.predictor.points_num == 1 and model.sem_seg_head.predictor.sem_loss_on
    for n, item in enumerate(got):
        _equal(item, g, "i0_d0", n)
    got = model.prepare_instance_targets(torch.from_numpy(g["maps"]).long(), instance_discriminative=True, ignore_label=-1)
    for n, item in enumerate(got):
        _equal(item, g, "i-1_d1", n)

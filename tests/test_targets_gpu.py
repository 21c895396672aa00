"""GPU: the instance-target kernels (pct_instance_targets_census, pct_instance_targets_planes through pctrans_amd/targets.py)
against the torch mode -- the trainer's loop restated, itself held to the reference's output by test_targets_cpu.py -- and the
reference's own centre points (tests/golden/targets_small.npz).  Everything but the centre points is integer or 0 / 1 data and
compared exactly; the centre points are compared exactly where the reference's float chain is exact (the fixture) and against
the exact rational centre elsewhere."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = [("i0_d0", 0, False), ("i0_d1", 0, True), ("i-1_d0", -1, False), ("i-1_d1", -1, True)]
# the fixture's largest label, 65 535, in a dtype that cannot hold it: that dtype's largest value (the ascending order stays)
DTYPES = [(torch.uint8, 255), (torch.int16, 32767), (torch.int32, 65535), (torch.int64, 65535), (torch.float32, 65535)]


def _fixture_maps(dtype, top):
    maps = torch.from_numpy(load_golden("targets_small")["maps"]).long()
    maps[maps == 65535] = top
    return maps.to(dtype)


def _same_lists(got, want, centres=True):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert type(a) is dict and set(a) == set(b)
        for k in b:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, (k, a[k].dtype, a[k].shape)
            if k != "center_points" or centres:
                assert torch.equal(a[k], b[k]), k


def _planes_agree(got):
    masks = [t["masks"] for t in got]
    assert got.planes.dtype == torch.float32 and got.planes.is_contiguous() and got.planes.device == masks[0].device
    assert torch.equal(got.planes, torch.cat(masks).float())
    counts = [int(m.shape[0]) for m in masks]
    assert got.counts_host == counts and got.counts.dtype == got.starts.dtype == torch.int32
    assert got.counts.tolist() == counts and got.starts.tolist() == [sum(counts[:n]) for n in range(len(counts))]


def _exact_centres(gt):
    """{id: (Fraction x, Fraction y)} of an integer numpy map: sum x / (count W), sum y / (count W) in Python integers."""
    H, W = gt.shape
    out = {}
    for v in np.unique(gt):
        ys, xs = np.nonzero(gt == v)
        out[int(v)] = (Fraction(int(xs.astype(np.int64).sum()), len(xs) * W), Fraction(int(ys.astype(np.int64).sum()), len(xs) * W))
    return out


def _centres_within_one_rounding(item, gt, ids):
    """|c - exact| <= 2^-23 |exact|: two fp64 divisions (2^-53 each) and one rounding to fp32 (2^-24) stay below it."""
    exact = _exact_centres(gt)
    got = item["center_points"].cpu().double().numpy()
    worst = 0.0
    for row, v in zip(got, ids):
        for c, e in zip(row, exact[int(v)]):
            err = abs(Fraction(float(c)) - e)
            assert err <= Fraction(1, 2 ** 23) * abs(e), (v, float(c), float(e))
            worst = max(worst, float(err / e) if e else 0.0)
    return worst


@pytest.mark.parametrize("case,ignore,disc", CASES)
@pytest.mark.parametrize("dtype,top", DTYPES)
def test_hip_mode_equals_torch_mode_and_the_reference_centres(case, ignore, disc, dtype, top):
    from pctrans_amd import targets
    g = load_golden("targets_small")
    maps = _fixture_maps(dtype, top)                                            # a CPU map: crosses the bus once
    assert targets.supported(maps, 1, DEV)
    kw = dict(points_num=1, semantic_loss_on=True, instance_discriminative=disc, ignore_label=ignore, device=DEV)
    want = targets.prepare_instance_targets(maps, mode="torch", **kw)
    got = targets.prepare_instance_targets(maps, mode="hip", **kw)
    assert isinstance(got, targets.TargetList) and got.planes is not None
    _same_lists(got, want, centres=False)
    _planes_agree(got)
    for n, item in enumerate(got):
        ref = torch.from_numpy(g["%s.%d.center_points" % (case, n)])
        G = item["center_points"].shape[0]
        # (uint8 with ignore_label -1: torch compares in the map's dtype, where -1 is 255 -- the last id leaves in both modes)
        assert G == ref.shape[0] - (1 if dtype == torch.uint8 and ignore == -1 else 0)
        assert torch.equal(item["center_points"].cpu(), ref[:G]), (n, item["center_points"].cpu(), ref)
        if disc:
            assert item["labels"].tolist() == sorted(item["labels"].tolist()) and item["labels"].numel() == G


def test_image_without_instances_on_the_device():
    from pctrans_amd import targets
    g = load_golden("targets_small")
    maps = torch.cat([torch.from_numpy(g["empty"]), torch.from_numpy(g["maps"])])              # empty image first, then two others
    want = targets.prepare_instance_targets(maps, semantic_loss_on=True, device=DEV, mode="torch")   # (a CPU map, as the trainer's:
    got = targets.prepare_instance_targets(maps.cuda(), semantic_loss_on=True, mode="hip")           # the host's float mean is exact here)
    assert got.planes is not None and got.counts_host == [1, 4, 3]
    _same_lists(got, want)
    _planes_agree(got)
    assert got[0]["masks"].dtype == torch.float32 and got[0]["labels"].numel() == 0 and got[0]["fg_masks"].dtype == torch.float32
    assert torch.equal(got[0]["center_points"].cpu(), torch.from_numpy(g["empty.0.center_points"]))


def test_centres_are_exact_where_fp32_sums_are_not():
    """One label over a whole 512 x 512 image but one pixel: sum x = 6.7e7 > 2^24, where a float sum of the coordinates drops
    bits.  The kernels' integer sums are exact: each centre within one fp32 rounding of the exact rational."""
    from pctrans_amd import targets
    gt = np.full((512, 512), 5, dtype=np.int32)
    gt[100, 300] = 9
    maps = torch.from_numpy(gt)[None]
    got = targets.prepare_instance_targets(maps, device=DEV, mode="hip")
    assert got.planes is not None and got.counts_host == [2]
    worst = _centres_within_one_rounding(got[0], gt, [5, 9])
    want = targets.prepare_instance_targets(maps, device=DEV, mode="torch")
    _same_lists(got, want, centres=False)
    _planes_agree(got)
    exact = _exact_centres(gt)
    torch_err = max(abs(float(Fraction(float(c)) - e) / float(e))
                    for row, v in zip(want[0]["center_points"].cpu().double().numpy(), [5, 9]) for c, e in zip(row, exact[v]))
    print("512 x 512 one label: hip centre error %.3g (bound %.3g), torch mode error %.3g" % (worst, 2.0 ** -23, torch_err))


@functools.lru_cache(maxsize=None)
def _many(K):
    """A 64 x 64 map of K instances: pixel p carries label 7 (p % K) + 1 (gaps between the values, no background)."""
    p = np.arange(64 * 64)
    return (7 * (p % K) + 1).reshape(64, 64).astype(np.int32)


@pytest.mark.parametrize("K", [300, 512])
def test_table_limits_inside(K):
    from pctrans_amd import targets
    gt = _many(K)
    maps = torch.from_numpy(gt)[None].cuda()
    got = targets.prepare_instance_targets(maps, semantic_loss_on=True, instance_discriminative=True, mode="hip")
    want = targets.prepare_instance_targets(maps, semantic_loss_on=True, instance_discriminative=True, mode="torch")
    assert got.planes is not None and got.counts_host == [K]
    _same_lists(got, want, centres=False)
    _planes_agree(got)
    _centres_within_one_rounding(got[0], gt, got[0]["labels"].tolist())


def test_table_limit_exceeded_gives_the_torch_result():
    from pctrans_amd import targets
    maps = torch.from_numpy(_many(513))[None].cuda()
    got = targets.prepare_instance_targets(maps, semantic_loss_on=True, mode="hip")
    want = targets.prepare_instance_targets(maps, semantic_loss_on=True, mode="torch")
    assert got.planes is None and got.starts is None and got.counts is None and got[0]["masks"].shape[0] == 513
    _same_lists(got, want)


@pytest.mark.parametrize("dtype,value", [(torch.float32, 2.5), (torch.int32, 70000), (torch.int16, -3)])
def test_values_outside_the_tables_give_the_torch_result(dtype, value):
    from pctrans_amd import targets
    maps = _fixture_maps(torch.int32, 65535).to(dtype) if dtype != torch.int16 else _fixture_maps(dtype, 32767)
    maps[1, 5, 7] = value
    assert targets.supported(maps, 1, DEV)                                      # the shapes are covered: the VALUES are not
    got = targets.prepare_instance_targets(maps, semantic_loss_on=True, instance_discriminative=True, device=DEV, mode="hip")
    want = targets.prepare_instance_targets(maps, semantic_loss_on=True, instance_discriminative=True, device=DEV, mode="torch")
    assert got.planes is None
    _same_lists(got, want)


@pytest.mark.parametrize("dtype", [torch.int32, torch.float32])
def test_census_and_label_overlap_keep_the_same_values(dtype):
    """The census that the targets and the validation metrics share (csrc/label_census.hpp): the kept ids of
    pct_instance_targets_census, the ground-truth values of pct_label_overlap and torch.unique of the map are one list, element
    for element.  31 / 32 is a bitmap-word boundary, 255 / 256 the boundary between two threads of the rank step, 65 535 the top
    value; image 1 holds a subset; `ignore_label` is a value no pixel has, so it leaves nothing out."""
    from pctrans_amd import _lib, metrics, targets
    N, H, W = 2, 19, 17
    p = torch.arange(H * W)
    full, part = torch.tensor([0, 1, 31, 32, 255, 256, 65535]), torch.tensor([1, 32, 255, 65535])
    maps = torch.stack([full[p % 7], part[(3 * p) % 4]]).view(N, H, W).to(dtype).to(DEV)
    ws = torch.empty(N * targets.WORKSPACE_PER_IMAGE // 4, dtype=torch.int32, device=DEV)
    ids = torch.empty((N, targets.MAX_INSTANCES), dtype=torch.int32, device=DEV)
    pixels = torch.empty_like(ids)
    centres = torch.empty((N, targets.MAX_INSTANCES, 2), dtype=torch.float32, device=DEV)
    word = torch.empty((2, N), dtype=torch.int32, device=DEV)                   # num, status
    with torch.cuda.device(DEV):
        rc = _lib.lib().pct_instance_targets_census(maps.data_ptr(), targets._DTYPES[dtype], N, H, W, 7, ws.data_ptr(),
                                                    ids.data_ptr(), pixels.data_ptr(), centres.data_ptr(), word[0].data_ptr(),
                                                    word[1].data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(rc, "instance_targets_census")
    ov = metrics.label_overlap(maps, maps, mode="hip")
    assert ov.mode == "hip" and ov.status.tolist() == [0, 0]
    num, status = word.tolist()
    assert status == [0, 0] and num == [7, 4] and ov.num[:, 1].tolist() == num
    for n in range(N):
        want = torch.unique(maps[n]).to(torch.int32)
        assert torch.equal(ids[n, :num[n]], want) and torch.equal(ov.values[n, 1, :num[n]], want)
        assert torch.equal(ids[n, :num[n]], ov.values[n, 1, :num[n]])


def test_views_repeats_and_the_single_allocation():
    from pctrans_amd import targets
    big = torch.zeros((2, 74, 60), dtype=torch.int64)
    big[:, ::2, 3:56] = _fixture_maps(torch.int64, 65535)
    view = big.cuda()[:, ::2, 3:56]
    assert not view.is_contiguous()
    a = targets.prepare_instance_targets(view, semantic_loss_on=True, instance_discriminative=True, mode="hip")
    b = targets.prepare_instance_targets(view.contiguous(), semantic_loss_on=True, instance_discriminative=True, mode="hip")
    c = targets.prepare_instance_targets(view, semantic_loss_on=True, instance_discriminative=True, mode="hip")
    for other in (b, c):                                                        # the contiguous copy; a second call: the same bits
        _same_lists(a, other)
        assert torch.equal(a.planes, other.planes) and torch.equal(a.starts, other.starts) and torch.equal(a.counts, other.counts)
    _planes_agree(a)
    masks = [t["masks"] for t in a]
    assert all(m.dtype == torch.bool and m.is_contiguous() for m in masks)
    assert len({m.untyped_storage().data_ptr() for m in masks}) == 1           # views of one allocation, one after the other
    assert masks[1].data_ptr() == masks[0].data_ptr() + masks[0].numel()
    assert len({t["fg_masks"].untyped_storage().data_ptr() for t in a}) == 1
    # the default mode is the device path where it is supported
    d = targets.prepare_instance_targets(view, semantic_loss_on=True, instance_discriminative=True)
    assert d.planes is not None


def _handoff_case():
    g = torch.Generator().manual_seed(7)
    maps = torch.zeros((2, 64, 64), dtype=torch.int32)
    maps[0, 2:20, 3:30], maps[0, 25:60, 10:28], maps[0, 40:44, 40:63] = 4, 9, 11
    maps[1, 1:9, 1:60], maps[1, 12:31, 5:16], maps[1, 12:31, 20:40], maps[1, 40:63, 2:20], maps[1, 50:60, 30:50] = 2, 7, 8, 300, 4000
    preds = [torch.randn(2, 12, 16, 16, generator=g).cuda() for _ in range(2)]
    emb = torch.randn(2, 16, 16, 16, generator=g).cuda()
    return maps, preds, emb


def test_planes_hand_off_skips_the_concatenation(monkeypatch):
    """forward_many, loss_masks and loss_embedding with the hip switches on: a TargetList hands its planes and index vectors
    over -- no torch.cat of the masks runs -- and every result has the bits the plain list of the same dicts gives."""
    from pctrans_amd import targets
    from pctrans_amd.loss import maskformer_criterion as crit
    from pctrans_amd.loss import matcher as matcher_mod
    maps, preds, emb = _handoff_case()
    handed = targets.prepare_instance_targets(maps, semantic_loss_on=True, device=DEV, mode="hip")
    assert handed.counts_host == [3, 5] and handed.planes is not None
    plain = [dict(t) for t in handed]
    cat_of_masks = []
    real_cat = torch.cat

    def watching_cat(tensors, *a, **kw):
        tensors = list(tensors)
        if tensors and all(torch.is_tensor(t) and t.dtype == torch.bool and t.dim() == 3 for t in tensors):
            cat_of_masks.append(len(tensors))
        return real_cat(tensors, *a, **kw)

    assert crit.torch is torch and matcher_mod.torch is torch
    monkeypatch.setattr(torch, "cat", watching_cat)
    out, cats = {}, {}
    for name, tg in (("handed", handed), ("plain", plain)):
        del cat_of_masks[:]
        c = crit.SetCriterion(1, matcher_mod.Point_HungarianMatcher(num_points=70), {}, 0.1, ["masks", "embedding"], 70, 3.0, 0.75)
        c.point_loss = c.point_select = c.emb_loss = c.matcher.point_sample = c.matcher.match_cost = "hip"
        torch.manual_seed(3)
        indices = c.matcher.forward_many([{"pred_masks": p} for p in preds], tg)
        c.matcher.check()
        torch.manual_seed(4)
        p = preds[0].clone().requires_grad_(True)
        lm = c.loss_masks({"pred_masks": p}, tg, indices[0], 8.0)
        e = emb.clone().requires_grad_(True)
        le = c.loss_embedding(e, tg)
        (lm["loss_mask"] + lm["loss_dice"] + le["loss_emb"]).backward()
        out[name] = (indices, lm, le, p.grad, e.grad)
        cats[name] = list(cat_of_masks)
    monkeypatch.undo()
    assert cats["handed"] == [] and cats["plain"] == [2, 2], cats             # (the plain list: once in the matcher, once in the criterion)
    for a, b in zip(out["handed"][0], out["plain"][0]):
        for (sa, ta), (sb, tb) in zip(a, b):
            assert torch.equal(sa, sb) and torch.equal(ta, tb)
    for k in ("loss_mask", "loss_dice"):
        assert torch.equal(out["handed"][1][k], out["plain"][1][k])
    assert torch.equal(out["handed"][2]["loss_emb"], out["plain"][2]["loss_emb"])
    assert torch.equal(out["handed"][3], out["plain"][3]) and torch.equal(out["handed"][4], out["plain"][4])


def test_model_method_end_to_end():
    """MaskFormer.prepare_instance_targets -> model(volume, targets, True) on the smallest model of the GPU tests: the losses
    from device-built targets against those from torch-mode targets, by the rule the training tests compare two steps with
    (test_head_gpu.py: |a - b| <= 2e-4 max(1, |a|) per loss)."""
    import random
    from pctrans_amd import targets
    from pctrans_amd.arch import maskformer as mfm
    from pctrans_amd.arch.resnet import ResNet
    from pctrans_amd.config import get_cfg
    torch.manual_seed(0)
    cfg = get_cfg(num_queries=12, norm="BN", sem_norm="BN", enc_layers=2, dec_layers=3, train_num_points=512, dataset="BBBC")
    model = mfm.MaskFormer(**mfm.MaskFormer.from_config(cfg, ResNet(18, 3, norm="BN"))).cuda().train()
    H = W = 128
    vol = torch.randn(2, 3, H, W, device="cuda")
    maps = torch.zeros((2, H, W), dtype=torch.int64)                          # the loader's CPU label map
    maps[:, 16:45, 16:45], maps[:, 70:110, 60:101], maps[0, 30:51, 90:111], maps[1, 30:51, 81:102] = 1, 2, 3, 3
    got = model.prepare_instance_targets(maps)
    want = targets.prepare_instance_targets(maps, points_num=1, semantic_loss_on=True, device=vol.device, mode="torch")
    assert got.planes is not None and want.planes is None
    _same_lists(got, want, centres=False)
    assert float(torch.cat([(a["center_points"] - b["center_points"]).abs() for a, b in zip(got, want)]).max()) <= 2.0 ** -23

    def step(tg):
        random.seed(3)
        torch.manual_seed(3)
        losses = model(vol, tg, True)
        return {k: float(v.detach()) for k, v in losses.items() if torch.is_tensor(v)}

    la, lb = step(got), step(want)
    assert la.keys() == lb.keys() and "loss_refpoints" in la and "loss_emb" in la and "loss_sem" in la
    for k in la:
        assert np.isfinite(la[k]) and abs(la[k] - lb[k]) <= 2e-4 * max(1.0, abs(lb[k])), (k, la[k], lb[k])

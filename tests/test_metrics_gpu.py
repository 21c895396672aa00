"""GPU: the validation-metric kernels (pctrans_amd/metrics.py; pct_label_overlap, pct_label_metrics of
include/pctrans_hip_metrics.h) against the literal per-mask definitions and, for maps too large for those, the table-based
numpy reference (tests/metrics_reference.py): integer outputs exact, ratios as the bounds stated there; dtypes, foreground
map, determinism, status bits, refused geometry, and MaskFormer.validation_metrics."""
import functools

import numpy as np
import pytest
import torch

import metrics_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(maps, dtype=torch.int32):
    return torch.from_numpy(np.stack(maps)).to(dtype).to(DEV)


def _rows(result):
    cols = {k: v.cpu().tolist() for k, v in result.items()}
    return [{k: cols[k][n] for k in cols} for n in range(len(next(iter(cols.values()))))]


def _hip_rows(pred, gt, fg=None, check=True):
    """Both metric families of a batch from the kernels -> (one dict per image, status list)."""
    from pctrans_amd import metrics as M
    cv, bb = M.cvppp_metrics(pred, gt, fg, mode="hip", check=check), M.bbbc_metrics(pred, gt, fg, mode="hip", check=check)
    assert cv.mode == bb.mode == "hip" and torch.equal(cv.status, bb.status)
    assert all(v.device == pred.device for v in list(cv.values()) + list(bb.values()))
    assert all(cv[k].dtype == torch.float64 for k in cv) and bb["tp"].dtype == torch.int32 and bb["aji"].dtype == torch.float64
    return [dict(a, **b) for a, b in zip(_rows(cv), _rows(bb))], cv.status.cpu().tolist()


def _check_overlap(ov, n, pred, gt, literal):
    vp, vg, ap, ag, T = (R.literal_table if literal else R.table)(pred, gt)
    H, W = pred.shape
    assert ov.num[n].tolist() == [len(vp), len(vg)]
    assert ov.values[n, 0].tolist() == vp.tolist() + [0] * (512 - len(vp))
    assert ov.values[n, 1].tolist() == vg.tolist() + [0] * (512 - len(vg))
    assert ov.areas[n, 0].tolist() == ap.tolist() + [0] * (512 - len(vp))
    assert ov.areas[n, 1].tolist() == ag.tolist() + [0] * (512 - len(vg))
    assert ov.range[n].tolist() == [[vp[0], vp[-1]], [vg[0], vg[-1]]]
    full = np.zeros((512, 512), dtype=np.int64)
    full[:len(vg), :len(vp)] = T
    assert np.array_equal(ov.table[n].numpy(), full)


@functools.lru_cache(maxsize=None)
def _builder_batch(H, W):
    cases = R.small_builders(H, W)
    names = sorted(cases)
    return names, [cases[k][0] for k in names], [cases[k][1] for k in names]


@functools.lru_cache(maxsize=None)
def _odd_batch():
    """N = 3 images of 37 x 53 -- no multiple of 64, of a vector width or of a workgroup's 256-pixel pass -- with 5, 11 and
    17 instances."""
    gts = [R.random_instances(37, 53, c, seed=c, radius=(3, 6)) for c in (5, 11, 17)]
    return [R.perturbed(g, seed=7 + i) for i, g in enumerate(gts)], gts


def test_three_odd_images_against_the_literal_definitions():
    from pctrans_amd import metrics as M
    preds, gts = _odd_batch()
    assert len({len(np.unique(g)) for g in gts}) == 3 and 37 * 53 % 64 and 37 * 53 > 256
    p, g = _dev(preds, torch.int16), _dev(gts, torch.int64)
    ov = M.label_overlap(p, g, mode="hip")
    assert ov.mode == "hip" and ov.status.cpu().tolist() == [0, 0, 0]
    ov.values, ov.areas, ov.num, ov.range, ov.table = (x.cpu() for x in (ov.values, ov.areas, ov.num, ov.range, ov.table))
    rows, status = _hip_rows(p, g)
    assert status == [0, 0, 0]
    for n in range(3):
        _check_overlap(ov, n, preds[n], gts[n], literal=True)
        want = R.literal(preds[n], gts[n])
        assert want["tp"] >= 1 and 0 < want["aji"] < 1 and 0 < want["sbd"] < 1
        assert not R.mismatches(rows[n], want), (n, R.mismatches(rows[n], want))


@pytest.mark.parametrize("size", [(48, 40), (96, 96)])
def test_builders_against_the_literal_definitions(size):
    from pctrans_amd import metrics as M
    H, W = size
    names, preds, gts = _builder_batch(H, W)
    p, g = _dev(preds), _dev(gts)
    ov = M.label_overlap(p, g, mode="hip")
    ov.values, ov.areas, ov.num, ov.range, ov.table = (x.cpu() for x in (ov.values, ov.areas, ov.num, ov.range, ov.table))
    rows, status = _hip_rows(p, g)
    for n, name in enumerate(names):
        _check_overlap(ov, n, preds[n], gts[n], literal=True)
        want = R.literal(preds[n], gts[n])
        assert not R.mismatches(rows[n], want), (name, R.mismatches(rows[n], want))
        expect = (0 if preds[n].any() else M.STATUS_EMPTY_PRED) | (0 if gts[n].any() else M.STATUS_EMPTY_GT)
        assert status[n] == expect, name
    for name in ("empty_pred", "empty_gt", "empty_both"):
        row = rows[names.index(name)]
        assert row["aji"] == 0 and row["dq"] == 0 and row["pq"] == 0 and row["tp"] == 0, name
    assert all(rows[names.index("empty_both")][k] == 0 for k in R.FLOAT_KEYS + R.INT_KEYS)
    assert rows[names.index("raw_65535")]["abs_diff_fg"] == 0 and int(ov.range[names.index("raw_65535"), 0, 1]) == 65535


def test_512_distinct_values_are_covered_and_513_fall_back():
    from pctrans_amd import metrics as M
    few, many = R.many_values(512), R.many_values(513)
    other = R.perturbed(few, seed=4)
    preds, gts = [few, other, many, few], [other, few, few, many]
    p, g = _dev(preds), _dev(gts)
    ov = M.label_overlap(p, g, mode="hip")
    assert ov.status.cpu().tolist() == [0, 0, M.STATUS_PRED_COUNT, M.STATUS_GT_COUNT]       # that side only
    assert ov.num.cpu().tolist()[2:] == [[513, 512], [512, 513]] and ov.num.cpu().tolist()[0][0] == 512
    ov.values, ov.areas, ov.num, ov.range, ov.table = (x.cpu() for x in (ov.values, ov.areas, ov.num, ov.range, ov.table))
    for n in range(2):
        _check_overlap(ov, n, preds[n], gts[n], literal=False)
    rows, status = _hip_rows(p[:2], g[:2])
    assert status == [0, 0]
    for n in range(2):
        want = R.from_table(preds[n], gts[n])
        assert want["tp"] > 300 and not R.mismatches(rows[n], want), R.mismatches(rows[n], want)
    # the wrapper reads the status word and returns the torch mode's result for the whole call
    res = M.bbbc_metrics(p, g, mode="hip")
    assert res.mode == "torch" and res.status.cpu().tolist() == [0, 0, M.STATUS_PRED_COUNT, M.STATUS_GT_COUNT]
    cv = M.cvppp_metrics(p, g, mode="hip")
    got = [dict(a, **b) for a, b in zip(_rows(cv), _rows(res))]
    for n in range(4):
        assert not R.mismatches(got[n], R.from_table(preds[n], gts[n])), n
    assert M.bbbc_metrics(p, g, mode="hip", check=False).mode == "hip"                       # unread: the caller's decision


@functools.lru_cache(maxsize=None)
def _bbbc_image():
    gt = R.random_instances(520, 696, 200, seed=11, radius=(8, 16))
    return R.perturbed(gt, seed=5), gt


def test_bbbc_size_image_against_the_table_reference():
    from pctrans_amd import metrics as M
    pred, gt = _bbbc_image()
    assert 150 <= len(np.unique(gt)) <= 201
    p, g = _dev([pred], torch.int16), _dev([gt], torch.int16)
    ov = M.label_overlap(p, g, mode="hip")
    ov.values, ov.areas, ov.num, ov.range, ov.table = (x.cpu() for x in (ov.values, ov.areas, ov.num, ov.range, ov.table))
    _check_overlap(ov, 0, pred, gt, literal=False)
    rows, status = _hip_rows(p, g)
    want = R.from_table(pred, gt)
    assert status == [0] and want["tp"] > 100 and want["fp"] > 0 and want["fn"] > 0 and 0.3 < want["aji"] < 1
    assert not R.mismatches(rows[0], want), R.mismatches(rows[0], want)


def test_every_dtype_gives_the_same_bits_and_two_calls_agree():
    from pctrans_amd import metrics as M
    preds, gts = _odd_batch()                                                  # values <= 17: every dtype holds them
    base = None
    for dp, dg in ((torch.uint8, torch.float32), (torch.int16, torch.int64), (torch.int32, torch.uint8),
                   (torch.int64, torch.int16), (torch.float32, torch.int32)):
        p, g = _dev(preds, dp), _dev(gts, dg)
        ov = M.label_overlap(p, g, mode="hip")
        cv, bb = M.cvppp_metrics(p, g, mode="hip"), M.bbbc_metrics(p, g, mode="hip")
        got = [ov.values, ov.areas, ov.num, ov.range, ov.table, ov.status] + [cv[k] for k in sorted(cv)] + [bb[k] for k in sorted(bb)]
        got = [x.clone() for x in got]
        if base is None:
            base = got
            again = M.label_overlap(p, g, mode="hip")
            assert torch.equal(again.table, ov.table) and torch.equal(again.areas, ov.areas)
            cv2 = M.cvppp_metrics(p, g, mode="hip")
            assert all(torch.equal(cv2[k], cv[k]) for k in cv)                 # bit-identical float64
        assert all(torch.equal(a, b) for a, b in zip(got, base)), (dp, dg)


def test_foreground_map_equals_multiplying_first():
    from pctrans_amd import metrics as M
    preds, gts = _odd_batch()
    rng = np.random.RandomState(0)
    fg = [(rng.rand(37, 53) > 0.2) for _ in preds]
    p, g = _dev(preds, torch.int16), _dev(gts, torch.int16)
    want_rows, _ = _hip_rows(_dev([a * b for a, b in zip(preds, fg)], torch.int16), g)
    for f in (torch.from_numpy(np.stack(fg)).to(DEV), torch.from_numpy(np.stack(fg)).to(torch.uint8).to(DEV) * 255):
        rows, status = _hip_rows(p, g, f)
        assert rows == want_rows and status == [0, 0, 0]
    a = M.label_overlap(p, g, torch.from_numpy(np.stack(fg)).to(DEV), mode="hip")
    b = M.label_overlap(_dev([x * y for x, y in zip(preds, fg)], torch.int16), g, mode="hip")
    assert torch.equal(a.table, b.table) and torch.equal(a.values, b.values)
    # a value the kernels do not cover is no error where the foreground map masks it
    bad = _dev(preds, torch.float32)
    bad[0, 3, 4] = 2.5
    f = torch.ones((3, 37, 53), dtype=torch.bool, device=DEV)
    assert M.label_overlap(bad, g, f, mode="hip").status.cpu().tolist()[0] == M.STATUS_PRED_VALUE
    f[0, 3, 4] = False
    assert M.label_overlap(bad, g, f, mode="hip").status.cpu().tolist() == [0, 0, 0]


@pytest.mark.parametrize("value", [-1.0, 70000.0, 2.5])
def test_values_outside_the_tables_set_the_value_bit(value):
    from pctrans_amd import metrics as M
    preds, gts = _odd_batch()
    dtype = torch.float32 if value != int(value) else torch.int32
    good, bad = _dev(preds, dtype), _dev(preds, dtype)
    bad[1, 20, 30] = value
    g = _dev(gts, torch.int32)
    assert M.label_overlap(bad, g, mode="hip").status.cpu().tolist() == [0, M.STATUS_PRED_VALUE, 0]
    assert M.label_overlap(g, bad, mode="hip").status.cpu().tolist() == [0, M.STATUS_GT_VALUE, 0]
    res = M.cvppp_metrics(bad, g, mode="hip")                                  # the wrapper: the torch mode scores the odd value
    assert res.mode == "torch" and res.status.cpu().tolist() == [0, M.STATUS_PRED_VALUE, 0]
    want = M.cvppp_metrics(good, g, mode="hip")
    assert want.mode == "hip" and all(torch.equal(res[k][[0, 2]], want[k][[0, 2]]) for k in want)


def test_refused_geometry_launches_nothing():
    from pctrans_amd import _lib, metrics as M
    L = _lib.lib()
    x = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = x.data_ptr()
    torch.cuda.synchronize()
    assert L.pct_label_overlap(p, 2, p, 2, None, 0, 8, 8, p, p, p, p, p, p, p, None) == -4
    assert L.pct_label_overlap(p, 2, p, 2, None, 1, 4096, 4096, p, p, p, p, p, p, p, None) == -4
    assert L.pct_label_metrics(p, p, p, p, p, 0, p, p, None) == -4
    torch.cuda.synchronize()
    assert not x.any()
    big = torch.zeros((1, 1, 2 ** 24), dtype=torch.uint8, device=DEV)
    assert not M.supported(big, big) and M.cvppp_metrics(big[:, :, :4096], big[:, :, :4096]).mode == "hip"


class _StubHead(torch.nn.Module):
    def __init__(self, masks):
        super().__init__()
        self.masks = masks

    def forward(self, features):
        return {"pred_masks": self.masks}, None


@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_maskformer_validation_metrics(dataset):
    """The smallest whole model of tests/test_postprocess_gpu.py: a stub head in front of the real post-processing."""
    from pctrans_amd import metrics as M
    from pctrans_amd.arch import maskformer as mfm
    from test_postprocess_gpu import _case_masks
    H, W = 96, 88
    masks = torch.stack([torch.nn.functional.pad(_case_masks(c, dataset, H, W), (0, 0, 0, 0, 0, 14))[:14]
                         for c in ("base", "two_clusters", "nested")])
    logits = torch.where(masks, torch.tensor(8.0), torch.tensor(-8.0)).to(DEV)
    net = mfm.MaskFormer(backbone=torch.nn.Identity(), sem_seg_head=_StubHead(logits), criterion=torch.nn.Identity(),
                         num_queries=14, dataset_name=dataset).eval()
    volume = torch.zeros(3, 3, H, W, device=DEV)
    gt = _dev([R.spaced_blocks(H, W, 24, 22), R.random_instances(H, W, 6, seed=2, radius=(8, 14)), np.zeros((H, W), dtype=np.int64)],
              torch.int64)
    fg = gt > 0
    for switch in ("torch", "hip"):
        net.postprocess = switch
        labels, _ = net(volume)
        for f in (None, fg):
            res = net.validation_metrics(volume, gt, f)
            assert torch.equal(res.labels, labels) and res.mode == "hip"
            want = M.instance_metrics(labels, gt, dataset, f)
            assert set(res) == set(want) and all(torch.equal(res[k], want[k]) for k in want)
            assert torch.equal(res.status, want.status)
            host = M.instance_metrics(labels.cpu(), gt.cpu(), dataset, None if f is None else f.cpu(), mode="torch")
            key = "sbd" if dataset == "CVPPP" else "aji"
            assert torch.equal(res[key].cpu(), host[key]) and float(res[key].max()) > 0
    net.train()
    with pytest.raises(RuntimeError, match="eval"):
        net.validation_metrics(volume, gt)

"""GPU: the small-object merging kernels (pct_label_merge_small, pctrans_amd/csrc/label_merge.hip) against the table-based
restatement of the reference's merge_func (tests/label_merge_reference.py) -- maps, tables, merge counts and status exactly, on
every hand-built case and dtype, on random tie-free maps, on a 4 x 530 x 500 batch -- the tie bit, the fallback of the wrapper,
determinism, graph capture, refused arguments, and MaskFormer.test_labels / validation_metrics(merge=True)."""
import functools

import numpy as np
import pytest
import torch

import label_merge_cases as C
import label_merge_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"uint8": (torch.uint8, 255), "int16": (torch.int16, 32767), "int32": (torch.int32, 65535),
          "int64": (torch.int64, 65535), "float32": (torch.float32, 65535)}


@functools.lru_cache(maxsize=None)
def _want(name):
    seg, fg, passes = C.hand()[name]
    return R.merge(seg, passes, fg)


def _groups(names, limit):
    """The named hand-built cases whose values fit `limit`, batched by (shape, passes, gated or not)."""
    groups = {}
    for name in names:
        seg, fg, passes = C.hand()[name]
        if seg.min() >= 0 and seg.max() <= limit and (seg == np.trunc(seg)).all():
            groups.setdefault((seg.shape, passes, fg is not None), []).append(name)
    return groups


def _compare(got, wants, passes, names):
    """Every output of a device call against the restatement of each image."""
    from pctrans_amd import label_merge as LM
    assert got.mode == "hip" and got.status.dtype == torch.int32
    for n, (want, name) in enumerate(zip(wants, names)):
        k = len(want.values)
        assert np.array_equal(got[n].cpu().numpy().astype(np.int64), want.out.astype(np.int64)), name
        assert int(got.num[n]) == k, name
        assert got.status[n].item() == want.status, (name, got.status[n].item(), want.status)
        for mine, theirs in ((got.values, want.values), (got.final, want.final), (got.areas_before, want.before),
                             (got.areas_after, want.after)):
            assert mine[n, :k].cpu().tolist() == [int(v) for v in theirs], name
            assert not mine[n, k:].any(), name
        assert got.merges[n].cpu().tolist() == list(want.merges) + [0] * (LM.MAX_PASSES - len(passes)), name


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_hand_built_cases_against_the_restatement(dtype):
    from pctrans_amd import label_merge as LM
    tdtype, limit = DTYPES[dtype]
    names = sorted(C.tie_free_hand()) + list(C.TIED)
    groups = _groups(names, limit)
    assert sum(len(g) for g in groups.values()) >= (len(names) - 3 if limit < 65535 else len(names))
    for (shape, passes, gated), group in sorted(groups.items()):
        labels = torch.from_numpy(np.stack([C.hand()[k][0] for k in group])).to(tdtype).to(DEV)
        fg = torch.from_numpy(np.stack([C.hand()[k][1] for k in group])).to(DEV) if gated else None
        got = LM.merge_small_objects(labels, fg, passes, mode="hip", check=False)
        assert got.dtype == tdtype and got.shape == labels.shape
        _compare(got, [_want(k) for k in group], passes, group)
        for n, k in enumerate(group):
            assert bool(got.status[n].item() & LM.STATUS_TIE) == (k in C.TIED), k
        if gated:                                                                # a bool gate is the same gate
            again = LM.merge_small_objects(labels, fg != 0, passes, mode="hip", check=False)
            assert torch.equal(again, got)


def test_a_tie_follows_the_library_order():
    from pctrans_amd import label_merge as LM
    seg, _, passes = C.hand()["tie_two_objects"]
    got = LM.merge_small_objects(torch.from_numpy(seg[None]).to(DEV), None, passes, mode="hip")
    assert got.status.cpu().tolist() == [LM.STATUS_TIE]
    assert (got[0].cpu().numpy()[seg == 7] == 3).all()                           # 3 and 9 share the best count: the lower value


@pytest.mark.parametrize("name", sorted(C.UNCOVERED))
def test_check_falls_back_on_values_the_kernels_do_not_cover(name):
    from pctrans_amd import label_merge as LM
    seg, _, passes = C.hand()[name]
    good = C.hand()["gaps" if seg.shape == (C.SIDE, C.SIDE) else "count_512"][0]
    tdtype = torch.float32 if name == "fractional_value" else torch.int32
    labels = torch.from_numpy(np.stack([good, seg, good])).to(tdtype).to(DEV)
    raw = LM.merge_small_objects(labels, None, passes, mode="hip", check=False)
    assert raw.status.cpu().tolist() == [0, C.UNCOVERED[name], 0]
    got = LM.merge_small_objects(labels, None, passes, mode="hip")
    assert got.mode == "hip" and got.status.cpu().tolist() == [0, C.UNCOVERED[name], 0]
    want = R.merge(seg, passes)
    assert np.array_equal(got[1].cpu().numpy().astype(np.float64), want.out.astype(np.float64))
    assert got.merges[1, :len(passes)].cpu().tolist() == want.merges
    assert torch.equal(got[[0, 2]], raw[[0, 2]]) and np.array_equal(got[0].cpu().numpy(), R.merge(good, passes).out)


@pytest.mark.parametrize("size", [(37, 53), (64, 64)])
def test_random_tie_free_maps(size):
    from pctrans_amd import label_merge as LM
    H, W = size
    maps, draws = C.random_tie_free(H, W, 8, 11)
    assert draws <= 16                                                           # the filter drops at most half of the draws
    rng = np.random.default_rng(5)
    fg = (rng.random(maps.shape) > 0.02).astype(np.uint8)
    fg[::2] = 1
    wants = [R.merge(m, fg=f) for m, f in zip(maps, fg)]
    keep = [n for n, w in enumerate(wants) if w.ties == 0]                       # (the gate can make a tie)
    assert len(keep) >= 4 and sum(sum(wants[n].merges) for n in keep) >= 8
    labels = torch.from_numpy(maps[keep]).to(torch.int16).to(DEV)
    got = LM.merge_small_objects(labels, torch.from_numpy(fg[keep]).to(DEV), mode="hip", check=False)
    _compare(got, [wants[n] for n in keep], R.PASSES, keep)
    assert not got.status.any()


@functools.lru_cache(maxsize=None)
def _large():
    maps, draws = C.random_tie_free(530, 500, 4, 3, fragments=60)
    assert draws <= 8
    return maps, [R.merge(m) for m in maps]


def test_large_batch_twice_sliced_and_unaligned():
    from pctrans_amd import label_merge as LM
    maps, wants = _large()
    assert sum(sum(w.merges) for w in wants) >= 40
    labels = torch.from_numpy(maps).to(torch.int32).to(DEV)
    got = LM.merge_small_objects(labels, mode="hip", check=False)
    _compare(got, wants, R.PASSES, range(4))
    again = LM.merge_small_objects(labels, mode="hip", check=False)
    for a, b in ((again, got), (again.final, got.final), (again.areas_after, got.areas_after), (again.merges, got.merges)):
        assert torch.equal(a, b)
    # a slice (made contiguous by the wrapper), a width that is no multiple of 16 and a base that is not 16-byte aligned
    for tdtype in (torch.uint8, torch.int16, torch.int64, torch.float32):
        part = np.ascontiguousarray(maps[:2, 3:260, 5:232] % 251)                # 257 x 227
        wide = torch.zeros((2, 260, 240), dtype=tdtype, device=DEV)
        wide[:, 3:, 5:232] = torch.from_numpy(part).to(tdtype).to(DEV)
        sliced = wide[:, 3:, 5:232]
        assert not sliced.is_contiguous()
        want = [R.merge(p) for p in part]
        one = LM.merge_small_objects(sliced, mode="hip", check=False)
        flat = torch.zeros(part.size + 1, dtype=tdtype, device=DEV)
        flat[1:] = sliced.reshape(-1)
        shifted = flat[1:].view(part.shape)
        assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
        two = LM.merge_small_objects(shifted, mode="hip", check=False)
        for n in range(2):
            assert np.array_equal(one[n].cpu().numpy().astype(np.int64), want[n].out), tdtype
        assert torch.equal(one, two) and torch.equal(one.final, two.final) and torch.equal(one.status, two.status)
        assert [int(s) & ~LM.STATUS_TIE for s in one.status.cpu().tolist()] == [0, 0]


def test_replay_under_a_captured_graph():
    from pctrans_amd import label_merge as LM
    maps, _ = C.random_tie_free(64, 64, 8, 11)
    static = torch.from_numpy(maps[:4]).to(torch.int16).to(DEV)
    want = [R.merge(m) for m in maps]
    LM.merge_small_objects(static, mode="hip", check=False)                      # warm-up: the workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = LM.merge_small_objects(static, mode="hip", check=False)
    for lo in (0, 4):
        static.copy_(torch.from_numpy(maps[lo:lo + 4]).to(torch.int16))
        graph.replay()
        torch.cuda.synchronize()
        _compare(out, want[lo:lo + 4], R.PASSES, range(lo, lo + 4))


def test_refused_arguments_launch_nothing():
    from pctrans_amd import _lib, label_merge as LM
    import ctypes
    L = _lib.lib()
    x = torch.zeros(LM.WORKSPACE_PER_IMAGE // 4, dtype=torch.int32, device=DEV)
    p = x.data_ptr()
    torch.cuda.synchronize()
    call = lambda N, H, W, passes, dtype=2: L.pct_label_merge_small(
        p, dtype, None, N, H, W, ctypes.cast((ctypes.c_int32 * len(passes))(*passes), ctypes.c_void_p), len(passes) // 2,
        p, p, p, p, p, p, p, p, p, None)
    assert call(0, 8, 8, [5, 5]) == -4 and call(1, 4096, 4096, [5, 5]) == -4 and call(1, 8, 8, [5, 5], dtype=5) == -4
    assert call(1, 8, 8, [5, 32]) == -1 and call(1, 8, 8, [-1, 5]) == -1 and call(1, 8, 8, []) == -1 and call(1, 0, 8, [5, 5]) == -1
    torch.cuda.synchronize()
    assert not x.any()


FRAGMENTS = ((6, 7), (7, 7), (6, 8), (5, 9), (3, 15), (4, 11))


class _StubHead(torch.nn.Module):
    def __init__(self, masks):
        super().__init__()
        self.masks = masks

    def forward(self, features):
        return {"pred_masks": self.masks}, None


def test_maskformer_test_labels_and_merged_validation_metrics():
    """The smallest whole model of tests/test_postprocess_gpu.py: a stub head in front of the real post-processing.  Each query
    is a rectangle: four large objects and ten fragments of 42 - 49 pixels (the post-processing drops a mask of 40 or fewer)."""
    from pctrans_amd import label_merge as LM, metrics as M
    from pctrans_amd.arch import maskformer as mfm
    H, W, Q = 96, 88, 14
    rng = np.random.default_rng(2)
    masks = torch.zeros((2, Q, H, W), dtype=torch.bool)
    for n in range(2):
        for q in range(Q):
            h, w = (int(rng.integers(20, 40)), int(rng.integers(20, 40))) if q < 4 else FRAGMENTS[int(rng.integers(0, len(FRAGMENTS)))]
            y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            masks[n, q, y:y + h, x:x + w] = True
    logits = torch.where(masks, torch.tensor(8.0), torch.tensor(-8.0)).to(DEV)
    net = mfm.MaskFormer(backbone=torch.nn.Identity(), sem_seg_head=_StubHead(logits), criterion=torch.nn.Identity(),
                         num_queries=Q, dataset_name="CVPPP").eval()
    volume = torch.zeros(2, 3, H, W, device=DEV)
    gt = torch.from_numpy(np.stack([C.random_map(rng, H, W), C.random_map(rng, H, W)])).to(DEV)
    fg = torch.ones((2, H, W), dtype=torch.uint8, device=DEV)
    fg[:, :, :6] = 0
    for switch in ("torch", "hip"):
        net.postprocess = switch
        labels, _ = net(volume)
        for f in (None, fg):
            got = net.test_labels(volume, f)
            host = LM.merge_small_objects(labels.cpu(), None if f is None else f.cpu(), mode="torch")
            assert got.mode == "hip" and host.mode == "torch" and got.dtype == labels.dtype
            assert torch.equal(got.cpu(), host) and int(host.merges.sum()) > 0
            assert not torch.equal(got, labels if f is None else labels * f.to(labels.dtype))
            res = net.validation_metrics(volume, gt, f, merge=True)
            assert torch.equal(res.labels, got)
            want = M.instance_metrics(got, gt, "CVPPP")
            assert all(torch.equal(res[k], want[k]) for k in want)
            plain = net.validation_metrics(volume, gt, f)
            assert torch.equal(plain.labels, labels)
    net.train()
    with pytest.raises(RuntimeError, match="eval"):
        net.test_labels(volume)

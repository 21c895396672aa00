"""GPU: the device post-processing (pctrans_amd/postprocess.py; pct_instance_masks_*, pct_instance_labels_from_bits,
pct_instance_labels_* of include/pctrans_hip_post.h) against the literal restatement of the reference's instance_inference
(exact, on hard logits), against the float64 resize outside the band fp32 cannot decide (threshold stage), and against the
float64 helper fed the kernel's own bits (whole path); MaskFormer's switch, graph replay, stray writes."""
import functools

import pytest
import torch

import postprocess_reference as R
from test_arch_cpu import _instance_inference_literal, instance_logits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("base", "two_clusters", "hard_merge_drops", "nested", "floor_40_41", "no_survivor", "all_identical")


def _rect(H, W, y0, y1, x0, x1, extra=()):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[y0:y1, x0:x1] = True
    for y, x in extra:
        m[y, x] = True
    return m


def _case_masks(case, dataset, H, W, seed=0):
    """The real (non-empty) queries of a case as bool [k, H, W]; everything sits in the top-left 96 x 88 pixels."""
    if case == "base":
        return instance_logits(seed, H, W).sigmoid().float() > R.PARAMS[dataset]["t"]
    if case == "two_clusters":        # dice(A, B) and dice(B, C) above thres1, dice(A, C) below: B sits in both clusters
        if dataset == "CVPPP":
            return torch.stack([_rect(H, W, 10, 30, 10, 50), _rect(H, W, 10, 30, 25, 65), _rect(H, W, 10, 30, 38, 80)])
        return torch.stack([_rect(H, W, 10, 30, 10, 40), _rect(H, W, 10, 30, 30, 60), _rect(H, W, 10, 30, 50, 82)])
    if case == "hard_merge_drops":    # one cluster of three shifted copies: 2 of 3 is above 0.6, 1 of 3 is not
        return torch.stack([_rect(H, W, 40, 60, 10, 50), _rect(H, W, 41, 61, 14, 54), _rect(H, W, 42, 62, 18, 58),
                            _rect(H, W, 70, 90, 60, 85)])
    if case == "nested":              # a small mask inside a large one (NMS drops it on CVPPP), a third overlapping the large one
        return torch.stack([_rect(H, W, 5, 45, 5, 45), _rect(H, W, 20, 30, 20, 30), _rect(H, W, 5, 45, 30, 71),
                            _rect(H, W, 60, 80, 10, 33)])
    if case == "floor_40_41":         # 40 pixels: dropped; 41: kept
        return torch.stack([_rect(H, W, 10, 15, 10, 18), _rect(H, W, 30, 35, 10, 18, extra=[(35, 10)]),
                            _rect(H, W, 50, 70, 40, 70)])
    if case == "no_survivor":
        return torch.stack([_rect(H, W, 10, 15, 10, 18), _rect(H, W, 30, 33, 10, 14), _rect(H, W, 50, 51, 40, 41)])
    if case == "all_identical":
        return _rect(H, W, 20, 50, 15, 60)[None]
    raise KeyError(case)


def _slots(case, k, Q):
    """Where the real queries go: spread over the Q slots, so that they fall into different words of the kernels' query sets;
    the other slots are empty.  In 'all_identical' every slot holds the same mask."""
    return list(range(Q)) if case == "all_identical" else [(r * Q) // k for r in range(k)]


def _hard_logits(case, dataset, Q, H, W, device="cpu"):
    real = _case_masks(case, dataset, H, W).to(device)
    slots = _slots(case, real.shape[0], Q)
    assert len(set(slots)) == len(slots)
    logits = torch.full((Q, H, W), -8.0, device=device)
    logits[slots] = torch.where(real, 8.0, -8.0).to(device) if case != "all_identical" else torch.where(real, 8.0, -8.0).expand(Q, H, W)
    return logits


@functools.lru_cache(maxsize=None)
def _hard_want(case, dataset, Q, H, W):
    """The literal restatement's label map [H, W] for logits of +-8 at output resolution."""
    logits = _hard_logits(case, dataset, Q, H, W)
    masks = logits > 0
    # on the reference alone: no argsort tie, which torch leaves undefined, decides a label
    ref, info = R.labels_from_masks(masks, dataset)
    assert R.areas_distinct(info, dataset), (case, dataset, info)
    assert all(m > 1e-4 for m in info["margins"].values()), (case, dataset, info["margins"])     # ... and no threshold does
    if int((masks.flatten(1).sum(1) > 40).sum()) == 0:
        want = torch.zeros(H, W, dtype=torch.int16)              # the reference returns an all-zero map (:287-288)
    else:
        want = _instance_inference_literal(logits, dataset)[0]
    assert torch.equal(ref, want), (case, dataset)               # the float64 helper agrees as well
    return want


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("size", [(96, 88), (520, 696), (512, 512)])
@pytest.mark.parametrize("Q", [14, 100, 300])
@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_exact_on_hard_logits(dataset, Q, size, N):
    from pctrans_amd import postprocess as post
    H, W = size
    groups = [CASES[i:i + 1] for i in range(len(CASES))] if N == 1 else [CASES[0:3], CASES[3:6], (CASES[6], CASES[0], CASES[3])]
    seen = set()
    for group in groups:
        wants = [_hard_want(c, dataset, Q, H, W) for c in group]
        logits = torch.stack([_hard_logits(c, dataset, Q, H, W, DEV) for c in group])
        got = post.instance_labels(logits, size, dataset)
        assert got.shape == (N, H, W) and got.dtype == torch.int16
        got = got.cpu()
        for n, (c, want) in enumerate(zip(group, wants)):
            assert torch.equal(got[n], want), (c, dataset, Q, size, n, int((got[n] != want).sum()))
            seen.add(c)
    assert seen == set(CASES)
    assert int(_hard_want("no_survivor", dataset, Q, H, W).max()) == 0
    assert int(_hard_want("nested", dataset, Q, H, W).max()) >= 2


def _soft_logits(N, Q, h, w, seed):
    """Soft-edged discs whose logits cross both thresholds over a few pixels, some near-duplicates, some empty queries."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    out = torch.full((N, Q, h, w), -9.0)
    for n in range(N):
        for q in range(0, Q, 2):
            cy, cx = float(torch.rand((), generator=g)) * h, float(torch.rand((), generator=g)) * w
            r = 4.0 + float(torch.rand((), generator=g)) * min(h, w) / 6
            d = torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            out[n, q] = (r - d) * 0.9 + 0.05 * torch.randn(h, w, generator=g)
            if q % 6 == 0 and q + 1 < Q:                          # a near-duplicate of its neighbour: merged
                out[n, q + 1] = (r * 1.03 - d) * 0.9 + 0.05 * torch.randn(h, w, generator=g)
    return out


THRESHOLD_CASES = [((512, 512), (256, 256)), ((520, 696), (260, 348)), ((512, 512), (512, 512)), ((520, 696), (520, 696)),
                   ((96, 88), (48, 44)), ((96, 88), (96, 88))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("size,src", THRESHOLD_CASES)
@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_threshold_stage_against_float64(dataset, size, src, dtype):
    from pctrans_amd import postprocess as post
    H, W = size
    N, Q = 2, 5
    logits = _soft_logits(N, Q, src[0], src[1], seed=H + src[0]).to(dtype)
    x64 = R.resize64(logits, size)                                # of the values the kernel reads (bf16 ones included)
    want = R.threshold64(x64, dataset)
    band = R.ambiguous_band(x64, dataset, logits.double().abs().max())
    share = float(band.double().mean())
    print("threshold stage %s %s <- %s %s: banded share %.3g" % (dataset, size, src, dtype, share))
    assert share <= 1e-3                                          # on the reference alone
    bits, areas = post.instance_masks(logits.to(DEV), size, dataset)
    assert bits.shape == (N, Q, R.plane_words(H, W)) and bits.dtype == torch.int32 and areas.dtype == torch.int32
    got, pad = R.unpack_bits(bits.cpu(), H, W)
    assert not pad.any()                                          # the padding past H*W is written as zero
    wrong = (got != want) & ~band
    assert int(wrong.sum()) == 0, int(wrong.sum())
    assert torch.equal(areas.cpu().long(), got.flatten(2).sum(2))
    assert int(want.sum()) > 100 * N and int((~want).sum()) > 100 * N


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("size,src,Q", [((512, 512), (256, 256), 100), ((520, 696), (260, 348), 40), ((96, 88), (96, 88), 14)])
@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_whole_path_equals_float64_helper_on_the_kernels_bits(dataset, size, src, Q, dtype):
    """Rounding lives in the threshold stage only: from the bits on, everything is exact."""
    from pctrans_amd import postprocess as post
    H, W = size
    N = 2
    logits = (instance_logits(5, H, W)[None].repeat(N, 1, 1, 1) if src == size and Q == 14 else
              _soft_logits(N, Q, src[0], src[1], seed=Q)).to(dtype).to(DEV)
    bits, areas = post.instance_masks(logits, size, dataset)
    labels = post.instance_labels(logits, size, dataset).cpu()
    staged = post.instance_labels_from_bits(bits, areas, size, dataset).cpu()
    masks, _ = R.unpack_bits(bits.cpu(), H, W)
    for n in range(N):
        want, info = R.labels_from_masks(masks[n], dataset)
        assert torch.equal(labels[n], want), (n, int((labels[n] != want).sum()))
        assert torch.equal(staged[n], want), n
        assert int(want.max()) >= 3


@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_long_thin_geometry_at_the_limit_of_the_tap_tables(dataset):
    """H + W = 8000, the largest the resize's LDS tables allow: threshold stage against float64, labels against the helper."""
    from pctrans_amd import postprocess as post
    size, src, N, Q = (7000, 1000), (3500, 500), 1, 4
    H, W = size
    logits = _soft_logits(N, Q, src[0], src[1], seed=7)
    x64 = R.resize64(logits, size)
    band = R.ambiguous_band(x64, dataset, logits.double().abs().max())
    assert float(band.double().mean()) <= 1e-3
    bits, areas = post.instance_masks(logits.to(DEV), size, dataset)
    got, pad = R.unpack_bits(bits.cpu(), H, W)
    assert not pad.any() and int(((got != R.threshold64(x64, dataset)) & ~band).sum()) == 0
    assert torch.equal(areas.cpu().long(), got.flatten(2).sum(2)) and int(areas.max()) > 1000
    labels = post.instance_labels(logits.to(DEV), size, dataset).cpu()
    want, _ = R.labels_from_masks(got[0], dataset)
    assert torch.equal(labels[0], want) and int(want.max()) >= 1


class _StubHead(torch.nn.Module):
    def __init__(self, masks):
        super().__init__()
        self.masks = masks

    def forward(self, features):
        return {"pred_masks": self.masks}, None


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_maskformer_hip_equals_torch_on_hard_logits(dataset, half):
    """Through MaskFormer.forward with a stub head.  `half`: the head's masks are at half resolution, +-8 in blocks: their
    bilinear resize takes values in {0, +-4, +-8} only, exact in fp32 and far from both thresholds."""
    from pctrans_amd.arch import maskformer as mfm
    H, W = 96, 88
    cases = ("base", "two_clusters", "nested")
    if half:
        masks = torch.stack([torch.nn.functional.pad(_case_masks(c, dataset, H // 2, W // 2), (0, 0, 0, 0, 0, 14))[:14]
                             for c in cases])
    else:
        masks = torch.stack([torch.nn.functional.pad(_case_masks(c, dataset, H, W), (0, 0, 0, 0, 0, 14))[:14] for c in cases])
    logits = torch.where(masks, torch.tensor(8.0), torch.tensor(-8.0)).to(DEV)
    net = mfm.MaskFormer(backbone=torch.nn.Identity(), sem_seg_head=_StubHead(logits), criterion=torch.nn.Identity(),
                         num_queries=14, dataset_name=dataset).eval()
    volume = torch.zeros(3, 3, H, W, device=DEV)
    assert net.postprocess == "torch"
    want, bd0 = net(volume)
    net.postprocess = "hip"
    got, bd1 = net(volume)
    assert bd0 is None and bd1 is None and got.dtype == want.dtype == torch.int16 and got.shape == want.shape == (3, H, W)
    assert torch.equal(got, want) and int(want.max()) >= 2
    with torch.autocast("cuda", dtype=torch.bfloat16):
        net.sem_seg_head.masks = logits.bfloat16()
        assert torch.equal(net(volume)[0], want)


@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_captured_graph_replays_with_fresh_inputs(dataset):
    from pctrans_amd import postprocess as post
    size, N, Q = (96, 88), 2, 14
    half = lambda seed: torch.nn.functional.avg_pool2d(instance_logits(seed)[None], 2)[0]        # [14, 48, 44]
    inputs = [torch.stack([half(s), half(s + 10)]) for s in (1, 2, 3)]
    eager = [post.instance_labels(x.to(DEV), size, dataset).clone() for x in inputs]
    static = inputs[0].to(DEV).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = post.instance_labels(static, size, dataset)
    for x, want in list(zip(inputs, eager))[::-1]:
        static.copy_(x.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and int(want.max()) >= 3
    assert not torch.equal(eager[0], eager[1])


@pytest.mark.parametrize("dataset", ["CVPPP", "BBBC"])
def test_nothing_but_the_outputs_is_written_and_no_stale_workspace_is_read(dataset):
    """Through the C ABI with guard words around the workspace and the labels, an input that must stay as it is, and two
    different poisons in the workspace: the same labels both times, the guards untouched."""
    from pctrans_amd import _lib
    from pctrans_amd import postprocess as post
    size, N, Q = (96, 88), 2, 14
    H, W = size
    logits = torch.nn.functional.avg_pool2d(torch.stack([instance_logits(4), instance_logits(6)]), 2).contiguous().to(DEV)
    before = logits.clone()
    want = post.instance_labels(logits, size, dataset)
    nbytes, G = post.workspace_bytes(N, Q, H, W), 4096
    results = []
    for poison in (0xA5, 0x5A, 0xFF):
        ws = torch.full((G + nbytes + G,), poison, dtype=torch.uint8, device=DEV)
        lab = torch.full((G + N * H * W + G,), 0x7B7B, dtype=torch.int16, device=DEV)
        assert (ws.data_ptr() + G) % 16 == 0
        rc = _lib.lib().pct_instance_labels_f32(logits.data_ptr(), N, Q, 48, 44, H, W, post.DATASETS[dataset], ws.data_ptr() + G,
                                                lab.data_ptr() + 2 * G, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((ws[:G] == poison).all()) and bool((ws[G + nbytes:] == poison).all())
        assert bool((lab[:G] == 0x7B7B).all()) and bool((lab[G + N * H * W:] == 0x7B7B).all())
        results.append(lab[G:G + N * H * W].reshape(N, H, W).clone())
    assert all(torch.equal(r, want) for r in results)
    assert torch.equal(logits, before)

"""GPU: the pixel-embedding loss on the device (pctrans_amd/embedding_loss.py; pct_instance_label_map_f32,
pct_discriminative_loss_forward_f32, pct_discriminative_loss_backward_f32) against the golden fixture, against float64 inside the
bound of embedding_loss_reference.py, and its label map bit for bit against F.interpolate + argmax."""
import os

import numpy as np
import pytest
import torch

import embedding_loss_reference as R
from pctrans_amd import _lib, embedding_loss
from pctrans_amd.loss import maskformer_criterion as crit
from pctrans_amd.loss.matcher import Point_HungarianMatcher

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _run(emb, lab, L, params=R.PARAMS, grad_out=1.0):
    x = emb.to(DEV).requires_grad_(True)
    loss = embedding_loss.discriminative_loss(x, lab.to(DEV), L, **params)
    grad, = torch.autograd.grad(loss * grad_out, x)
    return loss.detach(), grad, loss.status


def _criterion(mode):
    c = crit.SetCriterion(1, Point_HungarianMatcher(num_points=16), {}, 0.1, ["embedding"], 16, 3.0, 0.75)
    c.emb_loss = mode
    return c


def _close(got, want, rtol, atol, what):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).double()
    assert bool(((got - want).abs() <= rtol * want.abs() + atol).all()), (what, float((got - want).abs().max()))


def test_golden_fixture():
    """The reference's own numbers, at the tolerances tests/test_criterion_golden.py applies to the torch path."""
    with np.load(os.path.join(ROOT, "tests", "golden", "loss_criterion.npz")) as z:
        g = {k: z[k] for k in ("emb", "seg_gt", "loss_emb", "grad_emb", "loss_emb_params")}
    emb, gt = torch.from_numpy(g["emb"]), torch.from_numpy(g["seg_gt"])
    assert tuple(emb.shape) == (3, 8, 12, 10)
    loss, grad, status = _run(emb, gt, 9)
    _close(loss, g["loss_emb"], 2e-5, 1e-6, "discriminative_loss")
    _close(grad, g["grad_emb"], 2e-4, 1e-7, "d discriminative_loss / d embedding")
    other, _, _ = _run(emb, gt, 9, R.OTHER_PARAMS)
    _close(other, g["loss_emb_params"], 2e-5, 1e-6, "discriminative_loss with non-default margins / weights")
    assert int(status) == 0


@pytest.mark.parametrize("name,E,h,w,L", R.cases())
def test_value_and_gradient_against_float64(name, E, h, w, L):
    emb, lab = R.family(name, E, h, w, L)
    want, wgrad, lb, gb = R.expected(name, E, h, w, L)
    loss, grad, status = _run(emb, lab, L)
    err = abs(float(loss) - want)
    excess = float(((grad.cpu().double() - wgrad).abs() - gb).max())
    print("%s E=%d %dx%d L=%d: loss %.9g err %.3g bound %.3g; gradient excess over its bound %.3g (largest bound %.3g)"
          % (name, E, h, w, L, want, err, lb, excess, float(gb.max())))
    assert err <= lb
    assert excess <= 0
    assert int(status) == 0
    outside = (R.clean_labels(lab, L) == 0)[:, None].expand_as(grad)
    assert float(grad.cpu()[outside].abs().max() if outside.any() else 0.0) == 0.0


def test_non_default_parameters_and_incoming_gradient():
    name, E, h, w, L = "near and far centroids", 16, 13, 11, 33
    emb, lab = R.family(name, E, h, w, L)
    want, wgrad = R.loss64(emb, lab, L, grad_out=-2.5, **R.OTHER_PARAMS)
    lb, gb = R.bounds(emb, lab, L, grad_out=-2.5, **R.OTHER_PARAMS)
    loss, grad, _ = _run(emb, lab, L, R.OTHER_PARAMS, grad_out=-2.5)
    assert abs(float(loss) - want) <= lb
    assert float(((grad.cpu().double() - wgrad).abs() - gb).max()) <= 0


def test_out_of_range_labels_are_counted_and_count_as_background():
    emb, lab = R.family("near and far centroids", 16, 67, 61, 31)
    lab = lab.clone()
    bad = torch.zeros_like(lab, dtype=torch.bool)
    bad[0, 3, ::7] = bad[1, 40:42, 5:9] = bad[1, 66, 60] = True
    lab[bad] = torch.tensor([32, -1, 1000, -2 ** 31, 2 ** 31 - 1], dtype=torch.int32).repeat(bad.sum() // 5 + 1)[:int(bad.sum())]
    loss, grad, status = _run(emb, lab, 31)
    assert int(status) == int(bad.sum())
    clean = R.clean_labels(lab, 31).to(torch.int32)
    loss2, grad2, status2 = _run(emb, clean, 31)
    assert int(status2) == 0 and torch.equal(loss, loss2) and torch.equal(grad, grad2)
    assert float(grad.cpu()[bad[:, None].expand_as(grad)].abs().max()) == 0.0


SIZES = [((48, 64), (12, 16)), ((50, 70), (13, 18)), ((64, 64), (8, 8))]


def _masks(size, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = size
    a = torch.zeros(5, H, W)
    a[0, : H // 2, : W // 2] = 1                       # overlapped by plane 1: the lowest index wins
    a[1, : H // 2 + 5, 3:] = 2.5
    a[2, 1, 1] = 1                                     # one pixel that no output pixel samples: vanishes under the resize
    a[3] = (torch.rand(H, W, generator=g) > 0.5).float()
    a[4, H // 2:, :] = 1
    a[4, H - 4, W - 4] = float("nan")                   # a NaN is not positive
    a[4, H - 8, W - 8] = -1.0
    b = torch.zeros(0, H, W)
    c = (torch.rand(3, H, W, generator=g) > 0.8).float()
    return [a, b, c]


@pytest.mark.parametrize("size,out", SIZES)
def test_label_map_is_bit_exact(size, out):
    masks = [m.to(DEV) for m in _masks(size, seed=size[0])]
    want = R.label_map_reference(masks, out)
    counts = [m.shape[0] for m in masks]
    starts = [sum(counts[:b]) for b in range(len(counts))]
    planes = torch.cat(masks).contiguous()
    got = embedding_loss.instance_label_map(planes, torch.tensor(starts, dtype=torch.int32, device=DEV),
                                            torch.tensor(counts, dtype=torch.int32, device=DEV), out)
    assert got.dtype == torch.int32 and torch.equal(got.long(), want)
    assert int(want[1].max()) == 0 and not bool((want[0] == 3).any()) and bool((want[0] == 1).any()) and bool((want[0] == 2).any())


def _targets(sizes, counts, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [{"masks": (torch.rand(n, *s, generator=g) > 0.9).to(DEV)} for n, s in zip(counts, sizes)]


def test_set_criterion_hip_against_torch(monkeypatch):
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(2, 16, 13, 18, generator=g)
    targets = _targets([(50, 70)] * 2, (7, 40))
    labels = R.label_map_reference([t["masks"] for t in targets], (13, 18)).cpu()
    want, wgrad = R.loss64(emb, labels, 40)
    lb, gb = R.bounds(emb, labels, 40)
    calls = []
    real = embedding_loss.discriminative_loss
    monkeypatch.setattr(embedding_loss, "discriminative_loss", lambda *a, **k: calls.append(a[2]) or real(*a, **k))
    for mode in ("torch", "hip"):
        x = emb.to(DEV).requires_grad_(True)
        loss = _criterion(mode).loss_embedding(x, targets)["loss_emb"]
        loss.backward()
        assert abs(float(loss) - want) <= lb, mode
        assert float(((x.grad.cpu().double() - wgrad).abs() - gb).max()) <= 0, mode
        assert calls == ([] if mode == "torch" else [40])                   # the device path ran, with L = the largest count
    assert int(loss.status) == 0


def test_set_criterion_masks_of_differing_sizes_take_the_torch_path(monkeypatch):
    g = torch.Generator().manual_seed(10)
    emb = torch.randn(2, 16, 13, 18, generator=g)
    targets = _targets([(50, 70), (52, 72)], (3, 4))
    got = {}
    for mode in ("torch", "hip"):
        if mode == "hip":
            monkeypatch.setattr(embedding_loss, "discriminative_loss",
                                lambda *a, **k: (_ for _ in ()).throw(AssertionError("device path on masks of two sizes")))
        x = emb.to(DEV).requires_grad_(True)
        loss = _criterion(mode).loss_embedding(x, targets)["loss_emb"]
        loss.backward()
        got[mode] = (loss.detach(), x.grad)
    assert torch.equal(got["torch"][0], got["hip"][0]) and torch.equal(got["torch"][1], got["hip"][1])


def test_two_calls_give_identical_bits():
    emb, lab = R.family("near and far centroids", 16, 67, 61, 70)
    a, b = _run(emb, lab, 70), _run(emb, lab, 70)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _guarded(shape, dtype, fill):
    """A tensor of `shape` inside a sentinel-filled buffer with 64 elements of margin on either side."""
    n = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((n + 128,), fill, dtype=dtype, device=DEV)
    return buf, buf[64:64 + n].view(shape)


def _margins_untouched(buf, fill):
    return bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all())


def test_guard_bands():
    """Every output of the three entries inside a sentinel-filled buffer: the margins stay as they were."""
    E, h, w, L, B = 3, 13, 11, 33, 2
    emb, lab = R.family("near and far centroids", E, h, w, L)
    emb, lab = emb.to(DEV), lab.to(DEV)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    ws_n = embedding_loss.workspace_bytes(B, h * w, L) // 4
    fb, ib = -7.25, -77
    ws_buf, ws = _guarded((ws_n,), torch.float32, fb)
    tb_buf, table = _guarded((B, L + 1, embedding_loss.TABLE_ROW), torch.float32, fb)
    lo_buf, loss = _guarded((), torch.float32, fb)
    st_buf, status = _guarded((), torch.int32, ib)
    gr_buf, grad = _guarded((B, E, h, w), torch.float32, fb)
    assert ws.data_ptr() % 16 == 0
    rc = lib.pct_discriminative_loss_forward_f32(emb.data_ptr(), lab.data_ptr(), B, E, h, w, L, 0.5, 3.0, 1.0, 1.0, 0.001,
                                                 ws.data_ptr(), table.data_ptr(), loss.data_ptr(), status.data_ptr(), stream)
    assert rc == 0
    go = torch.ones((), device=DEV)
    rc = lib.pct_discriminative_loss_backward_f32(emb.data_ptr(), lab.data_ptr(), table.data_ptr(), go.data_ptr(), B, E, h, w, L,
                                                  0.5, grad.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, fill in ((ws_buf, fb), (tb_buf, fb), (lo_buf, fb), (st_buf, ib), (gr_buf, fb)):
        assert _margins_untouched(buf, fill)
    want = _run(emb.cpu(), lab.cpu(), L)
    assert torch.equal(loss, want[0]) and torch.equal(grad, want[1]) and int(status) == 0
    assert not bool((table == fb).any())                                   # the table is fully overwritten
    # label map
    masks = _masks((50, 70), seed=1)
    counts = [m.shape[0] for m in masks]
    planes = torch.cat(masks).to(DEV)
    starts = torch.tensor([sum(counts[:b]) for b in range(3)], dtype=torch.int32, device=DEV)
    lb_buf, labels = _guarded((3, 13, 18), torch.int32, ib)
    rc = lib.pct_instance_label_map_f32(planes.data_ptr(), planes.shape[0], 50, 70, starts.data_ptr(),
                                        torch.tensor(counts, dtype=torch.int32, device=DEV).data_ptr(), 3, 13, 18,
                                        labels.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert _margins_untouched(lb_buf, ib) and int(labels.min()) >= 0


def test_graph_capture_replays_the_eager_bits():
    emb, lab = R.family("near and far centroids", 16, 67, 61, 33)
    eager = _run(emb, lab, 33)
    before = os.environ.get("GPU_MAX_HW_QUEUES")
    x = emb.to(DEV).requires_grad_(True)
    labels = lab.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                          # warm-up outside the capture
        loss = embedding_loss.discriminative_loss(x, labels, 33)
        torch.autograd.grad(loss, x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = embedding_loss.discriminative_loss(x, labels, 33)
        grad, = torch.autograd.grad(loss, x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), eager[0]) and torch.equal(grad, eager[1])
    assert os.environ.get("GPU_MAX_HW_QUEUES") == before


def test_unsupported_geometry_status_codes():
    emb = torch.zeros(1, 129, 4, 4, device=DEV)
    lab = torch.zeros(1, 4, 4, dtype=torch.int32, device=DEV)
    buf = torch.zeros(1 << 16, device=DEV)
    st = torch.zeros((), dtype=torch.int32, device=DEV)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    args = (0.5, 3.0, 1.0, 1.0, 0.001, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), st.data_ptr(), stream)
    assert lib.pct_discriminative_loss_forward_f32(emb.data_ptr(), lab.data_ptr(), 1, 129, 4, 4, 3, *args) == embedding_loss.UNSUPPORTED
    assert lib.pct_discriminative_loss_forward_f32(emb.data_ptr(), lab.data_ptr(), 1, 32, 4, 4, 1025, *args) == embedding_loss.UNSUPPORTED
    assert lib.pct_discriminative_loss_backward_f32(emb.data_ptr(), lab.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 129, 4, 4, 3,
                                                    0.5, buf.data_ptr(), stream) == embedding_loss.UNSUPPORTED
    assert not embedding_loss.supported(emb, 3) and not embedding_loss.supported(emb[:, :32].contiguous(), 1025)
    assert embedding_loss.supported(emb[:, :32].contiguous(), 1024)
    with pytest.raises(RuntimeError):
        embedding_loss.discriminative_loss(emb, lab, 3)


@pytest.mark.parametrize("E,h,w,L", [(33, 19, 17, 5), (64, 19, 17, 33), (80, 19, 17, 5), (96, 16, 16, 3), (128, 32, 32, 6), (128, 19, 17, 33)])
def test_more_than_32_channels_against_float64(E, h, w, L):
    """The channels in tiles of 32 (two tiles at 33 .. 64, four above, the last ones partly or wholly empty at 33, 80 and 96: at
    80 the fourth tile starts past the last channel and must write nothing): 128 is
    the width of the model's own pixel embedding (CONVS_DIM), which the criterion hands to this loss.  Same reference and bounds as
    the narrow cases; 19 x 17 pixels are two passes with a ragged end."""
    name = "near and far centroids"
    emb, lab = R.family(name, E, h, w, L)
    want, wgrad = R.loss64(emb, lab, L, **R.PARAMS)
    lb, gb = R.bounds(emb, lab, L, **R.PARAMS)
    loss, grad, status = _run(emb, lab, L)
    err = abs(float(loss) - want)
    excess = float(((grad.cpu().double() - wgrad).abs() - gb).max())
    print("E=%d %dx%d L=%d: loss %.9g err %.3g bound %.3g; gradient excess over its bound %.3g (largest bound %.3g)"
          % (E, h, w, L, want, err, lb, excess, float(gb.max())))
    assert err <= lb and excess <= 0 and int(status) == 0
    again = _run(emb, lab, L)
    assert torch.equal(loss, again[0]) and torch.equal(grad, again[1])
    outside = (R.clean_labels(lab, L) == 0)[:, None].expand_as(grad)
    assert float(grad.cpu()[outside].abs().max() if outside.any() else 0.0) == 0.0


@pytest.mark.parametrize("E", [40, 80, 128])
def test_guard_bands_of_the_wide_layouts(E):
    """test_guard_bands at 64 and 128 channel slots: the workspace slot is nch + 2 floats and the table row 4 + 2 nch there, and
    at 80 channels the fourth channel tile is empty.  The margins around every output stay as they were."""
    h, w, L, B = 13, 11, 33, 2
    emb, lab = R.family("near and far centroids", E, h, w, L)
    emb, lab = emb.to(DEV), lab.to(DEV)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    fb, ib = -7.25, -77
    ws_buf, ws = _guarded((embedding_loss.workspace_bytes(B, h * w, L, E) // 4,), torch.float32, fb)
    tb_buf, table = _guarded((B, L + 1, embedding_loss.table_row(E)), torch.float32, fb)
    lo_buf, loss = _guarded((), torch.float32, fb)
    st_buf, status = _guarded((), torch.int32, ib)
    gr_buf, grad = _guarded((B, E, h, w), torch.float32, fb)
    assert ws.data_ptr() % 16 == 0 and embedding_loss.table_row(E) == 4 + 2 * (64 if E <= 64 else 128)
    rc = lib.pct_discriminative_loss_forward_f32(emb.data_ptr(), lab.data_ptr(), B, E, h, w, L, 0.5, 3.0, 1.0, 1.0, 0.001,
                                                 ws.data_ptr(), table.data_ptr(), loss.data_ptr(), status.data_ptr(), stream)
    assert rc == 0
    go = torch.ones((), device=DEV)
    rc = lib.pct_discriminative_loss_backward_f32(emb.data_ptr(), lab.data_ptr(), table.data_ptr(), go.data_ptr(), B, E, h, w, L,
                                                  0.5, grad.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, fill in ((ws_buf, fb), (tb_buf, fb), (lo_buf, fb), (st_buf, ib), (gr_buf, fb)):
        assert _margins_untouched(buf, fill)
    want = _run(emb.cpu(), lab.cpu(), L)
    assert torch.equal(loss, want[0]) and torch.equal(grad, want[1]) and int(status) == 0
    assert not bool((table == fb).any())                                   # the table is fully overwritten


def test_set_criterion_copies_a_channels_last_embedding(monkeypatch):
    """The pixel decoder hands its 128-channel map over channels-last: dense, not contiguous.  With emb_loss = "hip" the
    criterion copies it, the kernels get [B, E, h, w] planes, and the gradient comes back through the copy to the map itself."""
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(2, 128, 13, 18, generator=g)
    targets = _targets([(50, 70)] * 2, (7, 40))
    labels = R.label_map_reference([t["masks"] for t in targets], (13, 18)).cpu()
    want, wgrad = R.loss64(emb, labels, 40)
    lb, gb = R.bounds(emb, labels, 40)
    calls = []
    real = embedding_loss.discriminative_loss
    monkeypatch.setattr(embedding_loss, "discriminative_loss",
                        lambda *a, **k: calls.append((a[2], a[0].is_contiguous())) or real(*a, **k))
    x = emb.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert not x.is_contiguous() and x.is_leaf
    loss = _criterion("hip").loss_embedding(x, targets)["loss_emb"]
    loss.backward()
    assert calls == [(40, True)]                                           # the device path ran, on a contiguous copy
    assert abs(float(loss) - want) <= lb
    assert x.grad is not None and x.grad.shape == x.shape
    assert float(((x.grad.cpu().double() - wgrad).abs() - gb).max()) <= 0
    assert int(loss.status) == 0


def test_the_largest_covered_label_count():
    """L = 1024 and E = 32: 33 label tiles, 32 blocks of the pairwise pass."""
    g = torch.Generator().manual_seed(12)
    emb = torch.randn(1, 32, 40, 40, generator=g)
    lab = torch.randint(0, 1025, (1, 40, 40), generator=g).to(torch.int32)
    lab[0, 0, 0] = 1024
    want, wgrad = R.loss64(emb, lab, 1024)
    lb, gb = R.bounds(emb, lab, 1024)
    loss, grad, status = _run(emb, lab, 1024)
    assert abs(float(loss) - want) <= lb and float(((grad.cpu().double() - wgrad).abs() - gb).max()) <= 0 and int(status) == 0

"""The single-head point-loss functions (pctrans_amd/point_loss.py: select_uncertain_points, point_mask_loss_forward,
point_mask_losses, match_costs) bit for bit: SHA-256 digests of their outputs on CPU-seeded inputs, recorded on an MI355X while
each of them still had a kernel and a launcher of its own.  The selection and the loss forward are now the one-head case of
the kernels with a head dimension (csrc/point_loss.hip: *_many_kernel; csrc/c_abi.hip).  Every bit must be as before.

Shapes, those of test_loss_heads_gpu.py: predictions [2, 5, 33, 20], targets [7, 41, 27], 6 pairs, one pair naming a plane past
the end (its NaN row and its index -1 are part of the digest); 144 candidates keeping 36 into rows with 3 sentinel points behind,
16 385 and 40 961 candidates on 2 pairs (the other two kernel classes), each with and without src_index and with and without
the index output; the loss forward at P = 48 and P = 1030; both loss scalars and the gradient for incoming gradients (1, 1) and
(0.3, 2.0) on [2, 5, 33, 20] and on [2, 5, 40, 256] (two bands of the backward), and once with 120 pairs on [2, 75, 33, 20]
(the scalars as sums of as many terms as a training step has); costs for 2 images with 3 and 65 targets, Q = 5 and 130,
P = 200, and once with the second image's planes starting 10 late (NaN columns).

`python tests/test_point_one_head_bits_gpu.py` prints the table of digests."""
import hashlib

import pytest
import torch

DEV = "cuda"
NPLANES, H, W = 10, 33, 20
NTGT, HT, WT = 7, 41, 27
K = 6
SENTINEL = -7.25

SELECT_CASES = [(S, keep, pairs, extra, with_src, with_index)
                for S, keep, pairs, extra in ((144, 36, K, 3), (16385, 16385 // 4, 2, 1), (40961, 40961 // 4, 2, 1))
                for with_src in (True, False) for with_index in (True, False)]
FORWARD_CASES = [48, 1030]
LOSS_CASES = [(shape, g) for shape in ((2, 5, H, W), (2, 5, 40, 256)) for g in ((1.0, 1.0), (0.3, 2.0))]
LOSS_CASES.append(((2, 75, H, W), (0.3, 2.0)))                # 120 pairs: the loss scalars are 120-term sums
COST_CASES = [(Q, late) for Q in (5, 130) for late in (False, True)]

DIGESTS = {
    "costs_Q130_inplace": "0b554935a20b9ed652c42c830185100644abb7b5b80608f4bf717235f5593eda",
    "costs_Q130_late": "27ebe9c63a0e836a5442ca109694fa25435cf00cb096b7bde46417f8cb570a12",
    "costs_Q5_inplace": "3cb4163c2558e960eb7541a40b8638fa4595cfcbd7252b034bf58c8d26a1e711",
    "costs_Q5_late": "a3279f6b23cf0ec05d3f64bcf63a0481b4ca3fc859894b896e87941772757d95",
    "forward_P1030": "79a1d2d6e68254568b3d2db608fb04ea3f2d813bebf8399e3f5b13d5d3771204",
    "forward_P48": "1ed8a9af332a704db1766ab62bf5f630d9cd79c52551287b6f5e1b75b7de7c5b",
    "losses_33x20_g0.3_2": "4222d43e9185b89035e1ff749e726357101bad832b89d7d183704f6524e0561c",
    "losses_33x20_g1_1": "4a492c06057b1d4f6a3d521b21a528f21a0c690c3000a64f10798bf129c57bff",
    "losses_40x256_g0.3_2": "279c2676f500ef52decef1f6f0c312540444102bf3304bc696cf12950abe35df",
    "losses_40x256_g1_1": "d65401a695db7ce0b2a777c42db40094c17d36b51d5bc33d73562838fa26a975",
    "losses_q75_33x20_g0.3_2": "7a624ca24f691f6f7e7012fa5dd3593e30932b9468e3f6a1fa68c0af5b369231",
    "select_S144_identity_index": "747cd83ed21b68367508040fa194a9effa0d06ebc5a53fb08cb5ff0d4579c92c",
    "select_S144_identity_noindex": "6c6febce72258b43fec955b5b3f47bd655cf7d3a237fed99c133baec4f956898",
    "select_S144_src_index": "86a145552882a52256f2d5422425f7bff816e5e1fcf4c3e970e79b7a5f2ccaaf",
    "select_S144_src_noindex": "140bd7daec9c99b40bc38399d14ade5ace446a571588fd765e2d92bd186382c3",
    "select_S16385_identity_index": "3b2cfe069c43e2b34fb1989e95eed4c92f84f6110e7761fe82f7f755bab82467",
    "select_S16385_identity_noindex": "1a35dc8e92a6c8e593779e4c47cb79abac98c1ececc82d30b6176e3845a3d849",
    "select_S16385_src_index": "7fa8afebaac86f0f0e476056add231157f78b58dd708cd7eefc284f62faa5305",
    "select_S16385_src_noindex": "b45ce0973e53b49319de2c33bb8a63f8c22ba1753f6cfaf4aec5d1960ae27d03",
    "select_S40961_identity_index": "b80b0cb0eb10202cdee550c79389a4d172ea68bab4d78f5522c6725477f609b0",
    "select_S40961_identity_noindex": "620a5af22a04fc02db6cbc8f364e30e7e9e06f2baac460b7d7c8187c3763f9a3",
    "select_S40961_src_index": "650d5d1678380340df642f811d30dd121c10388c6ee010ed676abbb1ce958fad",
    "select_S40961_src_noindex": "bf76a1491e4b93faeecc16fdba0f294238ec97bc83809ee87000f4146e8c2f83",
}


def _sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().reshape(-1).cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _data():
    """One head of test_loss_heads_gpu.py's kind: predictions, targets, an index permutation whose pair 2 names plane 10 of 10."""
    g = torch.Generator().manual_seed(131)
    pred = (torch.randn(2, 5, H, W, generator=g) * 3).to(DEV)
    tgt = (torch.rand(NTGT, HT, WT, generator=g) > 0.5).float().to(DEV)
    src = torch.randperm(NPLANES, generator=g)[:K].int()
    tix = torch.randperm(NTGT, generator=g)[:K].int()
    src_bad = src.clone()
    src_bad[2] = NPLANES
    return pred, tgt, src.to(DEV), src_bad.to(DEV), tix.to(DEV)


# ---- selection --------------------------------------------------------------------------------------------------------------
def select_name(S, keep, pairs, extra, with_src, with_index):
    return "select_S%d_%s_%s" % (S, "src" if with_src else "identity", "index" if with_index else "noindex")


def run_select(S, keep, pairs, extra, with_src, with_index):
    """-> (out [pairs, keep + extra, 2] with its sentinel tail, index or None, the index vector used or None)."""
    from pctrans_amd import point_loss
    pred, _, src, src_bad, _ = _data()
    g = torch.Generator().manual_seed(S + (1 if with_src else 0))
    cand = torch.rand(pairs, S, 2, generator=g).to(DEV)
    idx = (src_bad if pairs == K else src)[:pairs].contiguous() if with_src else None
    out = torch.full((pairs, keep + extra, 2), SENTINEL, device=DEV)
    got, index = point_loss.select_uncertain_points(pred, idx, cand, keep, out=out, with_index=with_index)
    assert got is out
    return out, index, idx


def select_digest(*case):
    out, index, _ = run_select(*case)
    return _sha(out, *([] if index is None else [index]))


@pytest.mark.gpu
@pytest.mark.parametrize("S,keep,pairs,extra,with_src,with_index", SELECT_CASES)
def test_selection_bits_and_the_rows_tails(S, keep, pairs, extra, with_src, with_index):
    out, index, idx = run_select(S, keep, pairs, extra, with_src, with_index)
    assert bool((out[:, keep:] == SENTINEL).all()), "the selection wrote behind the points it keeps"
    assert (index is None) == (not with_index)
    bad = with_src and pairs == K                                               # pair 2 names a plane past the end
    nan_rows = out[:, :keep].isnan().all(-1).all(-1)
    assert nan_rows.tolist() == [bad and k == 2 for k in range(pairs)] and not bool(out[~nan_rows].isnan().any())
    if with_index:
        assert index.shape == (pairs, keep) and index.dtype == torch.int32
        assert ((index == -1).all(-1)).tolist() == nan_rows.tolist() and bool((index[~nan_rows] >= 0).all())
    assert _sha(out, *([] if index is None else [index])) == DIGESTS[select_name(S, keep, pairs, extra, with_src, with_index)]


# ---- loss forward -----------------------------------------------------------------------------------------------------------
def run_forward(P):
    from pctrans_amd import point_loss
    pred, tgt, _, src_bad, tix = _data()
    coords = torch.rand(K, P, 2, generator=torch.Generator().manual_seed(100 + P)).to(DEV)
    return point_loss.point_mask_loss_forward(pred, src_bad, tgt, tix, coords), (pred, tgt, src_bad, tix, coords)


def forward_digest(P):
    return _sha(*run_forward(P)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("P", FORWARD_CASES)
def test_loss_forward_bits(P):
    (x, t, sums), _ = run_forward(P)
    assert x.shape == (K, P) and t.shape == (K, P) and sums.shape == (K, 4)
    nan_rows = x.isnan().all(-1) & t.isnan().all(-1) & sums.isnan().all(-1)
    assert nan_rows.tolist() == [k == 2 for k in range(K)] and int(x.isnan().any(-1).sum()) == 1
    assert _sha(x, t, sums) == DIGESTS["forward_P%d" % P]


# ---- losses and gradient ----------------------------------------------------------------------------------------------------
def loss_name(shape, g):
    return "losses_%s%dx%d_g%g_%g" % ("" if shape[1] == 5 else "q%d_" % shape[1], shape[2], shape[3], g[0], g[1])


def run_losses(shape, g):
    """-> (loss_mask, loss_dice, gradient of g[0] * loss_mask + g[1] * loss_dice)."""
    from pctrans_amd import point_loss
    gen = torch.Generator().manual_seed(41 + shape[3])
    pred = (torch.randn(*shape, generator=gen) * 3).to(DEV).requires_grad_(True)
    tgt = (torch.rand(NTGT, HT, WT, generator=gen) > 0.5).float().to(DEV)
    pairs = K if shape[1] == 5 else 120
    src = torch.randperm(shape[0] * shape[1], generator=gen)[:pairs].to(DEV)
    tix = (torch.randperm(NTGT, generator=gen)[:K] if pairs == K else torch.randint(0, NTGT, (pairs,), generator=gen)).to(DEV)
    coords = torch.rand(pairs, 48, 2, generator=gen).to(DEV)
    lm, ld = point_loss.point_mask_losses(pred, src, tgt, tix, coords, 6.0)
    (g[0] * lm + g[1] * ld).backward()
    return lm.detach(), ld.detach(), pred.grad, src


def losses_digest(shape, g):
    return _sha(*run_losses(shape, g)[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,g", LOSS_CASES)
def test_losses_and_gradient_bits(shape, g):
    lm, ld, grad, src = run_losses(shape, g)
    assert lm.shape == () and ld.shape == () and float(lm) > 0 and float(ld) > 0
    assert grad.shape == shape and grad.dtype == torch.float32
    touched = grad.flatten(0, 1).abs().sum((1, 2)) > 0
    assert sorted(touched.nonzero().flatten().tolist()) == sorted(src.tolist())         # the matched planes, and only they
    assert _sha(lm, ld, grad) == DIGESTS[loss_name(shape, g)]


# ---- costs ------------------------------------------------------------------------------------------------------------------
def run_costs(Q, late):
    from pctrans_amd import point_loss
    counts, P = [3, 65], 200
    g = torch.Generator().manual_seed(1000 + Q)
    pred = (torch.randn(2, Q, 7, 9, generator=g) * 3).to(DEV)
    tgt = (torch.rand(sum(counts), 14, 18, generator=g) > 0.5).float().to(DEV)
    coords = torch.rand(2, P, 2, generator=g).to(DEV)
    starts = torch.tensor([0, 13] if late else [0, 3], dtype=torch.int32, device=DEV)
    return point_loss.match_costs(pred, tgt, starts, torch.tensor(counts, dtype=torch.int32, device=DEV), coords, 5.0, 2.0, 65)


def costs_digest(Q, late):
    return _sha(run_costs(Q, late))


@pytest.mark.gpu
@pytest.mark.parametrize("Q,late", COST_CASES)
def test_cost_bits(Q, late):
    cost = run_costs(Q, late)
    assert cost.shape == (2, Q, 65)
    assert bool((cost[0, :, 3:] == 0).all()) and bool(cost[0, :, :3].isfinite().all())  # exactly zero past the count
    if late:                                                                            # planes 68 .. 77 do not exist
        assert bool(cost[1, :, 55:].isnan().all()) and bool(cost[1, :, :55].isfinite().all())
    else:
        assert bool(cost.isfinite().all()) and bool((cost[1] != 0).all())
    assert _sha(cost) == DIGESTS["costs_Q%d_%s" % (Q, "late" if late else "inplace")]


# ---- the C entries themselves -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_single_head_c_entries_write_the_functions_bits():
    """pct_point_select_uncertain_f32, pct_point_mask_loss_forward_f32 and pct_point_match_cost_f32 called directly: the bits of
    the Python functions above, whichever entry those reach."""
    from pctrans_amd import _lib, point_loss
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    pred, tgt, _, src_bad, tix = _data()
    # selection
    want, want_index, _ = run_select(144, 36, K, 3, True, True)
    cand = torch.rand(K, 144, 2, generator=torch.Generator().manual_seed(145)).to(DEV)
    out = torch.full((K, 39, 2), SENTINEL, device=DEV)
    index = torch.full((K, 36), -5, dtype=torch.int32, device=DEV)
    rc = L.pct_point_select_uncertain_f32(pred.data_ptr(), src_bad.data_ptr(), NPLANES, H, W, cand.data_ptr(), K, 144, 36,
                                          out.data_ptr(), 39, index.data_ptr(), stream)
    assert rc == 0 and _sha(out, index) == _sha(want, want_index)
    # loss forward
    (wx, wt, ws), (_, _, _, _, coords) = run_forward(1030)
    x, t = torch.empty(K, 1030, device=DEV), torch.empty(K, 1030, device=DEV)
    sums = torch.empty(K, 4, device=DEV)
    rc = L.pct_point_mask_loss_forward_f32(pred.data_ptr(), src_bad.data_ptr(), NPLANES, H, W, tgt.data_ptr(), tix.data_ptr(), NTGT,
                                           HT, WT, coords.data_ptr(), K, 1030, x.data_ptr(), t.data_ptr(), sums.data_ptr(), stream)
    assert rc == 0 and _sha(x, t, sums) == _sha(wx, wt, ws)
    # costs
    want = run_costs(130, True)
    g = torch.Generator().manual_seed(1130)
    cpred = (torch.randn(2, 130, 7, 9, generator=g) * 3).to(DEV)
    ctgt = (torch.rand(68, 14, 18, generator=g) > 0.5).float().to(DEV)
    ccoords = torch.rand(2, 200, 2, generator=g).to(DEV)
    starts = torch.tensor([0, 13], dtype=torch.int32, device=DEV)
    counts = torch.tensor([3, 65], dtype=torch.int32, device=DEV)
    cost = torch.empty(2, 130, 65, device=DEV)
    wsp = torch.empty(point_loss.match_cost_workspace_bytes(2, 130, 65, 200) // 4, device=DEV)
    rc = L.pct_point_match_cost_f32(cpred.data_ptr(), 2, 130, 7, 9, ctgt.data_ptr(), 68, 14, 18, starts.data_ptr(), counts.data_ptr(),
                                    65, ccoords.data_ptr(), 200, 5.0, 2.0, wsp.data_ptr(), cost.data_ptr(), stream)
    assert rc == 0 and _sha(cost) == _sha(want)


def all_digests():
    d = {select_name(*c): select_digest(*c) for c in SELECT_CASES}
    d.update({"forward_P%d" % P: forward_digest(P) for P in FORWARD_CASES})
    d.update({loss_name(*c): losses_digest(*c) for c in LOSS_CASES})
    d.update({"costs_Q%d_%s" % (Q, "late" if late else "inplace"): costs_digest(Q, late) for Q, late in COST_CASES})
    return d


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name, digest in sorted(all_digests().items()):
        print('    "%s": "%s",' % (name, digest))

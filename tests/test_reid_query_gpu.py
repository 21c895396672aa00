"""GPU: the re-id query kernels (pct_reid_nearest_positive_f32, pct_reid_query_rows_forward_f32,
pct_reid_query_rows_backward_f32, pct_contrast_loss_rows_f32 through pctrans_amd/reid_query.py) against the float64 reference of
reid_query_reference.py inside the bounds stated there, exact ties, images without items, the item without negatives,
bit-identical repeats, the fallback on inputs the kernels do not cover, and a whole decoder step with reid_query, reid_dice and
contrast_loss all "hip" beside the torch chain and a float64 copy."""
import contextlib
import copy
import functools
import random

import pytest
import torch

import reid_query_reference as R

pytestmark = pytest.mark.gpu

SHAPE_IDS = list(range(len(R.SHAPES)))


def _rows_run(query, image_start, key, gS, gC):
    """-> (S, Cs, norm, dL/dquery) of the device path on CPU inputs."""
    from pctrans_amd import reid_query
    x = query.cuda().requires_grad_(True)
    S, Cs = reid_query.query_rows(x, image_start.cuda(), key.tolist())
    grad, = torch.autograd.grad([S, Cs], x, [gS.cuda(), gC.cuda()])
    _, _, norm = reid_query.query_rows_forward(x.detach(), image_start.cuda(), key.cuda())
    return S.detach().cpu(), Cs.detach().cpu(), norm.cpu(), grad.cpu()


@functools.lru_cache(maxsize=None)
def _device_rows(shape):
    e = R.expected(shape)
    return _rows_run(e["query"], e["image_start"], e["key"], e["gS"], e["gC"])


def _check_nearest(query, pos_lists, got, exact):
    """The rule of reid_query_reference.py for every unmatched row.  exact: every gap must exceed the bound (no row left out)."""
    cos, (want, gap) = R.cos64(query, pos_lists), R.nearest64(query, pos_lists)
    Q = query.shape[0]
    decided = 0
    for n, pl in enumerate(pos_lists):
        if not pl:
            assert got[n] == [-1] * Q
            continue
        for r in range(Q):
            assert 0 <= got[n][r] < len(pl)
            if r in pl:
                continue
            assert float(cos[n][r].max() - cos[n][r, got[n][r]]) <= R.GAP, (n, r)
            if float(gap[n][r]) > R.GAP:
                assert got[n][r] == want[n][r], (n, r)
                decided += 1
            else:
                assert not exact, (n, r, float(gap[n][r]))
    return decided


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_nearest_positive_is_the_float64_first_argmax(shape):
    from pctrans_amd import reid_query
    e = R.expected(shape)
    got = reid_query.nearest_positive(e["query"].cuda(), e["pos_lists"])
    assert len(got) == R.SHAPES[shape][0] and all(len(g) == R.SHAPES[shape][1] for g in got)
    decided = _check_nearest(e["query"], e["pos_lists"], got, exact=shape == 0)
    print("shape %d: %d unmatched rows decided by a gap above %.2e" % (shape, decided, R.GAP))
    assert decided > 0
    assert got == reid_query.nearest_positive(e["query"].cuda(), e["pos_lists"])
    if shape == 0:
        assert got[1] == [-1] * R.SHAPES[0][1]                             # the image without positives


def test_equal_positive_rows_the_earlier_position_wins():
    from pctrans_amd import reid_query
    e = R.expected(1)
    query, pos_lists = e["query"].clone(), e["pos_lists"]
    first, second = 2, 7                                                   # positions in image 0's list
    query[pos_lists[0][second], 0] = query[pos_lists[0][first], 0]
    got = reid_query.nearest_positive(query.cuda(), pos_lists)
    want, _ = R.nearest64(query, pos_lists)
    assert second not in got[0]
    hit = [r for r in range(query.shape[0]) if want[0][r] in (first, second) and r not in pos_lists[0]]
    assert len(hit) > 0 and all(got[0][r] == first for r in hit)
    _check_nearest(query, pos_lists, got, exact=False)


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_rows_inside_the_bounds(shape):
    e = R.expected(shape)
    S, Cs, norm, _ = _device_rows(shape)
    L, u = R.CHAIN_LENGTH, R.U
    serr, cerr = (S.double() - e["S"]).abs(), (Cs.double() - e["Cs"]).abs()
    nerr = (norm.double() - e["norm"]).abs() / e["norm"]
    print("shape %d: S err/bound %.3f  Cs err/bound %.3f  norm rel err / u %.2f" % (
        shape, float((serr / (L * u * e["S_abs"])).max()), float(cerr.max() / R.COS_BOUND), float(nerr.max() / u)))
    assert S.shape == e["S"].shape and Cs.shape == e["Cs"].shape and norm.shape == e["norm"].shape
    assert bool((serr <= L * u * e["S_abs"]).all())
    assert bool((cerr <= R.COS_BOUND).all())
    assert bool((nerr <= (L / 2 + 2) * u).all())
    i = torch.arange(S.shape[0])
    assert float((Cs[i, e["key"].long()] - 1).abs().max()) <= R.COS_BOUND      # the diagonal is included
    assert bool((S[i, e["key"].long()] > 0).all())


def _check_backward(query, image_start, key, gS, gC, counts):
    S, Cs, norm, grad = _rows_run(query, image_start, key, gS, gC)
    g64, g_abs, T = R.grad64(query, image_start, key, gS, gC, norm, Cs)
    bound = (T[:, :, None] + 8) * R.U * g_abs
    err = (grad.double() - g64).abs()
    print("backward: err/bound %.3f (max |g| %.3e, T up to %d)" % (float((err / bound.clamp(min=1e-300)).max()),
                                                                   float(g64.abs().max()), int(T.max())))
    assert grad.shape == query.shape and bool(torch.isfinite(grad).all())
    assert bool((err <= bound).all())
    for n, c in enumerate(counts):
        if c == 0:
            assert int((grad[:, n] != 0).sum()) == 0                       # an image without items: exact zeros
        else:
            assert int((grad[:, n] != 0).sum()) > 0
    return grad


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_backward_inside_the_bounds(shape):
    e = R.expected(shape)
    counts = (e["image_start"][1:] - e["image_start"][:-1]).tolist()
    for gS, gC in ((e["gS"], e["gC"]), (e["gS"], torch.zeros_like(e["gC"])), (torch.zeros_like(e["gS"]), e["gC"])):
        _check_backward(e["query"], e["image_start"], e["key"], gS, gC, counts)


def test_backward_with_a_clamped_norm_and_a_repeated_key():
    e = R.expected(0)
    counts = (e["image_start"][1:] - e["image_start"][:-1]).tolist()
    query = e["query"].clone()
    row = min(r for r in range(query.shape[0]) if r not in e["pos_lists"][0])          # an unmatched query of image 0
    query[row, 0] = 1e-20                                                  # |x| < 1e-12: the norm is the clamp, a constant
    key = e["key"].clone()
    key[1] = key[0]                                                        # image 0: two items share a key
    _check_backward(query, e["image_start"], key, e["gS"], e["gC"], counts)


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_contrast_loss_inside_the_bounds(shape):
    from pctrans_amd import reid_query
    e = R.expected(shape)
    Q = R.SHAPES[shape][1]
    factor = (2 * Q + 32) * R.U
    for temperature, rows in ((2.0, e["S"].float()), (0.5, e["Cs"].float()), (2.0, 80 * torch.sign(e["gS"])),
                              (0.5, 80 * torch.sign(e["gC"]))):
        r = rows.cuda().requires_grad_(True)
        loss = reid_query.contrast_loss_rows(r, e["image_of"].cuda(), e["key"].cuda(), e["owner"].cuda(), temperature)
        _, coef = reid_query.contrast_loss_rows_forward(r.detach(), e["image_of"].cuda(), e["key"].cuda(), e["owner"].cuda(),
                                                        temperature)
        w = torch.linspace(0.5, 1.5, loss.shape[0]).cuda()
        grad, = torch.autograd.grad(loss, r, w)
        assert torch.equal(grad, w[:, None] * coef)                        # the backward is grad_loss[:, None] * coef
        loss64, coef64 = R.contrast64(rows, e["image_of"], e["key"], e["owner"], 1.0 / temperature)
        lerr = (loss.detach().cpu().double() - loss64).abs() / (1 + loss64.abs())
        cerr = (coef.cpu().double() - coef64).abs() * temperature
        print("shape %d T=%.1f max|rows| %.0f: loss err/bound %.3f  coef err/bound %.3f  (max loss %.3f)" % (
            shape, temperature, float(rows.abs().max()), float(lerr.max() / factor), float(cerr.max() / factor),
            float(loss64.max())))
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(coef).all())
        assert bool((lerr <= factor).all()) and bool((cerr <= factor).all())
        assert int((coef.cpu()[torch.arange(loss.shape[0]), e["key"].long()] != 0).sum()) == 0
        if shape == 0:                                                     # the single-instance image: no negatives
            assert e["plan"][-1][3] == [] and float(loss.detach()[-1]) == 0.0 and int((coef[-1] != 0).sum()) == 0
            assert float(loss.detach()[0]) > 0


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_two_calls_give_the_same_bits(shape):
    from pctrans_amd import reid_query
    e = R.expected(shape)
    first = _device_rows(shape)
    again = _rows_run(e["query"], e["image_start"], e["key"], e["gS"], e["gC"])
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    args = (e["S"].float().cuda(), e["image_of"].cuda(), e["key"].cuda(), e["owner"].cuda(), 2.0)
    a, b = reid_query.contrast_loss_rows_forward(*args), reid_query.contrast_loss_rows_forward(*args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_keys_outside_the_queries_raise_on_the_host():
    from pctrans_amd import reid_query
    e = R.expected(0)
    x = e["query"].cuda()
    for bad in (-1, R.SHAPES[0][1]):
        key = e["key"].tolist()
        key[0] = bad
        with pytest.raises(RuntimeError, match="keys must lie"):
            reid_query.query_rows(x, e["image_start"], key)
    with pytest.raises(RuntimeError, match="matched queries must lie"):
        reid_query.nearest_positive(x, [[0, R.SHAPES[0][1]], [], [1]])


def _items_equal(a, b):
    assert len(a) == len(b) > 0 and a.batched.keys() == b.batched.keys()
    for k in b.batched:
        assert torch.equal(a.batched[k], b.batched[k]), k


def test_inputs_the_kernels_do_not_cover_keep_the_torch_chain(monkeypatch):
    """bf16, C = 514, Q = 1025 and a non-contiguous query: the items are those of the switch being off, bit for bit, and no
    wrapper is entered."""
    from pctrans_amd import reid_query
    from pctrans_amd.transformer_decoder import query_contrast as qc
    assert reid_query.supported(torch.zeros(1024, 1, 512, device="cuda"), (3,))
    assert not reid_query.supported(torch.zeros(1025, 1, 8, device="cuda"), (3,))
    assert not reid_query.supported(torch.zeros(8, 1, 516, device="cuda"), (3,))
    assert not reid_query.supported(torch.zeros(8, 1, 514, device="cuda"), (3,))
    assert not reid_query.supported(torch.zeros(8, 1, 8, device="cuda"), (9,))
    assert not reid_query.supported(torch.zeros(8, 1, 8, device="cuda", dtype=torch.bfloat16), (3,))
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError())
    for name in ("nearest_positive", "query_rows"):
        monkeypatch.setattr(reid_query, name, boom)
    gen = torch.Generator().manual_seed(9)
    cases = {"bf16": torch.randn(20, 2, 16, generator=gen).to(torch.bfloat16),
             "C = 514": torch.randn(20, 2, 514, generator=gen),
             "Q = 1025": torch.randn(1025, 1, 8, generator=gen),
             "non-contiguous": torch.randn(2, 20, 16, generator=gen).transpose(0, 1)}
    for name, query in cases.items():
        query = query.cuda()
        Q, N = query.shape[:2]
        assert name != "non-contiguous" or not query.is_contiguous()
        masks = torch.randn(N, Q, 4, 4, generator=gen).cuda()
        pos = [(torch.tensor([5, 17, 2]), torch.tensor([0, 1, 2])) for _ in range(N)]
        random.seed(1)
        off = qc.query_contrast_items(query, masks, pos)
        random.seed(1)
        on = qc.query_contrast_items(query, masks, pos, reid_query="hip")
        _items_equal(on[0], off[0])
        _items_equal(on[1], off[1])
        assert "rows" not in on[0].batched


# ---- the whole decoder ------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


class _RecordedMatcher:
    """Hands out the assignments a run of the real matcher gave, one prediction after the other."""

    def __init__(self, indices_list):
        self.indices_list, self.at = indices_list, 0

    def __call__(self, outputs, targets):
        got = self.indices_list[self.at % len(self.indices_list)]
        self.at += 1
        return got


def _decoder_step(d, crit, feats, mf, targets, mode, f64=False):
    """One training forward of the decoder with targets and the backward of the three re-id losses.  -> a record of the losses,
    the gradients at the decoder's parameters, the plan, the queries and assignments, and how often the spied functions ran."""
    from pctrans_amd import reid_dice, reid_query
    from pctrans_amd.loss import maskformer_criterion as crit_mod
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    from pctrans_amd.transformer_decoder import query_contrast as qc
    d.reid_query = d.reid_dice = crit.contrast_loss = mode
    d.zero_grad(set_to_none=True)
    rec = {"calls": {}}
    real = {"items": qc.query_contrast_items, "float": torch.Tensor.float, "sine": dec.gen_sineembed_for_position}

    def counted(mod, name):
        inner, tag = getattr(mod, name), "%s.%s" % (mod.__name__.rsplit(".", 1)[-1], name)
        rec["calls"][tag] = 0

        def wrapper(*a, **k):
            rec["calls"][tag] += 1
            return inner(*a, **k)
        return _patched(mod, name, wrapper)

    def items(output, outputs_mask, indices, **k):
        got = real["items"](output, outputs_mask, indices, **k)
        rec["query"], rec["indices"], rec["switches"] = output.detach().clone(), indices, k
        rec["aux"] = {n: got[0].batched[n].detach().double().cpu() for n in ("aux_label", "aux_count", "aux_rows", "n_pos")}
        rec["keys"] = (sorted(got[0].batched), sorted(got[1].batched))
        return got

    def plan_spy(name):
        inner = getattr(qc, name)

        def wrapper(*a, **k):
            rec.setdefault("plans", []).append(copy.deepcopy(list(k["_plan_cache"])))
            return inner(*a, **k)
        return _patched(qc, name, wrapper)

    with contextlib.ExitStack() as stack:
        for mod, name in ((reid_query, "nearest_positive"), (reid_query, "query_rows_forward"), (reid_query, "query_rows_backward"),
                          (reid_query, "contrast_loss_rows_forward"), (reid_dice, "dice_rows_forward"),
                          (torch.nn.functional, "cosine_similarity"), (crit_mod, "_contrast_softplus")):
            stack.enter_context(counted(mod, name))
        stack.enter_context(_patched(qc, "query_contrast_items", items))
        stack.enter_context(plan_spy("select_pos_neg_query"))
        stack.enter_context(plan_spy("select_pos_neg_mask"))
        if f64:                                  # nothing of the arbiter is rounded to fp32 (tests/test_train_step_all_on_gpu.py)
            stack.enter_context(_patched(torch.Tensor, "float", lambda t, *a, **k: t if t.dtype == torch.float64
                                         else real["float"](t, *a, **k)))
            stack.enter_context(_patched(dec, "gen_sineembed_for_position", lambda p, *a, **k: real["sine"](p, *a, **k).to(p.dtype)))
        torch.manual_seed(11)
        random.seed(11)
        out = d(feats, targets, mf, criterion=crit)
        losses = {**crit.loss_reid_query(out, targets, None, 1.0), **crit.loss_reid_mask(out, targets, None, 1.0)}
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    rec["random"] = random.getstate()
    rec["losses"] = {k: v.detach().double().cpu() for k, v in losses.items()}
    rec["grads"] = {n: p.grad.detach().double().cpu() for n, p in d.named_parameters() if p.grad is not None}
    rec["indices_list"] = out["indices_list"]
    return rec


def _bound(name, on, off, f64, fails, zero_rule=False):
    """|on - off| <= max(2 |off - f64|, 5e-6 max|f64|): the rule of tests/test_train_step_all_on_gpu.py (a bias whose gradient is
    zero in exact arithmetic: 4 |off - f64|)."""
    err, yerr, top = float((on - off).abs().max()), float((off - f64).abs().max()), float(f64.abs().max())
    assert bool(torch.isfinite(on).all()) and bool(torch.isfinite(off).all()) and bool(torch.isfinite(f64).all()), name
    bound = 4.0 * yerr if zero_rule else max(2.0 * yerr, 5e-6 * top)
    print("%-60s |on - off| %.3e  |off - f64| %.3e  max|f64| %.3e  bound %.3e" % (name, err, yerr, top, bound))
    if err > bound:
        fails.append("%s: |on - off| %.3e > %.3e (|off - f64| %.3e, max|f64| %.3e)" % (name, err, bound, yerr, top))


def test_decoder_step_with_all_three_switches_on():
    from pctrans_amd.loss import maskformer_criterion as crit_mod
    from pctrans_amd.loss.matcher import Point_HungarianMatcher
    from pctrans_amd.transformer_decoder import mask2former_transformer_decoder as dec
    from pctrans_amd.transformer_decoder.position_encoding import PositionEmbeddingSine
    torch.manual_seed(2)
    Q = 12
    d = dec.MultiScaleMaskedTransformerDecoder(
        128, True, hidden_dim=128, num_queries=Q, nheads=8, dim_feedforward=256, dec_layers=2, pre_norm=False,
        mask_dim=16, enforce_input_project=False, points_num=1, sem_loss_on=False, norm="BN", rel_coord=True).cuda().train()
    make_crit = lambda matcher: crit_mod.SetCriterion(1, matcher, {}, 0.1, ["reid_query", "reid_mask"], 64, 3.0, 0.75)
    crit = make_crit(Point_HungarianMatcher(num_points=64))
    g = torch.Generator().manual_seed(4)
    mf = torch.randn(2, 128, 32, 32, generator=g).cuda()
    feats = [torch.randn(2, 128, s, s, generator=g).cuda() for s in (4, 8, 16)]
    targets = [{"masks": (torch.rand(3, 64, 64, generator=g) > 0.5).float().cuda(),
                "labels": torch.zeros(3, dtype=torch.long, device="cuda")} for _ in range(2)]
    d.reid_query = "triton"
    with pytest.raises(ValueError):
        d(feats, targets, mf, criterion=crit)
    off = _decoder_step(d, crit, feats, mf, targets, "torch")
    on = _decoder_step(d, crit, feats, mf, targets, "hip")
    d64 = copy.deepcopy(d).double()
    for m in d64.modules():
        if isinstance(m, PositionEmbeddingSine):
            m.register_forward_hook(lambda mod, i, o: o.double())
    f64 = _decoder_step(d64, make_crit(_RecordedMatcher(off["indices_list"])), [f.double() for f in feats], mf.double(),
                        [dict(t, masks=t["masks"].double()) for t in targets], "torch", f64=True)

    # the switches reached the call site, the wrappers ran, the torch formulations did not
    assert on["switches"] == {"mask_dice": "hip", "reid_query": "hip"} and off["switches"] == {"mask_dice": "torch", "reid_query": "torch"}
    c = on["calls"]
    assert c["reid_query.nearest_positive"] == 1 and c["reid_query.query_rows_forward"] == 1 == c["reid_query.query_rows_backward"]
    assert c["reid_query.contrast_loss_rows_forward"] == 2 and c["reid_dice.dice_rows_forward"] == 1
    assert c["functional.cosine_similarity"] == 0 == c["maskformer_criterion._contrast_softplus"]
    assert all(k in on["keys"][0] and k in on["keys"][1] for k in ("rows", "image", "key", "owner", "contrast", "n_pos"))
    for r in (off, f64):
        assert r["calls"]["functional.cosine_similarity"] == 1 and r["calls"]["maskformer_criterion._contrast_softplus"] == 2
        assert all(v == 0 for k, v in r["calls"].items() if k.startswith("reid_"))
        assert "rows" not in r["keys"][0] and "rows" not in r["keys"][1]

    # same seeds: same queries and assignments; the precondition on the model's actual queries: every unmatched row's top-two gap
    assert torch.equal(on["query"], off["query"])
    same = lambda a, b: all(torch.equal(x[0].cpu(), y[0].cpu()) and torch.equal(x[1].cpu(), y[1].cpu()) for x, y in zip(a, b))
    assert same(on["indices"], off["indices"]) and same(f64["indices"], off["indices"])
    pos_lists = [p[0].tolist() for p in on["indices"]]
    _, gap = R.nearest64(on["query"].cpu(), pos_lists)
    _, gap64 = R.nearest64(f64["query"].cpu(), pos_lists)
    for n, pl in enumerate(pos_lists):
        unmatched = [r for r in range(Q) if r not in pl]
        low = min(float(gap[n][unmatched].min()), float(gap64[n][unmatched].min()))
        print("image %d: minimum top-two cosine gap %.3e (needs %.3e)" % (n, low, R.GAP))
        assert low > R.GAP + 2 * float((on["query"].cpu().double() - f64["query"].cpu()).abs().max()), \
            "the decoder's queries leave a nearest positive undecided: choose other seeds"

    # the plan: items, clusters, drawn negatives
    assert len(on["plans"]) == 2 and on["plans"][0] == on["plans"][1] and len(on["plans"][0]) > 0
    assert on["plans"] == off["plans"] == f64["plans"]
    assert on["random"] == off["random"] == f64["random"]
    for k in on["aux"]:
        assert torch.equal(on["aux"][k], off["aux"][k]) and torch.equal(on["aux"][k], f64["aux"][k]), k

    fails = []
    assert sorted(on["losses"]) == sorted(off["losses"]) == ["loss_reid_mask", "loss_reid_query", "loss_reid_query_aux"]
    for k in off["losses"]:
        _bound("loss " + k, on["losses"][k], off["losses"][k], f64["losses"][k], fails)
    assert on["grads"].keys() == off["grads"].keys() == f64["grads"].keys() and len(on["grads"]) > 10
    g64 = f64["grads"]
    for n in off["grads"]:
        sib = n[:-len("bias")] + "weight"
        zero = n.endswith(".bias") and sib in g64 and float(g64[n].abs().max()) < 1e-12 * float(g64[sib].abs().max())
        _bound("grad " + n, on["grads"][n], off["grads"][n], g64[n], fails, zero_rule=zero)
    assert not fails, "\n".join(fails)

"""GPU: the reference-point L1 kernels (pct_refpoint_l1_forward_f32 / _backward_f32) and the strided sigmoid focal kernels
(pct_sigmoid_focal_strided_forward_f32 / _backward_f32) against the float64 restatements of tests/aux_loss_reference.py on the same
fp32 operands, through the wrappers of pctrans_amd/aux_loss.py.  The input families and the bounds are that module's;
tests/test_aux_loss_cpu.py asserts that every known-wrong variant leaves these bounds on these families by 10x.

Reference points: loss within (n + 2) 2^-24 sum|terms| for n summed terms; gradient exact zeros off the pairs, the exact sign on
them and a magnitude within 2 ulp of grad_loss / num_masks; a pair with an index out of range is counted and changes no other bit.
Focal: |hip - f64| <= max(2 |torch fp32 chain - f64|, 5e-6 max|f64|) for loss and gradient, the chain being
SetCriterion.loss_sem's on the same device.  Every call is repeated once and must give the same bits."""
import pytest
import torch

import aux_loss_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(case):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}


# ---------------------------------------------------------------- reference points
def _refpoint_run(case):
    from pctrans_amd import aux_loss
    d = _dev(case)
    src, tgt = d["src"].to(torch.int32), d["tgt"].to(torch.int32)
    out = []
    for _ in range(2):
        loss, status = aux_loss.refpoint_l1_forward(d["points"], d["target_points"], src, tgt, d["num_masks"])
        grad = aux_loss.refpoint_l1_backward(d["points"], d["target_points"], src, tgt, d["num_masks"], d["grad_loss"])
        out.append((loss.cpu(), int(status), grad.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][2], out[1][2]) and out[0][1] == out[1][1], "two calls differ"
    return out[0]


@pytest.mark.parametrize("name", sorted(R.REFPOINT_CASES))
def test_refpoint_l1_against_float64(name):
    case = R.refpoint_case(**R.REFPOINT_CASES[name])
    loss, status, grad = _refpoint_run(case)
    args = (case["points"], case["target_points"], case["src"], case["tgt"], case["num_masks"])
    want, _, terms, bad = R.refpoint_l1(*args)
    want_grad, count = R.refpoint_l1_grad(*args, case["grad_loss"])
    bound = R.refpoint_loss_bound(want, terms)
    err = (loss.double() - want).abs()
    print("%s: loss err max %.3e, bound min %.3e, terms %s" % (name, float(err.max()), float(bound.min()), terms[0]))
    assert status == bad == 0
    assert bool((err <= bound).all()), (err, bound)
    if terms[0] == 0:
        assert bool((loss == 0).all()) and bool((grad == 0).all())
    fails = R.refpoint_grad_failures(grad, want_grad, count, case["grad_loss"], case["num_masks"])
    assert not fails, "\n".join(fails)
    if "equal" in name:                                              # points == target in one coordinate: sgn(0) = 0
        for h in range(grad.shape[0]):
            s = int(case["src"][h, 0])
            assert int(count[h, s]) > 1 or (float(grad[h, s, 0]) == 0.0 and float(grad[h, s, 1]) != 0.0)


@pytest.mark.parametrize("name", ["h3_b2_q65_d4_p120_equal", "h1_b1_q3_d2_p1"])
def test_refpoint_pairs_out_of_range_are_counted_and_change_nothing_else(name):
    """Two pairs appended to every head, one with src == rows and one with tgt == -1 (then src == -5 and tgt == num_targets): the
    status counts 2 per head, and the loss and the whole gradient keep the bits of the call without them."""
    case = R.refpoint_case(**R.REFPOINT_CASES[name])
    loss, status, grad = _refpoint_run(case)
    heads, rows, _ = case["points"].shape
    T = case["target_points"].shape[0]
    for bad_src, bad_tgt in ((rows, -1), (-5, T)):
        worse = dict(case)
        worse["src"] = torch.cat([case["src"], torch.tensor([[bad_src, 0]] * heads)], dim=1)
        worse["tgt"] = torch.cat([case["tgt"], torch.tensor([[0, bad_tgt]] * heads)], dim=1)
        loss2, status2, grad2 = _refpoint_run(worse)
        assert status == 0 and status2 == 2 * heads
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_refpoint_function_and_its_status():
    """RefPointL1Function through refpoint_l1_losses: autograd hands the per-head gradients to the one backward launch, the
    status word rides on the result, and int64 indices are taken."""
    from pctrans_amd import aux_loss
    case = R.refpoint_case(**R.REFPOINT_CASES["h10_b2_q300_d2_p120_empty_repeat"])
    d = _dev(case)
    points = d["points"].clone().requires_grad_(True)
    loss = aux_loss.refpoint_l1_losses(points, d["target_points"], d["src"], d["tgt"], d["num_masks"])
    assert int(loss.status) == 0 and loss.shape == (10,)
    (loss * d["grad_loss"]).sum().backward()
    direct = aux_loss.refpoint_l1_backward(d["points"], d["target_points"], d["src"].int(), d["tgt"].int(), d["num_masks"], d["grad_loss"])
    assert torch.equal(points.grad, direct)
    assert not aux_loss.supported_refpoint(d["points"].cpu(), d["target_points"].cpu())
    assert not aux_loss.supported_refpoint(d["points"].double(), d["target_points"].double())
    assert not aux_loss.supported_refpoint(d["points"].transpose(0, 1), d["target_points"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not aux_loss.supported_refpoint(d["points"], d["target_points"])
    assert aux_loss.supported_refpoint(d["points"], d["target_points"])


# ---------------------------------------------------------------- focal
def _focal_run(case, grad_loss=1.5):
    from pctrans_amd import aux_loss
    d = _dev(case)
    g = torch.tensor(grad_loss, device=DEV)
    out = []
    for _ in range(2):
        loss, num_pos = aux_loss.sem_focal_forward(d["logits"], d["fg"], d["stride"], d["alpha"])
        grad = aux_loss.sem_focal_backward(d["logits"], d["fg"], d["stride"], d["alpha"], num_pos, g)
        out.append((loss.cpu(), float(num_pos), grad.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][2], out[1][2]) and out[0][1] == out[1][1], "two calls differ"
    return out[0]


def _focal_check(name, case):
    loss, num_pos, grad = _focal_run(case)
    args = (case["logits"], case["fg"], case["stride"], case["alpha"])
    want, want_pos, ell = R.sem_focal(*args)
    want_grad = R.sem_focal_grad_closed(*args, grad_loss=1.5)
    d = _dev(case)
    chain_loss, chain_grad = R.torch_chain_sem(d["logits"], d["fg"], d["stride"], d["alpha"], grad_loss=1.5)
    loss_bound, grad_bound = R.project_bound(chain_loss, want), R.project_bound(chain_grad, want_grad)
    loss_err, grad_err = abs(float(loss) - float(want)), float((grad.double() - want_grad).abs().max())
    print("%s: loss %.9g err %.3e bound %.3e (chain err %.3e); grad err %.3e bound %.3e (chain err %.3e); num_pos %d" % (
        name, float(want), loss_err, loss_bound, abs(float(chain_loss) - float(want)), grad_err, grad_bound,
        float((chain_grad.double().cpu() - want_grad).abs().max()), num_pos))
    assert num_pos == float(want_pos)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert loss_err <= loss_bound
    assert grad_err <= grad_bound
    return ell


@pytest.mark.parametrize("name", sorted(R.FOCAL_CASES))
def test_focal_against_float64(name):
    case = R.focal_case(**R.FOCAL_CASES[name])
    ell = _focal_check(name, case)
    if name == "20x28_f32":        # x = -100, t = 1, alpha 0.25: ce = 100 without overflow, m = 1, l = 25 -- as the only element
        one = {"logits": torch.full((1, 1, 1, 1), -100.0), "fg": torch.ones(1, 8, 8), "stride": 8, "alpha": 0.25}
        loss, num_pos, grad = _focal_run(one, grad_loss=1.0)
        assert float(loss) == 25.0 and num_pos == 1.0 and abs(float(grad) + 0.25) <= 2 ** -24
        assert float(ell.view(-1)[4]) == 25.0
    if name == "20x28_background":
        assert float(R.sem_focal(case["logits"], case["fg"], 8, 0.25)[1]) == 0.0


@pytest.mark.parametrize("name", sorted(R.FOCAL_CASES_LARGE))
def test_focal_on_several_workgroups_against_float64(name):
    _focal_check(name, R.focal_case(**R.FOCAL_CASES_LARGE[name]))


def test_focal_function_views_and_predicates():
    """SemFocalFunction through sem_focal_loss; maps that are slices of one buffer are read where they are, others are stacked."""
    from pctrans_amd import aux_loss
    case = R.focal_case(**R.FOCAL_CASES["20x28_bool_noalpha"])
    d = _dev(case)
    logits = d["logits"].clone().requires_grad_(True)
    loss = aux_loss.sem_focal_loss(logits, d["fg"], stride=8, alpha=-1.0)
    (loss * 1.5).backward()
    want_loss, num_pos, want_grad = _focal_run(case)
    assert torch.equal(loss.detach().cpu(), want_loss) and torch.equal(logits.grad.cpu(), want_grad)
    assert logits.grad.shape == logits.shape == (2, 1, 2, 3)
    buf = torch.zeros(16 + 2 * 20 * 28, dtype=torch.bool, device=DEV)
    fg = buf[16:].view(2, 20, 28)
    fg.copy_(d["fg"])
    dense = aux_loss.dense_maps([fg[0], fg[1]])
    assert dense.data_ptr() == fg.data_ptr() and dense.shape == fg.shape and torch.equal(dense, fg)
    stacked = aux_loss.dense_maps([fg[1], fg[0]])
    assert stacked.data_ptr() != fg.data_ptr() and torch.equal(stacked, fg.flip(0))
    mixed = aux_loss.dense_maps([fg[0], fg[1].float()])
    assert mixed.dtype == torch.float32 and torch.equal(mixed, fg.float())
    assert torch.equal(aux_loss.sem_focal_loss(d["logits"], dense, 8, -1.0).cpu(), want_loss)
    assert aux_loss.supported_sem(d["logits"], d["fg"], 8)
    assert not aux_loss.supported_sem(d["logits"], d["fg"], 4)                        # another slice: not these logits' size
    assert not aux_loss.supported_sem(d["logits"], d["fg"].to(torch.int32), 8)
    assert not aux_loss.supported_sem(d["logits"].cpu(), d["fg"].cpu(), 8)
    assert not aux_loss.supported_sem(d["logits"].bfloat16(), d["fg"], 8)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not aux_loss.supported_sem(d["logits"], d["fg"], 8)


def test_argument_errors_return_status_codes_without_a_launch():
    from pctrans_amd import _lib
    fails = R.status_code_failures(_lib.lib())
    assert not fails, "\n".join(fails)

"""CPU: the float64 restatements of tests/aux_loss_reference.py are SetCriterion.loss_refpoints / loss_sem; the two switches
defaults (PCT_REFPOINT_LOSS, PCT_SEM_LOSS) keep the rule of the others; the ctypes table has the header's parameter types; and the input families of
tests/test_aux_loss_gpu.py are hard enough: every known-wrong variant of either loss leaves that file's bounds by at least 10x."""
import re

import pytest
import torch

import aux_loss_reference as R
from pctrans_amd.loss import maskformer_criterion as crit
from pctrans_amd.loss.maskformer_criterion import SetCriterion


def _criterion(losses=("refpoints", "sem")):
    return SetCriterion(1, None, {}, 0.1, list(losses), 16, 3, 0.75)


# ---------------------------------------------------------------- the restatements are the criterion's losses
def _refpoint_inputs(counts, Q=7, L=4, seed=0):
    """Stacked points [L, N, Q, 2] float64, targets and an indices_list of L + 1 entries for images with counts[b] instances (an
    image without instances has the one zero point the target builders give it, and no pair)."""
    g = torch.Generator().manual_seed(seed)
    N = len(counts)
    stack = torch.rand(L, N, Q, 2, generator=g, dtype=torch.float64)
    targets = [{"center_points": torch.rand(max(c, 1), 1, 2, generator=g, dtype=torch.float64) * (c > 0),
                "labels": torch.ones(c, dtype=torch.long)} for c in counts]
    indices_list = [[(torch.randperm(Q, generator=g)[:c], torch.randperm(c, generator=g)) for c in counts] for _ in range(L + 1)]
    return stack, targets, indices_list


def _flat_pairs(indices, targets, Q):
    starts = [0]
    for t in targets[:-1]:
        starts.append(starts[-1] + t["center_points"].shape[0])
    src = torch.stack([torch.cat([s + b * Q for b, (s, _) in enumerate(ind)]) for ind in indices])
    tgt = torch.stack([torch.cat([t + starts[b] for b, (_, t) in enumerate(ind)]) for ind in indices])
    return src, tgt


@pytest.mark.parametrize("counts", [(3, 2), (4, 0), (1,)])
def test_refpoint_restatement_is_loss_refpoints_in_float64(counts):
    stack, targets, indices_list = _refpoint_inputs(counts)
    L, N, Q, dims = stack.shape
    c = _criterion()
    num_masks = float(max(sum(counts), 1))
    stack.requires_grad_(True)
    want = torch.stack([c.loss_refpoints({"reference_points": stack[j]}, targets, indices_list[j + 1], num_masks)["loss_refpoints"]
                        for j in range(L)])
    weights = torch.arange(1, L + 1, dtype=torch.float64)
    want_grad, = torch.autograd.grad((want * weights).sum(), stack)
    src, tgt = _flat_pairs(indices_list[1:], targets, Q)
    target_points = torch.cat([t["center_points"].flatten(1) for t in targets])
    got, _, terms, bad = R.refpoint_l1(stack.detach().view(L, N * Q, dims), target_points, src, tgt, num_masks)
    assert bad == 0 and terms == [2 * sum(counts)] * L
    assert float((got - want.detach()).abs().max()) <= 1e-12
    got_grad, count = R.refpoint_l1_grad(stack.detach().view(L, N * Q, dims), target_points, src, tgt, num_masks, weights)
    assert float((got_grad.view_as(want_grad) - want_grad).abs().max()) <= 1e-12
    assert int(count.sum()) == L * sum(counts)


def test_l1_backward_of_an_equal_coordinate_is_zero():
    """sgn(0) = 0: what torch's l1_loss backward gives and what the kernel's contract states."""
    a = torch.tensor([0.25, 0.5], dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad(torch.nn.functional.l1_loss(a, torch.tensor([0.25, 0.75], dtype=torch.float64), reduction="none").sum(), a)
    assert g.tolist() == [0.0, -1.0]


@pytest.mark.parametrize("kind", ["mixed", "background", "fraction"])
def test_focal_restatement_is_loss_sem_in_float64(kind, monkeypatch):
    case = R.focal_case(2, 20, 28, 8, 0.25, torch.float32 if kind == "fraction" else torch.bool, 21, kind=kind)
    logits = case["logits"].double().requires_grad_(True)
    c = _criterion()
    # loss_sem casts the targets with .float(), and binary_cross_entropy_with_logits of float64 logits and fp32 targets answers in
    # fp32: the maps go in as float64 and .float() leaves a float64 tensor as it is (the arbiter of test_train_step_all_on_gpu.py)
    real_float = torch.Tensor.float
    monkeypatch.setattr(torch.Tensor, "float", lambda t, *a, **k: t if t.dtype == torch.float64 else real_float(t, *a, **k))
    want = c.loss_sem({"sem_mask": logits}, [{"fg_masks": m.double()} for m in case["fg"]])["loss_sem"]
    assert want.dtype == torch.float64
    want_grad, = torch.autograd.grad(want, logits)
    got, num_pos, _ = R.sem_focal(logits.detach(), case["fg"], 8, 0.25)
    assert abs(float(got) - float(want.detach())) <= 1e-12
    assert (float(num_pos) == 0.0) == (kind == "background")          # the all-background batch: num_pos is clamped to 1
    assert float((R.sem_focal_grad(logits.detach(), case["fg"], 8, 0.25) - want_grad).abs().max()) <= 1e-12
    assert float((R.sem_focal_grad_closed(logits.detach(), case["fg"], 8, 0.25) - want_grad).abs().max()) <= 1e-12


def test_stack_of_a_float_map_among_bool_maps_is_fp32():
    maps = [torch.zeros(4, 4, dtype=torch.bool), torch.ones(4, 4, dtype=torch.float32)]
    assert torch.stack(maps).dtype == torch.float32


# ---------------------------------------------------------------- the switches
@pytest.mark.parametrize("function,variable", [("refpoint_default", "PCT_REFPOINT_LOSS"), ("sem_default", "PCT_SEM_LOSS")])
def test_switch_defaults_and_their_message(monkeypatch, function, variable):
    """The rule tests/test_abi.py states for the other switches: unset or empty gives "torch", "hip" and "torch" are taken,
    anything else raises with the variable's name and the value."""
    from pctrans_amd import aux_loss
    default = getattr(aux_loss, function)
    for value, want in ((None, "torch"), ("", "torch"), ("hip", "hip"), ("torch", "torch")):
        monkeypatch.delenv(variable, raising=False) if value is None else monkeypatch.setenv(variable, value)
        assert default() == want
    monkeypatch.setenv(variable, "triton")
    with pytest.raises(RuntimeError, match=re.escape("%s must be 'hip' or 'torch', got 'triton'" % variable)):
        default()


def test_the_library_exports_the_four_entries_and_the_table_names_their_test():
    from pctrans_amd import _lib
    assert sorted(_lib.AUX_LOSS_SYMBOLS) == ["pct_refpoint_l1_backward_f32", "pct_refpoint_l1_forward_f32",
                                             "pct_sigmoid_focal_strided_backward_f32", "pct_sigmoid_focal_strided_forward_f32"]
    assert all(v[2] == "tests/test_aux_loss_gpu.py" for v in _lib.AUX_LOSS_SYMBOLS.values())
    L = _lib.lib()
    for name, (argtypes, restype, _) in _lib.AUX_LOSS_SYMBOLS.items():
        assert getattr(L, name).argtypes == argtypes and getattr(L, name).restype == restype


def test_the_ctypes_table_has_the_parameter_types_of_the_header():
    """Parameter by parameter: a pointer is c_void_p, `long long` c_longlong, `float` c_float, `int` c_int.  (A pointer bound as
    c_int reaches the entry truncated to 32 bits: the status-code test cannot see that, a launch faults on it.)"""
    import ctypes
    import os
    from conftest import ROOT
    from pctrans_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pctrans_hip_aux_loss.h")).read()
    protos = dict(re.findall(r"PCT_API\s+int\s+(pct_\w+)\s*\(([^)]*)\)\s*;", hdr))
    assert sorted(protos) == sorted(_lib.AUX_LOSS_SYMBOLS)

    def ctype(param):
        if "*" in param:
            return ctypes.c_void_p
        return {"long long": ctypes.c_longlong, "float": ctypes.c_float, "int": ctypes.c_int}[" ".join(param.split()[:-1])]

    for name, params in protos.items():
        assert [ctype(p) for p in params.split(",")] == _lib.AUX_LOSS_SYMBOLS[name][0], name
        assert _lib.AUX_LOSS_SYMBOLS[name][1] == ctypes.c_int


def test_argument_errors_return_status_codes_without_a_launch():
    """No launch, so this runs without a GPU (tests/test_abi.py does the same for the encoder's entries)."""
    from pctrans_amd import _lib
    fails = R.status_code_failures(_lib.lib())
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- the GPU test's inputs are hard enough
REFPOINT_VARIANT_EXEMPT = {
    # no pair: every variant computes the same zeros
    ("h3_b1_q65_d2_p0", "shifted pairing"), ("h3_b1_q65_d2_p0", "difference for sign"),
    # one head: there is no other head's index row to take
    ("h1_b1_q3_d2_p1", "shifted pairing"),
}


@pytest.mark.parametrize("name", sorted(R.REFPOINT_CASES))
def test_refpoint_families_reject_the_wrong_variants(name):
    """On the float64 references alone: the head / indices pairing shifted by one leaves the loss bound, and the difference in
    place of its sign leaves the gradient rule, by at least 10x on every family (but where REFPOINT_VARIANT_EXEMPT says why not)."""
    case = R.refpoint_case(**R.REFPOINT_CASES[name])
    args = (case["points"], case["target_points"], case["src"], case["tgt"], case["num_masks"])
    want, _, terms, _ = R.refpoint_l1(*args)
    bound = R.refpoint_loss_bound(want, terms)
    if (name, "shifted pairing") not in REFPOINT_VARIANT_EXEMPT:
        wrong = R.refpoint_l1(*args, shift=1)[0]
        assert bool(((wrong - want).abs() >= 10 * bound).all()), (wrong, want, bound)
    if (name, "difference for sign") not in REFPOINT_VARIANT_EXEMPT:
        grad, count = R.refpoint_l1_grad(*args, case["grad_loss"])
        wrong = R.refpoint_l1_grad(*args, case["grad_loss"], sign=False)[0]
        assert R.refpoint_grad_failures(grad.float(), grad, count, case["grad_loss"], case["num_masks"]) == []
        fails = R.refpoint_grad_failures(wrong.float(), grad, count, case["grad_loss"], case["num_masks"])
        assert len(fails) >= case["points"].shape[0], fails               # every head fails the rule
        listed = count > 0
        g = (case["grad_loss"].double() / case["num_masks"])[:, None, None]
        # ... and by much more than 10 x 2 ulp: the worst element of every head is off by over a tenth of |g|
        off = ((wrong - grad).abs() / g)[listed[:, :, None].expand_as(grad)].view(grad.shape[0], -1)
        assert bool((off.max(dim=1).values > 0.1).all())


FOCAL_VARIANTS = {
    "offset 0": dict(offset=0),
    "alpha dropped": dict(use_alpha=False),
    "num_pos counts every pixel": dict(num_pos_mode="all"),
    "num_pos unclamped": dict(num_pos_mode="unclamped"),
    "m for m^2": dict(power=1),
}


def _focal_variant_applies(name, variant):
    cfg = R.FOCAL_CASES[name]
    if variant == "alpha dropped":
        return cfg["alpha"] >= 0                    # alpha = -1: there is no class weight to drop
    if variant == "num_pos unclamped":
        return cfg.get("kind") == "background"      # the clamp acts on a batch without positives alone
    return True


@pytest.mark.parametrize("name", sorted(R.FOCAL_CASES))
def test_focal_families_reject_the_wrong_variants(name):
    """On the float64 references alone, with the bound the GPU test applies (the torch fp32 chain evaluated here on the CPU): every
    wrong variant moves the loss by at least 10x the loss bound and the gradient by at least 10x the gradient bound -- but the
    unclamped num_pos, which differs on the all-background family alone (there it is not finite), and the dropped alpha, which
    needs an alpha to drop."""
    case = R.focal_case(**R.FOCAL_CASES[name])
    args = (case["logits"], case["fg"], case["stride"], case["alpha"])
    want, num_pos, _ = R.sem_focal(*args)
    want_grad = R.sem_focal_grad(*args, grad_loss=1.5)
    chain_loss, chain_grad = R.torch_chain_sem(*args, grad_loss=1.5)
    loss_bound, grad_bound = R.project_bound(chain_loss, want), R.project_bound(chain_grad, want_grad)
    assert loss_bound < 1e-4 * abs(float(want)) and grad_bound < 1e-4 * float(want_grad.abs().max())     # the yardstick is fp32 rounding
    assert float((R.sem_focal_grad_closed(*args, grad_loss=1.5) - want_grad).abs().max()) <= 1e-12
    for variant, kw in FOCAL_VARIANTS.items():
        if not _focal_variant_applies(name, variant):
            continue
        wrong = R.sem_focal(*args, **kw)[0]
        wrong_grad = R.sem_focal_grad(*args, grad_loss=1.5, **kw)
        if variant == "num_pos unclamped":
            assert float(num_pos) == 0 and not bool(torch.isfinite(wrong))
            continue
        assert abs(float(wrong) - float(want)) >= 10 * loss_bound, (variant, float(wrong), float(want), loss_bound)
        assert float((wrong_grad - want_grad).abs().max()) >= 10 * grad_bound, (variant, grad_bound)


def test_focal_planted_values():
    """x = -100, t = 1 with alpha 0.25: ce = 100 without overflow, m = 1, l = 25; x = 100, t = 0: l = 75."""
    case = R.focal_case(**R.FOCAL_CASES["20x28_f32"])
    _, _, ell = R.sem_focal(case["logits"], case["fg"], 8, 0.25)
    x, t = case["logits"].view(-1), R.focal_targets(case["fg"], 8).reshape(-1)
    assert (float(x[4]), float(t[4]), float(ell.view(-1)[4])) == (-100.0, 1.0, 25.0)
    assert (float(x[5]), float(t[5])) == (100.0, 0.0) and abs(float(ell.view(-1)[5]) - 75.0) < 1e-12

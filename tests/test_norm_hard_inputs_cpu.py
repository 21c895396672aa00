"""CPU: the properties of tests/norm_hard_inputs.py that the GPU tests of the normalising kernels lean on, stated on the
fixtures and on plain numpy evaluations alone:

  * exactness -- for every case the fp32 sum of a set, its mean and the centred values have the same bits in three summation
    orders (forward, reverse, a seeded permutation; np.cumsum is sequential) and the bits of float64;
  * the bound admits a correct kernel -- the plain fp32 two-pass formula stays within it in all three orders (constant sets:
    bit-exactly beta);
  * the bound rejects the wrong ones -- numpy mutants of the two-pass formula (one-pass variance; eps dropped, hard-coded to
    1e-5, added behind the square root; statistics of the neighbouring set) exceed it at least 100 times on every case of
    the family aimed at them."""
import numpy as np
import pytest

import norm_hard_inputs as nh

ALL = [(e,) + c for e in nh.ENTRIES for c in nh.case_ids(e, ["offset", "eps_matters", "constant"])]
FACTOR = 100.0


def _orders(n):
    fwd = np.arange(n)
    return [fwd, fwd[::-1].copy(), np.random.RandomState(n).permutation(n)]


def _seq_sum(a):
    return np.cumsum(a, axis=1, dtype=np.float32)[:, -1:]


def _f32(case):
    g = np.broadcast_to(case.gamma_sets, case.pre.shape).astype(np.float32)
    b = np.broadcast_to(case.beta_sets, case.pre.shape).astype(np.float32)
    return case.pre.astype(np.float32), g, b


def _normalise_f32(case, order, mutant=None):
    """The two-pass formula in fp32, summing in `order`; `mutant` names one deliberate mistake."""
    pre, gamma, beta = _f32(case)
    S, n = pre.shape
    v = pre[:, order]
    inv_n, one = np.float32(1.0 / n), np.float32(1.0)
    eps = np.float32(0.0 if mutant == "eps_dropped" else 1e-5 if mutant == "eps_hardcoded" else case.eps)
    mean = _seq_sum(v) * inv_n
    d = v - mean
    if mutant == "one_pass":
        var = np.maximum(_seq_sum(v * v) * inv_n - mean * mean, np.float32(0.0))
    else:
        var = _seq_sum(d * d) * inv_n
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = one / (np.sqrt(var) + eps) if mutant == "eps_outside" else one / np.sqrt(var + eps)
        if mutant == "neighbour":
            other = np.minimum(np.arange(S) ^ 1, S - 1)
            d, rstd = v - mean[other], rstd[other]
        out = np.empty_like(v)
        out[:, order] = d * rstd * gamma[:, order] + beta[:, order]
    return out


def _ratio(case, out):
    err = np.abs(out.astype(np.float64) - case.want_sets)
    r = err / np.maximum(nh.bound(case.want_sets, case.gz_sets, case.n), 1e-300)
    return float(np.where(np.isfinite(r), r, np.inf).max())


def _pre_norm_f32(entry, case):
    """The pre-norm values formed in fp32 from the fp32 inputs, as the kernels form them (library matmul order; both
    associations of bias and residual), in the layout of case.pre."""
    i = {k: (None if v is None else v.numpy()) for k, v in case.inputs.items()}
    assert all(v is None or v.dtype == np.float32 for v in i.values())
    if entry == "add_layer_norm":
        return [i["x"] if i["y"] is None else i["x"] + i["y"]]
    if entry == "groupnorm_flatten":
        return [i["x"].reshape(case.pre.shape)]
    if entry == "ffn_layer_norm":
        hid = np.maximum(i["x"] @ i["w1"].T + i["b1"], np.float32(0.0))
        prod = hid @ i["w2"].T
        return [(prod + i["b2"]) + i["x"], prod + (i["b2"] + i["x"])]
    if entry == "conv1x1_groupnorm_tokens":
        N, K = i["x"].shape[:2]
        prod = np.matmul(i["weight"].reshape(128, K), i["x"].reshape(N, K, -1))
        return [(prod + i["bias"][None, :, None]).reshape(case.pre.shape)]
    prod = i["x"] @ i["weight"].T
    return [(prod + i["bias"]) + i["residual"], prod + (i["bias"] + i["residual"])]


@pytest.mark.parametrize("entry,family,geometry,variant", ALL, ids=nh.case_name)
def test_sums_means_and_centred_values_are_exact_in_any_order(entry, family, geometry, variant):
    case = nh.build(entry, family, geometry, variant)
    pre32 = case.pre.astype(np.float32)
    n = case.n
    for formed in _pre_norm_f32(entry, case):
        assert formed.dtype == np.float32 and np.array_equal(formed.astype(np.float64), case.pre)
    assert n & (n - 1) == 0 and np.array_equal(pre32.astype(np.float64), case.pre)
    sum64 = case.pre.sum(axis=1, keepdims=True)
    mean64 = sum64 / n
    d64 = case.pre - mean64
    for order in _orders(n):
        s = _seq_sum(pre32[:, order])
        mean = s * np.float32(1.0 / n)
        d = np.empty_like(pre32)
        d[:, order] = pre32[:, order] - mean
        assert s.dtype == mean.dtype == d.dtype == np.float32
        assert np.array_equal(s.astype(np.float64), sum64)
        assert np.array_equal(mean.astype(np.float64), mean64)
        assert np.array_equal(d.astype(np.float64), d64)
    # every prefix of the forward sum as well: no partial sum is rounded
    assert np.array_equal(np.cumsum(pre32, axis=1, dtype=np.float32).astype(np.float64), np.cumsum(case.pre, axis=1))


@pytest.mark.parametrize("entry,family,geometry,variant", ALL, ids=nh.case_name)
def test_the_fp32_two_pass_formula_stays_inside_the_bound(entry, family, geometry, variant):
    case = nh.build(entry, family, geometry, variant)
    _, _, beta = _f32(case)
    worst = 0.0
    for order in _orders(case.n):
        out = _normalise_f32(case, order)
        if family == "constant":
            assert np.array_equal(out.view(np.int32), beta.view(np.int32))
        else:
            worst = max(worst, _ratio(case, out))
    print("%s %s: two-pass fp32 worst |err| / bound = %.3f" % (entry, nh.case_name((family, geometry, variant)), worst))
    assert worst <= 1.0, worst


def test_the_n_over_2_term_is_needed_and_sufficient_for_layernorm():
    """With a constant 16u alone the plain formula leaves the bound from n = 128 on (the sum of n squares is not exact);
    with the n/2 term it stays below a half."""
    for cols in (64, 128, 256):
        case = nh.build("add_layer_norm", "offset", (1031, cols, False))
        flat = 16.0 * nh.U * np.abs(case.gz_sets) + 2.0 * nh.U * np.abs(case.want_sets)
        r_flat = r_full = 0.0
        for order in _orders(cols):
            err = np.abs(_normalise_f32(case, order).astype(np.float64) - case.want_sets)
            r_flat, r_full = max(r_flat, float((err / flat).max())), max(r_full, _ratio(case, _normalise_f32(case, order)))
        print(cols, r_flat, r_full)
        assert r_full < 0.5 and r_flat > 0.3


def _mutant_cases(family, only=None):
    out = []
    for e in nh.ENTRIES:
        for c in nh.case_ids(e, [family]):
            if only is None or only(c):
                out.append((e,) + c)
    return out


def _mutant_ratio(entry, family, geometry, variant, mutant):
    case = nh.build(entry, family, geometry, variant)
    worst = min(_ratio(case, _normalise_f32(case, order, mutant)) for order in _orders(case.n))
    print("%s %s: %s exceeds the bound %.3g times" % (entry, nh.case_name((family, geometry, variant)), mutant, worst))
    return worst


@pytest.mark.parametrize("entry,family,geometry,variant", _mutant_cases("offset"), ids=nh.case_name)
def test_one_pass_variance_is_caught_on_offset(entry, family, geometry, variant):
    assert _mutant_ratio(entry, family, geometry, variant, "one_pass") >= FACTOR


@pytest.mark.parametrize("entry,family,geometry,variant", _mutant_cases("offset"), ids=nh.case_name)
def test_statistics_of_the_neighbouring_set_are_caught_on_offset(entry, family, geometry, variant):
    assert _mutant_ratio(entry, family, geometry, variant, "neighbour") >= FACTOR


@pytest.mark.parametrize("mutant", ["eps_dropped", "eps_outside"])
@pytest.mark.parametrize("entry,family,geometry,variant", _mutant_cases("eps_matters"), ids=nh.case_name)
def test_a_misplaced_eps_is_caught_on_eps_matters(entry, family, geometry, variant, mutant):
    assert _mutant_ratio(entry, family, geometry, variant, mutant) >= FACTOR


@pytest.mark.parametrize("entry,family,geometry,variant",
                         _mutant_cases("eps_matters", lambda c: nh.EPS_VARIANTS[c[2]][1] != 1e-5), ids=nh.case_name)
def test_a_hard_coded_eps_is_caught_where_the_module_sets_another(entry, family, geometry, variant):
    assert _mutant_ratio(entry, family, geometry, variant, "eps_hardcoded") >= FACTOR


def test_families_have_the_structure_they_claim():
    case = nh.build("add_layer_norm", "offset", (1031, 128, True))
    x, y = case.inputs["x"].double().numpy(), case.inputs["y"].double().numpy()
    assert np.array_equal((case.inputs["x"] + case.inputs["y"]).double().numpy(), x + y)          # x + y is exact in fp32
    mean, spread = case.pre.mean(axis=1), case.pre.std(axis=1)
    assert 100 < float((np.abs(mean) / spread).min()) and float((np.abs(mean) / spread).max()) < 3000
    mags = np.abs(mean)
    assert float(mags[:9].max() / mags[:9].min()) >= 2.0 ** 39                                   # neighbours up to 2^40 apart
    for entry in nh.ENTRIES:
        for family, geometry, variant in nh.case_ids(entry, ["eps_matters"]):
            c = nh.build(entry, family, geometry, variant)
            assert 1e-6 < float(c.pre.var(axis=1).min()) and float(c.pre.var(axis=1).max()) < 1e-4
        for family, geometry, variant in nh.case_ids(entry, ["constant"]):
            c = nh.build(entry, family, geometry, variant)
            assert float(np.ptp(c.pre, axis=1).max()) == 0.0 and len(np.unique(c.pre[:, 0])) >= 3
        for family, geometry, variant in nh.case_ids(entry, ["nonfinite"]):
            c = nh.build(entry, family, geometry, variant)
            hit = c.poisoned_sets
            assert 2 <= int(hit.sum()) < hit.size                                                  # something stays clean
            bad = [n for n, t in c.inputs.items() if t is not None and not bool(np.isfinite(t.numpy()).all())]
            assert bad and all(bool(np.isfinite(t.numpy()).all()) for t in c.clean.inputs.values() if t is not None)
            assert bool(c.poisoned.any()) and not bool(c.poisoned.all())
    # the split-bf16 GEMMs see operands whose first plane is the whole value, except x of the FFN (three planes, 24 bits)
    import torch
    for entry, names in (("linear_layer_norm", ("x", "weight")), ("conv1x1_groupnorm_tokens", ("x", "weight")),
                         ("ffn_layer_norm", ("w1", "w2"))):
        for family, geometry, variant in nh.case_ids(entry, ["offset", "eps_matters"]):
            c = nh.build(entry, family, geometry, variant)
            for name in names:
                t = c.inputs[name]
                assert torch.equal(t.bfloat16().float(), t), (entry, family, name)

"""GPU: the four forward paths of the dynamic mask head (csrc/dyn_mask_head.hip with fp32 and with bf16 output,
csrc/dyn_mask_head_mfma.hip, csrc/dyn_mask_head_fused.hip) and the default route against the float64 reference with each
path's documented rounding points (tests/dmh_exact_reference.py), through dynamic_mask_head_forward:

  * families A1 / A2 (inputs whose result does not depend on the order of any accumulation; tests/test_dmh_exact_cpu.py
    asserts that condition): every element of the upsampled output bit for bit, every byte of the attention mask -- exactly
    for targets at 1/2, 1/4, 1/8 of the map, elsewhere up to the band the fp32 quotient weights leave around the threshold;
  * family C (generic values): an elementwise bound propagated from each accumulation's own terms, and bit equality at
    every element whose four taps and whose own rounding are stable.
The attention mask is allocated with torch.empty, so every byte is compared (as uint8) and each path reruns with other
parameters into fresh outputs."""
import numpy as np
import pytest
import torch

import dmh_exact_reference as R

pytestmark = pytest.mark.gpu

# route -> (output dtype, `kernel` argument, rounding points of the reference)
ROUTES = {
    "f32": (torch.float32, None, "f32"),
    "valu": (torch.bfloat16, "valu", "valu_bf16"),
    "mfma": (torch.bfloat16, "mfma", "mfma"),
    "fused": (torch.bfloat16, "fused", "mfma"),
    "default": (torch.bfloat16, None, "mfma"),
}


def _routes(H, W, target):
    from pctrans_amd import dynamic_mask_head as dmh
    return [r for r in ROUTES if r != "fused" or dmh.fused_geometry(H, W, target)]


def _run(case, route, nq=None):
    from pctrans_amd import dynamic_mask_head as dmh
    dtype, kernel, _ = ROUTES[route]
    feats = torch.from_numpy(case["feats"]).cuda()
    ref = torch.from_numpy(case["ref"][:, :nq]).contiguous().cuda()
    params = torch.from_numpy(case["params"][:, :nq]).contiguous().cuda()
    up, amask = dmh.dynamic_mask_head_forward(feats, ref, params, R.STRIDE, case["rel"], case["target"], out_dtype=dtype,
                                              kernel=kernel)
    N, _, H, W = case["feats"].shape
    Q = params.shape[1]
    assert up.dtype == dtype and up.shape == (N, Q, 2 * H, 2 * W)
    assert amask.dtype == torch.bool and amask.shape == (N, Q, case["target"][0] * case["target"][1])
    return up, amask.view(torch.uint8).cpu().numpy().reshape(N, Q, *case["target"])


def _same_bits(up, want64):
    """Every element: bf16 outputs through their bit patterns, fp32 through torch.equal."""
    if up.dtype == torch.float32:
        w = torch.from_numpy(want64).float()
        assert torch.equal(w.double(), torch.from_numpy(want64)), "reference value is not an fp32 number"
        return torch.equal(up.cpu(), w), float((up.cpu() - w).abs().max())
    w = torch.from_numpy(want64).bfloat16()
    assert torch.equal(w.double(), torch.from_numpy(want64))
    bad = up.cpu().view(torch.int16) != w.view(torch.int16)
    return not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:4].tolist())


def _check_exact(case, o, route, up, mask):
    ok, info = _same_bits(up, o["up"])
    assert ok, (route, info)
    differ = mask != o["mask"].astype(np.uint8)                 # any byte that is neither 0 nor 1 differs from both
    assert not (differ & ~o["mask_free_exact"]).any(), (route, int((differ & ~o["mask_free_exact"]).sum()),
                                                        np.argwhere(differ & ~o["mask_free_exact"])[:4].tolist())
    assert set(np.unique(mask).tolist()) <= {0, 1}


@pytest.fixture(autouse=True)
def _no_kernel_override(monkeypatch):
    monkeypatch.delenv("PCT_DMH_KERNEL", raising=False)


@pytest.mark.parametrize("rel", [True, False])
@pytest.mark.parametrize("family", ["a1", "a2"])
@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)))
def test_exact_inputs_every_element_bit_for_bit(gi, family, rel):
    N, Q, H, W, target = R.GEOMETRIES[gi]
    case = R.exact_case(gi, family, rel)
    outs = {}
    for route in _routes(H, W, target):
        up, mask = _run(case, route)
        _check_exact(case, R.exact_reference(gi, family, rel, ROUTES[route][2]), route, up, mask)
        outs[route] = up
    if family == "a1":                                             # pass-through: the same bits from every bf16 path
        for route in outs:
            if route not in ("f32", "valu"):
                assert torch.equal(outs[route].view(torch.int16), outs["valu"].view(torch.int16)), route
        assert torch.equal(outs["f32"].bfloat16().view(torch.int16), outs["valu"].view(torch.int16))


@pytest.mark.parametrize("rel", [True, False])
@pytest.mark.parametrize("family", ["a1", "a2"])
def test_half_empty_last_pair(family, rel):
    """Q = 101: query 100 sits alone in its pair; the first 100 planes are those of a Q = 100 run."""
    gi = 8
    N, Q, H, W, target = R.GEOMETRIES[gi]
    assert Q == 101
    case = R.exact_case(gi, family, rel)
    for route in _routes(H, W, target):
        o = R.exact_reference(gi, family, rel, ROUTES[route][2])
        up, mask = _run(case, route)
        ok, info = _same_bits(up[:, 100:], o["up"][:, 100:])
        assert ok, (route, info)
        assert not ((mask[:, 100] != o["mask"][:, 100].astype(np.uint8)) & ~o["mask_free_exact"][:, 100]).any(), route
        up100, mask100 = _run(case, route, nq=100)
        same = up100.view(torch.int32 if up.dtype == torch.float32 else torch.int16) == \
            up[:, :100].view(torch.int32 if up.dtype == torch.float32 else torch.int16)
        assert bool(same.all()), route
        assert np.array_equal(mask100, mask[:, :100]), route


@pytest.mark.parametrize("gi", [7, 10])
def test_rerun_with_other_parameters_writes_every_mask_byte(gi):
    """The mask buffer is torch.empty and the caching allocator hands the previous run's block back: a byte a path does
    not write keeps the other parameters' value (or garbage) and fails the full comparison."""
    N, Q, H, W, target = R.GEOMETRIES[gi]
    for route in _routes(H, W, target):
        for family, rel in (("a1", True), ("a2", True), ("a1", False), ("a2", False), ("a1", True)):
            case = R.exact_case(gi, family, rel)
            up, mask = _run(case, route)
            _check_exact(case, R.exact_reference(gi, family, rel, ROUTES[route][2]), route, up, mask)
            del up


@pytest.mark.parametrize("ci", range(8))
def test_generic_values_elementwise_bound_and_forced_bits(ci):
    """Family C.  fp32: |got - want64| <= bound at every element, the bound propagated from each accumulation's own terms.
    bf16: bit equality wherever the four taps are stable logits and the blend is clear of a bf16 boundary, the bound elsewhere."""
    case = R.generic_case(ci)
    N, Q, H, W = case["geometry"]
    for route in _routes(H, W, case["target"]):
        o = R.generic_reference(ci, ROUTES[route][2])
        up, mask = _run(case, route)
        got = up.double().cpu().numpy()
        ratio = np.abs(got - o["up_pre"]) / o["up_bound"]
        share = float(o["up_bits"].mean())
        loose = ~o["up_bits"] & (route != "f32")
        print("family C case %d route %-7s max |got - want| / bound = %.4f   bit-checked share = %.4f   "
              "%d of the %d other bf16 elements differ from the rounded reference" %
              (ci, route, float(ratio.max()), share, int(((got != o["up"]) & loose).sum()), int(loose.sum())))
        assert ratio.max() <= 1.0, (route, float(ratio.max()), np.argwhere(ratio > 1)[:4].tolist())
        if route != "f32":
            wrong = (got != o["up"]) & o["up_bits"]
            assert not wrong.any(), (route, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
        differ = (mask != o["mask"].astype(np.uint8)) & ~o["mask_free"]
        assert not differ.any(), (route, int(differ.sum()), np.argwhere(differ)[:4].tolist())

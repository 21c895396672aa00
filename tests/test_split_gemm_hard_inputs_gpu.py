"""GPU: the split-bf16 GEMM kernels with a bias / ReLU epilogue on the operands of tests/split_gemm_hard_inputs.py, against the
exact float64 product, through the fused_ops wrappers (`*_supported` asserted first where the entry has such a predicate;
fused_ops.linear_k128 is called directly, as its predicate asks 4096 rows for routing purposes only).

  entry               kernel                                          shapes
  linear_k128         linear_k128_split.hip (linear_k128.hip under    rows 7/33/97 x n 128/256/384, relu and bias on and off; x_add
                      PCT_LIN_KERNEL=f32, one child process)          shared by 3 images of 45 rows; 6280 rows x n 1024 (slots of
                                                                      3 and 4 tiles), x_add shared by 8 images of 785 rows
  linear_k128_multi   the same kernel, three segments                 135 rows, n 128/256/128, add_x2 1/0/1 with period 45
  conv1x1_nchw        conv1x1_split.hip, split_tr_gemm.hpp            K 16/48/256, 8x16 / 8x32, N = 2
  fpn_stage           fpn_stage.hip, the 3 x 3 product                5x33 / 8x64, N = 2, enc NCHW and channels-last
  linear_add_layer_norm  linear_k128_split.hip, LayerNorm epilogue    rows 33/97 (cancel forms, bound of the norm tests)
  linear_layer_norm   linear_ln_split.hip                             K 32/96/1024, rows 7/129 (the same)
  ffn_layer_norm      ffn_fused_split.hip, both products              F 32/96, rows 37/257, + row stride 160 (the same)
  conv1x1_groupnorm_tokens  conv1x1_split.hip + GroupNorm records     K 16/48/256, 8x16 / 8x32, N = 2 (the same, n = 4 H W)

Families and what is asserted (tests/split_gemm_hard_inputs.py has the constructions and the derivation of the bound):
  planes, range   |got - want| <= 2u (|T| + |want|) per element; the worst ratio is printed
  routing         the selected operand bit for bit
  containment     two launches, clean and poisoned: reached rows / pixels entirely non-finite (behind the ReLU as well), every other
                  element has the bits of the clean run
and two calls on the planes cases give the same bits.  Under PCT_LIN_KERNEL=f32 the fp32-MFMA twin takes routing and containment
as they are and planes under the bound of a recursive fp32 sum, (K + 2) u sum |x w| + 2u |want|.

Why the twin keeps a bound of its own: an fp32 chain is NOT exact on these operands.  One product x w has up to 27 significant
bits (a 24-bit x times a 3-bit w), so fl32 rounds already the first term of a chain, and in a cancel form the sum that is left
is far below the terms that were rounded on the way: the error of an fp32 kernel scales with sum |x w|, not with |T|.  The rule
that makes hi and lo exact holds for bf16 pieces, whose products have 16 bits.  Routing and containment do not depend on it.

Observed on the MI355X, worst |err| / bound over the cases of an entry: linear_k128 planes 0.500, range 0.500; linear_k128_multi
planes 0.496; conv1x1_nchw planes 0.500, range 0.500; fpn_stage planes 0.500; under the bound of the norm tests
linear_add_layer_norm 0.435, linear_layer_norm 0.467, ffn_layer_norm planes 0.457 and range 0.495, conv1x1_groupnorm_tokens
0.414; linear_k128 under PCT_LIN_KERNEL=f32 planes 0.019 of its own bound.  0.500 is the least the bound allows a correct kernel:
one rounding of hi + lo and one of the bias add, u (|T| + |want|), against 2u (|T| + |want|).
Every routing case came back bit for bit, every reached row entirely non-finite (with the ReLU that passes a NaN on: fmaxf had
returned 0 for it) and no other row changed a bit, the 6280-row case and the three segments of the multi call included.  The case
with x in [2^-110, 2^-103) passed like the others: neither v_cvt_pk_bf16_f32 nor the matrix cores flush bf16 subnormals, so the
split's documented floor stays 2^-110.
The FFN's containment case takes a NaN and an inf, not the finite value above the split's domain: there the NaN of W1 x is
dropped by the hidden layer's fmaxf and the residual is finite, so nothing makes the row non-finite (read from the code, not
run: the norm's variance overflows and the row comes out as beta).
Hand mutations on a scratch build (not committed), one per kernel file, each run once, were all caught (the first five before the
FFN and GroupNorm cases existed, the counts are of the 299 cases of that day):
  linear_k128_split.hip, the tail-row clamp one row short: 177 cases (every entry of the file: planes, range, routing, containment,
    multi, both LayerNorm forms of the K = 128 epilogue -- the last ragged row is neither read nor stored);
  split_bf16.hpp, the w3 a1 term dropped from split_mfma6 as linear_k128_split.hip sees it: the 62 cases with w in three planes
    (planes w3 plain and cancel, range w_small / w_large, the routing mirror, multi, linear_add_layer_norm w3 probing plane 3;
    ratios from 9e2 to 8e6) and no other;
  conv1x1_split.hip, planes 2 and 3 of the weight image swapped in its staging store: the 12 x2w2 cases of conv1x1_nchw;
  fpn_stage.hip, the tap offset of the 3 x 3 loop transposed: all 8 fpn_stage planes cases;
  linear_ln_split.hip, planes 2 and 3 swapped in split_bf16x3_kernel's store: the 6 x2w2 cases of linear_layer_norm;
  ffn_fused_split.hip, planes 2 and 3 of the W2 image swapped in its staging store: the 5 second-GEMM x2w2 cases of
    ffn_layer_norm (four geometries and the strided rows) and no other of the 383.
Not probed: a3 w1 of the FFN's FIRST product (tests/split_gemm_hard_inputs.py says why no x with three pieces fits the norm's
rule there; the second product probes a3 w1 through b1), and the lateral product of fpn_stage."""
import atexit
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import split_gemm_hard_inputs as sg

pytestmark = pytest.mark.gpu

from pctrans_amd import fused_ops  # noqa: E402

WORST = {}


def _note(entry, family, ratio):
    WORST[(entry, family)] = max(WORST.get((entry, family), 0.0), ratio)


@atexit.register
def _report():
    for (entry, family), ratio in sorted(WORST.items()):
        print("worst |err| / bound  %-18s %-8s %.3f" % (entry, family, ratio))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _linear_module(w, bias):
    lin = nn.Linear(w.shape[1], w.shape[0], bias=bias is not None)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w))
        if bias is not None:
            lin.bias.copy_(torch.from_numpy(bias))
    return lin.cuda()


def _rows(case, x, x_add):
    """x (and x_add) as the wrappers take them: [images, period, 128] and [1, period, 128] with a shared x_add"""
    x = _dev(case.x if x is None else x)
    if not case.period:
        return x, None
    xa = _dev(case.x_add if x_add is None else x_add).view(1, case.period, 128)
    x = x.view(case.rows // case.period, case.period, 128)
    assert fused_ops._x_add_ok(x, xa)
    return x, xa


def run_linear(case, geometry=None, x=None, x_add=None):
    xt, xa = _rows(case, x, x_add)
    with torch.no_grad():
        out = fused_ops.linear_k128(xt, _dev(case.w), _dev(case.bias), relu=case.relu, x_add=xa)
    return out.reshape(case.rows, case.n).cpu().numpy()


def run_multi(cases, x=None, x_add=None):
    """-> [output per segment]; `cases`: objects with w, bias, use_add that share x, x_add, period"""
    xt, xa = _rows(cases[0], x, x_add)
    layers = [(_linear_module(c.w, c.bias), bool(c.use_add)) for c in cases]
    with torch.no_grad():
        outs = fused_ops.linear_k128_multi(xt, layers, x_add=xa)
    return [o.reshape(cases[0].rows, -1).cpu().numpy() for o in outs]


def run_conv(case, geometry, x=None, x_add=None):
    K, H, W = geometry
    conv = nn.Conv2d(K, 128, kernel_size=1, bias=case.bias is not None)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(case.w).view(128, K, 1, 1))
        if case.bias is not None:
            conv.bias.copy_(torch.from_numpy(case.bias))
    conv = conv.cuda()
    x4 = _dev(sg.rows_to_nchw(case.x if x is None else x, 2, H, W))
    with torch.no_grad():
        assert fused_ops.conv1x1_nchw_supported(x4, conv)
        out = fused_ops.conv1x1_nchw(x4, conv)
    return sg.nchw_to_rows(out.cpu().numpy())


def run_fpn(case, channels_last, enc=None):
    """The stage with a zero lateral input and no norm: y = enc exactly, out = relu(conv3x3(enc) + b3)."""
    from pctrans_amd.layers import Conv2d
    N, H, W = case.N, case.H, case.W
    lat = Conv2d(16, 128, kernel_size=1, bias=True, norm=None)
    outc = Conv2d(128, 128, kernel_size=3, stride=1, padding=1, bias=True, norm=None, activation=F.relu)
    with torch.no_grad():
        lat.bias.zero_()
        outc.weight.copy_(torch.from_numpy(case.w3))
        outc.bias.copy_(torch.from_numpy(case.bias))
    lat, outc = lat.cuda().eval(), outc.cuda().eval()
    e = _dev(case.enc if enc is None else enc)
    if channels_last:                                            # the view of the encoder's token rows
        e = e.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert fused_ops._fpn_enc_layout(e) == 1
    x = torch.zeros((N, 16, 2 * H, 2 * W), device="cuda")
    with torch.no_grad():
        assert fused_ops.fpn_stage_supported(x, e, lat, outc)
        out = fused_ops.fpn_stage(x, e, lat, outc)
    return sg.nchw_to_rows(out.cpu().numpy())


def run_linear_add_layer_norm(case):
    """pct_linear_k128_add_layernorm_f32 as fused_ops.linear_add_layer_norm calls it; called here because the wrapper's predicate
    asks 4096 rows (for routing purposes only) and these cases have 33 and 97."""
    from pctrans_amd import _lib
    i = {k: v.cuda() for k, v in case.inputs.items()}
    rows = i["x"].shape[0]
    out = torch.empty((rows, 128), dtype=torch.float32, device="cuda")
    with torch.cuda.device(out.device):
        rc = _lib.lib().pct_linear_k128_add_layernorm_f32(
            i["x"].data_ptr(), i["x"].stride(0), i["weight"].data_ptr(), i["bias"].data_ptr(), i["residual"].data_ptr(),
            i["residual"].stride(0), i["gamma"].data_ptr(), i["beta"].data_ptr(), float(case.eps), rows, out.data_ptr(), 128,
            torch.cuda.current_stream(out.device).cuda_stream)
    _lib.check(rc, "linear_add_layer_norm")
    return out


def run_linear_layer_norm(case):
    import test_norm_hard_inputs_gpu as tn                       # its runner: predicate asserted, fall-backs raise
    return tn.run_linear_layer_norm(case)


def run_ffn_layer_norm(case, row_stride=None):
    import test_norm_hard_inputs_gpu as tn
    return tn.run_ffn_layer_norm(case, row_stride=row_stride)


def run_conv1x1_groupnorm_tokens(case):
    import test_norm_hard_inputs_gpu as tn                       # predicate asserted, the token rows around the level untouched
    return tn.run_conv1x1_groupnorm_tokens(case)


def _norm_ratio(entry, family, label, case, got):
    import norm_hard_inputs as nh
    ratio = nh.error_ratio(case, got)
    print("%s %s %s: worst |err| / bound = %.3f" % (entry, family, label, ratio))
    _note(entry, family, ratio)
    assert ratio <= 1.0, (entry, family, label, ratio)


@pytest.mark.parametrize("geometry", sg.CONV_GEOMETRIES, ids=sg.name)
@pytest.mark.parametrize("variant", [v for v, _ in sg.GROUPNORM_VARIANTS])
def test_planes_in_front_of_group_norm(variant, geometry):
    """conv1x1_groupnorm_tokens: the cancel forms as the convolution, sets of 4 H W values, the norm tests' bound unchanged"""
    case = sg.groupnorm_case(variant, *geometry)
    _norm_ratio("conv1x1_groupnorm_tokens", "planes", sg.name((geometry, variant)), case, run_conv1x1_groupnorm_tokens(case))


FFN_CASES = [(g, w, v, p) for g in sg.FFN_GEOMETRIES for (w, v, p) in sg.FFN_VARIANTS]


@pytest.mark.parametrize("geometry,which,variant,probes", FFN_CASES, ids=sg.name)
def test_planes_in_the_fused_ffn(geometry, which, variant, probes):
    """ffn_layer_norm: `which` = 1 probes W1 x (x short, it is the residual), 2 probes W2 h through h = relu(b1) with W1 = 0"""
    case = sg.ffn_case(which, variant, probes, *geometry)
    _norm_ratio("ffn_layer_norm", "planes", sg.name((geometry, which, variant, probes)), case, run_ffn_layer_norm(case))


@pytest.mark.parametrize("which,variant,probes", sg.FFN_VARIANTS, ids=sg.name)
def test_planes_in_the_fused_ffn_on_strided_rows(which, variant, probes):
    case = sg.ffn_case(which, variant, probes, 257, 32)
    _norm_ratio("ffn_layer_norm", "planes", "stride 160 " + sg.name((which, variant, probes)), case,
                run_ffn_layer_norm(case, row_stride=160))


@pytest.mark.parametrize("geometry", sg.FFN_GEOMETRIES, ids=sg.name)
@pytest.mark.parametrize("which,variant,probes", sg.FFN_VARIANTS[:4], ids=sg.name)
def test_range_in_the_fused_ffn(which, variant, probes, geometry):
    """the first-GEMM cases with rows from 2^-40 to 2^40"""
    case = sg.ffn_case(which, variant, probes, *geometry, ex_set=sg.FFN_RANGE)
    _norm_ratio("ffn_layer_norm", "range", sg.name((geometry, which, variant, probes)), case, run_ffn_layer_norm(case))


LN_RUN = {"linear_add_layer_norm": run_linear_add_layer_norm, "linear_layer_norm": run_linear_layer_norm}
LN_CASES = [(e, g, v, p) for e, gs in sg.LAYER_NORM_GEOMETRIES.items() for g in gs for (v, p) in sg.LAYER_NORM_VARIANTS]


@pytest.mark.parametrize("entry,geometry,variant,probes", LN_CASES, ids=sg.name)
def test_planes_in_front_of_layer_norm(entry, geometry, variant, probes):
    """the cancel forms as the product of norm(residual + x W^T + bias), under the bound of tests/norm_hard_inputs.py, unchanged"""
    import norm_hard_inputs as nh
    case = sg.layer_norm_case(variant, *geometry, w_probes=probes)
    ratio = nh.error_ratio(case, LN_RUN[entry](case))
    print("%s planes %s: worst |err| / bound = %.3f" % (entry, sg.name((geometry, variant, probes)), ratio))
    _note(entry, "planes", ratio)
    assert ratio <= 1.0, (entry, geometry, variant, probes, ratio)


LINEAR_ALL = sg.LINEAR_GEOMETRIES + [sg.BIG_GEOMETRY]
PLANES = ([("linear_k128", g, v, c) for g in LINEAR_ALL for (v, c) in sg.PLANES]
          + [("conv1x1_nchw", g, v, c) for g in sg.CONV_GEOMETRIES for (v, c) in sg.PLANES])
RANGE = ([("linear_k128", g, r) for g in sg.LINEAR_GEOMETRIES for r in sg.RANGES]
         + [("conv1x1_nchw", g, r) for g in sg.CONV_GEOMETRIES for r in sg.RANGES])
RUN = {"linear_k128": run_linear, "conv1x1_nchw": run_conv}
BUILD_PLANES = {"linear_k128": sg.linear_planes, "conv1x1_nchw": sg.conv_planes}
BUILD_RANGE = {"linear_k128": sg.linear_range, "conv1x1_nchw": sg.conv_range}


def _check_ratio(entry, family, label, case, got):
    ratio = sg.ratio(case, got)
    print("%s %s %s: worst |err| / bound = %.3f" % (entry, family, label, ratio))
    _note(entry, family, ratio)
    assert ratio <= 1.0, (entry, family, label, ratio)


@pytest.mark.parametrize("entry,geometry,variant,cancel", PLANES, ids=sg.name)
def test_planes(entry, geometry, variant, cancel):
    case = BUILD_PLANES[entry](geometry, variant, cancel)
    _check_ratio(entry, "planes", sg.name((geometry, variant, cancel)), case, RUN[entry](case, geometry))


@pytest.mark.parametrize("variant,cancel", sg.PLANES, ids=sg.name)
def test_planes_multi(variant, cancel):
    cases = sg.multi_cases(variant, cancel)
    for s, (case, got) in enumerate(zip(cases, run_multi(cases))):
        _check_ratio("linear_k128_multi", "planes", "%s segment %d" % (sg.name((variant, cancel)), s), case, got)


@pytest.mark.parametrize("geometry", sg.FPN_GEOMETRIES, ids=sg.name)
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("cancel", [False, True])
def test_planes_fpn_stage(geometry, channels_last, cancel):
    case = sg.fpn_case(cancel, *geometry)
    _check_ratio("fpn_stage", "planes", sg.name((geometry, channels_last, cancel)), case, run_fpn(case, channels_last))


@pytest.mark.parametrize("entry,geometry,name", RANGE, ids=sg.name)
def test_range(entry, geometry, name):
    case = BUILD_RANGE[entry](geometry, name)
    _check_ratio(entry, "range", sg.name((geometry, name)), case, RUN[entry](case, geometry))


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("geometry", LINEAR_ALL, ids=sg.name)
def test_routing_linear(geometry, mirror):
    rows, n, relu, _, period = geometry
    case = sg.routing_case(mirror, rows, n, 128, relu, 0 if mirror else period)
    assert sg.routed_ok(case, run_linear(case)), (geometry, mirror)


def test_routing_multi():
    case, segments = sg.multi_routing()
    cases = [type(case)(**dict(vars(case), w=w, use_add=add)) for (w, add, _) in segments]
    for s, (got, (_, _, expect)) in enumerate(zip(run_multi(cases), segments)):
        assert np.array_equal(got, expect), s


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("geometry", sg.CONV_GEOMETRIES, ids=sg.name)
def test_routing_conv(geometry, mirror):
    K, H, W = geometry
    case = sg.routing_case(mirror, 2 * H * W, 128, K)
    assert sg.routed_ok(case, run_conv(case, geometry)), (geometry, mirror)


def _contained(label, hit, clean, bad):
    all_bad, others_same = sg.contained(hit, clean, bad)
    assert all_bad, "%s: a reached row has finite outputs (or the clean run has not)" % (label,)
    assert others_same, "%s: a row that no poisoned operand reaches differs from the clean run" % (label,)


@pytest.mark.parametrize("entry,geometry", [("linear_k128", g) for g in sg.LINEAR_GEOMETRIES]
                         + [("conv1x1_nchw", g) for g in sg.CONV_GEOMETRIES], ids=sg.name)
def test_containment(entry, geometry):
    case = BUILD_RANGE[entry](geometry, "x_small")
    x, xa, hit = sg.poisoned(case)
    _contained((entry, geometry), hit, RUN[entry](case, geometry), RUN[entry](case, geometry, x=x, x_add=xa))


def test_containment_in_the_large_case():
    """6280 rows x n = 1024 with the shared x_add: slots of 3 and 4 tiles, the paired-trip loop and its remainder"""
    case = sg.linear_planes(sg.BIG_GEOMETRY, "x3", False)
    x, xa, hit = sg.poisoned(case)
    assert hit.sum() == 2 + sg.BIG_IMAGES
    _contained(("linear_k128", sg.BIG_GEOMETRY), hit, run_linear(case), run_linear(case, x=x, x_add=xa))


def test_containment_multi():
    """three segments, add_x2 1 / 0 / 1: the +inf sits in x_add and reaches its row in every image -- in the segments that add"""
    cases = sg.multi_cases("x3", False)
    x, xa, hit = sg.poisoned(cases[0])
    in_x = hit & ~(np.arange(cases[0].rows) % cases[0].period == (cases[0].rows - 1) % cases[0].period)
    assert in_x.sum() == 2 and hit.sum() == 5
    for s, (clean, bad) in enumerate(zip(run_multi(cases), run_multi(cases, x=x, x_add=xa))):
        _contained(("linear_k128_multi", s), hit if cases[s].use_add else in_x, clean, bad)


@pytest.mark.parametrize("entry", ["linear_add_layer_norm", "linear_layer_norm", "ffn_layer_norm"])
def test_containment_in_front_of_layer_norm(entry):
    """A NaN, an inf and the largest finite fp32 in the GEMM operand x: the row is non-finite through the norm, every other row
    keeps its bits.  The FFN takes the NaN and the inf only: its hidden-layer fmaxf drops the NaN of W1 x and the row is
    non-finite through the residual x -- which the finite value is not."""
    if entry == "ffn_layer_norm":
        case, run = sg.ffn_case(1, "w3", (1,), 257, 96), run_ffn_layer_norm
    else:
        case, run = sg.layer_norm_case("w3", *sg.LAYER_NORM_GEOMETRIES[entry][-1], w_probes=(1,)), LN_RUN[entry]
    bad, hit = sg.poisoned_rows(case, "x", big=entry != "ffn_layer_norm")
    _contained((entry,), hit, run(case).cpu().numpy(), run(bad).cpu().numpy())


@pytest.mark.parametrize("geometry", sg.FPN_GEOMETRIES, ids=sg.name)
@pytest.mark.parametrize("channels_last", [False, True])
def test_containment_fpn_stage(geometry, channels_last):
    case = sg.fpn_case(False, *geometry)
    enc, hit = sg.fpn_poisoned(case)
    _contained(("fpn_stage", geometry, channels_last), hit, run_fpn(case, channels_last), run_fpn(case, channels_last, enc=enc))


def test_two_calls_give_the_same_bits():
    """None of these kernels uses atomics: the plain x3 case of every geometry, twice."""
    for entry, geometries in (("linear_k128", LINEAR_ALL), ("conv1x1_nchw", sg.CONV_GEOMETRIES)):
        for g in geometries:
            case = BUILD_PLANES[entry](g, "x3", False)
            a, b = RUN[entry](case, g), RUN[entry](case, g)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (entry, g)
    cases = sg.multi_cases("x3", False)
    for a, b in zip(run_multi(cases), run_multi(cases)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for g in sg.FPN_GEOMETRIES:
        case = sg.fpn_case(False, *g)
        a, b = run_fpn(case, True), run_fpn(case, True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), g


def child_main():
    """Body of the PCT_LIN_KERNEL=f32 child: linear_k128.hip on routing, containment and planes (bound of a recursive fp32 sum)."""
    assert os.environ.get("PCT_LIN_KERNEL") == "f32"
    worst = 0.0
    for g in LINEAR_ALL:
        rows, n, relu, _, period = g
        for mirror in (False, True):
            case = sg.routing_case(mirror, rows, n, 128, relu, 0 if mirror else period)
            assert sg.routed_ok(case, run_linear(case)), ("routing", g, mirror)
        for (v, c) in sg.PLANES:
            case = sg.linear_planes(g, v, c)
            got = run_linear(case).astype(np.float64)
            assert np.isfinite(got).all()
            bound = (case.K + 2) * sg.U * (np.abs(case.x_eff).astype(np.float64) @ np.abs(case.w).astype(np.float64).T) \
                + 2 * sg.U * np.abs(case.want)
            ratio = float((np.abs(got - case.want) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, ("planes", g, v, c, ratio)
    for g in sg.LINEAR_GEOMETRIES:
        case = sg.linear_range(g, "x_small")
        x, xa, hit = sg.poisoned(case, only_nan=True)
        _contained(("f32", g), hit, run_linear(case), run_linear(case, x=x, x_add=xa))
    print("worst |err| / bound  linear_k128[f32]   planes   %.3f" % worst)
    print("ok")


def test_linear_k128_on_the_fp32_mfma_kernel():
    """PCT_LIN_KERNEL=f32 routes linear_k128 to linear_k128.hip; the switch is read once per process, hence a fresh child (its own
    time limit, the parent's program is not replaced)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_split_gemm_hard_inputs_gpu as t\nt.child_main()\n"
            % (os.path.dirname(tests), tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PCT_LIN_KERNEL="f32"), capture_output=True,
                         text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), (out.stdout[-2000:], out.stderr[-2000:])

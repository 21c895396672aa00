"""GPU: every normalising kernel on the inputs of tests/norm_hard_inputs.py, against float64 of the plain formula on the
exact fp32 inputs, through the fused_ops wrappers (the `*_supported` predicate is asserted first and the wrappers' torch
fall-backs are made to raise, so no test passes on the library's kernels).

  entry                      kernel                                                     shapes
  add_layer_norm             add_layernorm.hip                                          cols 64/128/256, rows 7/1031, +-y
  linear_add_layer_norm      linear_k128_split.hip epilogue (linear_k128.hip under      rows 4099
                             PCT_LIN_KERNEL=f32, one child process)
  linear_layer_norm          linear_ln_split.hip                                        K 32/96/1024, rows 7/129
  ffn_layer_norm             ffn_fused_split.hip                                        F 32/96, rows 37/257, + row stride 160
  groupnorm_flatten          groupnorm_flatten.hip                                      16x16 / 32x32, groups 32/8, N = 2
  conv1x1_groupnorm_tokens   conv1x1_split.hip (tile records, finalize, apply)          K 32/256, 8x32 / 32x32, N = 2

Families and what is asserted (tests/norm_hard_inputs.py has the construction and the derivation of the bound):
  offset, eps_matters   |got - want| <= (n/2 + 16) u |gamma z| + 2u |want| per element; the worst ratio is printed
  constant              bit-exactly beta
  nonfinite             two launches, clean and poisoned: the poisoned sets come out entirely non-finite, every other
                        element has the bits of the clean run
and two calls on the offset case give the same bits for every entry.

Observed on the MI355X, worst |err| / bound over the cases of an entry (offset / eps_matters):
  add_layer_norm 0.489 / 0.476, linear_add_layer_norm 0.486 / 0.471 (the same under PCT_LIN_KERNEL=f32), linear_layer_norm
  0.457 / 0.417, ffn_layer_norm 0.454 / 0.442 (0.454 / 0.416 on strided rows), groupnorm_flatten 0.435 / 0.401,
  conv1x1_groupnorm_tokens 0.402 / 0.326.  The figures sit just under 1/2 because the worst element is one with gamma z near
  zero, where the only error is the rounding of the stored result (u |want| against 2u |want|).  Every constant set came
  out as beta bit for bit, every poisoned set entirely non-finite (the FFN's as well: fmaxf drops the NaN of the hidden
  layer, but the row is its own residual), and no clean set changed a bit next to a poisoned one.
Hand mutations on a scratch build (not committed), one per kernel file, were all caught: `+ eps` removed in
ffn_fused_split.hip failed all 31 FFN cases outside `nonfinite` (ratios 4.5e4 to 1.7e8; constant sets NaN); the mean taken
from red[..][row ^ 1] in linear_ln_split.hip failed all 48 linear_layer_norm cases (4.4e5 to 5.6e9; constant sets off beta,
poisoned rows partly finite); eps hard-coded to 1e-5 in add_layernorm.hip failed the 24 cases with eps = 1e-3 (9e5 to 3e6);
eps added behind the square root in linear_k128_split.hip failed offset and eps_matters (1e5 to 4e7); a one-pass variance in
gn_stats_kernel failed offset at all four geometries (1.7 to 319: the block-wide tree sum is kinder to E[x^2] than a
sequential one) and eps_matters with the offset; gn_finalize_kernel without the spread of the tile means failed offset (3.3 to
165) and eps_matters of conv1x1_groupnorm_tokens."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

import norm_hard_inputs as nh

pytestmark = pytest.mark.gpu

from pctrans_amd import fused_ops  # noqa: E402

ALL = [(e,) + c for e in nh.ENTRIES for c in nh.case_ids(e)]
GN_OFFSET, GN_TAIL = 7, 4            # groupnorm_flatten_into: token rows before / behind the level, NaN before and after
CONV_OFFSET, CONV_TAIL = 24, 16      # conv1x1_groupnorm_tokens_into: the same, filled with 7.0


@contextlib.contextmanager
def _kernel_only(*names):
    """The wrappers' fall-backs (fused_ops functions they call when their own kernel does not apply) raise."""
    def refuse(*args, **kwargs):
        raise AssertionError("the wrapper left its kernel for a fall-back")
    saved = {n: getattr(fused_ops, n) for n in names}
    for n in names:
        setattr(fused_ops, n, refuse)
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(fused_ops, n, f)


def _cuda(case):
    return {k: (None if v is None else v.cuda()) for k, v in case.inputs.items()}


def _norm(module, i):
    with torch.no_grad():
        module.weight.copy_(i["gamma"])
        module.bias.copy_(i["beta"])
    return module.cuda()


def _linear(weight, bias):
    lin = nn.Linear(weight.shape[1], weight.shape[0])
    with torch.no_grad():
        lin.weight.copy_(weight)
        lin.bias.copy_(bias)
    return lin.cuda()


def run_add_layer_norm(case):
    i = _cuda(case)
    ln = _norm(nn.LayerNorm(i["x"].shape[1], eps=case.eps), i)
    with torch.no_grad():
        assert fused_ops._fusable(i["x"], i["y"], ln.weight, ln.bias) and i["x"].shape[1] in (64, 128, 256)
        return fused_ops.add_layer_norm(i["x"], i["y"], ln)


def run_linear_add_layer_norm(case):
    i = _cuda(case)
    lin, ln = _linear(i["weight"], i["bias"]), _norm(nn.LayerNorm(128, eps=case.eps), i)
    with torch.no_grad(), _kernel_only("add_layer_norm"):
        assert fused_ops.linear_k128_supported(i["x"], lin.weight, lin.bias) and lin.out_features == 128
        return fused_ops.linear_add_layer_norm(i["x"], lin, i["residual"], ln)


def run_linear_layer_norm(case):
    i = _cuda(case)
    lin, ln = _linear(i["weight"], i["bias"]), _norm(nn.LayerNorm(128, eps=case.eps), i)
    with torch.no_grad(), _kernel_only("add_layer_norm"):
        assert fused_ops.linear_layer_norm_supported(i["x"], lin, i["residual"], ln)
        return fused_ops.linear_layer_norm(i["x"], lin, i["residual"], ln)


def run_ffn_layer_norm(case, row_stride=None):
    i = _cuda(case)
    l1, l2, ln = _linear(i["w1"], i["b1"]), _linear(i["w2"], i["b2"]), _norm(nn.LayerNorm(128, eps=case.eps), i)
    x = i["x"]
    if row_stride is not None:                       # rows that are a column slice of a wider tensor
        wide = torch.full((x.shape[0], row_stride), 5.0, device="cuda")
        wide[:, 16:144] = x
        x = wide[:, 16:144]
        assert x.stride(0) == row_stride and x.data_ptr() % 16 == 0
    with torch.no_grad(), _kernel_only("linear_layer_norm", "add_layer_norm"):
        assert fused_ops.ffn_layer_norm_supported(x, l1, l2, ln)
        return fused_ops.ffn_layer_norm(x, l1, l2, ln)


def run_groupnorm_flatten(case):
    i = _cuda(case)
    gn = _norm(nn.GroupNorm(case.groups, 128, eps=case.eps), i)
    N, _, H, W = i["x"].shape
    out = torch.full((N, GN_OFFSET + H * W + GN_TAIL, 128), float("nan"), device="cuda")
    with torch.no_grad():
        assert fused_ops.groupnorm_flatten_supported(i["x"], gn)
        fused_ops.groupnorm_flatten_into(i["x"], gn, out, GN_OFFSET)
    assert torch.isnan(out[:, :GN_OFFSET]).all() and torch.isnan(out[:, GN_OFFSET + H * W:]).all()    # nothing else touched
    return out[:, GN_OFFSET:GN_OFFSET + H * W].contiguous()


def run_conv1x1_groupnorm_tokens(case):
    from pctrans_amd.layers import Conv2d
    i = _cuda(case)
    N, K, H, W = i["x"].shape
    conv = Conv2d(K, 128, kernel_size=1)
    with torch.no_grad():
        conv.weight.copy_(i["weight"])
        conv.bias.copy_(i["bias"])
    conv, gn = conv.cuda(), _norm(nn.GroupNorm(32, 128, eps=case.eps), i)
    out = torch.full((N, CONV_OFFSET + H * W + CONV_TAIL, 128), 7.0, device="cuda")
    with torch.no_grad():
        assert fused_ops.conv1x1_groupnorm_tokens_supported(i["x"], conv, gn)
        fused_ops.conv1x1_groupnorm_tokens_into(i["x"], conv, gn, out, CONV_OFFSET)
    assert float((out[:, :CONV_OFFSET] - 7.0).abs().max()) == 0.0
    assert float((out[:, CONV_OFFSET + H * W:] - 7.0).abs().max()) == 0.0
    return out[:, CONV_OFFSET:CONV_OFFSET + H * W].contiguous()


RUNNERS = {"add_layer_norm": run_add_layer_norm, "linear_add_layer_norm": run_linear_add_layer_norm,
           "linear_layer_norm": run_linear_layer_norm, "ffn_layer_norm": run_ffn_layer_norm,
           "groupnorm_flatten": run_groupnorm_flatten, "conv1x1_groupnorm_tokens": run_conv1x1_groupnorm_tokens}


def check(label, case, run):
    """One case through `run` under its family's assertion; -> the error ratio (None where the comparison is exact)."""
    if case.family == "constant":
        got = run(case)
        assert nh.is_beta(case, got), label
        return None
    if case.family == "nonfinite":
        clean, poisoned = run(case.clean), run(case)
        all_bad, others_same = nh.nonfinite_ok(case, clean, poisoned)
        assert all_bad, "%s: a poisoned set has finite elements (or the clean run has not)" % label
        assert others_same, "%s: a set without non-finite input differs from the clean run" % label
        return None
    ratio = nh.error_ratio(case, run(case))
    print("%s: worst |err| / bound = %.3f" % (label, ratio))
    assert ratio <= 1.0, (label, ratio)
    return ratio


@pytest.mark.parametrize("entry,family,geometry,variant", ALL, ids=nh.case_name)
def test_kernel_on_hard_inputs(entry, family, geometry, variant):
    case = nh.build(entry, family, geometry, variant)
    check("%s %s" % (entry, nh.case_name((family, geometry, variant))), case, RUNNERS[entry])


@pytest.mark.parametrize("family", nh.FAMILIES)
def test_fused_ffn_on_strided_rows(family):
    """Rows 160 floats apart (a column slice of a wider tensor): the residual is read through the same stride."""
    variant = nh.variants(family)[-1]
    case = nh.build("ffn_layer_norm", family, (257, 32), variant)
    check("ffn_layer_norm stride 160 %s-%d" % (family, variant), case, lambda c: run_ffn_layer_norm(c, row_stride=160))


@pytest.mark.parametrize("entry", list(nh.ENTRIES))
def test_two_calls_give_the_same_bits(entry):
    """None of these kernels uses atomics: the offset case, twice."""
    for geometry in nh.ENTRIES[entry][1]:
        case = nh.build(entry, "offset", geometry)
        a, b = RUNNERS[entry](case), RUNNERS[entry](case)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (entry, geometry)


def child_main():
    """Body of the PCT_LIN_KERNEL=f32 child: every family of linear_add_layer_norm on the fp32-MFMA kernel's epilogue."""
    assert os.environ.get("PCT_LIN_KERNEL") == "f32"
    for family, geometry, variant in nh.case_ids("linear_add_layer_norm"):
        case = nh.build("linear_add_layer_norm", family, geometry, variant)
        check("linear_add_layer_norm[f32] %s" % nh.case_name((family, geometry, variant)), case, run_linear_add_layer_norm)
    print("ok")


def test_linear_add_layer_norm_on_the_fp32_mfma_kernel():
    """PCT_LIN_KERNEL=f32 routes the K = 128 entries to linear_k128.hip; the switch is read once per process, hence a
    fresh child (its own time limit, the parent's program is not replaced)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_norm_hard_inputs_gpu as t\nt.child_main()\n"
            % (os.path.dirname(tests), tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PCT_LIN_KERNEL="f32"), capture_output=True,
                         text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), (out.stdout[-2000:], out.stderr[-2000:])

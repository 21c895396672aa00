"""GPU: the differentiable fused MSDeformAttn front-end -- the C entry pct_ms_deform_attn_fused_backward_f32
(include/pctrans_hip_msda_train.h; pctrans_amd/csrc/msda_fused_backward.hip around the routed backward), the autograd Function of
pctrans_amd/msda_train.py and MSDeformAttn.train_front = "hip" -- against float64.

Entry vs the reference of tests/msda_fused_reference.py, per case and backward kernel (forced with pct_msda_set_bwd_kernel_choice,
asserted with pct_msda_last_bwd_kernel).  The bounds follow from tests/test_msda_bwd_col_gpu.py, which allows 2e-5 of a gradient's
magnitude (the 2^-21 fixed-point accumulators):
    grad_value      2e-5 * max(1, max|ref|)
    grad_offsets    per level and coordinate 2e-5 * max(1, max|gloc_ref|) / W_l (or H_l); samples within 1e-3 px of a cell boundary
                    are left out (grad_loc is discontinuous there) and are fewer than 1 %
    grad_logits     5e-5 * max(1, max|gw_ref|): an error e on every gw gives at most 2 w_j e <= 2 e, 1e-5 for the fp32 softmax
    a sample gated out (and not within 1e-3 px of the gate) has exactly zero grad_offsets
Every figure is printed before it is asserted; the unfused fp32 chain (torch-formed locations and weights,
ms_deform_attn_backward with the same kernel, torch autograd for the front) is measured against the same reference beside it.

Observed on the MI355X, worst error / bound (grad_value, grad_offsets, grad_logits); the unfused fp32 chain with the same kernel
gives the same figures to two digits, so no bound had to be replaced by that chain's:
    pyr3_shared    column 0.435 0.037 0.002    generic 0.019 0.039 0.002
    ragged_perimg  column 0.514 0.032 0.003    generic 0.028 0.032 0.003
    lq37_p8                                    generic 0.019 0.019 0.002
    peaked         column 0.200 0.032 0.002    generic 0.024 0.032 0.002
    far_offsets    column 0.242 0.034 0.004    generic 0.032 0.034 0.004
    win_pyr3       column 0.664 0.088 0.011    generic 0.104 0.085 0.011    windowed 0.604 0.088 0.011
    module: worst |hip - torch| / max(2 |torch - f64|, 5e-6 max|f64|) 0.07 (output_proj.weight); two-layer encoder 0.27
    (layers.1.self_attn.sampling_offsets.bias)
The five cases of 336 / 315 / 37 queries are too small for the windowed kernel (it declines calls of fewer than 32 768 records), so
win_pyr3 (one 64-32-16 image, 43 008 records) is the case that kernel runs; the repeatability test uses it for both kernels.
"""
import numpy as np
import pytest
import torch

import msda_fused_reference as R

pytestmark = pytest.mark.gpu

B_AUTO, B_WIN, B_GENERIC, B_COL = 0, 1, 2, 3
KERNEL = {B_AUTO: "auto", B_WIN: "windowed", B_GENERIC: "generic", B_COL: "column"}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pctrans_amd import _lib
    _lib.prepare_device(torch.device("cuda", torch.cuda.current_device()))
    return _lib.lib()


@pytest.fixture(scope="module")
def T():
    from pctrans_amd import msda_train
    return msda_train


class force:
    def __init__(self, lib, k):
        self.lib, self.k = lib, k

    def __enter__(self):
        self.lib.pct_msda_set_bwd_kernel_choice(self.k if self.k != B_AUTO else -1)

    def __exit__(self, *a):
        self.lib.pct_msda_set_bwd_kernel_choice(-1)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def operands(c, dtype=torch.float32):
    """value, shapes, starts, ref, offsets, logits on the device (ref with the batch expanded when the table is shared)."""
    N = c["dims"][0]
    ref = dev(c["ref"], dtype)
    return (dev(c["value"], dtype), dev(c["shapes"]), dev(c["starts"]), ref.expand(N, -1, -1, -1) if ref.shape[0] == 1 else ref,
            dev(c["offsets"], dtype), dev(c["logits"], dtype))


def covers(kernel, c):
    """Which backward kernel takes the case when forced (csrc/launchers.hpp: msda_col_covers; msda_backward_win.hip)."""
    N, S, M, D, L, Lq, P = c["dims"]
    geometry = D == 16 and P == 4 and 3 <= L <= 5
    if kernel == B_COL:
        return geometry and Lq == S
    if kernel == B_WIN:
        return geometry and N * Lq * M >= 32768
    return True


def torch_chain(value, shapes, starts, ref, offsets, logits, im2col_step=128):
    """The module's torch chain on the device, any float dtype: -> out, and the locations and weights it formed."""
    from pctrans_amd.pixel_decoder.ops.functions import MSDeformAttnFunction
    N, Lq, M, L, P, _ = offsets.shape
    w = torch.softmax(logits, -1).view(N, Lq, M, L, P)
    normalizer = torch.stack([shapes[..., 1], shapes[..., 0]], -1)
    loc = ref[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
    out = MSDeformAttnFunction.apply(value.contiguous(), shapes, starts, loc.contiguous(), w.contiguous(), im2col_step)
    return out, loc, w


def bounds(c, want):
    """name -> tolerance array (broadcastable) of the module docstring, from the reference alone."""
    wh = R.sizes_wh(c)
    return {"grad_value": 2e-5 * max(1.0, float(np.abs(want["grad_value"]).max())),
            "grad_offsets": 2e-5 * max(1.0, float(np.abs(want["gloc"]).max())) / wh[None, None, None, :, None, :],
            "grad_logits": 5e-5 * max(1.0, float(np.abs(want["gw"]).max()))}


def worst_ratios(got, c, want, tag):
    """Prints and returns name -> max |got - want| / bound, grad_offsets without the samples on a cell boundary."""
    tol, on_edge = bounds(c, want), R.edge_mask(c)
    assert on_edge.mean() < 0.01
    ratios = {}
    for name in ("grad_value", "grad_offsets", "grad_logits"):
        g = np.asarray(got[name], dtype=np.float64).reshape(want[name].shape)
        assert np.isfinite(g).all(), (tag, name)
        err = np.abs(g - want[name])
        if name == "grad_offsets":
            err = np.where(on_edge, 0.0, err)
        ratios[name] = float((err / tol[name]).max())
    print("%s: error / bound  grad_value %.3f  grad_offsets %.3f  grad_logits %.3f" % (
        tag, ratios["grad_value"], ratios["grad_offsets"], ratios["grad_logits"]))
    return ratios


def run_entry(T, lib, c, kernel, expect=None):
    value, shapes, starts, ref, offsets, logits = operands(c)
    with force(lib, kernel):
        gv, goff, glog = T.fused_backward(value, shapes, starts, ref, offsets, logits, dev(c["grad_out"]))
        torch.cuda.synchronize()
        ran = lib.pct_msda_last_bwd_kernel()
    assert ran == (kernel if expect is None else expect), (KERNEL[kernel], ran)
    assert gv.shape == value.shape and goff.shape == offsets.shape and glog.shape == logits.shape
    return {"grad_value": gv.cpu().numpy(), "grad_offsets": goff.cpu().numpy(), "grad_logits": glog.cpu().numpy()}


def run_unfused(lib, c, kernel):
    """The unfused fp32 chain with the same backward kernel: torch front, ms_deform_attn_backward, torch autograd."""
    value, shapes, starts, ref, offsets, logits = operands(c)
    value.requires_grad_(), offsets.requires_grad_(), logits.requires_grad_()
    with force(lib, kernel):
        out, _, _ = torch_chain(value, shapes, starts, ref, offsets, logits)
        out.backward(dev(c["grad_out"]))
        torch.cuda.synchronize()
    return {"grad_value": value.grad.cpu().numpy(), "grad_offsets": offsets.grad.cpu().numpy(), "grad_logits": logits.grad.cpu().numpy()}


ENTRY_RUNS = [(name, k) for name in R.CASES for k in (B_COL, B_WIN, B_GENERIC) if covers(k, R.make(name))]


@pytest.mark.parametrize("name,kernel", ENTRY_RUNS, ids=["%s-%s" % (n, KERNEL[k]) for n, k in ENTRY_RUNS])
def test_entry_vs_reference(T, lib, name, kernel):
    c = R.make(name)
    want = R.backward(c)
    got = run_entry(T, lib, c, kernel)
    ratios = worst_ratios(got, c, want, "%s %s fused" % (name, KERNEL[kernel]))
    worst_ratios(run_unfused(lib, c, kernel), c, want, "%s %s unfused fp32 chain" % (name, KERNEL[kernel]))
    gated = R.gated_out(c) & ~R.edge_mask(c)[..., 0]
    assert gated.any() and np.all(got["grad_offsets"][gated] == 0)
    assert all(r <= 1.0 for r in ratios.values()), ratios


def test_every_backward_kernel_serves_the_entry():
    assert {k for _, k in ENTRY_RUNS} == {B_COL, B_WIN, B_GENERIC}
    assert {n for n, _ in ENTRY_RUNS} == set(R.CASES)


def test_entry_auto_routes_as_the_unfused_backward(T, lib):
    """`auto`: the column kernel from 32 768 records of the pyramid's own pixels on, the generic kernel on the small cases."""
    for name, expect in (("win_pyr3", B_COL), ("pyr3_shared", B_GENERIC)):
        c = R.make(name)
        got = run_entry(T, lib, c, B_AUTO, expect=expect)
        ratios = worst_ratios(got, c, R.backward(c), "%s auto (%s)" % (name, KERNEL[expect]))
        assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("kernel", [B_COL, B_WIN], ids=["column", "windowed"])
def test_entry_is_bitwise_repeatable_in_offsets_and_logits(T, lib, kernel):
    """Both kernels form a sample's location and weight gradients without atomics (the column kernel from integer LDS sums and
    per-lane arithmetic, the windowed kernel per lane and by DPP sums over its four-lane group in a fixed order; float atomics
    only flush grad_value), and expand and fold have no atomics at all: two calls on the same operands give the same bits."""
    c = R.make("win_pyr3")
    a, b = run_entry(T, lib, c, kernel), run_entry(T, lib, c, kernel)
    np.testing.assert_array_equal(a["grad_offsets"], b["grad_offsets"])
    np.testing.assert_array_equal(a["grad_logits"], b["grad_logits"])
    scale = float(np.abs(a["grad_value"]).max())
    assert float(np.abs(a["grad_value"] - b["grad_value"]).max()) <= 1e-5 * scale


# ---------------------------------------------------------------- the autograd Function
def f64_chain(c, go):
    """float64 torch chain on the device: loss, and the gradients of value, offsets, logits, loc and w."""
    value, shapes, starts, ref, offsets, logits = operands(c, torch.float64)
    value.requires_grad_(), offsets.requires_grad_(), logits.requires_grad_()
    out, loc, w = torch_chain(value, shapes, starts, ref, offsets, logits)
    loc.retain_grad(), w.retain_grad()
    loss = (out * go.double()).sum()
    loss.backward()
    return out.detach(), loss.detach(), {"grad_value": value.grad.cpu().numpy(), "grad_offsets": offsets.grad.cpu().numpy(),
                                         "grad_logits": logits.grad.cpu().numpy(), "gloc": loc.grad.cpu().numpy(),
                                         "gw": w.grad.cpu().numpy()}


@pytest.fixture(scope="module")
def pyr3_f64():
    c = R.make("pyr3_shared")
    return (c,) + f64_chain(c, dev(c["grad_out"]))


def test_function_loss_and_gradients_vs_float64_chain(T, lib, pyr3_f64):
    from pctrans_amd import MultiScaleDeformableAttention as MSDA
    c, out64, loss64, want = pyr3_f64
    value, shapes, starts, ref, offsets, logits = operands(c)
    value.requires_grad_(), offsets.requires_grad_(), logits.requires_grad_()
    out = T.ms_deform_attn_fused_train(value, shapes, starts, ref, offsets, logits)
    with torch.no_grad():                                       # a training forward has the eval forward's bits
        assert torch.equal(out, MSDA.ms_deform_attn_fused_forward(value, shapes, starts, ref, offsets, logits))
    go = dev(c["grad_out"])
    loss = (out * go).sum()
    loss.backward()
    torch.cuda.synchronize()
    # the forward's tolerance: test_msda_gpu.py's 2e-5 of the magnitude for fp32 (its exp2 / rcp front-end included)
    assert float((out.detach().double() - out64).abs().max()) <= 2e-5 * max(1.0, float(out64.abs().max()))
    terms = float((out64 * go.double()).abs().sum())
    print("loss %.6f vs %.6f (sum of |terms| %.1f)" % (float(loss), float(loss64), terms))
    assert abs(float(loss) - float(loss64)) <= 2e-5 * terms
    got = {"grad_value": value.grad.cpu().numpy(), "grad_offsets": offsets.grad.cpu().numpy(), "grad_logits": logits.grad.cpu().numpy()}
    ratios = worst_ratios(got, c, want, "Function vs float64 chain on the device")
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (False, False, True), (True, False, True)],
                         ids=["value", "offsets", "logits", "value+logits"])
def test_function_honours_needs_input_grad(T, lib, pyr3_f64, need):
    """Inputs that need no gradient get none; the others get the full call's.  With only grad_value wanted the fold's results are
    dropped unread -- grad_value is the routed backward's own and matches as before."""
    c, _, _, want = pyr3_f64
    value, shapes, starts, ref, offsets, logits = operands(c)
    ts = (value, offsets, logits)
    for t, n in zip(ts, need):
        t.requires_grad_(n)
    out = T.ms_deform_attn_fused_train(value, shapes, starts, ref, offsets, logits)
    out.backward(dev(c["grad_out"]))
    torch.cuda.synchronize()
    tol, on_edge = bounds(c, want), R.edge_mask(c)
    for t, n, name in zip(ts, need, ("grad_value", "grad_offsets", "grad_logits")):
        assert (t.grad is not None) == n, name
        if n:
            err = np.abs(t.grad.cpu().numpy().astype(np.float64) - want[name])
            if name == "grad_offsets":
                err = np.where(on_edge, 0.0, err)
            assert float((err / tol[name]).max()) <= 1.0, name


def test_function_takes_a_non_contiguous_grad_output(T, lib, pyr3_f64):
    c, _, _, want = pyr3_f64
    N, S, M, D, L, Lq, P = c["dims"]
    value, shapes, starts, ref, offsets, logits = operands(c)
    value.requires_grad_(), offsets.requires_grad_(), logits.requires_grad_()
    out = T.ms_deform_attn_fused_train(value, shapes, starts, ref, offsets, logits)
    go = torch.zeros((N, Lq, 2 * M * D), device="cuda")[:, :, ::2]
    go.copy_(dev(c["grad_out"]))
    assert not go.is_contiguous()
    out.backward(go)
    torch.cuda.synchronize()
    got = {"grad_value": value.grad.cpu().numpy(), "grad_offsets": offsets.grad.cpu().numpy(), "grad_logits": logits.grad.cpu().numpy()}
    ratios = worst_ratios(got, c, want, "non-contiguous grad_output")
    assert all(r <= 1.0 for r in ratios.values()), ratios


def test_covered_and_function_refusals_on_the_device(T, lib):
    c = R.make("pyr3_shared")
    value, shapes, starts, ref, offsets, logits = operands(c)
    assert T.covered(value, ref, offsets, logits)
    assert T.covered(value, ref[:1], offsets, logits)                                        # one table for the batch
    assert not T.covered(value.cpu(), ref.cpu(), offsets.cpu(), logits.cpu())
    assert not T.covered(value.double(), ref.double(), offsets.double(), logits.double())
    assert not T.covered(value, torch.cat([ref, ref], -1), offsets, logits)                  # 4-d reference points
    assert not T.covered(value, ref.clone().requires_grad_(), offsets, logits)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not T.covered(value, ref, offsets, logits)
        with pytest.raises(RuntimeError, match="covered"):
            T.ms_deform_attn_fused_train(value, shapes, starts, ref, offsets, logits)
    with pytest.raises(RuntimeError, match="covered"):
        T.ms_deform_attn_fused_train(value.double(), shapes, starts, ref.double(), offsets.double(), logits.double())
    empty = T.fused_backward(value, shapes, starts, ref[:, :0], offsets[:, :0], logits[:, :0], dev(c["grad_out"])[:, :0])
    assert float(empty[0].abs().max()) == 0 and empty[1].numel() == 0 == empty[2].numel()


# ---------------------------------------------------------------- module and encoder
def value_rule(name, hip, torch32, f64, fails, worst):
    """|hip - torch| <= max(2 |torch - f64|, 5e-6 max|f64|): the all-on step test's rule (test_train_step_all_on_gpu.py)."""
    err = float((hip.double() - torch32.double()).abs().max())
    yerr = float((torch32.double() - f64).abs().max())
    top = float(f64.abs().max())
    bound = max(2.0 * yerr, 5e-6 * top)
    worst[name] = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    if not (np.isfinite(err) and err <= bound):
        fails.append("%s: |hip - torch| %.3e > %.3e (|torch - f64| %.3e, max|f64| %.3e)" % (name, err, bound, yerr, top))


class Spies:
    """Counts the calls of msda_train.fused_backward and of MSDeformAttnFunction.backward."""

    def __init__(self, monkeypatch):
        from pctrans_amd import msda_train
        from pctrans_amd.pixel_decoder.ops.functions import MSDeformAttnFunction
        self.fused = self.unfused = 0
        real_fused, real_unfused = msda_train.fused_backward, MSDeformAttnFunction.backward

        def fused(*a, **k):
            self.fused += 1
            return real_fused(*a, **k)

        def unfused(ctx, *grads):
            self.unfused += 1
            return real_unfused(ctx, *grads)

        monkeypatch.setattr(msda_train, "fused_backward", fused)
        monkeypatch.setattr(MSDeformAttnFunction, "backward", staticmethod(unfused))

    def take(self):
        r, self.fused, self.unfused = (self.fused, self.unfused), 0, 0
        return r


def make_module(dtype=torch.float32):
    from pctrans_amd.pixel_decoder.ops.modules import MSDeformAttn
    torch.manual_seed(11)
    m = MSDeformAttn(128, 3, 8, 4)
    with torch.no_grad():                              # the offsets / weights Linears start with zero weights: give them some
        m.sampling_offsets.weight.normal_(0, 0.05)
        m.attention_weights.weight.normal_(0, 0.3)
    return m.cuda().to(dtype).train()


def module_run(front, dtype, c, src, grad, pad, spies=None, autocast=False, ref_grad=False):
    """-> [out, input gradient, parameter gradients by name] and the spies' (fused, unfused) counts."""
    m = make_module(dtype)
    m.train_front = front
    x = src.to(dtype).clone().requires_grad_()
    N = c["dims"][0]
    ref = dev(c["ref"], dtype).expand(N, -1, -1, -1)
    if ref_grad:
        ref = ref.clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = m(x, ref, x, dev(c["shapes"]), dev(c["starts"]), pad)
    out.backward(grad.to(out.dtype))
    torch.cuda.synchronize()
    res = {"out": out.detach(), "grad input": x.grad}
    res.update({"grad " + n: p.grad for n, p in m.named_parameters()})
    return res, (spies.take() if spies is not None else None)


@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "padding_mask"])
def test_module_hip_front_vs_torch_chain(lib, monkeypatch, mask):
    c = R.make("pyr3_shared")
    N, S, M, D, L, Lq, P = c["dims"]
    rng = np.random.RandomState(21)
    src, grad = dev(rng.standard_normal((N, S, 128)).astype(np.float32)), dev(rng.standard_normal((N, S, 128)).astype(np.float32))
    pad = None
    if mask:
        pad = torch.zeros((N, S), dtype=torch.bool, device="cuda")
        pad[1, 300:] = True
        pad[0, 5:9] = True
    spies = Spies(monkeypatch)
    hip, n_hip = module_run("hip", torch.float32, c, src, grad, pad, spies)
    tor, n_tor = module_run("torch", torch.float32, c, src, grad, pad, spies)
    f64, _ = module_run("torch", torch.float64, c, src, grad, pad, spies)
    assert n_hip == (1, 0) and n_tor == (0, 1), (n_hip, n_tor)
    assert hip.keys() == tor.keys() == f64.keys() and len(hip) == 10 and all(v is not None for v in hip.values())
    fails, worst = [], {}
    for name in tor:
        value_rule(name, hip[name], tor[name], f64[name].double(), fails, worst)
    print("module (%s): worst |hip - torch| / bound %.3f (%s)" % ("mask" if mask else "no mask", max(worst.values()),
                                                                max(worst, key=worst.get)))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("how", ["autocast", "reference_points_need_a_gradient", "no_grad"])
def test_module_keeps_the_torch_chain_outside_covered(lib, monkeypatch, how):
    c = R.make("pyr3_shared")
    N, S, M, D, L, Lq, P = c["dims"]
    rng = np.random.RandomState(22)
    src, grad = dev(rng.standard_normal((N, S, 128)).astype(np.float32)), dev(rng.standard_normal((N, S, 128)).astype(np.float32))
    spies = Spies(monkeypatch)
    if how == "no_grad":
        m = make_module()
        m.train_front = "hip"
        with torch.no_grad():
            a = m(src, dev(c["ref"]).expand(N, -1, -1, -1), src, dev(c["shapes"]), dev(c["starts"]))
            m.train_front = "torch"
            b = m(src, dev(c["ref"]).expand(N, -1, -1, -1), src, dev(c["shapes"]), dev(c["starts"]))
        assert torch.equal(a, b) and spies.take() == (0, 0)
        return
    kw = dict(autocast=True) if how == "autocast" else dict(ref_grad=True)
    hip, n_hip = module_run("hip", torch.float32, c, src, grad, None, spies, **kw)
    tor, n_tor = module_run("torch", torch.float32, c, src, grad, None, spies, **kw)
    assert n_hip == (0, 1) == n_tor
    assert torch.equal(hip["out"], tor["out"])                  # the same chain
    for name in tor:
        assert bool(torch.isfinite(hip[name]).all()), name
        if how != "autocast":   # grad_value comes from float atomics: equal to their noise, not bit for bit (and under autocast a
            # bf16 rounding of it may fall either way)
            assert float((hip[name].double() - tor[name].double()).abs().max()) <= 1e-4 * max(1.0, float(tor[name].double().abs().max())), name


@pytest.mark.parametrize("input_grad", [True, False], ids=["input_grad", "parameters_only"])
def test_two_layer_encoder_hip_front_vs_torch_chain(lib, monkeypatch, input_grad):
    """Two encoder layers, dropout 0, train mode, ragged maps with per-image valid ratios (one reference table per image).
    Without an input gradient the first layer enters through forward_add_norm (its input requires no gradient)."""
    from pctrans_amd.pixel_decoder.msdeformattn import MSDeformAttnTransformerEncoder, MSDeformAttnTransformerEncoderLayer
    c = R.make("ragged_perimg")
    N, S, M, D, L, Lq, P = c["dims"]
    rng = np.random.RandomState(23)
    src = dev(rng.standard_normal((N, S, 128)).astype(np.float32))
    pos = dev(rng.standard_normal((1, S, 128)).astype(np.float32))
    grad = dev(rng.standard_normal((N, S, 128)).astype(np.float32))
    ratios = dev((0.8 + 0.2 * rng.random_sample((N, L, 2))).astype(np.float32))
    spies = Spies(monkeypatch)

    def run(front, dtype):
        torch.manual_seed(12)
        enc = MSDeformAttnTransformerEncoder(MSDeformAttnTransformerEncoderLayer(128, 256, 0.0, "relu", L, M, P), 2)
        with torch.no_grad():
            for layer in enc.layers:
                layer.self_attn.sampling_offsets.weight.normal_(0, 0.05)
                layer.self_attn.attention_weights.weight.normal_(0, 0.3)
        enc = enc.cuda().to(dtype).train()
        for layer in enc.layers:
            layer.self_attn.train_front = front
        x = src.to(dtype).clone().requires_grad_(input_grad)
        out = enc(x, dev(c["shapes"]), dev(c["starts"]), ratios.to(dtype), pos.to(dtype))
        out.backward(grad.to(dtype))
        torch.cuda.synchronize()
        res = {"out": out.detach()}
        if input_grad:
            res["grad input"] = x.grad
        res.update({"grad " + n: p.grad for n, p in enc.named_parameters()})
        return res, spies.take()

    hip, n_hip = run("hip", torch.float32)
    tor, n_tor = run("torch", torch.float32)
    f64, _ = run("torch", torch.float64)
    assert n_hip == (2, 0) and n_tor == (0, 2), (n_hip, n_tor)
    assert hip.keys() == tor.keys() == f64.keys() and all(v is not None for v in hip.values())
    fails, worst = [], {}
    for name in tor:
        value_rule(name, hip[name], tor[name], f64[name].double(), fails, worst)
    print("encoder (%s): worst |hip - torch| / bound %.3f (%s)" % ("input grad" if input_grad else "parameters only",
                                                                  max(worst.values()), max(worst, key=worst.get)))
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- HIP graph
def test_function_replays_from_a_hip_graph(T, lib):
    """Forward + backward of the Function captured on a side stream after prepare_device: three replays against the eager result,
    with the tolerance of test_msda_bwd_col_gpu.py::test_backward_replays_from_a_hip_graph for kernels that are not the column
    kernel (1e-5 of the magnitude; grad_value comes from float atomics), the forward bit for bit."""
    c = R.make("pyr3_shared")
    value, shapes, starts, ref, offsets, logits = operands(c)
    value.requires_grad_(), offsets.requires_grad_(), logits.requires_grad_()
    go = dev(c["grad_out"])

    def step():
        out = T.ms_deform_attn_fused_train(value, shapes, starts, ref, offsets, logits)
        return (out,) + torch.autograd.grad(out, (value, offsets, logits), go)

    eager = [t.detach().clone() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    for _ in range(3):
        for t in outs:
            t.detach().fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].detach(), eager[0])
        for got, want in zip(outs[1:], eager[1:]):
            assert float((got - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))

"""CPU: pins the float64 MSDeformAttn backward of tests/callsite_reference.py, which test_callsite_training_gpu.py holds
the kernels to: against the golden gradients generated from the reference's own autograd, against torch autograd through
ms_deform_attn_core_pytorch away from cell boundaries, and -- on the init-state geometry, where samples sit on pixel
centres -- against the C oracle's float64 backward, whose derivative must be one of the two one-sided candidates."""
import numpy as np
import pytest
import torch

import callsite_reference as ref
from msda_cases import make_case
from oracle import msda_oracle as orc


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _run(c, go, dtype=torch.float64, delta=1e-4):
    return ref.msda_backward(_t(c["value"]), _t(c["shapes"]), _t(c["starts"]), _t(c["loc"]), _t(c["attn"]), _t(go),
                             dtype=dtype, delta=delta)


def _loc_err(got, cands):
    """|got - nearest candidate| per coordinate"""
    got = torch.as_tensor(got, dtype=torch.float64)
    return (got[..., None] - cands).abs().min(-1).values


@pytest.mark.parametrize("name", ["grad_small_f64", "grad_head_geom_f32", "fwd_oddD_f64"])
def test_backward_reference_matches_the_golden_gradients(golden, name):
    g = golden(name)
    gv, gl, ga = _run(g, g["grad_out"])
    rel = 1e-12 if g["value"].dtype == np.float64 else 2e-6           # (the fp32 fixtures carry fp32 rounding)
    tol = lambda w: rel * max(1.0, float(np.abs(w).max()))
    np.testing.assert_allclose(gv.numpy(), g["grad_value"], rtol=0, atol=tol(g["grad_value"]))
    np.testing.assert_allclose(ga.numpy(), g["grad_attn"], rtol=0, atol=tol(g["grad_attn"]))
    assert float(_loc_err(g["grad_loc"], gl).max()) <= tol(g["grad_loc"])


def test_backward_reference_matches_torch_autograd_away_from_boundaries():
    from pctrans_amd.pixel_decoder.ops.functions import ms_deform_attn_core_pytorch
    shapes = [(6, 9), (3, 5), (2, 2)]
    c = make_case(seed=11, N=2, M=3, D=5, Lq=7, P=3, shapes=shapes, dtype=np.float64, lo=-0.1, hi=1.1)
    go = np.random.RandomState(12).standard_normal((2, 7, 15))
    v, loc, a = (_t(c[k]).requires_grad_() for k in ("value", "loc", "attn"))
    ms_deform_attn_core_pytorch(v, _t(c["shapes"]), loc, a).backward(_t(go))
    gv, gl, ga = _run(c, go)
    xy = ref.pixel_coords(_t(c["loc"]), _t(c["shapes"]))
    away = (xy - xy.round()).abs() > 1e-6
    assert away.all()                                                 # (uniform locations: no sample on a boundary)
    assert torch.equal(gl[..., 0], gl[..., 1])                        # one candidate everywhere
    torch.testing.assert_close(gv, v.grad, rtol=0, atol=1e-12)
    torch.testing.assert_close(ga, a.grad, rtol=0, atol=1e-12)
    torch.testing.assert_close(gl[..., 0], loc.grad, rtol=0, atol=1e-11)


def test_c_oracle_backward_is_one_of_the_candidates_at_the_init_state():
    """Init state: reference points at pixel centres, whole-pixel offsets -- every sample on its query's level sits on a
    texel, every coordinate on an integer (and some on the gate at -1 or H).  The oracle's float64 derivative must be one
    of the candidates; the candidates differ at a share of the coordinates."""
    shapes = [(8, 8), (4, 6), (2, 3)]
    S = sum(h * w for h, w in shapes)
    c = make_case(seed=21, N=1, M=8, D=4, Lq=S, P=4, shapes=shapes, init_like=True)
    go = np.random.RandomState(22).standard_normal((1, S, 8 * 4)).astype(np.float32)
    c64 = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in c.items()}
    wv, wl, wa = orc.backward(c64["value"], c64["shapes"], c64["starts"], c64["loc"], c64["attn"], go.astype(np.float64))
    gv, gl, ga = _run(c, go)
    np.testing.assert_allclose(gv.numpy(), wv, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ga.numpy(), wa, rtol=0, atol=1e-12)
    assert float(_loc_err(wl, gl).max()) <= 1e-11
    two = (gl[..., 0] != gl[..., 1]).double().mean()
    assert 0.1 < float(two) < 1.0, float(two)
    # the plain derivative (delta = 0) is always one of the candidates, in float64 and in float32
    for dt, tol in ((torch.float64, 1e-12), (torch.float32, 1e-4)):
        plain = _run(c, go, dtype=dt, delta=0)[1]
        assert torch.equal(plain[..., 0], plain[..., 1])
        assert float(_loc_err(plain[..., 0], gl).max()) <= tol


def test_candidates_at_the_gate():
    """A sample on the gate (y = H exactly, y = -1 exactly): the plain derivative is 0 (gated out), the inside side is
    H * (0 - v[H-1]) resp. H * (v[0] - 0), and the candidates hold both."""
    H, W = 4, 4
    value = torch.arange(1.0, 17.0, dtype=torch.float64).reshape(1, 16, 1, 1)
    shapes, starts = torch.tensor([[H, W]]), torch.tensor([0])
    attn = torch.ones(1, 2, 1, 1, 1, dtype=torch.float64)
    loc = torch.tensor([[[[[[1.5 / W, (H + 0.5) / H]]]]], [[[[[1.5 / W, -0.5 / H]]]]]], dtype=torch.float64)
    loc = loc.reshape(1, 2, 1, 1, 1, 2)                                # x = 1, y = H and x = 1, y = -1
    go = torch.ones(1, 2, 1, dtype=torch.float64)
    gv, gl, ga = ref.msda_backward(value, shapes, starts, loc, attn, go)
    assert float(gv.abs().max()) == 0 and float(ga.abs().max()) == 0
    assert sorted(gl[0, 0, 0, 0, 0, 1].tolist()) == [-H * float(value[0, (H - 1) * W + 1]), 0.0]
    assert sorted(gl[0, 1, 0, 0, 0, 1].tolist()) == [0.0, H * float(value[0, 1])]
    assert gl[0, :, 0, 0, 0, 0].abs().max() == 0                     # x: gated out on both sides of y's cell

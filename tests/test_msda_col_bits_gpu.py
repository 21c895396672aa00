"""The three pyramid-column MSDeformAttn kernels (csrc/msda_forward_col.hip, msda_forward_col16.hip, msda_backward_col.hip)
bit for bit: SHA-256 digests of their outputs on the seeded cases of test_msda_col_gpu.py / test_msda_bwd_col_gpu.py, recorded
on an MI355X with the kernels that each carried their own copy of the column grid, the lane slots, the cell tables, the item
decode, the XCD chunking, the forward kernels' two-ahead work queue and the quad-cooperative record fetch.  Stating those once
(msda_col_common.hpp; the phase planner and the backward's one-ahead queue stay in the kernels) must leave every output bit as
it was: a changed item order, slot or table entry moves a query to another lane, a changed phase plan a level to another
phase, and either shows here, where the tolerance tests would let a reordered sum pass.

Every call is forced onto the column kernel and `pct_msda_last_kernel` / `pct_msda_last_bwd_kernel` must say that it ran.

Forward, fp32, plain op: one phase, two phases (early second phase), global-memory levels, locations off the map, a level
narrower than the grid, 5 levels, levels fine to coarse, 4 heads, 1 head (the last-head branch of the decode), flat columns (no
tables) and maps wider than the 16-bit box corners.  Fused front end: a 4-level and a 3-level case as
test_fused_front_end_on_the_column_kernel builds them.  16-bit kernel: fp16 and bf16, 8 and 4 points, 5 / 4 / 3 levels, 3 heads,
flat columns.

Backward: grad_sampling_loc and grad_attn_weight, which are plain stores of sums formed in a fixed order (every case below gave
the same digest on two launches when it was recorded).  grad_value is accumulated with float atomics, is not bit-reproducible
and stays with the tolerance tests."""
import hashlib

import numpy as np
import pytest
import torch

from msda_cases import make_case, pixel_centres, starts_of
from test_msda_bwd_col_gpu import B_COL, BWD_COL_CASES, grad_out_for, run_bwd
from test_msda_col_gpu import COL16_CASES, COL_CASES, K_COL, P1, P2, _fused_case, dev, force, n_px

pytestmark = pytest.mark.gpu

FWD_IDS = ["col_P2_init_like", "col_P2_model_sigma2", "col_P2_sigma12", "col_P1_edges", "col_tiny_top_level", "col_L5",
           "col_levels_fine_to_coarse", "col_M4", "col_M1_wide_strip", "col_flat_columns_long_strip",
           "col_wider_than_the_box_corners"]
FUSED_CASES = [("fused_L4_P2_pixel_ref", P2, 1, True, 2.0, True), ("fused_L3_P1_pixel_ref", P1, 2, False, 1.0, True)]
C16_IDS = ["c16_P8_L5_model", "c16_P8_L4_init_like", "c16_P4_L4_model", "c16_P8_M3_heads", "c16_P4_flat_columns_long_strip"]
C16_DTYPES = [("f16", torch.float16), ("bf16", torch.bfloat16)]
BWD_IDS = [i for i in FWD_IDS if i in [c[0] for c in BWD_COL_CASES]]
BWD_STRIPS = [("long_strip", [(1, 15000), (1, 30000), (1, 60000)]),
              ("wider_than_the_box_corners", [(1, 17500), (1, 35000), (1, 70000)])]

DIGESTS = {
    "bwd_col_L5": "6a5e8d446eb543fc012e3399552e15ba3d432b123befb814ffe39864917aa692",
    "bwd_col_M1_wide_strip": "e00864224e70b91189c6c887173b86c5f43f9d4a38999fa9c6484b1a01862410",
    "bwd_col_M4": "f1811ecd54d61efa0ea9d07a0f8fe1ac594242308a9184bb9055c75c0922d27e",
    "bwd_col_P1_edges": "9a2deb94f8c4c301cfc4d593359d845f1a2c1931164c7e2427ded21164a7cc6d",
    "bwd_col_P2_init_like": "80bcbb0d164289ab78717fbfa6bb55dadbc7f9aa3de8e6a51fdcd402b148ac4c",
    "bwd_col_P2_model_sigma2": "b26171658c60afbba641385f23cdbe95c5f85e3a836c036680359b1ad79b83df",
    "bwd_col_P2_sigma12": "98346a52ea66f5aba6891830f8634708d495bcbd4d6c783e4cd2e5af4526ba58",
    "bwd_col_levels_fine_to_coarse": "d9665a90a9266e65854552565b57c173560692888a21b679ffd70ee55604e85a",
    "bwd_col_tiny_top_level": "616a2d71609541a370ae60c7c018430ebc83fc9618964509e3a3dd14960b9c54",
    "bwd_strip_long_strip": "5dbe6399719fdf755b5844afb053ddfd655e69ff2350bd512ad1e4f81883d440",
    "bwd_strip_wider_than_the_box_corners": "c139bdb01495fd125550918785df5cfeb2eeb52f0b59ce68d55da9c5d29235f3",
    "c16_P4_L4_model_bf16": "0dc8524895e839b83d325a6e0093c37b57a5fb14b5bd53dcfa812a9a7be940f6",
    "c16_P4_L4_model_f16": "10858f779da113d6f8d3df4099984dd27060b8b35db1c46188d2aebfda9c7d5b",
    "c16_P4_flat_columns_long_strip_bf16": "e1708a764b94f356bd21d332097d9e7660d0779995b12b449a3c6e6476ba5c54",
    "c16_P4_flat_columns_long_strip_f16": "8425bb1ca1c8e0007eed573e0dbe49f66fcdd90e55dc0ede1e9a7b1706c5c820",
    "c16_P8_L4_init_like_bf16": "919c15fb54384f754875771dfe7252f7f3e039cc06fdc742191f67cc48376793",
    "c16_P8_L4_init_like_f16": "daf6abe76f62bfb6c505f2d3851808223f2eec10e3e174b48907b81bc29a52cd",
    "c16_P8_L5_model_bf16": "9cf3c481e068c20f2c3d837800c905f58286fb2d23d3a05852ba85fe7f93187d",
    "c16_P8_L5_model_f16": "0e015addacb0743b4fb5142c6f8a390fc99fb65f821ae9a20e3aef399e549265",
    "c16_P8_M3_heads_bf16": "16101d833936f2a82d00c0037861d13d6cce4d6dd446edf016f489869738f932",
    "c16_P8_M3_heads_f16": "6dcfd0da580da6fe44fda7a213184d45c1d2915ce2d9c5e0d01e5b8f6772d779",
    "fused_L3_P1_pixel_ref": "55e47dca79241aeb19c7f51b534408b475760a44b0c37ebd01274f98ad2bd78d",
    "fused_L4_P2_pixel_ref": "c4775f5416566811e7ac308b1a14f62ddfe54fcd897f3ecc36771f3e4d9bb22a",
    "fwd_col_L5": "65dc5d02c69db538d4c22b671c8aad6562385d7a9d7b1f2dbf09759356922930",
    "fwd_col_M1_wide_strip": "22d21a797bde7f016ea42c0a30f2887eb7d8ea258e667666ef2d54870f456c4a",
    "fwd_col_M4": "c430de335964781c6c70bca01e0046971d3582fb69c89ff902ba927981a0dfdf",
    "fwd_col_P1_edges": "0ed38dcc77eb8041456f985c8601a36209adc874240d0dc0e90ecf99225cf6e9",
    "fwd_col_P2_init_like": "d8f986c7fdbff4c14fea0f792e70c4297b9dfa2ab44b08c759611519511be284",
    "fwd_col_P2_model_sigma2": "3006bd01bff91273046e057ea177732802034a790a180d5669fb10d1b1da6bf8",
    "fwd_col_P2_sigma12": "8b235127effeea5a600f3beb107ef2657ee2e191a4c7f6606fea06943baef888",
    "fwd_col_flat_columns_long_strip": "18b158a30df5bacf548bcaabce8b1680f0e74c6db2e364b337b8ac0ced459c50",
    "fwd_col_levels_fine_to_coarse": "90ac69fa770c5abed192b4ac26f5f5fc45ed0bec77b9b6682b6b8816d20b52b9",
    "fwd_col_tiny_top_level": "19683c1b89251e44c84ceb2308c90dd430475e285d9ce0a5846de5ec4c6a2b96",
    "fwd_col_wider_than_the_box_corners": "b1221d2313f80954852c9d93eb90909876a733b68a4f004f25c62f24174fc4da",
}


def _sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        t = t if isinstance(t, np.ndarray) else t.contiguous().cpu().view(torch.uint8).numpy()
        h.update(np.ascontiguousarray(t).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def MSDA():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pctrans_amd import MultiScaleDeformableAttention as m
    return m


@pytest.fixture(scope="module")
def lib():
    from pctrans_amd import _lib
    return _lib.lib()


def fwd_digest(MSDA, lib, cid):
    kw = dict(dict(M=8, D=16, P=4), **dict(COL_CASES)[cid])
    kw.pop("atol", None)
    c = make_case(dtype=np.float32, **kw)
    with force(lib, K_COL):
        out = MSDA.ms_deform_attn_forward(dev(c["value"]), dev(c["shapes"]), dev(c["starts"]), dev(c["loc"]), dev(c["attn"]), 64)
        assert lib.pct_msda_last_kernel() == K_COL
    return _sha(out)


def fused_digest(MSDA, lib, shapes, N, shared_ref, off_scale, pixel_ref):
    sh, value, offsets, logits, ref = _fused_case(shapes, 4, N, shared_ref, off_scale=off_scale)
    if pixel_ref:
        ref = np.broadcast_to(pixel_centres(sh)[None, :, None, :], (ref.shape[0], value.shape[1], len(shapes), 2)).astype(np.float32)
    ref_t = dev(ref).expand(N, -1, -1, -1) if shared_ref else dev(ref)
    with force(lib, K_COL):
        out = MSDA.ms_deform_attn_fused_forward(dev(value), dev(sh), dev(starts_of(sh)), ref_t, dev(offsets), dev(logits))
        assert lib.pct_msda_last_kernel() == K_COL
    return _sha(out)


def c16_digest(MSDA, lib, cid, tdt):
    _, P, shapes, kw = [c for c in COL16_CASES if c[0] == cid][0]
    c = make_case(seed=141, D=16, Lq=n_px(shapes), P=P, shapes=shapes, **dict(dict(M=8), **kw))
    v16 = torch.from_numpy(c["value"]).to(tdt)
    with force(lib, K_COL):
        out = MSDA.ms_deform_attn_forward(v16.cuda(), dev(c["shapes"]), dev(c["starts"]), dev(c["loc"]), dev(c["attn"]), 64)
        assert lib.pct_msda_last_kernel() == K_COL and out.dtype == tdt
    return _sha(out.view(torch.int16))


def bwd_digest(MSDA, lib, cid):
    kw = dict(dict(M=8, D=16, P=4), **dict(COL_CASES)[cid])
    kw.pop("atol", None)
    c = make_case(dtype=np.float32, **kw)
    _, gl, ga = run_bwd(MSDA, lib, c, grad_out_for(c, kw["seed"] + 100))       # (asserts that the column kernel ran)
    return _sha(gl, ga)


def bwd_strip_digest(MSDA, lib, shapes):
    c = make_case(seed=215, N=1, M=2, D=16, Lq=n_px(shapes), P=4, shapes=shapes, model_like=True, px_sigma=1.5)
    _, gl, ga = run_bwd(MSDA, lib, c, grad_out_for(c, 315), kernel=B_COL)
    return _sha(gl, ga)


@pytest.mark.parametrize("cid", FWD_IDS)
def test_column_forward_fp32_bits(MSDA, lib, cid):
    assert fwd_digest(MSDA, lib, cid) == DIGESTS["fwd_" + cid]


@pytest.mark.parametrize("name,shapes,N,shared_ref,off_scale,pixel_ref", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_column_forward_fused_front_end_bits(MSDA, lib, name, shapes, N, shared_ref, off_scale, pixel_ref):
    assert fused_digest(MSDA, lib, shapes, N, shared_ref, off_scale, pixel_ref) == DIGESTS[name]


@pytest.mark.parametrize("dname,tdt", C16_DTYPES, ids=[d[0] for d in C16_DTYPES])
@pytest.mark.parametrize("cid", C16_IDS)
def test_column_forward_16bit_bits(MSDA, lib, cid, dname, tdt):
    assert c16_digest(MSDA, lib, cid, tdt) == DIGESTS["%s_%s" % (cid, dname)]


@pytest.mark.parametrize("cid", BWD_IDS)
def test_column_backward_grad_loc_and_grad_attn_bits(MSDA, lib, cid):
    assert bwd_digest(MSDA, lib, cid) == DIGESTS["bwd_" + cid]


@pytest.mark.parametrize("cid,shapes", BWD_STRIPS, ids=[c[0] for c in BWD_STRIPS])
def test_column_backward_flat_columns_and_oversized_maps_bits(MSDA, lib, cid, shapes):
    assert bwd_strip_digest(MSDA, lib, shapes) == DIGESTS["bwd_strip_" + cid]


def all_digests(MSDA, lib):
    """Every digest of DIGESTS, for re-recording: call it twice from a script on the GPU, keep the cases whose two digests agree."""
    d = {"fwd_" + i: fwd_digest(MSDA, lib, i) for i in FWD_IDS}
    d.update({c[0]: fused_digest(MSDA, lib, *c[1:]) for c in FUSED_CASES})
    d.update({"%s_%s" % (i, n): c16_digest(MSDA, lib, i, t) for i in C16_IDS for n, t in C16_DTYPES})
    d.update({"bwd_" + i: bwd_digest(MSDA, lib, i) for i in BWD_IDS})
    d.update({"bwd_strip_" + c[0]: bwd_strip_digest(MSDA, lib, c[1]) for c in BWD_STRIPS})
    return d

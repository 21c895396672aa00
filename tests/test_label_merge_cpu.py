"""CPU: the table-based restatement of the reference's merge_func (tests/label_merge_reference.py) against vectors recorded from
the reference's own code (tests/golden/label_merge_small.npz), the torch formulation (pctrans_amd/label_merge.py, mode="torch")
against the restatement, the discrimination of the test inputs, the ABI bookkeeping of the entry
(include/pctrans_hip_merge.h) and the argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import label_merge_cases as C
import label_merge_reference as R
from conftest import ROOT

NAME = "pct_label_merge_small"
GOLDEN = os.path.join(ROOT, "tests", "golden", "label_merge_small.npz")


def _torch(seg, fg, passes, dtype=None):
    from pctrans_amd import label_merge as LM
    labels = torch.from_numpy(np.ascontiguousarray(seg)[None])
    labels = labels if dtype is None else labels.to(dtype)
    return LM.merge_small_objects(labels, None if fg is None else torch.from_numpy(fg[None]), passes, mode="torch")


def test_restatement_equals_the_recorded_reference_bit_for_bit():
    gold = np.load(GOLDEN)
    names = sorted(k[:-3] for k in gold.files if k.endswith(".in"))
    kinds = {n.split(".")[0] for n in names}
    assert kinds == {"hand", "random", "float", "pass0", "pass1", "pass2"} and len(names) >= 40
    merges = 0
    for name in names:
        seg, want, passes = gold[name + ".in"], gold[name + ".out"], [tuple(p) for p in gold[name + ".passes"].tolist()]
        got = R.merge(seg, passes)
        assert got.ties == 0, name
        assert got.out.dtype == want.dtype and np.array_equal(got.out, want), name
        merges += sum(got.merges)
        if name.startswith("hand."):                                            # the fixture is of the cases as they are now
            hand, fg, hp = C.hand()[name[5:]]
            assert np.array_equal(seg, hand if fg is None else hand * fg) and tuple(passes) == hp, name
    assert merges >= 100
    assert sorted(n[5:] for n in names if n.startswith("hand.")) == sorted(set(C.tie_free_hand()) - {"count_512"})


def test_hand_built_cases_are_tie_free_and_reach_their_branches():
    for name, (seg, fg, passes) in C.tie_free_hand().items():
        assert R.merge(seg, passes, fg).ties == 0, name
    for name in C.TIED:
        seg, fg, passes = C.hand()[name]
        assert R.merge(seg, passes, fg).ties > 0, name
    ev = lambda name: [(p, int(a), int(b)) for p, a, b in R.merge(*[C.hand()[name][i] for i in (0, 2, 1)]).events]
    assert ev("inside_object") == ev("beside_object") == ev("beside_two_objects") == ev("two_parts") == [(0, 7, 3)]
    assert ev("isolated") == ev("dominates_crop") == ev("deep_inside_object") == ev("all_zero") == []
    assert ev("borders") == [(0, 7, 3)]                                          # 8, near the top left corner, stays
    assert ev("chain_up") == ev("chain_grows_past_threshold") == [(0, 5, 6), (0, 6, 3)] and ev("chain_down") == [(0, 6, 5)]
    assert ev("second_pass") == [(1, 7, 3)] and ev("grows_past_fifty") == [(1, 6, 8)] and ev("small_background") == [(0, 0, 1)]
    assert ev("gate") == [(0, 4, 3)] and ev("tiny_9x7")[0] == (0, 7, 3) and ev("tiny_6x40") == [(1, 7, 3)]
    assert ev("gaps") == [(0, 40000, 3), (0, 65535, 700)] and ev("tie_two_objects") == [(0, 7, 3)]
    for name, want in (("count_512", 512), ("count_513", 513)):
        m = R.merge(*C.hand()[name][::2])
        assert len(m.values) == want and bool(m.status & R.STATUS_COUNT) == (want > 512)
    for name, bit in C.UNCOVERED.items():
        assert R.merge(*C.hand()[name][::2]).status & ~R.STATUS_TIE == bit, name


@pytest.mark.parametrize("size", [(37, 53), (64, 64)])
def test_the_tie_filter_keeps_at_least_half_of_the_draws(size):
    maps, draws = C.random_tie_free(size[0], size[1], 8, 11)
    assert len(maps) == 8 and draws <= 16
    assert sum(sum(R.merge(m).merges) for m in maps) >= 16


def test_torch_mode_equals_the_restatement_on_every_case():
    from pctrans_amd import label_merge as LM
    cases = dict(C.hand())
    for size in ((37, 53), (64, 64)):
        for n, m in enumerate(C.random_tie_free(size[0], size[1], 8, 11)[0]):
            cases["random_%dx%d_%d" % (size + (n,))] = (m, (m % 5 != 1).astype(np.uint8) if n % 2 else None, R.PASSES)
    for name, (seg, fg, passes) in sorted(cases.items()):
        want = R.merge(seg, passes, fg)
        for dtype in (None, torch.float32, torch.int32):
            if dtype is torch.int32 and name == "fractional_value":
                continue
            got = _torch(seg, fg, passes, dtype)
            k = len(want.values)
            assert got.mode == "torch" and got.shape == (1,) + seg.shape and got.status.dtype == torch.int32
            assert np.array_equal(got[0].numpy().astype(np.float64), want.out.astype(np.float64)), name
            assert got.status.tolist() == [want.status] and got.num.tolist() == [k], name
            assert got.merges[0].tolist() == want.merges + [0] * (LM.MAX_PASSES - len(passes)), name
            assert got.values[0, :k].tolist() == want.values.tolist() and got.final[0, :k].tolist() == want.final.tolist(), name
            assert got.areas_before[0, :k].tolist() == want.before.tolist(), name
            assert got.areas_after[0, :k].tolist() == want.after.tolist(), name
            assert got.values.shape[1] == max(LM.MAX_VALUES, k) and not got.areas_after[0, k:].any()


def test_the_inputs_tell_the_known_wrong_variants_apart():
    """Each wrong reading of the rules changes a pixel of at least one hand-built case, and of the case built for it."""
    expect = {"ceil_centroid": "half_centroid", "round_centroid": "half_centroid", "clamp_crop": "tiny_6x40",
              "live_sizes": "chain_grows_past_threshold", "snapshot_centroid": "chain_up", "stale_sums": "chain_up",
              "descending": "pair_order", "ge2_distinct": "deep_inside_object", "lt_threshold": "exact_threshold",
              "gate_after": "gate"}
    assert set(expect) == set(R.VARIANTS)
    for variant, name in expect.items():
        seg, fg, passes = C.hand()[name]
        assert not np.array_equal(R.merge(seg, passes, fg, variant=variant).out, R.merge(seg, passes, fg).out), (variant, name)
    seg, fg, passes = C.hand()["borders"]                                        # the empty crop at the top left corner
    assert (R.merge(seg, passes, variant="clamp_crop").out[seg == 8] == 4).all() and (R.merge(seg, passes).out[seg == 8] == 8).all()


def test_abi_bookkeeping():
    from pctrans_amd import _lib, label_merge as LM
    assert '#include "pctrans_hip_merge.h"' in open(os.path.join(ROOT, "include", "pctrans_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "pctrans_hip_merge.h")).read()
    declared = re.findall(r"PCT_API\s+[\w\s\*]+?\b(pct_\w+)\s*\(", header)
    assert declared == list(_lib.MERGE_SYMBOLS) == [NAME] and "trainer.py:744-777" in header
    for other in (_lib.SYMBOLS, _lib.OPT_IN_SYMBOLS, _lib.POST_SYMBOLS, _lib.METRICS_SYMBOLS, _lib.TARGETS_SYMBOLS):
        assert NAME not in other
    argtypes, restype, checked_by = _lib.MERGE_SYMBOLS[NAME]
    assert restype is ctypes.c_int and os.path.exists(os.path.join(ROOT, checked_by))
    decl = [a.strip() for a in re.search(r"PCT_API int %s\(([^)]*)\)" % NAME, header).group(1).split(",")]
    assert len(argtypes) == len(decl)
    for a, t in zip(decl, argtypes):
        assert (t is ctypes.c_void_p) == ("*" in a) and (t is ctypes.c_int) == a.startswith("int "), a
    assert hasattr(_lib.lib(), NAME)
    makefile = open(os.path.join(ROOT, "pctrans_amd", "csrc", "Makefile")).read()
    assert " label_merge.hip " in makefile and "pctrans_hip_merge.h" in makefile
    assert "launch_label_merge_small(" in open(os.path.join(ROOT, "pctrans_amd", "csrc", "launchers.hpp")).read()
    for macro, value in (("PCT_MERGE_MAX_VALUES", LM.MAX_VALUES), ("PCT_MERGE_MAX_PASSES", LM.MAX_PASSES),
                         ("PCT_MERGE_MAX_WINDOW", LM.MAX_WINDOW), ("PCT_MERGE_WORKSPACE_PER_IMAGE", LM.WORKSPACE_PER_IMAGE),
                         ("PCT_MERGE_STATUS_VALUE", LM.STATUS_VALUE), ("PCT_MERGE_STATUS_COUNT", LM.STATUS_COUNT),
                         ("PCT_MERGE_STATUS_TIE", LM.STATUS_TIE)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert (LM.STATUS_VALUE, LM.STATUS_COUNT, LM.STATUS_TIE) == (R.STATUS_VALUE, R.STATUS_COUNT, R.STATUS_TIE)


def test_argument_errors_are_reported_without_a_launch():
    """No launch, so this runs without a GPU: the pointers are host memory that is never dereferenced."""
    from pctrans_amd import _lib
    L = _lib.lib()
    UNSUP, BAD, ALIGN = -4, -1, -3
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0

    def call(N, H, W, passes, dtype=2, num=None, out=p, ws=p, status=p):
        arr = (ctypes.c_int32 * max(len(passes), 1))(*passes)
        return L.pct_label_merge_small(p, dtype, None, N, H, W, ctypes.cast(arr, ctypes.c_void_p) if passes is not None else None,
                                       len(passes) // 2 if num is None else num, ws, out, p, p, p, p, p, p, status, None)
    ok = [5, 5, 20, 11, 50, 11]
    assert call(0, 8, 8, ok) == UNSUP and call(65536, 8, 8, ok) == UNSUP
    assert call(1, 4096, 4096, ok) == UNSUP                                      # height * width = 2^24
    assert call(1, 8, 8, ok, dtype=5) == UNSUP and call(1, 8, 8, ok, dtype=-1) == UNSUP
    assert call(1, 0, 8, ok) == BAD and call(1, 8, -1, ok) == BAD
    assert call(1, 8, 8, ok, num=0) == BAD and call(1, 8, 8, ok * 3, num=9) == BAD
    assert call(1, 8, 8, [5, 0]) == BAD and call(1, 8, 8, [5, 32]) == BAD and call(1, 8, 8, [-1, 5]) == BAD
    assert L.pct_label_merge_small(p, 2, None, 1, 8, 8, None, 1, p, p, p, p, p, p, p, p, p, None) == BAD
    assert call(1, 8, 8, ok, out=None) == BAD and call(1, 8, 8, ok, status=None) == BAD
    assert call(1, 8, 8, ok, ws=p + 8) == ALIGN and call(1, 8, 8, ok, status=p + 2) == ALIGN and call(1, 8, 8, ok, out=p + 2) == ALIGN


def test_modes_switch_and_supported(monkeypatch):
    from pctrans_amd import label_merge as LM
    labels = torch.zeros((2, 16, 12), dtype=torch.int16)
    with pytest.raises(ValueError, match="mode"):
        LM.merge_small_objects(labels, mode="numpy")
    with pytest.raises(ValueError, match="passes"):
        LM.merge_small_objects(labels, passes=((5, 32),))
    with pytest.raises(ValueError, match="passes"):
        LM.merge_small_objects(labels, passes=())
    with pytest.raises(ValueError, match="fg"):
        LM.merge_small_objects(labels, fg=torch.ones((2, 16, 11)))
    with pytest.raises(ValueError, match="labels"):
        LM.merge_small_objects(labels[0])
    monkeypatch.delenv("PCT_LABEL_MERGE", raising=False)
    assert LM.default() == "hip"
    monkeypatch.setenv("PCT_LABEL_MERGE", "torch")
    assert LM.default() == "torch"
    monkeypatch.setenv("PCT_LABEL_MERGE", "cuda")
    with pytest.raises(RuntimeError, match="PCT_LABEL_MERGE"):
        LM.default()
    monkeypatch.delenv("PCT_LABEL_MERGE")
    assert not LM.supported(labels)                                              # CPU tensors: the default mode gives the torch result
    res = LM.merge_small_objects(labels)
    assert res.mode == "torch" and torch.equal(res, labels) and res.status.tolist() == [0, 0]

    class _Cuda:
        """What `supported` asks of a tensor, for a device this machine may not have."""
        def __init__(self, shape, dtype=torch.int16):
            self.shape, self.dtype, self.is_cuda, self.device = torch.Size(shape), dtype, True, torch.device("cuda", 0)
        def dim(self):
            return len(self.shape)
    monkeypatch.setattr(torch, "is_tensor", lambda x: isinstance(x, (torch.Tensor, _Cuda)))
    ok = lambda *shape, **kw: LM.supported(_Cuda(shape, **kw))
    assert ok(1, 520, 696) and ok(65535, 2, 2) and ok(1, 4095, 4096) and ok(33, 530, 500, dtype=torch.float32)
    assert not ok(65536, 2, 2) and not ok(0, 4, 4) and not ok(1, 4096, 4096) and not ok(1, 0, 4) and not ok(8, 8)
    assert not ok(1, 8, 8, dtype=torch.float64) and not ok(1, 8, 8, dtype=torch.bool)
    assert not LM.supported(_Cuda((1, 8, 8)), fg=_Cuda((1, 8, 8), torch.float32))
    assert LM.supported(_Cuda((1, 8, 8)), fg=_Cuda((1, 8, 8), torch.uint8)) and LM.supported(_Cuda((1, 8, 8)), fg=_Cuda((1, 8, 8), torch.bool))


def test_source_rules_of_the_kernel_file():
    src = open(os.path.join(ROOT, "pctrans_amd", "csrc", "label_merge.hip")).read()
    assert "asm" not in src and "__builtin_amdgcn" not in src                  # vector stores and plain C++ only
    for line in src.splitlines():                                              # no floating point but the float32 labels themselves
        if re.search(r"\b(float|double)\b", line):
            assert "m.labels" in line or "launch_apply<float>" in line, line
    assert "atomicAdd(&cnt[key], len)" in src                                  # integer adds: one per run
    assert not re.search(r"\b(malloc|hipMalloc|hipStreamSynchronize|hipDeviceSynchronize|hipMemcpy)\b", src)

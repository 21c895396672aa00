"""CPU: bench.py --dump-outputs writes what the timed path returned as <name>.npy, float32 / float64, under the 64 MB
budget, with the same positions sampled from run to run (so that two builds can be compared output for output).  Run in a
child process: importing bench sets MIOpen environment variables."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import json, sys
import torch
import bench
g = torch.Generator().manual_seed(0)
big = torch.randn(10, 64, 64, generator=g).to(torch.bfloat16).expand(1000, 10, 64, 64)      # 41M elements
out = {"pred_masks": big, "aux_outputs": [{"pred_masks": big}, {"pred_masks": big}],
       "reference_points": torch.rand(3, 5, 2, generator=g), "indices_list": [],
       "sem_mask": torch.randn(2, 3, 4, generator=g, dtype=torch.float64)}
print(json.dumps(bench.dump_outputs(out, sys.argv[1])))
"""


def _dump(d):
    r = subprocess.run([sys.executable, "-c", SCRIPT, str(d)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dump_outputs_names_dtypes_budget_and_repeatable_sample(tmp_path):
    m1, m2 = _dump(tmp_path / "a"), _dump(tmp_path / "b")
    assert m1 == m2
    names = {"pred_masks", "aux_outputs.0.pred_masks", "aux_outputs.1.pred_masks", "reference_points", "sem_mask"}
    assert set(m1) == names
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        total += os.path.getsize(tmp_path / "a" / (n + ".npy"))
        assert np.array_equal(a, b), n
        assert a.dtype == (np.float64 if n == "sem_mask" else np.float32), n
    assert total <= 64 * 10**6
    # the small arrays whole, in their shape; the large ones as a flat sample that fills the budget
    assert m1["reference_points"] == {"shape": [3, 5, 2], "sampled": None}
    assert np.load(tmp_path / "a" / "sem_mask.npy").shape == (2, 3, 4)
    for n in ("pred_masks", "aux_outputs.0.pred_masks"):
        assert m1[n]["shape"] == [1000, 10, 64, 64]
        assert np.load(tmp_path / "a" / (n + ".npy")).shape == (m1[n]["sampled"],)
        assert m1[n]["sampled"] > 4 * 10**6
    # same tensor, different name: a different (but fixed) set of positions
    assert not np.array_equal(np.load(tmp_path / "a" / "pred_masks.npy"),
                              np.load(tmp_path / "a" / "aux_outputs.0.pred_masks.npy"))

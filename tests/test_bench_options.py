"""CPU: bench.py's command line and its gate on the extras.  A plain run leaves the extra measurements (cpu_baseline) off;
--full turns them on and changes nothing about the timed steps' options.  Run in a child process: importing bench sets
MIOpen environment variables."""
import ast
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import json, sys
import bench
sys.argv = ["bench.py"] + sys.argv[1:]
a = bench.parse()
d = {k: getattr(a, k) for k in ("gpus", "steps", "warmup", "batch", "dump_outputs", "full", "no_cpu_baseline")}
d["cpu_baseline_by_world"] = [bench.wants_cpu_baseline(a, w) for w in (1, 2)]
print(json.dumps(d))
"""


def _parse(*argv):
    r = subprocess.run([sys.executable, "-c", SCRIPT] + list(argv), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_full_is_off_by_default_and_leaves_the_timed_options_alone():
    plain = _parse("--gpus", "1", "--steps", "7", "--warmup", "2")
    assert plain == {"gpus": 1, "steps": 7, "warmup": 2, "batch": 128, "dump_outputs": None, "full": False,
                     "no_cpu_baseline": False, "cpu_baseline_by_world": [False, False]}
    assert _parse("--gpus", "1", "--steps", "7", "--warmup", "2", "--full") == dict(
        plain, full=True, cpu_baseline_by_world=[True, False])
    out = _parse("--full", "--no-cpu-baseline", "--dump-outputs", "d")
    assert out["dump_outputs"] == "d" and out["cpu_baseline_by_world"] == [False, False]


def test_main_runs_the_cpu_baseline_only_behind_the_gate():
    """main() needs a GPU, so its source is read: the one call of cpu_baseline() sits under `if wants_cpu_baseline(...)`."""
    with open(os.path.join(ROOT, "bench.py")) as f:
        tree = ast.parse(f.read())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")

    def calls(node, name):
        return [c for c in ast.walk(node) if isinstance(c, ast.Call) and getattr(c.func, "id", None) == name]
    assert len(calls(main, "cpu_baseline")) == 1
    gates = [n for n in ast.walk(main) if isinstance(n, ast.If) and calls(n.test, "wants_cpu_baseline")]
    assert len(gates) == 1 and calls(ast.Module(body=gates[0].body, type_ignores=[]), "cpu_baseline")
    assert not calls(ast.Module(body=gates[0].orelse, type_ignores=[]), "cpu_baseline")

"""bench.py's options without a GPU: a plain run measures the headline only, --full turns the CPU baselines and the secondary
measurements on, and an option given explicitly wins either way.  Parsed in a child process: importing bench.py sets the
runtime's hardware-queue count in its environment."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("full", "cpu_seconds", "cpu_all_cores", "extras", "indel_callers", "steps", "warmup")


def _parsed(*argvs):
    code = ("import json, sys, bench\n"
            "print(json.dumps([{k: getattr(bench.parse(v), k) for k in %r} for v in json.loads(sys.argv[1])]))" % (KEYS,))
    r = subprocess.run([sys.executable, "-c", code, json.dumps(argvs)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_is_the_headline_only_and_full_adds_the_rest():
    plain, full, mixed, indel = _parsed(["--gpus", "1", "--steps", "20", "--warmup", "3"],
                                        ["--gpus", "1", "--steps", "20", "--warmup", "3", "--full"],
                                        ["--full", "--cpu-seconds", "0", "--extras", "0"],
                                        ["--mode", "indel", "--cpu-seconds", "8"])
    assert plain == dict(full=False, cpu_seconds=0.0, cpu_all_cores=0, extras=0, indel_callers=0, steps=20, warmup=3)
    assert full == dict(full=True, cpu_seconds=15.0, cpu_all_cores=1, extras=1, indel_callers=1, steps=20, warmup=3)
    assert (mixed["cpu_seconds"], mixed["cpu_all_cores"], mixed["extras"], mixed["indel_callers"]) == (0.0, 1, 0, 1)
    assert (indel["full"], indel["cpu_seconds"], indel["indel_callers"]) == (False, 8.0, 0)

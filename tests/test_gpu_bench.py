"""-m gpu: a plain `python bench.py` on the MI355X is lean - set-up, warm-up, timed steps, one JSON line - and everything that takes
runs of its own stays behind `--full` (tests/test_bench_cpu.py has the control flow of both on the stub engine)."""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

from tests.test_bench_cpu import FULL_ONLY

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.mark.timeout(300)
def test_plain_bench_run_spends_at_most_30_s_outside_its_steps(built_library):
    """Whole wall time of a fresh `bench.py --gpus 1 --steps N --warmup W` process, less (N + W) x ms_per_step: at most 30 s (library
    load, weights, contexts, graph capture and whatever the first step compiles or tunes are all in it), and none of the `--full`
    blocks on the line."""
    n, w = 3, 1
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(n), "--warmup", str(w)],
                       cwd=ROOT, capture_output=True, text=True, timeout=280)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    outside = wall - (n + w) * d["ms_per_step"] * 1e-3
    print(f"BENCH_PLAIN wall {wall:.2f} s, ms_per_step {d['ms_per_step']}, outside the steps {outside:.2f} s")
    assert d["full"] is False and d["steps"] == n and d["warmup"] == w and d["value"] > 0
    assert not [k for k in FULL_ONLY if k in d], sorted(d)
    assert d["roofline"]["frac"] > 0 and d["stage_ms_per_step"]["greedy_ms"] > 0     # read off the timed steps themselves
    assert outside <= 30.0, (wall, d["ms_per_step"])

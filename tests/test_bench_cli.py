"""bench.py's command line: a plain run times its steps and prints the result
line only; --full adds the context figures; --dump-outputs writes what the
last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tools import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, WIDTH = 9000, 128  # 1 152 000 entries: index / value are longer than bench.DUMP_SAMPLE, offset / label are not


def bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_help_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_last_step(tmp_path):
    d = str(tmp_path / "dump")
    line = bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--rows", str(ROWS), "--dump-outputs", d)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert "hbm_copy" not in line and line["cpu_baseline"] is None and "cpu_baseline_max_threads" not in line

    text, _ = synth.rows(synth.LIBSVM, ROWS, WIDTH, seed=1)  # the bench's shard at --rows ROWS
    o = po.parse_chunks(text.tobytes(), [0, len(text)], fmt=po.LIBSVM)
    assert o["status"] == 0
    total = 0
    for k in ("weight", "qid", "field"):  # slots this input does not fill: no file, never an empty one
        assert np.asarray(o.get(k, [])).size == 0 and not os.path.exists(os.path.join(d, k + ".npy")), k
    for k in ("offset", "label", "index", "value"):
        got = np.load(os.path.join(d, k + ".npy"))
        assert got.size > 0, k
        total += got.nbytes
        want = np.asarray(o[k])
        assert got.dtype == (np.float32 if k in ("label", "weight", "value") else np.float64), k
        if want.size > (1 << 20):  # the fixed sample (bench.dump_outputs)
            pos = np.sort(np.random.default_rng(0).integers(0, want.size, size=1 << 20, dtype=np.int64))
            want = want[pos]
        assert got.shape == want.shape, k
        assert got.tobytes() == want.astype(got.dtype).tobytes(), k
    res = np.load(os.path.join(d, "result.npy"))
    assert res[0] == ROWS and res[1] == ROWS * WIDTH and res[8] == 0  # rows, entries, error
    assert total <= 64 << 20


@pytest.mark.gpu
def test_bench_full_adds_context_figures():
    line = bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--rows", str(ROWS), "--full", "--cpu-budget", "0.2")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["hbm_copy"].get("GBps", 0) > 0, line["hbm_copy"]
    assert line["cpu_baseline"].get("value", 0) > 0, line["cpu_baseline"]

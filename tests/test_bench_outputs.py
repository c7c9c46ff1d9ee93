"""bench.py on a tiny workload: a plain run prints the headline without the --full sections, --full still adds them, and
--dump-outputs writes what the last timed step left, the same arrays from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--warmup", "1", "--width", "4", "--levels", "3"]
FULL_ONLY = {"roofline", "cpu_baseline"}
NAMES = ["r.npy", "residual_norm.npy", "x.npy"]


def _bench(steps, extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps)] + ARGS + extra, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _load(d):
    assert sorted(os.listdir(d)) == NAMES
    return {n[:-4]: np.load(os.path.join(d, n)) for n in NAMES}


def _same(a, b):
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-12, atol=1e-14 * max(np.abs(a[k]).max(), 1e-300))


@pytest.mark.gpu
def test_plain_run_dumps_what_the_last_timed_step_left(tmp_path):
    rec = _bench(3, ["--dump-outputs", str(tmp_path / "a")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert not FULL_ONLY & set(rec)
    a = _load(tmp_path / "a")
    nf, ne = rec["config"]["nf"], rec["config"]["cells"]
    for k, v in a.items():
        assert v.dtype == np.float64 and np.isfinite(v).all()
        assert v.shape == ((1,) if k == "residual_norm" else (nf * ne,))     # small enough to be written whole
    # the norm the result line reports for the state after the timed steps is the one dumped beside x and r
    assert a["residual_norm"][0] == rec["config"]["residual_norm_after"]
    assert np.abs(a["x"]).max() > 0 and np.abs(a["r"]).max() > 0 and not np.array_equal(a["x"], a["r"])

    _bench(3, ["--dump-outputs", str(tmp_path / "b")])
    _same(a, _load(tmp_path / "b"))

    rec4 = _bench(4, ["--dump-outputs", str(tmp_path / "c")])
    c = _load(tmp_path / "c")
    assert rec4["steps"] == 4 and c["residual_norm"][0] == rec4["config"]["residual_norm_after"]
    assert not np.allclose(c["x"], a["x"], rtol=1e-9, atol=0)               # one more timed V-cycle moves x


@pytest.mark.gpu
def test_full_run_keeps_the_extra_sections(tmp_path):
    rec = _bench(3, ["--full", "--cpu-sample-width", "4", "--tune-placement", "2", "--tuned-burst", "1",
                     "--dump-outputs", str(tmp_path / "full")])
    assert FULL_ONLY <= set(rec)
    assert rec["roofline"]["launches"] > 0 and len(rec["roofline"]["levels"]) == 3
    assert rec["config"]["placement"]["candidates"] == 2
    # the --full measurements run after the dump: it holds what a plain run with the same arguments dumps
    _bench(3, ["--dump-outputs", str(tmp_path / "plain")])
    _same(_load(tmp_path / "full"), _load(tmp_path / "plain"))

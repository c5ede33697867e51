"""A plain bench.py run on the GPU: the line carries the headline figures and none of the --full
extras, --steps sets the number of timed steps, and --dump-outputs writes the state the timed
steps left -- the same bits as an engine in this process stepped as often (1 first step + W-1
warm-up steps + K timed steps from the analytic IC).  (One child process beside the test's own.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_the_state_after_the_last_timed_step(tmp_path, case_factory):
    from hnumo.engine import Engine
    K, W = 2, 2
    d = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--config", "bump10", "--dump-outputs", d]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == K and line["warmup"] == W and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
    assert line["unit"] == "element-updates/s" and line["higher_is_better"] is True
    for extra in ("cpu_baseline", "c4_single_gpu", "c3_single_gpu", "c5_single_gpu"):
        assert extra not in line, extra
    roof = line["roofline"] or {}
    for extra in ("step_breakdown_us", "peak_measured"):
        assert extra not in roof, extra

    case = case_factory("bump10")
    e = Engine(case)
    e.set_resident(True)
    q, qb, qp = e.state()
    for _ in range(W + K):
        e.ti_rk_bcl(q, qb, qp)
    e.sync(q, qb, qp)
    e.close()
    assert sorted(os.listdir(d)) == ["q_df.npy", "qb_df.npy", "qprime_df.npy"]
    for name, ref in (("q_df", q), ("qb_df", qb), ("qprime_df", qp)):
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == np.float64 and a.shape == ref.shape, name
        assert np.array_equal(a, ref), name
        assert line["dumped_outputs"][name] == {"shape": list(ref.shape), "sampled": False}

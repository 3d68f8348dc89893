"""bench.py as a command: a plain run times exactly the requested steps, leaves the extras to --full and, with
--dump-outputs, writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_step_counts_are_validated_before_any_work():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--steps" in out.stderr


@pytest.mark.gpu
def test_plain_run_times_the_requested_steps_and_dumps_the_last_steps_outputs(tmp_path):
    """10k workload, 3 timed steps after 2 warm-up steps.  The dumped solution must solve V X = B for the seeded inputs of
    the LAST timed step (step index 2: sigma2 = (0.42, 0.58)) to the 1e-10 the fp64 parity tests use, and log det V must
    equal the dense slogdet to 1e-10 relative."""
    import bench
    dump = tmp_path / "out"
    run = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "2", "--workload", "10k",
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["unit"] == "nnz(L)/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - line["config"]["nnzL"] / (line["ms_per_step"] / 1e3)) <= 1e-9 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["config"]["solve_residual"] is None
    got = {f: np.load(dump / (f + ".npy")) for f in ("logdet", "solve", "solve_rows")}
    assert sorted(os.listdir(dump)) == ["logdet.npy", "solve.npy", "solve_rows.npy"]
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    A, C, y = bench.build_problem("10k", 0)
    n = y.size
    rows = got["solve_rows"].astype(np.int64)
    assert np.array_equal(rows, np.arange(n)) and got["solve"].shape == (n, 103)   # (small enough to be written whole)
    B = np.hstack([C, y[:, None], np.random.default_rng(100).standard_normal((n, 100))])
    V = (0.42 * A + 0.58 * sp.identity(n, format="csr")).tocsr()
    assert np.abs(V @ got["solve"] - B).max() <= 1e-10 * np.abs(B).max()
    ref = np.linalg.slogdet(V.toarray())[1]
    assert got["logdet"].shape == (1,) and abs(got["logdet"][0] - ref) <= 1e-10 * abs(ref)
    assert got["logdet"][0] == line["config"]["logdet"]

"""bench.py's plain run and `--dump-outputs`: a plain `--gpus 1 --steps K
--warmup W` run times K steps, reports `ms_per_step` consistently with its
headline value, measures none of the `--full` legs, and writes what the last
timed step returned as finite float32 / float64 .npy files (a failed tree's
NaN stored as 0, an overflowed sum as the largest float64); the inputs are seeded,
so two runs with the same arguments dump identical arrays, and they are the
arrays the engine gives a caller for the same batch, bit for bit.

Small sizes that still take the benchmark's path: 300 trees (above the
256-tree bar for tree code) x 5000 rows (no multiple of a row tile). With so
few row groups the tree code marks trees sticky PRECISE by default, and which
row group marks a tree first depends on the schedule (tests/test_jit_gpu.py),
so the FAST / PRECISE choice per tile is not fixed; the benchmark's own size
(1M rows) runs with the mark off, and so do these runs
(SRHIP_JIT_STICKY_TREE=0), which makes every tile's choice, and with it every
bit of the result, the same from run to run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import srhip
from srhip import constants as K

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NTREES, ROWS, NFEAT, STEPS, WARMUP = 300, 5000, 5, 3, 1


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env["SRHIP_JIT_STICKY_TREE"] = "0"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--ntrees", str(NTREES), "--rows", str(ROWS), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, env=env, timeout=120, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    a, b = tmp_path_factory.mktemp("dump_a"), tmp_path_factory.mktemp("dump_b")
    return (_bench(a), a), (_bench(b), b)


def test_plain_line_times_the_steps_asked_for(runs):
    (line, _), _ = runs
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "node·row/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert len(line["steps_detail"]["wall_ms"]["first3"]) == STEPS
    # value = node·rows of one step / time of one step
    node_rows = line["config"]["total_nodes_per_gpu"] * ROWS
    assert line["value"] == pytest.approx(node_rows / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # the legs of --full are not measured
    assert line["cpu_baseline"] is None and line["row_shard"] is None and line["weak"] is None


def test_dump_is_small_float_arrays_and_repeats(runs):
    (_, a), (_, b) = runs
    names = sorted(p.name for p in a.glob("*"))
    assert names == ["did_succeed.npy", "loss_sums.npy", "weight_sum.npy"]
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert np.isfinite(x).all(), n
        total += x.nbytes
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), n
    assert total <= 64 * 2**20
    assert np.load(a / "loss_sums.npy").shape == (NTREES,)
    assert np.load(a / "did_succeed.npy").shape == (NTREES,)
    assert np.load(a / "weight_sum.npy").shape == (1,)


def test_dump_is_what_the_engine_returns(runs, gpu_ctx, monkeypatch):
    (_, a), _ = runs
    monkeypatch.setenv("SRHIP_JIT_STICKY_TREE", "0")  # read per launch
    # the benchmark's batch (bench.py: dataset seed 1, trees seed 1000, maxsize 30)
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    X = np.random.default_rng(1).standard_normal((NFEAT, ROWS)).astype(np.float32)
    y = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    trees = srhip.random_population(NTREES, o, NFEAT, np.float32, seed=1000, maxsize=30)
    ds = srhip.DeviceDataset(gpu_ctx, X, y)
    prog = srhip.Program(gpu_ctx, srhip.flatten(trees, o, dtype=np.float32), np.float32)
    sums, wsum, ok = prog.eval_loss(ds, K.LOSS["L2"])
    assert ok.any() and not ok.all()  # the batch has succeeding and failing trees
    assert np.array_equal(np.load(a / "did_succeed.npy"), ok.astype(np.float32))
    assert np.isnan(sums[~ok]).all() and np.isfinite(sums[ok]).any()
    stored = np.load(a / "loss_sums.npy")
    big = np.finfo(np.float64).max
    assert np.array_equal(stored, np.where(np.isnan(sums), 0.0, np.clip(sums, -big, big)))
    assert np.array_equal(stored[~ok], np.zeros(int((~ok).sum())))
    assert np.load(a / "weight_sum.npy")[0] == wsum == float(ROWS)

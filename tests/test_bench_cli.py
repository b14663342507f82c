"""bench.py's command line: a plain run is lean, --full is there, --dump-outputs writes the last
timed step's results as float64 .npy files within the size budget, the same from run to run."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bench

ROOT = Path(__file__).resolve().parent.parent


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return bench.parse()


def test_plain_arguments_select_the_lean_c2_run(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.workload, a.steps, a.warmup, a.full, a.dump_outputs) == ("c2", 7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1"), ("--workload", "ingest", "--dump-outputs", "d")])
def test_arguments_that_cannot_be_honoured_are_refused(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones(tmp_path):
    small = np.arange(12, dtype=np.uint8).reshape(3, 4)
    big = np.arange(9_000_000, dtype=np.uint32)  # 72 MB as float64: over its share of the budget
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"small": small, "big": big})
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("small", "big")}
    assert got["small"].dtype == np.float64 and np.array_equal(got["small"], small)
    assert got["big"].dtype == np.float64 and got["big"].ndim == 1 and 1_000_000 < got["big"].size < big.size
    assert np.all(np.diff(got["big"]) > 0)  # a sample of the elements, in index order
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= bench.DUMP_BUDGET
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))  # the same sample every time


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_finalized_table(gpu, tmp_path):
    """One small plain run: --steps is the number of timed steps, no leg of --full runs, and the
    dumped table is bit for bit what a caller of accumulate + finalize gets for the same batch."""
    from zipkin_amd import DepsContext, DeviceColumns, tracegen_params

    S, records, seed, depth = 37, 30_000, 5, 6
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--records", str(records), "--services", str(S), "--seed", str(seed),
                        "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["full"] is False and line["ms_per_step"] > 0
    # four table sets, so four warm-up steps (one per set), then timed steps 5..7 go to sets 0, 1, 2:
    # set 0, whose launches the line counts, takes exactly one of them
    assert line["warmup"] == 1 and line["warmup_steps"] == 4
    assert line["detail"]["pipelined_k1_launches"] == 1
    assert line["cpu_baseline"] is None and line["parity"] is None and line["roofline"]["frac"] is None
    assert line["value"] == pytest.approx(line["config"]["total_records"] / (line["ms_per_step"] * 1e-3))
    got = {k: np.load(tmp_path / "d" / f"{k}.npy") for k in ("m0", "m1", "m2", "m3", "m4", "present")}
    assert all(v.dtype == np.float64 and v.shape == (S * S,) for v in got.values())
    p = tracegen_params(seed, int(records / 15) + 1000, target_records=records, max_depth=depth, num_services=S)
    with DepsContext(S) as ctx:
        dev = DeviceColumns(records)
        n, _ = ctx.tracegen_device(p, dev)
        ctx.accumulate(dev, clustered=True, verify=True)
        want = ctx.finalize()
    assert n == line["config"]["records_per_gpu"] and got["m0"].sum() > 0
    for k in got:
        assert np.array_equal(got[k], np.asarray(getattr(want, k)).ravel().astype(np.float64)), k

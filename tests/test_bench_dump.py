"""`bench.py --dump-outputs DIR`: what the headline workload's last timed step computed, written as DIR/<workload>.npy (the whole
batch, or a fixed seeded sample of its rows when that is over the byte budget) so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=300):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, env=e, timeout=timeout)


def test_dump_rows_fixed_sample_within_budget():
    import bench

    assert np.array_equal(bench.dump_rows(8, 1000), np.arange(8))
    row_bytes = 513 * 626 * 4  # one utterance of the linear-power headline
    rows = bench.dump_rows(256, row_bytes)
    assert 1 < len(rows) < 256 and len(rows) * row_bytes <= bench.DUMP_BYTES < 64e6
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 256
    assert np.array_equal(rows, bench.dump_rows(256, row_bytes))


def test_steps_and_dump_arguments_are_checked():
    r = _run(["--gpus", "1", "--steps", "0", "--dry-run"])
    assert r.returncode == 2 and "--steps" in r.stderr
    r = _run(["--gpus", "1", "--steps", "2", "--dry-run", "--dump-outputs", "unused"])
    assert r.returncode == 2 and "--dump-outputs" in r.stderr


@pytest.mark.gpu
def test_dump_holds_the_last_timed_step(tmp_path):
    from oracle import oracle as orc

    import bench

    d = tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--no-legs", "--no-cpu-baseline", "--preheat-s", "0", "--sustained-s", "0",
              "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    info = line["dump_outputs"]
    a = np.load(d / "linear_power.npy")
    rows = np.asarray(info["rows"])
    assert a.dtype == np.float32 and a.shape == (len(rows), 513, 626) and list(a.shape) == info["shape"]
    assert info["of_rows"] == 256 and np.array_equal(rows, bench.dump_rows(256, 513 * 626 * 4))
    assert os.path.getsize(d / "linear_power.npy") < 64e6
    pick = [0, len(rows) - 1]
    x = np.stack([bench.cfg_signal(int(rows[i])) for i in pick]).astype(np.float64)
    ref = orc.spectrogram_batch(orc.Params(n_fft=1024, hop=256), x)
    err = np.max(np.abs(a[pick] - ref)) / np.max(ref)
    assert err < 1e-5, err

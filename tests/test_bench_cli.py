"""bench.py honours --gpus: a world size that disagrees with --gpus is an error, not a silent
1-GPU run (checked before anything touches a GPU, so it runs here)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_must_match_world_size():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 1 but WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_full_and_dump_outputs_are_options():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_matches_writes_every_record_of_a_small_output(tmp_path):
    """--dump-outputs: at most DUMP_ROWS records are written whole, as float64, with the order-free summary"""
    import numpy as np
    import torch
    b = _bench_module()
    ts = torch.tensor([1700000000000, 1700000000001, 1700000000001], dtype=torch.int64)
    e1 = torch.tensor([5, 7, (1 << 32) + 3], dtype=torch.int64)
    e2 = torch.tensor([6, 9, 11], dtype=torch.int64)
    b.dump_matches(str(tmp_path), 0, 1, ts, e1, e2)
    rows = np.load(tmp_path / "matches.npy")
    summ = np.load(tmp_path / "summary.npy")
    assert rows.dtype == np.float64 and summ.dtype == np.float64
    assert np.array_equal(rows, np.stack([ts.numpy(), e1.numpy(), e2.numpy()], axis=1).astype(np.float64))
    assert summ.tolist() == [3.0, float(int(ts.sum()) % (1 << 32)), 15.0, 26.0]


def test_dump_matches_samples_a_large_output_at_fixed_positions(tmp_path, monkeypatch):
    """above DUMP_ROWS records: the same seeded positions every time, in delivery order, sums over all records"""
    import numpy as np
    import torch
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_ROWS", 100)
    n = 1000
    ts = torch.arange(n, dtype=torch.int64) + 1700000000000
    e1 = torch.arange(n, dtype=torch.int64) * 3
    e2 = e1 + 1
    b.dump_matches(str(tmp_path / "a"), 0, 1, ts, e1, e2)
    b.dump_matches(str(tmp_path / "b"), 0, 1, ts, e1, e2)
    ra, rb = np.load(tmp_path / "a" / "matches.npy"), np.load(tmp_path / "b" / "matches.npy")
    assert np.array_equal(ra, rb) and 50 < len(ra) <= 100
    pos = (ra[:, 1] / 3).astype(np.int64)
    assert np.all(np.diff(pos) > 0)  # distinct positions, ascending: the sample keeps delivery order
    assert np.array_equal(ra[:, 0], (ts.numpy()[pos]).astype(np.float64)) and np.array_equal(ra[:, 2], ra[:, 1] + 1)
    summ = np.load(tmp_path / "a" / "summary.npy")
    assert summ[0] == n and summ[2] == float(int(e1.sum()) % (1 << 32))

"""bench.py --dump-outputs: the last timed step's outputs as float32 .npy files (CPU: the writer on canned tensors; GPU: two plain runs with
different --steps dump the same arrays, and the result line reports exactly the steps it timed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _canned(B=3, nq=10):
    import torch

    g = torch.Generator().manual_seed(7)
    m = torch.randint(0, 100, (B, nq, 4), dtype=torch.int32, generator=g)
    m[..., 3] = torch.full((B, nq), 7.5).view(torch.int32)   # DMatch.distance travels bit-cast in an int32 column
    return {"idx": torch.randint(0, 100, (B, nq, 2), dtype=torch.int32, generator=g),
            "dist": torch.randint(0, 256, (B, nq, 2), dtype=torch.int32, generator=g),
            "matches": m, "count": torch.tensor([3, 0, nq], dtype=torch.int32)[:B]}


def test_dump_is_float32_and_masks_rows_past_the_count(tmp_path):
    import bench

    out = _canned()
    bench.dump_outputs(str(tmp_path), out)
    assert sorted(os.listdir(tmp_path)) == ["count.npy", "dist.npy", "idx.npy", "matches.npy"]
    for name in ("idx", "dist", "count"):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, out[name].numpy())
    m = np.load(tmp_path / "matches.npy")
    assert m.dtype == np.float32 and m.shape == (3, 10, 4)
    assert np.array_equal(m[0, :3, :3], out["matches"][0, :3, :3].numpy()) and (m[0, :3, 3] == 7.5).all()
    assert (m[0, 3:] == -1).all() and (m[1] == -1).all() and (m[2, :, 3] == 7.5).all()


def test_dump_samples_a_fixed_subset_past_the_size_cap(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 400)
    out = _canned()
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out)
    total = 0
    for name in sorted(os.listdir(tmp_path / "a")):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
        total += a.nbytes
    pb = np.load(tmp_path / "a" / "pair_index.npy").astype(int)
    assert 1 <= len(pb) < 3 and total <= 400 + 4 * len(pb)
    assert np.array_equal(np.load(tmp_path / "a" / "idx.npy"), out["idx"].numpy()[pb].astype(np.float32))


def _plain(tmp_path, steps, dump):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--pairs-per-gpu", "4",
           "--n", "2048", "--settle-steps", "0", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1])


@pytest.mark.gpu
def test_plain_runs_dump_the_same_outputs_and_time_exactly_the_given_steps(tmp_path):
    h3 = _plain(tmp_path, 3, tmp_path / "s3")
    h7 = _plain(tmp_path, 7, tmp_path / "s7")
    for h, steps in ((h3, 3), (h7, 7)):
        assert h["steps"] == steps and h["ms_per_step"] > 0 and h["value"] > 0 and h["higher_is_better"] is True
        assert h["roofline"]["kernel"] and h["cpu_baseline"] is None   # no CPU baseline without --full
    names = sorted(os.listdir(tmp_path / "s3"))
    assert names == ["count.npy", "dist.npy", "idx.npy", "matches.npy"]
    for name in names:
        a, b = np.load(tmp_path / "s3" / name), np.load(tmp_path / "s7" / name)
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), name
    count = np.load(tmp_path / "s3" / "count.npy")
    assert count.shape == (4,) and (abs(count - 1024) <= 20).all()

"""bench.py --dump-outputs on CPU: what dump_outputs writes from every rank's arrays (the GPU side only reads the batch's state)."""
import os

import numpy as np


def _parts(n_ranks, n_env, seed=0):
    rng = np.random.default_rng(seed)
    return [{"time": rng.normal(size=n_env).astype(np.float32), "qpos": rng.normal(size=(n_env, 28)).astype(np.float32),
             "qvel": rng.normal(size=(n_env, 27)).astype(np.float32), "qacc_warmstart": rng.normal(size=(n_env, 27)).astype(np.float32)}
            for _ in range(n_ranks)]


def test_dump_writes_every_env_in_rank_order(tmp_path):
    from bench import dump_outputs
    parts = _parts(2, 64)
    dump_outputs(str(tmp_path / "out"), parts)
    assert sorted(os.listdir(tmp_path / "out")) == ["qacc_warmstart.npy", "qpos.npy", "qvel.npy", "time.npy"]
    for k in parts[0]:
        got = np.load(tmp_path / "out" / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, np.concatenate([p[k] for p in parts]))


def test_dump_samples_the_same_envs_above_the_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16 << 10)
    parts = _parts(1, 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), parts)
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))  # (128: the .npy header)
    assert total <= 16 << 10
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and len(idx) > 10 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "qpos.npy"), parts[0]["qpos"][idx.astype(int)])
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))

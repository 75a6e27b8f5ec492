"""bench.py --dump-outputs: the last timed frame as float32 .npy files, whole or as a fixed sample within the size limit.  No GPU needed."""
import os

import numpy as np

import bench


def _sizes(d):
    return {n: os.path.getsize(os.path.join(d, n)) for n in os.listdir(d)}


def test_a_frame_within_the_limit_is_written_whole(tmp_path):
    frame = np.random.default_rng(3).random((6, 10, 3), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), frame)
    got = np.load(tmp_path / "out" / "frame.npy")
    assert set(os.listdir(tmp_path / "out")) == {"frame.npy"}
    assert got.dtype == np.float32 and (got.view(np.uint32) == frame.view(np.uint32)).all()


def test_a_larger_frame_is_a_seeded_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4096 + 20 * 100)
    frame = np.random.default_rng(4).random((64, 64, 3), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sum(_sizes(a).values()) <= bench.DUMP_LIMIT
    px, idx = np.load(a / "frame.npy"), np.load(a / "frame_pixel_index.npy")
    assert px.dtype == np.float32 and idx.dtype == np.float64 and px.shape == (100, 3) and idx.shape == (100,)
    assert (np.diff(idx) > 0).all()
    assert (px == frame.reshape(-1, 3)[idx.astype(np.int64)]).all()
    assert (np.load(b / "frame.npy") == px).all() and (np.load(b / "frame_pixel_index.npy") == idx).all()

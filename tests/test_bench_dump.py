"""bench.py --dump-outputs: the film of the last timed step as float32 .npy, capped at 64 MB by a fixed pixel sample."""
import os

import numpy as np

import bench


def test_small_film_is_written_whole(tmp_path):
    film = np.random.default_rng(3).random((24, 32, 5), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "d"), film)
    assert os.listdir(tmp_path / "d") == ["film.npy"]
    got = np.load(tmp_path / "d" / "film.npy")
    assert got.dtype == np.float32 and np.array_equal(got, film)


def test_large_film_is_a_fixed_sample_under_the_cap(tmp_path):
    film = np.random.default_rng(4).random((2048, 2048, 5), dtype=np.float32)        # 80 MB
    film[..., 0] = np.arange(2048 * 2048, dtype=np.float32).reshape(2048, 2048)     # channel 0 = pixel index (exact in float32)
    bench.dump_outputs(str(tmp_path / "a"), film)
    bench.dump_outputs(str(tmp_path / "b"), film.copy())
    assert os.listdir(tmp_path / "a") == ["film_sample.npy"]
    f = tmp_path / "a" / "film_sample.npy"
    assert os.path.getsize(f) <= bench.DUMP_MAX_BYTES
    a, b = np.load(f), np.load(tmp_path / "b" / "film_sample.npy")
    assert a.dtype == np.float32 and a.shape[1] == 5 and a.shape[0] > 3_000_000
    assert np.array_equal(a, b)
    # every sampled row is a whole pixel of the film, each pixel at most once, in ascending pixel order
    idx = a[:, 0].astype(np.int64)
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(a, film.reshape(-1, 5)[idx])

"""bench.py --dump-outputs: what dump_outputs writes (host tensors here; the bench passes the
device ring)."""
import os

import numpy as np
import torch


def test_small_outputs_are_written_whole_as_float32(tmp_path):
    import bench

    rgb = torch.arange(2 * 3 * 5 * 3, dtype=torch.float32).reshape(2, 3, 5, 3) / 7
    ppm = (torch.arange(2 * 3 * 5 * 3) % 256).to(torch.uint8).reshape(2, 3, 5, 3)
    bench.dump_outputs(str(tmp_path / "out"), {"rgb": rgb, "ppm": ppm})
    got_rgb, got_ppm = np.load(tmp_path / "out" / "rgb.npy"), np.load(tmp_path / "out" / "ppm.npy")
    assert got_rgb.dtype == np.float32 and got_ppm.dtype == np.float32
    assert np.array_equal(got_rgb.view(np.uint32), rgb.numpy().view(np.uint32))
    assert np.array_equal(got_ppm, ppm.numpy().astype(np.float32))


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 2 * 1000)  # 1000 elements for each of two arrays
    a = torch.arange(5001, dtype=torch.float32)
    b = torch.arange(999, dtype=torch.float32)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    one, two = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "two" / "a.npy")
    assert one.shape == (1000,) and np.array_equal(one, two)  # the same elements every run
    assert len(np.unique(one)) > 800 and one.min() < 100 and one.max() > 4900  # spread over the array
    assert np.array_equal(np.load(tmp_path / "one" / "b.npy"), b.numpy())  # under its share: whole
    files = [os.path.join(tmp_path, "one", f) for f in os.listdir(tmp_path / "one")]
    assert sum(os.path.getsize(f) for f in files) <= 4 * 2 * 1000 + 2 * 128  # two .npy headers

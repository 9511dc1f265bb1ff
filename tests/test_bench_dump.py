"""bench.py --dump-outputs: the writer itself (host logic, no GPU)."""
import numpy as np
import torch

import bench


def test_dump_outputs_whole_arrays(tmp_path):
    g = torch.Generator().manual_seed(3)
    arrays = {"rgb": torch.randn(2, 3, 8, 8, generator=g),
              "half": torch.randn(5, 7, generator=g).half(),
              "wide": torch.randn(4, generator=g, dtype=torch.float64)}
    bench.dump_outputs(tmp_path / "d", arrays)
    for name, t in arrays.items():
        a = np.load(tmp_path / "d" / f"{name}.npy")
        want = np.float64 if name == "wide" else np.float32
        assert a.dtype == want and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.to(torch.from_numpy(a).dtype).numpy())


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    g = torch.Generator().manual_seed(4)
    arrays = {"big": torch.randn(3000, generator=g), "small": torch.randn(1000, generator=g)}
    bench.dump_outputs(tmp_path / "a", arrays)
    bench.dump_outputs(tmp_path / "b", arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert sum(a.nbytes for a in got.values()) <= 4000
    assert got["big"].shape == (750,) and got["small"].shape == (250,)
    for n, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{n}.npy"))   # same sample again
        assert np.isin(a, arrays[n].numpy()).all()

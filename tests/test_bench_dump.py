"""bench.py --dump-outputs: what it writes for a step (CPU tensors standing in for the device ones).  CPU only."""
import os

import numpy as np
import torch

import bench
from cstp_amd.train import StepOutput


def _step_output():
    g = torch.Generator().manual_seed(3)
    s = lambda: torch.randn((), generator=g)                                           # noqa: E731
    return StepOutput(s(), s(), [s() for _ in range(6)], s(), None, [torch.randn(4, 5, generator=g) for _ in range(6)])


def test_dump_outputs_writes_float32_npy_with_a_fixed_sample_of_large_arenas(tmp_path):
    n = 3 * bench.DUMP_SAMPLE
    arenas = {"param": torch.arange(n, dtype=torch.float32), "grad": torch.arange(n, dtype=torch.float32) * 2,
              "target": torch.arange(1000, dtype=torch.float32), "buffers": torch.ones(40, dtype=torch.float64)}
    out = _step_output()
    bench.dump_outputs(str(tmp_path / "a"), out, arenas)
    bench.dump_outputs(str(tmp_path / "b"), out, arenas)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["loss_total.npy", "loss_byol.npy", "ce.npy", "grad_norm.npy", "buffers.npy", "param.npy",
                            "grad.npy", "target.npy"] + ["logits_%d.npy" % i for i in range(6)])      # no ntxent: it is None
    total = 0
    for name in names:
        a, b = np.load(str(tmp_path / "a" / name)), np.load(str(tmp_path / "b" / name))
        assert a.dtype == np.float32 and np.array_equal(a, b), name                    # same inputs -> same files
        total += a.nbytes
    assert total <= 64 << 20
    p = np.load(str(tmp_path / "a" / "param.npy"))
    assert p.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(p) >= 0) and p.max() < n   # sorted indices into the arena
    assert np.array_equal(np.load(str(tmp_path / "a" / "target.npy")), np.arange(1000))  # small arenas whole
    assert np.load(str(tmp_path / "a" / "ce.npy")).shape == (6,)
    assert np.array_equal(np.load(str(tmp_path / "a" / "logits_2.npy")), out.logits[2].numpy())

"""bench.py --dump-outputs on the host side: the shared 64 MB budget, the fixed seeded sample of arrays over their share,
float32 on disk.  The GPU test (test_pipeline_gpu.py) runs the real thing on a config small enough to dump whole."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(monkeypatch):
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return bench


def test_dump_shares_the_budget_and_samples_with_a_fixed_seed(tmp_path, monkeypatch):
    bench = _bench(monkeypatch)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096 + 4 * 5000)   # room for 5000 floats after the header reserve
    B = 50
    g = torch.Generator().manual_seed(1)
    flat = torch.randn(B * 38, generator=g)
    outs = {"color": torch.randn(1, 40, 30, generator=g), "radii": torch.arange(900, dtype=torch.int32),
            "all_map": torch.randn(4, 40, 30, generator=g), "invdepth": torch.randn(1, 40, 30, generator=g)}
    pipe = SimpleNamespace(w=SimpleNamespace(args=SimpleNamespace(mode="view"), B=B), last_step_gradient=lambda: flat,
                           last_outputs=outs)
    man = bench.dump_outputs(pipe, str(tmp_path / "d"))["arrays"]
    got = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in man}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.size for a in got.values()) <= 5000 and "sampled" not in man["last_view_radii"]
    # the small arrays are whole and exact
    np.testing.assert_array_equal(got["grad_curve_points"], flat[:12 * B].view(B, 4, 3).numpy())
    np.testing.assert_array_equal(got["grad_width"], flat[12 * B:13 * B].view(B, 1).numpy())
    np.testing.assert_array_equal(got["grad_opacity"], flat[13 * B:14 * B].view(B, 1).numpy())
    assert "sampled" not in man["grad_curve_points"]
    # the big ones are the documented sample of the flattened array
    for n in ("all_map", "color"):
        key = "last_view_" + n
        k = man[key]["sampled"]
        assert man[key]["shape"] == list(outs[n].shape) and got[key].shape == (k,)
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(outs[n].numel(), k, replace=False))
        np.testing.assert_array_equal(got[key], outs[n].reshape(-1).numpy()[idx])
    # the same call again writes the same files
    bench.dump_outputs(pipe, str(tmp_path / "e"))
    for n in man:
        np.testing.assert_array_equal(np.load(tmp_path / "e" / (n + ".npy")), got[n])

"""bench.py --dump-outputs, host side: the arrays written, their dtype, the
seeded row sample of an output larger than its share of the dump, and the
size of a dump of the headline batch (no GPU: the buffers are CPU tensors)."""
import os
import types

import numpy as np
import torch

import bench


def _fake_squares(k, n, seed):
    w = 2 * k
    g = torch.Generator().manual_seed(seed)
    u8 = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)  # noqa: E731
    return types.SimpleNamespace(k=k, n=n, eds=u8(n, w * w * 512), row_roots=u8(n, w, 90), col_roots=u8(n, w, 90),
                                 dah=u8(n, 32), status=torch.zeros(n, dtype=torch.int32))


def test_dump_outputs_arrays(tmp_path):
    ds = _fake_squares(16, 5, 1)  # 5 * 32 * 32 = 5120 EDS shares: more than the 4096 kept
    bench.dump_outputs(str(tmp_path / "a"), ds)
    bench.dump_outputs(str(tmp_path / "b"), ds)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["col_roots.npy", "dah.npy", "eds_sample.npy", "row_roots.npy", "status.npy"]
    a = {f: np.load(tmp_path / "a" / f) for f in names}
    assert all(v.dtype == np.float32 for v in a.values())
    for f in names:  # the same rows, run after run
        assert np.array_equal(a[f], np.load(tmp_path / "b" / f)), f
    assert np.array_equal(a["row_roots.npy"], ds.row_roots.view(-1, 90).numpy().astype(np.float32))
    assert np.array_equal(a["col_roots.npy"], ds.col_roots.view(-1, 90).numpy().astype(np.float32))
    assert np.array_equal(a["dah.npy"], ds.dah.numpy().astype(np.float32))
    assert a["status.npy"].shape == (5, 1) and not a["status.npy"].any()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED + 4).choice(5120, 4096, replace=False))
    assert len(set(idx.tolist())) == 4096
    assert np.array_equal(a["eds_sample.npy"], ds.eds.view(-1, 512).numpy()[idx].astype(np.float32))


def test_dump_stays_under_64_mb():
    """Whatever the batch, no array keeps more than DUMP_ROWS rows: the float32
    bytes of a full dump, .npy headers included, stay under 64 MB."""
    width = {"row_roots": 90, "col_roots": 90, "dah": 32, "status": 1, "eds_sample": 512}
    assert set(width) == set(bench.DUMP_ROWS)
    assert sum(4 * bench.DUMP_ROWS[n] * width[n] + 128 for n in width) < 64e6
    # the headline batch (256 squares of k = 128) keeps every root, DAH and status
    assert bench.DUMP_ROWS["row_roots"] >= 256 * 256 and bench.DUMP_ROWS["dah"] >= 256

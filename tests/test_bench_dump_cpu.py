"""CPU: bench.py --dump-outputs writes float arrays, whole below the byte budget and as one fixed
seeded sample of rows (the same rows of every array, the same on every run) above it."""
import numpy as np

import bench


def tables(n=40):
    rng = np.random.default_rng(1)
    lat = rng.integers(1, 2**40, size=(n, n), dtype=np.uint64)
    loss = rng.random((n, n), dtype=np.float32)
    return lat, loss


def test_dump_whole_below_budget(tmp_path):
    lat, loss = tables()
    w = bench.dump_outputs(str(tmp_path / "a"), {"latency_ns": lat, "packet_loss": loss})
    a, b = np.load(tmp_path / "a" / "latency_ns.npy"), np.load(tmp_path / "a" / "packet_loss.npy")
    assert a.dtype == np.float64 and b.dtype == np.float32
    assert np.array_equal(a.astype(np.uint64), lat) and np.array_equal(b, loss)
    assert w["latency_ns"]["sampled_of"] is None and w["packet_loss"]["shape"] == [40, 40]


def test_dump_sampled_rows_fixed(tmp_path, monkeypatch):
    lat, loss = tables()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 40 * 40 * 12 // 4)
    out = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"latency_ns": lat, "packet_loss": loss})
        out.append((np.load(tmp_path / d / "latency_ns.npy"), np.load(tmp_path / d / "packet_loss.npy")))
    (a0, b0), (a1, b1) = out
    assert a0.shape == b0.shape == (10, 40)
    assert a0.nbytes + b0.nbytes <= bench.DUMP_BUDGET
    assert np.array_equal(a0, a1) and np.array_equal(b0, b1)
    # the same rows of both tables, in table order
    rows = [int(np.flatnonzero((lat == r.astype(np.uint64)).all(axis=1))[0]) for r in a0]
    assert rows == sorted(rows) and len(set(rows)) == 10
    assert np.array_equal(b0, loss[rows])

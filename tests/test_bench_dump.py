"""bench.py --dump-outputs (CPU): what the last timed step returned -- every stream's length and a fixed sample of the streams' bytes --
lands in DIR/*.npy as float32 / float64, within 64 MB, the same files for the same streams, every sampled byte as it was."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _Stream:
    """stands in for the library's StreamBytes (len() and view())"""

    def __init__(self, data):
        self.data = data

    def __len__(self):
        return len(self.data)

    def view(self):
        return memoryview(self.data)


def test_dump_is_bounded_fixed_and_exact(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(7)
    # the headline's shape: 320 GOP streams of ~460 KB (590 MB as float32, far over the budget)
    outs = [_Stream(rng.integers(0, 256, size=int(rng.integers(440000, 480000)), dtype=np.uint8).tobytes()) for _ in range(320)]
    files = {}
    for run in ("a", "b"):
        d = tmp_path / run
        bench.dump_outputs(str(d), outs)
        names = sorted(os.listdir(d))
        assert names == ["stream_bytes.npy", "stream_index.npy", "stream_lengths.npy"]
        assert sum(os.path.getsize(d / n) for n in names) <= 64 * 10 ** 6
        files[run] = {n: np.load(d / n) for n in names}
    for n in files["a"]:
        assert files["a"][n].dtype in (np.float32, np.float64)
        assert np.array_equal(files["a"][n], files["b"][n]), n
    f = files["a"]
    assert np.array_equal(f["stream_lengths.npy"], [len(o) for o in outs])
    idx = f["stream_index.npy"].astype(int)
    assert len(idx) > 16 and list(idx) == sorted(set(idx))
    want = np.concatenate([np.frombuffer(outs[s].data, dtype=np.uint8) for s in idx])
    assert np.array_equal(f["stream_bytes.npy"], want.astype(np.float32))


def test_small_output_is_dumped_whole(tmp_path):
    bench = _bench()
    outs = [_Stream(bytes([s]) * (100 + s)) for s in range(8)]
    bench.dump_outputs(str(tmp_path), outs, prefix="rank1_", budget=10 ** 6)
    assert np.array_equal(np.load(tmp_path / "rank1_stream_index.npy"), np.arange(8))
    assert np.array_equal(np.load(tmp_path / "rank1_stream_bytes.npy"), np.concatenate([np.full(100 + s, s) for s in range(8)]))

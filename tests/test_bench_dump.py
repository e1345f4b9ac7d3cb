"""bench.py --dump-outputs on CPU: the arrays a dump holds are float64 and exact, the sample is the
same from call to call, a large output stays under the 64 MB a dump may take, and the whole-output
sums see a change the sample misses."""
import os

import numpy as np

import bench
import kvreplay as K


def _tuples(n):
    t = np.zeros(n, dtype=K.TUPLE_DTYPE)
    t["rec_off"] = np.arange(n, dtype=np.uint64) * 1037
    t["seg_idx"] = np.arange(n) >> 16
    t["crc32"] = (np.arange(n, dtype=np.uint64) * 2654435761) & 0xFFFFFFFF
    t["op"] = np.arange(n) % 2
    return t


def test_sample_index_is_fixed_and_ascending():
    a, b = bench.sample_index(5_000_000, bench.DUMP_ROWS), bench.sample_index(5_000_000, bench.DUMP_ROWS)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_ROWS
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 5_000_000
    assert np.array_equal(bench.sample_index(100, bench.DUMP_ROWS), np.arange(100))


def test_tuple_dump_is_exact_and_bounded(tmp_path):
    t = _tuples(bench.DUMP_ROWS + 1000)
    bench.dump_outputs(str(tmp_path), 0, 1, {"summary": [0, len(t), 0], **bench.tuple_arrays("tuples", t)})
    names = sorted(os.listdir(tmp_path))
    assert names == ["summary.npy", "tuples.npy", "tuples_rows.npy", "tuples_sums.npy"]
    arrs = {n[:-4]: np.load(tmp_path / n) for n in names}
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64_000_000
    rows = arrs["tuples_rows"].astype(np.int64)
    assert arrs["tuples"].shape == (bench.DUMP_ROWS, len(K.TUPLE_DTYPE.names))
    for i, f in enumerate(K.TUPLE_DTYPE.names):
        assert np.array_equal(arrs["tuples"][:, i].astype(np.uint64), t[f][rows].astype(np.uint64))
        assert int(arrs["tuples_sums"][i]) == int(t[f].astype(np.uint64).sum()) % (1 << 48)
    # a tuple outside the sample still changes the sums
    miss = int(np.setdiff1d(np.arange(len(t)), rows)[0])
    t["crc32"][miss] ^= 1
    again = bench.tuple_arrays("tuples", t)
    assert np.array_equal(again["tuples"], arrs["tuples"])
    assert again["tuples_sums"] != list(arrs["tuples_sums"].astype(np.int64))


def test_byte_dump_and_rank_prefix(tmp_path):
    b = (np.arange(3_000_000, dtype=np.uint64) * 7 % 251).astype(np.uint8)
    d = bench.byte_arrays("bytes", b)
    assert np.array_equal(d["bytes"], b[d["bytes_at"]]) and len(d["bytes"]) == bench.DUMP_BYTES
    assert d["bytes_hist"].sum() == len(b) and len(d["bytes_hist"]) == 256
    bench.dump_outputs(str(tmp_path), 1, 2, d)
    assert sorted(os.listdir(tmp_path)) == ["rank1_bytes.npy", "rank1_bytes_at.npy", "rank1_bytes_hist.npy"]
    assert sum(np.load(tmp_path / n).nbytes for n in os.listdir(tmp_path)) <= 64_000_000

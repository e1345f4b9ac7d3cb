"""The host side of the write path (no GPU): kvh_encode_batch, and kvs_put_many / kvs_set /
kvs_delete / kvs_list_keys on a store opened without a context (kvs_open_ex with ctx = NULL).

Expected values never come from the code under test (put_model.py): the Python framing, zlib.crc32,
a dict model, and the oracle's replay + fold of the directory's files.
"""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import kvreplay as K
import oracle_py as O
import put_model as M
from test_get_many_host import open_host_only
from test_open_index import crc_collisions


def raw_encode(o, keys, koff, vals, voff, cap, seg_idx=0, base_off=0):
    """kvh_encode_batch through ctypes over a canary-filled output: rc, out, out_len."""
    _, host = K.native()
    o = np.asarray(o, dtype=np.uint8)
    keys, vals = np.frombuffer(bytes(keys), dtype=np.uint8), np.frombuffer(bytes(vals), dtype=np.uint8)
    koff, voff = np.asarray(koff, dtype=np.uint64), np.asarray(voff, dtype=np.uint64)
    out = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    tup = np.zeros(max(len(o), 1), dtype=K.TUPLE_DTYPE)
    ol = C.c_uint64(12345)
    rc = host.kvh_encode_batch(o.ctypes.data, keys.ctypes.data if keys.size else None, koff.ctypes.data,
                               vals.ctypes.data if vals.size else None, voff.ctypes.data, len(o), seg_idx, base_off,
                               out.ctypes.data, cap, C.byref(ol), tup.ctypes.data)
    return rc, out, int(ol.value)


def test_val_lens_are_the_get_tests():
    import test_get_batch
    assert M.VAL_LENS == test_get_batch.VAL_LENS


@pytest.mark.parametrize("dels", [False, True])
def test_encode_matches_the_framing(dels):
    ops = M.edge_ops(seed=3, dels=dels)
    assert {len(k) for k, _ in ops} >= set(range(41)) | {300}
    assert {len(v) for _, v in ops if v is not None} >= set(M.VAL_LENS)
    assert any(v is None for _, v in ops) == dels
    want = M.frame(ops)
    r = K.host_encode_batch(ops, seg_idx=3, base_off=77)
    assert r.status == K.OK and r.out_len == len(want)
    assert r.data == want
    assert np.array_equal(r.tuples, M.oracle_tuples(want, 3, 77))
    assert [int(x) for x in r.tuples["crc32"]] == M.etags(ops)
    assert [int(x) for x in r.tuples["key_tag"]] == [zlib.crc32(k) for k, _ in ops]
    assert (r.tuples["flags"] == 0).all()
    # one byte short: KVR_CAPACITY with the size, nothing written
    o, keys, koff, vals, voff = K.op_arena(ops)
    rc, out, ol = raw_encode(o, keys.tobytes(), koff, vals.tobytes(), voff, len(want) - 1)
    assert rc == K.CAPACITY and ol == len(want) and (out == 0xA5).all()
    rc, out, ol = raw_encode(o, keys.tobytes(), koff, vals.tobytes(), voff, len(want) + 8)
    assert rc == K.OK and out[: len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()
    assert K.host_encode_batch([]).status == K.OK


def test_encode_rejects_bad_input():
    for bad in M.BAD_UTF8:
        assert not O.utf8_check(bad)[0]
        for key in (bad, b"ab" + bad, bad + b"z", b"\xd0\xba" + bad):
            ops = [(b"fine", b"v"), (key, b"value"), (b"later", None)]
            o, keys, koff, vals, voff = K.op_arena(ops)
            rc, out, _ = raw_encode(o, keys.tobytes(), koff, vals.tobytes(), voff, 256)
            assert rc == K.EINVAL and (out == 0xA5).all(), key
    for k in M.UTF8_KEYS:
        assert O.utf8_check(k)[0]
    cases = {
        "a DEL with a value": ([0, 1], b"abcd", [0, 2, 4], b"xy", [0, 1, 2]),
        "a bad op byte": ([0, 2], b"abcd", [0, 2, 4], b"x", [0, 1, 1]),
        "key offsets decrease": ([0, 0, 0], b"12345678", [0, 5, 3, 8], b"", [0, 0, 0, 0]),
        "value offsets decrease": ([0, 0, 0], b"abc", [0, 1, 2, 3], b"12345678", [0, 5, 3, 8]),
        "a 4-GiB key": ([0], b"a", [0, 1 << 32], b"", [0, 0]),
    }
    for name, (o, keys, koff, vals, voff) in cases.items():
        rc, out, _ = raw_encode(o, keys, koff, vals, voff, 256)
        assert rc == K.EINVAL and (out == 0xA5).all(), name


def test_host_index_update_matches_the_oracle():
    """kvh_index_update over the host-built table of the collision store: the live list after a
    batch is the oracle's over the segments plus the batch's bytes."""
    from test_open_index import check_index, collision_store
    segs, pairs = collision_store()
    want0, model, order = M.oracle_state(segs)
    idx = K.Index(want0, K.index_build_host(want0), segs, None)
    ops = [(k, b"over") for k in order[::3]] + [(k, None) for k in order[1::3]] + [(b"absent", None)]
    for j, (a, c) in enumerate(pairs):
        ops += [(a, b"a%d" % j), (c, None if j % 2 else b"c%d" % j)]
    ops += [(b"dup", b"1"), (b"dup", None), (b"dup2", None), (b"dup2", b""), (order[2], b"x"), (order[2], b"y")]
    r = K.host_encode_batch(ops, seg_idx=len(segs))
    assert r.status == K.OK and r.data == M.frame(ops)
    idx2 = K.host_index_update(idx, segs + [r.data], r.tuples, [k for k, _ in ops])
    M.apply(model, ops)
    want, od, _ = M.oracle_state(segs + [r.data])
    assert od == model
    check_index(idx2, segs + [r.data], want, [k for k, _ in ops if k not in model])


def check_store(s, d, model, mentioned, batches, seg_id):
    """The store against the dict model, the framing and the oracle's view of the directory."""
    keys = sorted(mentioned)
    assert [s.get(k) for k in keys] == [model.get(k) for k in keys]
    assert s.get_many(keys) == [model.get(k) for k in keys]
    st = s.stats()
    assert st.num_keys == len(model) and st.total_bytes == sum(len(v) for v in model.values())
    assert st.active_segment_id == seg_id
    path = os.path.join(str(d), "segment-%d.dat" % seg_id)
    data = open(path, "rb").read()
    assert data == b"".join(M.frame(b) for b in batches)
    files = K.discover(str(d))
    ids = [i for i, _ in files]
    segs = [open(p, "rb").read() for _, p in files]
    want, od, order = M.oracle_state(segs)
    assert od == model
    assert s.list_keys() == order                      # the store's live list is the oracle's, in order
    for w, k in zip(want, order):
        loc = (ids[int(w["seg_idx"])], int(w["rec_off"]) + 9 + int(w["key_len"]), int(w["val_len"]))
        assert s.locate(k) == loc
    for k in keys:
        if k not in model:
            assert s.locate(k) is None


def put_batches():
    a, c = crc_collisions(b"", 400_000, 1)[0]
    assert a != c and zlib.crc32(a) == zlib.crc32(c)
    big = np.random.RandomState(5).randint(0, 256, 5000, dtype=np.uint8).tobytes()
    b1 = [(a, b"A1"), (c, b"C1"), (b"k1", b"v1"), (b"k2", b"v2"), (b"k3", b""),
          (b"dup", b"first"), (b"dup", b"second"),          # SET, SET
          (b"sd", b"x"), (b"sd", None),                      # SET, DEL
          (b"ds", None), (b"ds", b"y"),                      # DEL, SET
          (b"absent", None), (b"big", big)]
    b2 = [(b"k1", b"v1b"), (b"k2", None), (b"nope", None), (b"sd", b"back"),   # overwrite, DELs, SET after a DEL
          (a, None), (c, b"C2"), (b"dup", None), (b"dup", b"third"), (b"k3", b"")]
    b3 = [(b"k2", b"again"), (b"k3", b"now-nonempty"), (b"ds", None), (M.UTF8_KEYS[0], b"utf8"), (b"", b"empty-key"),
          (c, None), (a, b"A3"), (b"big", None)]
    return [b1, b2, b3]


def test_store_put_many_on_the_host(tmp_path):
    d = tmp_path / "store"
    s = open_host_only(d)
    try:
        assert s.stats().active_segment_id == 1 and s.list_keys() == []
        model, mentioned, done = {}, set(), []
        for b in put_batches():
            assert s.put_many(b) == M.etags(b)
            M.apply(model, b)
            mentioned |= {k for k, _ in b}
            done.append(b)
            check_store(s, d, model, mentioned, done, 1)
        assert s.put_many([]) == []
        with pytest.raises(K.NativeError):
            s.put_many([(b"ok", b"v"), (M.BAD_UTF8[0], b"v")])
        check_store(s, d, model, mentioned, done, 1)     # the rejected batch changed nothing
    finally:
        s.close()


def test_set_and_delete_are_batches_of_one(tmp_path):
    d = tmp_path / "store"
    s = open_host_only(d)
    try:
        ops = [(b"a", b"1"), (b"b", b"22"), (b"a", None), (b"never", None), (b"b", b""), (b"a", b"333")]
        model, done = {}, []
        for k, v in ops:
            if v is None:
                s.delete(k)
            else:
                assert s.set(k, v) == zlib.crc32(v)
            M.apply(model, [(k, v)])
            done.append([(k, v)])
            check_store(s, d, model, {k for k, _ in ops}, done, 1)
    finally:
        s.close()

"""kvs_get_many / KVStore.get_many: the store's multi-get, on the device while the context still
holds the store's key table, else a host loop over kvr_index_find — the same answers both ways,
which are KVStore.get's (engine.rs:200-202) key by key.

The CPU tests need no GPU: argument checks, and an empty store opened without a context
(kvstore_host.h: kvs_open_ex with ctx = NULL), which only the host path can answer.
"""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import kvreplay as K
import oracle_py as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def open_host_only(path):
    _, host = K.native()
    h = C.c_void_p()
    err = K.Error()
    msg = C.create_string_buffer(4096)
    rc = host.kvs_open_ex(str(path).encode(), None, 0, C.byref(h), C.byref(err), msg, len(msg))
    assert rc == K.OK
    return K.KVStore(h, None)


def raw_get_many(store, ctx, keys, vals_cap, offs=None, null=()):
    _, host = K.native()
    arena, ko = K.key_arena(keys)
    if offs is not None:
        ko = np.asarray(offs, dtype=np.uint64)
    n = len(ko) - 1
    idx = np.full(max(n, 1), -7, dtype=np.int64)
    voff = np.full(n + 1, 77, dtype=np.uint64)
    vals = np.full(max(vals_cap, 1), 0xA5, dtype=np.uint8)
    vb = C.c_uint64(999)
    rc = host.kvs_get_many(store._h if store else None, ctx,
                           None if "keys" in null or not arena.size else arena.ctypes.data,
                           None if "key_off" in null else ko.ctypes.data, n,
                           None if "live_idx" in null else idx.ctypes.data,
                           None if "val_off" in null else voff.ctypes.data,
                           None if "vals" in null else vals.ctypes.data, vals_cap,
                           None if "val_bytes" in null else C.byref(vb))
    return rc, idx[:n], voff, vals, int(vb.value)


# ---- CPU -----------------------------------------------------------------------------------------
def test_get_batch_needs_a_context():
    rep, _ = K.native()
    vb = C.c_uint64()
    assert rep.kvr_get_batch(None, None, None, 0, 0, None, None, None, 0, C.byref(vb), None, None) == K.EINVAL
    assert rep.kvr_index_epoch(None) == 0
    assert rep.kvr_last_get_stats(None, None) == K.EINVAL


def test_get_many_empty_store_on_the_host(tmp_path):
    d = tmp_path / "emptied"
    shutil.copytree(os.path.join(GOLD, "persistence"), d)
    for f in d.glob("segment-*.dat"):
        f.write_bytes(b"")                       # an emptied store: every segment replays to nothing
    for path in (d, tmp_path / "new" / "store"):
        s = open_host_only(path)
        try:
            assert s.stats().num_keys == 0
            keys = [b"session", "counter", b"", b"x" * 300]
            assert s.get_many(keys) == [None] * 4 == [s.get(k) for k in keys]
            assert s.get_many(keys, device=False) == [None] * 4
            assert s.get_many([]) == []
        finally:
            s.close()


def test_get_many_argument_checks(tmp_path):
    s = open_host_only(tmp_path / "store")
    try:
        keys = [b"a", b"bc", b""]
        rc, idx, voff, vals, vb = raw_get_many(s, None, keys, 16)
        assert rc == K.OK and list(idx) == [-1, -1, -1] and list(voff) == [0, 0, 0, 0] and vb == 0
        assert (vals == 0xA5).all()
        rc, idx, voff, vals, vb = raw_get_many(s, None, keys, 0, null=("vals",))   # no room needed, none given
        assert rc == K.OK and vb == 0
        rc, _, voff, _, vb = raw_get_many(s, None, [], 0)
        assert rc == K.OK and vb == 0 and voff[0] == 0
        assert raw_get_many(None, None, keys, 16)[0] == K.EINVAL
        for missing in ("key_off", "live_idx", "val_off", "val_bytes", "vals", "keys"):
            assert raw_get_many(s, None, keys, 16, null=(missing,))[0] == K.EINVAL, missing
        assert raw_get_many(s, None, [b"12345678"], 16, offs=[0, 5, 3, 8])[0] == K.EINVAL   # decreasing
        assert raw_get_many(s, None, [b"12345678"], 16, offs=[0, 1 << 32])[0] == K.EINVAL   # a 4-GiB key
    finally:
        s.close()


@pytest.mark.parametrize("threads", [0, 1, 4, 500])
def test_host_loop_matches_the_oracle(threads):
    """kvh_get_many (the loop kvs_get_many falls back to) over the host-built table of the
    collision store: live_idx and values equal the oracle's map, on any number of threads."""
    from test_open_index import collision_store
    segs, pairs = collision_store()
    rc, t, _ = O.replay(segs)
    assert rc == 0
    live, nk, _ = O.fold_live(segs, t)
    want = t[live]
    d = {}
    for j, w in enumerate(want):
        ko = int(w["rec_off"]) + 5
        vo = ko + int(w["key_len"]) + 4
        s = segs[int(w["seg_idx"])]
        d[s[ko: ko + int(w["key_len"])]] = (j, s[vo: vo + int(w["val_len"])])
    idx = K.Index(want, K.index_build_host(want), segs, None)
    q = list(d) + [k for p in pairs for k in p] + [b"", b"never-written"] + list(d)[::-1]
    r = K.host_get_many(idx, q, threads=threads)
    assert r.status == K.OK
    assert [int(x) for x in r.live_idx] == [d[k][0] if k in d else -1 for k in q]
    assert [r.value(i) for i in range(len(q))] == [d[k][1] if k in d else None for k in q]
    vb = sum(len(d[k][1]) for k in q if k in d)
    assert r.val_bytes == vb and int(r.val_off[-1]) == vb
    assert K.host_get_many(idx, q, threads=threads, vals_cap=vb - 1).status == K.CAPACITY


# ---- GPU -----------------------------------------------------------------------------------------
def _golden_keys(d):
    names = sorted((n for n in os.listdir(d) if n.startswith("segment-")), key=lambda n: int(n[8:-4]))
    segs = [open(os.path.join(d, n), "rb").read() for n in names]
    rc, t, _ = O.replay(segs)
    assert rc == 0
    live, nk, _ = O.fold_live(segs, t)
    ks = [bytes(segs[w["seg_idx"]][w["rec_off"] + 5: w["rec_off"] + 5 + w["key_len"]]) for w in t]
    live_keys = [k for k, l in zip(ks, live) if l]
    assert nk == len(live_keys) > 0
    return live_keys, sorted(set(ks) - set(live_keys))


@pytest.mark.gpu
def test_get_many_matches_get(gctx, tmp_path):
    d = tmp_path / "persisted_store"
    shutil.copytree(os.path.join(GOLD, "persistence"), d)
    live_keys, dead_keys = _golden_keys(str(d))
    s = K.KVStore.open(str(d), gctx)
    try:
        assert s.open_stats().path == K.PATH_DEVICE_INDEX
        keys = live_keys + dead_keys + [b"no-such-key", b"", live_keys[0], b"z" * 300] + live_keys[::-1]
        for stage in ("opened", "compacted"):
            want = [s.get(k) for k in keys]
            assert want[: len(live_keys)] != [None] * len(live_keys) and want[len(live_keys)] is None
            epoch = gctx.index_epoch()
            assert epoch != 0
            assert s.get_many(keys) == want                     # the device path
            assert gctx.last_get_stats().n_keys == len(keys)    # (it did run on the device)
            assert s.get_many(keys, device=False) == want       # the host loop
            assert gctx.replay([b""]).status == K.OK            # the context used for something else:
            assert gctx.index_epoch() == 0                      # no table of this store's any more
            before = gctx.last_get_stats().n_keys
            assert s.get_many(keys) == want                     # -> the host loop again
            assert s.get_many([]) == []
            assert gctx.last_get_stats().n_keys == before
            if stage == "opened":
                s.compact()
                assert gctx.index_epoch() not in (0, epoch)
    finally:
        s.close()

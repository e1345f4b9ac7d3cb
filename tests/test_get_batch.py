"""kvr_get_batch: KVStore::get (engine.rs:200-202) for many keys at once on the device.

Expected answers never come from the code under test: oracle_py replays the segments
(engine.rs:79-154), folds them (engine.rs:137 insert / :141 remove) and the live tuples give a
Python dict key bytes -> (index into the live list, value bytes).  A query's live_idx and value
must equal the dict's entry, or -1 / None when the key is not in it.

Stores:
  collision store   test_open_index.collision_store: CRC-32-colliding key pairs (short, and long with
                    equal 16-B prefixes) with overwrites, empty values and DELs (IX_DEAD slots).
  edge store        SETs only; keys of 1 .. 40 bytes (values start at every address mod 16) and one
                    of 300 bytes; value lengths around every boundary of the gather (16-B words,
                    the 4-KiB round) and of the verify pass (4-KiB chunks); segment lengths that
                    are no multiple of 4, the last value ending on the segment's last byte.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import kvreplay as K
import oracle_py as O
from test_open_index import DEAD, collision_store, rec_set

pytestmark = pytest.mark.gpu

VAL_LENS = [0, 1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 4096 * 2 + 17]
KEY300 = b"K" * 300
MISS300 = b"K" * 299 + b"L"


def oracle_map(segs):
    """(live tuples in (segment, offset) order, {key: (live index, value)}) from the oracle."""
    rc, t, _ = O.replay(segs)
    assert rc == 0
    live, nk, _ = O.fold_live(segs, t)
    want = t[live]
    d = {}
    for j, w in enumerate(want):
        s, ko = segs[int(w["seg_idx"])], int(w["rec_off"]) + 5
        vo = ko + int(w["key_len"]) + 4
        d[bytes(s[ko: ko + int(w["key_len"])])] = (j, bytes(s[vo: vo + int(w["val_len"])]))
    assert len(d) == nk
    return want, d


@functools.lru_cache(maxsize=None)
def coll():
    segs, pairs = collision_store()
    want, d = oracle_map(segs)
    live = list(d)
    changed = [k[:-1] + bytes([k[-1] ^ 1]) for k in live]
    q = live + [k for p in pairs for k in p] + [b"", b"never-written"] + changed + live
    return segs, want, d, q


@functools.lru_cache(maxsize=None)
def edge():
    rng = np.random.RandomState(1234)
    keys = [bytes(97 + (n * 5 + i) % 26 for i in range(n)) for n in range(1, 41)] + [KEY300]
    recs = [rec_set(k, rng.randint(0, 256, VAL_LENS[i % len(VAL_LENS)], dtype=np.uint8).tobytes())
            for i, k in enumerate(keys)]
    # the 41 records in three segments; the last record of each is a SET, so its value ends on the
    # segment's last byte.  The record order is the first seeded shuffle that gives segment lengths
    # that are no multiple of 4 and values starting at every offset mod 16 (the base offsets of the
    # placement rotate those).
    for seed in range(1000):
        p = [recs[j] for j in np.random.RandomState(seed).permutation(len(recs))]
        segs = [b"".join(p[:13]), b"".join(p[13:29]), b"".join(p[29:])]
        want, d = oracle_map(segs)
        starts = {(int(w["rec_off"]) + 9 + int(w["key_len"])) % 16 for w in want}
        if all(len(s) % 4 for s in segs) and starts == set(range(16)):
            break
    else:
        raise AssertionError("no record order with the wanted alignments")
    assert len(d) == 41
    return segs, want, d, keys


def dev_place(segs, base_off, fill=0):
    """The segments in one torch buffer, segment i at an address = base_off (mod 256), as
    test_piece_mode._dev_place does; every byte outside a segment is fill."""
    torch = pytest.importorskip("torch")
    tot = sum((len(s) + 511) & ~255 for s in segs) + 512
    buf = torch.full((tot,), fill, dtype=torch.uint8, device="cuda")
    ptrs, off, offs = [], base_off, []
    for s in segs:
        buf[off: off + len(s)] = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda()
        ptrs.append((buf.data_ptr() + off, len(s)))
        offs.append(off)
        off = ((off + len(s) + 255) & ~255) + base_off
    torch.cuda.synchronize()
    return buf, ptrs, offs


def check(r, queries, d):
    assert r.status == K.OK
    assert [int(x) for x in r.live_idx] == [d[q][0] if q in d else -1 for q in queries]
    assert [r.value(i) for i in range(len(queries))] == [d[q][1] if q in d else None for q in queries]
    lens = [len(d[q][1]) if q in d else 0 for q in queries]
    assert [int(x) for x in r.val_off] == [0] + list(np.cumsum(lens))
    assert r.val_bytes == sum(lens) and r.stats.n_keys == len(queries)
    assert r.stats.n_found == sum(q in d for q in queries) and r.stats.val_bytes == sum(lens)


def raw_get(ctx, queries, flags, vals_cap, vals=True, offs=None):
    """kvr_get_batch through ctypes with host buffers (no retry): rc, live_idx, val_off, vals (0xA5
    where nothing was written), val_bytes."""
    rep, _ = K.native()
    arena, ko = K.key_arena(queries)
    if offs is not None:
        ko = np.asarray(offs, dtype=np.uint64)
    n = len(ko) - 1
    idx = np.full(max(n, 1), -7, dtype=np.int64)
    voff = np.full(n + 1, 77, dtype=np.uint64)
    out = np.full(max(vals_cap, 1), 0xA5, dtype=np.uint8)
    vb = C.c_uint64(12345)
    rc = rep.kvr_get_batch(ctx.h, arena.ctypes.data if arena.size else None, ko.ctypes.data, n, flags, idx.ctypes.data,
                           voff.ctypes.data, out.ctypes.data if vals else None, vals_cap, C.byref(vb), None, None)
    return rc, idx[:n], voff, out, int(vb.value)


# ---- 1. parity on the collision store --------------------------------------------------------------
@pytest.mark.parametrize("path", ["lds", "global"])
def test_get_parity_collisions(gctx, monkeypatch, path):
    """Every live key, both keys of every colliding pair, b"", an unwritten key, every live key with
    its last byte changed and the live keys again (duplicates) in one batch: live_idx equals
    Index.find and the oracle's, values equal the oracle's, in both table layouts."""
    if path == "global":
        monkeypatch.setenv("KVR_FOLD_GLOBAL", "1")
    segs, want, d, q = coll()
    idx = gctx.replay_index(segs)
    assert np.array_equal(idx.live, want)
    assert (idx.slots == DEAD).any()                       # misses probe past deleted keys' entries
    assert any(v == b"" for _, v in d.values())            # an empty value is not a miss
    r = gctx.get_batch(q)
    check(r, q, d)
    assert [int(x) for x in r.live_idx] == [idx.find(k, segs) for k in q]


# ---- 2. gather alignment and length edges ----------------------------------------------------------
@pytest.mark.parametrize("base_off", [0, 1, 3, 13])
def test_get_gather_edges(gctx, base_off):
    """The edge store resident in a torch buffer at base offsets +0 / +1 / +3 / +13, queried in an
    order unlike the store's (so source and destination alignments differ), values left in HBM:
    every value byte for byte, and nothing written past val_bytes."""
    torch = pytest.importorskip("torch")
    segs, want, d, keys = edge()
    buf, ptrs, _ = dev_place(segs, base_off)
    idx = gctx.replay_index(ptrs, on_device=True)
    assert np.array_equal(idx.live, want)
    q = [keys[(i * 17 + 5) % len(keys)] for i in range(len(keys))] + keys[::-1]
    assert sorted(set(q)) == sorted(keys)
    r0 = gctx.get_batch(q, values=False)
    lens = [len(d[k][1]) for k in q]
    assert r0.status == K.OK and r0.values is None and r0.val_bytes == sum(lens)
    vb, n = r0.val_bytes, len(q)
    for shift in (0, base_off):   # the output 16-B aligned, and at the segments' own misalignment
        arena, ko = K.key_arena(q)
        d_keys = torch.from_numpy(arena.copy()).cuda()
        d_ko = torch.from_numpy(ko.astype(np.int64)).cuda()
        d_idx = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        d_off = torch.full((n + 1,), 77, dtype=torch.int64, device="cuda")
        d_vals = torch.full((vb + 64 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r = gctx.get_batch(None, keys_ptr=(d_keys.data_ptr(), d_ko.data_ptr(), n),
                           out_ptrs=(d_idx.data_ptr(), d_off.data_ptr(), d_vals.data_ptr() + shift, vb + 64, None))
        assert r.status == K.OK and r.val_bytes == vb
        torch.cuda.synchronize()
        off = d_off.cpu().numpy()
        out = d_vals.cpu().numpy()
        assert [int(x) for x in d_idx.cpu().numpy()] == [d[k][0] for k in q]
        assert list(off) == [0] + list(np.cumsum(lens))
        for i, k in enumerate(q):
            assert out[shift + off[i]: shift + off[i + 1]].tobytes() == d[k][1], (i, len(k), len(d[k][1]))
        assert (out[:shift] == 0xA5).all() and (out[shift + vb:] == 0xA5).all()
    # and to host memory, 64 bytes of room behind the values
    rc, li, vo, out, got = raw_get(gctx, q, 0, vb + 64)
    assert rc == K.OK and got == vb and (out[vb:] == 0xA5).all()
    assert [out[vo[i]: vo[i + 1]].tobytes() for i in range(n)] == [d[k][1] for k in q]
    del buf


# ---- 3. batch-size edges -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_get_batch_sizes(gctx, n):
    """n around the wave and workgroup sizes; hits and misses alternate, a live and an absent key
    of 300 bytes among them."""
    segs, want, d, keys = edge()
    gctx.replay_index(segs)
    q = [keys[(i // 2) % len(keys)] if i % 2 == 0 else b"miss-%d" % i for i in range(n)]
    if n > 3:
        q[2], q[3] = KEY300, MISS300
        assert KEY300 in d and MISS300 not in d
    r = gctx.get_batch(q)
    check(r, q, d)
    assert len(r.live_idx) == n and len(r.val_off) == n + 1
    if n > 3:
        assert r.live_idx[2] >= 0 and r.live_idx[3] == -1


# ---- 4. capacity and flags -------------------------------------------------------------------------
def test_get_capacity_and_flags(gctx):
    segs, want, d, keys = edge()
    gctx.replay_index(segs)
    q = keys[::-1] + [b"absent"]
    lens = [len(d[k][1]) if k in d else 0 for k in q]
    vb = sum(lens)
    want_idx = [d[k][0] if k in d else -1 for k in q]
    want_off = [0] + list(np.cumsum(lens))
    rc, li, vo, out, got = raw_get(gctx, q, 0, vb - 1)
    assert rc == K.CAPACITY and got == vb
    assert list(li) == want_idx and list(vo) == want_off
    assert (out == 0xA5).all()                  # nothing written: not past vals + vals_cap either
    rc, li, vo, out, got = raw_get(gctx, q, K.GET_LOCATE_ONLY, 0, vals=False)
    assert rc == K.OK and got == vb and list(li) == want_idx and list(vo) == want_off
    rc, li, vo, out, got = raw_get(gctx, q, 0, vb)
    assert rc == K.OK and [out[vo[i]: vo[i + 1]].tobytes() for i in range(len(q))] == [d.get(k, (0, b""))[1] for k in q]
    dec = np.array([0, 5, 3, 8], dtype=np.uint64)   # host key_off that decreases
    rc, *_ = raw_get(gctx, [b"12345678"], 0, 64, offs=dec)
    assert rc == K.EINVAL
    rc, *_ = raw_get(gctx, q, 0x80, vb)             # an unknown flag bit
    assert rc == K.EINVAL
    rc, *_ = raw_get(gctx, q, 0x1, vb)              # a replay flag that means nothing here
    assert rc == K.EINVAL
    check(gctx.get_batch(q), q, d)                  # the wrapper retries KVR_CAPACITY at the reported size
    assert gctx.get_batch(q, vals_cap=vb - 1).status == K.CAPACITY


# ---- 5. index lifetime ---------------------------------------------------------------------------
def test_get_index_lifetime():
    segs, want, d, q = coll()
    ctx = K.Context(0)
    try:
        assert ctx.index_epoch() == 0
        with pytest.raises(K.NativeError, match="-1"):
            ctx.get_batch(q)                        # a fresh context: no index
        ctx.replay_index(segs)
        e1 = ctx.index_epoch()
        assert e1 != 0
        a, b = ctx.get_batch(q), ctx.get_batch(q)   # any number of gets after one build
        check(a, q, d)
        check(b, q, d)
        assert np.array_equal(a.values, b.values) and ctx.index_epoch() == e1
        ctx.replay_index(segs)
        e2 = ctx.index_epoch()
        assert e2 != 0 and e2 != e1
        check(ctx.get_batch(q), q, d)
        assert ctx.replay_live(segs).status == K.OK   # a live list, no table
        assert ctx.index_epoch() == 0
        with pytest.raises(K.NativeError, match="-1"):
            ctx.get_batch(q)
        ctx.replay_index(segs)
        assert ctx.index_epoch() not in (0, e1, e2)
        assert ctx.replay(segs).status == K.OK        # a plain replay replaces the index
        assert ctx.index_epoch() == 0
        with pytest.raises(K.NativeError, match="-1"):
            ctx.get_batch(q)
        e = ctx.replay_index([b""])                 # the empty store: every key is a miss
        assert len(e.live) == 0 and ctx.index_epoch() != 0
        r = ctx.get_batch(q)
        assert r.status == K.OK and (r.live_idx == -1).all() and r.val_bytes == 0 and not r.val_off.any()
        assert all(r.value(i) is None for i in range(len(q)))
    finally:
        ctx.close()


# ---- 6. device in, device out ----------------------------------------------------------------------
def test_get_device_in_device_out(gctx):
    torch = pytest.importorskip("torch")
    segs, want, d, q = coll()
    gctx.replay_index(segs)
    host = gctx.get_batch(q, verify=True)
    check(host, q, d)
    n, vb = len(q), host.val_bytes
    arena, ko = K.key_arena(q)
    d_keys = torch.from_numpy(arena.copy()).cuda()
    d_ko = torch.from_numpy(ko.astype(np.int64)).cuda()
    d_idx = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    d_off = torch.full((n + 1,), 77, dtype=torch.int64, device="cuda")
    d_vals = torch.full((vb + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    d_bad = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = gctx.get_batch(None, verify=True, keys_ptr=(d_keys.data_ptr(), d_ko.data_ptr(), n),
                       out_ptrs=(d_idx.data_ptr(), d_off.data_ptr(), d_vals.data_ptr(), vb + 32, d_bad.data_ptr()))
    torch.cuda.synchronize()
    assert r.status == K.OK and r.val_bytes == vb and r.n_crc_fail == 0 == host.n_crc_fail
    assert np.array_equal(d_idx.cpu().numpy(), host.live_idx)
    assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), host.val_off)
    assert np.array_equal(d_vals.cpu().numpy()[:vb], host.values) and (d_vals.cpu().numpy()[vb:] == 0xA5).all()
    assert not d_bad.cpu().numpy().any() and not host.bad.any()
    assert r.stats.n_found == host.stats.n_found
    # device key offsets that decrease are found on the device
    d_ko2 = d_ko.clone()
    d_ko2[3] = d_ko2[5] + 1
    torch.cuda.synchronize()
    with pytest.raises(K.NativeError, match="-1"):
        gctx.get_batch(None, values=False, keys_ptr=(d_keys.data_ptr(), d_ko2.data_ptr(), n),
                       out_ptrs=(d_idx.data_ptr(), d_off.data_ptr(), None, 0, None))


# ---- 7. verify on read -----------------------------------------------------------------------------
def test_get_verify_on_read(gctx):
    """KVR_GET_VERIFY over the device-resident edge store: clean, then one byte of one live value
    flipped in HBM (data, not memory safety) with the index left as it is."""
    torch = pytest.importorskip("torch")
    segs, want, d, keys = edge()
    buf, ptrs, offs = dev_place(segs, 3)
    gctx.replay_index(ptrs, on_device=True)
    q = [keys[(i * 11 + 3) % len(keys)] for i in range(len(keys))] + [b"absent", b""]
    r = gctx.get_batch(q, verify=True)
    check(r, q, d)
    assert r.n_crc_fail == 0 and not r.bad.any() and r.stats.n_crc_fail == 0
    victim = next(k for k in keys if len(d[k][1]) == 4097)
    w = want[d[victim][0]]
    pos = offs[int(w["seg_idx"])] + int(w["rec_off"]) + 9 + int(w["key_len"]) + 4000
    buf[pos] ^= 0x40
    torch.cuda.synchronize()
    r = gctx.get_batch(q, verify=True)
    assert r.status == K.OK and r.n_crc_fail == 1
    assert [i for i in range(len(q)) if r.bad[i]] == [i for i, k in enumerate(q) if k == victim]
    now = bytearray(d[victim][1])
    now[4000] ^= 0x40
    for i, k in enumerate(q):
        assert r.value(i) == (bytes(now) if k == victim else d[k][1] if k in d else None)
    del buf


# ---- 8. the ingest path ----------------------------------------------------------------------------
def test_get_after_ingest(gctx):
    segs, want, d, q = coll()
    ig = gctx.ingest_index(segs)
    assert np.array_equal(ig.live, want) and gctx.index_epoch() != 0
    check(gctx.get_batch(q, verify=True), q, d)

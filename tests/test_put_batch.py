"""kvr_put_batch: KVStore::set / delete (engine.rs:157-198) for many operations at once on the
device, with the index in HBM updated in place.

Expected values never come from the code under test (put_model.py): the bytes are the Python
framing, the ETags zlib.crc32, the map a Python dict, and the tuples and the live list the oracle's
replay + fold over "old segments + the bytes the put returned".
"""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import kvreplay as K
import put_model as M
from test_get_batch import VAL_LENS
from test_open_index import DEAD, check_index, collision_store

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def raw_put(ctx, ops, seg_id, cap, arrays=None):
    """kvr_put_batch through ctypes with host buffers over a canary-filled output (no retry):
    rc, out, out_len, tuples, seg_off."""
    rep, _ = K.native()
    o, keys, koff, vals, voff = arrays if arrays is not None else K.op_arena(ops)
    o = np.ascontiguousarray(o, dtype=np.uint8)
    keys, vals = np.ascontiguousarray(keys, dtype=np.uint8), np.ascontiguousarray(vals, dtype=np.uint8)
    koff, voff = np.ascontiguousarray(koff, dtype=np.uint64), np.ascontiguousarray(voff, dtype=np.uint64)
    n = len(o)
    out = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    tup = np.zeros(max(n, 1), dtype=K.TUPLE_DTYPE)
    ol, so = C.c_uint64(12345), C.c_uint64(999)
    rc = rep.kvr_put_batch(ctx.h, seg_id, o.ctypes.data if n else None, keys.ctypes.data if keys.size else None,
                           koff.ctypes.data, vals.ctypes.data if vals.size else None, voff.ctypes.data, n, 0,
                           out.ctypes.data, cap, C.byref(ol), tup.ctypes.data, C.byref(so))
    return rc, out, int(ol.value), tup[:n], int(so.value)


def dev_put(ctx, ops, seg_id, shift, cap=None, arrays=None):
    """The same call with every input and output in torch buffers over 0xA5 fill, the op bytes, the
    key arena, the value arena and the output at unaligned addresses (in the manner of
    test_get_batch.dev_place): PutResult, the whole output buffer, where the output starts in it,
    the tuples."""
    torch = pytest.importorskip("torch")
    o, keys, koff, vals, voff = arrays if arrays is not None else K.op_arena(ops)
    n = len(o)

    def place(a, sh):
        buf = torch.full((a.size + 64 + sh,), 0xA5, dtype=torch.uint8, device="cuda")
        if a.size:
            buf[sh: sh + a.size] = torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()
        return buf, buf.data_ptr() + sh

    b_ops, p_ops = place(o, shift)
    b_keys, p_keys = place(keys, (3 * shift + 1) % 16)
    b_vals, p_vals = place(vals, (5 * shift + 7) % 16)
    d_koff = torch.from_numpy(np.array(koff, dtype=np.uint64).astype(np.int64)).cuda()
    d_voff = torch.from_numpy(np.array(voff, dtype=np.uint64).astype(np.int64)).cuda()
    if cap is None:
        cap = int(9 * n + koff[-1] + voff[-1]) + 48
    d_out = torch.full((cap + 48,), 0xA5, dtype=torch.uint8, device="cuda")
    d_tup = torch.zeros((max(n, 1) * 32,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = ctx.put_batch(None, seg_id, keys_ptr=(p_ops, p_keys, d_koff.data_ptr(), p_vals, d_voff.data_ptr(), n),
                      out_ptrs=(d_out.data_ptr() + shift, cap, d_tup.data_ptr()))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    tup = np.frombuffer(d_tup.cpu().numpy().tobytes(), dtype=K.TUPLE_DTYPE)[:n]
    # the inputs are only read
    assert b_keys.cpu().numpy()[(3 * shift + 1) % 16:][: keys.size].tobytes() == np.asarray(keys).tobytes()
    assert b_vals.cpu().numpy()[(5 * shift + 7) % 16:][: vals.size].tobytes() == np.asarray(vals).tobytes()
    return r, out, shift, tup


def dev_bytes(ctx, ptr, n):
    """n bytes of device memory at ptr, read back with torch (through the array interface torch
    reads foreign device memory by); a torch build without it copies with the HIP runtime that
    libkvreplay is linked against."""
    torch = pytest.importorskip("torch")
    if n == 0:
        return b""

    class _Mem:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}

    try:
        return torch.as_tensor(_Mem(), device="cuda").cpu().numpy().tobytes()
    except (TypeError, RuntimeError, ValueError):
        rep, _ = K.native()
        rep.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        out = np.zeros(n, dtype=np.uint8)
        assert rep.hipMemcpy(out.ctypes.data, ptr, n, 2) == 0           # hipMemcpyDeviceToHost
        return out.tobytes()


def check_state(ctx, segs, model, mentioned, epoch_before=None):
    """The index on the context against the oracle's over segs (old + active segments' bytes) and the
    dict model: the live list exactly, a valid table without DEAD entries, every get, the key arena."""
    want, od, order = M.oracle_state(segs)
    assert od == model
    idx = ctx.index_fetch(segs)
    assert np.array_equal(idx.live, want)
    rep, _ = K.native()
    assert len(idx.slots) == rep.kvr_index_slots(len(want))
    assert not (idx.slots == DEAD).any()
    check_index(idx, segs, want, [k for k in mentioned if k not in model])
    q = sorted(mentioned) + [b"never-mentioned"]
    r = ctx.get_batch(q, verify=True)
    assert r.status == K.OK and r.n_crc_fail == 0 and not r.bad.any()
    assert [r.value(i) for i in range(len(q))] == [model.get(k) for k in q]
    assert [int(x) for x in r.live_idx] == [order.index(k) if k in model else -1 for k in q]
    arena, offs = ctx.live_keys(len(want))
    assert [arena[int(offs[i]): int(offs[i + 1])].tobytes() for i in range(len(want))] == order
    if epoch_before is not None:
        assert ctx.index_epoch() not in (0, epoch_before)
    return idx


# ---- 1. framing and tuples at every start offset mod 16 -------------------------------------------
def test_put_framing_and_tuples(gctx):
    """The edge batch (keys of 0 .. 40 and 300 bytes and multi-byte UTF-8 ones, the value lengths of
    the get tests, DELs mixed in) put at every offset mod 16 of the active segment, with host buffers
    and with device buffers at unaligned addresses: out is the Python framing byte for byte, the
    fill byte follows out_len, the tuples are the oracle's, the CRCs zlib's.  It starts from
    replay_index([]): a put into an index with no segment at all."""
    assert VAL_LENS == M.VAL_LENS
    idx = gctx.replay_index([])
    assert len(idx.live) == 0
    model, mentioned, active = {}, set(), b""
    seen = set()
    for rnd in range(2):
        for step in range(16):
            mode = ("host", "dev")[(step + rnd) % 2]    # every start offset in both modes over the two rounds
            # a record of odd size in front, so that the edge batch starts at step (mod 16)
            pad = (step - len(active) - 10) % 16
            pre = [(b"p", bytes([step]) * (pad if pad else 16))]
            r = gctx.put_batch(pre, 0)
            assert r.status == K.OK and r.data == M.frame(pre) and r.seg_off == len(active) and r.seg_idx == 0
            active += r.data
            M.apply(model, pre)
            assert len(active) % 16 == step
            seen.add(len(active) % 16)
            ops = M.edge_ops(seed=step * 2 + (mode == "dev"))
            want = M.frame(ops)
            if mode == "host":
                rc, out, ol, tup, so = raw_put(gctx, ops, 0, len(want) + 40)
                assert rc == K.OK
                at = 0
            else:
                r, out, at, tup = dev_put(gctx, ops, 0, shift=(step * 7 + 3) % 16)
                assert r.status == K.OK
                ol, so = r.out_len, r.seg_off
                assert (out[:at] == 0xA5).all()
            assert ol == len(want) and so == len(active)
            assert out[at: at + ol].tobytes() == want
            assert (out[at + ol:] == 0xA5).all()               # nothing written past out + out_len
            assert np.array_equal(tup, M.oracle_tuples(want, 0, len(active)))
            assert [int(x) for x in tup["crc32"]] == M.etags(ops)
            st = gctx.last_put_stats()
            assert st.n_ops == len(ops) and st.bytes_out == len(want)
            assert st.n_set == sum(v is not None for _, v in ops) and st.n_del == sum(v is None for _, v in ops)
            active += want
            M.apply(model, ops)
            mentioned |= {k for k, _ in ops} | {b"p"}
    assert seen == set(range(16))
    sid, sidx, ln, ptr = gctx.active_segment()
    assert (sid, sidx, ln) == (0, 0, len(active))
    assert dev_bytes(gctx, ptr, ln) == active
    check_state(gctx, [active], model, mentioned)


# ---- 2. index equivalence on the collision store ---------------------------------------------------
@pytest.mark.parametrize("path", ["lds", "global"])
def test_put_index_equivalence(gctx, monkeypatch, path):
    """One batch over the collision store (both table layouts, so DEAD slots exist before): overwrites
    and DELs of live keys, a DEL of an absent key, SETs of deleted keys, new keys, both keys of every
    CRC-colliding pair, in-batch duplicates in the three orders, an empty value."""
    if path == "global":
        monkeypatch.setenv("KVR_FOLD_GLOBAL", "1")
    segs, pairs = collision_store()
    idx0 = gctx.replay_index(segs)
    assert (idx0.slots == DEAD).any()
    _, model, order = M.oracle_state(segs)
    rc, t, _ = M.O.replay(segs)
    every = {bytes(segs[w["seg_idx"]][w["rec_off"] + 5: w["rec_off"] + 5 + w["key_len"]]) for w in t}
    dead = sorted(every - set(model))
    assert len(dead) >= 2 and len(order) >= 9
    ops = []
    ops += [(k, b"over-" + k) for k in order[0::3]]                       # overwrites of live keys
    ops += [(k, None) for k in order[1::3]]                               # DELs of live keys
    ops += [(b"never-there", None)]                                        # a DEL of an absent key
    ops += [(k, b"back-" + k) for k in dead[::2]]                          # SETs of keys whose last record was a DEL
    ops += [(b"new-%d" % i, b"n" * i) for i in range(20)]                  # new keys, one with an empty value
    for j, (a, c) in enumerate(pairs):                                     # both keys of every colliding pair
        ops += [(a, b"pa%d" % j), (c, None if j % 3 == 0 else b"pc%d" % j)] if j % 2 else \
               [(c, b"qc%d" % j), (a, None if j % 3 == 0 else b"qa%d" % j)]
    ops += [(b"dup-ss", b"1"), (b"dup-sd", b"1"), (b"dup-ds", None), (order[2], b"first"),
            (b"dup-ss", b"2"), (b"dup-sd", None), (b"dup-ds", b"2"), (order[2], None), (order[2], b"")]
    mentioned = every | {k for k, _ in ops}
    epoch = gctx.index_epoch()
    r = gctx.put_batch(ops, len(segs))
    want = M.frame(ops)
    assert r.status == K.OK and r.data == want and r.seg_idx == len(segs) and r.seg_off == 0
    assert np.array_equal(r.tuples, M.oracle_tuples(want, len(segs), 0))
    M.apply(model, ops)
    assert model[order[2]] == b"" and b"dup-sd" not in model and model[b"dup-ds"] == b"2"
    check_state(gctx, segs + [want], model, mentioned, epoch)
    st = gctx.last_put_stats()
    assert st.n_live == len(model) and st.n_superseded > 0


# ---- 3. sequences: appends to one active segment, then the next -----------------------------------
def test_put_sequences(gctx):
    """Three batches into one active segment, then two into a larger seg_id (reset_active_segment):
    the oracle comparison after each, and active_segment() reports id, index, length and bytes."""
    base = [M.frame([(b"k%d" % i, b"v%d" % i) for i in range(30)] + [(b"k3", None), (b"k7", None)]),
            M.frame([(b"k%d" % i, b"w%d" % i) for i in range(10, 20)])]
    gctx.replay_index(base, seg_ids=[4, 9])
    _, model, _ = M.oracle_state(base)
    mentioned = set(model) | {b"k3", b"k7"}
    rng = np.random.RandomState(11)
    acts = [b"", b""]
    for b in range(5):
        which, seg_id = (0, 10) if b < 3 else (1, 12)
        ops = []
        for j in range(60):
            k = b"k%d" % rng.randint(0, 45)
            ops.append((k, None if rng.randint(0, 4) == 0 else bytes(rng.randint(0, 256, rng.randint(0, 70), dtype=np.uint8))))
        epoch = gctx.index_epoch()
        r = gctx.put_batch(ops, seg_id)
        want = M.frame(ops)
        assert r.status == K.OK and r.data == want
        assert r.seg_idx == 2 + which and r.seg_off == len(acts[which])
        assert np.array_equal(r.tuples, M.oracle_tuples(want, 2 + which, len(acts[which])))
        acts[which] += want
        M.apply(model, ops)
        mentioned |= {k for k, _ in ops}
        segs = base + acts[: which + 1]
        check_state(gctx, segs, model, mentioned, epoch)
        sid, sidx, ln, ptr = gctx.active_segment()
        assert (sid, sidx, ln) == (seg_id, 2 + which, len(acts[which]))
        assert dev_bytes(gctx, ptr, ln) == acts[which]
    assert raw_put(gctx, [(b"x", b"y")], 11, 64)[0] == K.EINVAL      # a smaller seg_id than the active one


# ---- 4. the table grows, empties and fills again ---------------------------------------------------
def test_put_table_growth_and_shrink(gctx):
    rep, _ = K.native()
    base = [M.frame([(b"a", b"1"), (b"b", b"2"), (b"c", b"3")])]
    idx = gctx.replay_index(base)
    assert len(idx.slots) <= 16                                      # a small table to grow from
    model, mentioned = {b"a": b"1", b"b": b"2", b"c": b"3"}, {b"a", b"b", b"c"}
    active = b""
    batches = [[(b"grow-%d" % i, b"g%d" % i) for i in range(100)], None, [(b"z%d" % i, b"again") for i in range(5)]]
    for b, ops in enumerate(batches):
        if ops is None:
            ops = [(k, None) for k in sorted(model)]               # DEL every key
        r = gctx.put_batch(ops, 1)
        assert r.status == K.OK
        active += r.data
        assert r.data == M.frame(ops)
        M.apply(model, ops)
        mentioned |= {k for k, _ in ops}
        assert r.stats.n_live == len(model) and r.stats.n_slots == rep.kvr_index_slots(len(model))
        check_state(gctx, base + [active], model, mentioned)
        if b == 1:
            assert r.stats.n_live == 0 and r.stats.n_slots == 16 and r.stats.n_superseded == 103
            g = gctx.get_batch(sorted(mentioned))
            assert (g.live_idx == -1).all() and g.val_bytes == 0
    assert len(model) == 5


# ---- 5. contention: several workgroups, one hot key ------------------------------------------------
def test_put_contention(gctx):
    """5000 ops over 600 distinct keys, one of them repeated 1000 times, SETs and DELs mixed: the
    smallest shape that spans several workgroups and hammers one entry of the in-batch table."""
    rng = np.random.RandomState(20261019)
    keys = [b"key-%04d-%s" % (i, b"x" * (i % 23)) for i in range(600)]
    base = [M.frame([(k, b"old-" + k) for k in keys[::2]])]
    gctx.replay_index(base)
    _, model, _ = M.oracle_state(base)
    hot = keys[0]
    ops = []
    for i in range(5000):
        k = hot if i % 5 == 0 else keys[rng.randint(1, 600)]
        ops.append((k, None if rng.randint(0, 10) < 3 else bytes(rng.randint(0, 256, rng.randint(0, 41), dtype=np.uint8))))
    assert sum(k == hot for k, _ in ops) == 1000 and len({k for k, _ in ops}) > 590
    r = gctx.put_batch(ops, 1)
    want = M.frame(ops)
    assert r.status == K.OK and r.data == want
    assert np.array_equal(r.tuples, M.oracle_tuples(want, 1, 0))
    M.apply(model, ops)
    check_state(gctx, base + [want], model, set(keys))


# ---- 6. atomicity and errors -----------------------------------------------------------------------
def snapshot(ctx, segs):
    idx = ctx.index_fetch(segs)
    act = ctx.active_segment()
    return (ctx.index_epoch(), idx.live.tobytes(), idx.slots.tobytes(), act[:3] if act else None,
            dev_bytes(ctx, act[3], act[2]) if act else None)


def test_put_atomicity_and_errors(gctx):
    base = [M.frame([(b"k%d" % i, b"v%d" % i) for i in range(20)])]
    good = [(b"k1", b"new"), (b"k2", None), (b"fresh", b"f" * 100)]
    bad_mid = [(b"k3", b"x"), (b"ab" + M.BAD_UTF8[2] + b"c", b"y"), (b"k4", None)]
    for with_active in (False, True):
        gctx.replay_index(base, seg_ids=[5])
        segs = list(base)
        if with_active:
            r = gctx.put_batch(good, 6)
            assert r.status == K.OK
            segs.append(r.data)
        snap = snapshot(gctx, segs)
        assert (snap[3] is not None) == with_active
        # an invalid UTF-8 key in the middle of the batch, checked on the host and in the key kernel
        rc, out, ol, _, _ = raw_put(gctx, bad_mid, 6, 256)
        assert rc == K.EINVAL and (out == 0xA5).all()
        r, out, at, _ = dev_put(gctx, bad_mid, 6, shift=5)
        assert r.status == K.EINVAL and (out == 0xA5).all()
        # device inputs: a DEL with a value, a bad op byte
        o, keys, koff, vals, voff = K.op_arena(good)
        o2 = o.copy()
        o2[0] = K.OP_DEL
        assert dev_put(gctx, None, 6, 2, arrays=(o2, keys, koff, vals, voff))[0].status == K.EINVAL
        o2[0] = 7
        assert dev_put(gctx, None, 6, 2, arrays=(o2, keys, koff, vals, voff))[0].status == K.EINVAL
        assert raw_put(gctx, None, 6, 256, arrays=(o2, keys, koff, vals, voff))[0] == K.EINVAL
        # out_cap one byte short
        need = len(M.frame(good))
        rc, out, ol, _, _ = raw_put(gctx, good, 6, need - 1)
        assert rc == K.CAPACITY and ol == need and (out == 0xA5).all()
        r, out, at, _ = dev_put(gctx, good, 6, shift=9, cap=need - 1)
        assert r.status == K.CAPACITY and r.out_len == need and (out == 0xA5).all()
        # a seg_id not above the last segment's / below the active one
        for sid in (5, 4) if not with_active else (5,):
            rc, out, _, _, _ = raw_put(gctx, good, sid, 256)
            assert rc == K.EINVAL and (out == 0xA5).all()
        # n = 0 changes nothing
        rc, out, ol, _, so = raw_put(gctx, [], 6, 16)
        assert rc == K.OK and ol == 0 and (out == 0xA5).all()
        assert snapshot(gctx, segs) == snap
    # no index on the context (a later replay dropped it together with the active segment)
    assert gctx.replay([b""]).status == K.OK
    assert gctx.index_epoch() == 0 and gctx.active_segment() is None
    rc, out, _, _, _ = raw_put(gctx, good, 6, 256)
    assert rc == K.EINVAL and (out == 0xA5).all()
    gctx.replay_live(base)                                            # a live list without a key table
    assert raw_put(gctx, good, 6, 256)[0] == K.EINVAL


# ---- 7. the store ----------------------------------------------------------------------------------
def test_store_put_many_on_the_device(gctx, tmp_path):
    d = tmp_path / "persisted_store"
    shutil.copytree(os.path.join(GOLD, "persistence"), d)
    files = K.discover(str(d))
    _, model, order = M.oracle_state([open(p, "rb").read() for _, p in files])
    model = dict(model)
    assert len(order) >= 2
    s = K.KVStore.open(str(d), gctx)
    try:
        active_id = s.stats().active_segment_id
        mentioned = set(model)
        b1 = [(order[0], b"changed"), (order[1], None), (b"put-new", b"n" * 300), (b"put-new", b"second"), (b"gone", None),
              (b"extra", b"e")]
        b2 = [(order[1], b"back"), (b"extra", b""), (b"put-new", None), (M.UTF8_KEYS[0], b"u")]
        done = []
        for b in (b1, b2):
            assert s.put_many(b) == M.etags(b)
            assert gctx.last_put_stats().n_ops == len(b)                 # (encoded on the device)
            M.apply(model, b)
            mentioned |= {k for k, _ in b}
            done.append(b)
            q = sorted(mentioned)
            assert s.get_many(q) == [model.get(k) for k in q]
            assert gctx.last_get_stats().n_keys == len(q)               # still the device path
            assert [s.get(k) for k in q] == [model.get(k) for k in q]
            assert s.get_many(q, device=False) == [model.get(k) for k in q]
            assert sorted(s.list_keys()) == sorted(model)
            st = s.stats()
            assert st.num_keys == len(model) and st.total_bytes == sum(len(v) for v in model.values())
            data = open(os.path.join(str(d), "segment-%d.dat" % active_id), "rb").read()
            assert data == b"".join(M.frame(x) for x in done)
        s.close()
        s = K.KVStore.open(str(d), gctx)                                 # reopen: the same map
        q = sorted(mentioned)
        assert s.get_many(q) == [model.get(k) for k in q] and s.stats().num_keys == len(model)
        assert s.stats().active_segment_id == active_id + 1
        b3 = [(order[0], None), (b"after-reopen", b"r")]
        assert s.put_many(b3) == M.etags(b3)
        M.apply(model, b3)
        mentioned |= {k for k, _ in b3}
        s.compact()                                                      # the active segment is one of its inputs
        q = sorted(mentioned)
        assert s.get_many(q) == [model.get(k) for k in q] and s.stats().num_keys == len(model)
        b4 = [(b"after-compact", b"c" * 17), (b"extra", None)]
        assert s.put_many(b4) == M.etags(b4)                             # a put after the compaction
        assert gctx.last_put_stats().n_ops == len(b4)
        M.apply(model, b4)
        q = sorted(mentioned | {b"after-compact"})
        assert s.get_many(q) == [model.get(k) for k in q]
        assert [s.get(k) for k in q] == [model.get(k) for k in q]
        _, od, _ = M.oracle_state([open(p, "rb").read() for _, p in K.discover(str(d))])
        assert od == model
    finally:
        s.close()

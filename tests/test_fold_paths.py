"""The last-writer fold against the key prefixes of every replay path.

The fold (kvr_replay_live / _last / _index, kvr_ingest_index, kvr_compact, everything
kvr_get_batch answers) compares two side outputs of the replay pipeline instead of the key bytes in
the segments: the 16-byte key prefix beside every tuple (kpool -> ckeys) and the pair (key tag, key
length) (ctk).  The prefix has six writers in kvr_replay_kernel.hip (do_record and the exact loop
through key_prefix_mem, the batched speculative tiles, three sites in k_piece, k_rewalk) and
k_compact_s moves it in two ways (slot by slot, and run form).  Here every one of those paths gets
a store whose keys recur -- overwrites, DELs, keys deleted and set again -- so that a prefix that
differs between two records of one key changes the answer, and the side outputs themselves are read
back (kvr_fold_keys_fetch) and compared tuple by tuple, which names the emitter and also catches a
prefix that is wrong the same way every time.

Expected values never come from the library: oracle_py (replay, fold_live, compact) and the
independent Python walk and dict model of test_compaction (walk, py_map, py_compact).  Every
comparison is exact.
"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import kvreplay as K
import oracle_py as O
from test_compaction import py_compact, py_map, rec_del, rec_set, walk
from test_get_batch import check as check_get
from test_get_batch import dev_place
from test_gpu_parity import CAND_STORES, _varied_key, _varied_store, adversarial_store, mixed_store
from test_open_index import DEAD, check_index, keys_of
from test_piece_mode import _uniform
from test_piece_mode import engine  # noqa: F401  (a fixture: k_piece first, or k_replay's tiles alone)

TILE = 8192


# ---- the stores, one family per emitter -----------------------------------------------------------
ALPHA = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+-"


def ukey(j, klen):
    """Key j of klen ASCII bytes: j in base 64 in the first three bytes (distinct keys differ inside
    their first 16 bytes), then bytes that depend on j and the position."""
    return bytes(ALPHA[(j >> (6 * p)) & 63] if p < 3 else 97 + (j + 7 * p) % 26 for p in range(klen))


UNIFORM_SHAPES = [(0, 128), (1, 129), (3, 200), (4, 300), (7, 200), (12, 500), (15, 1024), (16, 1024), (17, 1024),
                  (24, 1000), (33, 4096), (36, 8192), (37, 1024), (16, 65536)]
BIG = (16, 65536)          # 45 records: exempt from the 30 % and DEL properties of its first segment


@functools.lru_cache(maxsize=None)
def uniform_store(klen, vlen, dels):
    """Half of test_piece_shapes' sizes (146 tiles; 366 for the 64-KiB values): record i has key
    i mod m; a second segment of another shape (9, 1500) with a key deleted and set again and a key
    whose last record is a DEL.  dels: three records of the last third are DELs of their keys."""
    n_rec = max(8, (1_200_000 if vlen < 60000 else 3_000_000) // (9 + klen + vlen))
    m = 11 if (klen, vlen) == BIG else max(1, min(n_rec // 3, 64 ** min(klen, 3)))
    third = 2 * n_rec // 3
    change = {third + 1: "del", (third + n_rec) // 2: "del", n_rec - 1: "del"} if dels else None
    return (_uniform(n_rec, klen, vlen, change=change, keyf=lambda i: ukey(i % m, klen)),
            _uniform(300, 9, 1500, change={150: "del", 290: "del"}, keyf=lambda i: ukey(i % 100, 9)))


PATTERN = bytes((j * 37 + 11) & 255 for j in range(2 * TILE + 512))
BOUNDARY_KLENS = [(0, 1, 3, 4), (5, 13, 15, 16), (17, 20, 33)]     # three stores of 3 - 4 MB


def bkey(klen, c):
    return bytes(97 + (klen * 3 + c * 5 + p * 7) % 26 for p in range(klen))


@functools.lru_cache(maxsize=None)
def boundary_store(group):
    """As test_gpu_parity.boundary_segment with 8-KiB tiles: a probe record starts at every offset
    r in [-44, 8] around a tile boundary, its key of klen bytes chosen by r mod 5 (so every key
    recurs at ten or more offsets), between fillers of the one key b"f" (a hot key).  One segment
    per key length; each ends with two DELs and a SET of a deleted key."""
    segs = []
    for klen in BOUNDARY_KLENS[group]:
        out = bytearray()
        for vlen in (0, 200):
            for r in range(-44, 9):
                b = (len(out) // TILE + 1) * TILE
                if b + r - len(out) < 10:
                    b += TILE
                fill = b + r - len(out) - 10                  # filler: 9 + 1 (key "f") + fill bytes
                p0 = len(out) & 255
                out += rec_set(b"f", PATTERN[p0: p0 + fill])
                assert len(out) == b + r
                out += rec_set(bkey(klen, r % 5), bytes((r * 7 + j) & 255 for j in range(vlen)))
        out += rec_del(bkey(klen, 0)) + rec_del(bkey(klen, 1)) + rec_set(bkey(klen, 1), b"again")
        segs.append(bytes(out))
    return tuple(segs)


@functools.lru_cache(maxsize=None)
def cand_store(name):
    """test_candidate_rounds' parameter sets with the keys drawn from a pool of 300 (mixed_keys from
    0 bytes on, so the empty key is among them): three segments of 250 KB."""
    kw = dict(CAND_STORES[name])
    if name == "mixed_keys":
        kw["klen_rng"] = (0, 40)
    rnd = random.Random(len(name))
    pool = [_varied_key(rnd, kw["klen_rng"], kw.get("key_alphabet")) for _ in range(300)]
    return tuple(_varied_store(1000 * i + len(name), 250_000, key_pool=pool, **kw) for i in range(3))


@functools.lru_cache(maxsize=None)
def rewalk_store():
    """test_adversarial_speculation's segment (values that are record chains and zero runs) twice:
    its key%d keys recur across the segments."""
    seg = adversarial_store()[0]
    return (seg, seg)


@functools.lru_cache(maxsize=None)
def hot_store(live):
    """test_pool_overflow_retry's mixed store over 5000 keys: 700 000 DELs of b"" make the empty key
    the hot bucket; live: the store ends with a SET of it."""
    tail = rec_del(b"k5") + rec_set(b"k5", b"v") + rec_del(b"k6") + (rec_set(b"", b"x") if live else b"")
    return (mixed_store(5000) + tail,)


SEGEND_LENS = [1, 2, 3, 5, 15, 17]


@functools.lru_cache(maxsize=None)
def segend_store(klen):
    """A few SETs that rewrite two keys; the last record is a DEL of the key of klen bytes, whose
    last byte is the segment's last byte."""
    k, b = bkey(klen, 2), b"other"
    return (rec_set(k, b"v1") + rec_set(b, b"w1") + rec_set(k, b"v2" * 40) + rec_del(b) + rec_set(b, b"w2") +
            rec_set(k, b"") + rec_del(k),)


BUILDERS = {"uniform": uniform_store, "boundary": boundary_store, "cand": cand_store, "rewalk": rewalk_store,
            "hot": hot_store, "segend": segend_store}
ALL_STORES = ([("uniform", k, v, d) for k, v in UNIFORM_SHAPES for d in (False, True)] +
              [("boundary", g) for g in range(len(BOUNDARY_KLENS))] + [("cand", n) for n in CAND_STORES] +
              [("rewalk",), ("hot", False), ("hot", True)] + [("segend", n) for n in SEGEND_LENS])


def store_id(s):
    return "-".join(str(int(x) if isinstance(x, bool) else x) for x in s)


# ---- what every store must give, from the oracle and the Python model ---------------------------------
class Truth:
    def __init__(self, segs):
        self.segs = list(segs)
        self.size = sum(len(s) for s in segs)
        rc, t, err = O.replay(self.segs)
        assert rc == 0, (err.kind, err.seg_idx, err.rec_off)
        live, nk, _ = O.fold_live(self.segs, t)
        self.t, self.want, self.nk = t, t[live], nk
        recs = [r for s in segs for r in walk(s)]
        assert len(recs) == len(t)
        self.keys = [r[1] for r in recs]
        self.ops = [r[0] for r in recs]
        self.map = py_map(self.segs)
        last = {}
        for i, k in enumerate(self.keys):
            last[k] = i
        self.last_idx = np.array(sorted(last.values()), dtype=np.int64)
        self.dead = [k for k, i in last.items() if self.ops[i] == 1]
        self.live_keys = keys_of(self.segs, self.want)
        # the side outputs: the first 16 key bytes zero padded, (key tag, key length)
        self.pre = np.frombuffer(b"".join(k[:16].ljust(16, b"\0") for k in self.keys), dtype=np.uint8).reshape(-1, 16)
        self.tl = np.stack([t["key_tag"], t["key_len"]], axis=1).astype(np.uint32)
        # KVStore::get: every key the walk saw, and each with its last byte changed
        self.queries = list(last) + [k[:-1] + bytes([k[-1] ^ 1]) if k else b"\x00" for k in last]
        self._compact = {}

    @functools.cached_property
    def model(self):
        """{key: (index into the live list, value bytes)}: the oracle's live order, py_map's values."""
        assert sorted(self.live_keys) == sorted(self.map)
        return {k: (j, self.map[k]) for j, k in enumerate(self.live_keys)}

    def compact(self, target):
        if target not in self._compact:
            rc, data, ends, _ = O.compact(self.segs, target)
            assert rc == 0
            if self.size < 1_000_000:
                assert (data, ends) == py_compact(self.segs, target)
            self._compact[target] = (data, ends)
        return self._compact[target]


@functools.lru_cache(maxsize=None)
def truth(*store):
    return Truth(BUILDERS[store[0]](*store[1:]))


# ---- CPU: the stores themselves -----------------------------------------------------------------------
@pytest.mark.parametrize("store", ALL_STORES, ids=store_id)
def test_store_properties(store):
    """The oracle replays the store, its fold keeps the keys of the Python map, and the keys recur:
    at least 30 % of the records rewrite an earlier key, a key's last record is a DEL, a key is
    deleted and later set again."""
    T = truth(*store)
    assert T.nk == len(T.map) == len(T.want) and set(T.live_keys) == set(T.map)
    assert len(T.last_idx) == len(T.map) + len(T.dead)
    seen, deleted, rewrites, reset = set(), set(), 0, 0
    for op, k in zip(T.ops, T.keys):
        rewrites += k in seen
        seen.add(k)
        if op == 1:
            deleted.add(k)
        elif k in deleted:
            reset += 1
    if store[:3] != ("uniform",) + BIG:
        assert rewrites >= 0.3 * len(T.keys), (rewrites, len(T.keys))
    assert T.dead and reset
    if store[0] == "uniform":
        n0 = int(np.count_nonzero(T.t["seg_idx"] == 0))
        assert len(T.segs[0]) >= (64 if store[:3] != ("uniform",) + BIG else 32) * TILE
        assert int(np.count_nonzero(T.t["op"][:n0])) == (3 if store[3] else 0)
        assert set(T.t["key_len"][:n0]) == {store[1]} and (T.t["val_len"][:n0][T.t["op"][:n0] == 0] == store[2]).all()
    if store[0] == "segend":
        assert T.ops[-1] == 1 and len(T.keys[-1]) == store[1] and T.segs[0].endswith(T.keys[-1])
    if store[0] == "hot":
        assert T.keys.count(b"") >= 700_000 and ((b"" in T.map) == store[1])


def test_key_lengths_covered():
    lens = set()
    for store in ALL_STORES:
        lens |= set(int(x) for x in np.unique(truth(*store).t["key_len"]))
    assert set(range(0, 6)) | set(range(12, 18)) | {20, 24, 33, 36, 37, 40} <= lens, sorted(lens)
    assert any(b"" in truth(*s).map for s in ALL_STORES)              # the empty key live


def test_accessor_without_context():
    rep, _ = K.native()
    n = C.c_size_t(7)
    buf = np.zeros(64, dtype=np.uint8)
    assert rep.kvr_fold_keys_fetch(None, buf.ctypes.data, buf.ctypes.data, 1, C.byref(n)) == K.EINVAL
    assert rep.kvr_fold_keys_fetch(None, None, None, 0, None) == K.EINVAL


# ---- GPU: every folding entry point over one store ----------------------------------------------------
def check_side(ctx, T):
    """kvr_fold_keys_fetch after a folding call: one prefix and one (tag, length) per replayed tuple."""
    pre, tl = ctx.fold_keys()
    assert len(pre) == len(tl) == len(T.t)
    bad = np.nonzero((pre != T.pre).any(axis=1) | (tl != T.tl).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        w = T.t[i]
        raise AssertionError(
            f"{len(bad)} of {len(pre)} tuples with wrong side outputs; the first: tuple {i} (segment {w['seg_idx']}, "
            f"offset {w['rec_off']}, op {w['op']}, key_len {w['key_len']}, val_len {w['val_len']}): prefix "
            f"{pre[i].tobytes().hex()} want {T.pre[i].tobytes().hex()}, (tag, len) {tl[i].tolist()} want {T.tl[i].tolist()}")


@pytest.mark.gpu
def test_accessor_contract():
    """kvr_fold_keys_fetch: KVR_EINVAL before any folding call and after one that failed or had no
    segments, KVR_CAPACITY with the count and nothing written when cap is short, and the last
    folding call's rows still there after calls that do not fold."""
    T, other = truth("segend", 5), truth("segend", 17)
    rep, _ = K.native()
    ctx = K.Context(0)
    try:
        with pytest.raises(K.NativeError, match=r"\(-1\)"):
            ctx.fold_keys()
        assert ctx.replay(T.segs).status == K.OK                      # a plain replay keeps none
        with pytest.raises(K.NativeError, match=r"\(-1\)"):
            ctx.fold_keys()
        assert ctx.replay_live(T.segs).status == K.OK
        check_side(ctx, T)
        n = C.c_size_t(0)
        pre = np.full((len(T.t), 16), 0xA5, dtype=np.uint8)
        tl = np.full((len(T.t), 2), 0xA5A5A5A5, dtype=np.uint32)
        rc = rep.kvr_fold_keys_fetch(ctx.h, pre.ctypes.data, tl.ctypes.data, len(T.t) - 1, C.byref(n))
        assert rc == K.CAPACITY and n.value == len(T.t) and (pre == 0xA5).all() and (tl == 0xA5A5A5A5).all()
        rc = rep.kvr_fold_keys_fetch(ctx.h, pre.ctypes.data, tl.ctypes.data, len(T.t), C.byref(n))
        assert rc == K.OK and n.value == len(T.t) and np.array_equal(pre, T.pre) and np.array_equal(tl, T.tl)
        assert ctx.live_keys(len(T.want))[0].tobytes() == b"".join(T.live_keys)
        assert ctx.replay(other.segs).status == K.OK                  # calls that do not fold leave them
        check_side(ctx, T)
        assert ctx.replay_last(other.segs).status == K.OK             # the next folding call replaces them
        check_side(ctx, other)
        assert ctx.replay_live([T.segs[0][:-1]]).status == K.CORRUPTED
        with pytest.raises(K.NativeError, match=r"\(-1\)"):
            ctx.fold_keys()
        assert ctx.replay_live(T.segs).status == K.OK
        check_side(ctx, T)
        assert ctx.replay_live([]).status == K.OK
        with pytest.raises(K.NativeError, match=r"\(-1\)"):
            ctx.fold_keys()
    finally:
        ctx.close()


def same_tuples(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0][:5]
        raise AssertionError(f"{what}: tuples differ at {bad}: gpu={got[bad]} want={want[bad]}")


def check_table(ctx, idx, T):
    n = len(T.want)
    same_tuples(idx.live, T.want, "replay_index")
    if n <= 3000:
        check_index(idx, T.segs, T.want, T.dead)
    else:
        ns = len(idx.slots)
        assert ns >= 16 and ns & (ns - 1) == 0 and ns > n
        used = idx.slots[(idx.slots != 0) & (idx.slots != DEAD)]
        assert len(used) == n and len(np.unique(used)) == n
        for j in range(0, n, -(-n // 3000)):
            assert idx.find(T.live_keys[j], T.segs) == j
        for k in T.dead:
            assert idx.find(k, T.segs) == -1
    arena, offs = ctx.live_keys(n)
    assert arena.tobytes() == b"".join(T.live_keys)
    assert [int(x) for x in offs] == [0] + list(np.cumsum([len(k) for k in T.live_keys], dtype=np.int64))


def run_checks(ctx, T, src=None, on_device=False, ingest=False):
    """src: what the library replays (the host segments, or (pointer, length) pairs in HBM)."""
    src = T.segs if src is None else src
    r = ctx.replay_live(src, on_device=on_device)
    assert r.status == K.OK
    check_side(ctx, T)
    same_tuples(r.tuples, T.want, "replay_live")
    assert r.n == len(T.map)
    rl = ctx.replay_last(src, on_device=on_device)
    assert rl.status == K.OK
    same_tuples(rl.tuples, T.t[T.last_idx], "replay_last")
    idx = ctx.replay_index(src, on_device=on_device)
    check_table(ctx, idx, T)
    g = ctx.get_batch(T.queries, verify=True)
    check_get(g, T.queries, T.model)
    assert g.n_crc_fail == 0 and not g.bad.any()
    for target in (0, 4096):
        data, ends = T.compact(target)
        c = ctx.compact(src, target, on_device=on_device)
        assert c.status == K.OK and c.seg_ends == ends, (target, c.seg_ends[:4], ends[:4])
        assert c.data == data, target
        check_side(ctx, T)
    if ingest:
        ig = ctx.ingest_index(T.segs)
        same_tuples(ig.live, T.want, "ingest_index")
        check_side(ctx, T)


def with_tps(ctx, tps, fn):
    ctx.set_tiles_per_stripe(tps)
    try:
        fn()
    finally:
        ctx.set_tiles_per_stripe(0)


@pytest.mark.gpu
@pytest.mark.parametrize("tps", [0, 2, 64])
@pytest.mark.parametrize("shape", UNIFORM_SHAPES, ids=[f"k{k}v{v}" for k, v in UNIFORM_SHAPES])
def test_fold_uniform(gctx, shape, tps, engine):
    """Equal records with recurring keys: k_piece's three prefix sites and the run-form copy of
    k_compact_s (engine piece), the batched speculative tiles (engine tiles); with three DELs in the
    last third the runs end early and the rest goes record by record."""
    for dels in (False, True):
        with_tps(gctx, tps, lambda: run_checks(gctx, truth("uniform", *shape, dels), ingest=tps == 0 and not dels))


@pytest.mark.gpu
@pytest.mark.parametrize("tps", [0, 2, 64])
@pytest.mark.parametrize("shape", [(7, 200), (36, 8192)], ids=["k7v200", "k36v8192"])
def test_fold_uniform_link_kernel(gctx, monkeypatch, shape, tps, engine):
    """The same with k_link before k_compact_s (its plain mode: the stripe offsets from k_link)."""
    monkeypatch.setenv("KVR_LINK_KERNEL", "1")
    for dels in (False, True):
        with_tps(gctx, tps, lambda: run_checks(gctx, truth("uniform", *shape, dels)))


@pytest.mark.gpu
@pytest.mark.parametrize("tps", [0, 1, 4])
@pytest.mark.parametrize("group", range(len(BOUNDARY_KLENS)), ids=["k0-4", "k5-16", "k17-33"])
def test_fold_boundary(gctx, group, tps):
    """Keys across tile limits: key_prefix_mem's byte path and its word path side by side."""
    with_tps(gctx, tps, lambda: run_checks(gctx, truth("boundary", group)))


@pytest.mark.gpu
@pytest.mark.parametrize("tps", [0, 2])
@pytest.mark.parametrize("name", list(CAND_STORES))
def test_fold_candidates(gctx, name, tps):
    """Record lengths that vary tile to tile (candidate rounds, the exact loop), 300 recurring keys."""
    with_tps(gctx, tps, lambda: run_checks(gctx, truth("cand", name), ingest=tps == 0))


@pytest.mark.gpu
@pytest.mark.parametrize("tps", [1, 2, 4])
def test_fold_rewalk(gctx, tps):
    """Values that are record chains: the records inside them never reach the fold (the tuple count
    and every prefix are the oracle's), whichever stripes were re-walked."""
    with_tps(gctx, tps, lambda: run_checks(gctx, truth("rewalk")))


@pytest.mark.gpu
def test_rewalk_store_rewalks(gctx):
    """The store does send stripes through k_rewalk at one of the stripe sizes test_fold_rewalk uses."""
    T = truth("rewalk")
    redo = {}
    for tps in (1, 2, 4):
        def one():
            r = gctx.replay(T.segs)
            assert r.status == K.OK and r.n == len(T.t)
            redo[tps] = int(r.stats.n_redo)
        with_tps(gctx, tps, one)
    assert max(redo.values()) >= 1, redo


@pytest.mark.gpu
@pytest.mark.parametrize("live", [False, True], ids=["deleted", "live"])
def test_fold_hot_empty_key(gctx, live):
    """The empty key as the hot bucket k_fold_hot takes over, behind the pool-overflow retry; its
    last record a DEL, or a SET (the empty key live)."""
    T = truth("hot", live)
    with_tps(gctx, 1024, lambda: run_checks(gctx, T))
    assert (b"" in T.model) == live


# ---- device-resident stores: every byte outside a segment is 0xA5 -----------------------------------
def run_device(ctx, T, base_off):
    buf, ptrs, _ = dev_place(T.segs, base_off, fill=0xA5)
    assert all(p % 256 == base_off for p, _ in ptrs)
    run_checks(ctx, T, src=ptrs, on_device=True)
    del buf


@pytest.mark.gpu
@pytest.mark.parametrize("base_off", [1, 3, 13])
@pytest.mark.parametrize("shape", [(0, 128), (7, 200), (36, 8192)], ids=["k0v128", "k7v200", "k36v8192"])
def test_fold_device_uniform(gctx, shape, base_off, engine):
    for tps in (0, 2):
        with_tps(gctx, tps, lambda: run_device(gctx, truth("uniform", *shape, True), base_off))


@pytest.mark.gpu
@pytest.mark.parametrize("base_off", [1, 3, 13])
@pytest.mark.parametrize("group", range(len(BOUNDARY_KLENS)), ids=["k0-4", "k5-16", "k17-33"])
def test_fold_device_boundary(gctx, group, base_off):
    for tps in (0, 1):
        with_tps(gctx, tps, lambda: run_device(gctx, truth("boundary", group), base_off))


@pytest.mark.gpu
@pytest.mark.parametrize("base_off", [1, 3, 13])
@pytest.mark.parametrize("source", ["prefixes", "segments"])
def test_fold_segment_end_keys(gctx, monkeypatch, source, base_off):
    """A short key that ends on a segment's last byte with 0xA5 behind it: the prefixes, and the
    fold's own key_prefix16 over the segment bytes (KVR_FOLD_SEGKEYS), which reads the dword that
    straddles the segment end."""
    if source == "segments":
        monkeypatch.setenv("KVR_FOLD_SEGKEYS", "1")
    for klen in SEGEND_LENS:
        run_device(gctx, truth("segend", klen), base_off)

"""Shared by test_put_host.py and test_put_batch.py: the expected side of the write path.

Nothing here calls the code under test.  The bytes a batch appends are the Python framing of
test_open_index (rec_set / rec_del, engine.rs:169-173 / :191-193), the ETags are zlib.crc32, the
map is a Python dict, and the tuples and the live list come from the oracle's replay + fold
(oracle_py) over "old segments + the bytes the put returned".
"""
import zlib

import numpy as np

import oracle_py as O
from test_open_index import rec_del, rec_set

# value lengths around every boundary of the copy (16-B words, the 4-KiB round) and of the CRC pass
# (4-KiB chunks): test_get_batch.VAL_LENS (that module is GPU-only, so the list is restated and
# test_put_batch asserts the two are equal)
VAL_LENS = [0, 1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 4096 * 2 + 17]
# keys of 0 .. 40 bytes (values then start at every address mod 16) and one of 300, valid UTF-8
EDGE_KEYS = [bytes(97 + (n * 5 + i) % 26 for i in range(n)) for n in range(0, 41)] + [b"K" * 300]
UTF8_KEYS = [b"\xd0\xba\xd0\xbb\xd1\x8e\xd1\x87", b"\xe2\x82\xac-key", b"\xf0\x9f\x98\x80", b"\xf4\x8f\xbf\xbf", b"\xed\x9f\xbf"]
# truncated sequence, overlong, surrogate, > U+10FFFF (the oracle's oracle_utf8_check rejects each)
BAD_UTF8 = [b"\xe2\x82", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"]


def frame(ops):
    """The bytes set / delete append for ops: (key, value) pairs, value None meaning DEL."""
    return b"".join(rec_del(k) if v is None else rec_set(k, v) for k, v in ops)


def apply(model, ops):
    for k, v in ops:
        if v is None:
            model.pop(k, None)
        else:
            model[k] = v


def etags(ops):
    return [0 if v is None else zlib.crc32(v) for _, v in ops]


def edge_ops(seed=7, dels=True):
    """One op per edge key: values of VAL_LENS in turn, every fifth op a DEL."""
    rng = np.random.RandomState(seed)
    keys = EDGE_KEYS + UTF8_KEYS
    ops = []
    for i, k in enumerate(keys):
        v = rng.randint(0, 256, VAL_LENS[(i + seed) % len(VAL_LENS)], dtype=np.uint8).tobytes()
        ops.append((k, None if dels and i % 5 == 4 else v))
    return ops


def oracle_tuples(data, seg_idx, base_off):
    """The tuples kvr_replay emits for records that lie at base_off of segment seg_idx."""
    rc, t, _ = O.replay([data])
    assert rc == 0
    t = t.copy()
    t["seg_idx"] = seg_idx
    t["rec_off"] += base_off
    return t


def oracle_state(segs):
    """(live tuples in (segment, offset) order, {key: value}, live keys in live order) of segs."""
    segs = [bytes(s) for s in segs]
    rc, t, _ = O.replay(segs)
    assert rc == 0
    live, nk, _ = O.fold_live(segs, t)
    want = t[live]
    d, order = {}, []
    for w in want:
        s, ko = segs[int(w["seg_idx"])], int(w["rec_off"]) + 5
        vo = ko + int(w["key_len"]) + 4
        k = s[ko: ko + int(w["key_len"])]
        d[k] = s[vo: vo + int(w["val_len"])]
        order.append(k)
    assert len(d) == nk
    return want, d, order

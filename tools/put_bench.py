"""Batched puts on the device against what the project offered before them.

Builds the cfg2 store in HBM as tools/get_bench.py does, runs kvr_replay_index, then times
kvr_put_batch over one batch of --ops operations with 1-KiB values — half of them overwrite live
keys, 10 % are DELs of live keys, the rest SET new keys — with every input and output in device
memory.  Each repetition starts from a fresh kvr_replay_index (a put changes the index); medians of
--reps after --warmup:
  (a) ms_frame + ms_crc as bytes/s, beside the gather rate of a kvr_get_batch of as many keys in the
      same process (k_gather_r, the project's copy yardstick);
  (b) ms_index beside kvr_replay_index over the store plus the appended segment — the only way to
      see a write before kvr_put_batch — timed in the same process; the two live lists are compared;
  (c) the whole call (wall) beside kvh_encode_batch + kvh_index_update + kvr_index_build_host on one
      host thread over host copies.

  python tools/put_bench.py [--segments N] [--ops K] [--reps R] [--no-host] [--out DIR]
Prints one JSON line and writes it to DIR/put_bench_<library hash>.json (default bench_out/put).
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mini-kvstore-v2_amd"))


def median(x):
    return float(np.median(np.asarray(x, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--ops", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "put"))
    args = ap.parse_args()
    import torch
    import kvreplay as K

    dev = torch.device("cuda", 0)
    spec = K.GenSpec(seed=0x6B767265706C6179 + 2, seg_bytes=64 << 20, val_min=1024, val_max=1024, key_space_log2=20)
    ctx = K.Context(0)
    sizes = [K.gen_segment_size(spec, s) for s in range(args.segments)]
    offs, tot = [], 0
    for ln, _ in sizes:
        offs.append(tot)
        tot += (ln + 255) & ~255
    data = torch.empty(tot + 256, dtype=torch.uint8, device=dev)
    for s, ((ln, nr), o) in enumerate(zip(sizes, offs)):
        ctx.gen_segment_device(spec, s, data.data_ptr() + o, ln)
    torch.cuda.synchronize()
    segs = [(data.data_ptr() + o, ln) for (ln, _), o in zip(sizes, offs)]
    idx = ctx.replay_index(segs, on_device=True)
    n_live = len(idx.live)
    karena, koff = ctx.live_keys(n_live)
    kl = int(koff[1] - koff[0])
    assert ((koff[1:] - koff[:-1]) == kl).all()              # cfg2's keys: "k%015u"

    # the batch: n/2 overwrites of live keys, n/10 DELs of live keys, the rest new keys; shuffled
    n = args.ops
    rng = np.random.RandomState(11)
    n_over, n_del = n // 2, n // 10
    n_new = n - n_over - n_del
    lk = karena.reshape(n_live, kl)
    new = np.frombuffer(b"".join(b"n%0*d" % (kl - 1, i) for i in range(n_new)), dtype=np.uint8).reshape(n_new, kl)
    keys = np.concatenate([lk[rng.randint(0, n_live, n_over)], lk[rng.randint(0, n_live, n_del)], new])
    ops = np.concatenate([np.zeros(n_over, np.uint8), np.ones(n_del, np.uint8), np.zeros(n_new, np.uint8)])
    perm = rng.permutation(n)
    keys, ops = np.ascontiguousarray(keys[perm]), np.ascontiguousarray(ops[perm])
    vlen = np.where(ops == 0, 1024, 0).astype(np.uint64)
    voff = np.zeros(n + 1, dtype=np.uint64)
    voff[1:] = np.cumsum(vlen)
    boff = np.arange(n + 1, dtype=np.uint64) * np.uint64(kl)
    vbytes = int(voff[-1])
    out_bytes = int((5 + kl) * n + (ops == 0).sum() * 4 + vbytes)

    d_ops = torch.from_numpy(ops).to(dev)
    d_keys = torch.from_numpy(keys.reshape(-1)).to(dev)
    d_koff = torch.from_numpy(boff.astype(np.int64)).to(dev)
    d_vals = torch.randint(0, 256, (vbytes + 256,), dtype=torch.uint8, device=dev)
    d_voff = torch.from_numpy(voff.astype(np.int64)).to(dev)
    d_out = torch.empty(out_bytes + 256, dtype=torch.uint8, device=dev)
    d_tup = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    kp = (d_ops.data_ptr(), d_keys.data_ptr(), d_koff.data_ptr(), d_vals.data_ptr(), d_voff.data_ptr(), n)
    op = (d_out.data_ptr(), out_bytes + 256, d_tup.data_ptr())
    seg_id = args.segments

    # the copy yardstick of this run: the gather of a get of n random live keys (values left in HBM)
    pick = rng.randint(0, n_live, n)
    gk = torch.from_numpy(np.ascontiguousarray(lk[pick]).reshape(-1)).to(dev)
    g_idx = torch.empty(n, dtype=torch.int64, device=dev)
    g_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    g_bytes = int(idx.live["val_len"][pick].sum())
    g_vals = torch.empty(g_bytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gather = []
    for i in range(args.warmup + args.reps):
        g = ctx.get_batch(None, keys_ptr=(gk.data_ptr(), d_koff.data_ptr(), n),
                          out_ptrs=(g_idx.data_ptr(), g_off.data_ptr(), g_vals.data_ptr(), g_bytes + 256, None))
        assert g.status == K.OK and g.stats.n_found == n
        if i >= args.warmup:
            gather.append(g.stats.ms_gather)
    del gk, g_idx, g_off, g_vals

    rows, rebuild = [], []
    same = True
    for i in range(args.warmup + args.reps):
        if i:
            ctx.replay_index(segs, on_device=True)             # the state every repetition starts from
        t0 = time.perf_counter()
        r = ctx.put_batch(None, seg_id, keys_ptr=kp, out_ptrs=op)
        wall = (time.perf_counter() - t0) * 1e3
        assert r.status == K.OK and r.out_len == out_bytes and r.stats.n_ops == n
        st = r.stats
        put_live = ctx.index_fetch().live
        # (b) what the parent offered for the same result: the index rebuilt over store + new segment
        sid, sidx, ln, ptr = ctx.active_segment()
        t0 = time.perf_counter()
        full = ctx.replay_index(segs + [(ptr, ln)], on_device=True)
        rwall = (time.perf_counter() - t0) * 1e3
        same = same and np.array_equal(full.live, put_live)
        if i >= args.warmup:
            rows.append((st.ms_frame, st.ms_crc, st.ms_index, wall))
            rebuild.append((full.stats.ms_replay + full.stats.ms_fold, full.stats.ms_wall, rwall))
    fr, crc, ix, wall = [median(c) for c in zip(*rows)]
    rb_dev, rb_wall, rb_py = [median(c) for c in zip(*rebuild)]
    g_ms = median(gather)

    res = {
        "tool": "tools/put_bench.py", "lib_sha256_16": hashlib.sha256(open(K.lib_paths()[0], "rb").read()).hexdigest()[:16],
        "store": f"cfg2: {args.segments} x 64 MiB segments, 1 KiB values, uniform keys over 2^20",
        "store_bytes": int(sum(ln for ln, _ in sizes)), "n_live": int(n_live),
        "batch_ops": n, "batch_overwrites": n_over, "batch_dels": n_del, "batch_new_keys": n_new, "key_bytes": kl,
        "value_bytes": vbytes, "bytes_out": out_bytes, "n_superseded": int(st.n_superseded), "n_live_after": int(st.n_live),
        "reps": args.reps, "warmup": args.warmup,
        "a_ms_frame": fr, "a_ms_crc": crc,
        "a_frame_crc_gb_per_s": out_bytes / ((fr + crc) * 1e-3) / 1e9,
        "a_frame_tb_per_s_2x": 2 * out_bytes / (fr * 1e-3) / 1e12,
        "a_gather_ms": g_ms, "a_gather_tb_per_s_2v": 2 * g_bytes / (g_ms * 1e-3) / 1e12,
        "b_ms_index": ix, "b_rebuild_ms_device": rb_dev, "b_rebuild_ms_wall": rb_wall,
        "b_put_whole_call_ms_wall": wall, "b_index_speedup_over_rebuild_device": rb_dev / ix,
        "b_frame_plus_index_ms": fr + ix, "b_put_beats_rebuild": bool(ix < rb_dev),
        # the whole call also frames the batch, computes the ETags and copies out and tuples, which the rebuild (whose
        # appended bytes are already in HBM) does not: reported, not the comparison
        "b_call_wall_over_rebuild_wall": wall / rb_wall,
        "b_live_lists_equal": bool(same),
        "c_put_ms_wall": wall,
    }

    if not args.no_host:
        # (c) one host thread: the reference's loop and the host index update, over host copies
        host = data.cpu().numpy()
        hsegs = [host[o: o + ln] for (ln, _), o in zip(sizes, offs)]
        hvals = d_vals.cpu().numpy()[:vbytes]
        import ctypes as C
        _, hostlib = K.native()
        karr = np.ascontiguousarray(keys.reshape(-1))
        hout = np.zeros(out_bytes, dtype=np.uint8)                 # (touched before the clock starts)
        htup = np.zeros(n, dtype=K.TUPLE_DTYPE)
        ol = C.c_uint64()
        t0 = time.perf_counter()
        rc = hostlib.kvh_encode_batch(ops.ctypes.data, karr.ctypes.data, boff.ctypes.data, hvals.ctypes.data, voff.ctypes.data,
                                      n, args.segments, 0, hout.ctypes.data, out_bytes, C.byref(ol), htup.ctypes.data)
        t1 = time.perf_counter()
        assert rc == K.OK and ol.value == out_bytes
        hidx = K.host_index_update(K.Index(idx.live, idx.slots, None, None), hsegs + [hout], htup, (karr, boff))
        t2 = time.perf_counter()
        res["c_host_encode_ms"] = (t1 - t0) * 1e3
        res["c_host_index_ms"] = (t2 - t1) * 1e3
        res["c_host_total_ms"] = (t2 - t0) * 1e3
        res["c_speedup_over_host_1t"] = res["c_host_total_ms"] / wall
        res["c_host_live_equals_device"] = bool(np.array_equal(hidx.live, put_live))
        res["c_host_bytes_equal_device"] = bool(np.array_equal(hout, d_out.cpu().numpy()[:out_bytes]))

    os.makedirs(args.out, exist_ok=True)
    line = json.dumps(res)
    with open(os.path.join(args.out, f"put_bench_{res['lib_sha256_16']}.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()

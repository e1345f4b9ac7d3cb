"""Multi-get on the device against the host loop it replaces.

Builds the cfg2 store in HBM (kvr_gen_segment_device, as bench.py does), runs kvr_replay_index
once, then times kvr_get_batch over 1 M uniformly random live keys plus 10 % misses with keys and
outputs in device memory — the device events of kvr_last_get_stats, the median of --reps calls
after --warmup:
  (a) KVR_GET_LOCATE_ONLY                keys/s
  (b) the full get                       GiB/s of value bytes, ms_probe, ms_gather
  (c) (b) with KVR_GET_VERIFY            ms_verify
  (d) the host loop (kvh_get_many: kvr_index_find + memcpy) over a host copy of the index and the
      segments, on 1 and on 16 threads   wall time
Byte models: the gather moves 2 x value bytes (each read once, written once); the probe makes
three dependent random accesses per key (slot, tuple, key bytes in the segment) plus one per
further probe step.

  python tools/get_bench.py [--segments N] [--keys K] [--reps R] [--no-host] [--out DIR]
Prints one JSON line and writes it to DIR/get_bench_<library hash>.json (default bench_out/get).
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

HBM_COPY_TBS = 6.29   # measured copy rate of the MI355X (the gather's yardstick)


def median(x):
    return float(np.median(np.asarray(x, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "get"))
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

    # the batch: uniformly random live keys + 10 % keys that were never written, shuffled
    rng = np.random.RandomState(7)
    pick = rng.randint(0, n_live, args.keys)
    klen = (koff[1:] - koff[:-1]).astype(np.int64)
    assert (klen == klen[0]).all()              # cfg2's keys: "k%015u"
    kl = int(klen[0])
    live_keys = karena.reshape(n_live, kl)[pick]
    n_miss = args.keys // 10
    miss = np.frombuffer(b"".join(b"m%0*d" % (kl - 1, i) for i in range(n_miss)), dtype=np.uint8).reshape(n_miss, kl)
    batch = np.concatenate([live_keys, miss])
    rng.shuffle(batch)
    n = len(batch)
    arena = np.ascontiguousarray(batch).reshape(-1)
    boff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(kl))
    vbytes = int(idx.live["val_len"][pick].sum())

    d_keys = torch.from_numpy(arena).to(dev)
    d_koff = torch.from_numpy(boff.astype(np.int64)).to(dev)
    d_idx = torch.empty(n, dtype=torch.int64, device=dev)
    d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_vals = torch.empty(vbytes + 256, dtype=torch.uint8, device=dev)
    d_bad = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    kp = (d_keys.data_ptr(), d_koff.data_ptr(), n)
    op = (d_idx.data_ptr(), d_off.data_ptr(), d_vals.data_ptr(), vbytes + 256, d_bad.data_ptr())

    def timed(**kw):
        rows = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            r = ctx.get_batch(None, keys_ptr=kp, out_ptrs=op, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            assert r.status == K.OK and r.stats.n_found == args.keys and r.n_crc_fail == 0
            if i >= args.warmup:
                rows.append((r.stats.ms_probe, r.stats.ms_gather, r.stats.ms_verify, wall))
        return [median(c) for c in zip(*rows)]

    a = timed(values=False)
    b = timed()
    c = timed(verify=True)
    assert int(d_off[-1].item()) == vbytes
    gib = vbytes / 2.0 ** 30

    # average probe length over the batch, from the host copy of the table (hits: steps to the key's
    # entry; misses: steps to the free slot)
    rep, _ = K.native()
    mask = len(idx.slots) - 1
    tags = np.array([K.crc32(bytes(k)) for k in batch[:20000]], dtype=np.uint32)
    home = np.array([rep.kvr_index_hash(int(t)) for t in tags], dtype=np.uint64) & np.uint64(mask)
    li = d_idx.cpu().numpy()[:20000]
    steps = []
    for h, j in zip(home, li):
        s, h = 1, int(h)
        while idx.slots[h] != 0 and int(idx.slots[h]) - 1 != j:
            h = (h + 1) & mask
            s += 1
        steps.append(s)

    res = {
        "tool": "tools/get_bench.py", "lib_sha256_16": hashlib.sha256(open(K.lib_paths()[0], "rb").read()).hexdigest()[:16],
        "store": f"cfg2: {args.segments} x 64 MiB segments, 1 KiB values, uniform keys over 2^20",
        "store_bytes": int(sum(ln for ln, _ in sizes)), "n_live": int(n_live), "n_slots": int(len(idx.slots)),
        "batch_keys": int(n), "batch_hits": int(args.keys), "batch_misses": int(n_miss), "key_bytes": kl,
        "value_bytes": vbytes, "reps": args.reps, "warmup": args.warmup,
        "avg_probe_steps": float(np.mean(steps)),
        "a_locate_ms_probe": a[0], "a_locate_ms_wall": a[3], "a_locate_keys_per_s": n / (a[0] * 1e-3),
        "a_ns_per_key": a[0] * 1e6 / n,
        "b_get_ms_probe": b[0], "b_get_ms_gather": b[1], "b_get_ms_wall": b[3],
        "b_get_gib_per_s_device": gib / ((b[0] + b[1]) * 1e-3), "b_get_gib_per_s_wall": gib / (b[3] * 1e-3),
        "b_gather_tb_per_s_2v": 2 * vbytes / (b[1] * 1e-3) / 1e12,
        "b_gather_share_of_copy_rate": (2 * vbytes / (HBM_COPY_TBS * 1e12)) / (b[1] * 1e-3),
        "c_verify_ms_probe": c[0], "c_verify_ms_gather": c[1], "c_verify_ms_verify": c[2], "c_verify_ms_wall": c[3],
        "c_verify_gib_per_s_device": gib / ((c[0] + c[1] + c[2]) * 1e-3),
    }

    if not args.no_host:
        # (d) the host loop over a host copy of the index and the segments
        host = data.cpu().numpy()
        hsegs = [host[o: o + ln] for (ln, _), o in zip(sizes, offs)]
        want_idx = d_idx.cpu().numpy()
        want_vals = d_vals.cpu().numpy()[:vbytes]
        for th in (1, 16):
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                r = K.host_get_many(idx, (arena, boff), threads=th, segments=hsegs, vals_cap=vbytes)
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            assert r.status == K.OK and np.array_equal(r.live_idx, want_idx) and np.array_equal(r.values, want_vals)
            res[f"d_host_{th}t_ms"] = best
            res[f"d_host_{th}t_gib_per_s"] = gib / (best * 1e-3)
            res[f"d_host_{th}t_keys_per_s"] = n / (best * 1e-3)
        res["host_results_equal_device"] = True
        res["b_speedup_over_host_16t_wall"] = res["d_host_16t_ms"] / b[3]

    out = args.out
    os.makedirs(out, exist_ok=True)
    line = json.dumps(res)
    with open(os.path.join(out, f"get_bench_{res['lib_sha256_16']}.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()

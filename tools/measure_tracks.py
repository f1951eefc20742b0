"""Times the tracks stage (rfid_batch_tracks + rfid_batch_get_tracks) beside the host route it replaces, in one process on one GPU:

  device   rfid_batch_tracks_ms (HIP events, first launch to the end of the last) and the wall time of Context.batch_tracks_fetch()
  host     Context.batch_windows() (every window and result of the pass copied to numpy arrays) and a VECTORISED numpy grouping of
           them (numpy.unique over (trace, frame) + a stable sort, no Python loop over reads).  Its result is asserted equal to the
           device's, byte for byte, before its time counts.

  python tools/measure_tracks.py replicas [--streams 1024]      # configs[1]'s shape: noise replicas of the 71-round trace
  python tools/measure_tracks.py long [--rounds 2000]           # one FIXED_Q = 4 trace, 8 tags (10000 rounds: configs[2])

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
BIG = (1 << 31) - 2


def host_tracks(rfid, w, r, used):
    """windows + results of a pass (ordered by (stream, seq)) and n_windows_used per trace -> (reads, offsets) as the device lists them"""
    m = (r["type"] == 1) & (r["crc_ok"] == 1) & (w["seq"] < used[w["stream"]])
    w, r = w[m], r[m]
    n = len(w)
    reads = np.zeros(n, dtype=rfid.capi.TAG_READ_DTYPE)
    if n == 0:
        return reads, np.zeros(1, dtype=np.int64)
    key = np.empty((n, 5), dtype=np.uint32)
    key[:, 0] = w["stream"]
    key[:, 1:] = r["bits"]
    uniq, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    by_first = np.argsort(first, kind="stable")              # groups in the order of their first reads = (stream, first_seq)
    place = np.empty(len(uniq), dtype=np.int64)
    place[by_first] = np.arange(len(uniq))
    g = place[inverse]                                       # global entry index of every read
    order = np.argsort(g, kind="stable")                     # (the input is in (stream, seq) order: stable keeps seq ascending)
    w, r, g = w[order], r[order], g[order]
    ent_stream = uniq[by_first, 0].astype(np.int64)
    ent_base = np.concatenate([[0], np.cumsum(np.bincount(ent_stream, minlength=int(used.shape[0])))])
    reads["stream"], reads["seq"], reads["start"] = w["stream"], w["seq"], w["start"]
    reads["entry"] = g - ent_base[w["stream"]]
    reads["h_re"], reads["h_im"], reads["T"], reads["index"] = r["h_re"], r["h_im"], r["T"], r["index"]
    off = np.concatenate([[0], np.cumsum(np.bincount(g, minlength=len(uniq)))]).astype(np.int64)
    return reads, off


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shape", choices=["replicas", "long"])
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=2000)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--host-passes", type=int, default=3)
    args = ap.parse_args()
    import torch
    import rfid
    from rfid import synth
    if args.shape == "replicas":
        t = synth.make_trace(n_rounds=71, fixed_q=0, tag_ids=(0x27,), sigma=0.0, seed=7, corrupt_rounds=(36,), noise=False, render=False)
        ctx = rfid.Context(device=0)
        B, max_tags = args.streams, 4
    else:
        t = synth.make_trace(n_rounds=args.rounds, fixed_q=4, tag_ids=tuple(0x11 + 0x10 * k for k in range(8)), sigma=0.0, seed=2024,
                             noise=False, render=False)
        ctx = rfid.Context(device=0, fixed_q=4, max_num_queries=BIG)
        B, max_tags = 1, 64
    L = ctx.synth_gen2_size(t.plan)
    stride = (L + 1) & ~1
    if args.shape == "replicas":
        base = torch.zeros(2 * stride, dtype=torch.float32, device="cuda:0")
        data = torch.zeros((B, 2 * stride), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.synth_gen2_ptr(t.plan, base.data_ptr(), stride)
        ctx.synth_replicas_ptr(base.data_ptr(), L, data.data_ptr(), stride, B, 0.002, 777, first_replica=0)
    else:
        data = torch.zeros(2 * stride, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.synth_gen2_ptr(t.plan, data.data_ptr(), stride, sigma=0.002, seed=99)
    ctx.batch_sync()
    ctx.batch_plan(B, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_tracks()
    trk_ms, inv_ms, fetch_ms = [], [], []
    for _ in range(args.passes + 1):
        ctx.batch_process_ptr(data.data_ptr(), stride, L, 0)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_sync()
        t0 = time.perf_counter()
        reads, off = ctx.batch_tracks_fetch()
        fetch_ms.append((time.perf_counter() - t0) * 1e3)
        trk_ms.append(ctx.batch_tracks_ms())
        inv_ms.append(ctx.batch_inventory_ms())
    ent, counts = ctx.batch_inventory_fetch()
    used = ctx.batch_stats()["n_windows_used"].astype(np.int64)
    copy_ms, group_ms = [], []
    for _ in range(args.host_passes):
        t0 = time.perf_counter()
        w, r, _s = ctx.batch_windows()
        t1 = time.perf_counter()
        h_reads, h_off = host_tracks(rfid, w, r, used)
        t2 = time.perf_counter()
        assert h_reads.tobytes() == reads.tobytes() and np.array_equal(h_off, off), "the host route and the device disagree"
        copy_ms.append((t1 - t0) * 1e3)
        group_ms.append((t2 - t1) * 1e3)
    med = lambda xs: float(np.median(xs))
    print(json.dumps(dict(shape=args.shape, traces=B, raw_samples_per_trace=int(L), windows=int(len(w)), entries=int(len(ent)), reads=int(len(reads)),
                          tracks_ms=med(trk_ms[1:]), tracks_ms_all=[round(x, 4) for x in trk_ms[1:]], inventory_ms=med(inv_ms[1:]),
                          fetch_ms=med(fetch_ms[1:]), fetch_ms_all=[round(x, 3) for x in fetch_ms[1:]],
                          host_copy_ms=med(copy_ms), host_group_ms=med(group_ms), host_copy_ms_all=[round(x, 2) for x in copy_ms],
                          host_group_ms_all=[round(x, 2) for x in group_ms], device=torch.cuda.get_device_name(0))))
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

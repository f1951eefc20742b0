"""Times the fine stage (rfid_batch_fine: the data-aided channel estimate of every EPC window) beside the quality stage and the decoder
of the same pass, in one process on one GPU.  Both stages gather the same 512 samples per EPC window; the fine stage writes 128 bytes
per window where the quality stage writes 32.

  python tools/measure_fine.py replicas [--streams 1024]      # the headline shape: noise replicas of the 71-round trace
  python tools/measure_fine.py q4 [--streams 64 --rounds 40]  # a FIXED_Q = 4 batch, 8 tags
  python tools/measure_fine.py ragged                         # eight traces of 14 .. 7 rounds, FIXED_Q = 3, six tags

fine_ms / quality_ms / decode_ms: HIP events (rfid_batch_fine_ms, rfid_batch_quality_ms, rfid_batch_timing.decode_ms), median over
the passes behind a warm-up pass, and the least and the largest of them.  The two stages take turns in going first.  Prints one JSON
line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
BIG = (1 << 31) - 2


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shape", choices=["replicas", "q4", "ragged"])
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--passes", type=int, default=9)
    args = ap.parse_args()
    import torch
    import rfid
    from rfid import batch as rb
    from rfid import synth
    d_lens = 0
    if args.shape == "ragged":
        ts = [synth.make_trace(n_rounds=14 - k, fixed_q=3, tag_ids=(0x27, 0x27, 0x31, 0x31, 0x4C, 0x5A), seed=900 + k, sigma=0.03,
                               t1_jitter_raw=3).samples for k in range(8)]
        ctx = rfid.Context(device=0, fixed_q=3, max_num_queries=BIG)
        B, q, L = 8, 3, max(map(len, ts))
        stride = (L + 1) & ~1
        host = np.zeros((B, stride), dtype=np.complex64)
        for i, t in enumerate(ts):
            host[i, : len(t)] = t
        data = torch.from_numpy(host.view(np.float32)).to("cuda:0")
        lens = torch.from_numpy(np.array([len(t) for t in ts], dtype=np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        d_lens = lens.data_ptr()
    else:
        if args.shape == "replicas":
            t = synth.make_trace(n_rounds=71, fixed_q=0, tag_ids=(0x27,), sigma=0.0, seed=7, corrupt_rounds=(36,), noise=False, render=False)
            ctx = rfid.Context(device=0)
            B, q = args.streams or 1024, 0
        else:
            t = synth.make_trace(n_rounds=args.rounds, fixed_q=4, tag_ids=tuple(0x11 + 0x10 * k for k in range(8)), sigma=0.0, seed=2024,
                                 noise=False, render=False)
            ctx = rfid.Context(device=0, fixed_q=4, max_num_queries=BIG)
            B, q = args.streams or 64, 4
        L = ctx.synth_gen2_size(t.plan)
        stride = (L + 1) & ~1
        base = torch.zeros(2 * stride, dtype=torch.float32, device="cuda:0")
        data = torch.zeros((B, 2 * stride), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.synth_gen2_ptr(t.plan, base.data_ptr(), stride)
        ctx.synth_replicas_ptr(base.data_ptr(), L, data.data_ptr(), stride, B, 0.01, 777, first_replica=0)
        ctx.batch_sync()
    ctx.batch_plan(B, L)
    ctx.batch_plan_inventory(64)
    ctx.batch_plan_tracks()
    ctx.batch_plan_quality()
    ctx.batch_plan_fine()
    fine_ms, qual_ms, decode_ms = [], [], []
    for k in range(args.passes + 1):
        ctx.batch_process_ptr(data.data_ptr(), stride, L, d_lens)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        for stage in ((ctx.batch_fine_enqueue, ctx.batch_quality_enqueue) if k & 1 else (ctx.batch_quality_enqueue, ctx.batch_fine_enqueue)):
            stage()
        ctx.batch_sync()
        fine_ms.append(ctx.batch_fine_ms())
        qual_ms.append(ctx.batch_quality_ms())
        decode_ms.append(ctx.batch_timing()["decode_ms"])
    st = ctx.batch_stats()
    epc_windows = int((st["n_windows_used"] // 2).sum())
    f, reads = ctx.batch_fine_fetch(), ctx.batch_tracks_fetch()[0]
    qrec = ctx.batch_quality_fetch()
    ff = rb.fine_fields(f)
    h_est = reads["h_re"].astype(np.float64) + 1j * reads["h_im"].astype(np.float64)
    med = lambda xs: float(np.median(xs))
    span = lambda xs: [round(float(min(xs)), 4), round(float(max(xs)), 4)]
    f_ms, q_ms, d_ms = med(fine_ms[1:]), med(qual_ms[1:]), med(decode_ms[1:])
    print(json.dumps(dict(shape=args.shape, traces=B, fixed_q=q, raw_samples_per_trace=int(L), epc_windows=epc_windows, reads=int(len(f)),
                          fine_ms=f_ms, fine_ms_span=span(fine_ms[1:]), quality_ms=q_ms, quality_ms_span=span(qual_ms[1:]), decode_ms=d_ms,
                          fine_to_quality=f_ms / q_ms, fine_ms_all=[round(x, 4) for x in fine_ms[1:]],
                          quality_ms_all=[round(x, 4) for x in qual_ms[1:]],
                          aligned_with_the_tracks=bool(np.array_equal(f["seq"], reads["seq"]) and np.array_equal(f["seq"], qrec["seq"])),
                          median_hd_snr_db=med(ff["snr_db"]) if len(f) else None,
                          mean_abs_h_over_abs_h_est=float(np.mean(np.abs(ff["h"]) / np.abs(h_est))) if len(f) else None,
                          device=torch.cuda.get_device_name(0))))
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

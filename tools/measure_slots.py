"""Times the slots stage (rfid_batch_slots: the second-order moments of every window) beside the decoder of the same pass, in one
process on one GPU.  The decoder reads every window in full (12 960 bytes per slot) and is unchanged by the stage: the yardstick.
The stage reads 240 samples of every window (3 840 bytes per slot).

  python tools/measure_slots.py replicas [--streams 1024]      # the headline shape: noise replicas of the 71-round trace
  python tools/measure_slots.py q4 [--streams 64 --rounds 40]  # a FIXED_Q = 4 batch, 8 tags: most slots empty or collided

slots_ms / decode_ms: HIP events (rfid_batch_slots_ms, rfid_batch_timing.decode_ms), median over the passes behind a warm-up pass.
Prints one JSON line."""
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
    ap.add_argument("shape", choices=["replicas", "q4"])
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--passes", type=int, default=9)
    args = ap.parse_args()
    import torch
    import rfid
    from rfid import batch as rb
    from rfid import synth
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
    ctx.batch_plan_slots()
    slots_ms, decode_ms, total_ms = [], [], []
    for _ in range(args.passes + 1):
        ctx.batch_process_ptr(data.data_ptr(), stride, L, 0)
        ctx.batch_slots_enqueue()
        ctx.batch_sync()
        slots_ms.append(ctx.batch_slots_ms())
        tm = ctx.batch_timing()
        decode_ms.append(tm["decode_ms"])
        total_ms.append(tm["total_ms"])
    st = ctx.batch_stats()
    windows = int(st["n_windows_used"].sum())
    # what the records say about trace 0, against the slot table the trace was made from
    slots = rb.classify_slots(ctx.batch_window_moments(0))
    truth = np.array([min(int(s.n_tags), 2) for s in t.slots[: len(slots)]])
    med = lambda xs: float(np.median(xs))
    s_ms, d_ms = med(slots_ms[1:]), med(decode_ms[1:])
    print(json.dumps(dict(shape=args.shape, traces=B, fixed_q=q, raw_samples_per_trace=int(L), windows=windows,
                          slots_ms=s_ms, slots_ms_all=[round(x, 4) for x in slots_ms[1:]],
                          decode_ms=d_ms, decode_ms_all=[round(x, 4) for x in decode_ms[1:]], ratio=s_ms / d_ms,
                          pass_total_ms=med(total_ms[1:]),
                          bytes_read=windows * 1920, read_tb_per_s=windows * 1920 / (s_ms * 1e-3) / 1e12,
                          trace0_slots=int(len(slots)), trace0_misclassified=int((slots["cls"] != truth).sum()),
                          device=torch.cuda.get_device_name(0))))
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

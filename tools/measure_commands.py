"""Times the commands stage (rfid_batch_commands: the reader's PIE command in front of every window) beside the decoder and the slots
stage of the same pass, in one process on one GPU.  The stage reads 704 samples in front of every window (5 632 bytes per window).

  python tools/measure_commands.py replicas [--streams 1024]      # the headline shape: noise replicas of the 71-round trace
  python tools/measure_commands.py q4 [--streams 64 --rounds 40]  # a FIXED_Q = 4 batch, 8 tags

commands_ms / slots_ms / decode_ms: HIP events (rfid_batch_commands_ms, rfid_batch_slots_ms, rfid_batch_timing.decode_ms), median
over the passes behind a warm-up pass.  Prints one JSON line."""
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
    ctx.batch_plan_commands()
    ctx.batch_plan_slots()
    cmd_ms, slots_ms, decode_ms = [], [], []
    for _ in range(args.passes + 1):
        ctx.batch_process_ptr(data.data_ptr(), stride, L, 0)
        ctx.batch_commands_enqueue()
        ctx.batch_slots_enqueue()
        ctx.batch_sync()
        cmd_ms.append(ctx.batch_commands_ms())
        slots_ms.append(ctx.batch_slots_ms())
        decode_ms.append(ctx.batch_timing()["decode_ms"])
    st = ctx.batch_stats()
    windows = int(st["n_windows_used"].sum())
    # what the records say about trace 0, against the slot table the trace was made from
    # (and of EVERY trace: the replicas share the slot table, so every trace's commands, Q and ACKed RN16 are the plan's)
    want_all = [(1, int(s["q"]), -1) if int(s["cmd"]) == 0 else (2, -1, -1) for s in t.plan.slots]
    want_all = [x for w, s in zip(want_all, t.plan.slots) for x in (w, (3, -1, int(s["ack"])))]
    wrong = 0
    for b in range(B):
        g = rb.command_fields(ctx.batch_window_commands(b))
        names = {"query": 1, "queryrep": 2, "ack": 3}
        got = [(names.get(str(r["name"]), 0), int(r["q"]), int(r["rn16"])) for r in g]
        wrong += sum(x != y for x, y in zip(got, want_all)) + abs(len(got) - len(want_all))
    f = rb.command_fields(ctx.batch_window_commands(0))
    want = [n for s in t.plan.slots for n in ("query" if int(s["cmd"]) == 0 else "queryrep", "ack")][: len(f)]
    med = lambda xs: float(np.median(xs))
    c_ms, s_ms, d_ms = med(cmd_ms[1:]), med(slots_ms[1:]), med(decode_ms[1:])
    print(json.dumps(dict(shape=args.shape, traces=B, fixed_q=q, raw_samples_per_trace=int(L), windows=windows,
                          commands_ms=c_ms, commands_ms_all=[round(x, 4) for x in cmd_ms[1:]], slots_ms=s_ms, decode_ms=d_ms,
                          ratio_to_decode=c_ms / d_ms, bytes_read=windows * 5632, read_tb_per_s=windows * 5632 / (c_ms * 1e-3) / 1e12,
                          trace0_windows=int(len(f)), trace0_wrong_command=int(sum(a != b for a, b in zip(f["name"], want))),
                          trace0_acks_echoing=int((f["ack_echo"] == 1).sum()), windows_not_the_plans=int(wrong), device=torch.cuda.get_device_name(0))))
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

#!/usr/bin/env python3
"""bench.py -- Gen2 receive path (matched_filter -> gate -> tag_decoder) on MI355X.

One "step" = one pass of the whole hot path over a batch of synthetic traces already
resident in HBM.  Prints ONE JSON line.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config 1|2|3stream|4shard] [--full] [--dump-outputs DIR]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run builds the workload, warms up, times the K steps and prints the headline line.  --full adds everything
else: per-kernel times and roofline, the passes each waited for, the device's state, the workload's result check, the
streaming leg, the short configs[2] / configs[3] measurements and the CPU baseline.  --dump-outputs DIR writes what the
last timed step computed (window table, decoded results, per-trace statistics) as DIR/<name>.npy.

Workloads (BASELINE.json `configs`; the default -- the driver's line -- is configs[1]):
  --config 1        configs[1]: 1024 noise replicas per GPU of the 71-round file_source_test stand-in
  --config 2        configs[2]: ONE multi-tag inventory trace, FIXED_Q=4 (16 slots/round), 10 000 rounds
                    (~2.2 G raw samples, 17.5 GB), generated in HBM by the device-side Gen2 synthesiser
  --config 3stream  configs[3], the per-GPU workload: one long RX stream per GPU (different tags/seed per rank)
  --config 4shard   configs[4], the per-GPU shard: as many replicas of the 71-round trace as HBM holds
                    (~250 GB incl. the matched-filter output), full chain over all of them

Multi-GPU: one process per GPU, traces sharded per rank, no data-path collective (weak
scaling); torch.distributed is used only for the barrier and the max-over-ranks time.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0         # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s) -- `frac` is priced against this
HBM_ACHIEVABLE_GBS = 6300.0   # what a plain streaming kernel reaches on this part (same guide) -- `frac_of_achievable`
RN16_WIN, EPC_WIN = 250, 1370
PER_WINDOW_WS = 24 * 3 + 48 + 144      # window table + two compact lists + result + scores (bytes)
DUMP_BYTES = 64_000_000       # --dump-outputs: at most this many bytes of arrays in all
DUMP_SEED = 20261015          # --dump-outputs: the row sample of tables that do not fit (fixed: the same rows run after run)


def _usable_cores():
    """Host threads worth starting: the affinity mask, capped by a cgroup CPU quota if there is one."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(float(parts[0]) / float(parts[1]) + 0.999)))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f2:
                        n = min(n, max(1, int(q / int(f2.read().split()[0]) + 0.999)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def cpu_baseline(x, seconds_target, fixed_q=0, what="1 replica of the workload trace"):
    """The oracle (CPU port of the reference algorithm) timed on this host on a bounded sample `x` of the
    workload -- first on one thread (the reference is single-threaded per stream; per-stage split), then
    one independent copy per host core at once (`value`, `cores`)."""
    from oracle import oracle
    cfg = oracle.config(fixed_q=fixed_q, max_num_queries=1 << 30)
    t = oracle.time_trace(x, reps=1, cfg=cfg)
    t_pass = max(t["total_s"], 1e-4)
    reps1 = max(1, min(20000, int(0.5 * seconds_target / t_pass)))
    t = oracle.time_trace(x, reps=reps1, cfg=cfg)
    msps1 = len(x) * reps1 / t["total_s"] / 1e6
    cores = _usable_cores()
    # calibrate the all-cores leg with one pass per thread, then size it to ~half the time budget of wall time
    cal = oracle.time_trace_mt(x, reps=1, nthreads=cores, cfg=cfg)
    reps_mt = max(1, min(20000, int(0.5 * seconds_target / max(cal["wall_s"], 1e-4))))
    m = oracle.time_trace_mt(x, reps=reps_mt, nthreads=cores, cfg=cfg)
    msps = len(x) * reps_mt * cores / m["wall_s"] / 1e6
    return {"value": round(msps, 3), "unit": "Msamples/s", "cores": cores, "kind": "port",
            "sample": f"{cores} host threads x {reps_mt} passes over {what} ({len(x)} raw samples "
                      f"each) in {m['wall_s']:.2f} s wall, oracle/rfid_oracle.c; one thread alone: {reps1} passes, "
                      f"FIR {t['fir_s']:.2f}s + gate/decoder {t['gate_decoder_s']:.2f}s",
            "single_thread_msamples_per_s": round(msps1, 3),
            "epc_per_s": round(m["n_epc_correct"] * reps_mt * cores / m["wall_s"], 1)}


# ---------------------------------------------------------------------------------------------------
# workloads: each returns a dict(data, ptr, stride, L, B, fixed_q, describe, check(stats)->(ok, text), sample())
# ---------------------------------------------------------------------------------------------------
def _fst_plan(synth):
    """Slot table of the noise-free 71-round stand-in for misc/data/file_source_test (one EPC corrupted)."""
    return synth.make_trace(n_rounds=71, fixed_q=0, tag_ids=(0x27,), sigma=0.0, seed=7, corrupt_rounds=(36,),
                            noise=False, render=False)


def _replicas(torch, ctx, device, plan, B, sigma, seed, first_replica):
    """The plan's trace built in HBM by the device-side Gen2 synthesiser, then B noise replicas of it by the
    replica generator (replica index = first_replica + row).  torch only owns the buffers."""
    L = ctx.synth_gen2_size(plan)
    stride = (L + 1) & ~1
    base = torch.zeros(2 * stride, dtype=torch.float32, device=device)
    data = torch.empty((B, 2 * stride), dtype=torch.float32, device=device)
    torch.cuda.synchronize()     # the library runs on its own (non-blocking) stream: torch's fills must be over
    ctx.synth_gen2_ptr(plan, base.data_ptr(), stride, sigma=0.0)
    ctx.synth_replicas_ptr(base.data_ptr(), L, data.data_ptr(), stride, B, sigma, seed, first_replica=first_replica)
    if stride != L:
        data[:, 2 * L:] = 0
    ctx.batch_sync()
    return data, base, L, stride


def workload_replicas(torch, rfid, synth, args, device, rank, B, tag):
    t = _fst_plan(synth)
    ctx = rfid.Context(device=device.index)
    data, base, L, stride = _replicas(torch, ctx, device, t.plan, B, args.sigma, args.seed, rank * B)

    def check(st):
        ok = bool((st["n_epc_correct"] == 70).all() and (st["n_queries_sent"] == 72).all()
                  and (st["tag_reads"][:, 0x27] == 70).all() and (st["n_unique_tags"] == 1).all())
        return ok, ("ok: every replica 70/71 EPC, tag 0x27" if ok else
                    "FAILED: %d EPC ok, expected %d" % (int(st["n_epc_correct"].sum()), 70 * B))

    def sample():
        rng = np.random.default_rng(123)
        b = base.cpu().numpy().view(np.complex64)[:L]
        n = rng.standard_normal((L, 2), dtype=np.float32)
        return (b + np.float32(args.sigma) * (n[:, 0] + 1j * n[:, 1])).astype(np.complex64), "1 replica of the workload trace"

    return dict(ctx=ctx, data=data, stride=stride, L=L, B=B, fixed_q=0, check=check, sample=sample,
                describe="%s: batch of %d noise-replicas per GPU of the 71-round file_source_test stand-in trace, "
                         "FM0 40 kHz BLF @ 2 Msps (%d raw I/Q samples each, sigma=%g), generated and resident in HBM"
                         % (tag, B, L, args.sigma))


def workload_single_trace(torch, rfid, synth, args, device, rank, fixed_q, n_rounds, n_tags, tag, reuse=None):
    """One long trace built in HBM from its slot table (different tags / seed per rank).  reuse: a workload of the same shape whose
    context and buffer are used again (the trace is synthesised anew, with args.sigma)."""
    tag_ids = tuple(((0x11 + 0x10 * k + rank) & 0xFF) for k in range(n_tags))
    t0 = time.perf_counter()
    kw = {} if args.leak_phase is None else {"leak": complex(np.cos(args.leak_phase), np.sin(args.leak_phase))}
    t = synth.make_trace(n_rounds=n_rounds, fixed_q=fixed_q, tag_ids=tag_ids, sigma=0.0, seed=args.seed + rank,
                         noise=False, render=False, **kw)
    plan_s = time.perf_counter() - t0
    ctx = reuse["ctx"] if reuse else rfid.Context(device=device.index, fixed_q=fixed_q, max_num_queries=(1 << 31) - 2)
    L = ctx.synth_gen2_size(t.plan)
    stride = (L + 1) & ~1
    if reuse:
        assert reuse["L"] == L and reuse["stride"] == stride
        ctx.batch_sync()
        data = reuse["data"]
    else:
        data = torch.zeros((1, 2 * stride), dtype=torch.float32, device=device)
    torch.cuda.synchronize()
    ctx.synth_gen2_ptr(t.plan, data.data_ptr(), stride, sigma=args.sigma, seed=args.seed, replica=rank)
    ctx.batch_sync()
    n_slots = len(t.slots)
    n_valid = sum(1 for s in t.slots if s.epc_valid)
    hist = np.zeros(256, dtype=np.int64)
    for s in t.slots:
        if s.epc_valid:
            hist[s.tag_id] += 1

    def check(st):
        # every single-responder slot's EPC must be CRC-verified; collided / empty slots decode noise and pass the
        # 16-bit CRC by chance with probability 2^-16 each (a handful among 10^5 such slots).  At SURVEY 8(d)'s stress noise
        # levels the weakest tag's frames fail now and then in the reference's decoder too (sigma = 0.06: 18 of 50 887 in
        # configs[2], the oracle's count): a few per mille may miss there; tests/test_gpu_configs.py compares every window with the oracle
        reads = st[0]["tag_reads"].astype(np.int64)
        missed = int(np.maximum(hist - reads, 0).sum())
        extra = int(np.maximum(reads - hist, 0).sum())
        allow = int(n_valid * (0.003 if args.sigma >= 0.05 else (0.0005 if args.sigma >= 0.02 else 0.0)))
        ok = bool(st[0]["n_windows"] == 2 * n_slots and 0 <= extra <= 12 and missed <= allow
                  and int(st[0]["n_epc_correct"]) == n_valid - missed + extra
                  and st[0]["n_queries_sent"] == n_slots + 1
                  and st[0]["cur_inventory_round"] == n_slots // (1 << fixed_q) + 1)
        return ok, ("ok: %d slots -> %d RN16 + %d EPC windows, %s single-responder EPCs CRC-verified with the slot "
                    "table's tag ids (+%d chance CRC passes among the %d collided/empty slots)"
                    % (n_slots, n_slots, n_slots, ("all %d" % n_valid) if missed == 0 else ("%d of %d (sigma=%g: %d lost to noise, <= %d allowed)" % (n_valid - missed, n_valid, args.sigma, missed, allow)),
                       extra, n_slots - n_valid)
                    if ok else "FAILED: windows %d (want %d), EPC ok %d (want >= %d)"
                    % (int(st[0]["n_windows"]), 2 * n_slots, int(st[0]["n_epc_correct"]), n_valid - allow))

    def sample():
        n = min(L, 24_000_000)     # the first ~1 750 slots of the trace
        x = data[0, : 2 * n].cpu().numpy().view(np.complex64)
        return x, "the first %d raw samples of the workload trace" % n

    return dict(ctx=ctx, data=data, stride=stride, L=L, B=1, fixed_q=fixed_q, check=check, sample=sample,
                describe="%s: one RX trace per GPU, FIXED_Q=%d (%d slots/round), %d rounds, %d tags (collisions and "
                         "empty slots included), FM0 40 kHz BLF @ 2 Msps: %d raw I/Q samples (%.1f GB), sigma=%g, built in "
                         "HBM by rfid_synth_gen2 from a %d-slot table (host planning %.1f s)%s"
                         % (tag, fixed_q, 1 << fixed_q, n_rounds, n_tags, L, 8e-9 * L, args.sigma, n_slots, plan_s,
                            "" if args.leak_phase is None else ", carrier leak phase %g rad" % args.leak_phase))


def streaming_leg(torch, rfid, wl, args, device):
    """The drop-in path from HOST memory, end to end: one RX stream (the first --stream-replicas replicas of the
    workload back to back = 71 x K inventory rounds) lies in page-locked host memory and goes through rfid_stream_work
    chunk by chunk -- DMA to HBM, matched filter, gate, tag_decoder, decoded windows back -- with the upload of chunk
    k+1 overlapping the processing of chunk k.  PCIe-inclusive, never the headline `value`."""
    K = min(args.stream_replicas, wl["B"])
    L, stride = wl["L"], wl["stride"]
    if stride != L:
        return None
    n_total = K * L
    host = torch.empty(2 * n_total, dtype=torch.float32, pin_memory=True)
    host.copy_(wl["data"][:K].reshape(-1)[: 2 * n_total])
    torch.cuda.synchronize()
    x = host.numpy().view(np.complex64)
    ctx = rfid.Context(device=device.index, max_num_queries=(1 << 31) - 2)
    try:
        chunk = min(args.stream_chunk, n_total)
        ctx.stream_begin(chunk)
        best = None
        for rep in range(3):
            if rep:
                ctx.stream_end()
                ctx.stream_begin(chunk)
            n_win, n_ok = 0, 0
            t0 = time.perf_counter()
            for pos in range(0, n_total, chunk):
                w, r = ctx.stream_work(x[pos:pos + chunk])
                n_win += len(w); n_ok += int(r["crc_ok"].sum())
            w, r = ctx.stream_work(flush=True)
            n_win += len(w); n_ok += int(r["crc_ok"].sum())
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        ok = (n_win == 142 * K and n_ok == 70 * K)
        return {"msamples_per_s": round(n_total / best / 1e6, 1), "host_gb_per_s": round(8e-9 * n_total / best, 2),
                "stream_raw_samples": n_total, "chunk_raw_samples": chunk, "calls": (n_total + chunk - 1) // chunk + 1,
                "source": "page-locked host memory (a pinned torch tensor), uploaded by DMA from where it lies",
                "check": ("ok: %d windows, %d of %d EPCs CRC-verified" % (n_win, n_ok, 71 * K)) if ok else
                         ("FAILED: %d windows, %d EPC ok" % (n_win, n_ok)),
                "note": "rfid_stream_work: raw chunk in -> decoded windows out, block state carried on the device; best of 3"}
    finally:
        ctx.close()


def timed_path_outputs(ctx, budget):
    """What a caller of the timed path receives from its last pass: the window table and the decoded results (ordered by
    trace and window; the pass runs without scores) and the per-trace statistics.  -> {name: array}, one array per record
    field: float fields as float32 (bit for bit), integer fields as float64 (exact).  When the arrays would exceed `budget`
    bytes, every table keeps the same share of its rows, drawn with a fixed seed (the same rows for the same shapes);
    `windows_row` / `stats_row` are the rows kept (the results share the windows' rows)."""
    w, r, _ = ctx.batch_windows(want_scores=False)
    st = ctx.batch_stats()
    groups = [("windows", (("windows", w), ("results", r))), ("stats", (("stats", st),))]

    def fields(a):
        return [f for f in a.dtype.names if not f.endswith("_")]

    def row_bytes(a):
        return sum((4 if a.dtype[f].base.kind == "f" else 8) * int(np.prod(a.dtype[f].shape)) for f in fields(a))

    sizes = [(len(tabs[0][1]), 8 + sum(row_bytes(a) for _, a in tabs)) for _, tabs in groups]
    total = sum(n * b for n, b in sizes)
    budget -= 256 * sum(1 + sum(len(fields(a)) for _, a in tabs) for _, tabs in groups)     # (each file's .npy header)
    share = 1.0 if total <= budget else budget / total
    out = {}
    for (gname, tabs), (n, _) in zip(groups, sizes):
        if share < 1.0:
            rows = np.sort(np.random.default_rng(DUMP_SEED).choice(n, int(n * share), replace=False))
        else:
            rows = np.arange(n)
        out[gname + "_row"] = rows.astype(np.float64)
        for tname, a in tabs:
            for f in fields(a):
                v = a[f][rows]
                out["%s_%s" % (tname, f)] = np.ascontiguousarray(v, dtype=np.float32 if v.dtype.kind == "f" else np.float64)
    return out


def write_outputs(dirpath, arrays, prefix=""):
    os.makedirs(dirpath, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirpath, prefix + name + ".npy"), a)


WAKE_S = 0.08      # seconds of the workload's own passes before the warm-up steps (see measure())


# ---------------------------------------------------------------------------------------------------
# device_state: what the device's clocks / power / temperature were around the timed region.  Boxes of the pool differ by
# +-3-7 % on an untouched kernel (2.40 -> 2.56 ms); this is what lets a reader attribute that.  sysfs only
# (readable by an ordinary user), sampled by a thread every few ms while the timed region's passes run ONCE MORE right behind it
# (inside it the reads cost the headline 3 - 6 %: measure()); rocm-smi once, before the workload is built.
# ---------------------------------------------------------------------------------------------------
def _sysfs_card(torch, device):
    """The /sys/class/drm/cardN/device directory of `device` (matched by PCI address; else the index-th amdgpu card)."""
    import glob
    cards = []
    for d in sorted(glob.glob("/sys/class/drm/card[0-9]*/device")):
        try:
            if open(os.path.join(d, "vendor")).read().strip() == "0x1002" and os.path.exists(os.path.join(d, "pp_dpm_sclk")):
                cards.append(d)
        except OSError:
            continue
    try:
        pr = torch.cuda.get_device_properties(device)
        want = "%04x:%02x:%02x" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        for d in cards:
            if want in os.path.realpath(d):
                return d
    except Exception:
        pass
    idx = device.index or 0
    return cards[idx] if idx < len(cards) else (cards[0] if cards else None)


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def _dpm_current(text):
    """'0: 132Mhz\n1: 2400Mhz *' -> 2400 (the starred level; a single level counts as current)."""
    if not text:
        return None
    lines = [ln for ln in text.splitlines() if ln.strip()]
    pick = [ln for ln in lines if "*" in ln] or (lines if len(lines) == 1 else [])
    if not pick:
        return None
    m = re.search(r"(\d+(?:\.\d+)?)\s*[Mm][Hh]z", pick[0])
    return float(m.group(1)) if m else None


class DeviceStateSampler:
    """Samples sclk / mclk / power / temperature from sysfs on a thread while a region runs."""

    def __init__(self, torch, device, period_s=0.004):
        import glob
        self.card = _sysfs_card(torch, device)
        self.period = period_s
        self.samples = []
        self._stop = False
        self._thread = None
        self.hwmon = None
        if self.card:
            hw = sorted(glob.glob(os.path.join(self.card, "hwmon", "hwmon*")))
            self.hwmon = hw[0] if hw else None

    def _one(self):
        c, h = self.card, self.hwmon
        s = {"t": time.perf_counter()}
        if c:
            s["sclk_mhz"] = _dpm_current(_read(os.path.join(c, "pp_dpm_sclk")))
            s["mclk_mhz"] = _dpm_current(_read(os.path.join(c, "pp_dpm_mclk")))
            b = _read(os.path.join(c, "gpu_busy_percent"))
            s["busy_pct"] = int(b) if b and b.isdigit() else None
        if h:
            for key, names, scale in (("power_w", ("power1_average", "power1_input"), 1e-6),
                                      ("temp_edge_c", ("temp1_input",), 1e-3), ("temp_junction_c", ("temp2_input",), 1e-3),
                                      ("temp_mem_c", ("temp3_input",), 1e-3)):
                for n in names:
                    v = _read(os.path.join(h, n))
                    if v and v.lstrip("-").isdigit():
                        s[key] = round(int(v) * scale, 1)
                        break
        return s

    def start(self):
        if not self.card:
            return
        import threading

        def loop():
            while not self._stop:
                self.samples.append(self._one())
                time.sleep(self.period)
        self._thread = threading.Thread(target=loop, daemon=True)
        self._thread.start()

    def stop(self):
        self._stop = True
        if self._thread is not None:
            self._thread.join(timeout=1.0)

    def summary(self, t0=None, t1=None):
        ss = [s for s in self.samples if (t0 is None or s["t"] >= t0) and (t1 is None or s["t"] <= t1)] or self.samples
        out = {"samples": len(ss), "period_ms": round(1e3 * self.period, 1)}
        for key in ("sclk_mhz", "mclk_mhz", "power_w", "temp_edge_c", "temp_junction_c", "temp_mem_c", "busy_pct"):
            v = [s[key] for s in ss if s.get(key) is not None]
            if v:
                out[key] = {"min": min(v), "median": statistics.median(v), "max": max(v)}
        return out


def device_state_static(torch, device):
    """Power cap, clock table, driver / runtime versions: read once, outside every timed region."""
    card = _sysfs_card(torch, device)
    out = {"sysfs": card}
    if card:
        import glob
        hw = sorted(glob.glob(os.path.join(card, "hwmon", "hwmon*")))
        if hw:
            for n in ("power1_cap", "power1_cap_max", "power1_cap_default"):
                v = _read(os.path.join(hw[0], n))
                if v and v.isdigit():
                    out[n + "_w"] = round(int(v) * 1e-6, 1)
        for n in ("pp_dpm_sclk", "pp_dpm_mclk", "pp_dpm_fclk"):
            v = _read(os.path.join(card, n))
            if v:
                out[n] = " | ".join(ln.strip() for ln in v.splitlines())
        out["power_dpm_force_performance_level"] = _read(os.path.join(card, "power_dpm_force_performance_level"))
        out["vbios_version"] = _read(os.path.join(card, "vbios_version"))
    out["amdgpu_driver"] = _read("/sys/module/amdgpu/version")
    out["kernel"] = os.uname().release
    out["hip_runtime"] = getattr(torch.version, "hip", None)
    out["torch"] = torch.__version__
    try:
        import subprocess
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--showtemp", "--showperflevel", "--showmaxpower", "--json"],
                           capture_output=True, text=True, timeout=20)
        if r.returncode == 0 and r.stdout.strip():
            j = json.loads(r.stdout.strip().splitlines()[-1])
            k = "card%d" % (device.index or 0)
            out["rocm_smi_idle"] = j.get(k, j)
    except Exception as e:
        out["rocm_smi_idle"] = "unavailable: %r" % (e,)
    return out


def measure(torch, wl, steps, warmup, barrier, gather_elapsed=None, n_series=None, back_to_back=True, wake_s=None,
            full=True, collect=None):
    """`warmup` untimed passes, then exactly `steps` timed passes of the workload's whole chain, enqueued one behind the other
    and waited for once (bracketed by `barrier()`, which synchronises the device; back_to_back=False: every pass waited for
    by itself, as rounds 1-3 timed it -- the profiled runs use that, a kernel trace then holds no queueing), then (full) an
    untimed series of the same passes read out through HIP events per kernel.  collect(): called right behind the timed
    region, its value returned as `outputs`.  full=False stops there (the passes' statistics read once).
    -> dict(elapsed, step_s, k_ms, k_min, k_med, alg, key, n_launch, rep, st, parity_ok, parity_text, roof, outputs, ...)"""
    ctx, data, stride, L, B = wl["ctx"], wl["data"], wl["stride"], wl["L"], wl["B"]
    ctx.batch_plan(B, L)
    ptr = data.data_ptr()

    def step():
        ctx.batch_process_ptr(ptr, stride, L, 0, want_scores=False)
        ctx.batch_sync()

    # the device's clocks: a GPU that has idled through the host's set-up work (planning a trace, building contexts) takes some
    # tens of ms of load to reach its sustained clocks -- 5 warm-up passes of 2.7 ms end before that, and the first ten passes
    # then run 3 % slower than every later one (profiles/r04/bench_warm.txt).  The same passes are run for WAKE_S of wall
    # time before the W warm-up steps; neither is timed.
    wake_t0, wake_n = time.perf_counter(), 0
    while time.perf_counter() - wake_t0 < (WAKE_S if wake_s is None else wake_s) and wake_n < 4000:
        step()
        wake_n += 1
    wake_ms = 1e3 * (time.perf_counter() - wake_t0)
    for _ in range(warmup):
        step()

    # ---- the timed region: exactly `steps` passes, nothing else -------------------------------------------------------
    step_s = []
    barrier()
    t0 = time.perf_counter()
    if back_to_back:
        for _ in range(steps):
            ctx.batch_process_ptr(ptr, stride, L, 0, want_scores=False)
        ctx.batch_sync()
    else:
        for _ in range(steps):
            ts = time.perf_counter()
            step()
            step_s.append(time.perf_counter() - ts)
    barrier()
    elapsed = time.perf_counter() - t0
    ms_by_rank = [1e3 * elapsed / steps]
    if gather_elapsed is not None:
        every = gather_elapsed(elapsed)               # control plane only: every rank's time; the job's = the slowest
        ms_by_rank = [1e3 * t / steps for t in every]
        elapsed = max(every)
    outputs = collect() if collect is not None else None
    b2b_ms = (1e3 * elapsed / steps) if back_to_back else None
    if not full:
        st = ctx.batch_stats()
        return dict(elapsed=elapsed, step_s=step_s, b2b_ms=b2b_ms, wake={"passes": wake_n, "ms": round(wake_ms, 1)},
                    ms_by_rank=ms_by_rank, st=st, n_epc_ok=int(st["n_epc_correct"].sum()), n_windows=int(st["n_windows"].sum()),
                    outputs=outputs)

    # ---- kernel durations: HIP events on the ctx stream around each launch, read in a separate (untimed)
    #      series of the same passes so that the event reads stay out of the timed region -----------------
    k_series = {"mf_ms": [], "gate_ms": [], "decode_ms": [], "stats_ms": [], "front_ms": []}
    launches = {"front_chunks": 1, "decode_launches": 2}
    fused = ls_fused = False
    for _ in range(n_series if n_series is not None else max(3, min(steps, 20))):
        step()
        t = ctx.batch_timing()
        for k in k_series:
            k_series[k].append(t[k])
        launches = {"front_chunks": int(t["front_chunks"]), "decode_launches": int(t["decode_launches"])}
        fused = int(t["fused_front"]) == 1          # front_end_fused_kernel (many traces)
        ls_fused = int(t["fused_front"]) == 2       # the long-stream front end with its fused first pass (few, long traces)
    # the same passes each waited for by itself (outside the timed region; how rounds 1-3 timed a step): the host's wait and
    # the next submission then lie between two passes -- and the matched filter of a long-stream pass cannot run beside the
    # front end of the pass before
    torch.cuda.synchronize()
    if back_to_back:
        for _ in range(steps):
            ts = time.perf_counter()
            step()
            step_s.append(time.perf_counter() - ts)
    # the device's state under this load: the SAME K passes once more, behind everything that is measured, with a thread reading sysfs
    # every 4 ms (clocks / power / temperature).  Not inside the timed region: there the reads cost the headline 3 - 6 % (the
    # first half of round 6 sampled inside: 2.84 ms per pass against 2.67 - 2.76 for round 5's tree on the same box -- hwmon and
    # pp_dpm reads go to the SMU -- and the kernel series right behind such a region still ran 6 % slow: profiles/r06/
    # device_state_sampling.txt); the replay's own time is reported beside the samples
    sampler = DeviceStateSampler(torch, data.device)
    sampler.start()
    r0 = time.perf_counter()
    if back_to_back:
        for _ in range(steps):
            ctx.batch_process_ptr(ptr, stride, L, 0, want_scores=False)
        ctx.batch_sync()
    else:
        for _ in range(steps):
            step()
    r1 = time.perf_counter()
    sampler.stop()
    dev_state = sampler.summary(r0, r1)
    if isinstance(dev_state, dict):
        dev_state["replay_ms_per_step"] = round(1e3 * (r1 - r0) / steps, 4)
    k_ms = {k: statistics.fmean(v) for k, v in k_series.items()}
    k_min = {k: min(v) for k, v in k_series.items()}
    k_med = {k: statistics.median(v) for k, v in k_series.items()}

    # ---- result checks (size-independent properties of the workload) ----------------------
    st = ctx.batch_stats()
    n_epc_ok = int(st["n_epc_correct"].sum())
    n_windows = int(st["n_windows"].sum())
    parity_ok, parity_text = wl["check"](st)

    # ---- roofline: algorithmic bytes per launch / measured kernel time
    n_dec = L // 5
    n_rn16 = int(n_windows // 2 + n_windows % 2)
    n_epc = int(n_windows // 2)
    dec_bytes = n_rn16 * (8.0 * RN16_WIN + 48) + n_epc * (8.0 * EPC_WIN + 48)
    if fused:
        # rfid_batch_process() default: one front-end launch (matched filter inside the gate's filter
        # waves): reads every raw sample once, writes y once for the decoder, writes the window records
        alg = {"front_end_fused": B * (8.0 * L + 8.0 * n_dec) + 24.0 * n_windows, "tag_decoder": dec_bytes}
        key = {"front_end_fused": "gate_ms", "tag_decoder": "decode_ms"}
        n_launch = {"front_end_fused": 1, "tag_decoder": launches["decode_launches"]}
    else:
        alg = {"mf_boxcar25_decim5": B * (8.0 * L + 8.0 * n_dec),
               "gate_scan": B * 8.0 * n_dec + 24.0 * n_windows, "tag_decoder": dec_bytes}
        key = {"mf_boxcar25_decim5": "mf_ms", "gate_scan": "gate_ms", "tag_decoder": "decode_ms"}
        n_launch = {"mf_boxcar25_decim5": launches["front_chunks"], "gate_scan": launches["front_chunks"],
                    "tag_decoder": launches["decode_launches"]}
    rep = ctx.batch_ls_report()
    if ls_fused:
        # the long-stream front end, matched filter inside its first launch (round 5): the whole launch sequence -- fused first
        # pass, chains, re-runs, state machine, dc_est, assembly, the self-skipping fallback -- is timed and priced as ONE unit
        # that reads every raw sample once, writes y once for the decoder and writes the window records
        alg = {"front_long_stream": B * (8.0 * L + 8.0 * n_dec) + 24.0 * n_windows, "tag_decoder": dec_bytes}
        key = {"front_long_stream": "gate_ms", "tag_decoder": "decode_ms"}
        n_launch = {"front_long_stream": 1, "tag_decoder": launches["decode_launches"]}
    elif rep["pieces"] and not fused:
        # the gate ran as the long-stream front end: its launch sequence (cut searches, avg_ampl / state machine / dc_est
        # rounds, assembly, the self-skipping sequential scan behind them) is timed and priced as ONE unit
        alg = {("gate_long_stream" if k == "gate_scan" else k): v for k, v in alg.items()}
        key = {("gate_long_stream" if k == "gate_scan" else k): v for k, v in key.items()}
        n_launch = {("gate_long_stream" if k == "gate_scan" else k): (1 if k == "gate_scan" else v) for k, v in n_launch.items()}
    traffic, traffic_source = {}, None
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            pt = json.load(f)
        for ent in [pt] + list(pt.get("other_workloads", [])):     # (configs[1]; configs[2] and configs[3]'s stream since round 5)
            if ent.get("streams") == B and ent.get("raw_per_stream") == L:
                traffic = ent.get("hbm_bytes_per_step", {})
                traffic_source = ("profiles/pmc_traffic.json: rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE passes of "
                                  "this workload (%s); a committed cross-reference, NOT measured in this run" % ent.get("source", "?"))
                break
    except Exception:
        pass

    def roof(name):
        # a pass issues n_launch launches of this kernel (time chunks / window types), each moving
        # 1/n_launch of the bytes: the per-launch ratio equals the per-pass ratio
        nl = max(1, n_launch[name])
        dur = k_ms[key[name]]
        ach = alg[name] / (dur * 1e-3) / 1e9 if dur > 0 else 0.0
        tr = traffic.get(name)
        return {"kernel": name, "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(ach / HBM_PEAK_GBS, 4),
                "achievable_peak": HBM_ACHIEVABLE_GBS, "frac_of_achievable": round(ach / HBM_ACHIEVABLE_GBS, 4),
                "traffic": (int(tr / nl) if tr else None),
                "traffic_source": traffic_source if tr else None,
                "algorithmic_bytes": int(alg[name] / nl), "launches_per_step": nl,
                "avg_launch_ms": round(dur / nl, 4), "ms_per_step": round(dur, 4),
                "min_ms_per_step": round(k_min[key[name]], 4), "median_ms_per_step": round(k_med[key[name]], 4),
                "timing": "HIP events on the library's stream around each launch, %d untimed passes after the timed region"
                          % len(k_series["gate_ms"])}

    return dict(elapsed=elapsed, step_s=step_s, b2b_ms=b2b_ms, dev_state=dev_state, wake={"passes": wake_n, "ms": round(wake_ms, 1)}, ms_by_rank=ms_by_rank, k_ms=k_ms, alg=alg, key=key, roof=roof, rep=rep, st=st,
                n_epc_ok=n_epc_ok, n_windows=n_windows, n_rn16=n_rn16, n_epc=n_epc, parity_ok=parity_ok, parity_text=parity_text,
                outputs=outputs)


def other_configs(torch, rfid, synth, args, device, rank):
    """configs[3] (per-GPU stream: one RX stream, 2 000 rounds) and configs[2] (one FIXED_Q=4 trace of 10 000 rounds, 17.6 GB;
    only when >= 40 GB of HBM are free) measured like the headline -- untimed warm-up, a few timed passes, the per-kernel
    series, the workload's result check -- and reported compactly."""
    import copy
    res = {}
    specs = [("configs[3] per GPU", dict(fixed_q=0, n_rounds=2000, n_tags=1, steps=10, warmup=2))]
    free, _ = torch.cuda.mem_get_info(device)
    if free >= 40e9:
        specs.append(("configs[2]", dict(fixed_q=4, n_rounds=10000, n_tags=8, steps=6, warmup=1)))
    else:
        res["configs[2]"] = {"skipped": "%.0f GB of HBM free, 40 needed" % (free / 1e9)}
    for name, sp in specs:
        a = copy.copy(args)
        t0 = time.perf_counter()
        try:
            wl = workload_single_trace(torch, rfid, synth, a, device, rank, sp["fixed_q"], sp["n_rounds"], sp["n_tags"], name)
        except Exception as e:      # (a full device: the headline line must still be printed)
            res[name] = {"skipped": "workload not built: %r" % (e,)}
            continue
        try:
            m = measure(torch, wl, sp["steps"], sp["warmup"], torch.cuda.synchronize, None, n_series=3)
            el = m["elapsed"] / sp["steps"]
            entry = {"workload": wl["describe"], "steps": sp["steps"], "warmup": sp["warmup"],
                     "ms_per_step": round(1e3 * el, 4), "value": round(wl["L"] / el / 1e6, 2), "unit": "Msamples/s",
                     "ms_per_step_each_waited_for": round(1e3 * statistics.fmean(m["step_s"]), 4),
                     "epc_decodes_per_s": round(m["n_epc_ok"] / el, 1), "windows_per_step": m["n_windows"],
                     "parity_check": m["parity_text"], "device_state": m["dev_state"],
                     "roofline_by_kernel": {k: {f: m["roof"](k)[f] for f in ("ms_per_step", "achieved", "frac", "frac_of_achievable",
                                                                             "algorithmic_bytes", "traffic", "traffic_source")}
                                            for k in m["alg"]},
                     "setup_s": round(time.perf_counter() - t0, 2)}
            if m["rep"]["pieces"]:
                entry["long_stream"] = {k: m["rep"][k] for k in ("pieces", "units", "avg_rounds", "dc_rounds", "verified", "gave_up")
                                        if k in m["rep"]}
            if not m["parity_ok"]:
                entry["FAILED"] = True
            # the same workload at SURVEY 8(d)'s stress noise (sigma = 0.03): a light measurement (2 passes each waited for) of what the
            # long-stream front end does there.  With the survey's carrier leak (phase 0.7: 25 sin 0.7 = 16.1) dc_est hovers across a
            # binade edge under this noise and the finishing walk takes most units (long_stream.dc_finished): slower, never wrong
            try:
                a2 = copy.copy(a)
                a2.sigma = 0.03
                wl2 = workload_single_trace(torch, rfid, synth, a2, device, rank, sp["fixed_q"], sp["n_rounds"], sp["n_tags"], name, reuse=wl)
                m2 = measure(torch, wl2, 2, 0, torch.cuda.synchronize, None, n_series=1, back_to_back=False, wake_s=0.0)
                entry["noise"] = {"sigma": 0.03, "ms_per_step_each_waited_for": round(1e3 * statistics.fmean(m2["step_s"]), 4),
                                  "parity_check": m2["parity_text"],
                                  "long_stream": {k: m2["rep"][k] for k in ("avg_rounds", "dc_rounds", "dc_reruns", "dc_finished", "verified", "gave_up") if k in m2["rep"]}}
                if not m2["parity_ok"]:
                    entry["FAILED"] = True
            except Exception as e:
                entry["noise"] = {"skipped": repr(e)}
            res[name] = entry
        finally:
            wl["ctx"].close()
            del wl
            torch.cuda.empty_cache()
    return res


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: re-execute this script once per GPU (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_* as torch.distributed.run would set them), rank 0's stdout -- the one JSON line -- passed
    through.  Returns the worst exit code."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=os.environ.get("MASTER_PORT", str(port)), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--config", default="1", choices=["1", "2", "3stream", "4shard"])
    ap.add_argument("--streams", type=int, default=None, help="traces per GPU (configs 1 / 4shard)")
    ap.add_argument("--rounds", type=int, default=None, help="inventory rounds of the single trace (configs 2 / 3stream)")
    ap.add_argument("--tags", type=int, default=8, help="tags in the field (config 2)")
    ap.add_argument("--hbm-frac", type=float, default=0.90, help="4shard: fraction of the free HBM to fill")
    ap.add_argument("--sigma", type=float, default=0.002)
    ap.add_argument("--leak-phase", type=float, default=None, help="configs 2 / 3stream: phase (rad) of the carrier leak L = e^{j phase} (SURVEY 8(d): 0.7); "
                    "0.7 puts 25 sin(0.7) = 16.1 next to a power of two, where dc_est hovers across the binade edge under noise")
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--wake-ms", type=float, default=None, help="ms of the workload's own passes before the warm-up steps (default: WAKE_S; untimed)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stream-leg", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short configs[2] / configs[3] measurements")
    ap.add_argument("--no-back-to-back", action="store_true", help="time every pass waited for by itself (as rounds 1-3 did) instead of the K passes enqueued one behind the other: the profiled runs use it, a kernel trace then holds no queueing")
    ap.add_argument("--stream-replicas", type=int, default=160, help="replicas concatenated into the host-resident stream")
    ap.add_argument("--stream-chunk", type=int, default=32_000_000, help="raw samples per rfid_stream_work call")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: per-kernel times and roofline, the passes "
                    "each waited for, the device's state, the result check, the streaming leg, configs[2] / configs[3], the CPU "
                    "baseline (the --no-* options above apply to it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed (window table, "
                    "decoded results, per-trace statistics; float32 / float64, at most 64 MB in all) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 10 if args.config in ("1", "3stream") else (6 if args.config == "2" else 3)
    if args.warmup is None:
        args.warmup = 2 if args.config in ("1", "3stream") else 1

    # The ROCm runtime maps a process's streams onto four hardware queues by default; this process holds up to three contexts
    # (the headline's, the streaming leg's, other_configs') with two streams each, and streams that share a queue do not
    # overlap: the long-stream passes of other_configs then lose the next pass's matched filter beside the front end (10.9
    # instead of 10.3 ms per pass, measured).  Eight queues; set before the runtime starts.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))     # plain `python bench.py --gpus N`: start the N ranks ourselves

    import torch
    import rfid
    from rfid import synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the receive path has no CPU fallback")
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # one process per GPU.  (RFID_BENCH_SHARE_DEVICES=1 + RFID_BENCH_BACKEND=gloo: several ranks on the devices at hand -- the
    # multi-rank path on a one-GPU box; RCCL itself refuses two ranks per device.)
    n_dev = torch.cuda.device_count()
    dev_index = local_rank % n_dev if os.environ.get("RFID_BENCH_SHARE_DEVICES") else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist = None
    backend = os.environ.get("RFID_BENCH_BACKEND", "nccl")
    if world > 1 or os.environ.get("RFID_BENCH_FORCE_DIST"):   # (the env var lets a 1-GPU box exercise the RCCL path)
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    ctl_device = device if backend == "nccl" else torch.device("cpu")   # where the control-plane tensors live
    n_gpus = world

    dev_static = device_state_static(torch, device) if rank == 0 and args.full else {}
    if args.config == "1":
        wl = workload_replicas(torch, rfid, synth, args, device, rank, args.streams or 1024, "configs[1]")
    elif args.config == "4shard":
        B = args.streams
        if B is None:
            free, _ = torch.cuda.mem_get_info(device)
            L0 = 1076066
            per_trace = 8 * (L0 + 2) + 8 * (L0 // 5 + 2) + (L0 // 5 // 347 + 2) * PER_WINDOW_WS + 1056 + 1016
            B = max(1, int(free * args.hbm_frac / per_trace))
        wl = workload_replicas(torch, rfid, synth, args, device, rank, B, "configs[4], the per-GPU shard")
    elif args.config == "2":
        wl = workload_single_trace(torch, rfid, synth, args, device, rank, 4, args.rounds or 10000, args.tags, "configs[2]")
    else:
        wl = workload_single_trace(torch, rfid, synth, args, device, rank, 0, args.rounds or 2000, 1,
                                   "configs[3], the per-GPU workload")
    ctx, data, stride, L, B = wl["ctx"], wl["data"], wl["stride"], wl["L"], wl["B"]

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def gather_elapsed(elapsed):
        mine = torch.tensor([elapsed], dtype=torch.float64, device=ctl_device)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        return [float(t.item()) for t in every]

    def collect():
        return timed_path_outputs(ctx, DUMP_BYTES / world)

    m = measure(torch, wl, args.steps, args.warmup, barrier, gather_elapsed if dist is not None else None,
                back_to_back=not args.no_back_to_back, wake_s=None if args.wake_ms is None else args.wake_ms / 1e3,
                full=args.full, collect=collect if args.dump_outputs else None)
    elapsed, step_s = m["elapsed"], m["step_s"]
    n_epc_ok, n_windows = m["n_epc_ok"], m["n_windows"]
    total_raw = float(B) * L * args.steps * n_gpus
    out = {
        "metric": "I/Q Msamples/s through matched_filter->gate->tag_decoder (+ EPC decodes/s), 40 kHz FM0",
        "value": round(total_raw / elapsed / 1e6, 2),
        "unit": "Msamples/s",
        "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "timed_region": ("the K passes enqueued one behind the other, one wait at the end (barrier + device synchronisation on both sides)"
                         if m["b2b_ms"] is not None else "every pass waited for by itself (--no-back-to-back)"),
        "device_wake": dict(m["wake"], note="the same passes run for %.0f ms of wall time before the W warm-up steps (the device's clocks after the host's set-up work); untimed" % m["wake"]["ms"]),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": wl["describe"], "streams_per_gpu": B, "raw_samples_per_stream": L,
                   "hbm_bytes_traces": int(8 * stride * B),
                   "parallelism": "traces sharded per GPU, no collective"},
        "epc_decodes_per_s": round(n_epc_ok * n_gpus * args.steps / elapsed, 1),
        "windows_per_step": n_windows,
        "ms_per_step_by_rank": [round(v, 4) for v in m["ms_by_rank"]],
        "control_plane": ("torch.distributed/%s: barrier + all_gather of the ranks' times%s" % (backend, " and checks" if args.full else ""))
                         if dist is not None else "single process",
        "full": bool(args.full),
    }
    if args.full or m["b2b_ms"] is None:
        out["passes_each_waited_for"] = {
            "ms_per_step": round(statistics.fmean(step_s) * 1e3, 4), "min_ms_per_step": round(min(step_s) * 1e3, 4),
            "median_ms_per_step": round(statistics.median(step_s) * 1e3, 4),
            "note": ("the same K passes, each submitted and waited for by itself (the timed region of rounds 1-3); "
                     "outside the timed region" if m["b2b_ms"] is not None else "this IS the timed region")}
    if B == 1:
        out["single_stream"] = {"raw_msamples_per_s": round(L / (elapsed / args.steps) / 1e6, 2),
                                "x_realtime_at_2Msps": round(L / (elapsed / args.steps) / 2e6, 1)}
    parity_ok, parity_by_rank = True, []
    if args.full:
        k_ms, alg, key, roof, rep = m["k_ms"], m["alg"], m["key"], m["roof"], m["rep"]
        n_rn16, n_epc = m["n_rn16"], m["n_epc"]
        parity_ok, parity_text = m["parity_ok"], m["parity_text"]

        # every rank's check and device, gathered over the control plane: the job fails if ANY rank's results are wrong
        dev_name = torch.cuda.get_device_name(device)
        try:      # (a box without the amdgpu.ids table gives an empty marketing name: the architecture and the CU count say which part it is)
            pr = torch.cuda.get_device_properties(device)
            arch = getattr(pr, "gcnArchName", "") or ""
            dev_name = ("%s %s, %d CUs, %.0f GB" % (dev_name, arch.split(":")[0], pr.multi_processor_count, pr.total_memory / 1e9)).strip()
        except Exception:
            pass
        devices = ["%s (cuda:%d)" % (dev_name, dev_index)]
        parity_by_rank = [parity_text]
        if dist is not None:
            got = [None] * world
            dist.all_gather_object(got, {"device": devices[0], "parity": parity_text, "ok": bool(parity_ok)})
            devices = [g["device"] for g in got]
            parity_by_rank = [g["parity"] for g in got]
            parity_ok = all(g["ok"] for g in got)

        dominant = max(alg, key=lambda k: k_ms[key[k]])
        out.update({
            "decoder_gated_msamples_per_s": round((n_rn16 * RN16_WIN + n_epc * EPC_WIN) / (k_ms["decode_ms"] * 1e-3) / 1e6, 1)
            if k_ms["decode_ms"] > 0 else None,
            "parity_check": parity_text if all(t == parity_text for t in parity_by_rank) else
                            "; ".join("rank %d: %s" % (r, t) for r, t in enumerate(parity_by_rank)),
            "roofline": roof(dominant),
            "roofline_by_kernel": {k: roof(k) for k in alg},
            "front_end_ms": round(k_ms["front_ms"], 4),
            "devices_by_rank": devices,
            "device_state": dict(under_load=m["dev_state"], **dev_static,
                                 note="rank 0's device; under_load = sysfs (pp_dpm_sclk / pp_dpm_mclk starred level, hwmon power and "
                                      "temperatures) sampled every 4 ms by a thread while the SAME K passes ran once more behind all "
                                      "measured series (replay_ms_per_step: that run's own time -- the reads perturb it, which is why they are not "
                                      "inside the timed region); the rest read once before the workload was built"),
        })
        if rep["pieces"]:
            out["long_stream"] = dict(rep, note="traces cut along time into pieces processed at once (avg_ampl, state machine, dc_est) "
                                      "from guessed start values; accepted only when every piece's run is exact or provably covers its "
                                      "true start (verified = 1), i.e. the windows ARE those of the sequential scan; no host "
                                      "synchronisation inside a pass")
        # the legs below belong to the single-GPU line (the contract's cpu_baseline is "on rank 0 at N = 1 only"; with N > 1 the
        # other ranks would sit in the closing barrier while rank 0 works through them)
        solo = n_gpus == 1
        if rank == 0 and solo and args.config == "1" and not args.no_stream_leg:
            out["streaming"] = streaming_leg(torch, rfid, wl, args, device)
        if rank == 0 and solo and args.config == "1" and not args.no_other_configs:
            # the other single-GPU BASELINE configurations, each a short measurement of its own OUTSIDE the headline's timed
            # region (rank 0's GPU only): configs[3]'s per-GPU stream always, configs[2] when the device has room for it
            out["other_configs"] = other_configs(torch, rfid, synth, args, device, rank)
        if rank == 0 and solo and not args.no_cpu_baseline:
            x, what = wl["sample"]()
            out["cpu_baseline"] = cpu_baseline(x, args.cpu_seconds, fixed_q=wl["fixed_q"], what=what)
        elif rank == 0:
            out["cpu_baseline"] = None
    if args.dump_outputs:
        write_outputs(args.dump_outputs, m["outputs"], prefix=("rank%d_" % rank) if world > 1 else "")
    if rank == 0:
        print(json.dumps(out))
    ctx.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if not parity_ok:
        sys.stderr.write("bench.py: result check FAILED: %s\n" % "; ".join("rank %d: %s" % (r, t) for r, t in enumerate(parity_by_rank)))
        raise SystemExit(2)


if __name__ == "__main__":
    main()

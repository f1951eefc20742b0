"""ctypes wrapper of tests/wave_emu/librfid_wave_emu.so -- TEST INFRASTRUCTURE ONLY.

Runs the product's kernel source on the lock-step host emulator so kernel logic can be
checked against the oracle without a GPU.  Never imported by the product package."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
sys.path.insert(0, HERE)
from rfid import _capi as capi  # noqa: E402  (struct dtypes only)
import build as _build  # noqa: E402

_libs = {}
EMU_DEADLOCK = -100   # (emu_driver.cpp: a launch of the call deadlocked or did not end)

SCHEDULES = {"seq": 0, "in-order": 1, "reversed": 2, "random": 3, "late": 4}
# seq: the workgroups of a launch one after the other in index order (the default).  The others keep them all resident at once,
# interleaved: the lowest / highest index that can make progress first, a seeded random pick after every wave-level step, or the
# lower half of each trace's workgroups dispatched only once the others wait or are done (rfid_device_env.h here)


class EmuDeadlock(RuntimeError):
    """Every live workgroup of a launch waited (at a grid meeting, a flag or a barrier) with nothing left to run -- or, under the
    concurrent schedules, a workgroup took more wave-level steps than sweep_limit() allows without finishing (it does not end)."""


def sweep_limit(n: int = 0, fin_wpb: int = 16) -> int:
    """wave-level steps a workgroup may take under the concurrent schedules (n > 0 sets it) -> the limit before"""
    f = lib(fin_wpb).emu_sweep_limit
    f.restype = C.c_long
    return int(f(C.c_long(n)))


def lib(fin_wpb: int = 16):
    """fin_wpb: waves per workgroup of the dc_est finishing walk the emulator is built with (16, or the device's 1)"""
    if fin_wpb not in _libs:
        L = C.CDLL(_build.build(fin_wpb=fin_wpb))
        for name in ("emu_gate_stream", "emu_decode_one", "emu_chain_scan2", "emu_mf_stream", "emu_selftest", "emu_chain_scan",
                     "emu_synth_replicas"):   # (the calls whose result is only a status)
            getattr(L, name).errcheck = lambda rc, fn, args, L=L: _raise_deadlock(L, fn.__name__) if rc == EMU_DEADLOCK else rc
        _libs[fin_wpb] = L
    return _libs[fin_wpb]


def _raise_deadlock(L, what):
    buf = C.create_string_buffer(8192)
    L.emu_last_error(buf, len(buf))
    raise EmuDeadlock("%s: %s" % (what, buf.value.decode(errors="replace")))


def grid_meet_selftest(gx: int, gy: int = 1, leave=False, schedule: str = "in-order", seed: int = 0, fin_wpb: int = 16):
    """gx x gy one-wave workgroups meet twice; leave: the last of each row returns between the meetings (True), or loops for
    ever there ("loop") -> [gy][gx] ones"""
    L = lib(fin_wpb)
    L.emu_schedule(SCHEDULES[schedule], C.c_ulonglong(seed))
    out = np.zeros((gy, gx), dtype=np.int32)
    try:
        rc = L.emu_grid_meet_selftest(gx, gy, 2 if leave == "loop" else (1 if leave else 0), C.c_void_p(out.ctypes.data))
    finally:
        L.emu_schedule(0, C.c_ulonglong(0))
    if rc != 0:
        _raise_deadlock(L, "grid_meet_selftest")
    return out


def batch_process(raw: np.ndarray, lens=None, fixed_q=0, max_num_queries=1000, number_unique_tags=100,
                  want_y=False, gate_chunk=0, unaligned=False):
    """raw: [B][L] complex64.  -> dict(windows, results, scores, stats, y)"""
    raw = np.ascontiguousarray(raw, dtype=np.complex64)
    if raw.ndim == 1:
        raw = raw[None, :]
    B, L = raw.shape
    # 16-byte aligned copy with even stride so the float4 path is exercised
    stride = (L + 1) & ~1
    buf = np.zeros(B * stride + 2, dtype=np.complex64)
    off = (16 - buf.ctypes.data % 16) % 16 // 8
    if unaligned:          # rows 8-byte aligned only: the kernels' float2 load path
        off ^= 1
    view = buf[off:off + B * stride].reshape(B, stride)
    view[:, :L] = raw
    cap = B * (L // 5 // 347 + 2)
    windows = np.zeros(cap, dtype=capi.WINDOW_DTYPE)
    results = np.zeros(cap, dtype=capi.RESULT_DTYPE)
    scores = np.zeros(cap, dtype=capi.SCORES_DTYPE)
    stats = np.zeros(B, dtype=capi.STATS_DTYPE)
    n = C.c_long(0)
    y = np.zeros((B, L // 5), dtype=np.complex64) if want_y else None
    lens_arr = None
    if lens is not None:
        lens_arr = np.ascontiguousarray(lens, dtype=np.int64)
    rc = lib().emu_batch_process(
        C.c_void_p(view.ctypes.data), B, C.c_long(stride), C.c_long(L),
        C.c_void_p(lens_arr.ctypes.data) if lens_arr is not None else None,
        fixed_q, max_num_queries, number_unique_tags,
        C.c_void_p(windows.ctypes.data), C.c_void_p(results.ctypes.data), C.c_void_p(scores.ctypes.data),
        C.c_long(cap), C.byref(n), C.c_void_p(stats.ctypes.data),
        C.c_void_p(y.ctypes.data) if y is not None else None, C.c_long(gate_chunk))
    if rc == EMU_DEADLOCK:
        _raise_deadlock(lib(), "batch_process")
    assert rc == 0
    k = n.value
    return dict(windows=windows[:k], results=results[:k], scores=scores[:k], stats=stats, y=y)


LS2_CTL_FIELDS = (["fail", "ok", "n_pieces", "n_heads"] + [f"avg_count{r}" for r in range(12)] + [f"avg_list{r}" for r in range(12)] + [f"fsm_count{r}" for r in range(12)] +
                  ["avg_reruns", "fsm_reruns", "dc_reruns", "avg_rounds", "fsm_rounds", "dc_rounds", "n_units", "n_windows",
                   "wb_clash", "n_dc_pieces", "dc_open_alloc", "dc_finished"] + [f"dc_count{r}" for r in range(65)])


def ls2_process(raw: np.ndarray, lens=None, fixed_q=0, max_num_queries=1000, number_unique_tags=100, min_piece=512,
                target=131072, state=None, hold_last=False, cuts=None, y_skip=0, chain_slots=64, generous=True, dc_rounds=-1, fsm_lanes=False, dc_two_levels=False, dc_bias=0,
                fused=False, fin_wpb=16, fin_waves=0, schedule="seq", seed=0):
    """batch_process() with the long-stream front end (rfid_ls2.hpp) in place of the sequential gate scan.
    fin_wpb / fin_waves: the emulator build (waves per workgroup of the finishing walk) and the walk's waves per trace (0: as the
    library chooses); schedule / seed: how a launch's workgroups are run (SCHEDULES).  A deadlock raises EmuDeadlock.
    -> dict(windows, results, scores, stats, ctl, ok[, consumed])"""
    lb = lib(fin_wpb)
    raw = np.ascontiguousarray(raw, dtype=np.complex64)
    if raw.ndim == 1:
        raw = raw[None, :]
    B, L = raw.shape
    stride = (L + 1) & ~1
    buf = np.zeros(B * stride + 2, dtype=np.complex64)
    off = (16 - buf.ctypes.data % 16) % 16 // 8
    view = buf[off:off + B * stride].reshape(B, stride)
    view[:, :L] = raw
    cap = B * (L // 5 // 347 + 4)
    windows = np.zeros(cap, dtype=capi.WINDOW_DTYPE)
    results = np.zeros(cap, dtype=capi.RESULT_DTYPE)
    scores = np.zeros(cap, dtype=capi.SCORES_DTYPE)
    stats = np.zeros(B, dtype=capi.STATS_DTYPE)
    n = C.c_long(0)
    lens_arr = None
    if lens is not None:
        lens_arr = np.ascontiguousarray(lens, dtype=np.int64)
    lb.emu_ls2_fsm_lanes_min(0 if fsm_lanes else 1 << 30)
    lb.emu_ls2_dcb_bias(int(dc_bias))   # (ulps added to the first round's centres: what the rounding drift of a long trace does to the ring means)
    lb.emu_ls2_dcb_top_min(0 if dc_two_levels else 64)   # (the dc_est chain's second level, as on traces of more than 4 096 idle-grid slots)
    lb.emu_ls2_chain_slots(int(chain_slots))   # (several workgroups per trace in the chain launches, as on long traces)
    lb.emu_ls2_fin_waves(int(fin_waves))
    lb.emu_schedule(SCHEDULES[schedule], C.c_ulonglong(seed))
    nw = lb.emu_ls2_ctl_words()
    ctl = np.zeros(nw, dtype=np.int32)
    consumed = np.zeros(1, dtype=np.int32)
    pcs = np.full((4096, 8), -1, dtype=np.int32)
    cuts_arr = None if cuts is None else np.ascontiguousarray(cuts, dtype=np.int32)
    try:
        ok = lb.emu_ls2_process(
            C.c_void_p(view.ctypes.data), B, C.c_long(stride), C.c_long(L),
            C.c_void_p(lens_arr.ctypes.data) if lens_arr is not None else None,
            fixed_q, max_num_queries, number_unique_tags,
            C.c_void_p(windows.ctypes.data), C.c_void_p(results.ctypes.data), C.c_void_p(scores.ctypes.data),
            C.c_long(cap), C.byref(n), C.c_void_p(stats.ctypes.data), int(min_piece), int(target),
            C.c_void_p(ctl.ctypes.data), nw,
            C.c_void_p(state.ctypes.data) if state is not None else None, 1 if hold_last else 0, C.c_void_p(consumed.ctypes.data),
            C.c_void_p(pcs.ctypes.data), len(pcs) - 1,
            C.c_void_p(cuts_arr.ctypes.data) if cuts_arr is not None else None, 0 if cuts_arr is None else len(cuts_arr), int(y_skip), 1 if generous else 0, int(dc_rounds),
            1 if fused else 0)
    finally:
        lb.emu_schedule(0, C.c_ulonglong(0))
        lb.emu_ls2_fin_waves(0)
    if ok == EMU_DEADLOCK:
        _raise_deadlock(lb, "ls2_process")
    assert ok >= 0
    k = n.value
    npc = int(np.argmax(pcs[:, 0] < 0)) if (pcs[:, 0] < 0).any() else len(pcs)
    return dict(windows=windows[:k], results=results[:k], scores=scores[:k], stats=stats, ok=int(ok),
                ctl=dict(zip(LS2_CTL_FIELDS, ctl.tolist())), consumed=int(consumed[0]), pieces=pcs[:npc].copy())


class GateStream:
    def __init__(self):
        self.state = np.zeros(lib().emu_gate_state_size(), dtype=np.uint8)

    def work(self, x: np.ndarray, seek_type: int = -1):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        out = np.zeros(max(len(x), 1), dtype=np.complex64)
        c, w, o = C.c_int(0), C.c_int(0), C.c_int(0)
        lib().emu_gate_stream(C.c_void_p(self.state.ctypes.data), C.c_void_p(x.ctypes.data), len(x), seek_type,
                              C.c_void_p(out.ctypes.data), C.byref(c), C.byref(w), C.byref(o))
        return c.value, out[:w.value].copy(), o.value


def decode_one(win: np.ndarray, type_: int):
    win = np.ascontiguousarray(win, dtype=np.complex64)
    res = np.zeros(1, dtype=capi.RESULT_DTYPE)
    sc = np.zeros(1, dtype=capi.SCORES_DTYPE)
    lib().emu_decode_one(C.c_void_p(win.ctypes.data), type_, C.c_void_p(res.ctypes.data), C.c_void_p(sc.ctypes.data))
    return res[0], sc[0]


def chain_scan2(x, ca, cb):
    """-> (sums from carry ca, sums from carry cb, scanned): chain_add_auto2 on one 64-sample step"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    oa = np.zeros(64, dtype=np.float32); ob = np.zeros(64, dtype=np.float32)
    sc = C.c_int(0)
    lib().emu_chain_scan2(C.c_void_p(x.ctypes.data), C.c_float(ca), C.c_float(cb), C.c_void_p(oa.ctypes.data),
                          C.c_void_p(ob.ctypes.data), C.byref(sc))
    return oa, ob, bool(sc.value)


DECODE_ALL, DECODE_EPC3, DECODE_RN16X4 = 0, 1, 2
RES_FILL, SCORE_FILL, SUM_FILL = 0xA5, 0x5A, 0x3C     # the bytes decode_lists() prefills the result tables with


def decode_lists(y: np.ndarray, epc, rn16, which: int = DECODE_ALL, n_wg: int = 1, wmax: int = 0, schedule: str = "seq", seed: int = 0):
    """Caller-given window lists (capi.WINDOW_DTYPE records: start, dc, type; stream 0, seq = the result slot) through
    decode_all_kernel, or decode_epc3_kernel / decode_rn16x4_kernel on their own, on n_wg one-wave workgroups.
    -> dict(results, scores, sum, tickets): [wmax] tables prefilled with RES_FILL / SCORE_FILL / SUM_FILL bytes."""
    y = np.ascontiguousarray(y, dtype=np.complex64)
    epc = np.ascontiguousarray(epc, dtype=capi.WINDOW_DTYPE)
    rn16 = np.ascontiguousarray(rn16, dtype=capi.WINDOW_DTYPE)
    wmax = max(int(wmax), 1)
    results = np.frombuffer(bytearray([RES_FILL]) * (wmax * capi.RESULT_DTYPE.itemsize), dtype=capi.RESULT_DTYPE)
    scores = np.frombuffer(bytearray([SCORE_FILL]) * (wmax * capi.SCORES_DTYPE.itemsize), dtype=capi.SCORES_DTYPE)
    sums = np.frombuffer(bytearray([SUM_FILL]) * (wmax * 4), dtype=np.int32)
    tickets = np.array([0, 12345], dtype=np.int32)
    L = lib()
    L.emu_schedule(SCHEDULES[schedule], C.c_ulonglong(seed))
    try:
        rc = L.emu_decode_lists(C.c_void_p(y.ctypes.data), C.c_long(len(y)),
                                C.c_void_p(epc.ctypes.data) if len(epc) else None, len(epc),
                                C.c_void_p(rn16.ctypes.data) if len(rn16) else None, len(rn16), int(which), int(n_wg), wmax,
                                C.c_void_p(results.ctypes.data), C.c_void_p(scores.ctypes.data), C.c_void_p(sums.ctypes.data),
                                C.c_void_p(tickets.ctypes.data))
    finally:
        L.emu_schedule(0, C.c_ulonglong(0))
    if rc == EMU_DEADLOCK:
        _raise_deadlock(L, "decode_lists")
    assert rc == 0, rc
    return dict(results=results, scores=scores, sum=sums, tickets=tickets)


def mf_stream(staging: np.ndarray, in_off: int, n_out: int, unaligned: bool = False) -> np.ndarray:
    """mf_boxcar25_decim5_kernel in its streaming form: output k sums staging[in_off + 5 k + 0..24] (samples in front of the
    staging buffer count as zeros)."""
    buf = np.zeros(len(staging) + 2, dtype=np.complex64)
    off = (16 - buf.ctypes.data % 16) % 16 // 8
    if unaligned:          # rows 8-byte aligned only: the kernels' float2 load path
        off ^= 1
    st = buf[off:off + len(staging)]
    st[:] = staging
    out = np.zeros(max(n_out, 1), dtype=np.complex64)
    lib().emu_mf_stream(C.c_void_p(st.ctypes.data), len(st), in_off, n_out, C.c_void_p(out.ctypes.data))
    return out[:n_out]


def selftest(x, num, den, carry):
    x, num, den = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, num, den))
    outs = [np.zeros(64, dtype=np.float32) for _ in range(4)]
    lib().emu_selftest(C.c_void_p(x.ctypes.data), C.c_void_p(num.ctypes.data), C.c_void_p(den.ctypes.data),
                       C.c_float(carry), *[C.c_void_p(o.ctypes.data) for o in outs])
    return outs


def gate_fsm_selftest(records):
    """gate_fsm_selftest_kernel on capi.GATE_FSM_IN_DTYPE records -> (wave-uniform form, per-lane form), GATE_FSM_OUT_DTYPE"""
    rec = np.ascontiguousarray(records, dtype=capi.GATE_FSM_IN_DTYPE)
    ow = np.zeros(len(rec), dtype=capi.GATE_FSM_OUT_DTYPE)
    ol = np.zeros(len(rec), dtype=capi.GATE_FSM_OUT_DTYPE)
    rc = lib().emu_gate_fsm_selftest(C.c_void_p(rec.ctypes.data), len(rec), C.c_void_p(ow.ctypes.data), C.c_void_p(ol.ctypes.data))
    if rc == EMU_DEADLOCK:
        _raise_deadlock(lib(), "gate_fsm_selftest")
    assert rc == 0, rc
    return ow, ol


def stats_selftest(results, wcount, waves, from_summaries, max_slot_number, max_num_queries, number_unique_tags, out=None):
    """stream_stats_kernel as rfid_selftest_stats launches it: a [n_streams][wmax] table of capi.RESULT_DTYPE records, `waves`
    wavefronts per trace, from the records or from their one-word summaries.  out: STATS_DTYPE rows the kernel writes into
    (a copy; it may hold rows behind n_streams, which the kernel must leave alone) -> the rows after the launch."""
    res = np.ascontiguousarray(results, dtype=capi.RESULT_DTYPE)
    wc = np.ascontiguousarray(wcount, dtype=np.int32)
    n_streams, wmax = res.shape
    assert len(wc) == n_streams
    st = np.zeros(n_streams, dtype=capi.STATS_DTYPE) if out is None else np.ascontiguousarray(out, dtype=capi.STATS_DTYPE).copy()
    assert len(st) >= n_streams
    rc = lib().emu_stats_selftest(C.c_void_p(res.ctypes.data), C.c_void_p(wc.ctypes.data), n_streams, wmax, int(waves),
                                  1 if from_summaries else 0, int(max_slot_number), int(max_num_queries), int(number_unique_tags),
                                  C.c_void_p(st.ctypes.data))
    if rc == EMU_DEADLOCK:
        _raise_deadlock(lib(), "stats_selftest")
    assert rc != -2, "stream_stats_kernel: a 16-byte load on an address that is no multiple of 16"
    assert rc == 0, rc
    return st


def inventory_selftest(results, wcount, n_windows_used, start, waves, max_tags, slots, reads_cap, reads_len=None, prefill=0):
    """The inventory's and the tracks' kernels as rfid_selftest_inventory launches them: a [n_streams][wmax] table of capi.RESULT_DTYPE
    records with its window counts, cut-offs and window starts, `waves` (1 or 16) wavefronts per trace.  Every output array starts
    from `prefill` in every 32-bit word -> dict(rows, counts, overflow, head, ent_off, packed, base, reads_head, offsets, reads)."""
    res = np.ascontiguousarray(results, dtype=capi.RESULT_DTYPE)
    n_streams, wmax = res.shape
    wc = np.ascontiguousarray(wcount, dtype=np.int32)
    used = np.ascontiguousarray(n_windows_used, dtype=np.int32)
    st = np.ascontiguousarray(start, dtype=np.int32)
    assert len(wc) == n_streams and len(used) == n_streams and st.shape == (n_streams, wmax)
    reads_len = int(reads_cap if reads_len is None else reads_len)
    assert reads_len >= reads_cap and reads_len >= 1
    out = capi.inventory_selftest_outputs(n_streams, int(max_tags), reads_len, prefill)
    rc = lib().emu_inventory_selftest(C.c_void_p(res.ctypes.data), C.c_void_p(wc.ctypes.data), C.c_void_p(used.ctypes.data),
                                      C.c_void_p(st.ctypes.data), n_streams, wmax, int(waves), int(max_tags), int(slots), C.c_long(reads_cap),
                                      *[C.c_void_p(out[k].ctypes.data) for k in capi.INVENTORY_SELFTEST_OUTPUTS])
    if rc == EMU_DEADLOCK:
        _raise_deadlock(lib(), "inventory_selftest")
    assert rc != -2, "a 16-byte load of the inventory or the tracks kernel on an address that is no multiple of 16"
    assert rc == 0, rc
    return out


def chain_scan(x, carry):
    """-> (chain, scan, clean): the exact 63-deep chain, chain_add_scan (or its fallback), and whether the scan applied."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    chain = np.zeros(64, dtype=np.float32)
    scan = np.zeros(65, dtype=np.float32)
    lib().emu_chain_scan(C.c_void_p(x.ctypes.data), C.c_float(carry), C.c_void_p(chain.ctypes.data), C.c_void_p(scan.ctypes.data))
    return chain, scan[:64], bool(scan[64])


def synth_replicas(base: np.ndarray, n_streams: int, sigma: float, seed: int, first_replica: int = 0) -> np.ndarray:
    base = np.ascontiguousarray(base, dtype=np.complex64)
    out = np.zeros((n_streams, len(base)), dtype=np.complex64)
    lib().emu_synth_replicas(C.c_void_p(base.ctypes.data), C.c_long(len(base)), C.c_void_p(out.ctypes.data),
                             C.c_long(len(base)), n_streams, C.c_float(sigma), C.c_ulonglong(seed), C.c_long(first_replica))
    return out


def synth_gen2(plan, sigma: float = 0.0, seed: int = 0, replica: int = 0) -> np.ndarray:
    """synth_gen2_kernel on the emulator: the trace of an rfid.synth.TracePlan."""
    p = capi.SynthGen2Params()
    lk = np.complex64(plan.leak)
    p.leak_re, p.leak_im = float(lk.real), float(lk.imag)
    for k, h in enumerate(plan.hs):
        hk = np.complex64(h)
        p.h_re[k], p.h_im[k] = float(hk.real), float(hk.imag)
    p.n_tags, p.tail_us = len(plan.hs), int(plan.tail_us)
    slots = np.ascontiguousarray(plan.slots)
    buf = np.zeros(plan.n_raw + 2, dtype=np.complex64)
    off = (16 - buf.ctypes.data % 16) % 16 // 8
    out = buf[off:off + plan.n_raw]
    fn = lib().emu_synth_gen2
    fn.restype = C.c_long
    n = fn(C.byref(p), C.c_void_p(slots.ctypes.data), C.c_long(len(slots)), C.c_void_p(out.ctypes.data),
           C.c_long(plan.n_raw), C.c_float(sigma), C.c_ulonglong(seed), C.c_long(replica))
    if n == EMU_DEADLOCK:
        _raise_deadlock(lib(), "synth_gen2")
    assert n == plan.n_raw, (n, plan.n_raw)
    return out.copy()


def philox4x32_10(ctr, key) -> np.ndarray:
    c = np.asarray(ctr, dtype=np.uint32); k = np.asarray(key, dtype=np.uint32); o = np.zeros(4, dtype=np.uint32)
    lib().emu_philox4x32_10(C.c_void_p(c.ctypes.data), C.c_void_p(k.ctypes.data), C.c_void_p(o.ctypes.data))
    return o

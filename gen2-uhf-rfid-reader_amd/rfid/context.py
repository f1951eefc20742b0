"""rfid.Context -- one RX stream / one batch workspace on one MI355X.

Thin object wrapper over the C-ABI (include/rfid_mi355x.h).  All sample arithmetic runs in
the HIP kernels behind it.  Device buffers are passed as raw pointers; torch (or any other
allocator) is only used by callers to own HBM.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _capi as capi


def _c64(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.complex64)
    return a


class Context:
    def __init__(self, device: int = 0, **params):
        self._lib = capi.load()
        self.params = capi.default_params(**params)
        h = C.c_void_p()
        capi.check(self._lib.rfid_ctx_create(C.byref(self.params), int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._planned: Optional[Tuple[int, int]] = None
        self._active = 0

    # -- lifetime ------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.rfid_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, status: int) -> None:
        capi.check(status, self._h)

    def reset(self) -> None:
        self._chk(self._lib.rfid_ctx_reset(self._h))

    def selftest(self) -> int:
        n = C.c_int(0)
        self._chk(self._lib.rfid_selftest(self._h, C.byref(n)))
        return n.value

    def selftest_gate_fsm(self, records) -> Tuple[np.ndarray, np.ndarray]:
        """rfid_selftest_gate_fsm: one step of the gate's state machine per GATE_FSM_IN_DTYPE record
        -> (wave-uniform form, per-lane form), GATE_FSM_OUT_DTYPE records.  A test entry: nothing is judged here."""
        rec = np.ascontiguousarray(records, dtype=capi.GATE_FSM_IN_DTYPE)
        ow = np.zeros(len(rec), dtype=capi.GATE_FSM_OUT_DTYPE)
        ol = np.zeros(len(rec), dtype=capi.GATE_FSM_OUT_DTYPE)
        if len(rec):
            self._chk(self._lib.rfid_selftest_gate_fsm(self._h, rec.ctypes.data, len(rec), ow.ctypes.data, ol.ctypes.data))
        return ow, ol

    def selftest_arith(self, records, prefill: int = 0) -> np.ndarray:
        """rfid_selftest_arith: every arithmetic primitive on each ARITH_IN_DTYPE record (one wave's operands) -> len(records) + 1
        ARITH_OUT_DTYPE records whose every byte started as `prefill` (0 .. 255); the last one is the guard behind the records
        written.  A test entry: nothing is judged here."""
        rec = np.ascontiguousarray(records, dtype=capi.ARITH_IN_DTYPE)
        out = np.full((len(rec) + 1) * capi.ARITH_OUT_DTYPE.itemsize, prefill, dtype=np.uint8).view(capi.ARITH_OUT_DTYPE)
        if len(rec):
            self._chk(self._lib.rfid_selftest_arith(self._h, rec.ctypes.data, len(rec), out.ctypes.data))
        return out

    def selftest_stats(self, results, wcount, waves: int, from_summaries: bool, max_slot_number: int, max_num_queries: int,
                       number_unique_tags: int, out=None) -> np.ndarray:
        """rfid_selftest_stats: the statistics kernel by itself on a [n_streams][wmax] table of RESULT_DTYPE records, `waves`
        wavefronts per trace, from the records or from their one-word summaries.  out: STATS_DTYPE rows the device copy starts
        from (default zeros; rows behind n_streams are not passed) -> the rows after the launch.  A test entry: nothing is
        judged here."""
        res = np.ascontiguousarray(results, dtype=capi.RESULT_DTYPE)
        wc = np.ascontiguousarray(wcount, dtype=np.int32)
        n_streams, wmax = res.shape
        assert len(wc) == n_streams
        st = np.zeros(n_streams, dtype=capi.STATS_DTYPE) if out is None else np.ascontiguousarray(out, dtype=capi.STATS_DTYPE).copy()
        assert len(st) >= n_streams
        self._chk(self._lib.rfid_selftest_stats(self._h, res.ctypes.data, wc.ctypes.data, n_streams, wmax, int(waves),
                                                1 if from_summaries else 0, int(max_slot_number), int(max_num_queries),
                                                int(number_unique_tags), st.ctypes.data))
        return st

    def selftest_inventory(self, results, wcount, n_windows_used, start, waves: int, max_tags: int, slots: int, reads_cap: int,
                           reads_len: Optional[int] = None, prefill: int = 0) -> dict:
        """rfid_selftest_inventory: the inventory's and the tracks' kernels by themselves, in the batch calls' launch sequence, on a
        [n_streams][wmax] table of RESULT_DTYPE records with its window counts, cut-offs and window starts; `waves` (1 or 16)
        wavefronts per trace.  Every output array starts from `prefill` in every 32-bit word -> dict(rows, counts, overflow, head,
        ent_off, packed, base, reads_head, offsets, reads) as the launches left them.  A test entry: nothing is judged here."""
        res = np.ascontiguousarray(results, dtype=capi.RESULT_DTYPE)
        n_streams, wmax = res.shape
        wc = np.ascontiguousarray(wcount, dtype=np.int32)
        used = np.ascontiguousarray(n_windows_used, dtype=np.int32)
        st = np.ascontiguousarray(start, dtype=np.int32)
        assert len(wc) == n_streams and len(used) == n_streams and st.shape == (n_streams, wmax)
        out = capi.inventory_selftest_outputs(n_streams, int(max_tags), int(reads_cap if reads_len is None else reads_len), prefill)
        self._chk(self._lib.rfid_selftest_inventory(self._h, res.ctypes.data, wc.ctypes.data, used.ctypes.data, st.ctypes.data, n_streams,
                                                    wmax, int(waves), int(max_tags), int(slots), int(reads_cap),
                                                    int(reads_cap if reads_len is None else reads_len),
                                                    *[out[k].ctypes.data for k in capi.INVENTORY_SELFTEST_OUTPUTS]))
        return out

    @property
    def stream_handle(self) -> int:
        return int(self._lib.rfid_ctx_stream(self._h) or 0)

    # -- READER_STATE ----------------------------------------------------------------------
    def state(self) -> capi.ReaderState:
        st = capi.ReaderState()
        self._chk(self._lib.rfid_get_state(self._h, C.byref(st)))
        return st

    def stats(self) -> dict:
        s = self.state()
        return dict(n_queries_sent=s.n_queries_sent, cur_inventory_round=s.cur_inventory_round,
                    cur_slot_number=s.cur_slot_number, n_epc_correct=s.n_epc_correct,
                    n_unique_tags=s.n_unique_tags, status=s.status,
                    tag_reads={i: s.tag_reads[i] for i in range(256) if s.tag_reads[i]})

    def print_results(self) -> str:
        buf = C.create_string_buffer(1 << 15)
        n = C.c_int(0)
        self._chk(self._lib.rfid_print_results(self._h, buf, len(buf), C.byref(n)))
        return buf.raw[: n.value].decode()

    # -- (1) streaming, host buffers ---------------------------------------------------------
    def mf_work(self, x, out_cap: Optional[int] = None) -> np.ndarray:
        """rfid_mf_work.  With late outputs (lookahead_set_late_outputs) the call returns what the call before it made;
        out_cap: the room the caller's output buffer has (default: this call's outputs, or everything held back)."""
        x = _c64(x)
        if out_cap is None:
            out_cap = max(len(x) // 5 + 2, self.mf_pending())
        out = np.empty(max(int(out_cap), 1), dtype=np.complex64)
        n = C.c_int(0)
        self._chk(self._lib.rfid_mf_work(self._h, x.ctypes.data if len(x) else None, len(x), out.ctypes.data, int(out_cap), C.byref(n)))
        return out[: n.value].copy()

    def lookahead_set_late_outputs(self, on: bool = True) -> None:
        """mf_work returns the filter outputs of the call before it (no call waits for the device); mf_work(empty) fetches
        what is held back at the end of the input."""
        self._chk(self._lib.rfid_lookahead_set_late_outputs(self._h, 1 if on else 0))

    def mf_pending(self) -> int:
        n = C.c_int(0)
        self._chk(self._lib.rfid_mf_pending(self._h, C.byref(n)))
        return n.value

    def gate_work(self, x, out_cap: Optional[int] = None) -> Tuple[int, np.ndarray]:
        """-> (consumed, gated samples), as gate_impl::general_work's consume_each()/output.  out_cap: the room of the caller's
        output buffer (default: as many items as the call is shown; a consume-ahead gate may be called without input)."""
        x = _c64(x)
        if out_cap is None:
            out_cap = max(len(x), 1)
        out = np.empty(max(int(out_cap), 1), dtype=np.complex64)
        cons, wr = C.c_int(0), C.c_int(0)
        self._chk(self._lib.rfid_gate_work(self._h, x.ctypes.data if len(x) else None, len(x), out.ctypes.data, int(out_cap),
                                           C.byref(cons), C.byref(wr)))
        return cons.value, out[: wr.value].copy()

    def lookahead_set_consume_ahead(self, on: bool = True) -> None:
        """gate_work consumes everything it is shown; the windows follow when the passes have found them (gate_forecast says
        when a call without input has something to hand out; lookahead_flush at the end of the input)."""
        self._chk(self._lib.rfid_lookahead_set_consume_ahead(self._h, 1 if on else 0))

    def gate_forecast(self, upstream_done: bool = False) -> bool:
        """-> True when the gate needs input to do anything (the reference's forecast), False when a call without input can."""
        n = C.c_int(1)
        self._chk(self._lib.rfid_gate_forecast(self._h, 1 if upstream_done else 0, C.byref(n)))
        return n.value != 0

    def decoder_work(self, x):
        """-> (consumed, port-0 floats, result record or None, scores record or None)."""
        x = _c64(x)
        bits = np.zeros(16, dtype=np.float32)
        cons, prod = C.c_int(0), C.c_int(0)
        res = np.zeros(1, dtype=capi.RESULT_DTYPE)
        sc = np.zeros(1, dtype=capi.SCORES_DTYPE)
        self._chk(self._lib.rfid_decoder_work(self._h, x.ctypes.data, len(x), bits.ctypes.data, len(bits),
                                              C.byref(cons), C.byref(prod), res.ctypes.data, sc.ctypes.data))
        if cons.value == 0:
            return 0, bits[:0], None, None
        return cons.value, bits[: prod.value].copy(), res[0], sc[0]

    def reader_work(self, n_in: int) -> int:
        cons = C.c_int(0)
        self._chk(self._lib.rfid_reader_work(self._h, int(n_in), C.byref(cons)))
        return cons.value

    def reader_work_tx(self, in_bits=None, dac_rate: int = 1000000):
        """reader_impl::general_work incl. the TX waveform -> (consumed, float32 samples written)."""
        bits = np.ascontiguousarray(in_bits if in_bits is not None else [], dtype=np.float32)
        out = np.zeros(self._lib.rfid_reader_tx_max(int(dac_rate)), dtype=np.float32)
        cons, wr = C.c_int(0), C.c_int(0)
        self._chk(self._lib.rfid_reader_work_tx(self._h, int(dac_rate), bits.ctypes.data if len(bits) else None, len(bits),
                                                out.ctypes.data, len(out), C.byref(cons), C.byref(wr)))
        return cons.value, out[: wr.value].copy()

    # -- (1b) whole-chain streaming ------------------------------------------------------------------
    def lookahead_enable(self, max_chunk_raw: int) -> None:
        """The per-block calls (mf_work / gate_work / decoder_work) answered from one whole-chain pass per mf_work call."""
        self._chk(self._lib.rfid_lookahead_enable(self._h, int(max_chunk_raw)))
        self._planned = (1, int(max_chunk_raw))   # (the look-ahead runs on a one-trace plan of its own: any batch plan is gone)
        self._active = 1

    def lookahead_enable_gate(self, max_items: int) -> None:
        """The same keyed on the gate's input (a flowgraph whose matched filter is not this library's): gate_work uploads
        what is new in its input and runs gate -> tag_decoder over it in one submission."""
        self._chk(self._lib.rfid_lookahead_enable_gate(self._h, int(max_items)))
        self._planned = (1, 5 * int(max_items))   # (the look-ahead runs on a one-trace plan of its own: any batch plan is gone)
        self._active = 1

    def lookahead_pending(self):
        """-> (windows found and not yet handed out by gate_work, windows handed out and waiting for decoder_work)."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self._lib.rfid_lookahead_pending(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def lookahead_flush(self) -> None:
        """End of the input: what the look-ahead still holds back is decided now (the gate / decoder calls hand it out)."""
        self._chk(self._lib.rfid_lookahead_flush(self._h))

    def stream_begin(self, max_chunk_raw: int) -> None:
        self._chk(self._lib.rfid_stream_begin(self._h, int(max_chunk_raw)))
        self._stream_cap = 4096
        self._planned = (1, int(max_chunk_raw))   # (the stream runs on a one-trace plan of its own)
        self._active = 1

    def stream_staging(self, idx: int) -> np.ndarray:
        """One of the two pinned staging buffers as a complex64 array (fill it, then pass a slice that starts at
        element 0 to stream_work: the upload is then a true asynchronous DMA)."""
        p, cap = C.c_void_p(), C.c_int64(0)
        self._chk(self._lib.rfid_stream_staging(self._h, int(idx), C.byref(p), C.byref(cap)))
        buf = (C.c_float * (2 * cap.value)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.complex64)

    def stream_work(self, raw=None, flush: bool = False):
        """-> (windows, results) completed by this call (rfid_stream_work)."""
        if raw is None:
            raw = np.zeros(0, dtype=np.complex64)
        raw = np.ascontiguousarray(raw, dtype=np.complex64)
        n = C.c_int64(0)
        ptr = raw.ctypes.data if len(raw) else None
        n_in = len(raw)
        while True:
            w = np.zeros(self._stream_cap, dtype=capi.STREAM_WINDOW_DTYPE)
            r = np.zeros(self._stream_cap, dtype=capi.RESULT_DTYPE)
            st = self._lib.rfid_stream_work(self._h, ptr, n_in, int(bool(flush)), w.ctypes.data, r.ctypes.data,
                                            self._stream_cap, C.byref(n))
            if st == capi.ERR_CAPACITY and n.value > self._stream_cap:   # arrays too small: nothing lost, ask again
                self._stream_cap = int(n.value) * 2
                ptr, n_in = None, 0
                continue
            self._chk(st)
            return w[: n.value].copy(), r[: n.value].copy()

    def stream_end(self) -> None:
        self._chk(self._lib.rfid_stream_end(self._h))

    # -- (2) batched offline, device buffers ---------------------------------------------------
    def batch_plan(self, n_streams: int, max_raw: int) -> None:
        self._chk(self._lib.rfid_batch_plan(self._h, int(n_streams), int(max_raw)))
        self._planned = (int(n_streams), int(max_raw))
        self._active = int(n_streams)

    def batch_set_streams(self, n_streams: int) -> None:
        """Process only the first n_streams (<= planned) rows in the following passes."""
        self._chk(self._lib.rfid_batch_set_streams(self._h, int(n_streams)))
        self._active = int(n_streams)

    def batch_process_ptr(self, d_raw: int, raw_stride: int, n_raw: int, d_lens: int = 0,
                          want_scores: bool = False) -> None:
        """Asynchronous mf->gate->decode->stats over [n_streams][raw_stride] complex64 in HBM."""
        self._chk(self._lib.rfid_batch_process(self._h, C.c_void_p(d_raw), int(raw_stride), int(n_raw),
                                               C.c_void_p(d_lens) if d_lens else None, int(bool(want_scores))))

    def batch_stage(self, which: str, *args) -> None:
        fn = {"mf": self._lib.rfid_batch_mf, "gate": self._lib.rfid_batch_gate,
              "decode": self._lib.rfid_batch_decode, "stats": self._lib.rfid_batch_stats}[which]
        if which == "mf":
            d_raw, raw_stride, n_raw, d_lens = args
            self._chk(fn(self._h, C.c_void_p(d_raw), int(raw_stride), int(n_raw),
                         C.c_void_p(d_lens) if d_lens else None))
        elif which == "decode":
            self._chk(fn(self._h, int(bool(args[0])) if args else 0))
        else:
            self._chk(fn(self._h))

    def batch_set_long_stream(self, mode: int) -> None:
        """0: never cut traces along time, 1: automatic (few long traces), 2: whenever possible."""
        self._chk(self._lib.rfid_batch_set_long_stream(self._h, int(mode)))

    def set_knob(self, name: str, value: int) -> None:
        """One of the switches the environment sets at context creation, by its lower-case name
        without the RFID_ prefix: ctx.set_knob("overlap", 0)."""
        self._chk(self._lib.rfid_ctx_set_knob(self._h, name.encode(), int(value)))

    def get_knob(self, name: str) -> int:
        v = C.c_int(0)
        self._chk(self._lib.rfid_ctx_get_knob(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def batch_ls_report(self) -> dict:
        r = capi.LsReport()
        self._chk(self._lib.rfid_batch_ls_report(self._h, C.byref(r)))
        return {n: int(getattr(r, n)) for n, _ in capi.LsReport._fields_}

    def batch_sync(self) -> None:
        self._chk(self._lib.rfid_batch_sync(self._h))

    def batch_timing(self) -> dict:
        t = capi.BatchTiming()
        self._chk(self._lib.rfid_batch_timing_get(self._h, C.byref(t)))
        return dict(mf_ms=t.mf_ms, gate_ms=t.gate_ms, decode_ms=t.decode_ms, stats_ms=t.stats_ms,
                    total_ms=t.total_ms, front_ms=t.front_ms, front_chunks=t.front_chunks,
                    decode_launches=t.decode_launches, fused_front=t.fused_front)

    def batch_stats(self) -> np.ndarray:
        n = self._active
        out = np.zeros(n, dtype=capi.STATS_DTYPE)
        self._chk(self._lib.rfid_batch_get_stats(self._h, out.ctypes.data, n))
        return out

    def batch_windows(self, want_scores: bool = False):
        """-> (windows, results, scores|None) ordered by (stream, seq)."""
        n = C.c_int64(0)
        self._chk(self._lib.rfid_batch_get_windows(self._h, None, None, None, 0, C.byref(n)))
        k = n.value
        w = np.zeros(k, dtype=capi.WINDOW_DTYPE)
        r = np.zeros(k, dtype=capi.RESULT_DTYPE)
        s = np.zeros(k, dtype=capi.SCORES_DTYPE) if want_scores else None
        if k:
            self._chk(self._lib.rfid_batch_get_windows(self._h, w.ctypes.data, r.ctypes.data,
                                                       s.ctypes.data if s is not None else None, k, C.byref(n)))
        return w, r, s

    def _sized_fetch(self, get, dtype, head=(), tail=(), extra: int = 0) -> np.ndarray:
        """The two calls every stage's fetch makes: `get` without an array tells the size (RFID_ERR_CAPACITY where there is
        something to fetch), then an array of that size plus `extra` records is filled.  head / tail: get's arguments before
        and behind (array, cap, n)."""
        n = C.c_int64(0)
        out = np.zeros(0, dtype=dtype)
        st = get(self._h, *head, None, 0, C.byref(n), *tail)
        if st in (capi.OK, capi.ERR_CAPACITY) and n.value + extra > 0:   # (the size is known now; a trace that overflowed fails again below)
            out = np.zeros(n.value + extra, dtype=dtype)
            st = get(self._h, *head, out.ctypes.data, len(out), C.byref(n), *tail)
        self._chk(st)
        return out

    def _stage_ms(self, get_ms) -> float:
        ms = C.c_float(0.0)
        self._chk(get_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def _window_rows(self, get, dtype, stream: int, extra: int) -> np.ndarray:
        """One trace's rows of a window-table stage (rfid_batch_get_window_*): those before the cut-off plus up to `extra`
        of the zeroed ones behind them."""
        return self._sized_fetch(get, dtype, head=(int(stream),), extra=max(int(extra), 0))

    def _one_window(self, call, dtype, gated, result) -> np.ndarray:
        """The per-call form of an EPC-window stage (rfid_repair_window, rfid_fine_window): one window's gated samples and
        its result record in, one record of `dtype` out."""
        gated = np.ascontiguousarray(gated, dtype=np.complex64)
        if len(gated) != 1370:
            raise ValueError("an EPC window has 1370 samples")
        res = np.zeros(1, dtype=capi.RESULT_DTYPE)
        res[0] = result
        out = np.zeros(1, dtype=dtype)
        self._chk(call(self._h, gated.ctypes.data, res.ctypes.data, out.ctypes.data))
        return out[0]

    def batch_plan_inventory(self, max_tags: int) -> None:
        """Reserves the inventory workspace of the current plan: up to max_tags distinct EPC frames per trace."""
        self._chk(self._lib.rfid_batch_plan_inventory(self._h, int(max_tags)))

    def batch_inventory_enqueue(self) -> None:
        """Asynchronous: the inventory of the last pass, behind its statistics (rfid_batch_inventory)."""
        self._chk(self._lib.rfid_batch_inventory(self._h))

    def batch_inventory_fetch(self):
        """-> (entries, per-trace counts) of the last batch_inventory_enqueue (synchronises)."""
        counts = np.zeros(max(self._active, 1), dtype=np.int32)
        ent = self._sized_fetch(self._lib.rfid_batch_get_inventory, capi.TAG_ENTRY_DTYPE, tail=(counts.ctypes.data,))
        return ent, counts[: self._active]

    def batch_inventory(self):
        """The distinct EPC frames of every trace of the last pass, built on the device: -> (structured array of
        capi.TAG_ENTRY_DTYPE ordered by (stream, first_seq), entries per trace)."""
        self.batch_inventory_enqueue()
        return self.batch_inventory_fetch()

    def batch_inventory_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_inventory_ms)

    def batch_plan_tracks(self) -> None:
        """Reserves the tracks workspace of the current plan (behind batch_plan_inventory; a new plan or a new
        batch_plan_inventory drops it)."""
        self._chk(self._lib.rfid_batch_plan_tracks(self._h))

    def batch_tracks_enqueue(self) -> None:
        """Asynchronous: the tracks of the last pass, behind its inventory (rfid_batch_tracks)."""
        self._chk(self._lib.rfid_batch_tracks(self._h))

    def batch_tracks_fetch(self):
        """-> (reads, offsets) of the last batch_tracks_enqueue (synchronises): capi.TAG_READ_DTYPE ordered by
        (stream, entry, seq); int64 offsets aligned with the entries of batch_inventory_fetch -- reads
        offsets[i]:offsets[i + 1] are entry i's."""
        ne = C.c_int64(0)      # the entries the offsets are aligned with
        si = self._lib.rfid_batch_get_inventory(self._h, None, 0, C.byref(ne), None)
        if si not in (capi.OK, capi.ERR_CAPACITY, capi.ERR_STATE):     # (no inventory: no tracks either, said below)
            self._chk(si)
        offsets = np.zeros(ne.value + 1, dtype=np.int64)
        reads = self._sized_fetch(self._lib.rfid_batch_get_tracks, capi.TAG_READ_DTYPE, tail=(offsets.ctypes.data,))
        return reads, offsets

    def batch_tracks(self):
        """Every tag's reads of the last pass in time order, built on the device behind batch_inventory():
        -> (reads, offsets), see batch_tracks_fetch."""
        self.batch_tracks_enqueue()
        return self.batch_tracks_fetch()

    def batch_tracks_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_tracks_ms)

    def batch_plan_quality(self) -> None:
        """Reserves the quality workspace of the current plan (behind batch_plan_tracks; a new plan, batch_plan_inventory or
        batch_plan_tracks drops it)."""
        self._chk(self._lib.rfid_batch_plan_quality(self._h))

    def batch_quality_enqueue(self) -> None:
        """Asynchronous: the read quality of the last pass, behind its tracks (rfid_batch_quality)."""
        self._chk(self._lib.rfid_batch_quality(self._h))

    def batch_quality_fetch(self) -> np.ndarray:
        """-> capi.QUALITY_DTYPE records of the last batch_quality_enqueue (synchronises), one per CRC-verified read:
        record i belongs to reads[i] of batch_tracks_fetch."""
        return self._sized_fetch(self._lib.rfid_batch_get_quality, capi.QUALITY_DTYPE)

    def batch_quality(self) -> np.ndarray:
        """SNR and decision margin of every read of the last pass, built on the device behind batch_tracks():
        see batch_quality_fetch; rfid.batch.quality_fields turns the records into snr_db and margin."""
        self.batch_quality_enqueue()
        return self.batch_quality_fetch()

    def batch_window_quality(self, stream: int, extra: int = 0) -> np.ndarray:
        """Debug tap (synchronises): the records of EVERY EPC window of one trace before the cut-off, in seq order, failed
        ones included (n_windows_used // 2 of them), of the last batch_quality_enqueue.  extra > 0: up to that many of the
        table's rows behind them as well (zeroed by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_quality, capi.QUALITY_DTYPE, stream, extra)

    def batch_quality_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_quality_ms)

    def batch_plan_repair(self) -> None:
        """Reserves the repair workspace of the current plan (behind batch_plan_inventory; a new plan or a new
        batch_plan_inventory drops it, batch_plan_tracks / batch_plan_quality do not)."""
        self._chk(self._lib.rfid_batch_plan_repair(self._h))

    def batch_repair_enqueue(self) -> None:
        """Asynchronous: the repair of the last pass, behind its inventory (rfid_batch_repair)."""
        self._chk(self._lib.rfid_batch_repair(self._h))

    def batch_repair_fetch(self) -> np.ndarray:
        """-> capi.REPAIR_DTYPE records of the last batch_repair_enqueue (synchronises): the repaired windows only
        (n_flips > 0), ordered by (stream, seq)."""
        return self._sized_fetch(self._lib.rfid_batch_get_repairs, capi.REPAIR_DTYPE)

    def batch_repair(self) -> np.ndarray:
        """The CRC-failed EPC windows of the last pass that reversing one to three of their eight weakest decisions makes
        pass, built on the device behind batch_inventory(): see batch_repair_fetch.  A repair is not a read: `entry` says
        whether the trace's inventory holds the repaired frame."""
        self.batch_repair_enqueue()
        return self.batch_repair_fetch()

    def batch_window_repairs(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the repair table (synchronises): the record of EVERY EPC window before the cut-off, in seq
        order (n_windows_used // 2 of them), of the last batch_repair_enqueue.  extra > 0: up to that many of the table's
        rows behind them as well (zeroed by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_repairs, capi.REPAIR_DTYPE, stream, extra)

    def batch_repair_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_repair_ms)

    def repair_window(self, gated, result) -> np.ndarray:
        """The repair search for ONE EPC window in host memory (rfid_repair_window): gated = its 1370 gated, DC-free
        samples, result = its capi.RESULT_DTYPE record (what decoder_work returned).  -> one capi.REPAIR_DTYPE record."""
        return self._one_window(self._lib.rfid_repair_window, capi.REPAIR_DTYPE, gated, result)

    def batch_plan_slots(self) -> None:
        """Reserves the slots workspace of the current plan (a new plan drops it; it needs none of the other workspaces)."""
        self._chk(self._lib.rfid_batch_plan_slots(self._h))

    def batch_slots_enqueue(self) -> None:
        """Asynchronous: the second-order moments of every window of the last pass, behind its statistics
        (rfid_batch_slots)."""
        self._chk(self._lib.rfid_batch_slots(self._h))

    def batch_window_moments(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the moments table (synchronises): the capi.MOMENTS_DTYPE record of EVERY window before the
        cut-off, RN16 and EPC alike, in seq order (n_windows_used of them), of the last batch_slots_enqueue.  extra > 0: up
        to that many of the table's rows behind them as well (zeroed by the stage).  rfid.batch.classify_slots turns a row
        into one record per slot."""
        return self._window_rows(self._lib.rfid_batch_get_window_moments, capi.MOMENTS_DTYPE, stream, extra)

    def batch_slots_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_slots_ms)

    def window_moments(self, gated) -> np.ndarray:
        """The same sums for windows in host memory (rfid_window_moments_of): gated = [n_windows][240] gated, DC-free samples
        (the first 240 of each window the gate handed out).  -> capi.MOMENTS_DTYPE records, stream = 0, seq = the window's
        position, flags = 0."""
        gated = np.ascontiguousarray(gated, dtype=np.complex64)
        if gated.ndim == 1:
            gated = gated.reshape(-1, capi.MOMENTS_SAMPLES) if len(gated) else gated.reshape(0, capi.MOMENTS_SAMPLES)
        if gated.ndim != 2 or gated.shape[1] != capi.MOMENTS_SAMPLES:
            raise ValueError("the moments of a window are taken over 240 samples")
        out = np.zeros(len(gated), dtype=capi.MOMENTS_DTYPE)
        self._chk(self._lib.rfid_window_moments_of(self._h, gated.ctypes.data, len(gated), out.ctypes.data))
        return out

    def batch_plan_commands(self) -> None:
        """Reserves the commands workspace of the current plan (a new plan drops it; it needs none of the other workspaces)."""
        self._chk(self._lib.rfid_batch_plan_commands(self._h))

    def batch_commands_enqueue(self) -> None:
        """Asynchronous: the reader's PIE command in front of every window of the last pass, behind its statistics
        (rfid_batch_commands)."""
        self._chk(self._lib.rfid_batch_commands(self._h))

    def batch_window_commands(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the commands table (synchronises): the capi.COMMAND_DTYPE record of EVERY window before the
        cut-off, RN16 and EPC alike, in seq order (n_windows_used of them), of the last batch_commands_enqueue.  extra > 0: up
        to that many of the table's rows behind them as well (zeroed by the stage).  rfid.batch.command_fields turns a row
        into names, Q, RN16 and timings."""
        return self._window_rows(self._lib.rfid_batch_get_window_commands, capi.COMMAND_DTYPE, stream, extra)

    def batch_commands_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_commands_ms)

    def commands_of(self, spans, levels) -> np.ndarray:
        """The same decode for spans in host memory (rfid_commands_of): spans = [n][704] samples of the matched filter's
        output in front of a window each, levels = [n] the dc of each window.  -> capi.COMMAND_DTYPE records, stream = 0,
        seq = the span's position, flag bits 0, 2 and 4 clear."""
        spans = np.ascontiguousarray(spans, dtype=np.complex64)
        levels = np.ascontiguousarray(levels, dtype=np.complex64).reshape(-1)
        if spans.ndim != 2 or spans.shape[1] != capi.CMD_SPAN:
            raise ValueError("a command is searched in the 704 samples before a window: spans must be (n, 704)")
        if len(levels) != len(spans):
            raise ValueError("one level per span")
        out = np.zeros(len(spans), dtype=capi.COMMAND_DTYPE)
        self._chk(self._lib.rfid_commands_of(self._h, spans.ctypes.data, levels.ctypes.data, len(spans), out.ctypes.data))
        return out

    def batch_plan_fine(self) -> None:
        """Reserves the fine-channel workspace of the current plan (behind batch_plan_tracks; a new plan, batch_plan_inventory or
        batch_plan_tracks drops it, batch_plan_quality / batch_plan_repair do not)."""
        self._chk(self._lib.rfid_batch_plan_fine(self._h))

    def batch_fine_enqueue(self) -> None:
        """Asynchronous: the data-aided channel estimates of the last pass, behind its tracks (rfid_batch_fine)."""
        self._chk(self._lib.rfid_batch_fine(self._h))

    def batch_fine_fetch(self) -> np.ndarray:
        """-> capi.FINE_DTYPE records of the last batch_fine_enqueue (synchronises), one per CRC-verified read:
        record i belongs to reads[i] of batch_tracks_fetch."""
        return self._sized_fetch(self._lib.rfid_batch_get_fine, capi.FINE_DTYPE)

    def batch_fine(self) -> np.ndarray:
        """The data-aided channel estimate of every read of the last pass, and of its eight 16-bit segments, built on the
        device behind batch_tracks(): see batch_fine_fetch; rfid.batch.fine_fields turns the records into h, snr_db, the
        segments' h_k and the drift of their phase."""
        self.batch_fine_enqueue()
        return self.batch_fine_fetch()

    def batch_window_fine(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the fine table (synchronises): the record of EVERY EPC window before the cut-off, in seq order,
        failed ones included (n_windows_used // 2 of them; flags bit 0 tells them apart), of the last batch_fine_enqueue.
        extra > 0: up to that many of the table's rows behind them as well (zeroed by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_fine, capi.FINE_DTYPE, stream, extra)

    def batch_fine_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_fine_ms)

    def fine_window(self, gated, result) -> np.ndarray:
        """The same sums for ONE EPC window in host memory (rfid_fine_window): gated = its 1370 gated, DC-free samples,
        result = its capi.RESULT_DTYPE record (what decoder_work returned, or that record with bits the caller has
        corrected).  -> one capi.FINE_DTYPE record, stream = seq = start = 0."""
        return self._one_window(self._lib.rfid_fine_window, capi.FINE_DTYPE, gated, result)

    def batch_plan_retune(self) -> None:
        """Reserves the retune workspace of the current plan (a new plan drops it; no other stage's plan call does, and it
        needs none of them)."""
        self._chk(self._lib.rfid_batch_plan_retune(self._h))

    def batch_retune_enqueue(self) -> None:
        """Asynchronous: the CRC-failed EPC windows of the last pass decoded again over the Gen2 BLF tolerance, behind its
        statistics (rfid_batch_retune).  The pass's per-trace lengths must still be valid."""
        self._chk(self._lib.rfid_batch_retune(self._h))

    def batch_window_retunes(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the retune table (synchronises): the capi.RETUNE_DTYPE record of EVERY EPC window before the
        cut-off, in seq order (n_windows_used // 2 of them), of the last batch_retune_enqueue: flags bit 0 = the window was a
        read (nothing searched), bit 1 = the frame decoded again passes the CRC, bit 2 = the search ran into the trace's end.
        extra > 0: up to that many of the table's rows behind them as well (zeroed by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_retunes, capi.RETUNE_DTYPE, stream, extra)

    def batch_retune_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_retune_ms)

    def retune_window(self, span, result) -> np.ndarray:
        """The retune search for ONE span in host memory (rfid_retune_window): span = 1370 .. 1408 DC-free samples from the
        window's first on (indices behind the last one are held there), result = the window's capi.RESULT_DTYPE record (its
        index is the sync).  -> one capi.RETUNE_DTYPE record, stream = seq = start = 0."""
        span = np.ascontiguousarray(span, dtype=np.complex64)
        if span.ndim != 1 or not 1370 <= len(span) <= capi.RETUNE_SPAN:
            raise ValueError("a span has 1370 to %d samples" % capi.RETUNE_SPAN)
        res = np.zeros(1, dtype=capi.RESULT_DTYPE)
        res[0] = result
        out = np.zeros(1, dtype=capi.RETUNE_DTYPE)
        self._chk(self._lib.rfid_retune_window(self._h, span.ctypes.data, len(span), res.ctypes.data, out.ctypes.data))
        return out[0]

    def batch_plan_collisions(self) -> None:
        """Reserves the collisions workspace of the current plan (a new plan drops it; no other stage's plan call does, and it
        needs none of them)."""
        self._chk(self._lib.rfid_batch_plan_collisions(self._h))

    def batch_collisions_enqueue(self) -> None:
        """Asynchronous: both RN16s and both channels of every RN16 window of the last pass, as of a two-tag collision, behind
        its statistics (rfid_batch_collisions)."""
        self._chk(self._lib.rfid_batch_collisions(self._h))

    def batch_window_collisions(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the collisions table (synchronises): the capi.COLLISION_DTYPE record of EVERY RN16 window before
        the cut-off, in seq order ((n_windows_used + 1) // 2 of them), of the last batch_collisions_enqueue: rn16_a / ha of the
        stronger tag, rn16_b / hb of the weaker, flags bit 0 / 1 = the decoder's own RN16 is tag A's / tag B's, bit 2 = one
        cluster only, bit 3 = the tags were swapped.  extra > 0: up to that many of the table's rows behind them as well (zeroed
        by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_collisions, capi.COLLISION_DTYPE, stream, extra)

    def batch_collisions_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_collisions_ms)

    def collisions_of(self, windows, results) -> np.ndarray:
        """The same records for RN16 windows in host memory (rfid_collisions_of): windows = [n][250] gated, DC-free samples,
        results = their n capi.RESULT_DTYPE records (type RN16, index 65 .. 79).  -> capi.COLLISION_DTYPE records, stream = 0,
        seq = the window's position."""
        windows = np.ascontiguousarray(windows, dtype=np.complex64)
        if windows.ndim == 1:
            windows = windows.reshape(-1, capi.RN16_WINDOW) if len(windows) else windows.reshape(0, capi.RN16_WINDOW)
        if windows.ndim != 2 or windows.shape[1] != capi.RN16_WINDOW:
            raise ValueError("an RN16 window has 250 samples")
        res = np.zeros(len(windows), dtype=capi.RESULT_DTYPE)
        res[:] = np.atleast_1d(results)
        out = np.zeros(len(windows), dtype=capi.COLLISION_DTYPE)
        self._chk(self._lib.rfid_collisions_of(self._h, windows.ctypes.data, res.ctypes.data, len(windows), out.ctypes.data))
        return out

    def batch_plan_lengths(self) -> None:
        """Reserves the lengths workspace of the current plan (a new plan drops it; no other stage's plan call does, and it
        needs none of them)."""
        self._chk(self._lib.rfid_batch_plan_lengths(self._h))

    def batch_lengths_enqueue(self) -> None:
        """Asynchronous: the CRC-failed EPC windows of the last pass read again at the length their PC word announces, behind
        its statistics (rfid_batch_lengths).  The pass's per-trace lengths must still be valid."""
        self._chk(self._lib.rfid_batch_lengths(self._h))

    def batch_window_lengths(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the lengths table (synchronises): the capi.SIZED_FRAME_DTYPE record of EVERY EPC window before
        the cut-off, in seq order (n_windows_used // 2 of them), of the last batch_lengths_enqueue: flags bit 0 = the window was
        a read (nothing done), bit 1 = the frame at the PC's length passes its CRC, bit 2 = the frame ran into the trace's end,
        bit 3 = the PC announces more words than a slot holds, bit 4 = it announces the decoder's own length.  extra > 0: up to
        that many of the table's rows behind them as well (zeroed by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_lengths, capi.SIZED_FRAME_DTYPE, stream, extra)

    def batch_lengths_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_lengths_ms)

    def length_window(self, span, result) -> np.ndarray:
        """The same for ONE span in host memory (rfid_length_window): span = 1370 .. 1728 DC-free samples from the window's
        first on (indices behind the last one are held there), result = the window's capi.RESULT_DTYPE record (its T, index,
        h and first five bits are used).  -> one capi.SIZED_FRAME_DTYPE record, stream = seq = start = 0."""
        span = np.ascontiguousarray(span, dtype=np.complex64)
        if span.ndim != 1 or not 1370 <= len(span) <= capi.LENGTHS_SPAN:
            raise ValueError("a span has 1370 to %d samples" % capi.LENGTHS_SPAN)
        res = np.zeros(1, dtype=capi.RESULT_DTYPE)
        res[0] = result
        out = np.zeros(1, dtype=capi.SIZED_FRAME_DTYPE)
        self._chk(self._lib.rfid_length_window(self._h, span.ctypes.data, len(span), res.ctypes.data, out.ctypes.data))
        return out[0]

    def batch_plan_diversity(self, members: int) -> None:
        """Reserves the diversity workspace of the current plan for groups of `members` consecutive traces, 2 .. 8: the receive
        antennas of one session, the first the anchor (a new plan drops it; no other stage's plan call does, and it needs none of
        them)."""
        self._chk(self._lib.rfid_batch_plan_diversity(self._h, int(members)))

    def batch_diversity_enqueue(self) -> None:
        """Asynchronous: the EPC windows of every group of the last pass combined before the sign is taken, behind its statistics
        (rfid_batch_diversity).  The pass's stream count must be a multiple of the groups' size and its per-trace lengths still
        valid."""
        self._chk(self._lib.rfid_batch_diversity(self._h))

    def batch_window_diversity(self, group: int, extra: int = 0) -> np.ndarray:
        """One GROUP's row of the diversity table (synchronises): the capi.DIVERSITY_DTYPE record of EVERY EPC window of the group's
        anchor before its cut-off, in seq order (n_windows_used // 2 of them), of the last batch_diversity_enqueue: flags bit 0 =
        a present member read it (nothing combined), bit 1 = the combined frame passes its CRC, bit 2 = fewer than two members are
        present (nothing combined).  extra > 0: up to that many of the table's rows behind them as well (zeroed by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_diversity, capi.DIVERSITY_DTYPE, group, extra)

    def batch_diversity_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_diversity_ms)

    def diversity_window(self, spans, results) -> np.ndarray:
        """The same for the windows of ONE row in host memory (rfid_diversity_window): spans = (members, 1370) DC-free samples,
        results = the members' capi.RESULT_DTYPE records, 2 .. 8 of them; all members are present.  -> one capi.DIVERSITY_DTYPE
        record, stream = seq = start = 0."""
        spans = np.ascontiguousarray(spans, dtype=np.complex64)
        if spans.ndim != 2 or spans.shape[1] != 1370 or not 2 <= len(spans) <= capi.DIVERSITY_MAX_MEMBERS:
            raise ValueError("spans must be (members, 1370), 2 to %d members" % capi.DIVERSITY_MAX_MEMBERS)
        if len(results) != len(spans):
            raise ValueError("one result per member")
        res = np.zeros(len(spans), dtype=capi.RESULT_DTYPE)
        for m, r in enumerate(results):
            res[m] = r
        out = np.zeros(1, dtype=capi.DIVERSITY_DTYPE)
        self._chk(self._lib.rfid_diversity_window(self._h, spans.ctypes.data, len(spans), res.ctypes.data, out.ctypes.data))
        return out[0]

    def batch_plan_match(self) -> None:
        """Reserves the match workspace of the current plan, with room for a list of capi.MATCH_MAX_LIST frames (a new plan drops
        it and the list; no other stage's plan call does)."""
        self._chk(self._lib.rfid_batch_plan_match(self._h))

    @staticmethod
    def _frames(frames) -> np.ndarray:
        f = np.ascontiguousarray(frames, dtype=np.uint32)
        if f.ndim == 1 and len(f) % 4 == 0:
            f = f.reshape(-1, 4)
        if f.ndim != 2 or f.shape[1] != 4:
            raise ValueError("frames must be (n, 4) words, packed as a result's bits")
        return f

    def batch_match_set_list(self, frames=None) -> None:
        """The candidates of every trace from now on (rfid_batch_match_set_list, synchronises): frames = (n, 4) uint32 words, packed
        as a result's bits (rfid.frame_of_epc builds one from an EPC), up to capi.MATCH_MAX_LIST of them, copied to the device.  None
        or an empty list: every trace's own inventory again."""
        f = self._frames(frames if frames is not None else np.zeros((0, 4), dtype=np.uint32))
        if len(f) > capi.MATCH_MAX_LIST:
            raise ValueError("a list holds at most %d frames" % capi.MATCH_MAX_LIST)
        self._chk(self._lib.rfid_batch_match_set_list(self._h, f.ctypes.data if len(f) else None, len(f)))

    def batch_match_enqueue(self) -> None:
        """Asynchronous: the CRC-failed EPC windows of the last pass correlated against the known tags' frames (rfid_batch_match):
        without a list behind the pass's inventory (batch_inventory_enqueue first, as for the repair stage), with one behind its
        statistics."""
        self._chk(self._lib.rfid_batch_match(self._h))

    def batch_window_matches(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the match table (synchronises): the capi.MATCH_DTYPE record of EVERY EPC window before the cut-off,
        in seq order (n_windows_used // 2 of them), of the last batch_match_enqueue: flags bit 0 = the window was a read, bit 1 =
        the trace's inventory overflowed, bit 2 = no candidates (nothing searched in all three), bit 3 = the candidates are the
        caller's list.  rfid.batch.match_fields() says which records are attributions.  extra > 0: up to that many of the table's
        rows behind them as well (zeroed by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_matches, capi.MATCH_DTYPE, stream, extra)

    def batch_match_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_match_ms)

    def match_window(self, gated, result, frames) -> np.ndarray:
        """The same for ONE window in host memory (rfid_match_window): gated = 1370 DC-free samples, result = the window's
        capi.RESULT_DTYPE record, frames = (n, 4) candidate frames, 1 .. capi.MATCH_MAX_LIST.  -> one capi.MATCH_DTYPE record,
        stream = seq = start = 0."""
        gated = np.ascontiguousarray(gated, dtype=np.complex64)
        if gated.ndim != 1 or len(gated) != 1370:
            raise ValueError("an EPC window has 1370 samples")
        f = self._frames(frames)
        if not 1 <= len(f) <= capi.MATCH_MAX_LIST:
            raise ValueError("1 to %d candidate frames" % capi.MATCH_MAX_LIST)
        res = np.zeros(1, dtype=capi.RESULT_DTYPE)
        res[0] = result
        out = np.zeros(1, dtype=capi.MATCH_DTYPE)
        self._chk(self._lib.rfid_match_window(self._h, gated.ctypes.data, res.ctypes.data, f.ctypes.data, len(f), out.ctypes.data))
        return out[0]

    def batch_plan_stack(self) -> None:
        """Reserves the stack workspace of the current plan (a new plan drops it; no other stage's plan call does)."""
        self._chk(self._lib.rfid_batch_plan_stack(self._h))

    def batch_stack_enqueue(self, rho_min: float = 0.5) -> None:
        """Asynchronous: the CRC-failed EPC windows of the last pass that hold the same frame found by the correlation of their
        decision values (s >= rho_min * a, 0 < rho_min <= 1) and combined before the sign is taken (rfid_batch_stack): behind
        the pass's statistics, as the match stage with a list."""
        self._chk(self._lib.rfid_batch_stack(self._h, float(rho_min)))

    def batch_window_stacks(self, stream: int, extra: int = 0) -> np.ndarray:
        """One trace's row of the stack table (synchronises): the capi.STACK_DTYPE record of EVERY EPC window before the cut-off,
        in seq order (n_windows_used // 2 of them), of the last batch_stack_enqueue: flags bit 0 = the window was a read, bit 1 =
        a combination was formed (the window has partners: member_mask, bit l = failed row 64 * (ordinal // 64) + l), bit 2 = the
        combination's CRC holds and `frame` is a frame.  extra > 0: up to that many of the table's rows behind them as well
        (zeroed by the stage)."""
        return self._window_rows(self._lib.rfid_batch_get_window_stacks, capi.STACK_DTYPE, stream, extra)

    def batch_stack_ms(self) -> float:
        return self._stage_ms(self._lib.rfid_batch_stack_ms)

    def stack_windows(self, gated, results, rho_min: float = 0.5) -> np.ndarray:
        """The same for n = 1 .. capi.STACK_MAX_WINDOWS windows in host memory, one block (rfid_stack_windows): gated = (n, 1370)
        DC-free samples, results = the windows' capi.RESULT_DTYPE records.  -> n capi.STACK_DTYPE records, stream = seq = start = 0."""
        gated = np.ascontiguousarray(gated, dtype=np.complex64)
        if gated.ndim != 2 or gated.shape[1] != 1370 or not 1 <= gated.shape[0] <= capi.STACK_MAX_WINDOWS:
            raise ValueError("gated must be (n, 1370), n = 1 .. %d" % capi.STACK_MAX_WINDOWS)
        if len(results) != len(gated):
            raise ValueError("one result record per window")
        res = np.zeros(len(gated), dtype=capi.RESULT_DTYPE)
        for i, r in enumerate(results):
            res[i] = r
        out = np.zeros(len(gated), dtype=capi.STACK_DTYPE)
        self._chk(self._lib.rfid_stack_windows(self._h, gated.ctypes.data, res.ctypes.data, len(gated), float(rho_min), out.ctypes.data))
        return out

    def batch_mf_output(self, stream: int) -> np.ndarray:
        cap = self._planned[1] // 5 + 1
        out = np.empty(cap, dtype=np.complex64)
        n = C.c_int64(0)
        self._chk(self._lib.rfid_batch_get_mf(self._h, int(stream), out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].copy()

    def batch_gated_output(self, stream: int, seq: int) -> np.ndarray:
        """Gated, DC-removed samples of window `seq` of trace `stream` (the gate block's output; debug tap)."""
        out = np.empty(1370, dtype=np.complex64)
        n = C.c_int64(0)
        self._chk(self._lib.rfid_batch_get_gated(self._h, int(stream), int(seq), out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def synth_replicas_ptr(self, d_base: int, n_raw: int, d_out: int, out_stride: int, n_streams: int, sigma: float,
                           seed: int, first_replica: int = 0) -> None:
        """Asynchronous: d_out[s] = d_base + sigma * complex Gaussian noise (replica first_replica + s)."""
        self._chk(self._lib.rfid_synth_replicas(self._h, C.c_void_p(d_base), int(n_raw), C.c_void_p(d_out), int(out_stride),
                                                int(n_streams), C.c_float(sigma), C.c_uint64(seed), int(first_replica)))

    def _gen2_params(self, plan) -> "capi.SynthGen2Params":
        p = capi.SynthGen2Params()
        lk = np.complex64(plan.leak)
        p.leak_re, p.leak_im = float(lk.real), float(lk.imag)
        for k, h in enumerate(plan.hs):
            hk = np.complex64(h)
            p.h_re[k], p.h_im[k] = float(hk.real), float(hk.imag)
        p.n_tags = len(plan.hs)
        p.tail_us = int(plan.tail_us)
        return p

    def synth_gen2_size(self, plan) -> int:
        """Samples of the trace rfid_synth_gen2 builds from `plan` (rfid.synth.TracePlan)."""
        slots = np.ascontiguousarray(plan.slots)
        n = C.c_int64(0)
        p = self._gen2_params(plan)
        self._chk(self._lib.rfid_synth_gen2_size(C.byref(p), slots.ctypes.data, len(slots), C.byref(n)))
        return n.value

    def synth_gen2_ptr(self, plan, d_out: int, out_cap: int, sigma: float = 0.0, seed: int = 0, replica: int = 0) -> int:
        """Asynchronous: the Gen2 receive trace of `plan` generated in HBM at d_out; returns its sample count."""
        slots = np.ascontiguousarray(plan.slots)
        n = C.c_int64(0)
        p = self._gen2_params(plan)
        self._chk(self._lib.rfid_synth_gen2(self._h, C.byref(p), slots.ctypes.data, len(slots), C.c_void_p(d_out),
                                            int(out_cap), C.c_float(sigma), C.c_uint64(seed), int(replica), C.byref(n)))
        return n.value

    def batch_device_ptrs(self) -> dict:
        y, st, fc = C.c_void_p(), C.c_void_p(), C.c_void_p()
        stride = C.c_int64(0)
        self._chk(self._lib.rfid_batch_device_ptrs(self._h, C.byref(y), C.byref(stride), C.byref(st), C.byref(fc)))
        return dict(mf_out=y.value, mf_stride=stride.value, stats=st.value, flat_count=fc.value)


def unpack_bits(words: np.ndarray, n_bits: int) -> np.ndarray:
    """rfid_decode_result.bits -> array of n_bits 0/1 values (frame order)."""
    words = np.asarray(words, dtype=np.uint32)
    j = np.arange(n_bits)
    return ((words[j >> 5] >> (j & 31)) & 1).astype(np.uint8)


def frame_of_epc(epc_hex: str, pc: int = 0x3000) -> np.ndarray:
    """PC + EPC + CRC-16: the 128-bit frame a tag with this 96-bit EPC (24 hex digits, MSB first as sent) and PC word replies with,
    packed as rfid_decode_result.bits -> four uint32 words.  The CRC is Gen2's (CCITT 0x1021, preset 0xFFFF, complemented) over
    the 112 bits before it: what rfid_batch_match_set_list and rfid_match_window take as a candidate."""
    digits = "".join(str(epc_hex).split()).lower()
    if digits.startswith("0x"):
        digits = digits[2:]
    if len(digits) != 24:
        raise ValueError("an EPC has 24 hex digits (96 bits)")
    if not 0 <= int(pc) <= 0xFFFF:
        raise ValueError("the PC is a 16-bit word")
    body = (int(pc) << 96) | int(digits, 16)
    bits = [(body >> (111 - i)) & 1 for i in range(112)]
    reg = 0xFFFF
    for b in bits:
        msb = (reg >> 15) & 1
        reg = (reg << 1) & 0xFFFF
        if msb ^ b:
            reg ^= 0x1021
    reg ^= 0xFFFF
    bits += [(reg >> i) & 1 for i in range(15, -1, -1)]
    words = np.zeros(4, dtype=np.uint32)
    for j, b in enumerate(bits):
        words[j >> 5] |= np.uint32(b << (j & 31))
    return words

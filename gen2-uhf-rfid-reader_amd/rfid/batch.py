"""Bulk offline decoding of recorded traces.

Trace files are what the reference's flowgraph reads and writes: headerless little-endian
interleaved float32 I,Q (blocks.file_source / file_sink, apps/reader.py:68-72,102-103;
misc/code/plot_signal.m:5-9).  Traces are packed into one [n_traces][stride] HBM buffer
(pinned host staging, asynchronous copies) and decoded by one rfid_batch_process() pass.
torch is used to own the pinned / device memory only.
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence

import numpy as np

from . import _capi as capi
from ._capi import CMD_ACK, CMD_QUERY, CMD_QUERY_REP, CMD_SPAN     # (RFID_CMD_*: one copy, the binding's)
from .context import Context


def read_trace_file(path: str) -> np.ndarray:
    """Interleaved float32 I,Q file -> complex64 array (zero-copy view of the file's bytes)."""
    return np.fromfile(path, dtype=np.complex64)


def write_trace_file(path: str, samples: np.ndarray) -> None:
    np.ascontiguousarray(samples, dtype=np.complex64).tofile(path)


class BatchDecoder:
    """Decode many independent traces per pass on one GPU."""

    def __init__(self, device: int = 0, **params):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("rfid.batch needs a GPU: the receive path has no CPU fallback")
        self._torch = torch
        self.device = int(device)
        self.ctx = Context(device=device, **params)
        self._planned = (0, 0)
        self._dev = None
        self._pinned = None
        self._lens_dev = None
        self._inv_tags = 0
        self._trk_planned = False
        self.last_inventory = None    # (entries, per-trace counts) of the last decode(..., inventory=True)
        self.last_tracks = None       # (reads, offsets) of the last decode(..., tracks=True)
        self._qual_planned = False
        self.last_quality = None      # one record per read, aligned with last_tracks[0], of the last decode(..., quality=True)
        self._rep_planned = False
        self.last_repairs = None      # the repaired windows, ordered by (stream, seq), of the last decode(..., repair=True)
        self._slots_planned = False
        self.last_slots = None        # one moments array per trace (every window before the cut-off) of the last decode(..., slots=True)
        self._cmd_planned = False
        self.last_commands = None     # one commands array per trace (every window before the cut-off) of the last decode(..., commands=True)
        self._fine_planned = False
        self.last_fine = None         # one record per read, aligned with last_tracks[0], of the last decode(..., fine=True)
        self._ret_planned = False
        self.last_retunes = None      # one retune array per trace (every EPC window before the cut-off) of the last decode(..., retune=True)
        self._col_planned = False
        self.last_collisions = None   # one collisions array per trace (every RN16 window before the cut-off) of the last decode(..., collisions=True)
        self._len_planned = False
        self.last_lengths = None      # one sized-frame array per trace (every EPC window before the cut-off) of the last decode(..., lengths=True)
        self._div_members = 0         # (the group size the diversity workspace was planned for; 0: none)
        self.last_diversity = None    # one diversity array per GROUP (every EPC window before its anchor's cut-off) of the last decode(..., diversity=M)
        self._mat_planned = False
        self.last_matches = None      # one match array per trace (every EPC window before the cut-off) of the last decode(..., match=True)
        self._stk_planned = False
        self.last_stacks = None       # one stack array per trace (every EPC window before the cut-off) of the last decode(..., stack=rho)

    def close(self) -> None:
        self.ctx.close()

    def _ensure(self, n_traces: int, max_len: int) -> int:
        torch = self._torch
        stride = (max_len + 1) & ~1
        if self._planned[0] < n_traces or self._planned[1] < max_len:
            self.ctx.batch_plan(max(n_traces, self._planned[0]), max(max_len, self._planned[1]))
            self._planned = (max(n_traces, self._planned[0]), max(max_len, self._planned[1]))
            self._inv_tags = 0        # (a new plan drops the inventory workspace, and the tracks and quality workspaces with it)
            self._trk_planned = False
            self._qual_planned = False
            self._rep_planned = False
            self._slots_planned = False
            self._cmd_planned = False
            self._fine_planned = False
            self._ret_planned = False
            self._col_planned = False
            self._len_planned = False
            self._div_members = 0
            self._mat_planned = False
            self._stk_planned = False
        # the plan may be larger than this batch (decoder reuse): process exactly n_traces rows
        self.ctx.batch_set_streams(n_traces)
        need = n_traces * stride * 2
        if self._dev is None or self._dev.numel() < need:
            self._dev = torch.empty(need, dtype=torch.float32, device=f"cuda:{self.device}")
            self._pinned = torch.empty(need, dtype=torch.float32, pin_memory=True)
        return stride

    def decode(self, traces: Sequence[np.ndarray], want_scores: bool = False, timing: Optional[dict] = None,
               inventory: bool = False, max_tags: int = 64, tracks: bool = False, quality: bool = False,
               repair: bool = False, slots: bool = False, commands: bool = False, fine: bool = False,
               retune: bool = False, collisions: bool = False, lengths: bool = False, diversity: int = 0,
               match: bool = False, match_list=None, stack: float = 0.0):
        """traces: list of complex64 arrays (ragged).  Returns (stats, windows, results, scores).

        `timing` (optional dict) receives h2d_s / gpu_s / total_s of this call.  inventory=True: the distinct EPC frames
        of every trace (up to max_tags per trace) are listed on the device behind the pass and kept as
        `self.last_inventory` = (entries, per-trace counts); the return value is the same.  tracks=True (implies
        inventory=True): every tag's reads in time order are listed behind the inventory and kept as `self.last_tracks` =
        (reads, offsets), offsets aligned with the entries.  quality=True (implies tracks=True): the SNR and decision
        margin of every EPC window are worked out behind the tracks; `self.last_quality` keeps one record per read, aligned
        with the reads (quality_fields() turns them into snr_db and margin); a trace's whole row, failed windows included:
        `self.ctx.batch_window_quality(stream)`.  repair=True (implies inventory=True): the CRC-failed EPC windows that
        reversing one to three of their eight weakest decisions makes pass are searched behind the inventory;
        `self.last_repairs` keeps their records (capi.REPAIR_DTYPE, ordered by (stream, seq)); a repair is not a read and
        changes nothing else; a trace's whole row: `self.ctx.batch_window_repairs(stream)`.  slots=True (implies nothing):
        the second-order moments of every window, RN16 and EPC alike, are worked out behind the pass; `self.last_slots` keeps
        one capi.MOMENTS_DTYPE array per trace (classify_slots() turns it into empty / single / collided per slot).
        commands=True (implies nothing): the reader's own PIE command in front of every window is decoded behind the pass;
        `self.last_commands` keeps one capi.COMMAND_DTYPE array per trace (command_fields() turns it into names, Q, RN16 and
        timings).  fine=True (implies tracks=True): the data-aided channel estimate of every EPC window -- from all 256 half-bit
        samples of the frame instead of six of the preamble -- and of its eight 16-bit segments is worked out behind the
        tracks; `self.last_fine` keeps one capi.FINE_DTYPE record per read, aligned with the reads (fine_fields() turns them
        into h, snr_db, the segments' h_k and the phase drift); a trace's whole row: `self.ctx.batch_window_fine(stream)`.
        retune=True (implies nothing): the CRC-failed EPC windows are decoded again behind the pass with the half-bit period
        searched over the whole +- 4 % Gen2 allows a tag's link frequency (the decoder searches +- 1 %); `self.last_retunes` keeps
        one capi.RETUNE_DTYPE array per trace, a record per EPC window (retune_fields() turns it into the link frequency and its
        offset); a retuned frame is not a read and changes nothing else.  collisions=True (implies slots=True: the report needs the
        class): both RN16s and both channels of every RN16 window, as of two tags replying at once, are worked out behind the pass;
        `self.last_collisions` keeps one capi.COLLISION_DTYPE array per trace, a record per RN16 window (classify_collisions() keeps
        those of the collided slots and tells two tags from more); nothing else changes.  lengths=True (implies nothing): the
        CRC-failed EPC windows are read again behind the pass at the length their own PC word announces (the decoder takes every
        reply for a 96-bit EPC); `self.last_lengths` keeps one capi.SIZED_FRAME_DTYPE array per trace, a record per EPC window
        (sized_frame_fields() turns one into PC, EPC and its length); such a frame is not a read and changes nothing else.
        diversity=M, 2 .. 8 (implies nothing): the traces are groups of M consecutive ones -- the receive antennas of one session, each
        group's first the anchor; len(traces) must be a multiple of M -- and the EPC windows no antenna read are decided again behind
        the pass from the antennas' summed decision values; `self.last_diversity` keeps one capi.DIVERSITY_DTYPE array per GROUP, a
        record per EPC window of its anchor (diversity_fields() turns it into flags, member lists and the summed channel power); a
        combined frame is not a read and changes nothing else.  match=True: the CRC-failed EPC windows are correlated behind the pass
        against the frames of known tags -- match_list=frames, (n, 4) words as frame_of_epc() builds them, the same for every trace, or
        without a list every trace's own inventory (then it implies inventory=True); `self.last_matches` keeps one capi.MATCH_DTYPE
        array per trace, a record per EPC window (match_fields() says which are attributions); an attribution is not a read and
        changes nothing else.  stack=rho (0 < rho <= 1; 0: off): the CRC-failed EPC windows of a trace whose decision values correlate
        (s >= rho * a, within blocks of 64 failed windows) are added up behind the pass before the sign is taken -- an unknown tag's
        repeated frame over the rounds of a session; `self.last_stacks` keeps one capi.STACK_DTYPE array per trace, a record per EPC
        window (stack_fields() turns it into flags and member lists); a stacked frame is not a read and changes nothing else."""
        torch = self._torch
        n = len(traces)
        match = bool(match) or match_list is not None
        own_match = match and (match_list is None or len(match_list) == 0)
        diversity = int(diversity)
        if diversity and n % diversity:
            raise ValueError("diversity: %d traces are no whole groups of %d" % (n, diversity))
        lens = np.array([len(t) for t in traces], dtype=np.int64)
        max_len = int(lens.max()) if n else 0
        if n == 0 or max_len == 0:
            raise ValueError("no samples")
        stride = self._ensure(n, max_len)
        t0 = time.perf_counter()
        host = self._pinned[: n * stride * 2].numpy().view(np.complex64).reshape(n, stride)
        for i, t in enumerate(traces):
            host[i, : len(t)] = t
        dev = self._dev[: n * stride * 2]
        with torch.cuda.device(self.device):
            dev.copy_(self._pinned[: n * stride * 2], non_blocking=True)
            self._lens_dev = torch.from_numpy(lens).to(dev.device, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        t1 = time.perf_counter()
        tracks = tracks or quality or fine
        slots = slots or collisions
        inventory = inventory or tracks or repair or own_match
        if inventory and self._inv_tags != int(max_tags):
            self.ctx.batch_plan_inventory(int(max_tags))
            self._inv_tags = int(max_tags)
            self._trk_planned = False
            self._rep_planned = False
        if repair and not self._rep_planned:
            self.ctx.batch_plan_repair()
            self._rep_planned = True
        if tracks and not self._trk_planned:
            self.ctx.batch_plan_tracks()
            self._trk_planned = True
            self._qual_planned = False
            self._fine_planned = False
        if quality and not self._qual_planned:
            self.ctx.batch_plan_quality()
            self._qual_planned = True
        if fine and not self._fine_planned:
            self.ctx.batch_plan_fine()
            self._fine_planned = True
        if slots and not self._slots_planned:
            self.ctx.batch_plan_slots()
            self._slots_planned = True
        if commands and not self._cmd_planned:
            self.ctx.batch_plan_commands()
            self._cmd_planned = True
        if retune and not self._ret_planned:
            self.ctx.batch_plan_retune()
            self._ret_planned = True
        if collisions and not self._col_planned:
            self.ctx.batch_plan_collisions()
            self._col_planned = True
        if lengths and not self._len_planned:
            self.ctx.batch_plan_lengths()
            self._len_planned = True
        if diversity and self._div_members != diversity:
            self.ctx.batch_plan_diversity(diversity)
            self._div_members = diversity
        if match:
            if not self._mat_planned:
                self.ctx.batch_plan_match()
                self._mat_planned = True
            self.ctx.batch_match_set_list(None if own_match else match_list)
        if stack and not self._stk_planned:
            self.ctx.batch_plan_stack()
            self._stk_planned = True
        self.ctx.batch_process_ptr(dev.data_ptr(), stride, max_len, self._lens_dev.data_ptr(), want_scores=want_scores)
        if inventory:
            self.ctx.batch_inventory_enqueue()
        if tracks:
            self.ctx.batch_tracks_enqueue()
        if quality:
            self.ctx.batch_quality_enqueue()
        if repair:
            self.ctx.batch_repair_enqueue()
        if slots:
            self.ctx.batch_slots_enqueue()
        if commands:
            self.ctx.batch_commands_enqueue()
        if fine:
            self.ctx.batch_fine_enqueue()
        if retune:
            self.ctx.batch_retune_enqueue()
        if collisions:
            self.ctx.batch_collisions_enqueue()
        if lengths:
            self.ctx.batch_lengths_enqueue()
        if diversity:
            self.ctx.batch_diversity_enqueue()
        if match:
            self.ctx.batch_match_enqueue()
        if stack:
            self.ctx.batch_stack_enqueue(float(stack))
        self.ctx.batch_sync()
        t2 = time.perf_counter()
        if inventory:
            self.last_inventory = self.ctx.batch_inventory_fetch()
        if tracks:
            self.last_tracks = self.ctx.batch_tracks_fetch()
        if quality:
            self.last_quality = self.ctx.batch_quality_fetch()
        if repair:
            self.last_repairs = self.ctx.batch_repair_fetch()
        if slots:
            self.last_slots = [self.ctx.batch_window_moments(b) for b in range(n)]
        if commands:
            self.last_commands = [self.ctx.batch_window_commands(b) for b in range(n)]
        if fine:
            self.last_fine = self.ctx.batch_fine_fetch()
        if retune:
            self.last_retunes = [self.ctx.batch_window_retunes(b) for b in range(n)]
        if collisions:
            self.last_collisions = [self.ctx.batch_window_collisions(b) for b in range(n)]
        if lengths:
            self.last_lengths = [self.ctx.batch_window_lengths(b) for b in range(n)]
        if diversity:
            self.last_diversity = [self.ctx.batch_window_diversity(g) for g in range(n // diversity)]
        if match:
            self.last_matches = [self.ctx.batch_window_matches(b) for b in range(n)]
        if stack:
            self.last_stacks = [self.ctx.batch_window_stacks(b) for b in range(n)]
        stats = self.ctx.batch_stats()[:n]
        w, r, s = self.ctx.batch_windows(want_scores=want_scores)
        if timing is not None:
            timing.update(h2d_s=t1 - t0, gpu_s=t2 - t1, total_s=time.perf_counter() - t0,
                          raw_samples=int(lens.sum()))
        return stats, w, r, s

    def decode_files(self, paths: Sequence[str], **kw):
        return self.decode([read_trace_file(p) for p in paths], **kw)


def summarize(stats: np.ndarray) -> List[dict]:
    """Per-trace READER_STATS as dicts (what reader_impl::print_results reports)."""
    out = []
    for s in stats:
        out.append(dict(n_queries_sent=int(s["n_queries_sent"]) - 1, cur_inventory_round=int(s["cur_inventory_round"]),
                        n_epc_correct=int(s["n_epc_correct"]), n_unique_tags=int(s["n_unique_tags"]),
                        tag_reads={i: int(c) for i, c in enumerate(s["tag_reads"]) if c}))
    return out


def format_results(stats_row) -> str:
    """The text reader_impl::print_results writes (lib/reader_impl.cc:173-192) for one trace of a batch."""
    s = stats_row
    lines = ["", " --------------------------", "| Number of queries/queryreps sent : %d" % (int(s["n_queries_sent"]) - 1),
             "| Current Inventory round : %d" % int(s["cur_inventory_round"]), " --------------------------",
             "| Correctly decoded EPC : %d" % int(s["n_epc_correct"]),
             "| Number of unique tags : %d" % int(s["n_unique_tags"])]
    for i, c in enumerate(s["tag_reads"]):
        if c:
            lines.append("| Tag ID : %x  Num of reads : %d" % (i, int(c)))
    lines.append(" --------------------------")
    return "\n".join(lines) + "\n"


def merge_inventory(entries: np.ndarray) -> np.ndarray:
    """Per-trace inventory entries (Context.batch_inventory) -> one entry per distinct frame over all traces: reads
    summed, `stream` / `first_seq` / `last_seq` / `best_*` those of the trace that read it best (largest |best h|,
    the lowest trace on ties); ordered by frame.  Host side: the tables are tiny."""
    entries = np.asarray(entries)
    if len(entries) == 0:
        return entries.copy()
    frames = np.ascontiguousarray(entries["frame"])
    _, first, inverse = np.unique(frames, axis=0, return_index=True, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    norm = entries["best_h_re"].astype(np.float64) ** 2 + entries["best_h_im"].astype(np.float64) ** 2
    out = entries[first].copy()
    for g in range(len(first)):
        idx = np.flatnonzero(inverse == g)
        out[g] = entries[idx[int(np.argmax(norm[idx]))]]
        out[g]["reads"] = int(entries["reads"][idx].sum())
    return out


def frame_fields(frame) -> tuple:
    """rfid_tag_entry.frame -> (PC as an int, EPC as 24 hex digits), bits MSB first as sent."""
    w = np.asarray(frame, dtype=np.uint32)
    j = np.arange(128)
    bits = ((w[j >> 5] >> (j & 31)) & 1).astype(np.uint8)
    val = lambda b: int("".join(map(str, b.tolist())), 2)
    return val(bits[:16]), "%024x" % val(bits[16:112])


def format_inventory(entries: np.ndarray) -> str:
    """One line per entry: EPC (24 hex digits), PC, reads, first / last window seq, 20 log10 |best h|."""
    lines = ["| EPC                       PC    reads  first   last   best |h| dB"]
    for e in entries:
        pc, epc = frame_fields(e["frame"])
        mag = float(np.hypot(np.float64(e["best_h_re"]), np.float64(e["best_h_im"])))
        db = 20.0 * np.log10(mag) if mag > 0 else float("-inf")
        lines.append("| %s  %04x  %5d  %5d  %5d  %8.2f" % (epc, pc, int(e["reads"]), int(e["first_seq"]), int(e["last_seq"]), db))
    lines.append(" --------------------------")
    return "\n".join(lines) + "\n"


TRACKS_HEADER = "file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T"
TRACKS_RATE = 400e3       # samples per second behind the decimation of a 2 Msps trace: what rfid_window::start counts


TRACKS_QUALITY_HEADER = TRACKS_HEADER + ",snr_db,margin"


def quality_fields(q: np.ndarray):
    """rfid_read_quality records -> (snr_db, margin), float64 arrays: snr_db = 10 log10(sig_sq / quad_sq) (+inf when
    quad_sq == 0 < sig_sq, nan when both are 0), margin = margin_min / (sig_abs / 128): the weakest of the 128 decisions
    relative to the mean one."""
    q = np.asarray(q)
    sig, quad = q["sig_sq"].astype(np.float64), q["quad_sq"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr_db = 10.0 * np.log10(sig / quad)
        margin = q["margin_min"].astype(np.float64) / (q["sig_abs"].astype(np.float64) / 128.0)
    return snr_db, margin


def format_quality(rows: np.ndarray) -> str:
    """One line for one trace's EPC windows before the cut-off (Context.batch_window_quality): how many there are, how many
    failed their CRC, the median snr_db of the reads and of the failed windows, the weakest margin among the reads."""
    rows = np.asarray(rows)
    ok = (rows["flags"] & 1) != 0
    snr_db, margin = quality_fields(rows)
    med = lambda v: "%.2f" % float(np.median(v)) if len(v) else "-"
    return ("| EPC windows : %d  failed : %d  median SNR dB reads : %s  failed : %s  weakest margin of a read : %s\n" %
            (len(rows), int((~ok).sum()), med(snr_db[ok]), med(snr_db[~ok]), ("%.3f" % float(margin[ok].min())) if ok.any() else "-"))


TRACKS_FINE_COLUMNS = ",hd_re,hd_im,hd_mag_db,hd_phase_rad,hd_snr_db,drift_rad_s"
FINE_SEGMENT_S = 16 * 25e-6       # a segment of 16 bits at 40 kbps: the segments' centres are 400 us apart


def fine_fields(f: np.ndarray) -> dict:
    """rfid_read_fine records -> a dict of float64 / complex128 arrays, one value per record:
    h = (sum_re + j sum_im) / 128, the data-aided channel estimate in the units of h_est; mag_db = 20 log10 |h|; phase_rad =
    angle(h); noise = (pow - |sum|^2 / 128) / 127, the noise power of one of the 128 differences (both components; what is
    left of their power when the part along the estimate is taken out); snr_db = 10 log10(|h|^2 / noise) (+inf when the noise
    is not positive, nan for an all-zero record); h_seg [n][8] = seg / 16, the channel of each 16-bit segment; drift_rad_s =
    the least-squares slope of angle(h_k conj(h)) over the segments' centres, 400 us apart."""
    f = np.asarray(f)
    re, im = f["sum_re"].astype(np.float64), f["sum_im"].astype(np.float64)
    sq = re * re + im * im                    # |sum|^2
    h = re / 128.0 + 1j * (im / 128.0)
    mag = np.sqrt(sq) / 128.0
    noise = (f["pow"].astype(np.float64) - sq / 128.0) / 127.0
    h_seg = (f["seg_re"].astype(np.float64) + 1j * f["seg_im"].astype(np.float64)) / 16.0
    t = (np.arange(capi.FINE_SEGMENTS) - (capi.FINE_SEGMENTS - 1) / 2.0) * FINE_SEGMENT_S
    with np.errstate(divide="ignore", invalid="ignore"):
        mag_db = 20.0 * np.log10(mag)
        snr_db = np.where(noise > 0, 10.0 * np.log10(mag ** 2 / np.where(noise > 0, noise, 1.0)), np.where(mag > 0, np.inf, np.nan))
    ph = np.angle(h_seg * np.conj(h)[..., None])
    drift = ((ph - ph.mean(axis=-1, keepdims=True)) * t).sum(axis=-1) / float((t * t).sum())
    return dict(h=h, mag_db=mag_db, phase_rad=np.arctan2(im, re), noise=noise, snr_db=snr_db, h_seg=h_seg, drift_rad_s=drift)


def format_fine(rows: np.ndarray) -> str:
    """One line for one trace's EPC windows before the cut-off (Context.batch_window_fine): how many there are, how many
    failed their CRC, and over the reads the median of the data-aided |h| in dB, of its SNR and of the magnitude of the
    phase drift inside a read."""
    rows = np.asarray(rows)
    ok = (rows["flags"] & 1) != 0
    ff = fine_fields(rows)
    med = lambda v, fmt: fmt % float(np.median(v)) if len(v) else "-"
    return ("| EPC windows : %d  failed : %d  data-aided h of the reads, medians: |h| dB : %s  SNR dB : %s  |drift| rad/s : %s\n" %
            (len(rows), int((~ok).sum()), med(ff["mag_db"][ok], "%.2f"), med(ff["snr_db"][ok], "%.2f"),
             med(np.abs(ff["drift_rad_s"][ok]), "%.1f")))


def format_tracks(entries: np.ndarray, reads: np.ndarray, offsets: np.ndarray, names: Sequence[str],
                  quality: Optional[np.ndarray] = None, fine: Optional[np.ndarray] = None) -> str:
    """CSV text, one line per read in the order of `reads` (grouped by tag, time order inside a tag):
    file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T with t_s = start / 400e3.  entries / offsets: the packed inventory
    and the offsets aligned with it (Context.batch_inventory_fetch / batch_tracks_fetch); names[stream]: the trace's file.
    Floats are printed with %.9g: binary32 values survive the round trip.  quality (optional; the records aligned with
    `reads`, Context.batch_quality_fetch): two more columns, snr_db,margin (quality_fields).  fine (optional; the records
    aligned with `reads`, Context.batch_fine_fetch): behind those, hd_re,hd_im,hd_mag_db,hd_phase_rad,hd_snr_db,drift_rad_s
    (fine_fields: the data-aided h, in the units of h_re,h_im)."""
    lines = [(TRACKS_HEADER if quality is None else TRACKS_QUALITY_HEADER) + (TRACKS_FINE_COLUMNS if fine is not None else "")]
    if quality is not None:
        assert len(quality) == len(reads)
        snr_db, margin = quality_fields(quality)
    if fine is not None:
        assert len(fine) == len(reads)
        ff = fine_fields(fine)
    for i, e in enumerate(entries):
        pc, epc = frame_fields(e["frame"])
        name = names[int(e["stream"])]
        for k in range(int(offsets[i]), int(offsets[i + 1])):
            r = reads[k]
            re, im = np.float64(r["h_re"]), np.float64(r["h_im"])
            mag = float(np.hypot(re, im))
            db = 20.0 * np.log10(mag) if mag > 0 else float("-inf")
            line = ("%s,%s,%04x,%d,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g" %
                    (name, epc, pc, int(r["seq"]), int(r["start"]) / TRACKS_RATE, float(r["h_re"]), float(r["h_im"]), db,
                     float(np.arctan2(im, re)), float(r["T"])))
            if quality is not None:
                line += ",%.9g,%.9g" % (float(snr_db[k]), float(margin[k]))
            if fine is not None:
                line += ",%.9g,%.9g,%.9g,%.9g,%.9g,%.9g" % (float(ff["h"][k].real), float(ff["h"][k].imag), float(ff["mag_db"][k]),
                                                            float(ff["phase_rad"][k]), float(ff["snr_db"][k]), float(ff["drift_rad_s"][k]))
            lines.append(line)
    return "\n".join(lines) + "\n"


REPAIRS_HEADER = "file,epc,pc,seq,t_s,n_flips,flips,cost,known"


def repair_flips(rec) -> List[int]:
    """rfid_repair::flips -> the indices of the reversed decisions, ascending"""
    w = int(rec["flips"]) & 0xFFFFFFFF
    return [(w >> (8 * k)) & 0xFF for k in range(int(rec["n_flips"]))]


def format_repair_summary(rows: np.ndarray) -> str:
    """One line for one trace's EPC windows before the cut-off (Context.batch_window_repairs): how many failed their CRC, how
    many of those were repaired, and how many of the repaired frames are a tag's of that trace's inventory."""
    rows = np.asarray(rows)
    failed = (rows["flags"] & 1) == 0
    fixed = rows["n_flips"] > 0
    return ("| failed EPC windows : %d  repaired : %d  of a tag in the inventory : %d\n" %
            (int(failed.sum()), int(fixed.sum()), int((fixed & (rows["entry"] >= 0)).sum())))


def format_repairs(repairs: np.ndarray, names: Sequence[str]) -> str:
    """CSV text, one line per repaired window in the order of `repairs` (Context.batch_repair_fetch: by trace, then by seq):
    file,epc,pc,seq,t_s,n_flips,flips,cost,known -- epc / pc of the REPAIRED frame, t_s = start / 400e3 as in the tracks CSV,
    flips: the reversed decisions joined by +, cost with %.9g (a binary32 value survives the round trip), known: 1 when the
    trace's inventory holds the repaired frame."""
    lines = [REPAIRS_HEADER]
    for r in repairs:
        pc, epc = frame_fields(r["frame"])
        lines.append("%s,%s,%04x,%d,%.9g,%d,%s,%.9g,%d" %
                     (names[int(r["stream"])], epc, pc, int(r["seq"]), int(r["start"]) / TRACKS_RATE, int(r["n_flips"]),
                      "+".join(map(str, repair_flips(r))), float(r["cost"]), 1 if int(r["entry"]) >= 0 else 0))
    return "\n".join(lines) + "\n"


RETUNES_HEADER = "file,epc,pc,seq,t_s,T,blf_khz,blf_off_pct,h_re,h_im,clamped,known"
RETUNE_HALF_BIT = 5.0     # samples per half-bit at the nominal link frequency: 400 ksps / (2 x 40 kHz)


def retune_fields(rows: np.ndarray) -> dict:
    """rfid_retune records -> a dict of arrays, one value per record: retuned (flags bit 1: the frame decoded again passes the
    CRC), clamped (bit 2), and in binary64 blf_khz = 200 / T, the tag's backscatter link frequency, and blf_off_pct =
    100 (5 / T - 1), its offset from the nominal 40 kHz (nan for a window that was a read: nothing was searched)."""
    rows = np.asarray(rows)
    T = rows["T"].astype(np.float64)
    searched = (rows["flags"] & 1) == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        khz = np.where(searched, 400.0 / (2.0 * T), np.nan)
        off = np.where(searched, 100.0 * (RETUNE_HALF_BIT / T - 1.0), np.nan)
    return dict(retuned=(rows["flags"] & 2) != 0, clamped=(rows["flags"] & 4) != 0, blf_khz=khz, blf_off_pct=off)


def retune_known(rows: np.ndarray, entries: np.ndarray) -> np.ndarray:
    """Host side: per record of one trace's retune rows, whether it was retuned AND the trace's inventory (`entries`: its
    capi.TAG_ENTRY_DTYPE records, Context.batch_inventory) holds the retuned frame."""
    rows = np.asarray(rows)
    have = {bytes(np.ascontiguousarray(f)) for f in np.asarray(entries)["frame"]} if len(entries) else set()
    return np.array([bool(r["flags"] & 2) and bytes(np.ascontiguousarray(r["frame"])) in have for r in rows], dtype=bool)


def format_retune(rows: np.ndarray, entries: np.ndarray) -> str:
    """One line for one trace's EPC windows before the cut-off (Context.batch_window_retunes) and its inventory: how many failed
    their CRC, how many of those pass when decoded again over the +- 4 % tolerance, how many distinct EPCs those are and how many of
    them the inventory lacks -- tags the pass did not see at all -- and the median and the extremes of their link-frequency offset."""
    rows = np.asarray(rows)
    f = retune_fields(rows)
    got = f["retuned"]
    known = retune_known(rows, entries)
    frames = {bytes(np.ascontiguousarray(r["frame"])) for r in rows[got]}
    new = {bytes(np.ascontiguousarray(r["frame"])) for r in rows[got & ~known]}
    off = f["blf_off_pct"][got]
    stat = ("median : %+.2f %%  min : %+.2f %%  max : %+.2f %%" % (float(np.median(off)), float(off.min()), float(off.max()))) if len(off) else "median : -  min : -  max : -"
    return ("| failed EPC windows : %d  retuned : %d  distinct EPCs : %d  not in the inventory : %d  BLF offset %s\n" %
            (int(((rows["flags"] & 1) == 0).sum()), int(got.sum()), len(frames), len(new), stat))


def format_retunes_csv(rows: Sequence[np.ndarray], entries: Sequence[np.ndarray], names: Sequence[str]) -> str:
    """CSV text, one line per retuned window, by trace, then by seq: file,epc,pc,seq,t_s,T,blf_khz,blf_off_pct,h_re,h_im,clamped,
    known.  rows[b]: the rfid_retune records of trace b; entries[b]: its inventory; names[b]: its file.  epc / pc of the RETUNED
    frame, t_s = start / 400e3 as in the tracks CSV, T, h_re and h_im with %.9g (a binary32 value survives the round trip), known: 1
    when the trace's inventory holds the frame."""
    lines = [RETUNES_HEADER]
    for rec, ent, name in zip(rows, entries, names):
        rec = np.asarray(rec)
        f = retune_fields(rec)
        known = retune_known(rec, ent)
        for k in np.flatnonzero(f["retuned"]):
            r = rec[k]
            pc, epc = frame_fields(r["frame"])
            lines.append("%s,%s,%04x,%d,%.9g,%.9g,%.6f,%.4f,%.9g,%.9g,%d,%d" %
                         (name, epc, pc, int(r["seq"]), int(r["start"]) / TRACKS_RATE, float(r["T"]), float(f["blf_khz"][k]),
                          float(f["blf_off_pct"][k]), float(r["h_re"]), float(r["h_im"]), int(f["clamped"][k]), int(known[k])))
    return "\n".join(lines) + "\n"


LENGTHS_HEADER = "file,epc,pc,epc_bits,seq,t_s,T,h_re,h_im,clamped"


def sized_frame_fields(rec) -> tuple:
    """One rfid_sized_frame record that was decoded (n_bits > 0) -> (PC as an int, EPC as epc_bits / 4 hex digits -- the empty string
    for a PC alone --, epc_bits = 16 x words), bits MSB first as sent."""
    n = int(rec["n_bits"])
    if n < 32:
        raise ValueError("not a decoded frame")
    w = np.asarray(rec["frame"], dtype=np.uint32)
    j = np.arange(n)
    bits = ((w[j >> 5] >> (j & 31)) & 1).astype(np.uint8)
    val = lambda b: int("".join(map(str, b.tolist())), 2) if len(b) else 0
    epc_bits = n - 32
    return val(bits[:16]), ("%0*x" % (epc_bits // 4, val(bits[16:n - 16]))) if epc_bits else "", epc_bits


def format_lengths(rows: np.ndarray) -> str:
    """One line for one trace's EPC windows before the cut-off (Context.batch_window_lengths): how many failed their CRC, how many
    of those pass when read at the length their PC announces, how many distinct EPCs those are, how many of them there are of each
    EPC length, and how many windows announce more words than the slot holds."""
    rows = np.asarray(rows)
    got = rows[(rows["flags"] & 2) != 0]
    frames = {(int(r["n_bits"]), bytes(np.ascontiguousarray(r["frame"]))) for r in got}
    by = sorted({int(r["n_bits"]) - 32 for r in got})
    hist = "  ".join("%d-bit : %d" % (b, int((got["n_bits"] == b + 32).sum())) for b in by) if by else "-"
    return ("| failed EPC windows : %d  pass at the PC's length : %d  distinct EPCs : %d  by EPC length : %s  longer than the slot : %d\n" %
            (int(((rows["flags"] & 1) == 0).sum()), len(got), len(frames), hist, int(((rows["flags"] & 8) != 0).sum())))


def format_lengths_csv(rows: Sequence[np.ndarray], names: Sequence[str], results: Sequence[np.ndarray]) -> str:
    """CSV text, one line per window that passes at its PC's length, by trace, then by seq: file,epc,pc,epc_bits,seq,t_s,T,h_re,h_im,
    clamped.  rows[b]: the rfid_sized_frame records of trace b; names[b]: its file; results[b]: its windows' capi.RESULT_DTYPE records
    in seq order -- T, h_re and h_im are the window's result's, with %.9g (a binary32 value survives the round trip); t_s =
    start / 400e3 as in the tracks CSV."""
    lines = [LENGTHS_HEADER]
    for rec, name, res in zip(rows, names, results):
        rec = np.asarray(rec)
        for r in rec[(rec["flags"] & 2) != 0]:
            pc, epc, epc_bits = sized_frame_fields(r)
            d = res[int(r["seq"])]
            lines.append("%s,%s,%04x,%d,%d,%.9g,%.9g,%.9g,%.9g,%d" %
                         (name, epc, pc, epc_bits, int(r["seq"]), int(r["start"]) / TRACKS_RATE, float(d["T"]), float(d["h_re"]),
                          float(d["h_im"]), 1 if int(r["flags"]) & 4 else 0))
    return "\n".join(lines) + "\n"


DIVERSITY_HEADER = "file,epc,pc,seq,t_s,members,h_db,margin_min,weakest,known"


def diversity_fields(rows: np.ndarray) -> dict:
    """rfid_diversity records -> a dict, one value per record: read (flags bit 0: a present member read the window itself), recovered
    (bit 1: the combined frame passes its CRC), lone (bit 2), combined (neither bit 0 nor bit 2: the members' decision values were
    added), in binary64 h_db = 10 log10 h_sq, the members' summed channel power (nan where nothing was combined), and the lists of
    member indices behind the two masks: members (present) and readers (reads)."""
    rows = np.asarray(rows)
    flags = rows["flags"]
    combined = (flags & 5) == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        h_db = np.where(combined, 10.0 * np.log10(rows["h_sq"].astype(np.float64)), np.nan)
    of = lambda mask: [m for m in range(capi.DIVERSITY_MAX_MEMBERS) if (int(mask) >> m) & 1]
    return dict(read=(flags & 1) != 0, recovered=(flags & 2) != 0, lone=(flags & 4) != 0, combined=combined, h_db=h_db,
                members=[of(p) for p in rows["present"]], readers=[of(p) for p in rows["reads"]])


def diversity_known(rows: np.ndarray, entries_of_members: Sequence[np.ndarray]) -> np.ndarray:
    """Host side: per record of one group's diversity rows, whether it was recovered AND the inventory of at least one member
    (`entries_of_members`: each member's capi.TAG_ENTRY_DTYPE records, Context.batch_inventory) holds the combined frame."""
    rows = np.asarray(rows)
    have = {bytes(np.ascontiguousarray(f)) for ent in entries_of_members for f in np.asarray(ent)["frame"]}
    return np.array([bool(r["flags"] & 2) and bytes(np.ascontiguousarray(r["frame"])) in have for r in rows], dtype=bool)


def format_diversity(rows: np.ndarray, entries_of_members: Sequence[np.ndarray]) -> str:
    """One line for one group's EPC windows before its anchor's cut-off (Context.batch_window_diversity) and its members' inventories:
    how many windows, how many at least one antenna read, how many none read, how many of those the combination recovers, how many
    distinct EPCs those are and how many of them no member's inventory holds -- tags no antenna saw at all."""
    rows = np.asarray(rows)
    f = diversity_fields(rows)
    got = f["recovered"]
    known = diversity_known(rows, entries_of_members)
    frames = {bytes(np.ascontiguousarray(r["frame"])) for r in rows[got]}
    new = {bytes(np.ascontiguousarray(r["frame"])) for r in rows[got & ~known]}
    return ("| EPC windows : %d  read by an antenna : %d  read by none : %d  recovered by combining : %d  distinct EPCs : %d  "
            "in no antenna's inventory : %d\n" % (len(rows), int(f["read"].sum()), int((~f["read"]).sum()), int(got.sum()), len(frames), len(new)))


def format_diversity_csv(rows: Sequence[np.ndarray], entries_of_members: Sequence[Sequence[np.ndarray]], names: Sequence[str]) -> str:
    """CSV text, one line per recovered window, by group, then by seq: file,epc,pc,seq,t_s,members,h_db,margin_min,weakest,known.
    rows[g]: the rfid_diversity records of group g; entries_of_members[g]: its members' inventories; names[g]: its ANCHOR's file.
    epc / pc of the COMBINED frame, t_s = start / 400e3 as in the tracks CSV (the anchor's), members: the present members' indices
    joined by +, h_db with %.4f, margin_min with %.9g (a binary32 value survives the round trip), known: 1 when a member's
    inventory holds the frame."""
    lines = [DIVERSITY_HEADER]
    for rec, ents, name in zip(rows, entries_of_members, names):
        rec = np.asarray(rec)
        f = diversity_fields(rec)
        known = diversity_known(rec, ents)
        for k in np.flatnonzero(f["recovered"]):
            r = rec[k]
            pc, epc = frame_fields(r["frame"])
            lines.append("%s,%s,%04x,%d,%.9g,%s,%.4f,%.9g,%d,%d" %
                         (name, epc, pc, int(r["seq"]), int(r["start"]) / TRACKS_RATE, "+".join(map(str, f["members"][k])),
                          float(f["h_db"][k]), float(r["margin_min"]), int(r["weakest"]), int(known[k])))
    return "\n".join(lines) + "\n"


MATCH_HEADER = "file,epc,pc,seq,t_s,rho,rho_second,diff,bit_errors,h_re,h_im,mag_db,phase_rad"
MATCH_MIN_RHO = 0.5       # the default of --match-min (match_fields says why)


def match_fields(rows: np.ndarray, min_rho: float = MATCH_MIN_RHO) -> dict:
    """rfid_match records -> a dict, one value per record: searched (a failed window that had candidates), in binary64 rho =
    score_best / sig_abs and rho_second = score_second / sig_abs (nan where there is none, or sig_abs is 0), gap = score_best -
    score_second, gap_needed = diff * sig_abs / 128, and attributed: the HOST's policy, a definition and no part of the device record.
    A window is attributed to `best` when both hold:
      threshold  rho >= min_rho.  In a window that does not hold the candidate's reply the signs of r_j are independent of the
                 pattern: rho has mean 0 and standard deviation sqrt(sum r^2) / sum |r|, for Gaussian r_j sqrt(pi / 2) / sqrt(128) =
                 0.111.  The default 0.5 lies 4.5 standard deviations out: about 3e-6 per window and candidate.
      gap        there is no second, or gap >= gap_needed.  best's and second's patterns differ on `diff` decisions, the mean |r_j| is
                 sig_abs / 128: a clean reply of best puts the two scores 2 diff mean|r| apart, a clean reply of second the negative
                 of it.  The rule asks for half of the former, diff mean|r|: the midpoint between "best's reply" and "cannot tell".
    An attribution is never a read."""
    rows = np.asarray(rows)
    searched = ((rows["flags"] & 1) == 0) & (rows["n_cand"] > 0)
    sig = rows["sig_abs"].astype(np.float64)
    sb, ss = rows["score_best"].astype(np.float64), rows["score_second"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(searched & (sig > 0), sb / sig, np.nan)
        rho_second = np.where(searched & (sig > 0) & (rows["second"] >= 0), ss / sig, np.nan)
    gap = np.where(rows["second"] >= 0, sb - ss, np.inf)
    gap_needed = np.where(rows["second"] >= 0, rows["diff"].astype(np.float64) * sig / 128.0, 0.0)
    with np.errstate(invalid="ignore"):
        attributed = searched & (rho >= float(min_rho)) & (gap >= gap_needed)
    return dict(searched=searched, rho=rho, rho_second=rho_second, gap=gap, gap_needed=gap_needed, attributed=attributed)


def _match_reads(rows: np.ndarray, results: np.ndarray) -> dict:
    """frame bytes -> the reads of that frame among one trace's rows (flags bit 0), from its result records by seq"""
    reads = {}
    for r in rows[(rows["flags"] & 1) != 0]:
        key = bytes(np.ascontiguousarray(results[int(r["seq"])]["bits"]))
        reads[key] = reads.get(key, 0) + 1
    return reads


def format_match(rows: np.ndarray, results: np.ndarray, min_rho: float = MATCH_MIN_RHO) -> str:
    """The lines for one trace's EPC windows before the cut-off (Context.batch_window_matches) and its result records by seq: how many
    windows failed, how many of those are attributed to a known tag, how many distinct tags those are; then per such tag its reads
    beside its attributed sightings, ordered by frame."""
    rows = np.asarray(rows)
    f = match_fields(rows, min_rho)
    got = rows[f["attributed"]]
    reads = _match_reads(rows, results)
    seen = {}
    for r in got:
        key = bytes(np.ascontiguousarray(r["frame"]))
        seen[key] = seen.get(key, 0) + 1
    text = ("| EPC windows : %d  failed : %d  attributed to a known tag : %d  distinct tags : %d\n" %
            (len(rows), int(((rows["flags"] & 1) == 0).sum()), len(got), len(seen)))
    for key in sorted(seen):
        pc, epc = frame_fields(np.frombuffer(key, dtype=np.uint32))
        text += "|   %s  %04x  reads : %d  attributed : %d\n" % (epc, pc, reads.get(key, 0), seen[key])
    return text


def format_match_csv(rows: Sequence[np.ndarray], names: Sequence[str], results: Sequence[np.ndarray], min_rho: float = MATCH_MIN_RHO) -> str:
    """CSV text, one line per attributed window, by trace, then by seq: file,epc,pc,seq,t_s,rho,rho_second,diff,bit_errors,h_re,h_im,
    mag_db,phase_rad.  epc / pc of best's frame, t_s = start / 400e3 as in the tracks CSV, rho with %.6f (rho_second and diff empty
    and -1 where there was one candidate), bit_errors = dist_best, h_re / h_im the window's own h_est (results[b][seq]) with %.9g, its
    magnitude in dB and its phase as in the tracks CSV: what a sighting adds to a tag's track."""
    lines = [MATCH_HEADER]
    for rec, name, res in zip(rows, names, results):
        rec = np.asarray(rec)
        f = match_fields(rec, min_rho)
        for k in np.flatnonzero(f["attributed"]):
            r = rec[k]
            d = res[int(r["seq"])]
            pc, epc = frame_fields(r["frame"])
            re, im = np.float64(d["h_re"]), np.float64(d["h_im"])
            mag = float(np.hypot(re, im))
            db = 20.0 * np.log10(mag) if mag > 0 else float("-inf")
            second = "" if int(r["second"]) < 0 else "%.6f" % float(f["rho_second"][k])
            lines.append("%s,%s,%04x,%d,%.9g,%.6f,%s,%d,%d,%.9g,%.9g,%.9g,%.9g" %
                         (name, epc, pc, int(r["seq"]), int(r["start"]) / TRACKS_RATE, float(f["rho"][k]), second, int(r["diff"]),
                          int(r["dist_best"]), float(d["h_re"]), float(d["h_im"]), db, float(np.arctan2(im, re))))
    return "\n".join(lines) + "\n"


def read_epc_list(path: str) -> np.ndarray:
    """A text file with one hex EPC per line (96 bits), optionally PC:EPC; blank lines and lines that start with # are skipped
    -> (n, 4) uint32 frames (frame_of_epc)."""
    from .context import frame_of_epc
    frames = []
    with open(path) as f:
        for ln in f:
            ln = ln.strip()
            if not ln or ln.startswith("#"):
                continue
            pc, _, epc = ln.rpartition(":")
            frames.append(frame_of_epc(epc, int(pc, 16) if pc else 0x3000))
    return np.array(frames, dtype=np.uint32).reshape(-1, 4)


STACK_HEADER = "file,epc,pc,seq,t_s,n_members,member_seqs,margin_min,weakest,known"
STACK_MIN_RHO = 0.5       # the default of --stack-min (DESIGN.md derives it)


def stack_fields(rows: np.ndarray) -> dict:
    """rfid_stack records of ONE trace, in seq order -> a dict, one value per record: read (flags bit 0), failed (not a read), stacked
    (bit 1: the window has partners and a combination was formed), passed (bit 2: the combination's CRC holds -- the acceptance
    test; rho_min only decides what is added up), members: the indices INTO rows of the record's members in ascending order, its
    own among them (empty for a read), and member_seqs: their seq."""
    rows = np.asarray(rows)
    flags = rows["flags"]
    read = (flags & 1) != 0
    where = np.flatnonzero(~read)                                  # ordinal f -> index into rows
    members = []
    for r, is_read in zip(rows, read):
        base = (int(r["ordinal"]) // capi.STACK_BLOCK) * capi.STACK_BLOCK
        members.append([] if is_read else [int(where[base + l]) for l in range(capi.STACK_BLOCK)
                                           if (int(r["member_mask"]) >> l) & 1 and base + l < len(where)])
    return dict(read=read, failed=~read, stacked=(flags & 2) != 0, passed=(flags & 4) != 0, members=members,
                member_seqs=[[int(rows[i]["seq"]) for i in m] for m in members])


def stack_known(rows: np.ndarray, entries: np.ndarray) -> np.ndarray:
    """Host side: per record of one trace's stack rows, whether its combination passes the CRC AND the trace's inventory (`entries`:
    capi.TAG_ENTRY_DTYPE records, Context.batch_inventory) holds that frame."""
    rows = np.asarray(rows)
    have = {bytes(np.ascontiguousarray(f)) for f in np.asarray(entries)["frame"]}
    return np.array([bool(r["flags"] & 4) and bytes(np.ascontiguousarray(r["frame"])) in have for r in rows], dtype=bool)


def format_stack(rows: np.ndarray, entries: np.ndarray) -> str:
    """One line for one trace's EPC windows before the cut-off (Context.batch_window_stacks) and its inventory: how many windows, how
    many failed, how many of those were stacked with partners, how many combinations pass the CRC, how many distinct EPCs those are
    and how many of them the inventory lacks -- tags the decoder did not read once."""
    rows = np.asarray(rows)
    f = stack_fields(rows)
    known = stack_known(rows, entries)
    frames = {bytes(np.ascontiguousarray(r["frame"])) for r in rows[f["passed"]]}
    new = {bytes(np.ascontiguousarray(r["frame"])) for r in rows[f["passed"] & ~known]}
    return ("| EPC windows : %d  failed : %d  stacked : %d  combinations that pass the CRC : %d  distinct EPCs : %d  "
            "not in the inventory : %d\n" % (len(rows), int(f["failed"].sum()), int(f["stacked"].sum()), int(f["passed"].sum()),
                                             len(frames), len(new)))


def format_stack_csv(rows: Sequence[np.ndarray], entries: Sequence[np.ndarray], names: Sequence[str]) -> str:
    """CSV text, one line per window whose combination passes the CRC, by trace, then by seq: file,epc,pc,seq,t_s,n_members,
    member_seqs,margin_min,weakest,known.  rows[b]: the rfid_stack records of trace b; entries[b]: its inventory; names[b]: its file.
    epc / pc of the COMBINED frame, t_s = start / 400e3 as in the tracks CSV, member_seqs: the members' seq joined by +, the window's own
    among them, margin_min with %.9g (a binary32 value survives the round trip), known: 1 when the trace's inventory holds the frame."""
    lines = [STACK_HEADER]
    for rec, ents, name in zip(rows, entries, names):
        rec = np.asarray(rec)
        f = stack_fields(rec)
        known = stack_known(rec, ents)
        for k in np.flatnonzero(f["passed"]):
            r = rec[k]
            pc, epc = frame_fields(r["frame"])
            lines.append("%s,%s,%04x,%d,%.9g,%d,%s,%.9g,%d,%d" %
                         (name, epc, pc, int(r["seq"]), int(r["start"]) / TRACKS_RATE, len(f["members"][k]),
                          "+".join(map(str, f["member_seqs"][k])), float(r["margin_min"]), int(r["weakest"]), int(known[k])))
    return "\n".join(lines) + "\n"


MOMENTS_N = 240           # RFID_MOMENTS_SAMPLES: the samples of a window its moments are taken over
SLOT_EMPTY, SLOT_SINGLE, SLOT_COLLIDED, SLOT_UNKNOWN = 0, 1, 2, -1
SCHOUTE = 2.39            # Schoute's estimate of the tags behind a collided slot of a framed-ALOHA round
SLOT_DTYPE = np.dtype([("seq", "<i4"), ("cls", "<i4"), ("answered", "<i4"), ("crc_ok", "<i4"), ("l1", "<f8"), ("l2", "<f8"),
                       ("floor", "<f8")])
SLOTS_HEADER = "file,slot,seq,t_s,class,l1_db,l2_db,floor_db,answered,crc_ok"


def moment_fields(rows: np.ndarray):
    """rfid_window_moments records -> (l1, l2), float64 arrays: the eigenvalues l1 >= l2 >= 0 of the windows' 2 x 2 scatter
    matrices, per sample.  With n = 240: cxx = sxx - sx^2 / n, cyy = syy - sy^2 / n, cxy = sxy - sx sy / n, tr = cxx + cyy,
    d = hypot(cxx - cyy, 2 cxy), l1 = (tr + d) / 2 / n, l2 = max((tr - d) / 2, 0) / n."""
    rows = np.asarray(rows)
    n = float(MOMENTS_N)
    sx, sy = rows["sx"].astype(np.float64), rows["sy"].astype(np.float64)
    cxx = rows["sxx"].astype(np.float64) - sx * sx / n
    cyy = rows["syy"].astype(np.float64) - sy * sy / n
    cxy = rows["sxy"].astype(np.float64) - sx * sy / n
    tr, d = cxx + cyy, np.hypot(cxx - cyy, 2.0 * cxy)
    return (tr + d) / 2.0 / n, np.maximum((tr - d) / 2.0, 0.0) / n


def classify_slots(rows: np.ndarray, empty_k: float = 3.0, collided_k: float = 3.0) -> np.ndarray:
    """One trace's moments (Context.batch_window_moments: every window before the cut-off, in seq order) -> one SLOT_DTYPE
    record per slot.  Slot k is rows 2k (its RN16 window) and 2k + 1 (its EPC window); a last RN16 without its EPC is left out.
    floor: the median l2 over the trace's EPC rows -- the minor eigenvalue of an EPC window is noise whether the slot was
    empty, single or collided (a floor from the RN16 windows breaks down once most slots collide).  cls: SLOT_EMPTY when the
    RN16 window's l1 <= empty_k floor, else SLOT_COLLIDED when its l2 > collided_k floor, else SLOT_SINGLE; answered: the
    EPC window's l1 > empty_k floor (somebody answered the ACK); crc_ok: of the EPC window; seq, l1, l2: the RN16 window's.
    A floor that is 0 or not finite (a noise-free trace): cls = SLOT_UNKNOWN for every slot.  The defaults are "three times
    the noise floor": at sigma = 0.03 empty slots stay below 1.93 floors and occupied ones above 22 (l1), single replies below
    1.55 and collided ones above 4.8 (l2)."""
    rows = np.asarray(rows)
    n_slots = len(rows) // 2
    out = np.zeros(n_slots, dtype=SLOT_DTYPE)
    if n_slots == 0:
        return out
    l1, l2 = moment_fields(rows[: 2 * n_slots])
    rn_l1, rn_l2, epc_l1, epc_l2 = l1[0::2], l2[0::2], l1[1::2], l2[1::2]
    floor = float(np.median(epc_l2))
    out["seq"] = rows["seq"][0: 2 * n_slots: 2]
    out["crc_ok"] = rows["flags"][1: 2 * n_slots: 2] & 1
    out["l1"], out["l2"], out["floor"] = rn_l1, rn_l2, floor
    if not (np.isfinite(floor) and floor > 0.0):
        out["cls"] = SLOT_UNKNOWN
        return out
    out["cls"] = np.where(rn_l1 <= empty_k * floor, SLOT_EMPTY, np.where(rn_l2 > collided_k * floor, SLOT_COLLIDED, SLOT_SINGLE))
    out["answered"] = epc_l1 > empty_k * floor
    return out


def estimate_population(cls, n_rounds: int) -> float:
    """Schoute's estimate of the tags in the field, per inventory round: (singles + 2.39 collided) / rounds."""
    cls = np.asarray(cls)
    if n_rounds <= 0:
        return 0.0
    return (float((cls == SLOT_SINGLE).sum()) + SCHOUTE * float((cls == SLOT_COLLIDED).sum())) / float(n_rounds)


def suggest_q(n: float) -> int:
    """The Q whose 2^Q slots per round suit n tags best: clamp(round(log2(max(n, 1))), 0, 15)."""
    return int(min(max(int(round(float(np.log2(max(float(n), 1.0))))), 0), 15))


def format_slots(slots: np.ndarray, fixed_q: int) -> str:
    """One line for one trace's slots (classify_slots): how many there are, how many were empty / single / collided, in how
    many the ACK was answered, how many gave a CRC-verified read, the efficiency (reads per slot), the estimated tags per
    round (rounds = slots / 2^Q, rounded up) and the Q that would suit them beside the Q in use."""
    slots = np.asarray(slots)
    n = len(slots)
    cls = slots["cls"]
    read = int((slots["crc_ok"] != 0).sum())
    if n and (cls == SLOT_UNKNOWN).all():
        return "| slots : %d  not classified (no noise floor)  read : %d  efficiency : %.3f\n" % (n, read, read / n)
    rounds = -(-n // (1 << int(fixed_q)))
    est = estimate_population(cls, rounds)
    return ("| slots : %d  empty : %d  single : %d  collided : %d  answered : %d  read : %d  efficiency : %.3f  "
            "tags per round : %.2f  suggested Q : %d (in use : %d)\n" %
            (n, int((cls == SLOT_EMPTY).sum()), int((cls == SLOT_SINGLE).sum()), int((cls == SLOT_COLLIDED).sum()),
             int((slots["answered"] != 0).sum()), read, (read / n) if n else 0.0, est, suggest_q(est), int(fixed_q)))


def format_slots_csv(slots: Sequence[np.ndarray], starts: Sequence[np.ndarray], names: Sequence[str]) -> str:
    """CSV text, one line per slot, by trace, then by slot: file,slot,seq,t_s,class,l1_db,l2_db,floor_db,answered,crc_ok.
    slots[b]: classify_slots of trace b; starts[b][seq]: rfid_window::start of its windows; names[b]: its file.  seq is the
    slot's RN16 window, t_s = start / 400e3 as in the tracks CSV, class one of empty / single / collided / unknown, the three
    levels 10 log10 of l1, l2 (the RN16 window's) and the floor, printed with %.9g."""
    label = {SLOT_EMPTY: "empty", SLOT_SINGLE: "single", SLOT_COLLIDED: "collided", SLOT_UNKNOWN: "unknown"}
    lines = [SLOTS_HEADER]
    with np.errstate(divide="ignore"):
        for b, (rec, name) in enumerate(zip(slots, names)):
            for k, r in enumerate(rec):
                db = [10.0 * np.log10(np.float64(r[f])) for f in ("l1", "l2", "floor")]
                lines.append("%s,%d,%d,%.9g,%s,%.9g,%.9g,%.9g,%d,%d" %
                             (name, k, int(r["seq"]), int(starts[b][int(r["seq"])]) / TRACKS_RATE, label[int(r["cls"])],
                              float(db[0]), float(db[1]), float(db[2]), int(r["answered"]), int(r["crc_ok"])))
    return "\n".join(lines) + "\n"


COLLISIONS_HEADER = "file,slot,seq,t_s,rn16_a,rn16_b,ha_re,ha_im,hb_re,hb_im,ratio_db,fit,order,decoded"
COLLISION_ORDER_K = 0.0477        # fit above which a collided slot held three or more tags (classify_collisions)
COLLISION_SLOT_DTYPE = np.dtype([("slot", "<i4"), ("seq", "<i4"), ("order", "<i4"), ("rn16_a", "<i4"), ("rn16_b", "<i4"),
                                 ("ha", "<c16"), ("hb", "<c16"), ("ratio_db", "<f8"), ("fit", "<f8"), ("decoded", "U1")])


def collision_fields(rows: np.ndarray) -> dict:
    """rfid_collision records -> a dict of arrays, one value per record, in binary64: ha_db / hb_db = 20 log10 of |hA| / |hB| (the
    stronger and the weaker tag, in the units of h_est), ratio_db = hb_db - ha_db (<= 0), phase_rad = arg(hB conj(hA)), fit =
    resid / sum_sq (nan when sum_sq == 0): how much of the window's energy four points do NOT explain, and decoded: "a" when the
    decoder's own RN16 is the stronger tag's, "b" when the weaker's (and not also the stronger's), "-" when neither's."""
    rows = np.asarray(rows)
    ha = rows["ha_re"].astype(np.float64) + 1j * rows["ha_im"].astype(np.float64)
    hb = rows["hb_re"].astype(np.float64) + 1j * rows["hb_im"].astype(np.float64)
    resid, sum_sq = rows["resid"].astype(np.float64), rows["sum_sq"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ha_db, hb_db = 20.0 * np.log10(np.abs(ha)), 20.0 * np.log10(np.abs(hb))
        fit = np.where(sum_sq != 0.0, resid / sum_sq, np.nan)
        ratio = hb_db - ha_db
    decoded = np.where((rows["flags"] & 1) != 0, "a", np.where((rows["flags"] & 2) != 0, "b", "-"))
    return dict(ha_db=ha_db, hb_db=hb_db, ratio_db=ratio, phase_rad=np.angle(hb * np.conj(ha)), fit=fit, decoded=decoded)


def classify_collisions(rows: np.ndarray, slots: np.ndarray, order_k: float = COLLISION_ORDER_K) -> np.ndarray:
    """One trace's collision rows (Context.batch_window_collisions: row k is the RN16 window of slot k) and its slots
    (classify_slots of the same pass) -> one COLLISION_SLOT_DTYPE record per slot whose class is SLOT_COLLIDED: the two handles and
    channels, their ratio, fit and decoded (collision_fields), and order = 2 when fit <= order_k (two tags: rn16_a and rn16_b are
    theirs), else 3 -- three or more tags, which four points do not explain; the handles are then of no use.  On the reference's
    records of the test traces (sigma = 0.03; the ragged batch and the crowded trace of tests/collide_suite.py and
    tests/test_gpu_collide.py) the fit of two-tag slots stays at or below 0.0151 and that of slots with three or more tags at or
    above 0.150: the default lies between them, at their geometric mean."""
    rows, slots = np.asarray(rows), np.asarray(slots)
    n = min(len(rows), len(slots))
    pick = np.flatnonzero(slots["cls"][:n] == SLOT_COLLIDED)
    out = np.zeros(len(pick), dtype=COLLISION_SLOT_DTYPE)
    f = collision_fields(rows[pick])
    out["slot"], out["seq"] = pick, rows["seq"][pick]
    out["rn16_a"], out["rn16_b"] = rows["rn16_a"][pick], rows["rn16_b"][pick]
    out["ha"] = rows["ha_re"][pick].astype(np.float64) + 1j * rows["ha_im"][pick].astype(np.float64)
    out["hb"] = rows["hb_re"][pick].astype(np.float64) + 1j * rows["hb_im"][pick].astype(np.float64)
    out["ratio_db"], out["fit"], out["decoded"] = f["ratio_db"], f["fit"], f["decoded"]
    out["order"] = np.where(f["fit"] <= order_k, 2, 3)
    return out


def format_collisions(collided: np.ndarray) -> str:
    """One line for one trace's collided slots (classify_collisions): how many there are, how many were resolved as two tags and how
    many held more; among the resolved ones, whether the RN16 the decoder handed to the ACK was the stronger tag's, the weaker's
    or neither's, and the median |hB| / |hA| in dB."""
    collided = np.asarray(collided)
    two = collided[collided["order"] == 2]
    med = ("%.2f" % float(np.median(two["ratio_db"]))) if len(two) else "-"
    return ("| collided slots : %d  two tags : %d  more : %d  decoder's RN16 the stronger tag's : %d  the weaker's : %d  neither's : %d  "
            "median |hB|/|hA| dB : %s\n" %
            (len(collided), len(two), len(collided) - len(two), int((two["decoded"] == "a").sum()), int((two["decoded"] == "b").sum()),
             int((two["decoded"] == "-").sum()), med))


def format_collisions_csv(collided: Sequence[np.ndarray], starts: Sequence[np.ndarray], names: Sequence[str]) -> str:
    """CSV text, one line per collided slot, by trace, then by slot: file,slot,seq,t_s,rn16_a,rn16_b,ha_re,ha_im,hb_re,hb_im,
    ratio_db,fit,order,decoded.  collided[b]: classify_collisions of trace b; starts[b][seq]: rfid_window::start of its windows;
    names[b]: its file.  seq is the slot's RN16 window, t_s = start / 400e3 as in the tracks CSV, the handles four hex digits,
    floats with %.9g (a binary32 value survives the round trip), order 2 or 3 (three or more), decoded a, b or -."""
    lines = [COLLISIONS_HEADER]
    for b, (rec, name) in enumerate(zip(collided, names)):
        for r in rec:
            lines.append("%s,%d,%d,%.9g,%04x,%04x,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%d,%s" %
                         (name, int(r["slot"]), int(r["seq"]), int(starts[b][int(r["seq"])]) / TRACKS_RATE, int(r["rn16_a"]),
                          int(r["rn16_b"]), r["ha"].real, r["ha"].imag, r["hb"].real, r["hb"].imag, float(r["ratio_db"]),
                          float(r["fit"]), int(r["order"]), str(r["decoded"])))
    return "\n".join(lines) + "\n"


COMMAND_NAMES = ("none", "query", "queryrep", "ack", "nak", "queryadjust", "unknown")   # by RFID_CMD_*
SAMPLE_US = 2.5           # one sample behind the decimation of a 2 Msps trace (400 ksps)
COMMAND_FIELDS_DTYPE = np.dtype([("seq", "<i4"), ("name", "U11"), ("q", "<i4"), ("rn16", "<i4"), ("crc5_ok", "<i4"), ("ack_echo", "<i4"),
                                 ("rtcal_us", "<f8"), ("trcal_us", "<f8"), ("t1_us", "<f8")])
COMMANDS_HEADER = "file,seq,t_s,cmd,n_bits,bits,q,rn16,crc5_ok,ack_echo,rtcal_us,trcal_us,t1_us"


def command_bits(rec) -> str:
    """rfid_command::bits as sent: the first min(n_bits, 32) data bits, the first one sent leftmost"""
    w = int(rec["bits"]) & 0xFFFFFFFF
    return "".join(str((w >> k) & 1) for k in range(min(max(int(rec["n_bits"]), 0), 32)))


def command_fields(rows: np.ndarray) -> np.ndarray:
    """One trace's rfid_command records (Context.batch_window_commands) -> one COMMAND_FIELDS_DTYPE record per window: name
    (COMMAND_NAMES); q: the Q a Query announces (data bits 13..16, MSB first), -1 for any other command; rn16: the RN16 an ACK
    carries (data bits 2..17, MSB first, as the tag sent it), -1 otherwise; crc5_ok: a Query's CRC-5 holds (-1: not a Query);
    ack_echo: the ACK carries the RN16 decoded in the window before (-1: not an ACK); rtcal / trcal in us at 2.5 us per sample
    (nan when absent); t1_us: from the command's last rising edge to the window's first sample (nan without a command)."""
    rows = np.asarray(rows)
    out = np.zeros(len(rows), dtype=COMMAND_FIELDS_DTYPE)
    for k, r in enumerate(rows):
        cmd, w, flags = int(r["cmd"]), int(r["bits"]) & 0xFFFFFFFF, int(r["flags"])
        msb_first = lambda lo, n: sum(((w >> (lo + i)) & 1) << (n - 1 - i) for i in range(n))
        o = out[k]
        o["seq"] = int(r["seq"])
        o["name"] = COMMAND_NAMES[cmd] if 0 <= cmd < len(COMMAND_NAMES) else "unknown"
        o["q"] = msb_first(13, 4) if cmd == CMD_QUERY else -1
        o["rn16"] = msb_first(2, 16) if cmd == CMD_ACK else -1
        o["crc5_ok"] = ((flags >> 1) & 1) if cmd == CMD_QUERY else -1
        o["ack_echo"] = ((flags >> 2) & 1) if cmd == CMD_ACK else -1
        o["rtcal_us"] = SAMPLE_US * int(r["rtcal"]) if int(r["rtcal"]) > 0 else np.nan
        o["trcal_us"] = SAMPLE_US * int(r["trcal"]) if int(r["trcal"]) > 0 else np.nan
        o["t1_us"] = SAMPLE_US * (CMD_SPAN - int(r["end"])) if int(r["n_syms"]) > 0 else np.nan
    return out


def format_commands(rows: np.ndarray) -> str:
    """One line for one trace's commands (Context.batch_window_commands): how many windows were opened by a Query, a QueryRep,
    an ACK, another command or none that could be found; the Q values the Queries announced; the Queries whose CRC-5 failed;
    how many ACKs echo the RN16 decoded in the window before them; the median RTcal, TRcal and T1 in us."""
    f = command_fields(rows)
    name = f["name"]
    count = lambda n: int((name == n).sum())
    nq, nr, na, nn = count("query"), count("queryrep"), count("ack"), count("none")
    qs = sorted(set(int(q) for q in f["q"][name == "query"]))
    med = lambda v: ("%.1f" % float(np.median(v[~np.isnan(v)]))) if (~np.isnan(v)).any() else "-"
    return ("| commands : %d  query : %d  queryrep : %d  ack : %d  other : %d  none : %d  Q : %s  failed CRC-5 : %d  "
            "ACKs echoing the decoded RN16 : %d of %d  median RTcal us : %s  TRcal us : %s  T1 us : %s\n" %
            (len(f), nq, nr, na, len(f) - nq - nr - na - nn, nn, ("{" + ",".join(map(str, qs)) + "}") if qs else "-",
             int((f["crc5_ok"] == 0).sum()), int((f["ack_echo"] == 1).sum()), na, med(f["rtcal_us"]), med(f["trcal_us"]), med(f["t1_us"])))


def format_commands_csv(rows: Sequence[np.ndarray], starts: Sequence[np.ndarray], names: Sequence[str]) -> str:
    """CSV text, one line per window, by trace, then by seq: file,seq,t_s,cmd,n_bits,bits,q,rn16,crc5_ok,ack_echo,rtcal_us,
    trcal_us,t1_us.  rows[b]: the rfid_command records of trace b; starts[b][seq]: rfid_window::start of its windows; names[b]:
    its file.  t_s = start / 400e3 as in the tracks CSV; bits as sent (command_bits); rn16 as four hex digits; a field that
    does not apply to the command is empty."""
    lines = [COMMANDS_HEADER]
    opt = lambda v, fmt: "" if (v < 0 or v != v) else fmt % v
    for b, (rec, name) in enumerate(zip(rows, names)):
        for r, f in zip(rec, command_fields(rec)):
            lines.append("%s,%d,%.9g,%s,%d,%s,%s,%s,%s,%s,%s,%s,%s" %
                         (name, int(r["seq"]), int(starts[b][int(r["seq"])]) / TRACKS_RATE, f["name"], int(r["n_bits"]), command_bits(r),
                          opt(int(f["q"]), "%d"), opt(int(f["rn16"]), "%04x"), opt(int(f["crc5_ok"]), "%d"), opt(int(f["ack_echo"]), "%d"),
                          opt(float(f["rtcal_us"]), "%.1f"), opt(float(f["trcal_us"]), "%.1f"), opt(float(f["t1_us"]), "%.1f")))
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    """python -m rfid.batch [--device N] [--fixed-q Q] [--inventory [--max-tags N]] [--tracks OUT.csv] [--quality] [--repair OUT.csv] [--slots OUT.csv] [--commands OUT.csv] [--fine] [--retune OUT.csv] [--collisions OUT.csv] [--lengths OUT.csv] [--antennas M --diversity OUT.csv] [--match OUT.csv [--match-list EPCS.txt] [--match-min RHO]] [--stack OUT.csv [--stack-min RHO]] TRACE_FILE...  -- decode recorded traces in one batched pass."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m rfid.batch", description=main.__doc__)
    ap.add_argument("files", nargs="+")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fixed-q", type=int, default=0)
    ap.add_argument("--max-queries", type=int, default=1000)
    ap.add_argument("--inventory", action="store_true", help="list the distinct EPCs of every trace (built on the device)")
    ap.add_argument("--max-tags", type=int, default=64, help="distinct EPCs per trace the inventory has room for (1..512)")
    ap.add_argument("--tracks", metavar="OUT.csv", default=None,
                    help="write every tag's reads in time order (t_s, h_est, T) to this CSV file; implies --inventory")
    ap.add_argument("--quality", action="store_true",
                    help="one line per file on the SNR and decision margin of its EPC windows (built on the device); with --tracks the "
                         "CSV gains the columns snr_db,margin")
    ap.add_argument("--repair", metavar="OUT.csv", default=None,
                    help="search the CRC-failed EPC windows for one to three weak decisions whose reversal makes the frame pass "
                         "(built on the device); one line per file, the repaired windows to this CSV file; implies --inventory")
    ap.add_argument("--slots", metavar="OUT.csv", default=None,
                    help="classify every slot as empty, single or collided from the second-order moments of its windows (built "
                         "on the device); one line per file, the slots to this CSV file")
    ap.add_argument("--commands", metavar="OUT.csv", default=None,
                    help="decode the reader's own PIE command in front of every window (built on the device): which command, "
                         "which Q, which RN16 was ACKed and whether it is the one decoded; one line per file, the commands to "
                         "this CSV file")
    ap.add_argument("--fine", action="store_true",
                    help="the data-aided channel estimate of every EPC window, from all 256 half-bit samples of its frame (built on "
                         "the device); one line per file, and with --tracks the CSV gains the columns "
                         "hd_re,hd_im,hd_mag_db,hd_phase_rad,hd_snr_db,drift_rad_s")
    ap.add_argument("--retune", metavar="OUT.csv", default=None,
                    help="decode the CRC-failed EPC windows again with the half-bit period searched over the +- 4 %% Gen2 allows a "
                         "tag's link frequency (built on the device): finds tags the decoder's +- 1 %% never reads; one line per "
                         "file, the retuned windows to this CSV file; implies --inventory")
    ap.add_argument("--collisions", metavar="OUT.csv", default=None,
                    help="separate the two RN16s and the two channels of every collided slot (built on the device): which handles "
                         "were on the air, how strong the two tags were, whether the decoder's RN16 was one of them, and whether "
                         "more than two tags collided; one line per file, the collided slots to this CSV file; classifies the slots "
                         "as --slots does, without its line and CSV")
    ap.add_argument("--lengths", metavar="OUT.csv", default=None,
                    help="read the CRC-failed EPC windows again at the length their own PC word announces (built on the device): "
                         "finds tags whose EPC is not the 96 bits the decoder takes every reply for; one line per file, the windows "
                         "that pass to this CSV file")
    ap.add_argument("--diversity", metavar="OUT.csv", default=None,
                    help="combine the EPC windows of traces recorded together -- the receive antennas of one reader session -- before "
                         "the sign is taken (built on the device): reads tags too weak for every antenna alone; one line per group, "
                         "the recovered windows to this CSV file; implies --inventory")
    ap.add_argument("--antennas", metavar="M", type=int, default=2,
                    help="with --diversity: the files are given capture by capture, each capture's M antennas in order (2..8, "
                         "default 2); the first of each is the anchor")
    ap.add_argument("--match", metavar="OUT.csv", default=None,
                    help="correlate the CRC-failed EPC windows against the replies of known tags (built on the device): finds "
                         "sightings of tags too weak to decode; per file the failed windows, how many are attributed, how many "
                         "distinct tags those are and each one's reads beside its sightings, the attributed windows to this CSV "
                         "file; without --match-list the known tags are each file's own inventory (implies --inventory)")
    ap.add_argument("--match-list", metavar="EPCS.txt", default=None,
                    help="with --match: the known tags, one hex EPC per line, optionally PC:EPC (default PC 3000), up to %d"
                         % capi.MATCH_MAX_LIST)
    ap.add_argument("--match-min", metavar="RHO", type=float, default=MATCH_MIN_RHO,
                    help="with --match: the least score / sum |r| of an attribution (default %.1f)" % MATCH_MIN_RHO)
    ap.add_argument("--stack", metavar="OUT.csv", default=None,
                    help="add up the CRC-failed EPC windows of a file that hold the same frame (found by the correlation of their "
                         "decision values, built on the device): finds tags too weak in every round that nobody knows; per file the "
                         "failed windows, how many were stacked, how many combinations pass the CRC, how many distinct EPCs those "
                         "are and how many the inventory lacks, the windows whose combination passes to this CSV file (implies "
                         "--inventory, for the known column only)")
    ap.add_argument("--stack-min", metavar="RHO", type=float, default=STACK_MIN_RHO,
                    help="with --stack: the least correlation s / a of two windows that are added up, above 0 and at most 1 "
                         "(default %.1f); the CRC decides what is a frame" % STACK_MIN_RHO)
    args = ap.parse_args(argv)
    if args.stack and not 0.0 < args.stack_min <= 1.0:
        ap.error("--stack-min: above 0 and at most 1")
    match_list = None
    if args.match_list:
        if not args.match:
            ap.error("--match-list goes with --match OUT.csv")
        match_list = read_epc_list(args.match_list)
        if not 1 <= len(match_list) <= capi.MATCH_MAX_LIST:
            ap.error("--match-list: 1 to %d EPCs" % capi.MATCH_MAX_LIST)
    if args.diversity and (not 2 <= args.antennas <= capi.DIVERSITY_MAX_MEMBERS or len(args.files) % args.antennas):
        ap.error("--diversity: the files must be whole captures of --antennas M = 2..%d files each" % capi.DIVERSITY_MAX_MEMBERS)
    if args.tracks or args.repair or args.retune or args.diversity or args.stack or (args.match and match_list is None):
        args.inventory = True
    dec = BatchDecoder(device=args.device, fixed_q=args.fixed_q, max_num_queries=args.max_queries)
    try:
        timing = {}
        stats, windows, results, _ = dec.decode_files(args.files, timing=timing, inventory=args.inventory, max_tags=args.max_tags,
                                            tracks=bool(args.tracks), quality=args.quality, repair=bool(args.repair),
                                            slots=bool(args.slots), commands=bool(args.commands), fine=args.fine,
                                            retune=bool(args.retune), collisions=bool(args.collisions),
                                            lengths=bool(args.lengths), diversity=args.antennas if args.diversity else 0,
                                            match=bool(args.match), match_list=match_list,
                                            stack=args.stack_min if args.stack else 0.0)
        collided = ([classify_collisions(c, classify_slots(m)) for c, m in zip(dec.last_collisions, dec.last_slots)]
                    if args.collisions else None)
        by_seq = [results[windows["stream"] == b] for b in range(len(args.files))] if args.match else None   # (ordered by seq)
        per_trace = lambda entries, counts: np.split(entries, np.cumsum(counts)[:-1]) if len(counts) else []
        for i, (path, row) in enumerate(zip(args.files, stats)):
            print(path)
            print(format_results(row), end="")
            if args.quality:
                print(format_quality(dec.ctx.batch_window_quality(i)), end="")
            if args.repair:
                print(format_repair_summary(dec.ctx.batch_window_repairs(i)), end="")
            if args.slots:
                print(format_slots(classify_slots(dec.last_slots[i]), args.fixed_q), end="")
            if args.commands:
                print(format_commands(dec.last_commands[i]), end="")
            if args.fine:
                print(format_fine(dec.ctx.batch_window_fine(i)), end="")
            if args.retune:
                print(format_retune(dec.last_retunes[i], per_trace(*dec.last_inventory)[i]), end="")
            if args.collisions:
                print(format_collisions(collided[i]), end="")
            if args.lengths:
                print(format_lengths(dec.last_lengths[i]), end="")
            if args.match:
                print(format_match(dec.last_matches[i], by_seq[i], args.match_min), end="")
            if args.stack:
                print(format_stack(dec.last_stacks[i], per_trace(*dec.last_inventory)[i]), end="")
            if args.diversity and i % args.antennas == 0:           # (the group's line stands with its anchor)
                print(format_diversity(dec.last_diversity[i // args.antennas], per_trace(*dec.last_inventory)[i:i + args.antennas]), end="")
        print("%d traces, %.1f M raw samples: %.3f s (host->HBM %.3f s, GPU pass %.4f s)" %
              (len(args.files), timing["raw_samples"] / 1e6, timing["total_s"], timing["h2d_s"], timing["gpu_s"]))
        if args.inventory:
            entries, counts = dec.last_inventory
            k = 0
            for path, c in zip(args.files, counts):
                print("%s: %d tags" % (path, int(c)))
                print(format_inventory(entries[k:k + int(c)]), end="")
                k += int(c)
            merged = merge_inventory(entries)
            print("all traces: %d tags" % len(merged))
            print(format_inventory(merged), end="")
        if args.tracks:
            reads, offsets = dec.last_tracks
            with open(args.tracks, "w") as f:
                f.write(format_tracks(dec.last_inventory[0], reads, offsets, args.files, dec.last_quality if args.quality else None,
                                      dec.last_fine if args.fine else None))
        if args.repair:
            with open(args.repair, "w") as f:
                f.write(format_repairs(dec.last_repairs, args.files))
        if args.slots:
            starts = [windows["start"][windows["stream"] == b] for b in range(len(args.files))]     # (ordered by seq)
            with open(args.slots, "w") as f:
                f.write(format_slots_csv([classify_slots(m) for m in dec.last_slots], starts, args.files))
        if args.retune:
            with open(args.retune, "w") as f:
                f.write(format_retunes_csv(dec.last_retunes, per_trace(*dec.last_inventory), args.files))
        if args.collisions:
            starts = [windows["start"][windows["stream"] == b] for b in range(len(args.files))]     # (ordered by seq)
            with open(args.collisions, "w") as f:
                f.write(format_collisions_csv(collided, starts, args.files))
        if args.lengths:
            by_seq = [results[windows["stream"] == b] for b in range(len(args.files))]              # (ordered by seq)
            with open(args.lengths, "w") as f:
                f.write(format_lengths_csv(dec.last_lengths, args.files, by_seq))
        if args.diversity:
            ents = per_trace(*dec.last_inventory)
            with open(args.diversity, "w") as f:
                f.write(format_diversity_csv(dec.last_diversity, [ents[i:i + args.antennas] for i in range(0, len(args.files), args.antennas)],
                                             args.files[::args.antennas]))
        if args.match:
            with open(args.match, "w") as f:
                f.write(format_match_csv(dec.last_matches, args.files, by_seq, args.match_min))
        if args.stack:
            with open(args.stack, "w") as f:
                f.write(format_stack_csv(dec.last_stacks, per_trace(*dec.last_inventory), args.files))
        if args.commands:
            starts = [windows["start"][windows["stream"] == b] for b in range(len(args.files))]     # (ordered by seq)
            with open(args.commands, "w") as f:
                f.write(format_commands_csv(dec.last_commands, starts, args.files))
    finally:
        dec.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

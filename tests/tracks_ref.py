"""The tracks a pass must report (rfid_batch_tracks: every tag's reads in time order), worked out in numpy from the ORACLE's
per-window dumps and window openings alone (shared by tests/test_tracks_emu.py and tests/test_gpu_tracks.py); builds on
tests/inventory_ref.py.  A dump's position is its window's seq; Result.open_idx[seq] is what tests/parity.py equates with
rfid_window::start."""
import numpy as np

import inventory_ref as inv
from rfid import _capi as capi


def expected(dumps: np.ndarray, open_idx: np.ndarray, stream: int = 0):
    """oracle dumps + openings of one trace -> (entries, reads ordered by (entry, seq), reads before each entry [len(entries) + 1])"""
    ent = inv.expected(dumps, stream)
    seq = np.flatnonzero((dumps["type"] == 1) & (dumps["crc_ok"] == 1))
    reads = np.zeros(len(seq), dtype=capi.TAG_READ_DTYPE)
    if len(seq) == 0:
        return ent, reads, np.zeros(1, dtype=np.int64)
    which = {bytes(f): i for i, f in enumerate(np.ascontiguousarray(ent["frame"]))}
    entry = np.array([which[bytes(f)] for f in inv.pack_frames(dumps["bits"][seq])], dtype=np.int64)
    order = np.lexsort((seq, entry))                        # by entry, then by seq (both exact integers: a total order)
    seq, entry = seq[order], entry[order]
    reads["stream"], reads["entry"], reads["seq"] = stream, entry, seq
    reads["start"] = np.asarray(open_idx)[seq]
    h = np.ascontiguousarray(dumps["h_est"][seq]).astype(np.float32)
    reads["h_re"], reads["h_im"] = h[:, 0], h[:, 1]
    reads["T"], reads["index"] = dumps["T"][seq], dumps["index"][seq]
    off = np.concatenate([[0], np.cumsum(np.bincount(entry, minlength=len(ent)))]).astype(np.int64)
    return ent, reads, off


def expected_batch(results):
    """oracle Results of the traces -> (entries, per-trace entry counts, reads, offsets aligned with the entries)"""
    ents, reads, offs, base = [], [], [np.zeros(1, dtype=np.int64)], 0
    for s, o in enumerate(results):
        e, r, off = expected(o.dumps, o.open_idx, s)
        ents.append(e); reads.append(r); offs.append(off[1:] + base)
        base += len(r)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    return (cat(ents, capi.TAG_ENTRY_DTYPE), np.array([len(e) for e in ents], dtype=np.int32), cat(reads, capi.TAG_READ_DTYPE),
            np.concatenate(offs))


def expected_tables(res, wcount, n_windows_used, start, max_tags: int, slots: int) -> dict:
    """a crafted result table res[n][wmax] with its counts, cut-offs and window starts -> everything the inventory and the tracks
    of that table must report, with the limits the kernels have on top (inv.fits): per-trace entries (`per`), counts, overflow,
    head = [entries in all, the first overflowed trace or inv.NO_TRACE], the entries' offsets per trace, the packed entries, the
    reads' bases per trace, the reads in all, the reads' offsets aligned with the packed entries (+ 1), the reads"""
    n = len(res)
    per, reads, offs = [], [], []
    counts, over = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    base = np.zeros(n, dtype=np.int32)
    total = 0
    for s in range(n):
        e, r, off = expected(inv.dumps_of_table(res[s], wcount[s], n_windows_used[s]), start[s], s)
        if not inv.fits(len(e), max_tags, slots):
            over[s] = 1
            e, r, off = e[:0], r[:0], off[:1]
        per.append(e)
        counts[s] = len(e)
        base[s] = total
        reads.append(r)
        offs.append(off[:-1] + total)
        total += len(r)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    first_over = np.flatnonzero(over)
    return dict(per=per, counts=counts, overflow=over,
                head=np.array([counts.sum(), first_over[0] if len(first_over) else inv.NO_TRACE], dtype=np.int32),
                ent_off=(np.cumsum(counts) - counts).astype(np.int32), packed=cat(per, capi.TAG_ENTRY_DTYPE), base=base,
                reads_head=np.array([total], dtype=np.int32),
                offsets=np.concatenate(offs + [np.array([total], dtype=np.int64)]).astype(np.int64), reads=cat(reads, capi.TAG_READ_DTYPE))


def assert_equal(got, got_off, want, want_off, what="") -> None:
    """exact: integers equal, floats by bit pattern, then the bytes of the whole arrays"""
    assert len(got) == len(want), (what, len(got), len(want))
    for name in capi.TAG_READ_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (what, name, len(bad), bad[:8], a[bad[:8]], b[bad[:8]])
    assert got.tobytes() == want.tobytes(), what
    assert np.asarray(got_off).dtype == np.int64 and np.array_equal(got_off, want_off), (what, got_off, want_off)


def cross_check(reads, offsets, entries, counts, stats) -> None:
    """against the pass's own inventory and statistics"""
    assert len(offsets) == len(entries) + 1 and offsets[0] == 0 and offsets[-1] == len(reads)
    assert np.array_equal(np.diff(offsets), entries["reads"])
    local = np.concatenate([np.arange(c) for c in counts]) if len(counts) else np.zeros(0, dtype=np.int64)
    for i, e in enumerate(entries):
        r = reads[offsets[i]:offsets[i + 1]]
        assert (r["stream"] == e["stream"]).all() and (r["entry"] == local[i]).all(), i
        assert r["seq"][0] == e["first_seq"] and r["seq"][-1] == e["last_seq"], i
        assert (np.diff(r["seq"]) > 0).all() and (r["seq"] & 1).all(), i
        assert (np.diff(r["start"]) > 0).all(), i
        b = r[r["seq"] == e["best_seq"]]
        assert len(b) == 1 and b["h_re"].view(np.uint32)[0] == e["best_h_re"].view(np.uint32) \
            and b["h_im"].view(np.uint32)[0] == e["best_h_im"].view(np.uint32), i
    assert len(reads) == int(sum(int(stats[s]["n_epc_correct"]) for s in range(len(counts))))

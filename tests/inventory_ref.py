"""The inventory a pass must report, worked out in numpy from the ORACLE's per-window dumps alone (shared by
tests/test_inventory_emu.py and tests/test_gpu_inventory.py).  The oracle stops dumping at the TERMINATED cut-off
(gate_impl.cc:101-109), so every EPC dump with a verified CRC is a read that tag_reads[] counts; a dump's position is its
window's seq."""
import numpy as np

from rfid import _capi as capi


def pack_frames(bits: np.ndarray) -> np.ndarray:
    """[n][128] 0/1 -> [n][4] uint32, frame bit j at word j >> 5, bit j & 31 (rfid_decode_result::bits)"""
    b = np.asarray(bits, dtype=np.uint64).reshape(-1, 4, 32)
    return (b << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


# the fields of the oracle's dumps that expected() here and tests/tracks_ref.py's read
TABLE_DUMP_DTYPE = np.dtype([("type", "<i4"), ("index", "<i4"), ("h_est", "<f4", (2,)), ("T", "<f4"), ("bits", "u1", (128,)),
                             ("crc_ok", "<i4"), ("tag_id", "<i4")])
NO_TRACE = 2 ** 31 - 1      # the head's second word when no trace overflowed


def dumps_of_table(res: np.ndarray, wcount: int, n_windows_used: int) -> np.ndarray:
    """one row of a result table (capi.RESULT_DTYPE records, crafted or the library's own) -> the dumps-shaped array expected()
    takes: the records before min(wcount, n_windows_used), the bits unpacked from bits[4].  Fields are copied, floats bit for bit"""
    nw = max(0, min(int(wcount), int(n_windows_used), len(res)))
    r = res[:nw]
    d = np.zeros(nw, dtype=TABLE_DUMP_DTYPE)
    for f in ("type", "index", "T", "crc_ok", "tag_id"):
        d[f] = r[f]
    d["h_est"][:, 0], d["h_est"][:, 1] = r["h_re"], r["h_im"]
    d["bits"] = ((r["bits"][:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(nw, 128)
    return d


def fits(n_entries: int, max_tags: int, slots: int) -> bool:
    """the limits the kernels have on top: a trace with more distinct frames than max_tags, or than the table has slots, lists
    nothing (count 0, overflow 1, no reads)"""
    return n_entries <= max_tags and n_entries <= slots


def expected(dumps: np.ndarray, stream: int = 0) -> np.ndarray:
    """oracle dumps of one trace -> its rfid_tag_entry records, ordered by first_seq"""
    seq = np.flatnonzero((dumps["type"] == 1) & (dumps["crc_ok"] == 1))
    out = np.zeros(0, dtype=capi.TAG_ENTRY_DTYPE)
    if len(seq) == 0:
        return out
    frames = pack_frames(dumps["bits"][seq])
    h = np.ascontiguousarray(dumps["h_est"][seq]).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):      # (crafted tables: norms that overflow to +inf or underflow to 0)
        norm = h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]      # binary32: two products, one sum, each rounded
    assert norm.dtype == np.float32
    rows = []
    seen = {}
    for i, f in enumerate(map(bytes, frames)):
        seen.setdefault(f, []).append(i)
    for f, idx in seen.items():                            # (insertion order = order of the first reads)
        idx = np.array(idx)
        best = idx[np.flatnonzero(norm[idx] == norm[idx].max())[0]]      # earliest among the strongest
        e = np.zeros(1, dtype=capi.TAG_ENTRY_DTYPE)[0]
        e["stream"], e["reads"], e["frame"] = stream, len(idx), frames[idx[0]]
        e["first_seq"], e["last_seq"], e["best_seq"] = seq[idx[0]], seq[idx[-1]], seq[best]
        e["best_h_re"], e["best_h_im"] = h[best, 0], h[best, 1]
        e["tag_id"] = dumps["tag_id"][seq[idx[0]]]
        rows.append(e)
    return np.array(rows, dtype=capi.TAG_ENTRY_DTYPE)


def expected_batch(dumps_per_trace) -> tuple:
    per = [expected(d, s) for s, d in enumerate(dumps_per_trace)]
    return np.concatenate(per) if per else np.zeros(0, dtype=capi.TAG_ENTRY_DTYPE), np.array([len(p) for p in per], dtype=np.int32)


def assert_equal(got, counts, want, want_counts, what="") -> None:
    """exact: integers, frame words, and best_h_* by bit pattern"""
    assert np.array_equal(np.asarray(counts), want_counts), (what, counts, want_counts)
    assert len(got) == len(want), (what, len(got), len(want))
    for name in capi.TAG_ENTRY_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (what, name, a, b)
    assert got.tobytes() == want.tobytes(), what


def cross_check(entries, counts, stats) -> None:
    """against the pass's own one-byte statistics: sum(reads | tag_id == t) == tag_reads[t], sum(reads) == n_epc_correct,
    entries of a trace sorted by first_seq"""
    k = 0
    for s, c in enumerate(counts):
        e = entries[k:k + c]
        k += c
        assert (e["stream"] == s).all()
        assert (np.diff(e["first_seq"]) > 0).all(), (s, e["first_seq"])
        assert (e["first_seq"] <= e["best_seq"]).all() and (e["best_seq"] <= e["last_seq"]).all()
        hist = np.bincount(e["tag_id"], weights=e["reads"], minlength=256).astype(np.int64)
        assert np.array_equal(hist, stats[s]["tag_reads"]), s
        assert int(e["reads"].sum()) == int(stats[s]["n_epc_correct"]), s
    assert k == len(entries)

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


def expected(dumps: np.ndarray, stream: int = 0) -> np.ndarray:
    """oracle dumps of one trace -> its rfid_tag_entry records, ordered by first_seq"""
    seq = np.flatnonzero((dumps["type"] == 1) & (dumps["crc_ok"] == 1))
    out = np.zeros(0, dtype=capi.TAG_ENTRY_DTYPE)
    if len(seq) == 0:
        return out
    frames = pack_frames(dumps["bits"][seq])
    h = np.ascontiguousarray(dumps["h_est"][seq]).astype(np.float32)
    norm = h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]          # binary32: two products, one sum, each rounded
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

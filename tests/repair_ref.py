"""The repairs a pass must report (rfid_batch_repair / rfid_repair_window: CRC-failed EPC frames made to pass by reversing up to
three of their eight weakest sign decisions), worked out from the ORACLE alone (shared by tests/test_repair_emu.py and
tests/test_gpu_repair.py).  The decision values r_j are built as tests/quality_ref.py builds them -- y = oracle.fir(raw), the gated
samples s = y[open_idx[k] : open_idx[k] + 1370] - dc[k] per component, the window's dump (h_est, T, index), every operation one
numpy.float32 operation -- and then the definition of include/rfid_mi355x.h (rfid_repair) is run LITERALLY: a Python loop over the
92 masks, the oracle's check_crc for the CRC, numpy.float32 additions for the cost.  Before that the signs of r_j are asserted to
reproduce the dump's bits and check_crc to agree with crc_ok on every unflipped frame.  `entry` comes from tests/inventory_ref.py."""
import numpy as np

import inventory_ref as inv
import quality_ref as qref
from rfid import _capi as capi

EPC_WIN = 1370
F = np.float32
N_CAND, MAX_FLIPS = 8, 3
MASKS = [m for m in range(1, 1 << N_CAND) if bin(m).count("1") <= MAX_FLIPS]
assert len(MASKS) == 92 and (N_CAND, MAX_FLIPS) == (capi.REPAIR_CANDIDATES, capi.REPAIR_MAX_FLIPS)


def check_crc(oracle_mod, bits) -> bool:
    """the reference's check_crc (tag_decoder_impl.cc:401-445, the oracle's copy) on 128 0/1 values"""
    return oracle_mod.lib().orc_check_crc(bytes(48 + int(b) for b in bits), 128) == 1


def decision_values(s_re, s_im, h_re, h_im, T, index) -> np.ndarray:
    """r_j, j = 0..127, of one window from its gated samples (float32 arrays) and its dump: the rfid_read_quality definition"""
    h_re, h_im, T, fidx = F(h_re), F(h_im), F(T), F(index)
    j = np.arange(128, dtype=np.int64)
    ia = (j.astype(F) * (F(2.0) * T) + fidx).astype(np.int64)
    ib = (((j * 2).astype(F) * T + T) + fidx).astype(np.int64)
    assert (ia >= 0).all() and (ib >= 0).all() and max(ia.max(), ib.max()) < EPC_WIN
    dx, dy = s_re[ia] - s_re[ib], s_im[ia] - s_im[ib]
    r = dx * h_re - dy * (-h_im)
    assert dx.dtype == F and r.dtype == F
    return r


def bits_of_signs(r) -> np.ndarray:
    """tag_decoder_impl.cc:171-190: bit j = (sign j differs from sign j - 1), the sign before the first one positive"""
    cur = r > 0
    prev = np.concatenate([[True], cur[:-1]])
    return (cur != prev).astype(np.uint8)


def toggled(bits, js) -> np.ndarray:
    """the frame with decisions js reversed: each toggles frame bits j and j + 1, j = 127 bit 127 only"""
    f = np.array(bits, dtype=np.uint8).copy()
    for j in js:
        f[j] ^= 1
        if j < 127:
            f[j + 1] ^= 1
    return f


def passing(oracle_mod, r, bits):
    """steps 2 to 5 of the definition, literally -> [(cost, m, decisions of m in ascending j, frame(m))] of every passing mask, m ascending"""
    a = np.abs(np.asarray(r, dtype=F))
    assert np.isfinite(a).all()
    cand = sorted(range(128), key=lambda j: (a[j], j))[:N_CAND]          # (binary32 values compare exactly as Python floats)
    out = []
    for m in MASKS:
        idx = [i for i in range(N_CAND) if (m >> i) & 1]
        frame = toggled(bits, [cand[i] for i in idx])
        if not check_crc(oracle_mod, frame):
            continue
        cost = F(0.0)
        for i in idx:
            cost = F(cost + a[cand[i]])
        out.append((cost, m, sorted(cand[i] for i in idx), frame))
    return out


def search(oracle_mod, r, bits):
    """the winner -> (n_flips, flips word, cost, frame bits | None)"""
    best = None
    for p in passing(oracle_mod, r, bits):                                # m ascending: the smaller m stays on equal cost
        if best is None or p[0] < best[0]:
            best = p
    if best is None:
        return 0, -1, F(0.0), None
    cost, m, js, frame = best
    word = 0
    for k in range(4):
        word |= (js[k] if k < len(js) else 0xFF) << (8 * k)
    return len(js), int(np.uint32(word).view(np.int32)), cost, frame


def flip_list(rec) -> list:
    """rfid_repair::flips -> the decision indices"""
    w = int(np.int32(rec["flips"]).view(np.uint32))
    return [(w >> (8 * k)) & 0xFF for k in range(int(rec["n_flips"]))]


def _fill(rec, oracle_mod, r, bits, crc_ok):
    """search one window into a record whose stream / seq / start / flags bit 1 are set already"""
    assert np.array_equal(bits_of_signs(r), bits), "the signs of r_j are not the dump's bits"
    assert check_crc(oracle_mod, bits) == bool(crc_ok), "check_crc disagrees with crc_ok"
    rec["flags"] |= int(crc_ok) & 1
    rec["n_flips"], rec["flips"], rec["cost"], rec["entry"] = 0, -1, 0.0, -1
    if crc_ok:
        return
    n, word, cost, frame = search(oracle_mod, r, bits)
    if n:
        rec["n_flips"], rec["flips"], rec["cost"] = n, word, cost
        rec["frame"] = inv.pack_frames(frame[None, :])[0]
        assert check_crc(oracle_mod, frame)


def expected_window(oracle_mod, win, dump) -> np.ndarray:
    """one caller-supplied DC-free EPC window + the oracle's dump of it -> the record rfid_repair_window must give"""
    win = np.ascontiguousarray(win, dtype=np.complex64)
    assert len(win) == EPC_WIN and int(dump["type"]) == 1
    s_re, s_im = np.ascontiguousarray(win.real).astype(F), np.ascontiguousarray(win.imag).astype(F)
    r = decision_values(s_re, s_im, dump["h_est"][0], dump["h_est"][1], dump["T"], dump["index"])
    rec = np.zeros(1, dtype=capi.REPAIR_DTYPE)
    _fill(rec[0], oracle_mod, r, dump["bits"], dump["crc_ok"])
    return rec[0]


def result_of_dump(dump) -> np.ndarray:
    """the oracle's dump of a window as the rfid_decode_result the library gives for it"""
    res = np.zeros(1, dtype=capi.RESULT_DTYPE)[0]
    res["type"], res["index"], res["T"], res["n_bits"] = dump["type"], dump["index"], dump["T"], dump["n_bits"]
    res["h_re"], res["h_im"] = dump["h_est"][0], dump["h_est"][1]
    res["bits"] = inv.pack_frames(dump["bits"][None, :])[0]
    res["crc_ok"] = dump["crc_ok"]
    res["tag_id"] = dump["tag_id"] if dump["crc_ok"] else -1
    return res


def expected(oracle_mod, result, y: np.ndarray, stream: int = 0, overflow: bool = False):
    """oracle Result of one trace + its matched-filter output -> (records of the repaired windows in seq order, records of all
    EPC windows in seq order).  overflow: the trace's inventory overflowed (flag bit 1, no entry looked up)"""
    dumps, open_idx, dc = result.dumps, result.open_idx, result.dc
    seq = np.flatnonzero(dumps["type"] == 1)
    rows = np.zeros(len(seq), dtype=capi.REPAIR_DTYPE)
    if len(seq) == 0:
        return rows, rows
    assert (seq & 1).all()
    ent = inv.expected(dumps, stream)
    which = {bytes(f): i for i, f in enumerate(np.ascontiguousarray(ent["frame"]))} if len(ent) else {}
    yr, yi = np.ascontiguousarray(y.real).astype(F), np.ascontiguousarray(y.imag).astype(F)
    margins = qref.expected_windows(dumps, open_idx, dc, y, stream)
    for n, k in enumerate(seq):
        d = dumps[k]
        start = int(open_idx[k])
        assert start >= 0 and start + EPC_WIN <= len(y)
        dck = np.complex64(dc[k])
        s_re, s_im = yr[start:start + EPC_WIN] - F(dck.real), yi[start:start + EPC_WIN] - F(dck.imag)
        r = decision_values(s_re, s_im, d["h_est"][0], d["h_est"][1], d["T"], d["index"])
        a = np.abs(r)                                                     # (the same values the quality reference forms)
        assert a.min().tobytes() == margins["margin_min"][n].tobytes() and int(a.argmin()) == margins["margin_bit"][n]
        rec = rows[n]
        rec["stream"], rec["seq"], rec["start"], rec["flags"] = stream, k, start, 2 if overflow else 0
        _fill(rec, oracle_mod, r, d["bits"], d["crc_ok"])
        if rec["n_flips"] and not overflow:
            rec["entry"] = which.get(bytes(np.ascontiguousarray(rec["frame"])), -1)
    return rows[rows["n_flips"] > 0], rows


def expected_batch(oracle_mod, results, ys, overflow=()):
    packed, rows = [], []
    for s, (o, y) in enumerate(zip(results, ys)):
        p, r = expected(oracle_mod, o, y, s, s in overflow)
        packed.append(p); rows.append(r)
    return (np.concatenate(packed) if packed else np.zeros(0, dtype=capi.REPAIR_DTYPE)), rows


def assert_equal(got, want, what="") -> None:
    """exact: integers equal, floats by bit pattern, then the bytes of the whole arrays"""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == capi.REPAIR_DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in capi.REPAIR_DTYPE.names if len(got) else ():
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero((a != b).reshape(len(got), -1).any(axis=1))
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][bad[:8]], want[name][bad[:8]])
    assert got.tobytes() == want.tobytes(), what


def structure_ok(oracle_mod, rows, bits_of_seq) -> None:
    """what holds for every repaired record whatever the noise: 1..3 flips in ascending order, the frame passes check_crc and differs
    from the window's decoded bits (bits_of_seq(stream, seq) -> 128 0/1 values) exactly by the toggles of its flips"""
    for rec in rows:
        n = int(rec["n_flips"])
        if n == 0:
            assert rec["flips"] == -1 and rec["entry"] == -1 and rec["cost"] == 0 and not rec["frame"].any()
            continue
        js = flip_list(rec)
        assert 1 <= n <= MAX_FLIPS and js == sorted(set(js)) and max(js) < 128, (rec, js)
        assert (int(np.int32(rec["flips"]).view(np.uint32)) >> (8 * n)) == (0xFFFFFFFF >> (8 * n)), rec
        assert not (rec["flags"] & 1), rec
        j = np.arange(128)
        frame = ((rec["frame"][j >> 5] >> (j & 31)) & 1).astype(np.uint8)
        assert check_crc(oracle_mod, frame), rec
        assert np.array_equal(frame, toggled(bits_of_seq(int(rec["stream"]), int(rec["seq"])), js)), rec

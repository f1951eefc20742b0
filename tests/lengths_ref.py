"""The records the lengths stage must report (rfid_batch_lengths / rfid_length_window: CRC-failed EPC windows read again at the length
their own PC word announces), worked out from the ORACLE alone (shared by tests/test_lengths_emu.py and tests/test_gpu_lengths.py):
y = oracle.fir(raw), the span s[i] = y[open_idx[k] + min(i, last)] - dc[k] per component, T, index, h and the first five bits from
the window's dump, the CRC by the oracle's check_crc over n bits.  The definition of include/rfid_mi355x.h (rfid_sized_frame) is
restated twice, every operation one numpy.float32 operation: `decide` works on arrays, `decide_literal` is the definition as a Python
loop over scalars with the CRC written out.  `expected` asserts the two equal on the first and the last decoded window of every
trace it is given."""
import numpy as np

import inventory_ref as inv
from rfid import _capi as capi

F = np.float32
EPC_WIN, SPAN, MAX_WORDS, OWN_WORDS = 1370, 1728, 8, 6
assert (SPAN, MAX_WORDS) == (capi.LENGTHS_SPAN, capi.LENGTHS_MAX_WORDS)
DTYPE = capi.SIZED_FRAME_DTYPE
PASS, CLAMPED, TOO_LONG, OWN = 2, 4, 8, 16


def words_of(bits) -> int:
    """L = sum of bit_i << (4 - i) over frame bits 0 .. 4"""
    return sum(int(bits[i]) << (4 - i) for i in range(5))


def span_of(y: np.ndarray, start: int, dc, last: int):
    """s[i] = y[start + min(i, last)] - dc per component, i < SPAN -> (s_re, s_im) float32; no sample behind start + last is read"""
    assert 0 <= last < SPAN and start + last < len(y)
    at = start + np.minimum(np.arange(SPAN), last)
    dc = np.complex64(dc)
    s_re = np.ascontiguousarray(y.real).astype(F)[at] - F(dc.real)
    s_im = np.ascontiguousarray(y.imag).astype(F)[at] - F(dc.imag)
    assert s_re.dtype == F
    return s_re, s_im


def check_crc(oracle_mod, bits) -> bool:
    """the reference's check_crc (tag_decoder_impl.cc:401-445, the oracle's copy) over len(bits) 0/1 values"""
    return oracle_mod.lib().orc_check_crc(bytes(48 + int(b) for b in bits), len(bits)) == 1


def decide(oracle_mod, s_re, s_im, L: int, T, index: int, h_re, h_im, last: int) -> dict:
    """the definition on arrays"""
    assert 0 <= L <= MAX_WORDS and L != OWN_WORDS
    n = 32 + 16 * L
    T, fidx, h_re, h_im = F(T), F(index), F(h_re), F(h_im)
    j = np.arange(n, dtype=np.int64)
    ia = (j.astype(F) * (F(2.0) * T) + fidx).astype(np.int64)
    ib = (((j * 2).astype(F) * T + T) + fidx).astype(np.int64)
    far = int(max(ia.max(), ib.max()))
    assert ia.min() >= 0 and ib.min() >= 0 and far < SPAN
    dx, dy = s_re[ia] - s_re[ib], s_im[ia] - s_im[ib]
    r = dx * h_re - dy * (-h_im)
    assert dx.dtype == F and r.dtype == F
    cur = r > 0
    bits = (cur != np.concatenate([[True], cur[:-1]])).astype(np.uint8)
    data = np.packbits(bits)                                              # (MSB first)
    calc = int(oracle_mod.lib().orc_crc16_bytes(data[:-2].tobytes(), len(data) - 2)) & 0xFFFF
    rcvd = (int(data[-2]) << 8) | int(data[-1])
    ok = check_crc(oracle_mod, bits)
    assert ok == (calc == rcvd)
    return dict(n_bits=n, bits=bits, rcvd=rcvd, calc=calc, passes=ok, clamped=far > last)


def decide_literal(s_re, s_im, L: int, T, index: int, h_re, h_im, last: int) -> dict:
    """the definition as written: a loop over the decisions, scalars throughout, the CRC byte by byte"""
    n = 32 + 16 * L
    T, h_re, h_im = F(T), F(h_re), F(h_im)
    hold = lambda i: min(max(i, 0), SPAN - 1)
    prev, bits, far = True, [], 0
    for j in range(n):
        ia = int(F(F(F(j) * F(F(2.0) * T)) + F(index)))
        ib = int(F(F(F(F(2 * j) * T) + T) + F(index)))
        far = max(far, ia, ib)
        dx = F(s_re[hold(ia)] - s_re[hold(ib)])
        dy = F(s_im[hold(ia)] - s_im[hold(ib)])
        r = F(F(dx * h_re) - F(dy * F(-h_im)))
        cur = bool(r > 0)
        bits.append(1 if cur != prev else 0)
        prev = cur
    data = [sum(bits[8 * i + k] << (7 - k) for k in range(8)) for i in range(n // 8)]
    crc = 0xFFFF
    for b in data[:-2]:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    crc ^= 0xFFFF
    rcvd = (data[-2] << 8) | data[-1]
    return dict(n_bits=n, bits=np.array(bits, dtype=np.uint8), rcvd=rcvd, calc=crc, passes=crc == rcvd, clamped=far > last)


def same(a: dict, b: dict) -> bool:
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a) and a.keys() == b.keys()


def pack(bits) -> np.ndarray:
    w = np.zeros(5, dtype=np.uint32)
    for j, b in enumerate(bits):
        if b:
            w[j >> 5] |= np.uint32(1 << (j & 31))
    return w


def _fill(rec, found) -> None:
    rec["flags"] |= (PASS if found["passes"] else 0) | (CLAMPED if found["clamped"] else 0)
    rec["n_bits"], rec["crc_rcvd"], rec["crc_calc"] = found["n_bits"], found["rcvd"], found["calc"]
    rec["frame"] = pack(found["bits"])


def _announce(rec, L: int) -> bool:
    """-> whether the frame is decoded"""
    rec["words"] = L
    if L == OWN_WORDS:
        rec["flags"] |= OWN
    elif L > MAX_WORDS:
        rec["flags"] |= TOO_LONG
    return L != OWN_WORDS and L <= MAX_WORDS


def expected(oracle_mod, result, y: np.ndarray, stream: int = 0) -> np.ndarray:
    """oracle Result of one trace + its matched-filter output (ALL of it: its length is the trace's own) -> the records of all EPC
    windows in seq order"""
    dumps, open_idx, dc = result.dumps, result.open_idx, result.dc
    seq = np.flatnonzero(dumps["type"] == 1)
    rows = np.zeros(len(seq), dtype=DTYPE)
    assert (seq & 1).all()
    todo = [n for n, k in enumerate(seq) if not dumps[k]["crc_ok"] and words_of(dumps[k]["bits"]) not in (6,) + tuple(range(9, 32))]
    for n, k in enumerate(seq):
        d = dumps[k]
        start = int(open_idx[k])
        rec = rows[n]
        rec["stream"], rec["seq"], rec["start"], rec["flags"] = stream, k, start, int(d["crc_ok"]) & 1
        if d["crc_ok"]:
            continue
        L = words_of(d["bits"])
        if not _announce(rec, L):
            continue
        assert start >= 0 and start + EPC_WIN <= len(y)
        last = min(len(y) - 1 - start, SPAN - 1)
        s_re, s_im = span_of(y, start, dc[k], last)
        args = (L, d["T"], int(d["index"]), d["h_est"][0], d["h_est"][1], last)
        found = decide(oracle_mod, s_re, s_im, *args)
        if n in (todo[0], todo[-1]):
            assert same(found, decide_literal(s_re, s_im, *args)), (stream, k)
        assert (found["bits"][:128] == d["bits"][: found["n_bits"]][:128]).all(), (stream, k)       # (decisions below 128: the decoder's)
        _fill(rec, found)
    return rows


def expected_batch(oracle_mod, results, ys):
    return [expected(oracle_mod, o, y, s) for s, (o, y) in enumerate(zip(results, ys))]


def expected_window(oracle_mod, span, result, literal: bool = False) -> np.ndarray:
    """one caller-held DC-free span (1370 .. 1728 samples) + the window's result record -> the record rfid_length_window must give"""
    span = np.ascontiguousarray(span, dtype=np.complex64)
    n = len(span)
    assert EPC_WIN <= n <= SPAN and int(result["type"]) == 1
    rec = np.zeros(1, dtype=DTYPE)[0]
    rec["flags"] = int(result["crc_ok"]) & 1
    if rec["flags"]:
        return rec
    w0 = int(np.asarray(result["bits"])[0])
    L = words_of([(w0 >> i) & 1 for i in range(5)])
    if not _announce(rec, L):
        return rec
    s_re, s_im = span_of(span, 0, 0, n - 1)
    args = (L, result["T"], int(result["index"]), result["h_re"], result["h_im"], n - 1)
    found = decide(oracle_mod, s_re, s_im, *args)
    if literal:
        assert same(found, decide_literal(s_re, s_im, *args))
    _fill(rec, found)
    return rec


def frame_bits(rec) -> np.ndarray:
    """the n_bits bits of a record's frame"""
    j = np.arange(int(rec["n_bits"]))
    return ((np.asarray(rec["frame"])[j >> 5] >> (j & 31)) & 1).astype(np.uint8)


def assert_equal(got, want, what="") -> None:
    """exact: integers equal, then the bytes of the whole arrays (a record holds no floats)"""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in DTYPE.names if len(got) else ():
        a, b = got[name], want[name]
        bad = np.flatnonzero((a != b).reshape(len(got), -1).any(axis=1))
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][bad[:8]], want[name][bad[:8]])
    assert got.tobytes() == want.tobytes(), what

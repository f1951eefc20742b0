"""The reader commands a pass must report (rfid_batch_commands: the PIE command in front of every window), worked out in numpy from
the ORACLE alone (shared by tests/test_commands_emu.py and tests/test_gpu_commands.py): y = oracle.fir(raw), the openings, dc_est and
RN16 dumps of oracle.run_trace, then the definition of include/rfid_mi355x.h (rfid_command), literally: one span at a time, a Python
loop over the edges, the one float comparison per sample in numpy.float32 -- numpy rounds each operation by itself and fuses nothing.
Also what the synthesiser's slot table says every window's command must be."""
import numpy as np

from rfid import _capi as capi
from rfid import synth

SPAN, MAX_EDGES, GAP = 704, 64, 120
NONE, QUERY, QUERY_REP, ACK, NAK, QUERY_ADJUST, UNKNOWN = range(7)
F = np.float32


def low_of(span, level, clipped=0):
    """[704] complex64 samples, the window's dc, the number of leading positions before the trace's start -> low[704] (bool)"""
    re, im = np.ascontiguousarray(span.real).astype(F), np.ascontiguousarray(span.imag).astype(F)
    dr, di = F(np.complex64(level).real), F(np.complex64(level).imag)
    thr = F(F(0.25) * F(F(dr * dr) + F(di * di)))
    low = (re * re + im * im) < thr                      # (binary32 arrays: a product and the sum are rounded by themselves)
    low[:clipped] = False
    return low


def crc5_holds(bits):
    """bits: the 22 data bits of a Query in the order sent"""
    return synth.crc5(bits[:17]) == list(bits[17:22])


def record_of(low, stream=0, seq=0, type_flag=0, clipped=False, rn16_before=None):
    """the definition, literally -> one COMMAND_DTYPE record.  rn16_before: the low 16 decoded bits of window seq - 1, or None"""
    r = np.zeros(1, dtype=capi.COMMAND_DTYPE)[0]
    r["stream"], r["seq"] = stream, seq
    edges = [p for p in range(1, SPAN) if low[p - 1] and not low[p]]
    r["n_edges"] = len(edges)
    e = edges[-MAX_EDGES:]
    c = e[:]
    for j in range(len(e) - 1, 0, -1):
        if e[j] - e[j - 1] > GAP:
            c = e[j:]
            break
    m = len(c)
    d = [0] + [c[k] - c[k - 1] for k in range(1, m)]
    r["n_syms"] = m
    r["end"] = c[-1] if m else 0
    flags = type_flag | (8 if len(edges) > MAX_EDGES else 0) | (16 if clipped else 0)
    cmd = NONE
    if m >= 2:
        r["d0"] = d[1]
    if m >= 3:
        rtcal = d[2]
        r["rtcal"] = rtcal
        trcal = d[3] if (m >= 4 and d[3] > rtcal) else 0
        r["trcal"] = trcal
        data = [int(2 * d[k] > rtcal) for k in range(4 if trcal else 3, m)]
        r["n_bits"] = len(data)
        r["bits"] = sum(b << k for k, b in enumerate(data[:32]))
        nb = len(data)
        cmd = UNKNOWN
        if trcal > 0:
            if nb == 22 and data[:4] == [1, 0, 0, 0]:
                cmd = QUERY
        elif nb == 4 and data[:2] == [0, 0]:
            cmd = QUERY_REP
        elif nb == 18 and data[:2] == [0, 1]:
            cmd = ACK
        elif nb == 8 and data == [1, 1, 0, 0, 0, 0, 0, 0]:
            cmd = NAK
        elif nb == 9 and data[:4] == [1, 0, 0, 1]:
            cmd = QUERY_ADJUST
        if cmd == QUERY and crc5_holds(data):
            flags |= 2
        if cmd == ACK and (seq & 1) and rn16_before is not None:
            if sum(b << k for k, b in enumerate(data[2:18])) == (int(rn16_before) & 0xFFFF):
                flags |= 4
        if 2 * d[1] > rtcal:
            flags |= 32
    r["cmd"], r["flags"] = cmd, flags
    return r


def rn16_word(dump):
    """an oracle RN16 dump -> its 16 decoded bits packed as rfid_decode_result::bits[0] (bit k = the k-th bit)"""
    bits = np.asarray(dump["bits"]).reshape(-1)[:16]
    return int(sum(int(b) << k for k, b in enumerate(bits)))


def expected(result, y, stream=0):
    """oracle Result of one trace + the oracle's matched-filter output -> one record per window, in seq order"""
    n = len(result.open_idx)
    out = np.zeros(n, dtype=capi.COMMAND_DTYPE)
    assert np.array_equal(result.dumps["type"][:n], np.arange(n) & 1)
    for k in range(n):
        a = int(result.open_idx[k])
        clipped = max(SPAN - a, 0)
        span = np.zeros(SPAN, dtype=np.complex64)
        span[clipped:] = y[a - SPAN + clipped:a]
        low = low_of(span, result.dc[k], clipped)
        out[k] = record_of(low, stream, k, k & 1, clipped > 0, rn16_word(result.dumps[k - 1]) if k & 1 else None)
    return out


def expected_batch(results, ys):
    return [expected(o, y, s) for s, (o, y) in enumerate(zip(results, ys))]


def expected_of(spans, levels):
    """[n][704] spans and their levels -> the per-call records: stream = 0, seq = position, flag bits 0, 2 and 4 clear"""
    spans = np.ascontiguousarray(spans, dtype=np.complex64).reshape(-1, SPAN)
    out = np.zeros(len(spans), dtype=capi.COMMAND_DTYPE)
    for k in range(len(spans)):
        out[k] = record_of(low_of(spans[k], levels[k]), 0, k)
    return out


def assert_equal(got, want, what="") -> None:
    """exact: every field equal, then the bytes of the whole arrays"""
    assert got.dtype == capi.COMMAND_DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in capi.COMMAND_DTYPE.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][bad[:8]], want[name][bad[:8]], got[bad[:2]], want[bad[:2]])
    assert got.tobytes() == want.tobytes(), what


def plan_truth(trace):
    """the synthesiser's slot table -> per window (cmd, q or -1, crc5 holds or -1, ACKed RN16 or -1, one responder): window 2 k is
    opened by slot k's Query / QueryRep, window 2 k + 1 by its ACK"""
    out = []
    for s in trace.plan.slots:
        out.append((QUERY, int(s["q"]), 1, -1, False) if int(s["cmd"]) == 0 else (QUERY_REP, -1, -1, -1, False))
        out.append((ACK, -1, -1, int(s["ack"]), int(s["n_tags"]) == 1))
    return out


def fields_of(rec):
    """a record -> (cmd, q, crc5, ACKed RN16) in plan_truth's terms, by the definition's bit order alone"""
    w, cmd = int(rec["bits"]), int(rec["cmd"])
    msb_first = lambda lo, n: sum(((w >> (lo + i)) & 1) << (n - 1 - i) for i in range(n))
    return (cmd, msb_first(13, 4) if cmd == QUERY else -1, ((int(rec["flags"]) >> 1) & 1) if cmd == QUERY else -1,
            msb_first(2, 16) if cmd == ACK else -1)


def check_truth(rows, trace, what=""):
    """EVERY window's (cmd, q, crc5, ACKed RN16) equals the plan's; flag bit 2 on every slot with exactly one responder"""
    truth = plan_truth(trace)[: len(rows)]
    assert len(truth) == len(rows), (what, len(truth), len(rows))
    for k, (r, t) in enumerate(zip(rows, truth)):
        assert fields_of(r) == t[:4], (what, k, r, t)
        if t[4]:
            assert int(r["flags"]) & 4, (what, k, r)

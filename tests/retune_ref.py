"""The records the retune stage must report (rfid_batch_retune / rfid_retune_window: CRC-failed EPC windows decoded again with the
half-bit period searched over 5.0 +- 4 % samples), worked out from the ORACLE alone (shared by tests/test_retune_emu.py and
tests/test_gpu_retune.py): y = oracle.fir(raw), the span s[i] = y[open_idx[k] + min(i, last)] - dc[k] per component, the sync from
the window's dump (index - 65), the CRC by the oracle's check_crc.  The definition of include/rfid_mi355x.h (rfid_retune) is
restated twice, every operation one numpy.float32 operation: `search` works on arrays (all 81 candidates at once, the 256 additions
of a candidate still one after the other), `search_literal` is the definition as a Python loop over scalars.  `expected` asserts the
two equal on the first and the last failed window of every trace it is given."""
import numpy as np

import inventory_ref as inv
import repair_ref
from rfid import _capi as capi

F = np.float32
EPC_WIN, SPAN, N_CAND = 1370, 1408, 81
ONES = (0, 1, 3, 6, 10, 11)                  # the half-bits of TAG_PREAMBLE that are 1
assert (SPAN, N_CAND) == (capi.RETUNE_SPAN, capi.RETUNE_CANDIDATES)
check_crc = repair_ref.check_crc


def grid() -> np.ndarray:
    """T_t = 4.8f + (float)t * ((5.2f - 4.8f) / 80.0f), t = 0 .. 80"""
    step = F(F(F(5.2) - F(4.8)) / F(80.0))
    T = F(4.8) + np.arange(N_CAND).astype(F) * step
    assert T.dtype == F and step.dtype == F
    return T


def span_of(y: np.ndarray, start: int, dc, last: int):
    """s[i] = y[start + min(i, last)] - dc per component, i < SPAN -> (s_re, s_im) float32; no sample behind start + last is read"""
    assert 0 <= last and start + last < len(y)
    at = start + np.minimum(np.arange(SPAN), last)
    dc = np.complex64(dc)
    s_re = np.ascontiguousarray(y.real).astype(F)[at] - F(dc.real)
    s_im = np.ascontiguousarray(y.imag).astype(F)[at] - F(dc.imag)
    assert s_re.dtype == F
    return s_re, s_im


def _decide(oracle_mod, s_re, s_im, m, T, last, energy_idx_max):
    """h, the 128 decisions, the frame and the CRC at half-bit period T (float32 scalar) -> (h_re, h_im, bits, passes, clamped)"""
    fm, T = F(m), F(T)
    fidx = F(fm + F(F(13.0) * T))
    hr, hi, far = F(0.0), F(0.0), int(energy_idx_max)
    for j in ONES:
        at = int(F(fm + F(F(j) * T)))
        far = max(far, at)
        hr, hi = F(hr + s_re[at]), F(hi + s_im[at])
    h_re, h_im = F(hr / F(6.0)), F(hi / F(6.0))
    j = np.arange(128, dtype=np.int64)
    ia = (j.astype(F) * F(F(2.0) * T) + fidx).astype(np.int64)
    ib = (((j * 2).astype(F) * T + T) + fidx).astype(np.int64)
    far = max(far, int(ia.max()), int(ib.max()))
    assert far < SPAN
    dx, dy = s_re[ia] - s_re[ib], s_im[ia] - s_im[ib]
    r = dx * h_re - dy * (-h_im)
    assert r.dtype == F
    bits = repair_ref.bits_of_signs(r)
    return h_re, h_im, bits, check_crc(oracle_mod, bits), far > last


def energies(s_re, s_im, m: int):
    """energy[t] of all candidates side by side, each candidate's 256 terms added in order -> (energy, the largest index gathered)"""
    assert 0 <= m <= 14
    T = grid()
    idx = F(m) + F(13.0) * T
    p = s_re * s_re + s_im * s_im
    i = np.arange(256).astype(F)
    at = (i[None, :] * T[:, None] + idx[:, None])
    assert at.dtype == F and p.dtype == F
    at = at.astype(np.int64)
    assert at.min() >= 0 and at.max() < SPAN
    energy = np.zeros(N_CAND, dtype=F)
    for k in range(256):
        energy = energy + p[at[:, k]]
    assert energy.dtype == F
    return energy, int(at.max())


def search(oracle_mod, s_re, s_im, m: int, last: int) -> dict:
    """the definition on arrays"""
    T = grid()
    energy, far = energies(s_re, s_im, m)
    t = int(np.argmax(energy))                                            # the first maximum
    h_re, h_im, bits, ok, clamped = _decide(oracle_mod, s_re, s_im, m, T[t], last, far)
    return dict(t_index=t, T=T[t], h_re=h_re, h_im=h_im, energy=energy[t], bits=bits, passes=ok, clamped=clamped)


def search_literal(oracle_mod, s_re, s_im, m: int, last: int) -> dict:
    """the definition as written: a loop over candidates, a loop over the 256 terms, scalars throughout"""
    step = F(F(F(5.2) - F(4.8)) / F(80.0))
    best, best_e, far = 0, None, 0
    for t in range(N_CAND):
        T = F(F(4.8) + F(F(t) * step))
        idx = F(F(m) + F(F(13.0) * T))
        e = F(0.0)
        for i in range(256):
            at = int(F(F(F(i) * T) + idx))
            far = max(far, at)
            e = F(e + F(F(s_re[at] * s_re[at]) + F(s_im[at] * s_im[at])))
        if best_e is None or e > best_e:
            best, best_e = t, e
    T = F(F(4.8) + F(F(best) * step))
    h_re, h_im, bits, ok, clamped = _decide(oracle_mod, s_re, s_im, m, T, last, far)
    return dict(t_index=best, T=T, h_re=h_re, h_im=h_im, energy=best_e, bits=bits, passes=ok, clamped=clamped)


def same(a: dict, b: dict) -> bool:
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a) and a.keys() == b.keys()


def _fill(rec, found) -> None:
    rec["flags"] |= (2 if found["passes"] else 0) | (4 if found["clamped"] else 0)
    for name in ("t_index", "T", "h_re", "h_im", "energy"):
        rec[name] = found[name]
    rec["frame"] = inv.pack_frames(found["bits"][None, :])[0]


def expected(oracle_mod, result, y: np.ndarray, stream: int = 0) -> np.ndarray:
    """oracle Result of one trace + its matched-filter output (ALL of it: its length is the trace's own) -> the records of all EPC
    windows in seq order"""
    dumps, open_idx, dc = result.dumps, result.open_idx, result.dc
    seq = np.flatnonzero(dumps["type"] == 1)
    rows = np.zeros(len(seq), dtype=capi.RETUNE_DTYPE)
    assert (seq & 1).all()
    failed = [n for n, k in enumerate(seq) if not dumps[k]["crc_ok"]]
    for n, k in enumerate(seq):
        d = dumps[k]
        start = int(open_idx[k])
        rec = rows[n]
        rec["stream"], rec["seq"], rec["start"], rec["flags"] = stream, k, start, int(d["crc_ok"]) & 1
        if d["crc_ok"]:
            continue
        assert start >= 0 and start + EPC_WIN <= len(y)
        last = min(len(y) - 1 - start, SPAN - 1)
        s_re, s_im = span_of(y, start, dc[k], last)
        m = int(d["index"]) - 65
        found = search(oracle_mod, s_re, s_im, m, last)
        if n in (failed[0], failed[-1]):
            assert same(found, search_literal(oracle_mod, s_re, s_im, m, last)), (stream, k)
        _fill(rec, found)
    return rows


def expected_batch(oracle_mod, results, ys):
    return [expected(oracle_mod, o, y, s) for s, (o, y) in enumerate(zip(results, ys))]


def expected_window(oracle_mod, span, result, literal: bool = False) -> np.ndarray:
    """one caller-held DC-free span (1370 .. 1408 samples) + the window's result record -> the record rfid_retune_window must give"""
    span = np.ascontiguousarray(span, dtype=np.complex64)
    n = len(span)
    assert EPC_WIN <= n <= SPAN and int(result["type"]) == 1
    rec = np.zeros(1, dtype=capi.RETUNE_DTYPE)[0]
    rec["flags"] = int(result["crc_ok"]) & 1
    if rec["flags"]:
        return rec
    s_re, s_im = span_of(span, 0, 0, n - 1)
    m = int(result["index"]) - 65
    found = search(oracle_mod, s_re, s_im, m, n - 1)
    if literal:
        assert same(found, search_literal(oracle_mod, s_re, s_im, m, n - 1))
    _fill(rec, found)
    return rec


def frame_bits(rec) -> np.ndarray:
    j = np.arange(128)
    return ((np.asarray(rec["frame"])[j >> 5] >> (j & 31)) & 1).astype(np.uint8)


def assert_equal(got, want, what="") -> None:
    """exact: integers equal, floats by bit pattern, then the bytes of the whole arrays"""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == capi.RETUNE_DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in capi.RETUNE_DTYPE.names if len(got) else ():
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero((a != b).reshape(len(got), -1).any(axis=1))
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][bad[:8]], want[name][bad[:8]])
    assert got.tobytes() == want.tobytes(), what

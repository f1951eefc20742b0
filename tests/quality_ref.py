"""The read quality a pass must report (rfid_batch_quality: SNR and decision margin of every EPC window), worked out in numpy from
the ORACLE alone (shared by tests/test_quality_emu.py and tests/test_gpu_quality.py): y = oracle.fir(raw), the gated samples
s = y[open_idx[k] : open_idx[k] + 1370] - dc[k] per component, and the window's dump (h_est, T, index, crc_ok) -- then the loop of
include/rfid_mi355x.h (rfid_read_quality) with every operation in numpy.float32: numpy rounds each operation by itself and fuses
nothing; numpy.add.accumulate over binary32 values adds in the order of the axis.  Builds on tests/tracks_ref.py for the order of
the packed array."""
import numpy as np

import tracks_ref as trk
from rfid import _capi as capi

EPC_WIN = 1370
F = np.float32


def one_window_slow(s_re, s_im, h_re, h_im, T, index):
    """the definition, literally: a Python loop over j, every operation one numpy.float32 operation"""
    h_re, h_im, T, fidx = F(h_re), F(h_im), F(T), F(index)
    sig_abs = sig_sq = quad_sq = F(0.0)
    a, bit = None, 0
    for j in range(128):
        ia = int(F(j) * (F(2.0) * T) + fidx)
        ib = int((F(j * 2) * T + T) + fidx)
        dx, dy = F(s_re[ia] - s_re[ib]), F(s_im[ia] - s_im[ib])
        r = F(F(dx * h_re) - F(dy * F(-h_im)))
        q = F(F(dy * h_re) - F(dx * h_im))
        sig_abs = F(sig_abs + abs(r)); sig_sq = F(sig_sq + F(r * r)); quad_sq = F(quad_sq + F(q * q))
        if j == 0:
            a = abs(r)
        elif abs(r) < a:
            a, bit = abs(r), j
    return sig_abs, sig_sq, quad_sq, F(a), bit


def fir_pieces(get_raw, n_raw: int, oracle_mod, piece: int = 40_000_000) -> np.ndarray:
    """oracle.fir over a trace too long for one piece: get_raw(lo, hi) -> complex64 raw samples [lo, hi).  Pieces start at a
    multiple of 5 and overlap by 25 raw samples: behind its first five outputs a piece's sums are those of the whole trace."""
    piece -= piece % 5
    out = []
    for pos in range(0, n_raw - n_raw % 5, piece):
        hi = min(pos + piece, n_raw - n_raw % 5)
        lo = pos - 25 if pos else 0
        y = oracle_mod.fir(get_raw(lo, hi))
        out.append(y[5:] if pos else y)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.complex64)


def expected_windows(dumps: np.ndarray, open_idx: np.ndarray, dc: np.ndarray, y: np.ndarray, stream: int = 0) -> np.ndarray:
    """oracle dumps, openings and dc_est of one trace + the oracle's matched-filter output -> one record per EPC window, in seq order"""
    seq = np.flatnonzero(dumps["type"] == 1)
    out = np.zeros(len(seq), dtype=capi.QUALITY_DTYPE)
    if len(seq) == 0:
        return out
    assert (seq & 1).all()
    start = np.asarray(open_idx)[seq].astype(np.int64)
    assert (start >= 0).all() and (start + EPC_WIN <= len(y)).all()
    d = dumps[seq]
    h = np.ascontiguousarray(d["h_est"]).astype(F)
    h_re, h_im, T, fidx = h[:, 0:1], h[:, 1:2], d["T"].astype(F)[:, None], d["index"].astype(F)[:, None]
    dcs = np.asarray(dc)[seq].astype(np.complex64)
    j = np.arange(128, dtype=np.int64)[None, :]
    ia = (j.astype(F) * (F(2.0) * T) + fidx).astype(np.int64)
    ib = (((j * 2).astype(F) * T + T) + fidx).astype(np.int64)
    assert ia.dtype == np.int64 and (ia >= 0).all() and (ib >= 0).all() and max(ia.max(), ib.max()) < EPC_WIN, (ia.max(), ib.max())
    yr, yi = np.ascontiguousarray(y.real).astype(F), np.ascontiguousarray(y.imag).astype(F)
    dcr, dci = dcs.real.astype(F)[:, None], dcs.imag.astype(F)[:, None]
    sax, sbx = yr[start[:, None] + ia] - dcr, yr[start[:, None] + ib] - dcr      # s[i] = y[start + i] - dc, per component
    say, sby = yi[start[:, None] + ia] - dci, yi[start[:, None] + ib] - dci
    dx, dy = sax - sbx, say - sby
    r = dx * h_re - dy * (-h_im)
    q = dy * h_re - dx * h_im
    for v in (dx, dy, r, q):
        assert v.dtype == F
    ar = np.abs(r)
    acc = lambda t: np.add.accumulate(t, axis=1, dtype=F)[:, -1]               # (0.0f + t_0 == t_0: the terms are not negative)
    out["stream"], out["seq"] = stream, seq
    out["sig_abs"], out["sig_sq"], out["quad_sq"] = acc(ar), acc(r * r), acc(q * q)
    out["margin_min"], out["margin_bit"] = ar.min(axis=1), ar.argmin(axis=1)    # (argmin: the first that attains it)
    out["flags"] = d["crc_ok"] & 1
    # the vectorised form against the literal one, on the first and the last window
    for k in {0, len(seq) - 1}:
        s_re, s_im = yr[start[k]:start[k] + EPC_WIN] - dcr[k, 0], yi[start[k]:start[k] + EPC_WIN] - dci[k, 0]
        slow = one_window_slow(s_re, s_im, h_re[k, 0], h_im[k, 0], T[k, 0], d["index"][k])
        fast = (out["sig_abs"][k], out["sig_sq"][k], out["quad_sq"][k], out["margin_min"][k])
        assert [F(v).tobytes() for v in slow[:4]] == [F(v).tobytes() for v in fast] and slow[4] == out["margin_bit"][k], (k, slow, fast)
    return out


def expected(result, y: np.ndarray, stream: int = 0):
    """oracle Result of one trace + its matched-filter output -> (records of the CRC-verified reads ordered as tracks_ref.expected's
    reads, records of all EPC windows in seq order)"""
    rows = expected_windows(result.dumps, result.open_idx, result.dc, y, stream)
    _, reads, _ = trk.expected(result.dumps, result.open_idx, stream)
    packed = rows[reads["seq"] >> 1] if len(reads) else rows[:0]
    assert (packed["seq"] == reads["seq"]).all() and (packed["flags"] == 1).all()
    return packed, rows


def expected_batch(results, ys):
    packed, rows = [], []
    for s, (o, y) in enumerate(zip(results, ys)):
        p, r = expected(o, y, s)
        packed.append(p); rows.append(r)
    return (np.concatenate(packed) if packed else np.zeros(0, dtype=capi.QUALITY_DTYPE)), rows


def assert_equal(got, want, what="") -> None:
    """exact: integers equal, floats by bit pattern, then the bytes of the whole arrays"""
    assert got.dtype == capi.QUALITY_DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in capi.QUALITY_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][bad[:8]], want[name][bad[:8]])
    assert got.tobytes() == want.tobytes(), what


def snr_db(q) -> np.ndarray:
    """10 log10(sig_sq / quad_sq) in float64, straight from the records (not through the package)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(q["sig_sq"].astype(np.float64) / q["quad_sq"].astype(np.float64))

"""The fine channel records a pass must report (rfid_batch_fine / rfid_fine_window: the data-aided channel estimate of every EPC window
and of its eight 16-bit segments), worked out in numpy from the ORACLE alone (shared by tests/test_fine_emu.py and
tests/test_gpu_fine.py): y = oracle.fir(raw), the gated samples s = y[open_idx[k] : open_idx[k] + 1370] - dc[k] per component, and the
window's dump (T, index, bits, crc_ok; NOT h_est) -- then the definition of include/rfid_mi355x.h (rfid_read_fine) with every
operation in numpy.float32: numpy rounds each operation by itself and fuses nothing; numpy.add.accumulate over binary32 values adds in
the order of the axis, here from an explicit 0.0f in front of the terms.  A vectorised form and a literal Python loop, asserted to
agree on the first and the last window.  Builds on tests/tracks_ref.py for the order of the packed array."""
import numpy as np

import tracks_ref as trk
from rfid import _capi as capi

EPC_WIN = 1370
F = np.float32
SEGS, SEG_BITS = 8, 16


def _clamp(i):
    return 0 if i < 0 else (EPC_WIN - 1 if i > EPC_WIN - 1 else i)


def one_window_slow(s_re, s_im, T, index, bits):
    """the definition, literally: Python loops over the segments and their j, every operation one numpy.float32 operation
    -> (sum_re, sum_im, pow, seg_re[8], seg_im[8], seg_pow[8])"""
    T, fidx = F(T), F(index)
    seg = np.zeros((3, SEGS), dtype=F)
    n_set = 0
    for k in range(SEGS):
        re = im = pw = F(0.0)
        for j in range(SEG_BITS * k, SEG_BITS * (k + 1)):
            ia = _clamp(int(F(j) * (F(2.0) * T) + fidx))
            ib = _clamp(int((F(j * 2) * T + T) + fidx))
            dx, dy = F(s_re[ia] - s_re[ib]), F(s_im[ia] - s_im[ib])
            n_set += int(bits[j])
            g = F(1.0) if n_set % 2 == 0 else F(-1.0)
            re = F(re + F(g * dx))
            im = F(im + F(g * dy))
            pw = F(pw + F(F(dx * dx) + F(dy * dy)))
        seg[0, k], seg[1, k], seg[2, k] = re, im, pw
    tot = []
    for c in range(3):
        acc = F(0.0)
        for k in range(SEGS):
            acc = F(acc + seg[c, k])
        tot.append(acc)
    return tot[0], tot[1], tot[2], seg[0], seg[1], seg[2]


def _in_order(t):
    """(((0.0f + t_0) + t_1) + ...) along the last axis, in binary32"""
    t = np.ascontiguousarray(t, dtype=F)
    z = np.zeros(t.shape[:-1] + (1,), dtype=F)
    return np.add.accumulate(np.concatenate([z, t], axis=-1), axis=-1, dtype=F)[..., -1]


def _fill(out, s_a, s_b, bits):
    """out: records; s_a / s_b: (re, im) of the gathered samples [n][128] (dc already taken out); bits [n][128]"""
    dx, dy = s_a[0] - s_b[0], s_a[1] - s_b[1]
    g = np.where(np.cumsum(bits.astype(np.int64), axis=1) % 2 == 0, F(1.0), F(-1.0)).astype(F)
    pw = dx * dx + dy * dy
    for v in (dx, dy, g, pw):
        assert v.dtype == F
    n = len(out)
    shape = (n, SEGS, SEG_BITS)
    out["seg_re"], out["seg_im"], out["seg_pow"] = _in_order((g * dx).reshape(shape)), _in_order((g * dy).reshape(shape)), _in_order(pw.reshape(shape))
    out["sum_re"], out["sum_im"], out["pow"] = _in_order(out["seg_re"]), _in_order(out["seg_im"]), _in_order(out["seg_pow"])


def _indices(T, fidx):
    """T, fidx [n][1] binary32 -> ia, ib [n][128], clamped into the window"""
    j = np.arange(128, dtype=np.int64)[None, :]
    ia = (j.astype(F) * (F(2.0) * T) + fidx).astype(np.int64)
    ib = (((j * 2).astype(F) * T + T) + fidx).astype(np.int64)
    return np.clip(ia, 0, EPC_WIN - 1), np.clip(ib, 0, EPC_WIN - 1)


def _check_slow(out, k, s_re, s_im, T, index, bits):
    slow = one_window_slow(s_re, s_im, T, index, bits)
    fast = (out["sum_re"][k], out["sum_im"][k], out["pow"][k], out["seg_re"][k], out["seg_im"][k], out["seg_pow"][k])
    for a, b in zip(slow, fast):
        assert np.asarray(a, dtype=F).tobytes() == np.asarray(b, dtype=F).tobytes(), (k, slow, fast)


def expected_windows(dumps: np.ndarray, open_idx: np.ndarray, dc: np.ndarray, y: np.ndarray, stream: int = 0) -> np.ndarray:
    """oracle dumps, openings and dc_est of one trace + the oracle's matched-filter output -> one record per EPC window, in seq order"""
    seq = np.flatnonzero(dumps["type"] == 1)
    out = np.zeros(len(seq), dtype=capi.FINE_DTYPE)
    if len(seq) == 0:
        return out
    assert (seq & 1).all()
    start = np.asarray(open_idx)[seq].astype(np.int64)
    assert (start >= 0).all() and (start + EPC_WIN <= len(y)).all()
    d = dumps[seq]
    T, fidx = d["T"].astype(F)[:, None], d["index"].astype(F)[:, None]
    dcs = np.asarray(dc)[seq].astype(np.complex64)
    ia, ib = _indices(T, fidx)
    yr, yi = np.ascontiguousarray(y.real).astype(F), np.ascontiguousarray(y.imag).astype(F)
    dcr, dci = dcs.real.astype(F)[:, None], dcs.imag.astype(F)[:, None]
    s_a = (yr[start[:, None] + ia] - dcr, yi[start[:, None] + ia] - dci)          # s[i] = y[start + i] - dc, per component
    s_b = (yr[start[:, None] + ib] - dcr, yi[start[:, None] + ib] - dci)
    bits = np.ascontiguousarray(d["bits"])[:, :128]
    _fill(out, s_a, s_b, bits)
    out["stream"], out["seq"], out["start"] = stream, seq, start
    out["flags"] = d["crc_ok"] & 1
    # the vectorised form against the literal one, on the first and the last window
    for k in {0, len(seq) - 1}:
        s_re, s_im = yr[start[k]:start[k] + EPC_WIN] - dcr[k, 0], yi[start[k]:start[k] + EPC_WIN] - dci[k, 0]
        _check_slow(out, k, s_re, s_im, T[k, 0], d["index"][k], bits[k])
    return out


def expected_window(win, dump, bits=None) -> np.ndarray:
    """one caller-supplied DC-free EPC window + the oracle's dump of it (bits: a frame to use instead of the dump's) -> the record
    rfid_fine_window must give"""
    win = np.ascontiguousarray(win, dtype=np.complex64)
    assert len(win) == EPC_WIN and int(dump["type"]) == 1
    s_re, s_im = np.ascontiguousarray(win.real).astype(F), np.ascontiguousarray(win.imag).astype(F)
    bits = np.asarray(dump["bits"] if bits is None else bits)[None, :128]
    ia, ib = _indices(np.array([[dump["T"]]], dtype=F), np.array([[dump["index"]]]).astype(F))
    out = np.zeros(1, dtype=capi.FINE_DTYPE)
    zero = F(0.0)
    _fill(out, (s_re[ia] - zero, s_im[ia] - zero), (s_re[ib] - zero, s_im[ib] - zero), bits)
    out["flags"] = int(dump["crc_ok"]) & 1
    _check_slow(out, 0, s_re, s_im, dump["T"], dump["index"], bits[0])
    return out[0]


def expected(result, y: np.ndarray, stream: int = 0):
    """oracle Result of one trace + its matched-filter output -> (records of the CRC-verified reads ordered as tracks_ref.expected's
    reads, records of all EPC windows in seq order)"""
    rows = expected_windows(result.dumps, result.open_idx, result.dc, y, stream)
    _, reads, _ = trk.expected(result.dumps, result.open_idx, stream)
    packed = rows[reads["seq"] >> 1] if len(reads) else rows[:0]
    assert (packed["seq"] == reads["seq"]).all() and (packed["flags"] == 1).all() and (packed["start"] == reads["start"]).all()
    return packed, rows


def expected_batch(results, ys):
    packed, rows = [], []
    for s, (o, y) in enumerate(zip(results, ys)):
        p, r = expected(o, y, s)
        packed.append(p); rows.append(r)
    return (np.concatenate(packed) if packed else np.zeros(0, dtype=capi.FINE_DTYPE)), rows


def assert_equal(got, want, what="") -> None:
    """exact: integers equal, floats by bit pattern, then the bytes of the whole arrays"""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == capi.FINE_DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in capi.FINE_DTYPE.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][tuple(bad[0])], want[name][tuple(bad[0])])
    assert got.tobytes() == want.tobytes(), what


def h_of(f) -> np.ndarray:
    """(sum_re + j sum_im) / 128 in float64, straight from the records (not through the package)"""
    return (f["sum_re"].astype(np.float64) + 1j * f["sum_im"].astype(np.float64)) / 128.0

"""The records the match stage must report (rfid_batch_match / rfid_match_window: known tags' frames found in CRC-failed EPC windows),
worked out from the ORACLE alone (shared by tests/test_match_emu.py and tests/test_gpu_match.py): y = oracle.fir(raw), the window
s = y[open_idx[k] : + 1370] - dc[k] per component, T, index, h and the decoded bits from the window's dump, a trace's own candidates
from tests/inventory_ref.py, sig_abs against tests/quality_ref.py.  The definition of include/rfid_mi355x.h (rfid_match) is restated
twice, every operation one numpy.float32 operation: `search` works on arrays (the pattern as a cumulative XOR, the scores as
numpy.add.accumulate from a leading 0.0f), `search_literal` is the definition as a Python loop over scalars (the pattern by the
decoder's own chain, c_j = c_(j-1) XOR b_j from c_(-1) = 1).  `expected_rows` asserts the two equal on the first and the last searched
row of every trace it is given.  `policy` restates the host's attribution rule in binary64, straight from the records."""
import numpy as np

import inventory_ref
import quality_ref
from rfid import _capi as capi

F = np.float32
EPC_WIN = 1370
DTYPE = capi.MATCH_DTYPE
READ, OVERFLOW, NO_CANDIDATES, LIST = 1, 2, 4, 8
FLOATS = ("score_best", "score_second", "sig_abs")
MAX_LIST = capi.MATCH_MAX_LIST
assert MAX_LIST == 1024


def unpack(words) -> np.ndarray:
    """[..., 4] uint32 -> [..., 128] 0/1, frame bit j at word j >> 5, bit j & 31"""
    w = np.asarray(words, dtype=np.uint32)
    j = np.arange(128)
    return ((w[..., j >> 5] >> (j & 31).astype(np.uint32)) & np.uint32(1)).astype(np.uint8)


def pack(bits) -> np.ndarray:
    return inventory_ref.pack_frames(np.asarray(bits).reshape(1, 128))[0]


def window_of(y: np.ndarray, start: int, dc):
    """s[i] = y[start + i] - dc per component, i < 1370 -> (s_re, s_im) float32"""
    assert 0 <= start and start + EPC_WIN <= len(y)
    dc = np.complex64(dc)
    w = y[start:start + EPC_WIN]
    s_re = np.ascontiguousarray(w.real).astype(F) - F(dc.real)
    s_im = np.ascontiguousarray(w.imag).astype(F) - F(dc.imag)
    assert s_re.dtype == F
    return s_re, s_im


def decision_values(s_re, s_im, T, index, h_re, h_im) -> np.ndarray:
    """r_j, j = 0 .. 127, of the rfid_read_quality definition, on arrays"""
    T, fidx, h_re, h_im = F(T), F(index), F(h_re), F(h_im)
    j = np.arange(128, dtype=np.int64)
    ia = np.clip((j.astype(F) * (F(2.0) * T) + fidx).astype(np.int64), 0, EPC_WIN - 1)
    ib = np.clip((((j * 2).astype(F) * T + T) + fidx).astype(np.int64), 0, EPC_WIN - 1)
    dx, dy = s_re[ia] - s_re[ib], s_im[ia] - s_im[ib]
    r = dx * h_re - dy * (-h_im)
    assert dx.dtype == F and r.dtype == F
    return r


def in_order(t) -> np.float32:
    """(((0.0f + t_0) + t_1) + ...): the leading +0 matters for the sign of a zero sum"""
    return np.add.accumulate(np.concatenate([[F(0.0)], np.asarray(t, dtype=F)]), dtype=F)[-1]


def pattern(bits) -> np.ndarray:
    """c_j = 1 XOR b_0 XOR ... XOR b_j -> bool[128]"""
    return (np.bitwise_xor.accumulate(np.asarray(bits, dtype=np.uint8)) ^ 1).astype(bool)


def search(r, decoded, cands) -> dict:
    """the definition on arrays.  r: the 128 decision values; decoded: the window's 128 decoded bits; cands: [n][128] candidate bits"""
    cands = np.asarray(cands, dtype=np.uint8).reshape(-1, 128)
    assert len(cands) >= 1
    scores = [in_order(np.where(pattern(b), r, -r)) for b in cands]
    order = sorted(range(len(cands)), key=lambda i: (-float(scores[i]), i))      # the larger score, the lower index on equal scores
    best = order[0]
    second = order[1] if len(order) > 1 else -1
    out = dict(best=best, second=second, score_best=F(scores[best]), score_second=F(scores[second]) if second >= 0 else F(0.0),
               sig_abs=in_order(np.abs(r)), dist_best=int((cands[best] != np.asarray(decoded, dtype=np.uint8)).sum()),
               diff=int((pattern(cands[best]) != pattern(cands[second])).sum()) if second >= 0 else -1, frame=pack(cands[best]))
    return out


def search_literal(s_re, s_im, T, index, h_re, h_im, decoded, cands) -> dict:
    """the definition as written: loops over decisions and candidates, scalars throughout"""
    hold = lambda i: min(max(i, 0), EPC_WIN - 1)
    T, h_re, h_im = F(T), F(h_re), F(h_im)
    r = []
    for j in range(128):
        ia = hold(int(F(F(F(j) * F(F(2.0) * T)) + F(index))))
        ib = hold(int(F(F(F(F(2 * j) * T) + T) + F(index))))
        dx = F(s_re[ia] - s_re[ib])
        dy = F(s_im[ia] - s_im[ib])
        r.append(F(F(dx * h_re) - F(dy * F(-h_im))))
    sig = F(0.0)
    for j in range(128):
        sig = F(sig + F(abs(r[j])))

    def signs(b):
        c, prev = [], 1
        for j in range(128):
            prev ^= int(b[j])               # bit_j = c_j XOR c_(j-1)
            c.append(prev)
        return c

    best = second = -1
    sb = ss = F(0.0)
    for i, b in enumerate(cands):
        c = signs(b)
        s = F(0.0)
        for j in range(128):
            s = F(s + (r[j] if c[j] else F(-r[j])))
        if best < 0 or s > sb:
            second, ss, best, sb = best, sb, i, s
        elif second < 0 or s > ss:
            second, ss = i, s
    dist = sum(int(a) != int(b) for a, b in zip(cands[best], decoded))
    diff = sum(a != b for a, b in zip(signs(cands[best]), signs(cands[second]))) if second >= 0 else -1
    return dict(best=best, second=second, score_best=sb, score_second=ss if second >= 0 else F(0.0), sig_abs=sig, dist_best=dist, diff=diff,
                frame=pack(cands[best]))


def same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a
                                        if k not in ("best", "second", "dist_best", "diff")) and \
        all(int(a[k]) == int(b[k]) for k in ("best", "second", "dist_best", "diff"))


def _fill(rec, found, n_cand) -> None:
    rec["n_cand"] = n_cand
    for k in ("best", "second", "score_best", "score_second", "sig_abs", "dist_best", "diff", "frame"):
        rec[k] = found[k]


def expected_rows(result, y: np.ndarray, stream: int = 0, frames=None, max_tags: int = 64):
    """the oracle Result of one trace + its matched-filter output -> the records of all its EPC windows in seq order.  frames: the
    caller's list as [n][4] words, or None: the trace's own inventory (inventory_ref.expected), overflowed above max_tags"""
    dumps, open_idx = result.dumps, result.open_idx
    seq = np.flatnonzero(dumps["type"] == 1)
    assert (seq & 1).all() and len(seq) == len(dumps) // 2
    rows = np.zeros(len(seq), dtype=DTYPE)
    if frames is not None:
        cands, trace_flags = unpack(np.asarray(frames, dtype=np.uint32).reshape(-1, 4)), LIST
        assert 1 <= len(cands) <= MAX_LIST
    else:
        entries = inventory_ref.expected(dumps, stream)
        over = len(entries) > max_tags
        cands = unpack(entries["frame"]) if len(entries) and not over else np.zeros((0, 128), dtype=np.uint8)
        trace_flags = OVERFLOW if over else (NO_CANDIDATES if len(cands) == 0 else 0)
    quality = quality_ref.expected_windows(dumps, open_idx, result.dc, y, stream) if len(seq) else None
    todo = [n for n, k in enumerate(seq) if dumps[k]["crc_ok"] != 1 and len(cands)]
    for n, k in enumerate(seq):
        rec, d = rows[n], dumps[k]
        rec["stream"], rec["seq"], rec["start"] = stream, k, int(open_idx[k])
        rec["flags"] = (READ if d["crc_ok"] == 1 else 0) | trace_flags
        if n not in todo:
            continue
        s_re, s_im = window_of(y, int(open_idx[k]), result.dc[k])
        args = (d["T"], int(d["index"]), d["h_est"][0], d["h_est"][1])
        found = search(decision_values(s_re, s_im, *args), d["bits"], cands)
        assert F(found["sig_abs"]).tobytes() == F(quality["sig_abs"][n]).tobytes(), (stream, k)      # as rfid_read_quality::sig_abs
        if n in (todo[0], todo[-1]):
            assert same(found, search_literal(s_re, s_im, *args, d["bits"], cands)), (stream, k)
        _fill(rec, found, len(cands))
    return rows


def expected_window(span, result, frames, literal: bool = False) -> np.ndarray:
    """a caller-held DC-free span (1370) + the window's result record + [n][4] candidate words -> the record rfid_match_window must give"""
    span = np.ascontiguousarray(span, dtype=np.complex64)
    cands = unpack(np.asarray(frames, dtype=np.uint32).reshape(-1, 4))
    assert span.shape == (EPC_WIN,) and int(result["type"]) == 1 and 1 <= len(cands) <= MAX_LIST
    rec = np.zeros(1, dtype=DTYPE)[0]
    rec["flags"] = LIST | (READ if int(result["crc_ok"]) == 1 else 0)
    if rec["flags"] & READ:
        return rec
    s_re, s_im = window_of(span, 0, 0)
    args = (result["T"], int(result["index"]), result["h_re"], result["h_im"])
    decoded = unpack(result["bits"])
    found = search(decision_values(s_re, s_im, *args), decoded, cands)
    if literal:
        assert same(found, search_literal(s_re, s_im, *args, decoded, cands))
    _fill(rec, found, len(cands))
    return rec


def policy(rows, min_rho: float = 0.5) -> np.ndarray:
    """the host's attribution rule in binary64, straight from the records: searched, score_best / sig_abs >= min_rho, and no second or
    score_best - score_second >= diff * sig_abs / 128"""
    rows = np.atleast_1d(rows)
    out = np.zeros(len(rows), dtype=bool)
    for i, r in enumerate(rows):
        if int(r["flags"]) & READ or int(r["n_cand"]) == 0 or not float(r["sig_abs"]) > 0:
            continue
        sig, sb, ss = float(r["sig_abs"]), float(r["score_best"]), float(r["score_second"])
        out[i] = sb / sig >= min_rho and (int(r["second"]) < 0 or sb - ss >= int(r["diff"]) * sig / 128.0)
    return out


def frame_bits(rec) -> np.ndarray:
    return unpack(rec["frame"])


def assert_equal(got, want, what="") -> None:
    """exact: integers equal, the floats by bit pattern, then the bytes of the whole arrays"""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in DTYPE.names if len(got) else ():
        a, b = got[name], want[name]
        if name in FLOATS:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero((a != b).reshape(len(got), -1).any(axis=1))
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][bad[:8]], want[name][bad[:8]])
    assert got.tobytes() == want.tobytes(), what

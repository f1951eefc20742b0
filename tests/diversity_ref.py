"""The records the diversity stage must report (rfid_batch_diversity / rfid_diversity_window: the EPC windows of traces recorded together --
the receive antennas of one session -- combined before the sign is taken), worked out from the ORACLE alone (shared by
tests/test_diversity_emu.py and tests/test_gpu_diversity.py): per member y = oracle.fir(raw), its own window s = y[open_idx[k] : + 1370] -
dc[k] per component, T, index and h from that member's dump of the window, the CRC by the oracle's check_crc.  The definition of
include/rfid_mi355x.h (rfid_diversity) is restated twice, every operation one numpy.float32 operation: `combine` works on arrays,
`combine_literal` is the definition as a Python loop over scalars with the CRC written out.  `expected_group` asserts the two equal on
the first and the last combined row of every group it is given."""
import numpy as np

from rfid import _capi as capi

F = np.float32
EPC_WIN, SLACK, MAX_MEMBERS = 1370, 4, 8
assert (SLACK, MAX_MEMBERS) == (capi.DIVERSITY_SLACK, capi.DIVERSITY_MAX_MEMBERS)
DTYPE = capi.DIVERSITY_DTYPE
READ, PASS, LONE = 1, 2, 4
FLOATS = ("h_sq", "margin_min")


def window_of(y: np.ndarray, start: int, dc):
    """s[i] = y[start + i] - dc per component, i < 1370 -> (s_re, s_im) float32"""
    assert 0 <= start and start + EPC_WIN <= len(y)
    dc = np.complex64(dc)
    w = y[start:start + EPC_WIN]
    s_re = np.ascontiguousarray(w.real).astype(F) - F(dc.real)
    s_im = np.ascontiguousarray(w.imag).astype(F) - F(dc.imag)
    assert s_re.dtype == F
    return s_re, s_im


def combine(oracle_mod, members) -> dict:
    """the definition on arrays.  members: [(s_re, s_im, T, index, h_re, h_im)] of the present members in ascending m"""
    acc, h_sq = None, F(0.0)
    j = np.arange(128, dtype=np.int64)
    for s_re, s_im, T, index, h_re, h_im in members:
        T, fidx, h_re, h_im = F(T), F(index), F(h_re), F(h_im)
        ia = np.clip((j.astype(F) * (F(2.0) * T) + fidx).astype(np.int64), 0, EPC_WIN - 1)
        ib = np.clip((((j * 2).astype(F) * T + T) + fidx).astype(np.int64), 0, EPC_WIN - 1)
        dx, dy = s_re[ia] - s_re[ib], s_im[ia] - s_im[ib]
        r = dx * h_re - dy * (-h_im)
        assert dx.dtype == F and r.dtype == F
        acc = r if acc is None else acc + r
        h_sq = F(h_sq + F(F(h_re * h_re) + F(h_im * h_im)))
    assert acc.dtype == F
    cur = acc > 0
    bits = (cur != np.concatenate([[True], cur[:-1]])).astype(np.uint8)
    data = np.packbits(bits)                                              # (MSB first)
    calc = int(oracle_mod.lib().orc_crc16_bytes(data[:14].tobytes(), 14)) & 0xFFFF
    rcvd = (int(data[14]) << 8) | int(data[15])
    ok = oracle_mod.lib().orc_check_crc(bytes(48 + int(b) for b in bits), 128) == 1
    assert ok == (calc == rcvd)
    mag = np.abs(acc)
    return dict(bits=bits, rcvd=rcvd, calc=calc, passes=ok, margin=F(mag.min()), weakest=int(np.argmin(mag)), h_sq=h_sq)


def combine_literal(members) -> dict:
    """the definition as written: a loop over the decisions, scalars throughout, the CRC byte by byte"""
    hold = lambda i: min(max(i, 0), EPC_WIN - 1)
    acc = [None] * 128
    h_sq = F(0.0)
    for s_re, s_im, T, index, h_re, h_im in members:
        T, h_re, h_im = F(T), F(h_re), F(h_im)
        for j in range(128):
            ia = hold(int(F(F(F(j) * F(F(2.0) * T)) + F(index))))
            ib = hold(int(F(F(F(F(2 * j) * T) + T) + F(index))))
            dx = F(s_re[ia] - s_re[ib])
            dy = F(s_im[ia] - s_im[ib])
            r = F(F(dx * h_re) - F(dy * F(-h_im)))
            acc[j] = r if acc[j] is None else F(acc[j] + r)
        h_sq = F(h_sq + F(F(h_re * h_re) + F(h_im * h_im)))
    prev, bits = True, []
    margin, weakest = None, 0
    for j in range(128):
        cur = bool(acc[j] > 0)
        bits.append(1 if cur != prev else 0)
        prev = cur
        a = F(abs(acc[j]))
        if margin is None or a < margin:
            margin, weakest = a, j
    data = [sum(bits[8 * i + k] << (7 - k) for k in range(8)) for i in range(16)]
    crc = 0xFFFF
    for b in data[:14]:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    crc ^= 0xFFFF
    rcvd = (data[14] << 8) | data[15]
    return dict(bits=np.array(bits, dtype=np.uint8), rcvd=rcvd, calc=crc, passes=crc == rcvd, margin=F(margin), weakest=weakest, h_sq=h_sq)


def same(a: dict, b: dict) -> bool:
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a) and a.keys() == b.keys()


def pack(bits) -> np.ndarray:
    w = np.zeros(4, dtype=np.uint32)
    for j, b in enumerate(bits):
        if b:
            w[j >> 5] |= np.uint32(1 << (j & 31))
    return w


def _fill(rec, found) -> None:
    rec["flags"] |= PASS if found["passes"] else 0
    rec["frame"] = pack(found["bits"])
    rec["crc_rcvd"], rec["crc_calc"] = found["rcvd"], found["calc"]
    rec["h_sq"], rec["margin_min"], rec["weakest"] = found["h_sq"], found["margin"], found["weakest"]


def classify(rec, present: int, reads: int) -> bool:
    """the masks and the flag they give -> whether the row is combined"""
    rec["present"], rec["reads"] = present, reads
    if reads:
        rec["flags"] = READ
    elif bin(present).count("1") < 2:
        rec["flags"] = LONE
    return rec["flags"] == 0


def expected_group(oracle_mod, results, ys, anchor_stream: int = 0):
    """the oracle Results of one group's members + their matched-filter outputs (ALL of each: its length is the trace's own) -> (the
    records of all EPC windows of the anchor in seq order, the member-rows left out: members absent from a row)"""
    M = len(results)
    assert 2 <= M <= MAX_MEMBERS
    d0, open0 = results[0].dumps, results[0].open_idx
    seq = np.flatnonzero(d0["type"] == 1)
    assert (seq & 1).all() and len(seq) == len(d0) // 2
    rows = np.zeros(len(seq), dtype=DTYPE)
    plans, left_out = [], 0
    for n, k in enumerate(seq):
        rec = rows[n]
        rec["stream"], rec["seq"], rec["start"] = anchor_stream, k, int(open0[k])
        present = reads = 0
        for m, o in enumerate(results):
            there = m == 0 or (k < len(o.dumps) and o.dumps[k]["type"] == 1 and abs(int(o.open_idx[k]) - int(open0[k])) <= SLACK)
            if there:
                present |= 1 << m
                if o.dumps[k]["type"] == 1 and o.dumps[k]["crc_ok"] == 1:
                    reads |= 1 << m
            else:
                left_out += 1
        if classify(rec, present, reads):
            plans.append((n, k, present))
        elif reads:
            low = (reads & -reads).bit_length() - 1
            rec["frame"] = pack(results[low].dumps[k]["bits"])
    for i, (n, k, present) in enumerate(plans):
        members = []
        for m, (o, y) in enumerate(zip(results, ys)):
            if (present >> m) & 1:
                d = o.dumps[k]
                members.append(window_of(y, int(o.open_idx[k]), o.dc[k]) + (d["T"], int(d["index"]), d["h_est"][0], d["h_est"][1]))
        found = combine(oracle_mod, members)
        if i in (0, len(plans) - 1):
            assert same(found, combine_literal(members)), (anchor_stream, k)
        _fill(rows[n], found)
    return rows, left_out


def expected_batch(oracle_mod, results, ys, M: int):
    """-> ([rows of group g], [member-rows left out of group g])"""
    assert len(results) % M == 0
    out = [expected_group(oracle_mod, results[g:g + M], ys[g:g + M], g) for g in range(0, len(results), M)]
    return [r for r, _ in out], [n for _, n in out]


def expected_window(oracle_mod, spans, results, literal: bool = False) -> np.ndarray:
    """caller-held DC-free spans (members, 1370) + the members' result records -> the record rfid_diversity_window must give"""
    spans = np.ascontiguousarray(spans, dtype=np.complex64)
    M = len(spans)
    assert spans.shape == (M, EPC_WIN) and len(results) == M and all(int(r["type"]) == 1 for r in results)
    rec = np.zeros(1, dtype=DTYPE)[0]
    reads = sum(1 << m for m, r in enumerate(results) if int(r["crc_ok"]) == 1)
    if not classify(rec, (1 << M) - 1, reads):
        low = (reads & -reads).bit_length() - 1
        rec["frame"] = results[low]["bits"]
        return rec
    members = [window_of(s, 0, 0) + (r["T"], int(r["index"]), r["h_re"], r["h_im"]) for s, r in zip(spans, results)]
    found = combine(oracle_mod, members)
    if literal:
        assert same(found, combine_literal(members))
    _fill(rec, found)
    return rec


def frame_bits(rec) -> np.ndarray:
    j = np.arange(128)
    return ((np.asarray(rec["frame"])[j >> 5] >> (j & 31)) & 1).astype(np.uint8)


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

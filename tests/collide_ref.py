"""The records the collisions stage must report (rfid_batch_collisions / rfid_collisions_of: both RN16s and both channels of an RN16
window, as of two tags replying at once), worked out from the ORACLE alone (shared by tests/test_collide_emu.py and
tests/test_gpu_collide.py): y = oracle.fir(raw), the window's start and dc from open_idx and dc of oracle.run_trace, its index, h_est
and 16 bits from the window's dump.  The definition of include/rfid_mi355x.h (rfid_collision) is restated twice, every operation one
numpy.float32 operation: `records` works on arrays (all windows side by side, the 16 terms of a sum still one after the other),
`record_literal` is the definition as a Python loop over scalars.  `expected` asserts the two equal on the first and the last RN16
window of every trace it is given.  Below them the truth helpers: which handles were sent in a slot (Trace.plan.slots)."""
import numpy as np

from rfid import _capi as capi

F = np.float32
WIN, FIRST = 250, 65
assert WIN == capi.RN16_WINDOW
FLOATS = ("ha_re", "ha_im", "hb_re", "hb_im", "resid", "sum_sq", "c_re", "c_im")


def _dist(px, py, qx, qy):
    ex, ey = px - qx, py - qy
    return ex * ex + ey * ey


def _in_order(terms: np.ndarray, take: np.ndarray) -> np.ndarray:
    """per window (((0.0f + t_j0) + t_j1) + ...) over the j with take[:, j], j ascending"""
    acc = np.zeros(len(terms), dtype=F)
    for j in range(terms.shape[1]):
        acc = np.where(take[:, j], acc + terms[:, j], acc)
    assert acc.dtype == F
    return acc


def _handles(pos: np.ndarray) -> np.ndarray:
    """pos[:, j]: decision j positive -> bit_j = (pos_j != pos_j-1), pos_-1 positive; the sum of bit_j << (15 - j)"""
    prev = np.concatenate([np.ones((len(pos), 1), dtype=bool), pos[:, :-1]], axis=1)
    return ((pos != prev).astype(np.int64) << (15 - np.arange(16))[None, :]).sum(axis=1)


def handle_of_bits(bits) -> int:
    """the decoder's own 16 bits (the first decided first) as a handle: MSB first as sent"""
    return int(sum(int(b) << (15 - j) for j, b in enumerate(np.asarray(bits)[:16])))


def records(y: np.ndarray, starts, dcs, index, h_re, h_im, dec) -> np.ndarray:
    """the definition on arrays: N windows of y (complex64) -> N records (stream = seq = 0)"""
    n = len(starts)
    rows = np.zeros(n, dtype=capi.COLLISION_DTYPE)
    if n == 0:
        return rows
    starts, index, dec = np.asarray(starts, dtype=np.int64), np.asarray(index, dtype=np.int64), np.asarray(dec, dtype=np.int64)
    dcs = np.asarray(dcs, dtype=np.complex64)
    hre, him = np.asarray(h_re, dtype=F)[:, None], np.asarray(h_im, dtype=F)[:, None]
    y_re, y_im = np.ascontiguousarray(y.real).astype(F), np.ascontiguousarray(y.imag).astype(F)
    m = np.clip(index - FIRST, 0, 14)
    at = (starts + m + FIRST)[:, None] + 5 * np.arange(32)[None, :]
    assert at.min() >= 0 and at.max() < len(y) and ((at - starts[:, None]) < WIN).all()
    zr, zi = y_re[at] - dcs.real.astype(F)[:, None], y_im[at] - dcs.imag.astype(F)[:, None]
    dx, dy = zr[:, 0::2] - zr[:, 1::2], zi[:, 0::2] - zi[:, 1::2]
    wx, wy = dx * dx - dy * dy, (F(2.0) * dx) * dy
    ax, ay = hre * hre - him * him, (F(2.0) * hre) * him
    assert dx.dtype == F and wy.dtype == F and ay.dtype == F
    g_a = _dist(wx, wy, ax, ay)
    # ---- two clusters, one centre held at A ----
    k = np.arange(n)
    far = np.argmax(g_a, axis=1)                                  # the first maximum
    cx, cy = wx[k, far], wy[k, far]
    for _ in range(4):
        mem = _dist(wx, wy, cx[:, None], cy[:, None]) < g_a
        cnt = mem.sum(axis=1)
        sx, sy = _in_order(wx, mem), _in_order(wy, mem)
        div = np.maximum(cnt, 1).astype(F)
        cx, cy = np.where(cnt > 0, sx / div, cx), np.where(cnt > 0, sy / div, cy)
    assert cx.dtype == F
    mem = _dist(wx, wy, cx[:, None], cy[:, None]) < g_a
    nd = mem.sum(axis=1)
    ns = 16 - nd
    # ---- the signed means of the two sets ----
    pos = dx * hre + dy * him > F(0.0)
    ssx, ssy = _in_order(np.where(pos, dx, -dx), ~mem), _in_order(np.where(pos, dy, -dy), ~mem)
    low = np.argmax(mem, axis=1)                                  # the member of lowest j (0 where there is none: unused)
    rx, ry = dx[k, low][:, None], dy[k, low][:, None]
    pos = dx * rx + dy * ry > F(0.0)
    sdx, sdy = _in_order(np.where(pos, dx, -dx), mem), _in_order(np.where(pos, dy, -dy), mem)
    div_s, div_d = np.maximum(ns, 1).astype(F), np.maximum(nd, 1).astype(F)
    hsx, hsy = np.where(ns > 0, ssx / div_s, hre[:, 0]), np.where(ns > 0, ssy / div_s, him[:, 0])
    hdx, hdy = np.where(nd > 0, sdx / div_d, F(0.0)), np.where(nd > 0, sdy / div_d, F(0.0))
    assert hsx.dtype == F and hdy.dtype == F
    # ---- the four points ----
    four = np.stack([_dist(dx, dy, hsx[:, None], hsy[:, None]), _dist(dx, dy, -hsx[:, None], -hsy[:, None]),
                     _dist(dx, dy, hdx[:, None], hdy[:, None]), _dist(dx, dy, -hdx[:, None], -hdy[:, None])])
    pick = np.argmin(four, axis=0)                                # the first minimum
    best = np.take_along_axis(four, pick[None], axis=0)[0]
    every = np.ones_like(mem)
    resid, sum_sq = _in_order(best, every), _in_order(dx * dx + dy * dy, every)
    ra, rb = _handles((pick == 0) | (pick == 2)), _handles((pick == 0) | (pick == 3))
    h1x, h1y, h2x, h2y = (hsx + hdx) / F(2.0), (hsy + hdy) / F(2.0), (hsx - hdx) / F(2.0), (hsy - hdy) / F(2.0)
    swap = h2x * h2x + h2y * h2y > h1x * h1x + h1y * h1y
    assert h1x.dtype == F and resid.dtype == F
    rows["rn16_a"], rows["rn16_b"] = np.where(swap, rb, ra), np.where(swap, ra, rb)
    rows["ha_re"], rows["ha_im"] = np.where(swap, h2x, h1x), np.where(swap, h2y, h1y)
    rows["hb_re"], rows["hb_im"] = np.where(swap, h1x, h2x), np.where(swap, h1y, h2y)
    rows["flags"] = (dec == rows["rn16_a"]) * 1 + (dec == rows["rn16_b"]) * 2 + (nd == 0) * 4 + swap * 8
    rows["n_same"], rows["n_diff"], rows["resid"], rows["sum_sq"], rows["c_re"], rows["c_im"] = ns, nd, resid, sum_sq, cx, cy
    return rows


def record_literal(y: np.ndarray, start: int, dc, index: int, h_re, h_im, dec: int) -> np.ndarray:
    """the definition as written: one window, loops over j, scalars throughout"""
    rec = np.zeros(1, dtype=capi.COLLISION_DTYPE)[0]
    dc = np.complex64(dc)
    dcr, dci, hsx0, hsy0 = F(dc.real), F(dc.imag), F(h_re), F(h_im)
    m = min(max(int(index) - FIRST, 0), 14)
    z = []
    for i in range(32):
        v = np.complex64(y[start + m + FIRST + 5 * i])
        z.append((F(F(v.real) - dcr), F(F(v.imag) - dci)))
    d = [(F(z[2 * j][0] - z[2 * j + 1][0]), F(z[2 * j][1] - z[2 * j + 1][1])) for j in range(16)]
    sq = lambda vx, vy: (F(F(vx * vx) - F(vy * vy)), F(F(F(2.0) * vx) * vy))

    def dist(px, py, qx, qy):
        ex, ey = F(px - qx), F(py - qy)
        return F(F(ex * ex) + F(ey * ey))

    w = [sq(*v) for v in d]
    ax, ay = sq(hsx0, hsy0)
    g_a = [dist(wx, wy, ax, ay) for wx, wy in w]
    far, cx, cy = g_a[0], w[0][0], w[0][1]
    for j in range(1, 16):
        if g_a[j] > far:
            far, cx, cy = g_a[j], w[j][0], w[j][1]
    for _ in range(4):
        sx, sy, cnt = F(0.0), F(0.0), 0
        for j in range(16):
            if dist(w[j][0], w[j][1], cx, cy) < g_a[j]:
                sx, sy, cnt = F(sx + w[j][0]), F(sy + w[j][1]), cnt + 1
        if cnt:
            cx, cy = F(sx / F(cnt)), F(sy / F(cnt))
    mem = [bool(dist(w[j][0], w[j][1], cx, cy) < g_a[j]) for j in range(16)]
    nd = sum(mem)
    ns = 16 - nd
    ssx, ssy, sdx, sdy, r = F(0.0), F(0.0), F(0.0), F(0.0), None
    for j in range(16):
        dx, dy = d[j]
        if mem[j]:
            if r is None:
                r = d[j]
            pos = F(F(dx * r[0]) + F(dy * r[1])) > F(0.0)
            sdx, sdy = F(sdx + (dx if pos else -dx)), F(sdy + (dy if pos else -dy))
        else:
            pos = F(F(dx * hsx0) + F(dy * hsy0)) > F(0.0)
            ssx, ssy = F(ssx + (dx if pos else -dx)), F(ssy + (dy if pos else -dy))
    hsx, hsy = (F(ssx / F(ns)), F(ssy / F(ns))) if ns else (hsx0, hsy0)
    hdx, hdy = (F(sdx / F(nd)), F(sdy / F(nd))) if nd else (F(0.0), F(0.0))
    points = ((hsx, hsy, True, True), (F(-hsx), F(-hsy), False, False), (hdx, hdy, True, False), (F(-hdx), F(-hdy), False, True))
    resid, sum_sq, ra, rb, prev_a, prev_b = F(0.0), F(0.0), 0, 0, True, True
    for j in range(16):
        dx, dy = d[j]
        best, alpha, beta = None, None, None
        for px, py, al, be in points:
            v = dist(dx, dy, px, py)
            if best is None or v < best:
                best, alpha, beta = v, al, be
        resid = F(resid + best)
        sum_sq = F(sum_sq + F(F(dx * dx) + F(dy * dy)))
        ra |= int(alpha != prev_a) << (15 - j)
        rb |= int(beta != prev_b) << (15 - j)
        prev_a, prev_b = alpha, beta
    h1 = (F(F(hsx + hdx) / F(2.0)), F(F(hsy + hdy) / F(2.0)))
    h2 = (F(F(hsx - hdx) / F(2.0)), F(F(hsy - hdy) / F(2.0)))
    swap = bool(F(F(h2[0] * h2[0]) + F(h2[1] * h2[1])) > F(F(h1[0] * h1[0]) + F(h1[1] * h1[1])))
    if swap:
        ra, rb, h1, h2 = rb, ra, h2, h1
    rec["flags"] = (1 if dec == ra else 0) | (2 if dec == rb else 0) | (4 if nd == 0 else 0) | (8 if swap else 0)
    rec["n_same"], rec["n_diff"], rec["rn16_a"], rec["rn16_b"] = ns, nd, ra, rb
    rec["ha_re"], rec["ha_im"], rec["hb_re"], rec["hb_im"] = h1[0], h1[1], h2[0], h2[1]
    rec["resid"], rec["sum_sq"], rec["c_re"], rec["c_im"] = resid, sum_sq, cx, cy
    return rec


def expected(oracle_mod, result, y: np.ndarray, stream: int = 0) -> np.ndarray:
    """oracle Result of one trace + its matched-filter output -> the records of all RN16 windows in seq order"""
    dumps, open_idx, dc = result.dumps, result.open_idx, result.dc
    seq = np.flatnonzero(dumps["type"] == 0)
    assert not (seq & 1).any() and (seq == 2 * np.arange(len(seq))).all()
    dec = [handle_of_bits(dumps[k]["bits"]) for k in seq]
    with np.errstate(all="ignore"):
        rows = records(y, open_idx[seq], dc[seq], dumps["index"][seq], dumps["h_est"][seq, 0], dumps["h_est"][seq, 1], dec)
        for n in sorted({0, len(seq) - 1} if len(seq) else ()):
            k = seq[n]
            lit = record_literal(y, int(open_idx[k]), dc[k], int(dumps[k]["index"]), dumps[k]["h_est"][0], dumps[k]["h_est"][1], dec[n])
            assert lit.tobytes() == rows[n].tobytes(), (stream, k, lit, rows[n])
    rows["stream"], rows["seq"] = stream, seq
    return rows


def expected_batch(oracle_mod, results, ys):
    return [expected(oracle_mod, o, y, s) for s, (o, y) in enumerate(zip(results, ys))]


def expected_of(windows: np.ndarray, results: np.ndarray, literal: bool = True) -> np.ndarray:
    """caller-held DC-free windows [n][250] + their result records -> the records rfid_collisions_of must give (stream = 0,
    seq = the window's position); literal: the loop over scalars must agree on every one of them"""
    windows = np.ascontiguousarray(windows, dtype=np.complex64).reshape(-1, WIN)
    results = np.atleast_1d(results)
    n = len(windows)
    y = windows.reshape(-1)
    dec = [handle_of_bits((int(r["bits"][0]) >> np.arange(16)) & 1) for r in results]
    with np.errstate(all="ignore"):
        rows = records(y, WIN * np.arange(n), np.zeros(n, dtype=np.complex64), results["index"], results["h_re"], results["h_im"], dec)
        for k in range(n if literal else 0):
            lit = record_literal(y, WIN * k, 0, int(results[k]["index"]), results[k]["h_re"], results[k]["h_im"], dec[k])
            assert lit.tobytes() == rows[k].tobytes(), (k, lit, rows[k])
    rows["seq"] = np.arange(n)
    return rows


def fit(rows) -> np.ndarray:
    """resid / sum_sq in binary64 (nan where sum_sq == 0)"""
    rows = np.asarray(rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(rows["sum_sq"] != 0, rows["resid"].astype(np.float64) / rows["sum_sq"].astype(np.float64), np.nan)


# ---- the truth: what was on the air ------------------------------------------------------------------------------------------------
def sent(plan_slots: np.ndarray):
    """Trace.plan.slots -> per slot (n_tags, the list of the handles that were sent, bit 15 first)"""
    return [(int(s["n_tags"]), [int(v) for v in s["rn16"][: int(s["n_tags"])]]) for s in plan_slots]


def pair(rec) -> set:
    return {int(rec["rn16_a"]), int(rec["rn16_b"])}


def assert_equal(got, want, what="") -> None:
    """exact: integers equal, floats by bit pattern, then the bytes of the whole arrays"""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == capi.COLLISION_DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in capi.COLLISION_DTYPE.names if len(got) else ():
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][bad[:8]], want[name][bad[:8]])
    assert got.tobytes() == want.tobytes(), what

"""The window moments a pass must report (rfid_batch_slots: the five second-order sums of every window's first 240 gated samples),
worked out in numpy from the ORACLE alone (shared by tests/test_slots_emu.py and tests/test_gpu_slots.py): y = oracle.fir(raw), the
openings and dc_est of oracle.run_trace, then the definition of include/rfid_mi355x.h (rfid_window_moments) with every operation in
numpy.float32 -- numpy rounds each operation by itself and fuses nothing; numpy.add.accumulate over binary32 values adds in the order
of the axis, and the explicit leading 0.0f column is the sum's first operand (-0.0 as the first term gives +0.0).  Also an
independent binary64 restatement of rfid.batch.classify_slots, written as a loop over the slots."""
import math

import numpy as np

from rfid import _capi as capi

N = 240
F = np.float32


def one_window_slow(yr, yi, start, dc_re, dc_im):
    """the definition, literally: a Python loop over i, every operation one numpy.float32 operation, the sums from 0.0f"""
    dc_re, dc_im = F(dc_re), F(dc_im)
    sx = sy = sxx = sxy = syy = F(0.0)
    for i in range(N):
        x, y = F(F(yr[start + i]) - dc_re), F(F(yi[start + i]) - dc_im)
        sx = F(sx + x); sy = F(sy + y)
        sxx = F(sxx + F(x * x)); sxy = F(sxy + F(x * y)); syy = F(syy + F(y * y))
    return sx, sy, sxx, sxy, syy


def in_order(t):
    """[k][N] binary32 terms -> (((0.0f + t_0) + t_1) + ...) + t_{N-1} per row"""
    assert t.dtype == F
    lead = np.zeros((t.shape[0], 1), dtype=F)
    return np.add.accumulate(np.concatenate([lead, t], axis=1), axis=1, dtype=F)[:, -1]


def sums_of(x, y):
    """[k][N] binary32 samples -> the five sums, each [k]"""
    assert x.dtype == F and y.dtype == F and x.shape[1] == N
    return in_order(x), in_order(y), in_order(x * x), in_order(x * y), in_order(y * y)


def expected_windows(dumps, open_idx, dc, y, stream=0):
    """oracle dumps, openings and dc_est of one trace + the oracle's matched-filter output -> one record per window, in seq order"""
    n = len(open_idx)
    out = np.zeros(n, dtype=capi.MOMENTS_DTYPE)
    if n == 0:
        return out
    assert len(dumps) == n and len(dc) == n
    seq = np.arange(n)
    assert np.array_equal(dumps["type"], seq & 1)
    start = np.asarray(open_idx).astype(np.int64)
    assert (start >= 0).all() and (start + N <= len(y)).all()
    yr, yi = np.ascontiguousarray(y.real).astype(F), np.ascontiguousarray(y.imag).astype(F)
    dcs = np.asarray(dc).astype(np.complex64)
    dcr, dci = dcs.real.astype(F)[:, None], dcs.imag.astype(F)[:, None]
    idx = start[:, None] + np.arange(N, dtype=np.int64)[None, :]
    x, yy = yr[idx] - dcr, yi[idx] - dci
    out["stream"], out["seq"] = stream, seq
    out["sx"], out["sy"], out["sxx"], out["sxy"], out["syy"] = sums_of(x, yy)
    out["flags"] = np.where(seq & 1, 2 | (dumps["crc_ok"] & 1), 0)
    # the vectorised form against the literal one, on the first and the last window
    for k in {0, n - 1}:
        slow = one_window_slow(yr, yi, int(start[k]), dcr[k, 0], dci[k, 0])
        fast = tuple(out[f][k] for f in ("sx", "sy", "sxx", "sxy", "syy"))
        assert [F(v).tobytes() for v in slow] == [F(v).tobytes() for v in fast], (k, slow, fast)
    return out


def expected(result, y, stream=0):
    return expected_windows(result.dumps, result.open_idx, result.dc, y, stream)


def expected_batch(results, ys):
    return [expected(o, y, s) for s, (o, y) in enumerate(zip(results, ys))]


def expected_of(gated):
    """[k][240] complex64 gated (DC-free) samples -> the per-call records: dc = 0, stream = 0, seq = position, flags = 0"""
    g = np.ascontiguousarray(gated, dtype=np.complex64).reshape(-1, N)
    out = np.zeros(len(g), dtype=capi.MOMENTS_DTYPE)
    if len(g) == 0:
        return out
    x = np.ascontiguousarray(g.real).astype(F) - F(0.0)
    y = np.ascontiguousarray(g.imag).astype(F) - F(0.0)
    out["seq"] = np.arange(len(g))
    out["sx"], out["sy"], out["sxx"], out["sxy"], out["syy"] = sums_of(x, y)
    return out


def assert_equal(got, want, what="") -> None:
    """exact: integers equal, floats by bit pattern, then the bytes of the whole arrays"""
    assert got.dtype == capi.MOMENTS_DTYPE and len(got) == len(want), (what, len(got), len(want))
    for name in capi.MOMENTS_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got[name][bad[:8]], want[name][bad[:8]])
    assert got.tobytes() == want.tobytes(), what


# ---- the classification, restated: binary64, one slot at a time, nothing shared with rfid.batch -------------------------
def eig(rec):
    n = float(N)
    sx, sy = float(rec["sx"]), float(rec["sy"])
    cxx, cyy, cxy = float(rec["sxx"]) - sx * sx / n, float(rec["syy"]) - sy * sy / n, float(rec["sxy"]) - sx * sy / n
    tr, d = cxx + cyy, math.hypot(cxx - cyy, 2.0 * cxy)
    return (tr + d) / 2.0 / n, max((tr - d) / 2.0, 0.0) / n


def classify(rows, empty_k=3.0, collided_k=3.0):
    """-> list of (cls, answered, crc_ok, l1, l2, floor) per slot; cls -1 everywhere when there is no noise floor"""
    n_slots = len(rows) // 2
    if n_slots == 0:
        return []
    e = [eig(r) for r in rows[: 2 * n_slots]]
    minor = sorted(e[2 * k + 1][1] for k in range(n_slots))
    floor = minor[n_slots // 2] if n_slots & 1 else 0.5 * (minor[n_slots // 2 - 1] + minor[n_slots // 2])
    out = []
    for k in range(n_slots):
        (l1, l2), (a1, _) = e[2 * k], e[2 * k + 1]
        crc_ok = int(rows["flags"][2 * k + 1]) & 1
        if not (math.isfinite(floor) and floor > 0.0):
            out.append((-1, 0, crc_ok, l1, l2, floor))
            continue
        cls = 0 if l1 <= empty_k * floor else (2 if l2 > collided_k * floor else 1)
        out.append((cls, int(a1 > empty_k * floor), crc_ok, l1, l2, floor))
    return out


def truth(slots):
    """rfid.synth SlotTruth records -> (cls, answered) per slot: min(n_tags, 2), an EPC frame was sent"""
    return [(min(int(s.n_tags), 2), int(s.epc is not None)) for s in slots]


# the five shapes of the classification check: (fixed_q, tag ids, rounds, seed)
SHAPES = ((2, (0x11, 0x22, 0x33, 0x44, 0x55), 12, 1),
          (0, (0x27,), 8, 7),
          (1, (1, 2, 3, 4, 5), 12, 2),
          (3, (1, 2, 3), 6, 4),
          (2, (1, 2, 3, 4), 4, 11))


def shape_trace(synth_mod, shape, sigma=0.01):
    q, tags, rounds, seed = shape
    return synth_mod.make_trace(n_rounds=rounds, fixed_q=q, tag_ids=tags, seed=seed, sigma=sigma)

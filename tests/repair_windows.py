"""Crafted EPC windows for the repair search (rfid_repair_window; shared by tests/test_repair_emu.py and tests/test_gpu_repair.py): the
noise-free valid frames of tests/decoder_windows.py (samples 0 or 10-5j, h_est = 10-5j, every decision value +-125) with chosen
decisions made weak, wrong or exactly 0 by rewriting the first of their two half-bit samples: s_a = s_b + e gives
r_j = Re(e conj(h_est)), an exact small integer (e = k (2-1j): 25 k; e = 0: 0, which decides "low").  Every window is decoded by the
oracle again and `check` asserts from tests/repair_ref.py alone that each set still has the property it is there for."""
import itertools

import numpy as np

import decoder_windows as dw
import repair_ref as ref

F = np.float32
UNIT = np.complex64(2 - 1j)        # Re(UNIT conj(10-5j)) = 25


def _positions(dump):
    T, idx = F(dump["T"]), F(int(dump["index"]))
    j = np.arange(128)
    return (j.astype(F) * (F(2) * T) + idx).astype(np.int64), (((j * 2).astype(F) * T + T) + idx).astype(np.int64)


def craft(oracle_mod, frame, edits):
    """frame: index into valid_frames(EPC).  edits: {decision j: (k, wrong)} -- |r_j| = 25 k, reversed when `wrong`.
    -> (window, the oracle's dump of it, r of the window, the decisions that are wrong now)"""
    w0 = dw.valid_frames(dw.EPC)[frame][0]
    d0 = oracle_mod.decode_window(w0, dw.EPC)
    r0 = dw.decisions(w0, d0)
    assert d0["crc_ok"] == 1 and (np.abs(r0) == 125).all()
    ia, ib = _positions(d0)
    w = w0.copy()
    wrong = []
    for j, (k, bad) in edits.items():
        was = r0[j] > 0
        now = (not was) if bad else was
        w[ia[j]] = w[ib[j]] + (UNIT * F(k) if now else -UNIT * F(k))
        if (k > 0 and bad) or (k == 0 and was):        # (r == 0 decides "low": wrong where the decision was "high")
            wrong.append(j)
    d = oracle_mod.decode_window(w, dw.EPC)
    assert d["index"] == d0["index"] and d["T"].tobytes() == d0["T"].tobytes(), "the edits moved the sync index or the half period"
    r = dw.decisions(w, d)
    assert np.array_equal(ref.bits_of_signs(r), d["bits"])
    assert sorted(np.flatnonzero((r > 0) != (r0 > 0)).tolist()) == sorted(wrong)
    return w, d, r, sorted(wrong)


# ---- CRC arithmetic for crafting only (expected values never come from here) ------------------------------------------
def _syndrome(bits) -> int:
    reg = 0xFFFF
    for b in bits[:112]:
        msb = (reg >> 15) & 1
        reg = (reg << 1) & 0xFFFF
        if msb ^ int(b):
            reg ^= 0x1021
    rcvd = int("".join(str(int(b)) for b in bits[112:128]), 2)
    return (~reg & 0xFFFF) ^ rcvd


def equal_cost_pair(r0, gap=3):
    """two disjoint sets of up to three decisions, the first among the "high" decisions (r0 > 0) and the second among the "low" ones,
    whose toggles together form a CRC codeword: with all of them at r = 0 the first are wrong, the second right, and reversing
    either set makes the frame pass at cost 0.  -> (S1, S2) or None"""
    zero = np.zeros(128, dtype=np.uint8)
    s0 = _syndrome(zero)
    col = [_syndrome(ref.toggled(zero, [j])) ^ s0 for j in range(128)]
    hi = [j for j in range(2, 126, gap) if r0[j] > 0]
    lo = [j for j in range(3, 126, gap) if not r0[j] > 0]
    table = {}
    for n in (1, 2, 3):
        for c in itertools.combinations(lo, n):
            x = 0
            for j in c:
                x ^= col[j]
            table.setdefault(x, c)
    for n in (1, 2, 3):
        for c in itertools.combinations(hi, n):
            x = 0
            for j in c:
                x ^= col[j]
            if x in table and all(abs(a - b) > 1 for a in c for b in table[x]):
                return list(c), list(table[x])
    return None


def build(oracle_mod):
    """name -> (window, dump, expected record, r, wrong decisions)"""
    out = {}

    def add(name, frame, edits):
        w, d, r, wrong = craft(oracle_mod, frame, edits)
        out[name] = (w, d, ref.expected_window(oracle_mod, w, d), r, wrong)

    r0 = lambda f: dw.decisions(dw.valid_frames(dw.EPC)[f][0], oracle_mod.decode_window(dw.valid_frames(dw.EPC)[f][0], dw.EPC))
    # (a) ten decisions of exactly 0: the two lowest were "high" (now wrong), the eight behind them were "low" (still right)
    r = r0(3)
    hi = [j for j in range(4, 40, 3) if r[j] > 0][:2]
    lo = [j for j in range(hi[-1] + 3, 127, 3) if not r[j] > 0][:8]
    out_a = {j: (0, False) for j in hi + lo}
    add("zeros", 3, out_a)
    # (b) the last decision alone, weak and wrong
    add("last", 5, {127: (1, True)})
    # (c) two sets of equal cost that both pass
    for f in range(15):
        pair = equal_cost_pair(r0(f))
        if pair:
            add("equal", f, {j: (0, False) for j in pair[0] + pair[1]})
            break
    # (d) four weak wrong decisions: out of reach
    add("four", 8, {11: (1, True), 47: (1, True), 80: (2, True), 119: (2, True)})
    # three wrong decisions that are NOT the weakest: five right ones are weaker, all eight are candidates
    add("decoys", 11, {9: (2, True), 60: (3, True), 101: (2, True), 20: (1, False), 33: (1, False), 64: (1, False), 90: (1, False),
                       126: (1, False)})
    # a frame that verifies: nothing is searched
    w, bits, _ = dw.valid_frames(dw.EPC)[0]
    d = oracle_mod.decode_window(w, dw.EPC)
    out["verified"] = (w, d, ref.expected_window(oracle_mod, w, d), dw.decisions(w, d), [])
    return out


def check(oracle_mod, sets):
    """each set still has its property, by the reference alone"""
    w, d, rec, r, wrong = sets["zeros"]
    zeros = np.flatnonzero(r == 0)
    assert len(zeros) >= 9 and d["crc_ok"] == 0 and len(wrong) == 2
    assert wrong == zeros[:2].tolist() and not set(wrong) & set(zeros[-8:].tolist())      # ("larger j first" would leave them out)
    assert rec["n_flips"] == 2 and ref.flip_list(rec) == wrong and rec["cost"] == 0
    w, d, rec, r, wrong = sets["last"]
    assert wrong == [127] and d["crc_ok"] == 0 and rec["n_flips"] == 1 and ref.flip_list(rec) == [127] and rec["cost"] == 25
    assert np.array_equal(ref.toggled(d["bits"], [127])[:127], d["bits"][:127])
    if "equal" in sets:
        w, d, rec, r, wrong = sets["equal"]
        ok = ref.passing(oracle_mod, r, d["bits"])
        assert d["crc_ok"] == 0 and len(ok) >= 2 and len({p[0].tobytes() for p in ok}) == 1, ok
        assert sorted(p[2] for p in ok)[0] != sorted(p[2] for p in ok)[1]
        assert ref.flip_list(rec) == min(ok, key=lambda p: p[1])[2] and rec["cost"] == 0
    w, d, rec, r, wrong = sets["four"]
    assert len(wrong) == 4 and d["crc_ok"] == 0 and rec["n_flips"] == 0 and rec["flips"] == -1
    assert sorted(np.argsort(np.abs(r), kind="stable")[:4].tolist()) == wrong       # (the four weakest: they ARE candidates)
    w, d, rec, r, wrong = sets["decoys"]
    assert rec["n_flips"] == 3 and ref.flip_list(rec) == wrong == [9, 60, 101] and rec["cost"] == 175
    assert sorted(np.argsort(np.abs(r), kind="stable")[:5].tolist()) == [20, 33, 64, 90, 126]
    w, d, rec, r, wrong = sets["verified"]
    assert d["crc_ok"] == 1 and rec["flags"] == 1 and rec["n_flips"] == 0

"""The records the stack stage must report (rfid_batch_stack / rfid_stack_windows: an unknown tag's repeated EPC frames, found among the
CRC-failed windows of a trace by the correlation of their decision values and combined before the sign is taken), worked out from the
ORACLE alone (shared by tests/test_stack_emu.py and tests/test_gpu_stack.py): y = oracle.fir(raw), the window s = y[open_idx[k] : + 1370]
- dc[k] per component, T, index and h from the window's dump, the CRC by the oracle's check_crc.  The definition of
include/rfid_mi355x.h (rfid_stack) is restated twice, every operation one numpy.float32 operation: `block` works on arrays (all
pairs of a block at once, the sums as numpy.add.accumulate from a leading 0.0f), `anchor_literal` is the definition as a Python loop
over scalars with the CRC written out.  `expected_rows` and `expected_windows` assert the two equal on the first and the last combined
row they meet."""
import numpy as np

from match_ref import decision_values, in_order, pack, unpack, window_of
from rfid import _capi as capi

F = np.float32
EPC_WIN, BLOCK = 1370, 64
assert (BLOCK, 64) == (capi.STACK_BLOCK, capi.STACK_MAX_WINDOWS)
DTYPE = capi.STACK_DTYPE
READ, FORMED, PASS = 1, 2, 4
FLOATS = ("sig_abs", "margin_min")


def _sums(t):
    """[..., 128] float32 -> the in-order sums from a leading 0.0f over the last axis"""
    t = np.asarray(t, dtype=F)
    lead = np.zeros(t.shape[:-1] + (1,), dtype=F)
    out = np.add.accumulate(np.concatenate([lead, t], axis=-1), axis=-1, dtype=F)[..., -1]
    assert out.dtype == F
    return out


def partners_of(r, rho_min) -> np.ndarray:
    """r: [n][128] the decision values of a block's rows -> bool [n][n]: g is a partner of f"""
    r = np.asarray(r, dtype=F)
    p = r[:, None, :] * r[None, :, :]
    assert p.dtype == F
    s, a = _sums(p), _sums(np.abs(p))
    need = F(rho_min) * a
    assert need.dtype == F
    with np.errstate(invalid="ignore"):
        out = (s > 0) & (s >= need)
    np.fill_diagonal(out, False)
    return out


def combine(oracle_mod, r, members) -> dict:
    """the members' rows added in ascending ordinal, then the decoder's sign chain and CRC"""
    R = np.add.accumulate(np.concatenate([np.zeros((1, 128), dtype=F), np.asarray(r, dtype=F)[sorted(members)]]), axis=0, dtype=F)[-1]
    assert R.dtype == F
    cur = R > 0
    bits = (cur != np.concatenate([[True], cur[:-1]])).astype(np.uint8)
    data = np.packbits(bits)                                              # (MSB first)
    calc = int(oracle_mod.lib().orc_crc16_bytes(data[:14].tobytes(), 14)) & 0xFFFF
    ok = oracle_mod.lib().orc_check_crc(bytes(48 + int(b) for b in bits), 128) == 1
    assert ok == (calc == ((int(data[14]) << 8) | int(data[15])))
    mag = np.abs(R)
    return dict(bits=bits, passes=bool(ok), sig_abs=in_order(mag), margin=F(mag.min()), weakest=int(np.argmin(mag)))


def block(oracle_mod, r, rho_min) -> list:
    """the definition on arrays.  r: [n][128] -> per row (mask, n_partners, what combine found or None)"""
    part = partners_of(r, rho_min) if len(r) > 1 else np.zeros((len(r), len(r)), dtype=bool)
    out = []
    for i in range(len(r)):
        who = [int(g) for g in np.flatnonzero(part[i])]
        mask = sum(1 << g for g in who) | (1 << i)
        out.append((mask, len(who), combine(oracle_mod, r, who + [i]) if who else None))
    return out


def anchor_literal(r, i, rho_min):
    """the definition as written, for row i of a block: loops over rows and decisions, scalars throughout, the CRC byte by byte"""
    r = [[F(v) for v in row] for row in r]
    rho = F(rho_min)
    members = []
    for g in range(len(r)):
        if g == i:
            members.append(g)
            continue
        s = a = F(0.0)
        for j in range(128):
            p = F(r[i][j] * r[g][j])
            s = F(s + p)
            a = F(a + F(abs(p)))
        if s > 0 and s >= F(rho * a):
            members.append(g)
    mask = sum(1 << g for g in members)
    if len(members) == 1:
        return mask, 0, None
    prev, bits = True, []
    margin, weakest, sig = None, 0, F(0.0)
    for j in range(128):
        R = F(0.0)
        for m in members:
            R = F(R + r[m][j])
        cur = bool(R > 0)
        bits.append(1 if cur != prev else 0)
        prev = cur
        mag = F(abs(R))
        sig = F(sig + mag)
        if margin is None or mag < margin:
            margin, weakest = mag, j
    data = [sum(bits[8 * b + k] << (7 - k) for k in range(8)) for b in range(16)]
    crc = 0xFFFF
    for b in data[:14]:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    crc ^= 0xFFFF
    return mask, len(members) - 1, dict(bits=np.array(bits, dtype=np.uint8), passes=crc == ((data[14] << 8) | data[15]), sig_abs=sig,
                                        margin=F(margin), weakest=weakest)


def same(a, b) -> bool:
    if a[:2] != b[:2] or (a[2] is None) != (b[2] is None):
        return False
    return a[2] is None or (a[2].keys() == b[2].keys() and all(np.asarray(a[2][k]).tobytes() == np.asarray(b[2][k]).tobytes() for k in a[2]))


def _fill(rec, ordinal, found) -> None:
    mask, n_partners, comb = found
    rec["ordinal"], rec["member_mask"], rec["n_partners"] = ordinal, mask, n_partners
    if comb is not None:
        rec["flags"] = FORMED | (PASS if comb["passes"] else 0)
        rec["sig_abs"], rec["margin_min"], rec["weakest"], rec["frame"] = comb["sig_abs"], comb["margin"], comb["weakest"], pack(comb["bits"])


def _blocks(oracle_mod, recs, r, rho_min, what) -> None:
    """recs: the records of the failed rows in ordinal order, r: [F][128] their decision values"""
    r = np.asarray(r, dtype=F).reshape(-1, 128)
    checks = []
    for f0 in range(0, len(r), BLOCK):
        rb = r[f0:f0 + BLOCK]
        found = block(oracle_mod, rb, rho_min)
        for l, fd in enumerate(found):
            _fill(recs[f0 + l], f0 + l, fd)
            if fd[2] is not None:
                checks.append((rb, l, fd))
    for rb, l, fd in checks[:1] + checks[-1:]:
        assert same(fd, anchor_literal(rb, l, rho_min)), (what, l)


def expected_rows(oracle_mod, result, y: np.ndarray, stream: int = 0, rho_min=0.5):
    """the oracle Result of one trace + its matched-filter output -> the records of all its EPC windows in seq order"""
    dumps, open_idx = result.dumps, result.open_idx
    seq = np.flatnonzero(dumps["type"] == 1)
    assert (seq & 1).all() and len(seq) == len(dumps) // 2
    rows = np.zeros(len(seq), dtype=DTYPE)
    failed, r = [], []
    for n, k in enumerate(seq):
        rec, d = rows[n], dumps[k]
        rec["stream"], rec["seq"], rec["start"] = stream, k, int(open_idx[k])
        if d["crc_ok"] == 1:
            rec["flags"], rec["ordinal"] = READ, -1
            continue
        s_re, s_im = window_of(y, int(open_idx[k]), result.dc[k])
        r.append(decision_values(s_re, s_im, d["T"], int(d["index"]), d["h_est"][0], d["h_est"][1]))
        failed.append(n)
    _blocks(oracle_mod, [rows[n] for n in failed], r, rho_min, stream)
    return rows


def expected_windows(oracle_mod, spans, results, rho_min=0.5) -> np.ndarray:
    """caller-held DC-free spans (n, 1370) + the windows' result records -> the records rfid_stack_windows must give"""
    spans = np.ascontiguousarray(spans, dtype=np.complex64)
    n = len(spans)
    assert spans.shape == (n, EPC_WIN) and len(results) == n and 1 <= n <= BLOCK and all(int(q["type"]) == 1 for q in results)
    rows = np.zeros(n, dtype=DTYPE)
    failed, r = [], []
    for i, (sp, q) in enumerate(zip(spans, results)):
        if int(q["crc_ok"]) == 1:
            rows[i]["flags"], rows[i]["ordinal"] = READ, -1
            continue
        s_re, s_im = window_of(sp, 0, 0)
        r.append(decision_values(s_re, s_im, q["T"], int(q["index"]), q["h_re"], q["h_im"]))
        failed.append(i)
    _blocks(oracle_mod, [rows[i] for i in failed], r, rho_min, "windows")
    return rows


def members_of(rec) -> list:
    """the ordinals of a record's members"""
    base = (int(rec["ordinal"]) // BLOCK) * BLOCK
    return [base + l for l in range(BLOCK) if (int(rec["member_mask"]) >> l) & 1]


def frame_bits(rec) -> np.ndarray:
    return unpack(rec["frame"])


def assert_symmetric(rows) -> None:
    """g in members(f) <=> f in members(g), over the failed rows of one trace"""
    failed = rows[(rows["flags"] & READ) == 0]
    assert list(failed["ordinal"]) == list(range(len(failed)))
    sets = [set(members_of(q)) for q in failed]
    for f, who in enumerate(sets):
        assert f in who and len(who) == int(failed[f]["n_partners"]) + 1 and all(f // BLOCK == g // BLOCK for g in who), f
        assert all(f in sets[g] for g in who), f
        assert bool(failed[f]["flags"] & FORMED) == (len(who) > 1) and (failed[f]["flags"] & FORMED or not failed[f]["flags"]), f


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

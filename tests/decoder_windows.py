"""Crafted tag_decoder windows: the inputs on which the reference's comparison operators decide.

tag_sync keeps the FIRST of equal correlation maxima (`if (corr > max)` from max = 0: offset 0 when nothing exceeds 0,
tag_decoder_impl.cc:85-99), std::max_element the FIRST of equal energies (:165), and a half-bit difference of exactly 0
decides "low" (`result > 0`, :125,176).  Noisy traces never produce an equal pair, so these windows are built to: small
integers make every sum exact.  All of them are seeded and fixed; `check_*` assert each set's properties from the ORACLE's
scores before a kernel sees it, so a set that lost its ties fails instead of testing nothing.

Windows are complex64, DC-free as the decoder block sees them: 250 samples (type 0, RN16) or 1370 (type 1, EPC)."""
import numpy as np

from rfid import synth
from rfid.context import unpack_bits

RN16, EPC = 0, 1
WLEN = {RN16: 250, EPC: 1370}
N_LATTICE = 256
LATTICE_SEED = {RN16: 1, EPC: 1}
# floors of the lattice sets (windows out of 256): a tied sync maximum > 0, a tied energy maximum, a decision of exactly 0
MIN_SYNC_TIES, MIN_ENERGY_TIES, MIN_ZERO_DECISIONS = 20, 10, 200


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def lattice(type_):
    """[256][wlen]: real and imaginary parts drawn from {-1, 0, 1}"""
    rng = np.random.default_rng(LATTICE_SEED[type_])
    v = rng.integers(-1, 2, size=(N_LATTICE, WLEN[type_], 2)).astype(np.float32)
    return np.ascontiguousarray(v).view(np.complex64)[..., 0]      # (no arithmetic: every zero is +0)


def degenerate(type_):
    """name -> window.
    zero:     nothing exceeds 0 -> offset 0 (not a tie above 0)
    constant: every correlation and every energy equal
    period7:  offsets t and t + 7 see the same samples: pairwise ties
    first38:  unit-magnitude samples up to 38 behind the sync index, zero from there on.  For every half-period candidate
              T in [4.95, 5.05] the gathers i = 0..7 land inside (7 T < 36) and i >= 8 outside (8 T > 39), so all 20
              energies are 8 exactly, while the phases are drawn until the sync peak is unique."""
    n = WLEN[type_]
    out = {"zero": np.zeros(n, dtype=np.complex64),
           "constant": np.full(n, np.complex64(3 - 2j), dtype=np.complex64)}
    rng = np.random.default_rng(7 + type_)
    pat = (rng.integers(-2, 3, 7) + 1j * rng.integers(-2, 3, 7)).astype(np.complex64)
    out["period7"] = np.ascontiguousarray(pat[np.arange(n) % 7])
    taps = np.array([0, 5, 15, 30, 50, 55])
    for _ in range(100):
        w = np.zeros(n, dtype=np.complex64)
        w[:120] = np.array([1, -1, 1j, complex(0, -1)], dtype=np.complex64)[rng.integers(0, 4, 120)]   # (-1j is -0 - 1j)
        corr = np.array([abs(w[t + taps].sum()) ** 2 for t in range(15)])
        if (corr == corr.max()).sum() == 1:
            w[65 + int(np.argmax(corr)) + 38:] = 0
            out["first38"] = w
            break
    return out


def fm0_window(type_, bits, offset, h=np.complex64(2 - 1j)):
    """A noise-free FM0 reply whose preamble peak sits at sample `offset` (0..14 -> sync index 65 + offset): half-bit
    levels of 5 samples, smoothed by the 5-sample boxcar the matched filter is (ramps 0..5 between the levels: small
    integers), times h, on a zero background."""
    lv = synth.fm0_levels(bits)
    sq = np.repeat(lv, 5)
    sm = np.convolve(sq, np.ones(5, dtype=np.float32))          # sm[k] = sum sq[k-4..k]: full level 4 samples into a half-bit
    w = np.zeros(WLEN[type_] + len(sm) + 32, dtype=np.float32)
    # the sync taps (0, 5, 15, 30, 50, 55 behind an offset) all read a full level only at the fifth sample of the half-bits
    start = offset - 4
    if start >= 0:
        w[start:start + len(sm)] = sm
    else:
        w[:len(sm) + start] = sm[-start:]
    return np.ascontiguousarray(w[:WLEN[type_]] * h, dtype=np.complex64)


def valid_frames(type_):
    """[(window, bits, tag_id)] for sync offsets 0..14: EPC frames with a good CRC-16 (random PC / EPC bits, the tag id in
    frame bits 104..111) or, for type 0, random RN16s"""
    rng = np.random.default_rng(2024 + type_)
    out = []
    for m in range(15):
        if type_ == EPC:
            tag_id = int(rng.integers(0, 256))
            bits = synth.epc_frame(synth.epc_for_id(tag_id, rng), pc=rng.integers(0, 2, 16).tolist())
        else:
            tag_id, bits = -1, rng.integers(0, 2, 16).tolist()
        out.append((fm0_window(type_, bits, m), np.array(bits, dtype=np.uint8), tag_id))
    return out


def decisions(win, dump):
    """the half-bit differences the decisions are taken on (tag_decoder_impl.cc:125,176), from the oracle's index, h_est and
    T, in the reference's binary32 order -> float32[n_bits]"""
    f = np.float32
    idx = f(int(dump["index"]))
    hre, ci = f(dump["h_est"][0]), -f(dump["h_est"][1])
    if int(dump["type"]) == RN16:
        pa = int(dump["index"]) + 10 * np.arange(16)
        pb = pa + 5
    else:
        T = f(dump["T"])
        j = np.arange(128)
        pa = (j.astype(f) * (f(2) * T) + idx).astype(np.int64)
        pb = (((j * 2).astype(f) * T + T) + idx).astype(np.int64)
    d = win[pa] - win[pb]
    return d.real.astype(f) * hre - d.imag.astype(f) * ci


def set_properties(wins, dumps):
    """counts over a set, from the oracle's scores"""
    sync_tie = energy_tie = zero_dec = 0
    offsets, cands = set(), set()
    for w, d in zip(wins, dumps):
        c, e = d["corr"], d["energy"]
        if c.max() > 0 and (c == c.max()).sum() > 1:
            sync_tie += 1
        offsets.add(int(d["index"]) - 65)
        if int(d["type"]) == EPC:
            if (e == e.max()).sum() > 1:
                energy_tie += 1
            cands.add(int(np.argmax(e)))
        if (decisions(w, d) == 0).any():
            zero_dec += 1
    return dict(sync_tie=sync_tie, energy_tie=energy_tie, zero_decision=zero_dec, offsets=offsets, candidates=cands)


def check_lattice(type_, wins, dumps):
    p = set_properties(wins, dumps)
    assert p["sync_tie"] >= MIN_SYNC_TIES, p
    assert p["zero_decision"] >= MIN_ZERO_DECISIONS, p
    assert p["offsets"] == set(range(15)), p
    if type_ == EPC:
        assert p["energy_tie"] >= MIN_ENERGY_TIES, p
        assert p["candidates"] == set(range(20)), p
    return p


def check_degenerate(type_, wins, dumps):
    d = dict(zip(wins.keys(), dumps))
    z, c, p7, f38 = d["zero"], d["constant"], d["period7"], d["first38"]
    assert not z["corr"].any() and z["index"] == 65 and not z["h_est"].any()
    assert c["corr"][0] > 0 and (c["corr"] == c["corr"][0]).all() and c["index"] == 65
    assert p7["corr"].max() > 0 and _bits_equal(p7["corr"][:8], p7["corr"][7:])
    assert (f38["corr"] == f38["corr"].max()).sum() == 1 and f38["corr"].max() > 0
    assert (decisions(wins["first38"], f38)[4:] == 0).all()
    if type_ == EPC:
        assert not z["energy"].any() and z["T"] == np.float32(4.95)
        assert c["energy"][0] > 0 and (c["energy"] == c["energy"][0]).all() and c["T"] == np.float32(4.95)
        assert (f38["energy"] == 8).all() and f38["T"] == np.float32(4.95)


def check_valid_frames(type_, frames, dumps):
    for m, ((w, bits, tag_id), d) in enumerate(zip(frames, dumps)):
        assert d["index"] == 65 + m, (m, d["index"])
        assert (d["corr"] == d["corr"].max()).sum() == 1
        assert np.array_equal(d["bits"][: len(bits)], bits), m
        if type_ == EPC:
            assert d["crc_ok"] == 1 and d["tag_id"] == tag_id, m


class Sets:
    """every crafted window of both types with the oracle's answer, built once (a session fixture's worth)"""

    def __init__(self, oracle_mod):
        self.wins = {RN16: [], EPC: []}
        self.names = {RN16: [], EPC: []}
        self.dumps = {RN16: [], EPC: []}
        self.known = {RN16: {}, EPC: {}}          # index into wins -> (bits, tag_id) of the valid frames
        self.properties = {}
        for t in (RN16, EPC):
            lat = lattice(t)
            ld = [oracle_mod.decode_window(w, t) for w in lat]
            self.properties[t] = check_lattice(t, lat, ld)
            deg = degenerate(t)
            dd = [oracle_mod.decode_window(w, t) for w in deg.values()]
            check_degenerate(t, deg, dd)
            fr = valid_frames(t)
            fd = [oracle_mod.decode_window(w, t) for w, _, _ in fr]
            check_valid_frames(t, fr, fd)
            for name, w, d in ([("lattice%d" % i, w, d) for i, (w, d) in enumerate(zip(lat, ld))] +
                               [(n, w, d) for (n, w), d in zip(deg.items(), dd)] +
                               [("frame@%d" % m, f[0], d) for m, (f, d) in enumerate(zip(fr, fd))]):
                if name.startswith("frame@"):
                    m = int(name[6:])
                    self.known[t][len(self.wins[t])] = (fr[m][1], fr[m][2])
                self.names[t].append(name)
                self.wins[t].append(np.ascontiguousarray(w, dtype=np.complex64))
                self.dumps[t].append(d)

    def pick(self, type_, k):
        """the k-th window of a type, cycling -> (window, dump, name)"""
        i = k % len(self.wins[type_])
        return self.wins[type_][i], self.dumps[type_][i], self.names[type_][i]


_sets = None


def sets(oracle_mod):
    global _sets
    if _sets is None:
        _sets = Sets(oracle_mod)
    return _sets


def compare_window(res, sc, dump, what=""):
    """one result (+ scores) record with the oracle's dump of the same window, bit for bit: index, h_est, corr, energy, T,
    bits, crc_ok, tag_id (-1 unless the CRC holds: include/rfid_mi355x.h)"""
    t = int(dump["type"])
    assert res["type"] == t and res["index"] == dump["index"], (what, int(res["index"]), int(dump["index"]))
    assert res["n_bits"] == dump["n_bits"] == (128 if t else 16), what
    assert _bits_equal([res["h_re"], res["h_im"]], dump["h_est"]), ("h_est", what)
    assert _bits_equal(res["T"], dump["T"]), ("T", what, float(res["T"]), float(dump["T"]))
    n = int(dump["n_bits"])
    assert np.array_equal(unpack_bits(res["bits"], n), dump["bits"][:n]), ("bits", what)
    assert np.array_equal(unpack_bits(res["bits"], 128)[n:], np.zeros(128 - n, np.uint8)), ("bits behind the frame", what)
    assert res["crc_ok"] == dump["crc_ok"], ("crc_ok", what)
    assert res["tag_id"] == (dump["tag_id"] if dump["crc_ok"] else -1), ("tag_id", what)
    if sc is not None:
        assert _bits_equal(sc["corr"], dump["corr"]), ("corr", what)
        assert _bits_equal(sc["energy"], dump["energy"]), ("energy", what)


def drive_decoder_work(ctx, oracle_mod, s, n_pairs):
    """rfid_decoder_work on crafted windows, RN16 and EPC in turn as the reader state demands (the gate call without input
    arms n_samples_to_ungate, gate_impl.cc:112-123), the oracle's decoder and reader stepped alongside: results, scores,
    port-0 bits and the reader state equal after every call.  -> windows decoded"""
    sim = oracle_mod.BlockSim()
    n = 0

    def reader(q):
        for _ in range(8):
            before = ctx.state().gen2_logic_status
            if before == 3:
                break
            ctx.reader_work(q)
            q = 0
            if ctx.state().gen2_logic_status == before:
                break

    reader(0)
    sim.reader_until_idle(0)
    for k in range(n_pairs):
        for type_ in (RN16, EPC):
            st = ctx.state()
            assert st.decoder_status == type_ == sim.state.decoder_status
            assert st.gate_status == (3 if type_ else 2) == sim.state.gate_status
            ctx.gate_work(np.zeros(0, dtype=np.complex64))
            sim.arm_gate()
            w, dump, name = s.pick(type_, k)
            cons, bits, res, sc = ctx.decoder_work(w)
            ocons, obits, odump = sim.decoder_work(w)
            assert cons == ocons == WLEN[type_], name
            assert np.array_equal(bits, obits), name
            compare_window(res, sc, dump, name)
            assert odump.tobytes() == dump.tobytes(), name      # (the decoder keeps nothing from window to window)
            reader(len(bits))
            sim.reader_until_idle(len(obits))
            st, so = ctx.state(), sim.state
            for f in ("status", "gen2_logic_status", "gate_status", "decoder_status", "n_queries_sent", "cur_inventory_round",
                      "cur_slot_number", "n_epc_correct", "n_unique_tags"):
                assert getattr(st, f) == getattr(so, f), (f, name)
            assert list(st.tag_reads) == list(so.tag_reads), name
            n += 1
    return n


def shifted(win, dc):
    """float32(dc + win), what a window looks like in the matched filter's output in front of the gate -- asserted to give
    the window back bit for bit when the decoder subtracts dc (integers below the next binade of dc do)"""
    dc = np.complex64(dc)
    y = np.empty(len(win), dtype=np.complex64)
    y.real = win.real + dc.real
    y.imag = win.imag + dc.imag
    back = np.empty(len(win), dtype=np.complex64)
    back.real = y.real - dc.real
    back.imag = y.imag - dc.imag
    assert np.array_equal(back.view(np.uint32), np.ascontiguousarray(win).view(np.uint32)), "dc + w - dc != w"
    return y


def layout(items, slots, window_dtype, gap=3):
    """items: [(type, window)]; slots: their result slots (seq).  -> (y, window records): the windows laid out one behind
    the other in one row, `gap` samples apart, each on a dc of its own (small integers; 0 for a window that is not made of
    integers, which no other dc would give back exactly)"""
    recs = np.zeros(len(items), dtype=window_dtype)
    parts, pos = [], 0
    for k, ((type_, w), slot) in enumerate(zip(items, slots)):
        integral = np.array_equal(w.real, np.round(w.real)) and np.array_equal(w.imag, np.round(w.imag))
        dc = np.complex64(complex(k % 5 - 2, k % 3 - 1) * 4 if integral else 0)
        recs[k] = (0, slot, pos + gap, type_, dc.real, dc.imag)
        parts += [np.full(gap, np.complex64(77 - 55j)), shifted(w, dc)]
        pos += gap + len(w)
    parts.append(np.full(gap, np.complex64(77 - 55j)))
    return np.concatenate(parts).astype(np.complex64), recs


# ---- a clean trace: its empty and collided slots are constant windows -------------------------------------------------

CLEAN_KW = dict(n_rounds=3, fixed_q=2, tag_ids=(0x27,), sigma=0.0, noise=False, seed=4)


def clean_trace(oracle_mod, synth_mod):
    """-> (samples, oracle result), with the ties asserted from the oracle: at least 12 windows whose 15 correlations are all
    equal and greater than 0, at least 6 EPC windows whose 20 energies are all equal"""
    t = synth_mod.make_trace(**CLEAN_KW).samples
    o = oracle_mod.run_trace(t, oracle_mod.config(fixed_q=2))
    d = o.dumps
    sync15 = sum(1 for x in d if x["corr"][0] > 0 and (x["corr"] == x["corr"][0]).all())
    energy20 = sum(1 for x in d if x["type"] == 1 and (x["energy"] == x["energy"][0]).all())
    print("clean trace: %d windows, %d with a 15-way sync tie, %d of %d EPC windows with a 20-way energy tie" %
          (o.n_windows, sync15, energy20, int((d["type"] == 1).sum())))
    assert o.n_windows == 24 and sync15 >= 12 and energy20 >= 6, (o.n_windows, sync15, energy20)
    return t, o

"""What the fine stage's cases (tests/fine_suite.py, on both sides; tests/test_fine_emu.py and tests/test_gpu_fine.py, on one) are built
from: their small inputs, with what the ORACLE alone says about them, the plan and the check that are the same wherever the records
come from, and the crafted windows of the per-call form (rfid_fine_window) with the checks on them.  Everything expected comes from
tests/fine_ref.py, i.e. from the oracle alone.

The traces are FIXED_Q = 2, tags (0x27, 0x27, 0x31), sigma = 0.02: a third of the slots are empty or collided, and the reference ACKs
every one of them.  4, 3, 2 and 3 inventory rounds: 16, 12, 8 and 12 EPC windows -- a trace's rows fill two packs of eight, one and a
half, or one."""
import numpy as np
import pytest

import decoder_windows as dw
import fine_ref as ref
import repair_ref
from stage_backend import lay_out, oracle_pass

TAGS = (0x27, 0x27, 0x31)
SEEDS = ((104, 4), (112, 3), (120, 2), (128, 3))       # (seed, inventory rounds) per trace
PHIS = (0.0, 0.3, 0.6)         # phase a frame gains over its 1370 samples
SEG_SPAN = 1120.0              # samples between the centres of segments 0 and 7: 7 x 16 bits x 10 samples


def ragged_batch(oracle_mod, synth_mod):
    """-> (host, lens, L, stride, oracle Results, matched-filter outputs, (packed, rows)) of the four traces, the first cut short"""
    ts = [synth_mod.make_trace(n_rounds=n, fixed_q=2, tag_ids=TAGS, seed=seed, sigma=0.02, t1_jitter_raw=3).samples for seed, n in SEEDS]
    host, lens, L, stride = lay_out(ts, shorten=777)
    refs, ys = oracle_pass(oracle_mod, host, lens, 2)
    packed, rows = ref.expected_batch(refs, ys)
    # the input does what the case is about, by the oracle alone: row counts that fill two packs, one and a half, and one; failed
    # windows next to the reads in every trace
    assert [len(r) for r in rows] == [16, 12, 8, 12], [len(r) for r in rows]
    for b, r in enumerate(rows):
        ok = r["flags"] == 1
        assert len(r) == refs[b].n_windows // 2 and (~ok).sum() >= 1 and ok.sum() >= 2, (b, len(r), ok.sum())
    assert len(packed) == sum(o.state.n_epc_correct for o in refs)
    return host, lens, L, stride, refs, ys, (packed, rows)


def corrupted_trace(oracle_mod, synth_mod):
    """FIXED_Q = 0, one tag, five rounds, one bit of round 3's EPC frame flipped by the tag -> (host, lens, L, stride, (packed, [rows])):
    by the oracle alone that window fails its CRC; five rows: less than a pack"""
    x = synth_mod.make_trace(n_rounds=5, fixed_q=0, tag_ids=(0x27,), seed=7, sigma=0.02, corrupt_rounds=(3,)).samples
    host, lens, L, stride = lay_out([x])
    (o,), (y,) = oracle_pass(oracle_mod, host, lens, 0)
    packed, rows = ref.expected(o, y, 0)
    assert len(rows) == 5 and rows["flags"].tolist() == [1, 1, 0, 1, 1] and packed["seq"].tolist() == [1, 3, 7, 9]
    # the corrupted frame is a cleanly modulated frame whose CRC is wrong: its decision-directed estimate is as good as a read's
    h = ref.h_of(rows)
    assert abs(abs(h[2]) / np.median(np.abs(h)) - 1.0) < 0.2 and np.ptp(np.angle(h * np.conj(h[0]))) < 0.1, h
    return host, lens, L, stride, (packed, [rows])


def first_traces(want, n):
    """the expected records of the first n traces of a batch"""
    return want[0][want[0]["stream"] < n], want[1][:n]


def plan(ctx, n, L, max_tags=8):
    ctx.batch_plan(n, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_tracks()
    ctx.batch_plan_fine()


def enqueue(ctx):
    ctx.batch_inventory_enqueue()
    ctx.batch_tracks_enqueue()
    ctx.batch_fine_enqueue()


def check(ctx, want, what="", extra=3):
    """inventory + tracks + fine of the last pass; the packed records (aligned with the tracks) and every trace's row against the
    oracle's: check_rows -> all the bytes"""
    enqueue(ctx)
    ctx.batch_inventory_fetch()
    reads, off = ctx.batch_tracks_fetch()
    f = ctx.batch_fine_fetch()
    assert np.array_equal(f["stream"], reads["stream"]) and np.array_equal(f["seq"], reads["seq"])
    assert np.array_equal(f["start"], reads["start"])
    return check_rows(ctx, want, what, extra)


def rotated_frames(oracle_mod):
    """the 15 noise-free EPC frames of decoder_windows.valid_frames (sync offsets 0..14), each turned by exp(j phi i / 1370):
    -> [(name, window, the oracle's dump, phi)], every one decoded by the oracle with a good CRC and the frame's own bits"""
    out = []
    i = np.arange(ref.EPC_WIN, dtype=np.float64)
    for m, (w, bits, tag_id) in enumerate(dw.valid_frames(dw.EPC)):
        for phi in PHIS:
            wr = np.ascontiguousarray(w.astype(np.complex128) * np.exp(1j * phi * i / ref.EPC_WIN)).astype(np.complex64)
            d = oracle_mod.decode_window(wr, dw.EPC)
            assert d["crc_ok"] == 1 and d["tag_id"] == tag_id and np.array_equal(d["bits"][:128], bits), (m, phi)
            out.append(("frame@%d phi=%.1f" % (m, phi), wr, d, phi))
    assert len(out) == 45
    return out


def check_crafted_windows(ctx, oracle_mod, rfid):
    """rfid_fine_window on the rotated frames and the degenerate windows, by bytes against fine_ref; the drift of the rotated frames
    from the device's own records; a frame with bits the caller changed; what the call refuses"""
    frames = rotated_frames(oracle_mod)
    for name, w, d, phi in frames:
        want = ref.expected_window(w, d)
        got = ctx.fine_window(w, repair_ref.result_of_dump(d))
        ref.assert_equal(got, want, name)
        assert got["flags"] == 1 and got["stream"] == 0 and got["seq"] == 0 and got["start"] == 0 and got["reserved_"] == 0
        # the restatement gives 0.2449-0.2457 (phi = 0.3) and 0.4898-0.4915 (0.6) against phi x 1120 / 1370 = 0.2453 and 0.4905
        s0 = complex(got["seg_re"][0], got["seg_im"][0])
        s7 = complex(got["seg_re"][7], got["seg_im"][7])
        turn = float(np.angle(s7 * np.conj(s0)))
        assert abs(turn - phi * SEG_SPAN / ref.EPC_WIN) <= 0.005, (name, turn, phi * SEG_SPAN / ref.EPC_WIN)
    deg = dw.degenerate(dw.EPC)
    for name, w in deg.items():
        d = oracle_mod.decode_window(w, dw.EPC)
        want = ref.expected_window(w, d)
        got = ctx.fine_window(w, repair_ref.result_of_dump(d))
        ref.assert_equal(got, want, name)
        assert got["flags"] == (int(d["crc_ok"]) & 1)
    zero = ctx.fine_window(deg["zero"], repair_ref.result_of_dump(oracle_mod.decode_window(deg["zero"], dw.EPC)))
    assert not zero.tobytes().strip(b"\0")                       # (+0.0 everywhere: the sums start from 0.0f, g x 0 = -0.0 or not)
    # bits a caller has corrected: the signs follow the bits handed in, not the decoder's own
    name, w, d, phi = frames[4]
    bits = d["bits"][:128].copy()
    bits[40] ^= 1
    res = repair_ref.result_of_dump(d)
    res["bits"] = repair_ref.inv.pack_frames(bits[None, :])[0]
    res["crc_ok"] = 0
    want = ref.expected_window(w, d, bits=bits)
    want["flags"] = 0
    got = ctx.fine_window(w, res)
    ref.assert_equal(got, want, "changed bits")
    plain = ref.expected_window(w, d)
    assert got["seg_re"][:2].tobytes() == plain["seg_re"][:2].tobytes() and got["seg_re"][2:].tobytes() != plain["seg_re"][2:].tobytes()
    assert got["seg_pow"].tobytes() == plain["seg_pow"].tobytes()
    # not an EPC window's result; not an EPC window
    rn16 = res.copy()
    rn16["type"] = 0
    with pytest.raises(rfid.capi.RfidError) as e:
        ctx.fine_window(w, rn16)
    assert e.value.status == rfid.capi.ERR_INVALID
    with pytest.raises(ValueError):
        ctx.fine_window(w[:250], res)


def check_per_call_forms_share_one_buffer(rfid, oracle_mod, synth_mod):
    """The four per-call forms upload to, compute on and download from ONE device buffer of the context, which grows as a call
    needs: in one context without a plan -- repair_window, window_moments of 9 windows (two packs; grows the buffer), fine_window,
    commands_of 17 spans (two blocks; grows it again), window_moments of 1 window, repair_window on the first input again.  Every
    result equals, byte for byte, what the same call returns in a context of its own; the second repair equals the first."""
    import commands_cases
    frames = rotated_frames(oracle_mod)
    # a frame the decoder got right, handed in with one bit changed and its CRC marked as failed: the search has a frame to repair
    name, w, d, phi = frames[4]
    bits = d["bits"][:128].copy()
    bits[40] ^= 1
    res = repair_ref.result_of_dump(d)
    res["bits"] = repair_ref.inv.pack_frames(bits[None, :])[0]
    res["crc_ok"] = 0
    nine = np.stack([f[1][:240] for f in frames[:9]])
    spans, levels, names = commands_cases.crafted_spans(synth_mod)
    w2, d2 = frames[7][1], frames[7][2]
    calls = [
        ("repair", lambda c: c.repair_window(w, res)),
        ("moments of 9", lambda c: c.window_moments(nine)),
        ("fine", lambda c: c.fine_window(w2, repair_ref.result_of_dump(d2))),
        ("commands of 17", lambda c: c.commands_of(spans[:17], levels[:17])),
        ("moments of 1", lambda c: c.window_moments(nine[3:4])),
        ("repair again", lambda c: c.repair_window(w, res)),
    ]
    ctx = rfid.Context(device=0)
    try:
        got = [f(ctx).tobytes() for _, f in calls]
    finally:
        ctx.close()
    for (what, f), g in zip(calls, got):
        fresh = rfid.Context(device=0)
        try:
            assert f(fresh).tobytes() == g, what
        finally:
            fresh.close()
    assert got[5] == got[0] and got[0].strip(b"\0") and got[2].strip(b"\0")
    assert len(got[1]) == 9 * 32 and len(got[3]) == 17 * 48 and got[1][3 * 32 + 8:4 * 32] == got[4][8:]     # (behind stream, seq)


def check_rows(ctx, want, what="", extra=3, stats=True):
    """the packed records against want[0], every trace's row against want[1] (and `extra` zero rows behind it) -> all the bytes.
    stats: the context's statistics are still those of the pass the stage ran behind"""
    w_packed, w_rows = want
    f = ctx.batch_fine_fetch()
    ref.assert_equal(f, w_packed, what)
    st = ctx.batch_stats() if stats else None
    blob = f.tobytes()
    for b, w in enumerate(w_rows):
        r = ctx.batch_window_fine(b, extra=extra)
        assert len(r) == len(w) + extra, (what, b, len(r), len(w))
        assert st is None or int(st[b]["n_windows_used"]) // 2 == len(w), (what, b, len(w))
        ref.assert_equal(r[:len(w)], w, (what, "row", b))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, "rows behind the cut-off", b)
        blob += r.tobytes()
    return blob

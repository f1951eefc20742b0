"""The read-quality stage (rfid_batch_plan_quality / rfid_batch_quality / rfid_batch_get_quality / rfid_batch_get_window_quality:
SNR and decision margin of every EPC window, built on the device behind the tracks) on the CPU: csrc/rfid_capi.hip and
csrc/rfid_quality.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave emulator.  Every expected record is
worked out in numpy from the ORACLE alone (tests/quality_ref.py: oracle.fir, the oracle's openings, dc_est and per-window dumps), never
from the library's own windows or results, and every comparison is exact: by bit pattern, then by the bytes of the whole arrays.

The traces are those of tests/test_inventory_emu.py: seeds 104 (4 rounds) and 112 (3 rounds), FIXED_Q = 2, tags (0x27, 0x27, 0x31),
sigma = 0.02: a third of the slots are empty or collided, and the reference ACKs every one of them."""
import ctypes as C

import numpy as np
import pytest

import quality_ref as ref
import tracks_ref as tref
import emu_lib
from emu_lib import run_pass as _pass
from stage_backend import lay_out

TAGS = (0x27, 0x27, 0x31)
SEEDS = ((104, 4), (112, 3))       # (seed, inventory rounds) per trace


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


def _oracle(oracle_mod, host, lens, **cfg):
    """-> (oracle Results, the oracle's matched-filter outputs) of the traces"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ys


@pytest.fixture(scope="module")
def batch(oracle_mod, synth_mod):
    ts = [synth_mod.make_trace(n_rounds=n, fixed_q=2, tag_ids=TAGS, seed=seed, sigma=0.02, t1_jitter_raw=3).samples for seed, n in SEEDS]
    host, lens, L, stride = lay_out(ts, shorten=777)
    refs, ys = _oracle(oracle_mod, host, lens)
    packed, rows = ref.expected_batch(refs, ys)
    # the input does what the case is about, by the oracle alone: every trace holds failed EPC windows next to its reads, and the
    # measure tells the two apart with room to spare
    for b, r in enumerate(rows):
        ok = r["flags"] == 1
        snr = ref.snr_db(r)
        assert len(r) == refs[b].n_windows // 2 and (~ok).sum() >= 2 and ok.sum() >= 6, (b, len(r), ok.sum())
        assert snr[ok].min() - snr[~ok].max() > 6.0, (b, snr[ok].min(), snr[~ok].max())
    assert len(packed) == sum(o.state.n_epc_correct for o in refs)
    return host, lens, L, stride, refs, ys, (packed, rows)


def _plan(ctx, n, L, max_tags=8):
    ctx.batch_plan(n, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_tracks()
    ctx.batch_plan_quality()


def _check(ctx, want, what=""):
    """inventory + tracks + quality of the last pass; the packed records and every trace's row against the oracle's"""
    w_packed, w_rows = want
    ctx.batch_inventory()
    reads, off = ctx.batch_tracks()
    q = ctx.batch_quality()
    ref.assert_equal(q, w_packed, what)
    assert np.array_equal(q["stream"], reads["stream"]) and np.array_equal(q["seq"], reads["seq"])      # (aligned with the tracks)
    st = ctx.batch_stats()
    blob = q.tobytes()
    for b, w in enumerate(w_rows):
        r = ctx.batch_window_quality(b)
        assert len(r) == int(st[b]["n_windows_used"]) // 2
        ref.assert_equal(r, w, (what, "row", b))
        blob += r.tobytes()
    return blob


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_quality_of_a_ragged_batch_equals_the_oracles(batch, mode):
    """Two traces, both front ends; the pass twice: the same bytes both times, reads and failed windows alike"""
    import rfid
    host, lens, L, stride, refs, ys, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(mode)
        _plan(ctx, 2, L)
        blobs = []
        for rep in range(2):
            _pass(ctx, host, lens, L, stride)
            blobs.append(_check(ctx, want, (mode, rep)))
        assert blobs[0] == blobs[1]
        assert ctx.batch_quality_ms() >= 0.0
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        # the rows of the table behind a trace's windows are zero
        for b in range(2):
            r = ctx.batch_window_quality(b, extra=5)
            assert len(r) == len(want[1][b]) + 5 and not r[len(want[1][b]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(oracle_mod, batch):
    """MAX_NUM_QUERIES = 7 reached inside the traces (gate_impl.cc:101-109): the oracle stops after 14 windows in both; seven EPC
    windows each are reported, the rows behind them -- which an earlier, longer pass of the same context had filled -- are zero"""
    import rfid
    host, lens, L, stride, full_refs, full_ys, full_want = batch
    refs, ys = _oracle(oracle_mod, host, lens, max_num_queries=7)
    want = ref.expected_batch(refs, ys)
    assert all(o.state.status == 1 and o.n_windows == 14 for o in refs)
    assert [len(r) for r in want[1]] == [7, 7] and len(want[0]) < len(full_want[0])
    for mq, w in ((1000, full_want), (7, want)):
        ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=mq)
        try:
            ctx.batch_set_long_stream(0)
            _plan(ctx, 2, L)
            _pass(ctx, host, lens, L, stride)
            _check(ctx, w, mq)
            st = ctx.batch_stats()
            for b in range(2):
                n = C.c_int64(-1)
                rc = ctx._lib.rfid_batch_get_window_quality(ctx._h, b, None, 0, C.byref(n))
                assert rc == rfid.capi.ERR_CAPACITY and n.value == int(st[b]["n_windows_used"]) // 2 == len(w[1][b])
                many = ctx.batch_window_quality(b, extra=10_000)        # (more than the table has: the whole row of the trace)
                assert not many[len(w[1][b]):].tobytes().strip(b"\0")
        finally:
            ctx.close()
    # and in ONE context: a long pass fills the rows, the cut-off pass behind it must zero them again
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 2, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, full_want, "full")
        cut = lens.copy()
        for b in range(2):
            cut[b] = 5 * int(refs[b].open_idx[13] + 1370 + 40)              # (the trace ends behind its fourteenth window)
        short_refs, short_ys = _oracle(oracle_mod, host, cut)
        short = ref.expected_batch(short_refs, short_ys)
        assert [len(r) for r in short[1]] == [7, 7]
        ctx.batch_process_ptr(host.ctypes.data, stride, L, cut.ctypes.data)
        _check(ctx, short, "short")
        for b in range(2):
            r = ctx.batch_window_quality(b, extra=len(full_want[1][b]))
            assert not r[7:].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_a_corrupted_frame_fails_its_crc_with_the_snr_of_a_read(oracle_mod, synth_mod):
    """FIXED_Q = 0, one tag, one bit of round 3's EPC frame flipped: by the oracle alone that window fails its CRC with an SNR above
    15 dB -- a weak or damaged reply, not an empty or collided slot (those stay near 0 dB) -- and the stage reports just that"""
    import rfid
    from rfid import batch as rb
    x = synth_mod.make_trace(n_rounds=5, fixed_q=0, tag_ids=(0x27,), seed=7, sigma=0.02, corrupt_rounds=(3,)).samples
    host, lens, L, stride = lay_out([x])
    o = oracle_mod.run_trace(host[0, : lens[0]], oracle_mod.config(fixed_q=0))
    packed, rows = ref.expected(o, oracle_mod.fir(host[0, : lens[0]]), 0)
    failed = np.flatnonzero(rows["flags"] == 0)
    assert len(rows) == 5 and failed.tolist() == [2], rows["flags"]
    snr = ref.snr_db(rows)
    assert snr[failed[0]] > 15.0, snr
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 1, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, (packed, [rows]))
        got_snr, _ = rb.quality_fields(ctx.batch_window_quality(0))
        assert got_snr[2] > 15.0
    finally:
        ctx.close()


def test_only_one_trace_of_the_plan_and_a_trace_without_windows(oracle_mod, batch):
    import rfid
    host, lens, L, stride, refs, ys, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 3, L)
        ctx.batch_set_streams(1)
        _pass(ctx, host, lens, L, stride)
        one = ref.expected_batch(refs[:1], ys[:1])
        _check(ctx, one)
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_quality(ctx._h, 1, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID   # (not covered)
        # three traces, the middle one pure carrier: no window, no row, no read
        ctx.batch_set_streams(3)
        three = np.zeros((3, stride), dtype=np.complex64)
        three[0], three[2] = host[0], host[1]
        three[1, : L // 2] = 0.8 + 0.1j
        lens3 = np.array([lens[0], L // 2, lens[1]], dtype=np.int64)
        refs3, ys3 = _oracle(oracle_mod, three, lens3)
        want3 = ref.expected_batch(refs3, ys3)
        assert [len(r) for r in want3[1]][1] == 0 and len(want3[0]) == len(want[0])
        _pass(ctx, three, lens3, L, stride)
        _check(ctx, want3)
    finally:
        ctx.close()


def test_protocol_capacity_and_state_errors(batch):
    import rfid
    host, lens, L, stride, refs, ys, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    ERR_STATE, ERR_CAPACITY = rfid.capi.ERR_STATE, rfid.capi.ERR_CAPACITY

    def raises(fn, status):
        with pytest.raises(rfid.capi.RfidError) as e:
            fn()
        assert e.value.status == status, e.value

    try:
        raises(ctx.batch_plan_quality, ERR_STATE)                 # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_plan_quality, ERR_STATE)                 # no inventory workspace
        ctx.batch_plan_inventory(8)
        raises(ctx.batch_plan_quality, ERR_STATE)                 # no tracks workspace
        ctx.batch_plan_tracks()
        raises(ctx.batch_quality_enqueue, ERR_STATE)              # no quality workspace
        ctx.batch_plan_quality()
        raises(ctx.batch_quality_enqueue, ERR_STATE)              # no pass
        raises(ctx.batch_quality_fetch, ERR_STATE)                # nothing enqueued
        raises(lambda: ctx.batch_window_quality(0), ERR_STATE)
        raises(ctx.batch_quality_ms, ERR_STATE)
        _pass(ctx, host, lens, L, stride)
        raises(ctx.batch_quality_enqueue, ERR_STATE)              # a pass, but neither its inventory nor its tracks
        ctx.batch_inventory_enqueue()
        raises(ctx.batch_quality_enqueue, ERR_STATE)              # its inventory, but not its tracks
        _check(ctx, want, "first pass")
        # a second pass whose tracks were not enqueued: the tracks of the first are still there, the quality would mix passes
        _pass(ctx, host, lens, L, stride)
        raises(ctx.batch_quality_enqueue, ERR_STATE)
        ref.assert_equal(ctx.batch_quality_fetch(), want[0])      # (what was enqueued behind the first pass can still be fetched)
        ctx.batch_inventory_enqueue()
        raises(ctx.batch_quality_enqueue, ERR_STATE)              # (a new inventory: the earlier tracks are not its tracks)
        _check(ctx, want, "second pass")
        # a caller's array that is too small loses nothing
        small = np.zeros(len(want[0]) - 1, dtype=rfid.capi.QUALITY_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_quality(ctx._h, small.ctypes.data, len(small), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not small.tobytes().strip(b"\0")
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_quality(ctx._h, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(want[0])
        full = np.zeros(n.value, dtype=rfid.capi.QUALITY_DTYPE)
        assert ctx._lib.rfid_batch_get_quality(ctx._h, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        row = np.zeros(len(want[1][0]) - 1, dtype=rfid.capi.QUALITY_DTYPE)
        rc = ctx._lib.rfid_batch_get_window_quality(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[1][0]) and not row.tobytes().strip(b"\0")
        assert ctx._lib.rfid_batch_get_window_quality(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_quality(ctx._h, -1, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID
        # an inventory that overflowed names its first trace, as the tracks do
        ctx.set_knob("inventory_slots", 2)
        ctx.batch_plan_inventory(4)
        raises(ctx.batch_plan_quality, ERR_STATE)                 # (a new inventory workspace dropped the tracks workspace)
        ctx.batch_plan_tracks()
        ctx.batch_plan_quality()
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_quality_enqueue()
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_quality_fetch()
        assert e.value.status == ERR_CAPACITY and "trace 0" in str(e.value)
        ref.assert_equal(ctx.batch_window_quality(1), want[1][1])  # (the rows do not depend on the inventory)
        ctx.set_knob("inventory_slots", 0)
        # a new rfid_batch_plan_tracks drops the workspace, and so does a new plan
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        raises(ctx.batch_quality_enqueue, ERR_STATE)
        raises(ctx.batch_quality_fetch, ERR_STATE)
        ctx.batch_plan_quality()
        ctx.batch_plan_tracks()
        raises(ctx.batch_quality_fetch, ERR_STATE)
        ctx.batch_plan_quality()
        _check(ctx, want, "planned again")
        ctx.batch_plan(2, L)
        raises(ctx.batch_quality_enqueue, ERR_STATE)
        raises(ctx.batch_plan_quality, ERR_STATE)
        _plan(ctx, 2, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want, "new plan")
    finally:
        ctx.close()


def test_quality_fields_and_the_csv_columns(batch):
    """rfid.batch.quality_fields / format_tracks(..., quality) / format_quality (host side) on the oracle-derived records"""
    from rfid import batch as rb
    from rfid import _capi as capi
    host, lens, L, stride, refs, ys, (packed, rows) = batch
    snr, margin = rb.quality_fields(packed)
    assert snr.dtype == np.float64 and margin.dtype == np.float64
    for i, q in enumerate(packed):
        assert snr[i] == 10.0 * np.log10(float(q["sig_sq"]) / float(q["quad_sq"]))
        assert margin[i] == float(q["margin_min"]) / (float(q["sig_abs"]) / 128.0)
    assert np.array_equal(snr, ref.snr_db(packed)) and (margin > 0).all() and (margin <= 1.0).all()
    edge = np.zeros(2, dtype=capi.QUALITY_DTYPE)
    edge["sig_sq"][0] = 1.0
    s, m = rb.quality_fields(edge)
    assert s[0] == np.inf and np.isnan(s[1]) and np.isnan(m[1])
    ent, counts, reads, off = tref.expected_batch(refs)
    names = ["a.bin", "b.bin"]
    plain = rb.format_tracks(ent, reads, off, names)
    assert plain.splitlines()[0] == rb.TRACKS_HEADER == "file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T"
    lines = rb.format_tracks(ent, reads, off, names, packed).splitlines()
    assert lines[0] == rb.TRACKS_QUALITY_HEADER == rb.TRACKS_HEADER + ",snr_db,margin" and len(lines) == 1 + len(reads)
    for line, old, k in zip(lines[1:], plain.splitlines()[1:], range(len(reads))):
        f = line.split(",")
        assert ",".join(f[:-2]) == old                      # (the columns there were are untouched)
        assert f[-2] == "%.9g" % snr[k] and f[-1] == "%.9g" % margin[k]
    text = rb.format_quality(rows[0])
    ok = rows[0]["flags"] == 1
    assert text.startswith("| EPC windows : %d  failed : %d  " % (len(rows[0]), (~ok).sum())) and text.endswith("\n") and text.count("\n") == 1
    assert "%.2f" % np.median(ref.snr_db(rows[0])[ok]) in text and "%.2f" % np.median(ref.snr_db(rows[0])[~ok]) in text

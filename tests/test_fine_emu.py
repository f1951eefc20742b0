"""The fine-channel stage (rfid_batch_plan_fine / rfid_batch_fine / rfid_batch_get_fine / rfid_batch_get_window_fine and the per-call
rfid_fine_window: the data-aided channel estimate of every EPC window and of its eight 16-bit segments, built on the device behind the
tracks) on the CPU: csrc/rfid_capi.hip and csrc/rfid_fine.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the
wave emulator.  Every expected record is worked out in numpy from the ORACLE alone (tests/fine_ref.py: oracle.fir, the oracle's
openings, dc_est and per-window dumps), never from the library's own windows or results, and every comparison of records is exact: by
bit pattern, then by the bytes of the whole arrays.

The traces are FIXED_Q = 2, tags (0x27, 0x27, 0x31), sigma = 0.02: a third of the slots are empty or collided, and the reference ACKs
every one of them.  4, 3, 2 and 3 inventory rounds: 16, 12, 8 and 12 EPC windows -- a trace's rows fill two packs of eight, one and a
half, or one."""
import ctypes as C

import numpy as np
import pytest

import fine_cases as cases
import fine_ref as ref
import slots_cases
import tracks_ref as tref
import emu_lib
from emu_lib import run_pass as _pass
from stage_backend import lay_out

TAGS = (0x27, 0x27, 0x31)
SEEDS = ((104, 4), (112, 3), (120, 2), (128, 3))       # (seed, inventory rounds) per trace


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


def _oracle(oracle_mod, host, lens, fixed_q=2, **cfg):
    """-> (oracle Results, the oracle's matched-filter outputs) of the traces"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=fixed_q, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ys


@pytest.fixture(scope="module")
def batch(oracle_mod, synth_mod):
    ts = [synth_mod.make_trace(n_rounds=n, fixed_q=2, tag_ids=TAGS, seed=seed, sigma=0.02, t1_jitter_raw=3).samples for seed, n in SEEDS]
    host, lens, L, stride = lay_out(ts, shorten=777)
    refs, ys = _oracle(oracle_mod, host, lens)
    packed, rows = ref.expected_batch(refs, ys)
    # the input does what the case is about, by the oracle alone: row counts that fill two packs, one and a half, and one; failed
    # windows next to the reads in every trace
    assert [len(r) for r in rows] == [16, 12, 8, 12], [len(r) for r in rows]
    for b, r in enumerate(rows):
        ok = r["flags"] == 1
        assert len(r) == refs[b].n_windows // 2 and (~ok).sum() >= 1 and ok.sum() >= 2, (b, len(r), ok.sum())
    assert len(packed) == sum(o.state.n_epc_correct for o in refs)
    return host, lens, L, stride, refs, ys, (packed, rows)


def _plan(ctx, n, L, max_tags=8):
    ctx.batch_plan(n, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_tracks()
    ctx.batch_plan_fine()


def _check(ctx, want, what=""):
    """inventory + tracks + fine of the last pass; the packed records and every trace's row against the oracle's"""
    ctx.batch_inventory()
    reads, off = ctx.batch_tracks()
    f = ctx.batch_fine()
    assert np.array_equal(f["stream"], reads["stream"]) and np.array_equal(f["seq"], reads["seq"])      # (aligned with the tracks)
    assert np.array_equal(f["start"], reads["start"])
    return cases.check_rows(ctx, want, what)


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_fine_of_a_ragged_batch_equals_the_oracles(batch, mode):
    """Four traces, both front ends; the pass twice: the same bytes both times, reads and failed windows alike"""
    import rfid
    host, lens, L, stride, refs, ys, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(mode)
        _plan(ctx, 4, L)
        blobs = []
        for rep in range(2):
            _pass(ctx, host, lens, L, stride)
            blobs.append(_check(ctx, want, (mode, rep)))
        assert blobs[0] == blobs[1]
        assert ctx.batch_fine_ms() >= 0.0
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
    finally:
        ctx.close()


@pytest.mark.parametrize("wgs", [1, 3])
def test_a_workgroup_walks_many_packs(batch, wgs):
    """The knob fine_wgs: one or three workgroups for all the packs of the four traces -- packs with work behind packs behind a
    cut-off and the other way round, a trace's packs in one workgroup or spread over all three.  The same records"""
    import rfid
    host, lens, L, stride, refs, ys, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 4, L)
        ctx.set_knob("fine_wgs", wgs)
        _pass(ctx, host, lens, L, stride)
        first = _check(ctx, want, wgs)
        ctx.set_knob("fine_wgs", 0)
        ctx.batch_fine_enqueue()
        assert cases.check_rows(ctx, want, "default grid") == first
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(oracle_mod, batch):
    """MAX_NUM_QUERIES = 7 reached inside the traces (gate_impl.cc:101-109): the oracle stops after 14 windows; seven EPC windows
    each are reported -- a pack that is cut off inside -- and the rows behind them, which an earlier, longer pass of the same context
    had filled, are zero; the packed array holds no read from behind the cut-off"""
    import rfid
    host, lens, L, stride, full_refs, full_ys, full_want = batch
    host, lens = host[:2], lens[:2]
    full_want = (full_want[0][full_want[0]["stream"] < 2], full_want[1][:2])
    refs, ys = _oracle(oracle_mod, host, lens, max_num_queries=7)
    want = ref.expected_batch(refs, ys)
    assert all(o.state.status == 1 and o.n_windows == 14 for o in refs)
    assert [len(r) for r in want[1]] == [7, 7] and len(want[0]) < len(full_want[0])
    assert want[0]["seq"].max() < 14 <= full_want[0]["seq"].max()
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=7)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 2, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want, "max_num_queries")
        st = ctx.batch_stats()
        for b in range(2):
            n = C.c_int64(-1)
            rc = ctx._lib.rfid_batch_get_window_fine(ctx._h, b, None, 0, C.byref(n))
            assert rc == rfid.capi.ERR_CAPACITY and n.value == int(st[b]["n_windows_used"]) // 2 == 7
            many = ctx.batch_window_fine(b, extra=10_000)          # (more than the table has: the whole row of the trace)
            assert len(many) > 16 and not many[7:].tobytes().strip(b"\0")
    finally:
        ctx.close()
    # and in ONE context: a long pass fills the rows, the shorter pass behind it must zero them again
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
            r = ctx.batch_window_fine(b, extra=len(full_want[1][b]))
            assert not r[7:].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_a_corrupted_frame_has_its_record_and_says_so(oracle_mod, synth_mod):
    """FIXED_Q = 0, one tag, one bit of round 3's EPC frame flipped: by the oracle alone that window fails its CRC.  Its record is
    there, decision-directed, with flags = 0, and absent from the packed array; five rows: less than a pack"""
    import rfid
    x = synth_mod.make_trace(n_rounds=5, fixed_q=0, tag_ids=(0x27,), seed=7, sigma=0.02, corrupt_rounds=(3,)).samples
    host, lens, L, stride = lay_out([x])
    o = oracle_mod.run_trace(host[0, : lens[0]], oracle_mod.config(fixed_q=0))
    packed, rows = ref.expected(o, oracle_mod.fir(host[0, : lens[0]]), 0)
    assert len(rows) == 5 and rows["flags"].tolist() == [1, 1, 0, 1, 1] and packed["seq"].tolist() == [1, 3, 7, 9]
    # the corrupted frame is a cleanly modulated frame whose CRC is wrong: its decision-directed estimate is as good as a read's
    h = ref.h_of(rows)
    assert abs(abs(h[2]) / np.median(np.abs(h)) - 1.0) < 0.2 and np.ptp(np.angle(h * np.conj(h[0]))) < 0.1, h
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 1, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, (packed, [rows]))
        got = ctx.batch_window_fine(0)
        assert got["flags"].tolist() == [1, 1, 0, 1, 1] and got[2]["seq"] == 5 and got[2]["pow"] > 0
    finally:
        ctx.close()


def test_only_the_first_traces_of_the_plan_and_a_trace_without_windows(oracle_mod, batch):
    import rfid
    host, lens, L, stride, refs, ys, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 5, L)
        ctx.batch_set_streams(2)
        _pass(ctx, host, lens, L, stride)
        two = ref.expected_batch(refs[:2], ys[:2])
        _check(ctx, two)
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_fine(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID   # (not covered)
        # three traces, the middle one pure carrier: no window, no row, no read
        ctx.batch_set_streams(3)
        three = np.zeros((3, stride), dtype=np.complex64)
        three[0], three[2] = host[0], host[1]
        three[1, : L // 2] = 0.8 + 0.1j
        lens3 = np.array([lens[0], L // 2, lens[1]], dtype=np.int64)
        refs3, ys3 = _oracle(oracle_mod, three, lens3)
        want3 = ref.expected_batch(refs3, ys3)
        assert [len(r) for r in want3[1]][1] == 0 and len(want3[0]) == len(two[0])
        _pass(ctx, three, lens3, L, stride)
        _check(ctx, want3)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["fine-first", "fine-last"])
def test_other_stages_are_untouched(batch, order):
    """inventory + tracks + quality + repair + slots + commands on the same pass, with the fine stage enqueued before or behind them
    and without it: every other fetched array is byte-identical"""
    import rfid
    host, lens, L, stride, refs, ys, want = batch
    host, lens = host[:2], lens[:2]
    outs = []
    for fine in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            slots_cases.plan_all(ctx, 2, L)
            ctx.batch_plan_commands()
            if fine:
                ctx.batch_plan_fine()
            _pass(ctx, host, lens, L, stride)
            if fine and order == "fine-first":
                ctx.batch_inventory_enqueue()
                ctx.batch_tracks_enqueue()
                ctx.batch_fine_enqueue()
            ctx.batch_slots_enqueue()
            ctx.batch_commands_enqueue()
            parts = slots_cases.other_stage_outputs(ctx, 2)
            if fine and order == "fine-last":
                ctx.batch_fine_enqueue()
            for b in range(2):
                parts += [ctx.batch_window_moments(b, extra=2).tobytes(), ctx.batch_window_commands(b, extra=2).tobytes()]
            if fine:
                cases.check_rows(ctx, (want[0][want[0]["stream"] < 2], want[1][:2]), order)
            outs.append(parts)
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs))


def test_protocol_capacity_and_state_errors(batch):
    import rfid
    host, lens, L, stride, refs, ys, want = batch
    host, lens = host[:2], lens[:2]
    want = (want[0][want[0]["stream"] < 2], want[1][:2])
    ctx = rfid.Context(device=0, fixed_q=2)
    ERR_STATE, ERR_CAPACITY, ERR_INVALID, OK = rfid.capi.ERR_STATE, rfid.capi.ERR_CAPACITY, rfid.capi.ERR_INVALID, rfid.capi.OK
    lib = ctx._lib

    def raises(fn, status):
        with pytest.raises(rfid.capi.RfidError) as e:
            fn()
        assert e.value.status == status, e.value

    try:
        assert lib.rfid_abi_version() == 7                        # (functions were added, nothing changed)
        raises(ctx.batch_plan_fine, ERR_STATE)                    # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_plan_fine, ERR_STATE)                    # no inventory workspace
        ctx.batch_plan_inventory(8)
        raises(ctx.batch_plan_fine, ERR_STATE)                    # no tracks workspace
        ctx.batch_plan_tracks()
        raises(ctx.batch_fine_enqueue, ERR_STATE)                 # no fine workspace
        ctx.batch_plan_fine()
        raises(ctx.batch_fine_enqueue, ERR_STATE)                 # no pass
        raises(ctx.batch_fine_fetch, ERR_STATE)                   # nothing enqueued
        raises(lambda: ctx.batch_window_fine(0), ERR_STATE)
        raises(ctx.batch_fine_ms, ERR_STATE)
        _pass(ctx, host, lens, L, stride)
        raises(ctx.batch_fine_enqueue, ERR_STATE)                 # a pass, but neither its inventory nor its tracks
        ctx.batch_inventory_enqueue()
        raises(ctx.batch_fine_enqueue, ERR_STATE)                 # its inventory, but not its tracks
        _check(ctx, want, "first pass")
        # neither the quality nor the repair workspace is needed, and planning them drops nothing
        ctx.batch_plan_quality()
        ctx.batch_plan_repair()
        ctx.batch_fine_enqueue()
        ctx.batch_quality_enqueue()                               # (the stage did not move the level of the tracks)
        cases.check_rows(ctx, want, "beside quality and repair")
        # a second pass whose tracks were not enqueued: the tracks of the first are still there, the stage would mix passes
        _pass(ctx, host, lens, L, stride)
        raises(ctx.batch_fine_enqueue, ERR_STATE)
        ref.assert_equal(ctx.batch_fine_fetch(), want[0])         # (what was enqueued behind the first pass can still be fetched)
        ctx.batch_inventory_enqueue()
        raises(ctx.batch_fine_enqueue, ERR_STATE)                 # (a new inventory: the earlier tracks are not its tracks)
        _check(ctx, want, "second pass")
        # a caller's array that is too small loses nothing
        small = np.zeros(len(want[0]) - 1, dtype=rfid.capi.FINE_DTYPE)
        n = C.c_int64(0)
        rc = lib.rfid_batch_get_fine(ctx._h, small.ctypes.data, len(small), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not small.tobytes().strip(b"\0")
        n = C.c_int64(0)
        assert lib.rfid_batch_get_fine(ctx._h, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(want[0])
        full = np.zeros(n.value, dtype=rfid.capi.FINE_DTYPE)
        assert lib.rfid_batch_get_fine(ctx._h, full.ctypes.data, len(full), C.byref(n)) == OK
        ref.assert_equal(full, want[0])
        row = np.zeros(len(want[1][0]) - 1, dtype=rfid.capi.FINE_DTYPE)
        rc = lib.rfid_batch_get_window_fine(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[1][0]) and not row.tobytes().strip(b"\0")
        # arguments
        assert lib.rfid_batch_get_window_fine(ctx._h, 2, None, 0, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_get_window_fine(ctx._h, -1, None, 0, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_get_fine(ctx._h, None, 1, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_get_fine(ctx._h, full.ctypes.data, -1, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_get_fine(ctx._h, full.ctypes.data, len(full), None) == ERR_INVALID
        assert lib.rfid_batch_plan_fine(None) == ERR_INVALID and lib.rfid_batch_fine(None) == ERR_INVALID
        assert lib.rfid_batch_fine_ms(ctx._h, None) == ERR_INVALID
        assert lib.rfid_fine_window(ctx._h, None, None, None) == ERR_INVALID
        # an inventory that overflowed names its first trace, as the tracks do
        ctx.set_knob("inventory_slots", 2)
        ctx.batch_plan_inventory(4)
        raises(ctx.batch_plan_fine, ERR_STATE)                    # (a new inventory workspace dropped the tracks workspace)
        raises(ctx.batch_fine_fetch, ERR_STATE)                   # (... and this one with it)
        ctx.batch_plan_tracks()
        ctx.batch_plan_fine()
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_fine_enqueue()
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_fine_fetch()
        assert e.value.status == ERR_CAPACITY and "trace 0" in str(e.value)
        ref.assert_equal(ctx.batch_window_fine(1), want[1][1])    # (the rows do not depend on the inventory)
        ctx.set_knob("inventory_slots", 0)
        # a new rfid_batch_plan_tracks drops the workspace, and so does a new plan
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        raises(ctx.batch_fine_enqueue, ERR_STATE)
        raises(ctx.batch_fine_fetch, ERR_STATE)
        ctx.batch_plan_fine()
        ctx.batch_plan_tracks()
        raises(ctx.batch_fine_fetch, ERR_STATE)
        ctx.batch_plan_fine()
        _check(ctx, want, "planned again")
        ctx.batch_plan(2, L)
        raises(ctx.batch_fine_enqueue, ERR_STATE)
        raises(ctx.batch_plan_fine, ERR_STATE)
        _plan(ctx, 2, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want, "new plan")
    finally:
        ctx.close()


def test_crafted_windows_through_fine_window(oracle_mod):
    """rfid_fine_window: 15 noise-free frames at every sync offset, each turning by 0, 0.3 and 0.6 rad over its window -- the segments
    see the turn -- the degenerate windows (all zero, constant, period 7, 38 samples), and a frame whose bits the caller changed"""
    import rfid
    ctx = rfid.Context(device=0)
    try:
        cases.check_crafted_windows(ctx, oracle_mod, rfid)
    finally:
        ctx.close()


def test_per_call_forms_share_one_buffer(oracle_mod, synth_mod):
    """repair_window, window_moments, fine_window and commands_of interleaved in one context, the buffer growing twice: every
    result is what a context of its own returns"""
    import rfid
    cases.check_per_call_forms_share_one_buffer(rfid, oracle_mod, synth_mod)


def test_the_estimate_is_at_least_twice_as_steady_as_h_est(oracle_mod, synth_mod):
    """60 rounds, one tag, h = 0.10 e^{j 2.1}, sigma = 0.03: over the CRC-verified reads the phase of the data-aided h (fine_fields of
    the library's records) scatters at most half as much about the truth, 25 complex64(h), as the decoder's h_est does.  Theory: h_est
    has std 5 sigma / sqrt(6) per component, the data-aided estimate 5 sigma sqrt(2) / sqrt(128) -- 3.3 times less; the restatement
    gives 3.7 here (0.0310 against 0.0085 rad, rms about the truth); the factor of two is the margin that lets a sample of 60 reads stand.  The estimate is
    of the same channel: |h| / |h_est| has a mean within 0.90 .. 1.00 (0.96 here: the matched filter's ramps between half-bits)."""
    import rfid
    from rfid import batch as rb
    h_true = 0.10 * np.exp(2.1j)
    x = synth_mod.make_trace(n_rounds=60, fixed_q=0, tag_ids=(0x27,), seed=3, sigma=0.03, h=h_true).samples
    host, lens, L, stride = lay_out([x])
    o = oracle_mod.run_trace(host[0, : lens[0]], oracle_mod.config(fixed_q=0))
    packed, rows = ref.expected(o, oracle_mod.fir(host[0, : lens[0]]), 0)
    assert len(packed) == 60
    truth = 25.0 * complex(np.complex64(h_true))
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 1, L)
        _pass(ctx, host, lens, L, stride)
        ctx.batch_inventory()
        reads, off = ctx.batch_tracks()
        f = ctx.batch_fine()
        ref.assert_equal(f, packed)
    finally:
        ctx.close()
    assert len(reads) == 60 and np.array_equal(reads["seq"], f["seq"])
    ff = rb.fine_fields(f)
    h_est = reads["h_re"].astype(np.float64) + 1j * reads["h_im"].astype(np.float64)
    dev = lambda h: float(np.sqrt(np.mean(np.angle(h * np.conj(truth)) ** 2)))
    std_fine, std_est = dev(ff["h"]), dev(h_est)
    ratio = float(np.mean(np.abs(ff["h"]) / np.abs(h_est)))
    print("phase std about the truth: h_est %.4f rad, data-aided %.4f rad (%.2f times); mean |h| / |h_est| %.3f" %
          (std_est, std_fine, std_est / std_fine, ratio))
    assert std_fine <= 0.5 * std_est, (std_fine, std_est)
    assert 0.90 <= ratio <= 1.00, ratio


def test_fine_fields_and_the_csv_columns(batch):
    """rfid.batch.fine_fields / format_tracks(..., fine) / format_fine (host side) on the oracle-derived records"""
    from rfid import batch as rb
    from rfid import _capi as capi
    host, lens, L, stride, refs, ys, (packed, rows) = batch
    ff = rb.fine_fields(packed)
    assert ff["h"].dtype == np.complex128 and ff["h_seg"].shape == (len(packed), 8)
    for i, r in enumerate(packed):
        re, im = np.float64(r["sum_re"]), np.float64(r["sum_im"])
        sq = re * re + im * im
        mag = np.sqrt(sq) / 128.0
        assert ff["h"][i].real == re / 128.0 and ff["h"][i].imag == im / 128.0
        assert ff["noise"][i] == (np.float64(r["pow"]) - sq / 128.0) / 127.0 > 0
        assert ff["mag_db"][i] == 20.0 * np.log10(mag) and ff["phase_rad"][i] == np.arctan2(im, re)
        assert ff["snr_db"][i] == 10.0 * np.log10(mag ** 2 / ff["noise"][i])
        hk = (r["seg_re"].astype(np.float64) + 1j * r["seg_im"].astype(np.float64)) / 16.0
        assert np.array_equal(ff["h_seg"][i], hk)
        ph = np.angle(hk * np.conj(ff["h"][i]))
        slope = np.polyfit(400e-6 * np.arange(8), ph, 1)[0]
        assert abs(ff["drift_rad_s"][i] - slope) <= 1e-9 * max(1.0, abs(slope)), (i, ff["drift_rad_s"][i], slope)
    assert ref.h_of(packed).tobytes() == ff["h"].tobytes() and (ff["snr_db"] > 10.0).all()
    # a turning channel has the drift it was given: 0.6 rad over 1370 samples at 400 ksps
    edge = np.zeros(3, dtype=capi.FINE_DTYPE)
    turn = np.exp(1j * 0.6 * 160.0 / 1370.0 * np.arange(8))
    edge["seg_re"][0], edge["seg_im"][0] = 16.0 * turn.real, 16.0 * turn.imag
    edge["sum_re"][0], edge["sum_im"][0], edge["pow"][0] = edge["seg_re"][0].sum(), edge["seg_im"][0].sum(), 128.0
    edge["sum_re"][1], edge["pow"][1] = 128.0, 128.0
    e = rb.fine_fields(edge)
    assert abs(e["drift_rad_s"][0] - 0.6 * 400e3 / 1370.0) < 1e-3 and e["drift_rad_s"][1] == 0.0
    assert e["snr_db"][1] == np.inf and np.isnan(e["snr_db"][2]) and e["mag_db"][2] == -np.inf
    ent, counts, reads, off = tref.expected_batch(refs)
    names = ["a.bin", "b.bin", "c.bin", "d.bin"]
    plain = rb.format_tracks(ent, reads, off, names)
    assert plain.splitlines()[0] == rb.TRACKS_HEADER == "file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T"
    assert rb.TRACKS_FINE_COLUMNS == ",hd_re,hd_im,hd_mag_db,hd_phase_rad,hd_snr_db,drift_rad_s"
    lines = rb.format_tracks(ent, reads, off, names, None, packed).splitlines()
    assert lines[0] == rb.TRACKS_HEADER + rb.TRACKS_FINE_COLUMNS and len(lines) == 1 + len(reads)
    for line, old, k in zip(lines[1:], plain.splitlines()[1:], range(len(reads))):
        f = line.split(",")
        assert ",".join(f[:-6]) == old                      # (the columns there were are untouched)
        assert f[-6:] == ["%.9g" % v for v in (ff["h"][k].real, ff["h"][k].imag, ff["mag_db"][k], ff["phase_rad"][k], ff["snr_db"][k],
                                               ff["drift_rad_s"][k])]
    text = rb.format_fine(rows[0])
    ok = rows[0]["flags"] == 1
    assert text.startswith("| EPC windows : %d  failed : %d  " % (len(rows[0]), (~ok).sum())) and text.endswith("\n") and text.count("\n") == 1
    assert "%.2f" % np.median(rb.fine_fields(rows[0])["snr_db"][ok]) in text
    assert rb.format_fine(rows[0][:0]).startswith("| EPC windows : 0  failed : 0  ")

"""The cases of the fine-channel stage that run on both sides, written once: tests/test_fine_emu.py (the kernels on the wave emulator)
and tests/test_gpu_fine.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches the
library).  Pytest collects the imported functions in the importing module, resolves their fixtures there and applies that module's
marks.  Every expected record is worked out in numpy from the ORACLE alone (tests/fine_ref.py), never from the library's own windows
or results, and every comparison of records is exact; the inputs and the checks are in tests/fine_cases.py."""
import ctypes as C

import numpy as np
import pytest

import fine_cases as cases
import fine_ref as ref
import slots_cases
from stage_backend import carrier_between, lay_out, oracle_pass

__all__ = ["batch", "pair", "test_fine_of_a_ragged_batch_equals_the_oracles", "test_a_workgroup_walks_many_packs",
           "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero", "test_a_corrupted_frame_has_its_record_and_says_so",
           "test_only_the_first_traces_of_the_plan_and_a_trace_without_windows", "test_other_stages_are_untouched",
           "test_protocol_capacity_and_state_errors", "test_crafted_windows_through_fine_window",
           "test_per_call_forms_share_one_buffer", "test_the_estimate_is_at_least_twice_as_steady_as_h_est"]


@pytest.fixture(scope="module")
def batch(backend, oracle_mod, synth_mod):
    data = cases.ragged_batch(oracle_mod, synth_mod)
    return data + (backend.put(data[0], data[1]),)


@pytest.fixture(scope="module")
def pair(backend, batch):
    """the first two traces of the batch (16 and 12 EPC windows) as a batch of their own: -> (host, lens, L, stride, want, handle)"""
    host, lens, L, stride, refs, ys, want, _ = batch
    h, l = np.ascontiguousarray(host[:2]), lens[:2].copy()
    return h, l, L, stride, cases.first_traces(want, 2), backend.put(h, l)


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_fine_of_a_ragged_batch_equals_the_oracles(backend, batch, mode):
    """Four traces, both front ends; the pass backend.reps times: the same bytes every time, reads and failed windows alike"""
    import rfid
    host, lens, L, stride, refs, ys, want, dev = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(mode)
        cases.plan(ctx, 4, L)
        blobs = []
        for rep in range(backend.reps):
            backend.run_pass(ctx, dev, L, stride)
            blobs.append(cases.check(ctx, want, (mode, rep)))
        assert all(b == blobs[0] for b in blobs)
        assert ctx.batch_fine_ms() >= 0.0
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
    finally:
        ctx.close()


@pytest.mark.parametrize("wgs", [0, 1, 3])
def test_a_workgroup_walks_many_packs(backend, batch, wgs):
    """The knob fine_wgs: the launch's default grid, or one or three workgroups for all the packs of the four traces -- packs with
    work behind packs behind a cut-off and the other way round, a trace's packs in one workgroup or spread over all three; traces 1
    and 3 have twelve EPC windows, a pack and a half: a later trace whose rows cross a pack boundary.  The same records"""
    import rfid
    host, lens, L, stride, refs, ys, want, dev = batch
    assert len(want[1][1]) == 12 and len(want[1][3]) == 12
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 4, L)
        ctx.set_knob("fine_wgs", wgs)
        backend.run_pass(ctx, dev, L, stride)
        first = cases.check(ctx, want, wgs)
        ctx.set_knob("fine_wgs", 0)
        ctx.batch_fine_enqueue()
        assert cases.check_rows(ctx, want, "default grid") == first
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, batch):
    """MAX_NUM_QUERIES = 7 reached inside the traces (gate_impl.cc:101-109): the oracle stops after 14 windows; seven EPC windows
    each are reported -- a pack that is cut off inside -- and the rows behind them, which an earlier, longer pass of the same context
    had filled, are zero; the packed array holds no read from behind the cut-off"""
    import rfid
    host, lens, L, stride, full_refs, full_ys, full_want, dev = batch
    refs, ys = oracle_pass(oracle_mod, host, lens, 2, max_num_queries=7)
    want = ref.expected_batch(refs, ys)
    assert all(o.state.status == 1 and o.n_windows == 14 for o in refs)
    assert [len(r) for r in want[1]] == [7, 7, 7, 7] and len(want[0]) < len(full_want[0])
    assert want[0]["seq"].max() < 14 <= full_want[0]["seq"].max()
    for mq, w in ((1000, full_want), (7, want)):
        ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=mq)
        try:
            ctx.batch_set_long_stream(0)
            cases.plan(ctx, 4, L)
            backend.run_pass(ctx, dev, L, stride)
            cases.check(ctx, w, mq)
            st = ctx.batch_stats()
            for b in range(4):
                n = C.c_int64(-1)
                rc = ctx._lib.rfid_batch_get_window_fine(ctx._h, b, None, 0, C.byref(n))
                assert rc == rfid.capi.ERR_CAPACITY and n.value == int(st[b]["n_windows_used"]) // 2 == len(w[1][b])
                many = ctx.batch_window_fine(b, extra=10_000)          # (more than the table has: the whole row of the trace)
                assert len(many) > 16 and not many[len(w[1][b]):].tobytes().strip(b"\0")
        finally:
            ctx.close()
    # and in ONE context: a long pass fills the rows, the shorter pass behind it must zero them again
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 4, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, full_want, "full")
        cut = lens.copy()
        for b in range(4):
            cut[b] = 5 * int(refs[b].open_idx[13] + 1370 + 40)              # (the trace ends behind its fourteenth window)
        short = ref.expected_batch(*oracle_pass(oracle_mod, host, cut, 2))
        assert [len(r) for r in short[1]] == [7, 7, 7, 7]
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        cases.check(ctx, short, "short")
        for b in range(4):
            r = ctx.batch_window_fine(b, extra=len(full_want[1][b]))
            assert not r[7:].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_a_corrupted_frame_has_its_record_and_says_so(backend, oracle_mod, synth_mod):
    """One bit of round 3's EPC frame flipped: by the oracle alone (fine_cases.corrupted_trace) that window fails its CRC.  Its
    record is there, decision-directed, with flags = 0, and absent from the packed array; five rows: less than a pack"""
    import rfid
    host, lens, L, stride, want = cases.corrupted_trace(oracle_mod, synth_mod)
    dev = backend.put(host, lens)
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 1, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, want)
        got = ctx.batch_window_fine(0)
        assert got["flags"].tolist() == [1, 1, 0, 1, 1] and got[2]["seq"] == 5 and got[2]["pow"] > 0
    finally:
        ctx.close()


def test_only_the_first_traces_of_the_plan_and_a_trace_without_windows(backend, oracle_mod, batch):
    import rfid
    host, lens, L, stride, refs, ys, want, dev = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 5, L)
        ctx.batch_set_streams(2)
        backend.run_pass(ctx, dev, L, stride)
        two = ref.expected_batch(refs[:2], ys[:2])
        cases.check(ctx, two)
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_fine(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID   # (not covered)
        # three traces, the middle one pure carrier: no window, no row, no read
        ctx.batch_set_streams(3)
        three, lens3 = carrier_between(host, lens, L)
        want3 = ref.expected_batch(*oracle_pass(oracle_mod, three, lens3, 2))
        assert [len(r) for r in want3[1]][1] == 0 and len(want3[0]) == len(two[0])
        dev3 = backend.put(three, lens3)
        backend.run_pass(ctx, dev3, L, stride)
        cases.check(ctx, want3)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["fine-first", "fine-last"])
def test_other_stages_are_untouched(backend, pair, order):
    """inventory + tracks + quality + repair + slots + commands on the same pass, with the fine stage enqueued before or behind them
    and without it: every other fetched array is byte-identical"""
    import rfid
    host, lens, L, stride, want, dev = pair
    outs = []
    for fine in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            slots_cases.plan_all(ctx, 2, L)
            ctx.batch_plan_commands()
            if fine:
                ctx.batch_plan_fine()
            backend.run_pass(ctx, dev, L, stride)
            if fine and order == "fine-first":
                cases.enqueue(ctx)
            ctx.batch_slots_enqueue()
            ctx.batch_commands_enqueue()
            parts = slots_cases.other_stage_outputs(ctx, 2)
            if fine and order == "fine-last":
                ctx.batch_fine_enqueue()
            for b in range(2):
                parts += [ctx.batch_window_moments(b, extra=2).tobytes(), ctx.batch_window_commands(b, extra=2).tobytes()]
            if fine:
                cases.check_rows(ctx, want, order)
            outs.append(parts)
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs))


def test_protocol_capacity_and_state_errors(backend, pair):
    import rfid
    host, lens, L, stride, want, dev = pair
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
        backend.run_pass(ctx, dev, L, stride)
        raises(ctx.batch_fine_enqueue, ERR_STATE)                 # a pass, but neither its inventory nor its tracks
        ctx.batch_inventory_enqueue()
        raises(ctx.batch_fine_enqueue, ERR_STATE)                 # its inventory, but not its tracks
        cases.check(ctx, want, "first pass")
        # neither the quality nor the repair workspace is needed, and planning them drops nothing
        ctx.batch_plan_quality()
        ctx.batch_plan_repair()
        ctx.batch_fine_enqueue()
        ctx.batch_quality_enqueue()                               # (the stage did not move the level of the tracks)
        cases.check_rows(ctx, want, "beside quality and repair")
        # a second pass whose tracks were not enqueued: the tracks of the first are still there, the stage would mix passes
        backend.run_pass(ctx, dev, L, stride)
        raises(ctx.batch_fine_enqueue, ERR_STATE)
        ref.assert_equal(ctx.batch_fine_fetch(), want[0])         # (what was enqueued behind the first pass can still be fetched)
        ctx.batch_inventory_enqueue()
        raises(ctx.batch_fine_enqueue, ERR_STATE)                 # (a new inventory: the earlier tracks are not its tracks)
        cases.check(ctx, want, "second pass")
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
        cases.enqueue(ctx)
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
        cases.check(ctx, want, "planned again")
        ctx.batch_plan(2, L)
        raises(ctx.batch_fine_enqueue, ERR_STATE)
        raises(ctx.batch_plan_fine, ERR_STATE)
        cases.plan(ctx, 2, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, want, "new plan")
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


def test_the_estimate_is_at_least_twice_as_steady_as_h_est(backend, oracle_mod, synth_mod):
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
    (o,), (y,) = oracle_pass(oracle_mod, host, lens, 0)
    packed, rows = ref.expected(o, y, 0)
    assert len(packed) == 60
    truth = 25.0 * complex(np.complex64(h_true))
    dev = backend.put(host, lens)
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 1, L)
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_inventory()
        reads, off = ctx.batch_tracks()
        f = ctx.batch_fine()
        ref.assert_equal(f, packed)
    finally:
        ctx.close()
    assert len(reads) == 60 and np.array_equal(reads["seq"], f["seq"])
    ff = rb.fine_fields(f)
    h_est = reads["h_re"].astype(np.float64) + 1j * reads["h_im"].astype(np.float64)
    spread = lambda h: float(np.sqrt(np.mean(np.angle(h * np.conj(truth)) ** 2)))
    std_fine, std_est = spread(ff["h"]), spread(h_est)
    ratio = float(np.mean(np.abs(ff["h"]) / np.abs(h_est)))
    print("%s: phase std about the truth: h_est %.4f rad, data-aided %.4f rad (%.2f times); mean |h| / |h_est| %.3f" %
          (backend.name, std_est, std_fine, std_est / std_fine, ratio))
    assert std_fine <= 0.5 * std_est, (std_fine, std_est)
    assert 0.90 <= ratio <= 1.00, ratio

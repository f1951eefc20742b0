"""The cases of the quality stage that run on both sides, written once: tests/test_quality_emu.py (the kernels on the wave emulator)
and tests/test_gpu_quality.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches
the library).  Pytest collects the imported functions in the importing module, resolves their fixtures there and applies that
module's marks.  Every expected record is worked out in numpy from the ORACLE alone (tests/quality_ref.py), never from the library's
own windows or results, and every comparison is exact; the inputs and the checks are in tests/quality_cases.py."""
import ctypes as C

import numpy as np
import pytest

import quality_ref as ref
import quality_cases as cases
from stage_backend import carrier_between, oracle_pass

__all__ = ["batch", "test_quality_of_a_ragged_batch_equals_the_oracles",
           "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero",
           "test_a_corrupted_frame_fails_its_crc_with_the_snr_of_a_read",
           "test_only_one_trace_of_the_plan_and_a_trace_without_windows", "test_protocol_capacity_and_state_errors"]


@pytest.fixture(scope="module")
def batch(backend, oracle_mod, synth_mod):
    data = cases.ragged_batch(oracle_mod, synth_mod)
    return data + (backend.put(data[0], data[1]),)


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_quality_of_a_ragged_batch_equals_the_oracles(backend, batch, mode):
    """Two traces, both front ends; the pass backend.reps times: the same bytes every time, reads and failed windows alike, and the
    five rows of the table behind a trace's windows zero"""
    import rfid
    host, lens, L, stride, refs, ys, want, dev = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(mode)
        cases.plan(ctx, 2, L)
        blobs = []
        for rep in range(backend.reps):
            backend.run_pass(ctx, dev, L, stride)
            blobs.append(cases.check(ctx, want, (mode, rep), extra=5))
        assert all(b == blobs[0] for b in blobs)
        assert ctx.batch_quality_ms() >= 0.0
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, batch):
    """MAX_NUM_QUERIES = 7 reached inside the traces (gate_impl.cc:101-109): the oracle stops after 14 windows in both; seven EPC
    windows each are reported, the rows behind them -- which an earlier, longer pass of the same context had filled -- are zero"""
    import rfid
    host, lens, L, stride, full_refs, full_ys, full_want, dev = batch
    refs, ys = oracle_pass(oracle_mod, host, lens, 2, max_num_queries=7)
    want = ref.expected_batch(refs, ys)
    assert all(o.state.status == 1 and o.n_windows == 14 for o in refs)
    assert [len(r) for r in want[1]] == [7, 7] and len(want[0]) < len(full_want[0])
    for mq, w in ((1000, full_want), (7, want)):
        ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=mq)
        try:
            ctx.batch_set_long_stream(0)
            cases.plan(ctx, 2, L)
            backend.run_pass(ctx, dev, L, stride)
            cases.check(ctx, w, mq)
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
        cases.plan(ctx, 2, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, full_want, "full")
        cut = lens.copy()
        for b in range(2):
            cut[b] = 5 * int(refs[b].open_idx[13] + 1370 + 40)              # (the trace ends behind its fourteenth window)
        short = ref.expected_batch(*oracle_pass(oracle_mod, host, cut, 2))
        assert [len(r) for r in short[1]] == [7, 7]
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        cases.check(ctx, short, "short")
        for b in range(2):
            r = ctx.batch_window_quality(b, extra=len(full_want[1][b]))
            assert not r[7:].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_a_corrupted_frame_fails_its_crc_with_the_snr_of_a_read(backend, oracle_mod, synth_mod):
    """One bit of round 3's EPC frame flipped: by the oracle alone (quality_cases.corrupted_trace) that window fails its CRC with
    the SNR of a read, and the stage reports just that"""
    import rfid
    from rfid import batch as rb
    host, lens, L, stride, want = cases.corrupted_trace(oracle_mod, synth_mod)
    dev = backend.put(host, lens)
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 1, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, want)
        got_snr, _ = rb.quality_fields(ctx.batch_window_quality(0))
        assert got_snr[2] > 15.0
    finally:
        ctx.close()


def test_only_one_trace_of_the_plan_and_a_trace_without_windows(backend, oracle_mod, batch):
    import rfid
    host, lens, L, stride, refs, ys, want, dev = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 3, L)
        ctx.batch_set_streams(1)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, ref.expected_batch(refs[:1], ys[:1]))
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_quality(ctx._h, 1, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID   # (not covered)
        # three traces, the middle one pure carrier: no window, no row, no read
        ctx.batch_set_streams(3)
        three, lens3 = carrier_between(host, lens, L)
        want3 = ref.expected_batch(*oracle_pass(oracle_mod, three, lens3, 2))
        assert [len(r) for r in want3[1]][1] == 0 and len(want3[0]) == len(want[0])
        dev3 = backend.put(three, lens3)
        backend.run_pass(ctx, dev3, L, stride)
        cases.check(ctx, want3)
    finally:
        ctx.close()


def test_protocol_capacity_and_state_errors(backend, batch):
    import rfid
    host, lens, L, stride, refs, ys, want, dev = batch
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
        backend.run_pass(ctx, dev, L, stride)
        raises(ctx.batch_quality_enqueue, ERR_STATE)              # a pass, but neither its inventory nor its tracks
        ctx.batch_inventory_enqueue()
        raises(ctx.batch_quality_enqueue, ERR_STATE)              # its inventory, but not its tracks
        cases.check(ctx, want, "first pass")
        # a second pass whose tracks were not enqueued: the tracks of the first are still there, the quality would mix passes
        backend.run_pass(ctx, dev, L, stride)
        raises(ctx.batch_quality_enqueue, ERR_STATE)
        ref.assert_equal(ctx.batch_quality_fetch(), want[0])      # (what was enqueued behind the first pass can still be fetched)
        ctx.batch_inventory_enqueue()
        raises(ctx.batch_quality_enqueue, ERR_STATE)              # (a new inventory: the earlier tracks are not its tracks)
        cases.check(ctx, want, "second pass")
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
        cases.check(ctx, want, "planned again")
        ctx.batch_plan(2, L)
        raises(ctx.batch_quality_enqueue, ERR_STATE)
        raises(ctx.batch_plan_quality, ERR_STATE)
        cases.plan(ctx, 2, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, want, "new plan")
    finally:
        ctx.close()

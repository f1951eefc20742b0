"""The cases of the slots stage that run on both sides, written once: tests/test_slots_emu.py (the kernels on the wave emulator) and
tests/test_gpu_slots.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches the
library) and `call_ctx` (the context of the per-call case).  Pytest collects the imported functions in the importing module, resolves
their fixtures there and applies that module's marks.  Every expected record is worked out in numpy from the ORACLE alone
(tests/slots_ref.py) and every comparison is exact; the inputs and the checks are in tests/slots_cases.py."""
import ctypes as C

import numpy as np
import pytest

import slots_ref as ref
import slots_cases as cases
from stage_backend import lay_out

__all__ = ["ragged", "small", "test_abi_version_is_7", "test_moments_of_a_ragged_multi_tag_batch_equal_the_oracles",
           "test_single_tag_batch", "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero",
           "test_plan_larger_than_the_batch_and_a_new_plan", "test_other_stages_are_untouched",
           "test_per_call_path_on_crafted_windows", "test_protocol_capacity_and_state_errors"]


@pytest.fixture(scope="module")
def ragged(backend, oracle_mod, synth_mod):
    host, lens, L, stride, refs, want = cases.ragged_batch(oracle_mod, synth_mod)
    return host, lens, L, stride, refs, want, backend.put(host, lens)


@pytest.fixture(scope="module")
def small(backend, ragged):
    """the two short traces of the ragged batch (30 and 7 windows) as a batch of their own: what the protocol cases run on"""
    host, lens, L, stride, refs, want, _ = ragged
    w = [r.copy() for r in want[1:]]
    for r in w:
        r["stream"] -= 1
    h, l = np.ascontiguousarray(host[1:]), lens[1:].copy()
    return h, l, L, stride, refs[1:], w, backend.put(h, l)


def test_abi_version_is_7():
    import rfid
    assert rfid.capi.load().rfid_abi_version() == 7


def test_moments_of_a_ragged_multi_tag_batch_equal_the_oracles(backend, ragged):
    """Three traces of 93, 30 and 7 windows, odd row stride; the pass backend.reps times: the same table bytes every time"""
    import rfid
    host, lens, L, stride, refs, want, dev = ragged
    assert all(len(w) % 8 for w in want) and sum((w["flags"] == 3).sum() for w in want) >= 10
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_slots()
        blobs = []
        for rep in range(backend.reps):
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep))
        assert all(b == blobs[0] for b in blobs)
        assert ctx.batch_ls_report()["pieces"] == 0
        ms = ctx.batch_slots_ms()
        assert ms >= 0.0
        print("%s: slots of 3 traces (%d windows): %.4f ms; decode of the same pass %.4f ms" %
              (backend.name, sum(map(len, want)), ms, ctx.batch_timing()["decode_ms"]))
        many = ctx.batch_window_moments(2, extra=10_000)         # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(want[2])], want[2])
        assert not many[len(want[2]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_single_tag_batch(backend, oracle_mod, synth_mod):
    """FIXED_Q = 0, one tag, 8 rounds, in a context of its own: every RN16 and every EPC window"""
    import rfid
    from rfid import batch as rb
    t = ref.shape_trace(synth_mod, ref.SHAPES[1], cases.SIGMA)
    host, lens, L, stride = lay_out([t.samples])
    refs, want = cases.oracle_of(oracle_mod, host, lens, 0)
    assert len(want[0]) == 16 and (want[0]["flags"] == np.tile([0, 3], 8)).all()
    dev = backend.put(host, lens)
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(1, L)
        ctx.batch_plan_slots()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, want)
        got = cases.check_classification(rb, ctx.batch_window_moments(0), t.slots, ref.SHAPES[1])
        assert (got["cls"] == 1).all() and (got["crc_ok"] == 1).all()
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, small):
    """MAX_NUM_QUERIES = 5 reached inside the first trace: nrows == n_windows_used, the rows behind it zero; the second trace ends
    behind an RN16 window: an odd count.  Then in one context: rows an earlier, longer pass had filled are zeroed again"""
    import rfid
    host, lens, L, stride, full_refs, full_want, dev = small
    refs, want = cases.oracle_of(oracle_mod, host, lens, 2, max_num_queries=5)
    assert [o.state.status for o in refs] == [1, 0] and [len(w) for w in want] == [10, 7]
    for mq, w in ((1000, full_want), (5, want)):
        ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=mq)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_slots()
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            cases.check_rows(ctx, w, mq, extra=len(full_want[0]))
            assert [int(s["n_windows_used"]) for s in ctx.batch_stats()] == [len(r) for r in w]
        finally:
            ctx.close()
    # and in ONE context: a long pass fills the rows, a shorter pass behind it must zero them again
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_slots()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, full_want, "full")
        cut = lens.copy()
        cut[0] = cases.cut_behind(oracle_mod, host[0, : lens[0]], 2, 13)
        cut[1] = cases.cut_behind(oracle_mod, host[1, : lens[1]], 2, 4)
        short_refs, short = cases.oracle_of(oracle_mod, host, cut, 2)
        assert [len(r) for r in short] == [13, 4]
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, short, "short", extra=len(full_want[0]))
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_a_new_plan(backend, small):
    """A plan of five traces, two of them processed (rfid_batch_set_streams): two passes give the same table bytes; the traces not
    covered are not fetched; a new plan drops the workspace"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(5, L)
        ctx.batch_plan_slots()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1]
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_moments(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID     # (not covered)
        ctx.batch_plan(2, L)
        for fn in (ctx.batch_slots_enqueue, lambda: ctx.batch_window_moments(0), ctx.batch_slots_ms):
            with pytest.raises(rfid.capi.RfidError) as e:
                fn()
            assert e.value.status == rfid.capi.ERR_STATE
        backend.run_pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_slots_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_slots" in str(e.value)
        ctx.batch_plan_slots()
        ctx.batch_slots_enqueue()                                # (the pass before the workspace: its statistics are current)
        cases.check_rows(ctx, want, "planned again")
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["slots-first", "slots-last"])
def test_other_stages_are_untouched(backend, small, order):
    """inventory + tracks + quality + repair on the same pass, with the slots stage enqueued before or behind them and without it:
    every other fetched array is byte-identical"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    outs = []
    for slots in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            cases.plan_all(ctx, 2, L, slots=slots)
            backend.run_pass(ctx, dev, L, stride)
            if slots and order == "slots-first":
                ctx.batch_slots_enqueue()
            outs.append(cases.other_stage_outputs(ctx, 2))
            if slots and order == "slots-last":
                ctx.batch_slots_enqueue()
            if slots:
                cases.check_rows(ctx, want, order)
                again = cases.other_stage_outputs(ctx, 2)        # (and the stage lowered nothing: the others run again behind it)
                assert again == outs[-1]
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs)), [a == b for a, b in zip(*outs)]
    assert sum(map(len, outs[0])) > 5_000


def test_per_call_path_on_crafted_windows(oracle_mod, ragged, call_ctx):
    import rfid
    host, lens, L, stride, refs, want, _ = ragged
    g = cases.crafted_windows(oracle_mod, host, lens, refs, stream=0, seq=5)
    cases.check_crafted(call_ctx, g, want[0][5])
    with pytest.raises(ValueError):
        call_ctx.window_moments(np.zeros((2, 239), dtype=np.complex64))
    assert call_ctx._lib.rfid_window_moments_of(call_ctx._h, None, 1, None) == rfid.capi.ERR_INVALID
    assert call_ctx._lib.rfid_window_moments_of(call_ctx._h, g.ctypes.data, -1, None) == rfid.capi.ERR_INVALID


def test_protocol_capacity_and_state_errors(backend, small):
    import rfid
    host, lens, L, stride, refs, want, dev = small
    ctx = rfid.Context(device=0, fixed_q=2)
    ERR_STATE, ERR_CAPACITY, ERR_INVALID = rfid.capi.ERR_STATE, rfid.capi.ERR_CAPACITY, rfid.capi.ERR_INVALID

    def raises(fn, status):
        with pytest.raises(rfid.capi.RfidError) as e:
            fn()
        assert e.value.status == status, e.value

    try:
        raises(ctx.batch_plan_slots, ERR_STATE)                   # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_slots_enqueue, ERR_STATE)                # no workspace
        ctx.batch_plan_slots()
        raises(ctx.batch_slots_enqueue, ERR_STATE)                # no pass
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)    # nothing enqueued
        raises(ctx.batch_slots_ms, ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)    # a pass, but nothing enqueued behind it
        ctx.batch_slots_enqueue()                                 # (no inventory workspace: none is needed)
        cases.check_rows(ctx, want, "no inventory")
        # the level of the other stages is neither raised ...
        ctx.batch_plan_inventory(8)                               # (does not drop the slots workspace)
        ctx.batch_plan_tracks()
        ctx.batch_plan_quality()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)               # (the slots stage is not an inventory)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_slots_enqueue()
        ctx.batch_quality_enqueue()                               # ... nor lowered: the tracks are still this pass's
        cases.check_rows(ctx, want, "behind the tracks")
        # a caller's array that is too small loses nothing
        row = np.zeros(len(want[0]) - 1, dtype=rfid.capi.MOMENTS_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_window_moments(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not row.tobytes().strip(b"\0")
        assert "windows" in ctx._lib.rfid_last_error(ctx._h).decode()
        full = np.zeros(n.value, dtype=rfid.capi.MOMENTS_DTYPE)
        assert ctx._lib.rfid_batch_get_window_moments(ctx._h, 0, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        for s in (2, -1):
            assert ctx._lib.rfid_batch_get_window_moments(ctx._h, s, None, 0, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_moments(ctx._h, 0, None, 0, None) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_moments(ctx._h, 0, None, 4, C.byref(n)) == ERR_INVALID
        # what was enqueued behind a pass can still be fetched behind the next one, until the stage is enqueued again
        cut = lens.copy()
        cut[0] = lens[1]                                          # (the first trace ends early)
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ref.assert_equal(ctx.batch_window_moments(0), want[0], "earlier pass")
        ctx.batch_slots_enqueue()
        assert len(ctx.batch_window_moments(0)) < len(want[0])
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_slots_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)
        ctx.batch_plan_slots()
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, want, "new plan")
    finally:
        ctx.close()

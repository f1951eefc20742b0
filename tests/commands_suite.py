"""The cases of the commands stage that run on both sides, written once: tests/test_commands_emu.py (the kernels on the wave emulator)
and tests/test_gpu_commands.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass
reaches the library) and `call_ctx` (the context of the per-call case).  Pytest collects the imported functions in the importing
module, resolves their fixtures there and applies that module's marks.  Every expected record is worked out in numpy from the ORACLE
alone (tests/commands_ref.py) and compared by bytes; what every window's command must BE comes from the synthesiser's slot table.
The inputs and the checks are in tests/commands_cases.py."""
import ctypes as C

import numpy as np
import pytest

import commands_ref as ref
import commands_cases as cases
import slots_cases

__all__ = ["ragged", "small", "test_abi_version_stays_7",
           "test_commands_of_a_ragged_multi_tag_batch_equal_the_oracles_and_the_truth",
           "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero", "test_plan_larger_than_the_batch_and_a_new_plan",
           "test_other_stages_are_untouched", "test_a_clipped_span_at_batch_index_0_and_1", "test_per_call_path_on_crafted_spans",
           "test_protocol_capacity_and_state_errors"]


@pytest.fixture(scope="module")
def ragged(backend, oracle_mod, synth_mod):
    host, lens, L, stride, refs, want, plans = cases.ragged_batch(oracle_mod, synth_mod)
    return host, lens, L, stride, refs, want, plans, backend.put(host, lens)


@pytest.fixture(scope="module")
def small(backend, ragged):
    """the two short traces of the ragged batch (30 and 7 windows) as a batch of their own: what the protocol cases run on"""
    host, lens, L, stride, refs, want, plans, _ = ragged
    w = [r.copy() for r in want[1:]]
    for r in w:
        r["stream"] -= 1
    h, l = np.ascontiguousarray(host[1:]), lens[1:].copy()
    return h, l, L, stride, refs[1:], w, backend.put(h, l)


def test_abi_version_stays_7():
    import rfid
    assert rfid.capi.load().rfid_abi_version() == 7


def test_commands_of_a_ragged_multi_tag_batch_equal_the_oracles_and_the_truth(backend, oracle_mod, ragged):
    """Three traces of 93, 30 and 7 windows, odd row stride; the pass backend.reps times: the same table bytes every time.  EVERY
    window's (cmd, q, crc5, ACKed RN16) is the synthesiser's; every ACK of a slot with one responder echoes the decoded RN16"""
    import rfid
    host, lens, L, stride, refs, want, plans, dev = ragged
    for w, t in zip(want, plans):
        ref.check_truth(w, t, "the reference itself")
    assert sum(int((w["flags"] & 4 != 0).sum()) for w in want) >= 10
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_commands()
        blobs = []
        for rep in range(backend.reps):
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_commands_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep))
        assert all(b == blobs[0] for b in blobs)
        assert ctx.batch_ls_report()["pieces"] == 0
        ctx.batch_plan_slots()
        ctx.batch_slots_enqueue()
        ms = ctx.batch_commands_ms()
        assert ms >= 0.0
        print("%s: commands of 3 traces (%d windows): %.4f ms; decode of the same pass %.4f ms; its slots stage %.4f ms" %
              (backend.name, sum(map(len, want)), ms, ctx.batch_timing()["decode_ms"], ctx.batch_slots_ms()))
        # blocks of several rows per wave (what large batches get): 93, 30 and 7 rows in blocks of 16, 5 and 2 -- full blocks, tails,
        # a last block of one row; the same table bytes
        for rows in (16, 5, 2):
            ctx.set_knob("commands_rows", rows)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_commands_enqueue()
            assert cases.check_rows(ctx, want, ("rows", rows)) == blobs[0]
        ctx.set_knob("commands_rows", 0)
        for b, t in enumerate(plans):
            ref.check_truth(ctx.batch_window_commands(b), t, b)
        many = ctx.batch_window_commands(2, extra=10_000)        # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(want[2])], want[2])
        assert not many[len(want[2]):].tobytes().strip(b"\0")
        cases.check_span_of_a_batch_window(ctx, oracle_mod, host, lens, refs, want[0])
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, small):
    """MAX_NUM_QUERIES = 5 reached inside the first trace: nrows == n_windows_used, the rows behind it zero.  Then in one context:
    rows an earlier, longer pass had filled are zeroed again"""
    import rfid
    host, lens, L, stride, full_refs, full_want, dev = small
    refs, want = cases.oracle_of(oracle_mod, host, lens, 2, max_num_queries=5)
    assert [o.state.status for o in refs] == [1, 0] and [len(w) for w in want] == [10, 7]
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=5)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_commands()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, want, 5, extra=len(full_want[0]))
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_commands()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, full_want, "full")
        cut = lens.copy()
        cut[0] = slots_cases.cut_behind(oracle_mod, host[0, : lens[0]], 2, 13)
        cut[1] = slots_cases.cut_behind(oracle_mod, host[1, : lens[1]], 2, 4)
        short_refs, short = cases.oracle_of(oracle_mod, host, cut, 2)
        assert [len(r) for r in short] == [13, 4]
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, short, "short", extra=len(full_want[0]))
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_a_new_plan(backend, small):
    """A plan of five traces, two of them processed: two passes give the same table bytes; the traces not covered are not fetched;
    a new plan drops the workspace"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(5, L)
        ctx.batch_plan_commands()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_commands_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1]
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_commands(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID     # (not covered)
        ctx.batch_plan(2, L)
        for fn in (ctx.batch_commands_enqueue, lambda: ctx.batch_window_commands(0), ctx.batch_commands_ms):
            with pytest.raises(rfid.capi.RfidError) as e:
                fn()
            assert e.value.status == rfid.capi.ERR_STATE
        backend.run_pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_commands_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_commands" in str(e.value)
        ctx.batch_plan_commands()
        ctx.batch_commands_enqueue()                             # (the pass before the workspace: its statistics are current)
        cases.check_rows(ctx, want, "planned again")
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["commands-first", "commands-last"])
def test_other_stages_are_untouched(backend, small, order):
    """inventory + tracks + quality + repair + slots on the same pass, with the commands stage enqueued before or behind them and
    without it: every other fetched array is byte-identical"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    outs = []
    for commands in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            cases.plan_all(ctx, 2, L, commands=commands)
            backend.run_pass(ctx, dev, L, stride)
            if commands and order == "commands-first":
                ctx.batch_commands_enqueue()
            outs.append(cases.other_stage_outputs(ctx, 2))
            if commands and order == "commands-last":
                ctx.batch_commands_enqueue()
            if commands:
                cases.check_rows(ctx, want, order)
                again = cases.other_stage_outputs(ctx, 2)        # (and the stage lowered nothing: the others run again behind it)
                assert again == outs[-1]
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs)), [a == b for a, b in zip(*outs)]
    assert sum(map(len, outs[0])) > 5_000


def test_a_clipped_span_at_batch_index_0_and_1(backend, oracle_mod, synth_mod):
    """A trace whose first window opens 660 samples behind its start, at batch index 0 and at index 1 (behind a neighbour whose row
    ends high, then low): flag bit 4 is set, the Query is still decoded with a valid CRC-5, and the record does not depend on
    what the neighbouring row holds"""
    import rfid
    seen = []
    for host, lens, L, stride, want, k in cases.clipped_batches(oracle_mod, synth_mod):
        dev = backend.put(host, lens)
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_commands()
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_commands_enqueue()
            cases.check_rows(ctx, want, ("clipped at", k))
            r = ctx.batch_window_commands(k)
            assert int(r["flags"][0]) & 16 and int(r["cmd"][0]) == ref.QUERY and int(r["flags"][0]) & 2
            r["stream"] = 0
            seen.append(r.tobytes())
        finally:
            ctx.close()
    assert seen[0] == seen[1] == seen[2]


def test_per_call_path_on_crafted_spans(synth_mod, call_ctx):
    import rfid
    spans, levels, want = cases.check_crafted(call_ctx, synth_mod)
    for bad in (np.zeros((2, 703), dtype=np.complex64), np.zeros(704, dtype=np.complex64), np.zeros((1, 2, 704), dtype=np.complex64)):
        with pytest.raises(ValueError):
            call_ctx.commands_of(bad, np.zeros(2, dtype=np.complex64))
    with pytest.raises(ValueError):
        call_ctx.commands_of(spans[:2], levels[:1])
    out = np.zeros(1, dtype=rfid.capi.COMMAND_DTYPE)
    lib, h = call_ctx._lib, call_ctx._h
    assert lib.rfid_commands_of(h, None, levels.ctypes.data, 1, out.ctypes.data) == rfid.capi.ERR_INVALID
    assert lib.rfid_commands_of(h, spans.ctypes.data, None, 1, out.ctypes.data) == rfid.capi.ERR_INVALID
    assert lib.rfid_commands_of(h, spans.ctypes.data, levels.ctypes.data, 1, None) == rfid.capi.ERR_INVALID
    assert lib.rfid_commands_of(h, spans.ctypes.data, levels.ctypes.data, -1, out.ctypes.data) == rfid.capi.ERR_INVALID


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
        raises(ctx.batch_plan_commands, ERR_STATE)                # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_commands_enqueue, ERR_STATE)             # no workspace
        ctx.batch_plan_commands()
        raises(ctx.batch_commands_enqueue, ERR_STATE)             # no pass
        raises(lambda: ctx.batch_window_commands(0), ERR_STATE)   # nothing enqueued
        raises(ctx.batch_commands_ms, ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_commands(0), ERR_STATE)   # a pass, but nothing enqueued behind it
        ctx.batch_commands_enqueue()                              # (no inventory workspace: none is needed)
        cases.check_rows(ctx, want, "no inventory")
        # the level of the other stages is neither raised ...
        ctx.batch_plan_inventory(8)                               # (does not drop the commands workspace)
        ctx.batch_plan_tracks()
        ctx.batch_plan_quality()
        ctx.batch_plan_slots()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)               # (the commands stage is not an inventory)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_commands_enqueue()
        ctx.batch_quality_enqueue()                               # ... nor lowered: the tracks are still this pass's
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, want, "behind the tracks")
        # a caller's array that is too small loses nothing
        row = np.zeros(len(want[0]) - 1, dtype=rfid.capi.COMMAND_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_window_commands(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not row.tobytes().strip(b"\0")
        assert "rfid_batch_get_window_commands: cap is smaller than the number of windows" in ctx._lib.rfid_last_error(ctx._h).decode()
        full = np.zeros(n.value, dtype=rfid.capi.COMMAND_DTYPE)
        assert ctx._lib.rfid_batch_get_window_commands(ctx._h, 0, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        for s in (2, -1):
            assert ctx._lib.rfid_batch_get_window_commands(ctx._h, s, None, 0, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_commands(ctx._h, 0, None, 0, None) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_commands(ctx._h, 0, None, 4, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_commands_ms(ctx._h, None) == ERR_INVALID
        # what was enqueued behind a pass can still be fetched behind the next one, until the stage is enqueued again
        cut = lens.copy()
        cut[0] = lens[1]                                          # (the first trace ends early)
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ref.assert_equal(ctx.batch_window_commands(0), want[0], "earlier pass")
        ctx.batch_commands_enqueue()
        assert len(ctx.batch_window_commands(0)) < len(want[0])
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_commands_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_commands(0), ERR_STATE)
        ctx.batch_plan_commands()
        raises(lambda: ctx.batch_window_commands(0), ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, want, "new plan")
    finally:
        ctx.close()

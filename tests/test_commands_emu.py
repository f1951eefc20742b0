"""The commands stage (rfid_batch_plan_commands / rfid_batch_commands / rfid_batch_get_window_commands / rfid_batch_commands_ms, and the
per-call rfid_commands_of: the reader's own PIE command in front of every window, decoded on the device behind a pass) on the CPU:
csrc/rfid_capi.hip and csrc/rfid_commands.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave emulator.
Every expected record is worked out in numpy from the ORACLE alone (tests/commands_ref.py), never from the library's own windows, and
every comparison is by bytes; what every window's command must BE comes from the synthesiser's slot table.  The inputs and the checks
shared with tests/test_gpu_commands.py are in tests/commands_cases.py."""
import ctypes as C

import numpy as np
import pytest

import commands_ref as ref
import commands_cases as cases
import emu_lib
from emu_lib import run_pass as _pass


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


@pytest.fixture(scope="module")
def ragged(oracle_mod, synth_mod):
    return cases.ragged_batch(oracle_mod, synth_mod)


@pytest.fixture(scope="module")
def small(ragged):
    """the two short traces of the ragged batch (30 and 7 windows) as a batch of their own: what the protocol cases run on"""
    host, lens, L, stride, refs, want, plans = ragged
    w = [r.copy() for r in want[1:]]
    for r in w:
        r["stream"] -= 1
    return np.ascontiguousarray(host[1:]), lens[1:].copy(), L, stride, refs[1:], w


def test_abi_version_stays_7(emulated_library):
    assert emulated_library.rfid_abi_version() == 7


def test_commands_of_a_ragged_multi_tag_batch_equal_the_oracles_and_the_truth(oracle_mod, ragged):
    """Three traces of 93, 30 and 7 windows, odd row stride; the pass twice: the same table bytes both times.  EVERY window's
    (cmd, q, crc5, ACKed RN16) is the synthesiser's; every ACK of a slot with one responder echoes the decoded RN16"""
    import rfid
    host, lens, L, stride, refs, want, plans = ragged
    for w, t in zip(want, plans):
        ref.check_truth(w, t, "the reference itself")
    assert sum(int((w["flags"] & 4 != 0).sum()) for w in want) >= 10
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_commands()
        blobs = []
        for rep in range(2):
            _pass(ctx, host, lens, L, stride)
            ctx.batch_commands_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1]
        # blocks of several rows per wave (what large batches get): 93, 30 and 7 rows in blocks of 16, 5 and 2 -- full blocks, tails,
        # a last block of one row; the same table bytes
        for rows in (16, 5, 2):
            ctx.set_knob("commands_rows", rows)
            _pass(ctx, host, lens, L, stride)
            ctx.batch_commands_enqueue()
            assert cases.check_rows(ctx, want, ("rows", rows)) == blobs[0]
        ctx.set_knob("commands_rows", 0)
        assert ctx.batch_commands_ms() >= 0.0
        for b, t in enumerate(plans):
            ref.check_truth(ctx.batch_window_commands(b), t, b)
        many = ctx.batch_window_commands(2, extra=10_000)        # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(want[2])], want[2])
        assert not many[len(want[2]):].tobytes().strip(b"\0")
        cases.check_span_of_a_batch_window(ctx, oracle_mod, host, lens, refs, want[0])
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(oracle_mod, small):
    """MAX_NUM_QUERIES = 5 reached inside the first trace: nrows == n_windows_used, the rows behind it zero.  Then in one context:
    rows an earlier, longer pass had filled are zeroed again"""
    import rfid
    import slots_cases
    host, lens, L, stride, full_refs, full_want = small
    refs, want = cases.oracle_of(oracle_mod, host, lens, 2, max_num_queries=5)
    assert [o.state.status for o in refs] == [1, 0] and [len(w) for w in want] == [10, 7]
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=5)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_commands()
        _pass(ctx, host, lens, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, want, 5, extra=len(full_want[0]))
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_commands()
        _pass(ctx, host, lens, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, full_want, "full")
        cut = lens.copy()
        cut[0] = slots_cases.cut_behind(oracle_mod, host[0, : lens[0]], 2, 13)
        cut[1] = slots_cases.cut_behind(oracle_mod, host[1, : lens[1]], 2, 4)
        short_refs, short = cases.oracle_of(oracle_mod, host, cut, 2)
        assert [len(r) for r in short] == [13, 4]
        _pass(ctx, host, cut, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, short, "short", extra=len(full_want[0]))
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_a_new_plan(small):
    """A plan of five traces, two of them processed: two passes give the same table bytes; the traces not covered are not fetched;
    a new plan drops the workspace"""
    import rfid
    host, lens, L, stride, refs, want = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(5, L)
        ctx.batch_plan_commands()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            _pass(ctx, host, lens, L, stride)
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
        _pass(ctx, host, lens, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_commands_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_commands" in str(e.value)
        ctx.batch_plan_commands()
        ctx.batch_commands_enqueue()                             # (the pass before the workspace: its statistics are current)
        cases.check_rows(ctx, want, "planned again")
    finally:
        ctx.close()


def test_workgroups_go_round_their_loop_again(ragged):
    """The ragged batch under a plan for traces seven times as long, at one row per block (the knob commands_rows): more (trace,
    row) items than the launch has workgroups (20 per compute unit, 256 of them), so a workgroup of commands_kernel takes a second
    item.  The third trace's rows lie behind the first 5 120 items: its seven windows are second items with work, behind first
    items behind a cut-off, and the rows behind them second items behind a cut-off.  The stage twice: the same table bytes"""
    import rfid
    host, lens, L, stride, refs, want, plans = ragged
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, 7 * L)
        ctx.batch_plan_commands()
        ctx.set_knob("commands_rows", 1)
        _pass(ctx, host, lens, L, stride)
        blobs = []
        for rep in range(2):
            ctx.batch_commands_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep, extra=4000))       # (every row of the table)
        assert blobs[0] == blobs[1]
        wmax = cases.table_rows(ctx, 7 * L)
        assert 5120 < 2 * wmax and 3 * wmax < 2 * 5120 and wmax < 4000, wmax
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["commands-first", "commands-last"])
def test_other_stages_are_untouched(small, order):
    """inventory + tracks + quality + repair + slots on the same pass, with the commands stage enqueued before or behind them and
    without it: every other fetched array is byte-identical"""
    import rfid
    host, lens, L, stride, refs, want = small
    outs = []
    for commands in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            cases.plan_all(ctx, 2, L, commands=commands)
            _pass(ctx, host, lens, L, stride)
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


def test_a_clipped_span_at_batch_index_0_and_1(oracle_mod, synth_mod):
    """A trace whose first window opens 660 samples behind its start, at batch index 0 and at index 1 (behind a neighbour whose row
    ends high, then low): flag bit 4 is set, the Query is still decoded with a valid CRC-5, and the record does not depend on
    what the neighbouring row holds"""
    import rfid
    seen = []
    for host, lens, L, stride, want, k in cases.clipped_batches(oracle_mod, synth_mod):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_commands()
            _pass(ctx, host, lens, L, stride)
            ctx.batch_commands_enqueue()
            cases.check_rows(ctx, want, ("clipped at", k))
            r = ctx.batch_window_commands(k)
            assert int(r["flags"][0]) & 16 and int(r["cmd"][0]) == ref.QUERY and int(r["flags"][0]) & 2
            r["stream"] = 0
            seen.append(r.tobytes())
        finally:
            ctx.close()
    assert seen[0] == seen[1] == seen[2]


def test_per_call_path_on_crafted_spans(synth_mod):
    import rfid
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        spans, levels, want = cases.check_crafted(ctx, synth_mod)
        for bad in (np.zeros((2, 703), dtype=np.complex64), np.zeros(704, dtype=np.complex64), np.zeros((1, 2, 704), dtype=np.complex64)):
            with pytest.raises(ValueError):
                ctx.commands_of(bad, np.zeros(2, dtype=np.complex64))
        with pytest.raises(ValueError):
            ctx.commands_of(spans[:2], levels[:1])
        out = np.zeros(1, dtype=rfid.capi.COMMAND_DTYPE)
        lib, h = ctx._lib, ctx._h
        assert lib.rfid_commands_of(h, None, levels.ctypes.data, 1, out.ctypes.data) == rfid.capi.ERR_INVALID
        assert lib.rfid_commands_of(h, spans.ctypes.data, None, 1, out.ctypes.data) == rfid.capi.ERR_INVALID
        assert lib.rfid_commands_of(h, spans.ctypes.data, levels.ctypes.data, 1, None) == rfid.capi.ERR_INVALID
        assert lib.rfid_commands_of(h, spans.ctypes.data, levels.ctypes.data, -1, out.ctypes.data) == rfid.capi.ERR_INVALID
    finally:
        ctx.close()


def test_protocol_capacity_and_state_errors(small):
    import rfid
    host, lens, L, stride, refs, want = small
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
        _pass(ctx, host, lens, L, stride)
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
        _pass(ctx, host, cut, L, stride)
        ref.assert_equal(ctx.batch_window_commands(0), want[0], "earlier pass")
        ctx.batch_commands_enqueue()
        assert len(ctx.batch_window_commands(0)) < len(want[0])
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_commands_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_commands(0), ERR_STATE)
        ctx.batch_plan_commands()
        raises(lambda: ctx.batch_window_commands(0), ERR_STATE)
        _pass(ctx, host, lens, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, want, "new plan")
    finally:
        ctx.close()


def test_host_functions(ragged):
    """command_fields, command_bits, format_commands and format_commands_csv on emulator records and crafted ones"""
    import rfid
    from rfid import batch as rb
    host, lens, L, stride, refs, want, plans = ragged
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_commands()
        _pass(ctx, host, lens, L, stride)
        ctx.batch_commands_enqueue()
        rows = [ctx.batch_window_commands(b) for b in range(3)]
    finally:
        ctx.close()
    r, truth = rows[1], ref.plan_truth(plans[1])[:30]
    f = rb.command_fields(r)
    assert len(f) == 30 and np.array_equal(f["seq"], np.arange(30))
    names = {ref.QUERY: "query", ref.QUERY_REP: "queryrep", ref.ACK: "ack"}
    for k, (g, t) in enumerate(zip(f, truth)):
        assert (g["name"], int(g["q"]), int(g["crc5_ok"]), int(g["rn16"])) == (names[t[0]], t[1], t[2], t[3]), (k, g, t)
        assert int(g["ack_echo"]) == (-1 if t[0] != ref.ACK else (int(r["flags"][k]) >> 2) & 1) and (not t[4] or int(g["ack_echo"]) == 1)
        assert g["rtcal_us"] == 2.5 * int(r["rtcal"][k]) and g["t1_us"] == 2.5 * (704 - int(r["end"][k]))
        assert (g["trcal_us"] == 200.0) if t[0] == ref.QUERY else np.isnan(g["trcal_us"])
    assert rb.command_bits(r[1]) == "01" + format(truth[1][3], "016b") and rb.command_bits(r[0])[:4] == "1000" and len(rb.command_bits(r[0])) == 22
    n_q, n_a = sum(t[0] == ref.QUERY for t in truth), 15
    echo = int((r["flags"] & 4 != 0).sum())
    line = rb.format_commands(r)
    assert line == ("| commands : 30  query : %d  queryrep : %d  ack : %d  other : 0  none : 0  Q : {2}  failed CRC-5 : 0  "
                    "ACKs echoing the decoded RN16 : %d of %d  median RTcal us : %s  TRcal us : 200.0  T1 us : %s\n" %
                    (n_q, 15 - n_q, n_a, echo, n_a, "%.1f" % np.median(2.5 * r["rtcal"]), "%.1f" % np.median(2.5 * (704 - r["end"]))))
    assert echo >= sum(t[4] for t in truth) > 0 and line.count("\n") == 1
    # crafted records: a Query whose CRC-5 failed, an unknown command, nothing at all
    odd = np.zeros(4, dtype=rfid.capi.COMMAND_DTYPE)
    odd["seq"] = np.arange(4)
    odd[0] = r[0]
    odd[0]["flags"] &= ~2
    odd[1]["cmd"], odd[1]["n_bits"], odd[1]["bits"], odd[1]["n_syms"], odd[1]["end"], odd[1]["rtcal"] = ref.UNKNOWN, 40, 0x80000005, 43, 600, 30
    odd[2]["cmd"], odd[2]["n_bits"], odd[2]["bits"], odd[2]["n_syms"], odd[2]["end"], odd[2]["rtcal"], odd[2]["seq"] = ref.NAK, 8, 3, 11, 610, 28, 2
    line = rb.format_commands(odd)
    assert line.startswith("| commands : 4  query : 1  queryrep : 0  ack : 0  other : 2  none : 1  Q : {2}  failed CRC-5 : 1  "
                           "ACKs echoing the decoded RN16 : 0 of 0  median RTcal us : 72.5  TRcal us : 200.0  T1 us : ")
    assert rb.format_commands(odd[3:]).endswith("Q : -  failed CRC-5 : 0  ACKs echoing the decoded RN16 : 0 of 0  median RTcal us : -  TRcal us : -  T1 us : -\n")
    assert rb.command_bits(odd[1]) == "101" + "0" * 28 + "1"
    starts = [1000 + 400 * np.arange(30), np.arange(4)]
    text = rb.format_commands_csv([r, odd], starts, ["a.bin", "b.bin"])
    lines = text.splitlines()
    assert lines[0] == rb.COMMANDS_HEADER == "file,seq,t_s,cmd,n_bits,bits,q,rn16,crc5_ok,ack_echo,rtcal_us,trcal_us,t1_us" and len(lines) == 1 + 30 + 4
    for k, line in enumerate(lines[1:31]):
        c, t, g = line.split(","), truth[k], f[k]
        assert c[:2] == ["a.bin", str(k)] and c[2] == "%.9g" % (starts[0][k] / 400e3) and c[3] == names[t[0]]
        assert c[4] == str(int(r["n_bits"][k])) and c[5] == rb.command_bits(r[k])
        assert c[6] == (str(t[1]) if t[0] == ref.QUERY else "") and c[7] == ("%04x" % t[3] if t[0] == ref.ACK else "")
        assert c[8] == ("1" if t[0] == ref.QUERY else "") and c[9] == (str(int(g["ack_echo"])) if t[0] == ref.ACK else "")
        assert c[10] == "%.1f" % g["rtcal_us"] and c[11] == ("200.0" if t[0] == ref.QUERY else "") and c[12] == "%.1f" % g["t1_us"]
    assert lines[31].split(",")[8] == "0" and lines[32].startswith("b.bin,1,2.5e-06,unknown,40,101" + "0" * 28 + "1,,,,,75.0,,260.0")
    assert lines[33].startswith("b.bin,2,5e-06,nak,8,11000000,,,,,70.0,,235.0") and lines[34] == "b.bin,3,7.5e-06,none,0,,,,,,,,"

"""The commands stage on the device (rfid_batch_plan_commands / rfid_batch_commands / rfid_batch_get_window_commands /
rfid_batch_commands_ms, and the per-call rfid_commands_of): the reader's own PIE command in front of every window.  Every expected
record is worked out in numpy from the ORACLE alone (tests/commands_ref.py) and compared by bytes; what every window's command must BE
comes from the synthesiser's slot table.  The inputs and the checks are those of tests/test_commands_emu.py (tests/commands_cases.py):
the smallest shapes at which the kernel can still go wrong -- edges at the seams of the ballots, 64 / 65 edges, gaps of 120 / 121,
ties, odd counts, more than one trace, rows behind a cut-off, a span clipped at the trace's start."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import commands_ref as ref
import commands_cases as cases
import slots_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _dev(host, lens):
    """-> (device tensor of the traces, device tensor of their lengths); the caller keeps both alive"""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(host).view(np.float32)).to("cuda:0")
    dlens = torch.from_numpy(np.ascontiguousarray(lens)).to("cuda:0")
    torch.cuda.synchronize()
    return dev, dlens


@pytest.fixture(scope="module")
def ragged(oracle_mod, synth_mod):
    host, lens, L, stride, refs, want, plans = cases.ragged_batch(oracle_mod, synth_mod)
    return host, lens, L, stride, refs, want, plans, _dev(host, lens)


@pytest.fixture(scope="module")
def small(ragged):
    """the two short traces of the ragged batch (30 and 7 windows) as a batch of their own"""
    host, lens, L, stride, refs, want, plans, _ = ragged
    w = [r.copy() for r in want[1:]]
    for r in w:
        r["stream"] -= 1
    h, l = np.ascontiguousarray(host[1:]), lens[1:].copy()
    return h, l, L, stride, refs[1:], w, _dev(h, l)


def _pass(ctx, dev, L, stride):
    ctx.batch_process_ptr(dev[0].data_ptr(), stride, L, dev[1].data_ptr())


def test_abi_version_stays_7():
    import rfid
    assert rfid.capi.load().rfid_abi_version() == 7


def test_commands_of_a_ragged_multi_tag_batch_equal_the_oracles_and_the_truth(oracle_mod, ragged):
    """Three traces of 93, 30 and 7 windows, odd row stride; the pass three times: the same table bytes every time.  EVERY window's
    (cmd, q, crc5, ACKed RN16) is the synthesiser's; every ACK of a slot with one responder echoes the decoded RN16"""
    import rfid
    host, lens, L, stride, refs, want, plans, dev = ragged
    for w, t in zip(want, plans):
        ref.check_truth(w, t, "the reference itself")
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_commands()
        blobs = []
        for rep in range(3):
            _pass(ctx, dev, L, stride)
            ctx.batch_commands_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1] == blobs[2]
        assert ctx.batch_ls_report()["pieces"] == 0
        ctx.batch_plan_slots()
        ctx.batch_slots_enqueue()
        print("commands of 3 traces (%d windows): %.4f ms; decode of the same pass %.4f ms; its slots stage %.4f ms" %
              (sum(map(len, want)), ctx.batch_commands_ms(), ctx.batch_timing()["decode_ms"], ctx.batch_slots_ms()))
        # blocks of several rows per wave (what large batches get): 93, 30 and 7 rows in blocks of 16, 5 and 2 -- full blocks, tails,
        # a last block of one row; the same table bytes
        for rows in (16, 5, 2):
            ctx.set_knob("commands_rows", rows)
            _pass(ctx, dev, L, stride)
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


def test_long_stream_front_end_gives_the_same_records(ragged):
    """rfid_batch_set_long_stream mode 2 on one trace (the 93-window one): the records of the fused front end, the oracle's"""
    import rfid
    host, lens, L, stride, refs, want, plans, _ = ragged
    dev = _dev(host[:1], lens[:1])
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(1, L)
        ctx.batch_plan_commands()
        blobs = []
        for mode in (2, 0, 2):
            ctx.batch_set_long_stream(mode)
            _pass(ctx, dev, L, stride)
            ctx.batch_commands_enqueue()
            blobs.append(cases.check_rows(ctx, want[:1], mode))
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        assert blobs[0] == blobs[1] == blobs[2]
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(oracle_mod, small):
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
        _pass(ctx, dev, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, want, 5, extra=len(full_want[0]))
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_commands()
        _pass(ctx, dev, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, full_want, "full")
        cut = lens.copy()
        cut[0] = slots_cases.cut_behind(oracle_mod, host[0, : lens[0]], 2, 13)
        cut[1] = slots_cases.cut_behind(oracle_mod, host[1, : lens[1]], 2, 4)
        short_refs, short = cases.oracle_of(oracle_mod, host, cut, 2)
        assert [len(r) for r in short] == [13, 4]
        dcut = _dev(host, cut)
        _pass(ctx, dcut, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, short, "short", extra=len(full_want[0]))
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_a_new_plan(small):
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
            _pass(ctx, dev, L, stride)
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
        _pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_commands_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_commands" in str(e.value)
        ctx.batch_plan_commands()
        ctx.batch_commands_enqueue()                             # (the pass before the workspace: its statistics are current)
        cases.check_rows(ctx, want, "planned again")
    finally:
        ctx.close()


def test_two_result_sets_each_pass_gets_its_own_records(small):
    """44 traces (the two short ones, 22 times) at one row per block (the knob commands_rows: the stage would pack four): more
    (trace, row) items than the launch has workgroups, so a workgroup of commands_kernel goes round its loop again -- past blocks
    behind the cut-off and blocks with work alike.  Two result sets alternating (RFID_OVERLAP=2): the next pass -- the traces in
    the other order -- enqueued BEFORE this pass's records are fetched leaves them this pass's, then gets its own"""
    import rfid
    host, lens, L, stride, refs, want, _ = small
    order = np.arange(44) % 2
    dev_a = _dev(host[order], lens[order])
    dev_b = _dev(host[1 - order], lens[1 - order])

    def stamped(which):
        out = []
        for b, k in enumerate(which):
            r = want[k].copy()
            r["stream"] = b
            out.append(r)
        return out

    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.set_knob("overlap", 2)
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(44, L)
        ctx.batch_plan_commands()
        ctx.set_knob("commands_rows", 1)
        looped = False
        for rep in range(2):
            _pass(ctx, dev_a, L, stride)
            ctx.batch_commands_enqueue()
            _pass(ctx, dev_b, L, stride)
            for b, w in enumerate(stamped(order)):
                ref.assert_equal(ctx.batch_window_commands(b), w, ("a", rep, b))
            ctx.batch_commands_enqueue()
            cases.check_rows(ctx, stamped(1 - order), ("b", rep))
            if not looped:       # (the launch has at most 20 workgroups per compute unit)
                import torch
                wmax = cases.table_rows(ctx, L)
                assert 44 * wmax > 2 * 20 * torch.cuda.get_device_properties(0).multi_processor_count, wmax
                looped = True
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["commands-first", "commands-last"])
def test_other_stages_are_untouched(small, order):
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
            _pass(ctx, dev, L, stride)
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
        dev = _dev(host, lens)
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_commands()
            _pass(ctx, dev, L, stride)
            ctx.batch_commands_enqueue()
            cases.check_rows(ctx, want, ("clipped at", k))
            r = ctx.batch_window_commands(k)
            assert int(r["flags"][0]) & 16 and int(r["cmd"][0]) == ref.QUERY and int(r["flags"][0]) & 2
            r["stream"] = 0
            seen.append(r.tobytes())
        finally:
            ctx.close()
    assert seen[0] == seen[1] == seen[2]


def test_per_call_path_on_crafted_spans(synth_mod, gpu_ctx):
    import rfid
    spans, levels, want = cases.check_crafted(gpu_ctx, synth_mod)
    with pytest.raises(ValueError):
        gpu_ctx.commands_of(np.zeros((2, 703), dtype=np.complex64), np.zeros(2, dtype=np.complex64))
    out = np.zeros(1, dtype=rfid.capi.COMMAND_DTYPE)
    lib, h = gpu_ctx._lib, gpu_ctx._h
    assert lib.rfid_commands_of(h, None, levels.ctypes.data, 1, out.ctypes.data) == rfid.capi.ERR_INVALID
    assert lib.rfid_commands_of(h, spans.ctypes.data, None, 1, out.ctypes.data) == rfid.capi.ERR_INVALID
    assert lib.rfid_commands_of(h, spans.ctypes.data, levels.ctypes.data, -1, out.ctypes.data) == rfid.capi.ERR_INVALID
    # more blocks of sixteen spans (1 063) than the launch has workgroups (two per compute unit): a workgroup goes round its loop again
    reps = -(-17_001 // len(spans))
    big = np.ascontiguousarray(np.tile(spans, (reps, 1))[:17_001])
    big_levels = np.ascontiguousarray(np.tile(levels, reps)[:17_001])
    big_want = np.tile(want, reps)[:17_001]
    big_want["seq"] = np.arange(17_001)
    got = gpu_ctx.commands_of(big, big_levels)
    assert len(got) == 17_001 and int(got["seq"][-1]) == 17_000
    ref.assert_equal(got, big_want, "17 001 spans")


def test_protocol_capacity_and_state_errors(small):
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
        _pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_commands(0), ERR_STATE)   # a pass, but nothing enqueued behind it
        ctx.batch_commands_enqueue()                              # (no inventory workspace: none is needed)
        cases.check_rows(ctx, want, "no inventory")
        ctx.batch_plan_inventory(8)                               # (does not drop the commands workspace)
        ctx.batch_plan_tracks()
        ctx.batch_plan_quality()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)               # (the commands stage is not an inventory: the level is not raised ...)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_commands_enqueue()
        ctx.batch_quality_enqueue()                               # (... nor lowered: the tracks are still this pass's)
        cases.check_rows(ctx, want, "behind the tracks")
        row = np.zeros(len(want[0]) - 1, dtype=rfid.capi.COMMAND_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_window_commands(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not row.tobytes().strip(b"\0")
        full = np.zeros(n.value, dtype=rfid.capi.COMMAND_DTYPE)
        assert ctx._lib.rfid_batch_get_window_commands(ctx._h, 0, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        for s in (2, -1):
            assert ctx._lib.rfid_batch_get_window_commands(ctx._h, s, None, 0, C.byref(n)) == ERR_INVALID
        ctx.batch_plan(2, L)                                      # a new plan drops the workspace
        raises(ctx.batch_commands_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_commands(0), ERR_STATE)
        ctx.batch_plan_commands()
        _pass(ctx, dev, L, stride)
        ctx.batch_commands_enqueue()
        cases.check_rows(ctx, want, "new plan")
    finally:
        ctx.close()


def test_command_line_writes_the_commands_csv_and_a_line_per_file(oracle_mod, synth_mod, tmp_path):
    """python -m rfid.batch --commands OUT.csv on two trace files, in a fresh child process: exit status 0, one commands line per file
    behind its results block, the CSV's commands, Q and ACKed RN16 are the truth; nothing else is printed (--commands implies nothing)"""
    from rfid import batch as rb
    import slots_ref
    paths, rows, starts, truth = [], [], [], []
    for k, shape in enumerate((slots_ref.SHAPES[4], (2, (1, 2, 3), 3, 21))):
        t = slots_ref.shape_trace(synth_mod, shape, cases.SIGMA)
        p = str(tmp_path / ("trace%d.bin" % k))
        rb.write_trace_file(p, t.samples)
        paths.append(p)
        o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=2))
        rows.append(ref.expected(o, oracle_mod.fir(t.samples), k))
        starts.append(np.asarray(o.open_idx))
        truth.append(ref.plan_truth(t))
        ref.check_truth(rows[-1], t, k)
        assert len(rows[-1]) == len(truth[-1]) == 2 * shape[2] << 2
    csv = str(tmp_path / "commands.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    r = subprocess.run([sys.executable, "-m", "rfid.batch", "--fixed-q", "2", "--commands", csv] + paths, env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert " tags\n" not in out and "EPC windows :" not in out and "| slots :" not in out
    rule = " --------------------------\n"
    for k, p in enumerate(paths):
        line = rb.format_commands(rows[k])
        assert out.count(line) == 1, (line, out)
        at = out.index(line)
        assert out[at - len(rule):at] == rule and out.index(p + "\n") < at
        assert k + 1 == len(paths) or at < out.index(paths[k + 1] + "\n")
        n_q = sum(t[0] == ref.QUERY for t in truth[k])
        n_w = len(truth[k])
        singles = sum(t[4] for t in truth[k])
        assert line.startswith("| commands : %d  query : %d  queryrep : %d  ack : %d  other : 0  none : 0  Q : {2}  failed CRC-5 : 0  " %
                               (n_w, n_q, n_w // 2 - n_q, n_w // 2)), line
        assert int(line.split("RN16 : ")[1].split(" of ")[0]) >= singles > 0 and (" of %d  median" % (n_w // 2)) in line
    text = open(csv).read()
    assert text == rb.format_commands_csv(rows, starts, paths)
    lines = text.splitlines()
    assert lines[0] == rb.COMMANDS_HEADER and len(lines) == 1 + sum(map(len, truth))
    names = {ref.QUERY: "query", ref.QUERY_REP: "queryrep", ref.ACK: "ack"}
    i = 1
    for k, p in enumerate(paths):
        for j, t in enumerate(truth[k]):
            f = lines[i].split(",")
            assert f[:2] == [p, str(j)] and f[3] == names[t[0]] and abs(float(f[2]) - starts[k][j] / 400e3) <= 1e-9, (lines[i], t)
            assert f[6] == (str(t[1]) if t[0] == ref.QUERY else "") and f[7] == ("%04x" % t[3] if t[0] == ref.ACK else ""), (lines[i], t)
            assert f[8] == ("1" if t[0] == ref.QUERY else "") and (not t[4] or f[9] == "1"), (lines[i], t)
            i += 1

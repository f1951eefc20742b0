"""The slots stage (rfid_batch_plan_slots / rfid_batch_slots / rfid_batch_get_window_moments / rfid_batch_slots_ms, and the per-call
rfid_window_moments_of: the second-order moments of every window's gated samples, built on the device behind a pass) on the CPU:
csrc/rfid_capi.hip and csrc/rfid_slots.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave emulator.  Every
expected record is worked out in numpy from the ORACLE alone (tests/slots_ref.py), never from the library's own windows, and every
comparison is exact: by bit pattern, then by the bytes of the whole arrays.  The inputs and the checks shared with
tests/test_gpu_slots.py are in tests/slots_cases.py."""
import ctypes as C

import numpy as np
import pytest

import slots_ref as ref
import slots_cases as cases
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
    host, lens, L, stride, refs, want = ragged
    w = [r.copy() for r in want[1:]]
    for r in w:
        r["stream"] -= 1
    return np.ascontiguousarray(host[1:]), lens[1:].copy(), L, stride, refs[1:], w


def test_abi_version_is_7(emulated_library):
    assert emulated_library.rfid_abi_version() == 7


def test_moments_of_a_ragged_multi_tag_batch_equal_the_oracles(ragged):
    """Three traces of 93, 30 and 7 windows, odd row stride; the pass twice: the same table bytes both times"""
    import rfid
    host, lens, L, stride, refs, want = ragged
    assert all(len(w) % 8 for w in want) and sum((w["flags"] == 3).sum() for w in want) >= 10
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_slots()
        blobs = []
        for rep in range(2):
            _pass(ctx, host, lens, L, stride)
            ctx.batch_slots_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1]
        assert ctx.batch_slots_ms() >= 0.0
        many = ctx.batch_window_moments(2, extra=10_000)         # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(want[2])], want[2])
        assert not many[len(want[2]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_single_tag_batch(oracle_mod, synth_mod):
    """FIXED_Q = 0, one tag, 8 rounds, in a context of its own: every RN16 and every EPC window"""
    import rfid
    from rfid import batch as rb
    t = ref.shape_trace(synth_mod, ref.SHAPES[1], cases.SIGMA)
    host, lens, L, stride = cases.lay_out([t.samples], odd_stride=False)
    refs, want = cases.oracle_of(oracle_mod, host, lens, 0)
    assert len(want[0]) == 16 and (want[0]["flags"] == np.tile([0, 3], 8)).all()
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(1, L)
        ctx.batch_plan_slots()
        _pass(ctx, host, lens, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, want)
        got = cases.check_classification(rb, ctx.batch_window_moments(0), t.slots, ref.SHAPES[1])
        assert (got["cls"] == 1).all() and (got["crc_ok"] == 1).all()
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(oracle_mod, small):
    """MAX_NUM_QUERIES = 5 reached inside the first trace: nrows == n_windows_used, the rows behind it zero; the second trace ends
    behind an RN16 window: an odd count.  Then in one context: rows an earlier, longer pass had filled are zeroed again"""
    import rfid
    host, lens, L, stride, full_refs, full_want = small
    refs, want = cases.oracle_of(oracle_mod, host, lens, 2, max_num_queries=5)
    assert [o.state.status for o in refs] == [1, 0] and [len(w) for w in want] == [10, 7]
    for mq, w in ((1000, full_want), (5, want)):
        ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=mq)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_slots()
            _pass(ctx, host, lens, L, stride)
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
        _pass(ctx, host, lens, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, full_want, "full")
        cut = lens.copy()
        cut[0] = cases.cut_behind(oracle_mod, host[0, : lens[0]], 2, 13)
        cut[1] = cases.cut_behind(oracle_mod, host[1, : lens[1]], 2, 4)
        short_refs, short = cases.oracle_of(oracle_mod, host, cut, 2)
        assert [len(r) for r in short] == [13, 4]
        _pass(ctx, host, cut, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, short, "short", extra=len(full_want[0]))
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_a_new_plan(small):
    """A plan of five traces, two of them processed (rfid_batch_set_streams): two passes give the same table bytes; the traces not
    covered are not fetched; a new plan drops the workspace"""
    import rfid
    host, lens, L, stride, refs, want = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(5, L)
        ctx.batch_plan_slots()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            _pass(ctx, host, lens, L, stride)
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
        _pass(ctx, host, lens, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_slots_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_slots" in str(e.value)
        ctx.batch_plan_slots()
        ctx.batch_slots_enqueue()                                # (the pass before the workspace: its statistics are current)
        cases.check_rows(ctx, want, "planned again")
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["slots-first", "slots-last"])
def test_other_stages_are_untouched(small, order):
    """inventory + tracks + quality + repair on the same pass, with the slots stage enqueued before or behind them and without it:
    every other fetched array is byte-identical"""
    import rfid
    host, lens, L, stride, refs, want = small
    outs = []
    for slots in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            cases.plan_all(ctx, 2, L, slots=slots)
            _pass(ctx, host, lens, L, stride)
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


def test_per_call_path_on_crafted_windows(oracle_mod, ragged):
    import rfid
    host, lens, L, stride, refs, want = ragged
    g = cases.crafted_windows(oracle_mod, host, lens, refs, stream=0, seq=5)
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        cases.check_crafted(ctx, g, want[0][5])
        with pytest.raises(ValueError):
            ctx.window_moments(np.zeros((2, 239), dtype=np.complex64))
        assert ctx._lib.rfid_window_moments_of(ctx._h, None, 1, None) == rfid.capi.ERR_INVALID
        assert ctx._lib.rfid_window_moments_of(ctx._h, g.ctypes.data, -1, None) == rfid.capi.ERR_INVALID
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
        raises(ctx.batch_plan_slots, ERR_STATE)                   # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_slots_enqueue, ERR_STATE)                # no workspace
        ctx.batch_plan_slots()
        raises(ctx.batch_slots_enqueue, ERR_STATE)                # no pass
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)    # nothing enqueued
        raises(ctx.batch_slots_ms, ERR_STATE)
        _pass(ctx, host, lens, L, stride)
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
        _pass(ctx, host, cut, L, stride)
        ref.assert_equal(ctx.batch_window_moments(0), want[0], "earlier pass")
        ctx.batch_slots_enqueue()
        assert len(ctx.batch_window_moments(0)) < len(want[0])
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_slots_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)
        ctx.batch_plan_slots()
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)
        _pass(ctx, host, lens, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, want, "new plan")
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def classified(oracle_mod, synth_mod):
    """the five shapes at sigma = 0.01, each through a pass of its own context: -> per shape (trace, emulator records)"""
    import rfid
    out = []
    for shape in ref.SHAPES:
        t = ref.shape_trace(synth_mod, shape, cases.SIGMA)
        host, lens, L, stride = cases.lay_out([t.samples], odd_stride=False)
        ctx = rfid.Context(device=0, fixed_q=shape[0])
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(1, L)
            ctx.batch_plan_slots()
            _pass(ctx, host, lens, L, stride)
            ctx.batch_slots_enqueue()
            rows = ctx.batch_window_moments(0)
        finally:
            ctx.close()
        o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=shape[0]))
        ref.assert_equal(rows, ref.expected(o, oracle_mod.fir(t.samples)), shape)
        out.append((t, rows))
    return out


def test_classification_agrees_with_the_truth_on_the_five_shapes(classified):
    """classify_slots == SlotTruth for EVERY slot of every shape (no slot may be left out), == the restatement of slots_ref; the
    reference classification itself is within that on these inputs"""
    from rfid import batch as rb
    for shape, (t, rows) in zip(ref.SHAPES, classified):
        assert [c[:2] for c in ref.classify(rows)] == ref.truth(t.slots), shape        # (the reference alone)
        got = cases.check_classification(rb, rows, t.slots, shape)
        assert len(got) == shape[2] << shape[0]
    t, rows = classified[2]
    assert sum(s.n_tags >= 2 for s in t.slots) == 22 and len(t.slots) == 24            # (most slots collide: the floor is the EPC windows')
    t, rows = classified[0]
    est = rb.estimate_population(rb.classify_slots(rows)["cls"], 12)
    assert "%.2f" % est == "4.82" and rb.suggest_q(est) == 2


def test_host_functions(classified):
    """moment_fields, estimate_population, suggest_q, format_slots and format_slots_csv on emulator records and crafted ones"""
    from rfid import batch as rb
    t, rows = classified[4]
    l1, l2 = rb.moment_fields(rows)
    assert l1.dtype == np.float64 and (l1 >= l2).all() and (l2 >= 0).all()
    for k in (0, len(rows) - 1):
        e = ref.eig(rows[k])
        assert abs(l1[k] - e[0]) <= 1e-15 * e[0] and abs(l2[k] - e[1]) <= 1e-15 * e[0]
    # a noise-free trace has no floor: nothing is classified
    flat = np.zeros(6, dtype=rows.dtype)
    flat["seq"] = np.arange(6)
    none = rb.classify_slots(flat)
    assert len(none) == 3 and (none["cls"] == -1).all() and (none["answered"] == 0).all()
    assert "not classified" in rb.format_slots(none, 2)
    assert len(rb.classify_slots(rows[:1])) == 0 and len(rb.classify_slots(rows[:5])) == 2          # (a last RN16 without its EPC)
    assert rb.estimate_population(np.array([1, 1, 2, 0, 2, -1]), 2) == (2 + 2.39 * 2) / 2 and rb.estimate_population([], 0) == 0.0
    assert [rb.suggest_q(n) for n in (0, 1, 1.4, 1.5, 3, 5.6, 5.7, 100, 1e9)] == [0, 0, 0, 1, 2, 2, 3, 7, 15]
    slots = rb.classify_slots(rows)
    line = rb.format_slots(slots, 2)
    cls = slots["cls"]
    assert line.startswith("| slots : 16  empty : %d  single : %d  collided : %d  answered : %d  read : %d  efficiency : %.3f  " %
                           ((cls == 0).sum(), (cls == 1).sum(), (cls == 2).sum(), slots["answered"].sum(), slots["crc_ok"].sum(),
                            slots["crc_ok"].sum() / 16.0))
    assert line.endswith("suggested Q : 2 (in use : 2)\n") and line.count("\n") == 1 and "tags per round : 4.14" in line
    starts = 1000 + 400 * np.arange(len(rows))
    text = rb.format_slots_csv([slots, none], [starts, np.arange(6)], ["a.bin", "b.bin"])
    lines = text.splitlines()
    assert lines[0] == rb.SLOTS_HEADER == "file,slot,seq,t_s,class,l1_db,l2_db,floor_db,answered,crc_ok" and len(lines) == 1 + 16 + 3
    names = {0: "empty", 1: "single", 2: "collided"}
    for k, line in enumerate(lines[1:17]):
        f = line.split(",")
        s = slots[k]
        assert f[:3] == ["a.bin", str(k), str(2 * k)] and f[3] == "%.9g" % (starts[2 * k] / 400e3) and f[4] == names[int(s["cls"])]
        assert [float(v) for v in f[5:8]] == [float("%.9g" % (10 * np.log10(s[n]))) for n in ("l1", "l2", "floor")]
        assert f[8:] == [str(int(s["answered"])), str(int(s["crc_ok"]))]
    assert lines[17].startswith("b.bin,0,0,0,unknown,-inf,-inf,-inf,0,0")

"""The cases of the repair stage that run on both sides, written once: tests/test_repair_emu.py (the kernels on the wave emulator) and
tests/test_gpu_repair.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches the
library).  Pytest collects the imported functions in the importing module, resolves their fixtures there and applies that module's
marks.  Every expected record is worked out from the ORACLE alone (tests/repair_ref.py: the definition of include/rfid_mi355x.h run
literally, the oracle's check_crc for the CRC), never from the library's own windows or results, and every comparison is exact.  Each
case asserts from the reference that its input has the properties it is there for before a kernel sees it; the inputs and the checks
are in tests/repair_cases.py."""
import ctypes as C

import numpy as np
import pytest

import repair_ref as ref
import repair_cases as cases
import repair_windows as rw
import tracks_ref as tref
from stage_backend import oracle_pass

__all__ = ["single", "batch", "test_edge_trace_fourteen_of_fifteen_failed_frames_come_back",
           "test_lost_tag_is_repaired_without_an_inventory_entry", "test_mixed_slots_known_and_unknown_repairs",
           "test_repairs_of_a_ragged_batch_equal_the_oracles", "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero",
           "test_no_false_comfort_a_frame_sent_wrong_stays_unrepaired", "test_crafted_windows_through_repair_window",
           "test_protocol_capacity_and_state_errors"]


@pytest.fixture(scope="module")
def single(backend, oracle_mod, synth_mod):
    """name -> (host, lens, L, stride, fixed_q, oracle result, (packed, [rows]), y, handle) of the three traces, each on its own"""
    return {name: t + (backend.put(t[0], t[1]),) for name, t in cases.single_traces(oracle_mod, synth_mod).items()}


@pytest.fixture(scope="module")
def batch(backend, oracle_mod, synth_mod):
    data = cases.ragged_batch(oracle_mod, synth_mod)
    return data + (backend.put(data[0], data[1]),)


def _one_trace(backend, single, name):
    import rfid
    host, lens, L, stride, q, o, want, y, dev = single[name]
    ctx = rfid.Context(device=0, fixed_q=q)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 1, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, want, name)
        assert ctx.batch_repair_ms() >= 0.0
    finally:
        ctx.close()


def test_edge_trace_fourteen_of_fifteen_failed_frames_come_back(backend, single):
    """A = 0.016: 24 EPC windows, 9 verified, 15 failed; 14 repaired with 9 / 4 / 1 of them by 1 / 2 / 3 flips, all 14 the frame the
    inventory holds; seq 15 is out of reach.  (The test that cannot pass without the stage: its signatures do not exist.)"""
    packed, (rows,) = single["edge"][6]
    assert cases.summary(rows) == (24, 9, 15, [9, 4, 1])
    assert len(packed) == 14 and (packed["entry"] == 0).all() and (packed["flags"] == 0).all()
    assert ref.flip_list(rows[27 >> 1]) == [26, 99, 124] and rows[15 >> 1]["n_flips"] == 0 and not rows[15 >> 1]["flags"] & 1
    _one_trace(backend, single, "edge")


def test_lost_tag_is_repaired_without_an_inventory_entry(backend, single):
    """A = 0.014, three rounds: no window verifies, all three are repaired; the inventory is empty, so entry == -1 everywhere"""
    packed, (rows,) = single["lost"][6]
    assert cases.summary(rows) == (3, 0, 3, [2, 1, 0]) and single["lost"][5].state.n_epc_correct == 0
    assert [ref.flip_list(r) for r in packed] == [[54, 82], [119], [125]] and (packed["entry"] == -1).all()
    _one_trace(backend, single, "lost")


def test_mixed_slots_known_and_unknown_repairs(backend, single):
    """FIXED_Q = 2, two tags with one EPC and a third: 32 EPC windows, 6 verified, 26 failed of which 19 are empty or collided slots;
    six repairs, three of a tag of the inventory and three of none; the other twenty stay unrepaired"""
    packed, (rows,) = single["mixed"][6]
    assert cases.summary(rows) == (32, 6, 26, [4, 2, 0])
    assert packed["seq"].tolist() == [1, 13, 15, 25, 37, 43]
    assert (packed["entry"] >= 0).tolist() == [True, True, False, True, False, False]
    assert ((rows["flags"] & 1) == 0).sum() - len(packed) == 20
    _one_trace(backend, single, "mixed")


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_repairs_of_a_ragged_batch_equal_the_oracles(backend, batch, mode):
    """Four traces, both front ends; the pass backend.reps times: the same bytes every time, packed list and table rows alike, and
    the five rows of the table behind a trace's windows zero"""
    import rfid
    host, lens, L, stride, refs, ys, want, dev = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(mode)
        cases.plan(ctx, 4, L)
        blobs = []
        for rep in range(backend.reps):
            backend.run_pass(ctx, dev, L, stride)
            blobs.append(cases.check(ctx, want, (mode, rep), extra=5))
        assert all(b == blobs[0] for b in blobs)
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, batch):
    """MAX_NUM_QUERIES = 20 is reached inside the two long traces (gate_impl.cc:101-109): a full pass fills the table's rows, the
    cut-off pass behind it in a context of its own settings reports the windows before the cut-off only and zeroes the rest"""
    import rfid
    host, lens, L, stride, full_refs, full_ys, full_want, dev = batch
    refs, ys = oracle_pass(oracle_mod, host, lens, 2, max_num_queries=20)
    want = ref.expected_batch(oracle_mod, refs, ys)
    n_rows = [len(r) for r in want[1]]
    assert refs[0].state.status == 1 and refs[1].state.status == 1 and n_rows[0] < 32 and n_rows[1] < 24 and n_rows[3] == 3, n_rows
    assert 0 < len(want[0]) < len(full_want[0])
    cut_seq = {(int(r["stream"]), int(r["seq"])) for r in full_want[0]} - {(int(r["stream"]), int(r["seq"])) for r in want[0]}
    assert cut_seq and all(seq >= 2 * n_rows[s] for s, seq in cut_seq)          # (repairs of the full pass that lie behind the cut-off)
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=20)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 4, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, want, "cut")
        for b in range(4):
            n = C.c_int64(-1)
            rc = ctx._lib.rfid_batch_get_window_repairs(ctx._h, b, None, 0, C.byref(n))
            assert n.value == n_rows[b] and rc == (rfid.capi.ERR_CAPACITY if n_rows[b] else rfid.capi.OK)
            many = ctx.batch_window_repairs(b, extra=10_000)          # (more than the table has: the whole row of the trace)
            assert not many[n_rows[b]:].tobytes().strip(b"\0")
    finally:
        ctx.close()
    # and in ONE context: a long pass fills the rows, a pass over shortened traces behind it must zero them again
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 4, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, full_want, "full")
        cut = lens.copy()
        for b in (0, 1):
            cut[b] = 5 * int(full_refs[b].open_idx[13] + 1370 + 40)              # (the trace ends behind its fourteenth window)
        short = ref.expected_batch(oracle_mod, *oracle_pass(oracle_mod, host, cut, 2))
        assert [len(r) for r in short[1]] == [7, 7, 0, 3]
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        cases.check(ctx, short, "short")
        for b in (0, 1):
            r = ctx.batch_window_repairs(b, extra=len(full_want[1][b]))
            assert not r[7:].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_no_false_comfort_a_frame_sent_wrong_stays_unrepaired(backend, oracle_mod, synth_mod):
    """One bit of round 3's EPC frame was flipped by the TAG: a frame error, not a decision error -- a single frame bit is not what
    reversing a decision toggles.  By the reference the window stays unrepaired, and the stage says the same"""
    import rfid
    host, lens, L, stride, want = cases.frame_sent_wrong(oracle_mod, synth_mod)
    dev = backend.put(host, lens)
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        cases.plan(ctx, 1, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, want)
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_repairs(ctx._h, None, 0, C.byref(n)) == rfid.capi.OK and n.value == 0
    finally:
        ctx.close()


def test_crafted_windows_through_repair_window(oracle_mod):
    """rfid_repair_window on noise-free windows with decisions of exactly 0 (ten of them: the tie rule "smaller j first" admits the two
    wrong ones, the opposite rule would not), a lone wrong decision 127 (one frame bit), two sets of equal cost that both pass (the
    smaller mask wins), four wrong decisions (out of reach), wrong decisions behind weaker right ones, and a frame that verifies"""
    import rfid
    sets = rw.build(oracle_mod)
    rw.check(oracle_mod, sets)
    assert "equal" in sets
    ctx = rfid.Context(device=0)
    try:
        for name, (w, d, want, r, wrong) in sets.items():
            got = ctx.repair_window(w, ref.result_of_dump(d))
            ref.assert_equal(got, want, name)
        rn16 = ref.result_of_dump(sets["last"][1])
        rn16["type"] = 0
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.repair_window(sets["last"][0], rn16)
        assert e.value.status == rfid.capi.ERR_INVALID
        with pytest.raises(ValueError):
            ctx.repair_window(sets["last"][0][:250], ref.result_of_dump(sets["last"][1]))
    finally:
        ctx.close()


def test_protocol_capacity_and_state_errors(backend, oracle_mod, single):
    import rfid
    host, lens, L, stride, q, o, want, y, dev = single["mixed"]
    ctx = rfid.Context(device=0, fixed_q=q)
    ERR_STATE, ERR_CAPACITY = rfid.capi.ERR_STATE, rfid.capi.ERR_CAPACITY

    def raises(fn, status):
        with pytest.raises(rfid.capi.RfidError) as e:
            fn()
        assert e.value.status == status, e.value

    try:
        raises(ctx.batch_plan_repair, ERR_STATE)                  # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(1, L)
        raises(ctx.batch_plan_repair, ERR_STATE)                  # no inventory workspace
        ctx.batch_plan_inventory(8)
        raises(ctx.batch_repair_enqueue, ERR_STATE)               # no repair workspace
        ctx.batch_plan_repair()
        raises(ctx.batch_repair_enqueue, ERR_STATE)               # no pass
        raises(ctx.batch_repair_fetch, ERR_STATE)                 # nothing enqueued
        raises(lambda: ctx.batch_window_repairs(0), ERR_STATE)
        raises(ctx.batch_repair_ms, ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        raises(ctx.batch_repair_enqueue, ERR_STATE)               # a pass, but not its inventory
        cases.check(ctx, want, "first pass")
        # a side branch: the tracks and the quality of the same pass behind it are what they are without it, and the other way round
        ctx.batch_plan_tracks()
        ctx.batch_plan_quality()                                  # (neither plan drops the repair workspace)
        ent, counts, reads, off = tref.expected_batch([o])
        got_reads, got_off = ctx.batch_tracks()
        tref.assert_equal(got_reads, got_off, reads, off)
        ctx.batch_quality()
        ref.assert_equal(ctx.batch_repair(), want[0], "behind the tracks and the quality")
        # a second pass whose inventory was not enqueued: the repairs of the first can still be fetched, a new run would mix passes
        backend.run_pass(ctx, dev, L, stride)
        raises(ctx.batch_repair_enqueue, ERR_STATE)
        ref.assert_equal(ctx.batch_repair_fetch(), want[0])
        cases.check(ctx, want, "second pass")
        # a caller's array that is too small loses nothing
        small = np.zeros(len(want[0]) - 1, dtype=rfid.capi.REPAIR_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_repairs(ctx._h, small.ctypes.data, len(small), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not small.tobytes().strip(b"\0")
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_repairs(ctx._h, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(want[0])
        full = np.zeros(n.value, dtype=rfid.capi.REPAIR_DTYPE)
        assert ctx._lib.rfid_batch_get_repairs(ctx._h, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        row = np.zeros(len(want[1][0]) - 1, dtype=rfid.capi.REPAIR_DTYPE)
        rc = ctx._lib.rfid_batch_get_window_repairs(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[1][0]) and not row.tobytes().strip(b"\0")
        assert ctx._lib.rfid_batch_get_window_repairs(ctx._h, 1, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_repairs(ctx._h, -1, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID
        # an inventory that overflowed (two distinct frames, room for one) is no error here: flag bit 1, no entry
        ctx.set_knob("inventory_slots", 2)
        ctx.batch_plan_inventory(1)
        raises(ctx.batch_repair_enqueue, ERR_STATE)               # (a new inventory workspace dropped the repair workspace)
        raises(ctx.batch_repair_fetch, ERR_STATE)
        ctx.batch_plan_repair()
        ctx.batch_inventory_enqueue()
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory_fetch()
        assert e.value.status == ERR_CAPACITY and "trace 0" in str(e.value)
        over = ref.expected_batch(oracle_mod, [o], [y], overflow={0})
        assert (over[0]["flags"] == 2).all() and (over[0]["entry"] == -1).all() and len(over[0]) == len(want[0])
        got = ctx.batch_repair()
        ref.assert_equal(got, over[0], "overflow")
        ref.assert_equal(ctx.batch_window_repairs(0), over[1][0], "overflow, row")
        ctx.set_knob("inventory_slots", 0)
        # a new plan drops everything
        ctx.batch_plan(1, L)
        raises(ctx.batch_repair_enqueue, ERR_STATE)
        raises(ctx.batch_plan_repair, ERR_STATE)
        cases.plan(ctx, 1, L)
        backend.run_pass(ctx, dev, L, stride)
        cases.check(ctx, want, "new plan")
    finally:
        ctx.close()

"""The repair stage (rfid_batch_plan_repair / rfid_batch_repair / rfid_batch_get_repairs / rfid_batch_get_window_repairs and the
per-call rfid_repair_window: CRC-failed EPC frames recovered from their weakest decisions, built on the device behind the inventory) on
the CPU: csrc/rfid_capi.hip and csrc/rfid_repair.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave
emulator.  Every expected record is worked out from the ORACLE alone (tests/repair_ref.py: the definition of include/rfid_mi355x.h run
literally, the oracle's check_crc for the CRC), never from the library's own windows or results, and every comparison is exact: by bit
pattern, then by the bytes of the whole arrays.  Each test asserts from the reference that its input has the properties it is there
for before a kernel sees it.

The traces are at the sensitivity edge: sigma = 0.02, T1 jitter of 3 raw samples, tag amplitude A = 0.014 .. 0.018."""
import ctypes as C

import numpy as np
import pytest

import repair_ref as ref
import repair_windows as rw
import tracks_ref as tref
import emu_lib
from emu_lib import run_pass as _pass
from stage_backend import lay_out

TRACES = dict(      # name -> (A, make_trace arguments)
    edge=(0.016, dict(fixed_q=0, tag_ids=(0x27,), seed=1, n_rounds=24)),
    lost=(0.014, dict(fixed_q=0, tag_ids=(0x27,), seed=15, n_rounds=3)),
    mixed=(0.018, dict(fixed_q=2, tag_ids=(0x27, 0x27, 0x31), seed=2, n_rounds=8)),
)


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


def make(synth_mod, name):
    A, kw = TRACES[name]
    return synth_mod.make_trace(sigma=0.02, t1_jitter_raw=3, h=A * np.exp(2.1j), **kw).samples


def _oracle(oracle_mod, host, lens, fixed_q, **cfg):
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=fixed_q, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ys


@pytest.fixture(scope="module")
def single(oracle_mod, synth_mod):
    """name -> (host, lens, L, stride, fixed_q, oracle result, (packed, [rows]), y) of the three traces, each on its own"""
    out = {}
    for name, (A, kw) in TRACES.items():
        host, lens, L, stride = lay_out([make(synth_mod, name)])
        refs, ys = _oracle(oracle_mod, host, lens, kw["fixed_q"])
        out[name] = (host, lens, L, stride, kw["fixed_q"], refs[0], ref.expected_batch(oracle_mod, refs, ys), ys[0])
    return out


def _plan(ctx, n, L, max_tags=8):
    ctx.batch_plan(n, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_repair()


def _check(ctx, want, what=""):
    """inventory + repair of the last pass; the packed records and every trace's row against the oracle's"""
    w_packed, w_rows = want
    ctx.batch_inventory_enqueue()
    got = ctx.batch_repair()
    ref.assert_equal(got, w_packed, what)
    st = ctx.batch_stats()
    blob = got.tobytes()
    for b, w in enumerate(w_rows):
        r = ctx.batch_window_repairs(b)
        assert len(r) == int(st[b]["n_windows_used"]) // 2
        ref.assert_equal(r, w, (what, "row", b))
        blob += r.tobytes()
    return blob


def _one_trace(single, name):
    import rfid
    host, lens, L, stride, q, o, want, y = single[name]
    ctx = rfid.Context(device=0, fixed_q=q)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 1, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want, name)
        assert ctx.batch_repair_ms() >= 0.0
    finally:
        ctx.close()


def _summary(rows):
    ok = (rows["flags"] & 1) == 1
    return len(rows), int(ok.sum()), int((~ok).sum()), np.bincount(rows["n_flips"], minlength=4)[1:].tolist()


def test_edge_trace_fourteen_of_fifteen_failed_frames_come_back(single):
    """A = 0.016: 24 EPC windows, 9 verified, 15 failed; 14 repaired with 9 / 4 / 1 of them by 1 / 2 / 3 flips, all 14 the frame the
    inventory holds; seq 15 is out of reach.  (The test that cannot pass without the stage: its signatures do not exist.)"""
    packed, (rows,) = single["edge"][6]
    assert _summary(rows) == (24, 9, 15, [9, 4, 1])
    assert len(packed) == 14 and (packed["entry"] == 0).all() and (packed["flags"] == 0).all()
    assert ref.flip_list(rows[27 >> 1]) == [26, 99, 124] and rows[15 >> 1]["n_flips"] == 0 and not rows[15 >> 1]["flags"] & 1
    _one_trace(single, "edge")


def test_lost_tag_is_repaired_without_an_inventory_entry(single):
    """A = 0.014, three rounds: no window verifies, all three are repaired; the inventory is empty, so entry == -1 everywhere"""
    packed, (rows,) = single["lost"][6]
    assert _summary(rows) == (3, 0, 3, [2, 1, 0]) and single["lost"][5].state.n_epc_correct == 0
    assert [ref.flip_list(r) for r in packed] == [[54, 82], [119], [125]] and (packed["entry"] == -1).all()
    _one_trace(single, "lost")


def test_mixed_slots_known_and_unknown_repairs(single):
    """FIXED_Q = 2, two tags with one EPC and a third: 32 EPC windows, 6 verified, 26 failed of which 19 are empty or collided slots;
    six repairs, three of a tag of the inventory and three of none; the other twenty stay unrepaired"""
    packed, (rows,) = single["mixed"][6]
    assert _summary(rows) == (32, 6, 26, [4, 2, 0])
    assert packed["seq"].tolist() == [1, 13, 15, 25, 37, 43]
    assert (packed["entry"] >= 0).tolist() == [True, True, False, True, False, False]
    assert ((rows["flags"] & 1) == 0).sum() - len(packed) == 20
    _one_trace(single, "mixed")


@pytest.fixture(scope="module")
def batch(oracle_mod, synth_mod):
    """the three traces and a pure-carrier trace in the middle as one ragged batch, FIXED_Q = 2 for all of them"""
    ts = [make(synth_mod, "mixed"), make(synth_mod, "edge"), None, make(synth_mod, "lost")]
    ts[2] = np.full(len(ts[0]) // 2, np.complex64(0.8 + 0.1j))
    host, lens, L, stride = lay_out(ts)
    refs, ys = _oracle(oracle_mod, host, lens, 2)
    want = ref.expected_batch(oracle_mod, refs, ys)
    assert [len(r) for r in want[1]] == [32, 24, 0, 3] and [int((r["n_flips"] > 0).sum()) for r in want[1]] == [6, 14, 0, 3]
    assert np.array_equal(want[0]["stream"], np.repeat([0, 1, 3], [6, 14, 3])) and (np.diff(want[0]["seq"])[np.diff(want[0]["stream"]) == 0] > 0).all()
    return host, lens, L, stride, refs, ys, want


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_repairs_of_a_ragged_batch_equal_the_oracles(batch, mode):
    """Four traces, both front ends; the pass twice: the same bytes both times, packed list and table rows alike"""
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
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        for b in range(4):      # the rows of the table behind a trace's windows are zero
            r = ctx.batch_window_repairs(b, extra=5)
            assert len(r) == len(want[1][b]) + 5 and not r[len(want[1][b]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(oracle_mod, batch):
    """MAX_NUM_QUERIES = 20 is reached inside the two long traces (gate_impl.cc:101-109): a full pass fills the table's rows, the
    cut-off pass behind it in a context of its own settings reports the windows before the cut-off only and zeroes the rest"""
    import rfid
    host, lens, L, stride, full_refs, full_ys, full_want = batch
    refs, ys = _oracle(oracle_mod, host, lens, 2, max_num_queries=20)
    want = ref.expected_batch(oracle_mod, refs, ys)
    n_rows = [len(r) for r in want[1]]
    assert refs[0].state.status == 1 and refs[1].state.status == 1 and n_rows[0] < 32 and n_rows[1] < 24 and n_rows[3] == 3, n_rows
    assert 0 < len(want[0]) < len(full_want[0])
    cut_seq = {(int(r["stream"]), int(r["seq"])) for r in full_want[0]} - {(int(r["stream"]), int(r["seq"])) for r in want[0]}
    assert cut_seq and all(seq >= 2 * n_rows[s] for s, seq in cut_seq)          # (repairs of the full pass that lie behind the cut-off)
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=20)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 4, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want, "cut")
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
        _plan(ctx, 4, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, full_want, "full")
        cut = lens.copy()
        for b in (0, 1):
            cut[b] = 5 * int(full_refs[b].open_idx[13] + 1370 + 40)              # (the trace ends behind its fourteenth window)
        short_refs, short_ys = _oracle(oracle_mod, host, cut, 2)
        short = ref.expected_batch(oracle_mod, short_refs, short_ys)
        assert [len(r) for r in short[1]] == [7, 7, 0, 3]
        ctx.batch_process_ptr(host.ctypes.data, stride, L, cut.ctypes.data)
        _check(ctx, short, "short")
        for b in (0, 1):
            r = ctx.batch_window_repairs(b, extra=len(full_want[1][b]))
            assert not r[7:].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_no_false_comfort_a_frame_sent_wrong_stays_unrepaired(oracle_mod, synth_mod):
    """One bit of round 3's EPC frame was flipped by the TAG: a frame error, not a decision error -- a single frame bit is not what
    reversing a decision toggles.  By the reference the window stays unrepaired, and the stage says the same"""
    import rfid
    x = synth_mod.make_trace(n_rounds=5, fixed_q=0, tag_ids=(0x27,), seed=7, sigma=0.02, corrupt_rounds=(3,)).samples
    host, lens, L, stride = lay_out([x])
    refs, ys = _oracle(oracle_mod, host, lens, 0)
    want = ref.expected_batch(oracle_mod, refs, ys)
    rows = want[1][0]
    assert (rows["flags"] & 1).tolist() == [1, 1, 0, 1, 1] and not rows["n_flips"].any() and len(want[0]) == 0
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        _plan(ctx, 1, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want)
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


def test_protocol_capacity_and_state_errors(oracle_mod, single):
    import rfid
    host, lens, L, stride, q, o, want, y = single["mixed"]
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
        _pass(ctx, host, lens, L, stride)
        raises(ctx.batch_repair_enqueue, ERR_STATE)               # a pass, but not its inventory
        _check(ctx, want, "first pass")
        # a side branch: the tracks and the quality of the same pass behind it are what they are without it, and the other way round
        ctx.batch_plan_tracks()
        ctx.batch_plan_quality()                                  # (neither plan drops the repair workspace)
        ent, counts, reads, off = tref.expected_batch([o])
        got_reads, got_off = ctx.batch_tracks()
        tref.assert_equal(got_reads, got_off, reads, off)
        ctx.batch_quality()
        ref.assert_equal(ctx.batch_repair(), want[0], "behind the tracks and the quality")
        # a second pass whose inventory was not enqueued: the repairs of the first can still be fetched, a new run would mix passes
        _pass(ctx, host, lens, L, stride)
        raises(ctx.batch_repair_enqueue, ERR_STATE)
        ref.assert_equal(ctx.batch_repair_fetch(), want[0])
        _check(ctx, want, "second pass")
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
        _plan(ctx, 1, L)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want, "new plan")
    finally:
        ctx.close()


def test_format_helpers_and_the_csv_columns(single):
    """rfid.batch.repair_flips / format_repair_summary / format_repairs (host side) on the reference-made records"""
    from rfid import batch as rb
    packed, (rows,) = single["mixed"][6]
    assert [rb.repair_flips(r) for r in packed] == [ref.flip_list(r) for r in packed]
    assert rb.format_repair_summary(rows) == "| failed EPC windows : 26  repaired : 6  of a tag in the inventory : 3\n"
    assert rb.format_repair_summary(rows[:0]) == "| failed EPC windows : 0  repaired : 0  of a tag in the inventory : 0\n"
    lines = rb.format_repairs(packed, ["a.bin"]).splitlines()
    assert lines[0] == rb.REPAIRS_HEADER == "file,epc,pc,seq,t_s,n_flips,flips,cost,known" and len(lines) == 1 + len(packed)
    for line, r in zip(lines[1:], packed):
        f = line.split(",")
        pc, epc = rb.frame_fields(r["frame"])
        assert f[0] == "a.bin" and f[1] == epc and f[2] == "%04x" % pc and int(f[3]) == r["seq"]
        assert f[4] == "%.9g" % (int(r["start"]) / rb.TRACKS_RATE) and int(f[5]) == r["n_flips"]
        assert [int(v) for v in f[6].split("+")] == ref.flip_list(r)
        assert np.float32(f[7]).tobytes() == r["cost"].tobytes() and f[8] == ("1" if r["entry"] >= 0 else "0")
    # the formats that were there are what they were: no new column, no new line
    assert rb.TRACKS_HEADER == "file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T" and rb.TRACKS_QUALITY_HEADER == rb.TRACKS_HEADER + ",snr_db,margin"

"""The tracks stage (rfid_batch_plan_tracks / rfid_batch_tracks / rfid_batch_get_tracks: every tag's reads in time order, built on
the device behind the inventory) on the CPU: csrc/rfid_capi.hip and csrc/rfid_tracks.hpp, unmodified, through tests/fake_hip's
library -- the kernels run on the wave emulator.  Every expected array is worked out in numpy from the ORACLE's per-window dumps and
window openings (tests/tracks_ref.py), never from the library's own windows or results, and every comparison is exact.

The traces are those of tests/test_inventory_emu.py: seeds 104 (4 rounds) and 112 (3 rounds), FIXED_Q = 2, tags (0x27, 0x27, 0x31),
sigma = 0.02.  By the oracle alone the three frames' reads fall at seq [3,15,21,27] [5,13,31] [7,11,29] (seed 104) and [1,15]
[3,13,21] [7,9] (seed 112): the tags interleave in time, so the grouped order differs from the window order, and one tag has four
reads (asserted below before anything is compared)."""
import ctypes as C

import numpy as np
import pytest

import inventory_ref as iref
import tracks_ref as ref
import emu_lib
from emu_lib import oracle_runs as _oracle, run_pass as _pass
from stage_backend import lay_out

TAGS = (0x27, 0x27, 0x31)
SEEDS = ((104, 4), (112, 3))       # (seed, inventory rounds) per trace
SEQS = ([[3, 15, 21, 27], [5, 13, 31], [7, 11, 29]], [[1, 15], [3, 13, 21], [7, 9]])
SEQS_CUT = ([3, 5, 7, 11, 13], [1, 3, 7, 9, 13])      # max_num_queries = 7: what is left, in window order


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


def _traces(synth_mod):
    return [synth_mod.make_trace(n_rounds=n, fixed_q=2, tag_ids=TAGS, seed=seed, sigma=0.02, t1_jitter_raw=3).samples for seed, n in SEEDS]


def _seqs_by_entry(reads, off):
    return [reads["seq"][off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def batch(oracle_mod, synth_mod):
    host, lens, L, stride = lay_out(_traces(synth_mod), shorten=777)
    refs = _oracle(oracle_mod, host, lens)
    ent, counts, reads, off = ref.expected_batch(refs)
    # the input does what the case is about, by the oracle alone: the tags interleave in time, one of them is read four times
    got = _seqs_by_entry(reads, off)
    assert got[:3] == SEQS[0] and got[3:] == SEQS[1], got
    for b in range(2):
        r = reads[reads["stream"] == b]
        assert (np.diff(r["seq"]) < 0).any()                  # (grouped order is not window order)
        assert (np.diff(np.sort(r["seq"])) > 0).all()
    assert len(reads) == sum(o.state.n_epc_correct for o in refs)
    return host, lens, L, stride, refs, (ent, counts, reads, off)


def _check(ctx, want, what=""):
    """inventory + tracks of the last pass against the oracle's, and against the pass's own outputs"""
    w_ent, w_counts, w_reads, w_off = want
    ent, counts = ctx.batch_inventory()
    reads, off = ctx.batch_tracks()
    iref.assert_equal(ent, counts, w_ent, w_counts, what)
    ref.assert_equal(reads, off, w_reads, w_off, what)
    ref.cross_check(reads, off, ent, counts, ctx.batch_stats())
    return reads, off


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_tracks_of_a_ragged_batch_equal_the_oracles(batch, mode):
    """Two traces, both front ends; the pass twice: the same bytes both times; then the same pass through tables of 4 slots (three
    frames in four slots: probes collide, the later rounds run) and of 2 slots (more frames than slots: the trace overflows)."""
    import rfid
    host, lens, L, stride, refs, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(mode)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        first = None
        for rep in range(2):
            _pass(ctx, host, lens, L, stride)
            reads, off = _check(ctx, want, (mode, rep))
            first = first if first is not None else (reads.tobytes(), off.tobytes())
            assert (reads.tobytes(), off.tobytes()) == first
        assert ctx.batch_tracks_ms() >= 0.0
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        # forced collisions: the workspaces are planned again, the pass stays
        ctx.set_knob("inventory_slots", 4)
        ctx.batch_plan_inventory(4)
        ctx.batch_plan_tracks()
        reads, off = _check(ctx, want, "4 slots")
        assert (reads.tobytes(), off.tobytes()) == first
        ctx.batch_plan_inventory(3)
        ctx.batch_plan_tracks()
        _check(ctx, want, "4 slots, max_tags 3")
        ctx.set_knob("inventory_slots", 0)
        ctx.batch_plan_inventory(100)                   # (more than 64 tags per trace: the instantiation with the 1 024-slot table)
        ctx.batch_plan_tracks()
        reads, off = _check(ctx, want, "max_tags 100")
        assert (reads.tobytes(), off.tobytes()) == first
        ctx.set_knob("inventory_slots", 2)
        ctx.batch_plan_inventory(4)
        ctx.batch_plan_tracks()
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_tracks_fetch()
        assert e.value.status == rfid.capi.ERR_CAPACITY and "trace 0" in str(e.value)
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_tracks(ctx._h, None, 0, C.byref(n), None) == rfid.capi.ERR_CAPACITY and n.value == 0
    finally:
        ctx.close()


def test_reads_behind_the_cut_off_are_absent(oracle_mod, batch):
    """MAX_NUM_QUERIES = 7 reached inside the traces (gate_impl.cc:101-109): the oracle stops after 14 windows in both and keeps five
    reads of each trace; the tags still interleave"""
    import rfid
    host, lens, L, stride, full_refs, full_want = batch
    refs = _oracle(oracle_mod, host, lens, max_num_queries=7)
    want = ref.expected_batch(refs)
    ent, counts, reads, off = want
    assert all(o.state.status == 1 and o.n_windows == 14 for o in refs)
    for b in range(2):
        r = reads[reads["stream"] == b]
        assert sorted(r["seq"].tolist()) == SEQS_CUT[b] and (np.diff(r["seq"]) < 0).any(), (b, r["seq"])
    assert len(reads) < len(full_want[2])
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=7)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want)
        assert [int(s["n_windows_used"]) for s in ctx.batch_stats()] == [14, 14]
    finally:
        ctx.close()


def test_only_one_trace_of_the_plan(batch):
    """rfid_batch_set_streams(1) on a two-trace plan: the tracks cover the row the pass covered"""
    import rfid
    host, lens, L, stride, refs, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        ctx.batch_set_streams(1)
        _pass(ctx, host, lens, L, stride)
        _check(ctx, ref.expected_batch(refs[:1]))
    finally:
        ctx.close()


def test_a_trace_without_a_verified_read_has_an_empty_range(oracle_mod, synth_mod):
    """three traces, the middle one pure carrier: no window, no entry, no read -- the third trace's reads follow the first's"""
    import rfid
    ts = _traces(synth_mod)
    ts.insert(1, np.full(len(ts[0]) // 2, 0.8 + 0.1j, dtype=np.complex64))
    host, lens, L, stride = lay_out(ts, shorten=777)
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2)) for b in range(3)]
    want = ref.expected_batch(refs)
    ent, counts, reads, off = want
    assert counts.tolist() == [3, 0, 3] and not (reads["stream"] == 1).any() and (reads["stream"] == 2).sum() == 7
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want)
        # a batch that holds nothing but carrier: no reads at all, one offset
        ctx.batch_set_streams(1)
        only = np.ascontiguousarray(host[1:2])
        _pass(ctx, only, lens[1:2].copy(), L, stride)
        ent, counts = ctx.batch_inventory()
        reads, off = ctx.batch_tracks()
        assert len(ent) == 0 and len(reads) == 0 and off.tolist() == [0]
    finally:
        ctx.close()


def test_sixteen_waves_share_a_trace(oracle_mod, synth_mod):
    """A plan for a trace long enough to hold more than 2 048 windows takes the sixteen-wave kernels; the trace decoded under it
    has 20 rounds (160 windows): every wave owns 64 of them, three waves hold reads of every tag -- the counts per (tag, wave) and
    their prefix decide every place."""
    import rfid
    x = synth_mod.make_trace(n_rounds=20, fixed_q=2, tag_ids=TAGS, seed=131, sigma=0.02, t1_jitter_raw=3).samples
    host, lens, L, stride = lay_out([x])
    refs = _oracle(oracle_mod, host, lens)
    want = ref.expected_batch(refs)
    ent, counts, reads, off = want
    assert refs[0].n_windows > 128 and len(ent) == 3
    for i in range(3):                                     # every tag is read in the first 64 windows, the next 64 and behind them
        s = reads["seq"][off[i]:off[i + 1]]
        assert (s < 64).any() and ((s >= 64) & (s < 128)).any() and (s >= 128).any(), (i, s)
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(1, 3_600_000)                       # (room for 2 070 windows)
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        _pass(ctx, host, lens, L, stride)
        first = _check(ctx, want)
        ctx.set_knob("inventory_slots", 4)
        ctx.batch_plan_inventory(4)
        ctx.batch_plan_tracks()
        again = _check(ctx, want, "4 slots")
        assert first[0].tobytes() == again[0].tobytes()
        # room for more than 64 tags per trace: the instantiation with the 1 024-slot table and 512 x 16 counters
        ctx.set_knob("inventory_slots", 0)
        ctx.batch_plan_inventory(100)
        ctx.batch_plan_tracks()
        again = _check(ctx, want, "max_tags 100")
        assert first[0].tobytes() == again[0].tobytes()
    finally:
        ctx.close()


def test_protocol_capacity_and_state_errors(batch):
    import rfid
    host, lens, L, stride, refs, want = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    ERR_STATE, ERR_CAPACITY = rfid.capi.ERR_STATE, rfid.capi.ERR_CAPACITY

    def raises(fn, status):
        with pytest.raises(rfid.capi.RfidError) as e:
            fn()
        assert e.value.status == status, e.value

    try:
        raises(ctx.batch_plan_tracks, ERR_STATE)                 # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_plan_tracks, ERR_STATE)                 # no inventory workspace
        ctx.batch_plan_inventory(8)
        raises(ctx.batch_tracks_enqueue, ERR_STATE)              # no tracks workspace
        ctx.batch_plan_tracks()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)              # no pass
        raises(ctx.batch_tracks_fetch, ERR_STATE)                # nothing enqueued
        raises(ctx.batch_tracks_ms, ERR_STATE)
        _pass(ctx, host, lens, L, stride)
        raises(ctx.batch_tracks_enqueue, ERR_STATE)              # a pass, but not its inventory
        _check(ctx, want, "first pass")
        # a second pass whose inventory was not enqueued: the inventory of the first one is still there, the tracks would mix passes
        _pass(ctx, host, lens, L, stride)
        raises(ctx.batch_tracks_enqueue, ERR_STATE)
        ent, counts = ctx.batch_inventory_fetch()                # (what the inventory calls return has not changed)
        iref.assert_equal(ent, counts, want[0], want[1])
        ctx.batch_stage("stats")
        raises(ctx.batch_tracks_enqueue, ERR_STATE)
        _check(ctx, want, "second pass")
        # a caller's array that is too small loses nothing
        w_reads, w_off = want[2], want[3]
        small = np.zeros(len(w_reads) - 1, dtype=rfid.capi.TAG_READ_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_tracks(ctx._h, small.ctypes.data, len(small), C.byref(n), None)
        assert rc == ERR_CAPACITY and n.value == len(w_reads) and not small.tobytes().strip(b"\0")
        full = np.zeros(n.value, dtype=rfid.capi.TAG_READ_DTYPE)
        off = np.full(len(want[0]) + 1, -1, dtype=np.int64)
        assert ctx._lib.rfid_batch_get_tracks(ctx._h, full.ctypes.data, len(full), C.byref(n), off.ctypes.data) == rfid.capi.OK
        ref.assert_equal(full, off, w_reads, w_off)
        full[:] = 0
        assert ctx._lib.rfid_batch_get_tracks(ctx._h, full.ctypes.data, len(full), C.byref(n), None) == rfid.capi.OK    # offsets nullable
        assert full.tobytes() == w_reads.tobytes()
        # a new rfid_batch_plan_inventory drops the workspace, and so does a new plan
        ctx.batch_plan_inventory(8)
        raises(ctx.batch_tracks_enqueue, ERR_STATE)
        raises(ctx.batch_tracks_fetch, ERR_STATE)
        ctx.batch_plan_tracks()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)              # (the new inventory workspace holds no inventory yet)
        _check(ctx, want, "planned again")
        ctx.batch_plan(2, L)
        raises(ctx.batch_tracks_enqueue, ERR_STATE)
        raises(ctx.batch_plan_tracks, ERR_STATE)
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        _pass(ctx, host, lens, L, stride)
        _check(ctx, want, "new plan")
    finally:
        ctx.close()


def test_format_tracks_round_trips_binary32(batch):
    """rfid.batch.format_tracks (host side) on the oracle-derived arrays: one line per read, floats parse back to the same patterns"""
    from rfid import batch as rb
    ent, counts, reads, off = batch[5]
    names = ["a.bin", "b.bin"]
    lines = rb.format_tracks(ent, reads, off, names).splitlines()
    assert lines[0] == "file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T" and len(lines) == 1 + len(reads)
    owner = np.repeat(np.arange(len(ent)), np.diff(off))
    for line, r, i in zip(lines[1:], reads, owner):
        f = line.split(",")
        pc, epc = rb.frame_fields(ent[i]["frame"])
        assert f[0] == names[r["stream"]] and f[1] == epc and f[2] == "%04x" % pc and int(f[3]) == r["seq"]
        assert float(f[4]) == r["start"] / 400e3
        got = np.array([float(f[5]), float(f[6]), float(f[9])]).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), np.array([r["h_re"], r["h_im"], r["T"]], dtype=np.float32).view(np.uint32))
        h = complex(float(r["h_re"]), float(r["h_im"]))
        assert abs(float(f[7]) - 20 * np.log10(abs(h))) < 1e-6 and abs(float(f[8]) - np.angle(h)) < 1e-6

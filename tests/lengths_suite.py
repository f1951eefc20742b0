"""The cases of the lengths stage that run on both sides, written once: tests/test_lengths_emu.py (the kernels on the wave emulator) and
tests/test_gpu_lengths.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches the
library) and `call_ctx` (the context of the per-call cases).  Pytest collects the imported functions in the importing module, resolves
their fixtures there and applies that module's marks.  Every expected record is worked out in numpy from the ORACLE alone
(tests/lengths_ref.py) and every comparison is exact.

The ragged batch: four traces of 6, 5, 4 and 3 rounds, FIXED_Q = 2, three tags, sigma = 0.03, t1_jitter_raw = 3, odd row stride, the tags'
EPCs of (128, 64, 96), (112, 0, 32), (96, 96, 96) and (128, 128, 80) bits: 24 / 20 / 16 / 12 EPC rows -- block tails and more than one
block; the third group of lanes holds 32, 16 and 0 lanes, and some frames end inside the first group.  What is asserted of it before
anything runs (on the reference alone): every trace but the third holds at least 3 recovered windows, the batch at least 3 rows each
with flags bit 3 and bit 4, and the traces with a 96-bit tag -- the first and the third -- at least 3 reads."""
import ctypes as C

import numpy as np
import pytest

import repair_ref
import lengths_ref as ref
from stage_backend import lay_out

__all__ = ["ragged", "ragged_rows", "small", "test_abi_version_is_7", "test_ragged_batch_equals_the_reference_in_both_front_end_modes",
           "test_truth_every_lost_single_reply_of_another_length_is_recovered_and_no_empty_or_collided_slot_is",
           "test_trace_end_is_never_read_past", "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero",
           "test_plan_larger_than_the_batch_a_new_plan_and_a_small_grid", "test_overlap_each_pass_gets_its_own_records",
           "test_other_stages_results_and_statistics_are_untouched", "test_protocol_capacity_and_state_errors",
           "test_length_window_over_all_sync_offsets", "test_length_window_at_every_length", "test_length_window_on_crafted_spans",
           "test_length_window_refuses"]

SIGMA = 0.03
EPC_BITS = ((128, 64, 96), (112, 0, 32), (96, 96, 96), (128, 128, 80))
ROUNDS = (6, 5, 4, 3)
SEED = 101                                   # trace b: seed 101 + b (chosen so that lengths_ref alone meets the conditions and the truth case)
H = np.complex64(0.1 * np.exp(2.1j))         # the crafted spans' channel


def trace_of(synth_mod, b, **kw):
    return synth_mod.make_trace(n_rounds=ROUNDS[b], fixed_q=2, tag_ids=(1, 2, 3), seed=SEED + b, sigma=SIGMA, t1_jitter_raw=3,
                                epc_bits=EPC_BITS[b], **kw)


def oracle_of(oracle_mod, host, lens, **cfg):
    """-> (oracle Results, expected rows per trace)"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ref.expected_batch(oracle_mod, refs, ys)


def counts(rows):
    """-> (reads, pass at the PC's length, longer than the slot, the decoder's own length)"""
    f = rows["flags"]
    return int((f & 1).sum()), int(((f & 2) != 0).sum()), int(((f & 8) != 0).sum()), int(((f & 16) != 0).sum())


def check_rows(ctx, want, what="", extra=3):
    """every trace's row of the last batch_lengths_enqueue against the reference's, the rows behind it zero, nrows == n_windows_used / 2
    -> the bytes of all rows"""
    st = ctx.batch_stats()
    blob = b""
    for b, w in enumerate(want):
        r = ctx.batch_window_lengths(b, extra=extra)
        assert int(st[b]["n_windows_used"]) // 2 == len(w), (what, b, int(st[b]["n_windows_used"]), len(w))
        assert len(r) >= len(w) and (extra > 1000 or len(r) == len(w) + extra), (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, b)
        ref.assert_equal(r[: len(w)], w, (what, b))
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_window_lengths(ctx._h, b, None, 0, C.byref(n)) in (0, -5) and n.value == len(w)
        blob += r[: len(w) + 3].tobytes()
    return blob


@pytest.fixture(scope="module")
def ragged(backend, oracle_mod, synth_mod):
    ts = [trace_of(synth_mod, b) for b in range(4)]
    host, lens, L, stride = lay_out([t.samples for t in ts], odd_stride=True)
    refs, want = oracle_of(oracle_mod, host, lens)
    assert stride & 1
    long_, own = 0, 0
    for b, w in enumerate(want):                                  # (on the reference alone, before anything runs)
        reads, found, too_long, own_len = counts(w)
        long_, own = long_ + too_long, own + own_len
        assert len(w) == len(ts[b].slots) == 4 * ROUNDS[b]
        if b != 2:
            assert found >= 3, (b, reads, found)
        if b in (0, 2):
            assert reads >= 3, (b, reads, found)
    assert long_ >= 3 and own >= 3, (long_, own)
    # the third group of lanes holds 32, 16 and 0 lanes, and some frames end inside the first group
    seen = {int(r["n_bits"]) for w in want for r in w[(w["flags"] & 2) != 0]}
    assert {160, 144, 32, 64} <= seen and 128 not in seen, seen
    return host, lens, L, stride, refs, want, [t.slots for t in ts], backend.put(host, lens)


@pytest.fixture(scope="module")
def ragged_rows(backend, ragged):
    """one pass over the ragged batch through the fused front end -> (the rows per trace, their bytes, lengths ms, decode ms, results)"""
    import rfid
    host, lens, L, stride, refs, want, slots, dev = ragged
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(4, L)
        ctx.batch_plan_lengths()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_lengths_enqueue()
        blob = check_rows(ctx, want, "fixture")
        assert ctx.batch_ls_report()["pieces"] == 0
        rows = [ctx.batch_window_lengths(b) for b in range(4)]
        w, r, _ = ctx.batch_windows()
        return rows, blob, ctx.batch_lengths_ms(), ctx.batch_timing()["decode_ms"], [r[w["stream"] == b] for b in range(4)]
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def small(backend, ragged):
    """the second and the fourth trace of the ragged batch (20 and 12 EPC windows) as a batch of their own: what the protocol cases run on"""
    host, lens, L, stride, refs, want, slots, _ = ragged
    pick = [1, 3]
    w = [want[k].copy() for k in pick]
    for b, r in enumerate(w):
        r["stream"] = b
    h, l = np.ascontiguousarray(host[pick]), lens[pick].copy()
    return h, l, L, stride, [refs[k] for k in pick], w, backend.put(h, l)


def test_abi_version_is_7():
    import rfid
    assert rfid.capi.load().rfid_abi_version() == 7


def test_ragged_batch_equals_the_reference_in_both_front_end_modes(backend, ragged, ragged_rows):
    """the ragged batch, backend.reps passes through the fused front end and one through the long-stream front end (modes 0 and 2):
    the reference's records and the same table bytes every time"""
    import rfid
    host, lens, L, stride, refs, want, slots, dev = ragged
    rows, blob, ms, decode_ms, _ = ragged_rows
    print("%s: lengths of the ragged batch (%d EPC windows, %d decoded): %.4f ms; decode of the same pass %.4f ms" %
          (backend.name, sum(map(len, want)), sum(int((w["n_bits"] > 0).sum()) for w in want), ms, decode_ms))
    assert ms >= 0.0
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(4, L)
        ctx.batch_plan_lengths()
        for mode in [0] * (backend.reps - 1) + [2]:
            ctx.batch_set_long_stream(mode)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_lengths_enqueue()
            assert check_rows(ctx, want, mode) == blob
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        many = ctx.batch_window_lengths(3, extra=10_000)          # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(want[3])], want[3])
        assert len(many) > len(want[3]) and not many[len(want[3]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_truth_every_lost_single_reply_of_another_length_is_recovered_and_no_empty_or_collided_slot_is(ragged, ragged_rows):
    """Against SlotTruth: every single-responder EPC reply with an intact CRC and L != 6 that the decoder failed has flags bit 1, the
    frame that was sent and the right n_bits; no window of an empty or collided slot has bit 1.  A condition, not a measurement: the
    seeds are such that the reference alone meets it.  And for every decoded row: frame words 0 .. 3, masked to n bits, are the
    result's own bits"""
    host, lens, L, stride, refs, want, slots, _ = ragged
    rows, results = ragged_rows[0], ragged_rows[4]
    lost = 0
    for b in range(4):
        assert len(rows[b]) == len(slots[b])
        for rec, sl in zip(rows[b], slots[b]):
            single = sl.n_tags == 1 and sl.epc_valid
            if single and not rec["flags"] & 1 and len(sl.epc) != 128:
                lost += 1
                assert rec["flags"] & 2 and rec["n_bits"] == len(sl.epc) and list(ref.frame_bits(rec)) == list(sl.epc), (b, rec, sl)
                assert rec["words"] == (len(sl.epc) - 32) // 16
            if not single:
                assert not rec["flags"] & 2 and sl.epc is None, (b, rec, sl)
            if rec["n_bits"]:
                n = min(int(rec["n_bits"]), 128)
                mask = np.array([(1 << min(max(n - 32 * i, 0), 32)) - 1 for i in range(4)], dtype=np.uint64).astype(np.uint32)
                res = results[b][int(rec["seq"])]
                assert res["type"] == 1 and res["crc_ok"] == 0
                assert (rec["frame"][:4] & mask == res["bits"] & mask).all() and not (rec["frame"][:4] & ~mask).any(), (b, rec, res)
    assert lost >= 20


def oracle_of_q0(oracle_mod, x, stream=0):
    o = oracle_mod.run_trace(x, oracle_mod.config(fixed_q=0))
    return ref.expected(oracle_mod, o, oracle_mod.fir(x), stream)


def test_trace_end_is_never_read_past(backend, oracle_mod, synth_mod):
    """One tag with a 128-bit EPC, tail_us = 40, the trace cut one filtered sample short of the furthest sample its last frame's last
    decision takes: that index is held at the trace's last sample -- flags bit 2 -- the frame is recovered all the same and the record
    is the reference's; cut 100 samples earlier, the frame's end is missing: bit 2 alone.  Then the first of these traces as the
    short row of a batch whose other row is longer, the rest of its row filled with large samples, behind a pass over other samples
    in the same plan (which leaves the filter's output of a LONGER trace in that row): identical bytes -- nothing behind the trace's
    own length is read"""
    import rfid
    F = np.float32
    t = synth_mod.make_trace(n_rounds=2, fixed_q=0, tag_ids=(5,), seed=3, sigma=SIGMA, t1_jitter_raw=3, tail_us=40, epc_bits=(128,))
    o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=0))
    k = o.n_windows - 1
    assert k & 1 and o.n_windows == 4 and not o.dumps[k]["crc_ok"]
    d = o.dumps[k]
    far = int(F(F(F(F(2 * 159) * d["T"]) + d["T"]) + F(d["index"])))          # the second sample of decision 159
    assert 1600 < far < ref.SPAN
    n_raw = 5 * (int(o.open_idx[k]) + far)                                   # (the trace's last own sample: far - 1)
    assert n_raw < len(t.samples)
    short = t.samples[:n_raw]
    want = oracle_of_q0(oracle_mod, short)
    assert len(want) == 2 and want[1]["flags"] == 2 | 4 and want[0]["flags"] == 2, want["flags"]
    assert list(ref.frame_bits(want[1])) == list(t.slots[1].epc) and want[1]["n_bits"] == 160
    shorter = oracle_of_q0(oracle_mod, short[:n_raw - 500])
    assert len(shorter) == 2 and shorter[1]["flags"] == 4 and shorter[0].tobytes() == want[0].tobytes()
    long_ = synth_mod.make_trace(n_rounds=3, fixed_q=0, tag_ids=(9,), seed=4, sigma=SIGMA, epc_bits=(64,)).samples
    assert len(long_) > len(short) + 5 * 400
    host1, lens1, L1, stride1 = lay_out([short])
    host2, lens2, L2, stride2 = lay_out([short, long_], odd_stride=True)
    host2[0, len(short):] = np.complex64(1000 - 500j)              # (behind the trace's own length: never to be read)
    hostA, lensA, _, _ = lay_out([long_, long_[: len(long_) - 7]], odd_stride=True)
    assert hostA.shape == host2.shape
    want2 = [want, oracle_of_q0(oracle_mod, long_, stream=1)]
    assert counts(want2[1])[1] >= 2
    blobs = []
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L2)
        ctx.batch_plan_lengths()
        ctx.batch_set_streams(1)
        d1 = backend.put(host1, lens1)
        backend.run_pass(ctx, d1, L1, stride1)
        ctx.batch_lengths_enqueue()
        blobs.append(check_rows(ctx, [want], "alone"))
        lens0 = lens1.copy()
        lens0[0] = n_raw - 500
        d0 = backend.put(host1, lens0)
        backend.run_pass(ctx, d0, L1, stride1)
        ctx.batch_lengths_enqueue()
        check_rows(ctx, [shorter], "cut inside the frame's tail")
        ctx.batch_set_streams(2)
        dA, d2 = backend.put(hostA, lensA), backend.put(host2, lens2)
        backend.run_pass(ctx, dA, L2, stride2)                     # (the row of the short trace now holds a longer trace's y)
        ctx.batch_lengths_enqueue()
        backend.run_pass(ctx, d2, L2, stride2)
        ctx.batch_lengths_enqueue()
        check_rows(ctx, want2, "short row")
        blobs.append(ctx.batch_window_lengths(0, extra=3).tobytes())
    finally:
        ctx.close()
    assert blobs[0] == blobs[1]


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, ragged):
    """MAX_NUM_QUERIES = 5 reached inside the first block of eight rows of the longer traces: nrows == n_windows_used / 2 = 5, the rows
    behind it zero, also when more rows are asked for than the table has.  Then in one context: rows an earlier pass had filled are
    zeroed again"""
    import rfid
    host, lens, L, stride, full_refs, full_want, slots, dev = ragged
    refs, want = oracle_of(oracle_mod, host, lens, max_num_queries=5)
    assert [o.state.status for o in refs] == [1, 1, 1, 1] and [len(w) for w in want] == [5, 5, 5, 5]
    assert sum(int(((w["flags"] & 1) == 0).sum()) for w in want) >= 10
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=5)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(4, L)
        ctx.batch_plan_lengths()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_lengths_enqueue()
        check_rows(ctx, want, "cut")
        check_rows(ctx, want, "cut, all rows", extra=10_000)
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(4, L)
        ctx.batch_plan_lengths()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_lengths_enqueue()
        check_rows(ctx, full_want, "full")
        cut = lens.copy()
        for b in range(4):
            cut[b] = 5 * int(full_refs[b].open_idx[2 * (3 + b) + 1] + ref.EPC_WIN + 60)       # (4, 5, 6 and 7 EPC windows)
        short_refs, short = oracle_of(oracle_mod, host, cut)
        assert [len(r) for r in short] == [4, 5, 6, 7]
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ctx.batch_lengths_enqueue()
        check_rows(ctx, short, "short", extra=10_000)
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_a_new_plan_and_a_small_grid(backend, small):
    """A plan of five traces, two of them processed: two passes give the same table bytes, the second with lengths_wgs = 3 (five blocks
    of rows on three workgroups: a workgroup goes round its loop again); the traces not covered are not fetched; a new plan drops
    the workspace"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(5, L)
        ctx.batch_plan_lengths()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            if rep:
                ctx.set_knob("lengths_wgs", 3)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_lengths_enqueue()
            blobs.append(check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1] and ctx.get_knob("lengths_wgs") == 3
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_lengths(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID     # (not covered)
        ctx.batch_plan(2, L)
        for fn in (ctx.batch_lengths_enqueue, lambda: ctx.batch_window_lengths(0), ctx.batch_lengths_ms):
            with pytest.raises(rfid.capi.RfidError) as e:
                fn()
            assert e.value.status == rfid.capi.ERR_STATE
        backend.run_pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_lengths_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_lengths" in str(e.value)
        ctx.batch_plan_lengths()
        ctx.batch_lengths_enqueue()                              # (the pass before the workspace: its statistics are current)
        assert check_rows(ctx, want, "planned again") == blobs[0]
    finally:
        ctx.close()


@pytest.mark.parametrize("overlap", [1, 2])
def test_overlap_each_pass_gets_its_own_records(backend, small, overlap):
    """RFID_OVERLAP 1 and 2 (two result sets where the plan has them): the next pass -- the traces in the other order -- enqueued BEFORE
    this pass's records are fetched leaves them this pass's, then gets its own"""
    import rfid
    host, lens, L, stride, refs, want, dev_a = small
    dev_b = backend.put(np.ascontiguousarray(host[::-1]), lens[::-1].copy())

    def stamped(order):
        out = []
        for b, k in enumerate(order):
            r = want[k].copy()
            r["stream"] = b
            out.append(r)
        return out

    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.set_knob("overlap", overlap)
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_lengths()
        for rep in range(2):
            backend.run_pass(ctx, dev_a, L, stride)
            ctx.batch_lengths_enqueue()
            backend.run_pass(ctx, dev_b, L, stride)
            for b, w in enumerate(stamped((0, 1))):
                ref.assert_equal(ctx.batch_window_lengths(b), w, ("a", rep, b))
            ctx.batch_lengths_enqueue()
            check_rows(ctx, stamped((1, 0)), ("b", rep))
    finally:
        ctx.close()


def other_outputs(ctx, n):
    """everything else a pass and its stages report, as bytes (the other stages of the last pass are enqueued here)"""
    ent, counts_ = ctx.batch_inventory()
    reads, off = ctx.batch_tracks()
    q = ctx.batch_quality()
    rep = ctx.batch_repair()
    fine = ctx.batch_fine()
    ctx.batch_slots_enqueue()
    ctx.batch_commands_enqueue()
    ctx.batch_retune_enqueue()
    ctx.batch_collisions_enqueue()
    w, r, _ = ctx.batch_windows()
    parts = [ent, counts_, reads, off, q, rep, fine, ctx.batch_stats(), w, r]
    for b in range(n):
        parts += [ctx.batch_window_quality(b, extra=2), ctx.batch_window_repairs(b, extra=2), ctx.batch_window_fine(b, extra=2),
                  ctx.batch_window_moments(b, extra=2), ctx.batch_window_commands(b, extra=2), ctx.batch_window_retunes(b, extra=2),
                  ctx.batch_window_collisions(b, extra=2)]
    return [np.ascontiguousarray(p).tobytes() for p in parts]


@pytest.mark.parametrize("order", ["lengths-first", "lengths-last"])
def test_other_stages_results_and_statistics_are_untouched(backend, small, order):
    """inventory, tracks, quality, repair, fine, slots, commands, retune and collisions on the same pass, with the lengths stage enqueued
    before or behind them and without it: every other fetched array -- results and statistics among them -- is byte-identical"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    outs = []
    for lengths in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_inventory(8)
            ctx.batch_plan_tracks()
            for plan in (ctx.batch_plan_quality, ctx.batch_plan_repair, ctx.batch_plan_fine, ctx.batch_plan_slots, ctx.batch_plan_commands,
                         ctx.batch_plan_retune, ctx.batch_plan_collisions):
                plan()
            if lengths:
                ctx.batch_plan_lengths()
            backend.run_pass(ctx, dev, L, stride)
            if lengths and order == "lengths-first":
                ctx.batch_lengths_enqueue()
            outs.append(other_outputs(ctx, 2))
            if lengths and order == "lengths-last":
                ctx.batch_lengths_enqueue()
            if lengths:
                check_rows(ctx, want, order)
                assert other_outputs(ctx, 2) == outs[-1]         # (and the stage lowered nothing: the others run again behind it)
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs)), [a == b for a, b in zip(*outs)]
    assert sum(map(len, outs[0])) > 5_000


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
        raises(ctx.batch_plan_lengths, ERR_STATE)                 # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_lengths_enqueue, ERR_STATE)              # no workspace
        ctx.batch_plan_lengths()
        raises(ctx.batch_lengths_enqueue, ERR_STATE)              # no pass
        raises(lambda: ctx.batch_window_lengths(0), ERR_STATE)    # nothing enqueued
        raises(ctx.batch_lengths_ms, ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_lengths(0), ERR_STATE)    # a pass, but nothing enqueued behind it
        ctx.batch_lengths_enqueue()                               # (no inventory workspace: none is needed)
        blob = check_rows(ctx, want, "no inventory")
        # the level of the other stages is neither raised ...
        ctx.batch_plan_inventory(8)                               # (does not drop the lengths workspace)
        ctx.batch_plan_tracks()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)               # (the lengths stage is not an inventory)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_lengths_enqueue()
        ctx.batch_tracks_enqueue()                                # ... nor lowered: the inventory is still this pass's
        assert check_rows(ctx, want, "behind the tracks") == blob
        # a caller's array that is too small loses nothing
        row = np.zeros(len(want[0]) - 1, dtype=rfid.capi.SIZED_FRAME_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_window_lengths(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not row.tobytes().strip(b"\0")
        assert "EPC windows" in ctx._lib.rfid_last_error(ctx._h).decode()
        full = np.zeros(n.value, dtype=rfid.capi.SIZED_FRAME_DTYPE)
        assert ctx._lib.rfid_batch_get_window_lengths(ctx._h, 0, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        for s in (2, -1):
            assert ctx._lib.rfid_batch_get_window_lengths(ctx._h, s, None, 0, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_lengths(ctx._h, 0, None, 0, None) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_lengths(ctx._h, 0, None, 4, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_lengths_ms(ctx._h, None) == ERR_INVALID
        for fn in ("rfid_batch_plan_lengths", "rfid_batch_lengths"):
            assert getattr(ctx._lib, fn)(None) == ERR_INVALID
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_lengths_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_lengths(0), ERR_STATE)
    finally:
        ctx.close()


# ---- rfid_length_window on crafted, noise-free spans ----------------------------------------------------------------------------
def crafted_y(oracle_mod, synth_mod, frame, lead=100):
    """the matched filter's output of one noise-free, leak-free EPC reply of any length, `lead` raw samples into the trace"""
    wave = np.repeat(synth_mod.fm0_levels(frame), 25)
    raw = np.zeros(5 * 1800, dtype=np.complex64)
    assert lead + len(wave) < len(raw)
    raw[lead:lead + len(wave)] = H * wave
    return oracle_mod.fir(raw)


def crafted_frame(synth_mod, words):
    """PC + EPC + CRC-16 with an EPC of `words` words"""
    return synth_mod.sized_epc_frame(synth_mod.resize_epc(synth_mod.epc_for_id(0x27, np.random.default_rng(5)), 16 * words))


def result_for(oracle_mod, span):
    """the decoder's own result for the span's first 1 370 samples (the oracle's), as the library's record"""
    return repair_ref.result_of_dump(oracle_mod.decode_window(np.ascontiguousarray(span[: ref.EPC_WIN]), 1))


def with_words(res, words):
    """the result with its first five bits rewritten to announce `words`"""
    r = res.copy()
    w0 = int(r["bits"][0]) & ~0x1F
    for i in range(5):
        w0 |= ((words >> (4 - i)) & 1) << i
    r["bits"][0] = w0
    return r


def test_length_window_over_all_sync_offsets(oracle_mod, synth_mod, call_ctx):
    """L = 8, the span cut so that the decoder's sync offset takes every value 0 .. 14: each is recovered with the frame that was sent,
    the record the reference's (the literal loop on the first and the last)"""
    frame = crafted_frame(synth_mod, 8)
    assert len(frame) == 160
    y = crafted_y(oracle_mod, synth_mod, frame)
    seen = set()
    for a in range(0, 40):
        span = y[a:a + ref.SPAN]
        res = result_for(oracle_mod, span)
        m = int(res["index"]) - 65
        if m in seen:
            continue
        assert res["crc_ok"] == 0
        want = ref.expected_window(oracle_mod, span, res, literal=m in (0, 14))
        if not (want["flags"] & 2 and list(ref.frame_bits(want)) == list(frame)):
            continue                                               # (the reply has left the span, or the sync is an alias)
        seen.add(m)
        got = call_ctx.length_window(span, res)
        ref.assert_equal(got, want, m)
        assert got["flags"] == 2 and got["words"] == 8 and got["n_bits"] == 160 and got["crc_rcvd"] == got["crc_calc"]
    assert sorted(seen) == list(range(15)), sorted(seen)


def test_length_window_at_every_length(oracle_mod, synth_mod, call_ctx):
    """every L = 0 .. 8: but for 6 the frame that was sent, with its n_bits; at 6 the decoder reads it itself (flags == 1), and with
    a bit flipped it is the decoder's own length: bit 4 alone.  A PC rewritten to L = 9 and to L = 31: bit 3 alone"""
    for words in range(9):
        frame = crafted_frame(synth_mod, words)
        span = crafted_y(oracle_mod, synth_mod, frame)[10:10 + ref.SPAN]
        res = result_for(oracle_mod, span)
        want = ref.expected_window(oracle_mod, span, res, literal=True)
        got = call_ctx.length_window(span, res)
        ref.assert_equal(got, want, words)
        if words == 6:
            assert res["crc_ok"] == 1 and got["flags"] == 1 and not got.tobytes()[16:].strip(b"\0")
            bad = list(frame)
            bad[40] ^= 1
            span = crafted_y(oracle_mod, synth_mod, bad)[10:10 + ref.SPAN]
            res = result_for(oracle_mod, span)
            assert res["crc_ok"] == 0
            got = call_ctx.length_window(span, res)
            ref.assert_equal(got, ref.expected_window(oracle_mod, span, res), "6, flipped")
            assert got["flags"] == 16 and got["words"] == 6 and not got.tobytes()[20:].strip(b"\0")
        else:
            assert res["crc_ok"] == 0 and got["flags"] == 2 and got["words"] == words and got["n_bits"] == 32 + 16 * words == len(frame)
            assert list(ref.frame_bits(got)) == list(frame) and not (np.asarray(got["frame"]).view(np.uint8)[(len(frame) + 7) // 8:]).any()
    for words in (9, 31):
        r = with_words(res, words)                                 # (res: the L = 8 window's)
        got = call_ctx.length_window(span, r)
        ref.assert_equal(got, ref.expected_window(oracle_mod, span, r), words)
        assert got["flags"] == 8 and got["words"] == words and not got.tobytes()[20:].strip(b"\0")


def test_length_window_on_crafted_spans(oracle_mod, synth_mod, call_ctx):
    frame = crafted_frame(synth_mod, 8)
    y = crafted_y(oracle_mod, synth_mod, frame)
    span = y[10:10 + ref.SPAN]
    res = result_for(oracle_mod, span)
    # a result that says the CRC held: nothing is done
    held = res.copy()
    held["crc_ok"] = 1
    got = call_ctx.length_window(span, held)
    assert got["flags"] == 1 and not got.tobytes()[16:].strip(b"\0")
    ref.assert_equal(got, ref.expected_window(oracle_mod, span, held), "held")
    # one frame bit flipped, behind decision 127: the frame fails, and the two CRCs say so
    bad = list(frame)
    bad[140] ^= 1
    bspan = crafted_y(oracle_mod, synth_mod, bad)[10:10 + ref.SPAN]
    bres = result_for(oracle_mod, bspan)
    want = ref.expected_window(oracle_mod, bspan, bres, literal=True)
    assert want["flags"] == 0 and want["n_bits"] == 160 and want["crc_calc"] != want["crc_rcvd"] and list(ref.frame_bits(want)) == bad
    ref.assert_equal(call_ctx.length_window(bspan, bres), want, "flipped")
    # all zero: no decision is positive -- bit 0 alone is set, the frame fails
    zero = np.zeros(ref.SPAN, dtype=np.complex64)
    want = ref.expected_window(oracle_mod, zero, res, literal=True)
    assert want["flags"] == 0 and want["n_bits"] == 160 and list(want["frame"]) == [1, 0, 0, 0, 0]
    ref.assert_equal(call_ctx.length_window(zero, res), want, "zero")
    # n = 1370 with L = 8: the frame runs behind the span's end -- held at n - 1, flags bit 2 -- and so does every n up to the furthest index
    far = int(np.float32(np.float32(np.float32(np.float32(318) * res["T"]) + res["T"]) + np.float32(res["index"])))
    assert 1600 < far < ref.SPAN - 1
    for n in (1370, 1500, far, far + 1, ref.SPAN):
        want = ref.expected_window(oracle_mod, span[:n], res, literal=n == 1370)
        assert bool(want["flags"] & 4) == (n <= far) and (n > 1500 or not want["flags"] & 2) and (n < far or want["flags"] & 2), (n, want)
        ref.assert_equal(call_ctx.length_window(span[:n], res), want, n)
    # a short frame needs nothing behind the window: n = 1370 with L = 4 is whole
    f4 = crafted_frame(synth_mod, 4)
    s4 = crafted_y(oracle_mod, synth_mod, f4)[10:10 + ref.EPC_WIN]
    r4 = result_for(oracle_mod, s4)
    want = ref.expected_window(oracle_mod, s4, r4, literal=True)
    assert want["flags"] == 2 and list(ref.frame_bits(want)) == list(f4)
    ref.assert_equal(call_ctx.length_window(s4, r4), want, "short frame, short span")


def test_length_window_refuses(oracle_mod, synth_mod, call_ctx):
    import rfid
    span = crafted_y(oracle_mod, synth_mod, crafted_frame(synth_mod, 8))[10:10 + ref.SPAN]
    res = result_for(oracle_mod, span)
    for n in (1369, 1729, 0):
        with pytest.raises(ValueError):
            call_ctx.length_window(np.zeros(n, dtype=np.complex64), res)
    with pytest.raises(ValueError):
        call_ctx.length_window(np.zeros((2, 1400), dtype=np.complex64), res)
    lib, h, INVALID = call_ctx._lib, call_ctx._h, rfid.capi.ERR_INVALID
    r = np.zeros(1, dtype=rfid.capi.RESULT_DTYPE)
    out = np.zeros(1, dtype=rfid.capi.SIZED_FRAME_DTYPE)
    r[0] = res
    args = lambda n=ref.SPAN, s=span.ctypes.data, rr=r.ctypes.data, o=out.ctypes.data: (h, s, n, rr, o)
    assert lib.rfid_length_window(*args()) == rfid.capi.OK
    ref.assert_equal(out[0], ref.expected_window(oracle_mod, span, res), "accepted")
    for n in (1369, 1729, -1):
        assert lib.rfid_length_window(*args(n=n)) == INVALID
        assert "rfid_length_window" in lib.rfid_last_error(h).decode()
    assert lib.rfid_length_window(*args(s=None)) == INVALID and lib.rfid_length_window(*args(rr=None)) == INVALID
    assert lib.rfid_length_window(*args(o=None)) == INVALID and lib.rfid_length_window(None, *args()[1:]) == INVALID
    F = np.float32
    for field, value in (("type", 0), ("index", 64), ("index", 80), ("T", np.nextafter(F(4.95), F(0))), ("T", np.nextafter(F(5.05), F(9))),
                         ("T", F(0)), ("T", F(np.nan))):
        r[0] = res
        r[0][field] = value
        assert lib.rfid_length_window(*args()) == INVALID, (field, value)
        assert "rfid_length_window" in lib.rfid_last_error(h).decode()
    for value in (F(4.95), F(5.05)):                               # (the ends of the decoder's own range are accepted)
        r[0] = res
        r[0]["T"] = value
        assert lib.rfid_length_window(*args()) == rfid.capi.OK

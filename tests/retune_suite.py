"""The cases of the retune stage that run on both sides, written once: tests/test_retune_emu.py (the kernels on the wave emulator) and
tests/test_gpu_retune.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches the
library) and `call_ctx` (the context of the per-call cases).  Pytest collects the imported functions in the importing module, resolves
their fixtures there and applies that module's marks.  Every expected record is worked out in numpy from the ORACLE alone
(tests/retune_ref.py) and every comparison is exact.

The ragged batch: four traces of 6, 5, 4 and 3 rounds, FIXED_Q = 2, three tags, sigma = 0.03, t1_jitter_raw = 3, odd row stride, the tags'
half-bit periods off by (-4, 0, +4) %, (-2.5, +1.1, +2.5) %, (0, 0, 0) and (+4, +4, -4) %.  What is asserted of it before anything runs
(on the reference alone): every trace but the third holds at least 3 retuned and 3 failed-and-not-retuned windows, and every trace
with a tag inside the decoder's own +- 1 % -- the first and the third -- at least 3 reads.  (A trace whose tags are ALL off by 2.5 % or
more cannot hold a read: the decoder reads none of them, which is what the stage is for; at + 1.1 % it reads one reply in sixty.)"""
import ctypes as C

import numpy as np
import pytest

import repair_ref
import retune_ref as ref
from stage_backend import lay_out

__all__ = ["ragged", "ragged_rows", "small", "test_abi_version_is_7", "test_ragged_batch_equals_the_reference_in_both_front_end_modes",
           "test_truth_every_lost_single_reply_is_retuned_and_no_empty_or_collided_slot_is",
           "test_trace_end_is_never_read_past", "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero",
           "test_plan_larger_than_the_batch_a_new_plan_and_a_small_grid", "test_overlap_each_pass_gets_its_own_records",
           "test_other_stages_results_and_statistics_are_untouched", "test_protocol_capacity_and_state_errors",
           "test_retune_window_over_all_sync_offsets", "test_retune_window_on_crafted_spans", "test_retune_window_refuses"]

SIGMA = 0.03
OFFSETS = ((-0.04, 0.0, 0.04), (-0.025, 0.011, 0.025), (0.0, 0.0, 0.0), (0.04, 0.04, -0.04))
ROUNDS = (6, 5, 4, 3)
SEED = 30                                    # trace b: seed 30 + b (chosen so that retune_ref alone meets the truth case)
H = np.complex64(0.1 * np.exp(2.1j))         # the crafted spans' channel


def trace_of(synth_mod, b, **kw):
    return synth_mod.make_trace(n_rounds=ROUNDS[b], fixed_q=2, tag_ids=(1, 2, 3), seed=SEED + b, sigma=SIGMA, t1_jitter_raw=3,
                                blf_offsets=OFFSETS[b], **kw)


def oracle_of(oracle_mod, host, lens, **cfg):
    """-> (oracle Results, expected retune rows per trace)"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ref.expected_batch(oracle_mod, refs, ys)


def counts(rows):
    """-> (reads, retuned, failed and not retuned)"""
    f = rows["flags"]
    return int((f & 1).sum()), int(((f & 2) != 0).sum()), int(((f & 3) == 0).sum())


def check_rows(ctx, want, what="", extra=3):
    """every trace's row of the last batch_retune_enqueue against the reference's, the rows behind it zero, nrows == n_windows_used / 2
    -> the bytes of all rows"""
    st = ctx.batch_stats()
    blob = b""
    for b, w in enumerate(want):
        r = ctx.batch_window_retunes(b, extra=extra)
        assert int(st[b]["n_windows_used"]) // 2 == len(w), (what, b, int(st[b]["n_windows_used"]), len(w))
        assert len(r) >= len(w) and (extra > 1000 or len(r) == len(w) + extra), (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, b)
        ref.assert_equal(r[: len(w)], w, (what, b))
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_window_retunes(ctx._h, b, None, 0, C.byref(n)) in (0, -5) and n.value == len(w)
        blob += r[: len(w) + 3].tobytes()
    return blob


@pytest.fixture(scope="module")
def ragged(backend, oracle_mod, synth_mod):
    ts = [trace_of(synth_mod, b) for b in range(4)]
    host, lens, L, stride = lay_out([t.samples for t in ts], odd_stride=True)
    refs, want = oracle_of(oracle_mod, host, lens)
    assert stride & 1
    for b, w in enumerate(want):                                  # (on the reference alone, before anything runs)
        reads, retuned, lost = counts(w)
        assert len(w) == len(ts[b].slots) == 4 * ROUNDS[b]
        if b != 2:
            assert retuned >= 3 and lost >= 3, (b, reads, retuned, lost)
        if b in (0, 2):
            assert reads >= 3, (b, reads, retuned, lost)
    return host, lens, L, stride, refs, want, [t.slots for t in ts], backend.put(host, lens)


@pytest.fixture(scope="module")
def ragged_rows(backend, ragged):
    """one pass over the ragged batch through the fused front end -> (the rows per trace, their bytes, retune ms, decode ms)"""
    import rfid
    host, lens, L, stride, refs, want, slots, dev = ragged
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(4, L)
        ctx.batch_plan_retune()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_retune_enqueue()
        blob = check_rows(ctx, want, "fixture")
        assert ctx.batch_ls_report()["pieces"] == 0
        rows = [ctx.batch_window_retunes(b) for b in range(4)]
        return rows, blob, ctx.batch_retune_ms(), ctx.batch_timing()["decode_ms"]
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
    rows, blob, ms, decode_ms = ragged_rows
    print("%s: retune of the ragged batch (%d EPC windows, %d searched): %.4f ms; decode of the same pass %.4f ms" %
          (backend.name, sum(map(len, want)), sum(int(((w["flags"] & 1) == 0).sum()) for w in want), ms, decode_ms))
    assert ms >= 0.0
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(4, L)
        ctx.batch_plan_retune()
        for mode in [0] * (backend.reps - 1) + [2]:
            ctx.batch_set_long_stream(mode)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_retune_enqueue()
            assert check_rows(ctx, want, mode) == blob
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        many = ctx.batch_window_retunes(3, extra=10_000)          # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(want[3])], want[3])
        assert len(many) > len(want[3]) and not many[len(want[3]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_truth_every_lost_single_reply_is_retuned_and_no_empty_or_collided_slot_is(ragged, ragged_rows):
    """Against SlotTruth: every single-responder EPC reply with an intact CRC that the decoder failed is retuned with the frame that
    was sent; no window of an empty or collided slot has flags bit 1.  A condition, not a measurement: the seeds are such that the
    reference alone meets it"""
    host, lens, L, stride, refs, want, slots, _ = ragged
    rows = ragged_rows[0]
    lost = 0
    for b in range(4):
        assert len(rows[b]) == len(slots[b])
        for rec, sl in zip(rows[b], slots[b]):
            single = sl.n_tags == 1 and sl.epc_valid
            if single and not rec["flags"] & 1:
                lost += 1
                assert rec["flags"] & 2 and list(ref.frame_bits(rec)) == list(sl.epc), (b, rec, sl)
            if not single:
                assert not rec["flags"] & 2 and sl.epc is None, (b, rec, sl)
    assert lost >= 20


def test_trace_end_is_never_read_past(backend, oracle_mod, synth_mod):
    """One + 4 % tag, tail_us = 40, the trace cut 30 filtered samples behind the close of its last EPC window (the reader's carrier goes
    on for 376 samples behind that window, whatever the tail): the search runs into the trace's end -- flags bit 2 -- the frame is
    retuned all the same and the record is the reference's; cut 20 samples behind it, the frame's end is missing: bit 2 alone.  Then
    the first of these traces as the short row of a batch whose other row
    is longer, the rest of its row filled with large samples, behind a pass over other samples in the same plan (which leaves the
    filter's output of a LONGER trace in that row): identical bytes -- nothing behind the trace's own length is read"""
    import rfid
    t = synth_mod.make_trace(n_rounds=2, fixed_q=0, tag_ids=(5,), seed=3, sigma=SIGMA, t1_jitter_raw=3, tail_us=40, blf_offsets=(0.04,))
    o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=0))
    k = o.n_windows - 1
    assert k & 1 and o.n_windows == 4
    n_raw = 5 * (int(o.open_idx[k]) + ref.EPC_WIN + 30)
    assert n_raw < len(t.samples)
    short = t.samples[:n_raw]
    want = oracle_of_q0(oracle_mod, short)
    assert len(want) == 2 and want[1]["flags"] == 2 | 4 and want[0]["flags"] == 2, want["flags"]
    assert list(ref.frame_bits(want[1])) == list(t.slots[1].epc)
    shorter = oracle_of_q0(oracle_mod, short[:n_raw - 50])
    assert len(shorter) == 2 and shorter[1]["flags"] == 4 and shorter[0].tobytes() == want[0].tobytes()
    long_ = synth_mod.make_trace(n_rounds=3, fixed_q=0, tag_ids=(9,), seed=4, sigma=SIGMA, blf_offsets=(-0.04,)).samples
    assert len(long_) > len(short) + 5 * 200
    host1, lens1, L1, stride1 = lay_out([short])
    host2, lens2, L2, stride2 = lay_out([short, long_], odd_stride=True)
    host2[0, len(short):] = np.complex64(1000 - 500j)              # (behind the trace's own length: never to be read)
    hostA, lensA, _, _ = lay_out([long_, long_[: len(long_) - 7]], odd_stride=True)
    assert hostA.shape == host2.shape
    want2 = [want, oracle_of_q0(oracle_mod, long_, stream=1)]
    blobs = []
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L2)
        ctx.batch_plan_retune()
        ctx.batch_set_streams(1)
        d1 = backend.put(host1, lens1)
        backend.run_pass(ctx, d1, L1, stride1)
        ctx.batch_retune_enqueue()
        blobs.append(check_rows(ctx, [want], "alone"))
        lens0 = lens1.copy()
        lens0[0] = n_raw - 50
        d0 = backend.put(host1, lens0)
        backend.run_pass(ctx, d0, L1, stride1)
        ctx.batch_retune_enqueue()
        check_rows(ctx, [shorter], "cut 20 behind the window")
        ctx.batch_set_streams(2)
        dA, d2 = backend.put(hostA, lensA), backend.put(host2, lens2)
        backend.run_pass(ctx, dA, L2, stride2)                     # (the row of the short trace now holds a longer trace's y)
        ctx.batch_retune_enqueue()
        backend.run_pass(ctx, d2, L2, stride2)
        ctx.batch_retune_enqueue()
        check_rows(ctx, want2, "short row")
        blobs.append(ctx.batch_window_retunes(0, extra=3).tobytes())
    finally:
        ctx.close()
    assert blobs[0] == blobs[1]


def oracle_of_q0(oracle_mod, x, stream=0):
    o = oracle_mod.run_trace(x, oracle_mod.config(fixed_q=0))
    return ref.expected(oracle_mod, o, oracle_mod.fir(x), stream)


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
        ctx.batch_plan_retune()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_retune_enqueue()
        check_rows(ctx, want, "cut")
        check_rows(ctx, want, "cut, all rows", extra=10_000)
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(4, L)
        ctx.batch_plan_retune()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_retune_enqueue()
        check_rows(ctx, full_want, "full")
        cut = lens.copy()
        for b in range(4):
            cut[b] = 5 * int(full_refs[b].open_idx[2 * (3 + b) + 1] + ref.EPC_WIN + 60)       # (4, 5, 6 and 7 EPC windows)
        short_refs, short = oracle_of(oracle_mod, host, cut)
        assert [len(r) for r in short] == [4, 5, 6, 7]
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ctx.batch_retune_enqueue()
        check_rows(ctx, short, "short", extra=10_000)
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_a_new_plan_and_a_small_grid(backend, small):
    """A plan of five traces, two of them processed: two passes give the same table bytes, the second with retune_wgs = 3 (five blocks
    of rows on three workgroups: a workgroup goes round its loop again); the traces not covered are not fetched; a new plan drops
    the workspace"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(5, L)
        ctx.batch_plan_retune()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            if rep:
                ctx.set_knob("retune_wgs", 3)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_retune_enqueue()
            blobs.append(check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1] and ctx.get_knob("retune_wgs") == 3
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_retunes(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID     # (not covered)
        ctx.batch_plan(2, L)
        for fn in (ctx.batch_retune_enqueue, lambda: ctx.batch_window_retunes(0), ctx.batch_retune_ms):
            with pytest.raises(rfid.capi.RfidError) as e:
                fn()
            assert e.value.status == rfid.capi.ERR_STATE
        backend.run_pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_retune_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_retune" in str(e.value)
        ctx.batch_plan_retune()
        ctx.batch_retune_enqueue()                               # (the pass before the workspace: its statistics are current)
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
        ctx.batch_plan_retune()
        for rep in range(2):
            backend.run_pass(ctx, dev_a, L, stride)
            ctx.batch_retune_enqueue()
            backend.run_pass(ctx, dev_b, L, stride)
            for b, w in enumerate(stamped((0, 1))):
                ref.assert_equal(ctx.batch_window_retunes(b), w, ("a", rep, b))
            ctx.batch_retune_enqueue()
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
    w, r, _ = ctx.batch_windows()
    parts = [ent, counts_, reads, off, q, rep, fine, ctx.batch_stats(), w, r]
    for b in range(n):
        parts += [ctx.batch_window_quality(b, extra=2), ctx.batch_window_repairs(b, extra=2), ctx.batch_window_fine(b, extra=2),
                  ctx.batch_window_moments(b, extra=2), ctx.batch_window_commands(b, extra=2)]
    return [np.ascontiguousarray(p).tobytes() for p in parts]


@pytest.mark.parametrize("order", ["retune-first", "retune-last"])
def test_other_stages_results_and_statistics_are_untouched(backend, small, order):
    """inventory, tracks, quality, repair, fine, slots and commands on the same pass, with the retune stage enqueued before or behind
    them and without it: every other fetched array -- results and statistics among them -- is byte-identical"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    outs = []
    for retune in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_inventory(8)
            ctx.batch_plan_tracks()
            for plan in (ctx.batch_plan_quality, ctx.batch_plan_repair, ctx.batch_plan_fine, ctx.batch_plan_slots, ctx.batch_plan_commands):
                plan()
            if retune:
                ctx.batch_plan_retune()
            backend.run_pass(ctx, dev, L, stride)
            if retune and order == "retune-first":
                ctx.batch_retune_enqueue()
            outs.append(other_outputs(ctx, 2))
            if retune and order == "retune-last":
                ctx.batch_retune_enqueue()
            if retune:
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
        raises(ctx.batch_plan_retune, ERR_STATE)                  # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_retune_enqueue, ERR_STATE)               # no workspace
        ctx.batch_plan_retune()
        raises(ctx.batch_retune_enqueue, ERR_STATE)               # no pass
        raises(lambda: ctx.batch_window_retunes(0), ERR_STATE)    # nothing enqueued
        raises(ctx.batch_retune_ms, ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_retunes(0), ERR_STATE)    # a pass, but nothing enqueued behind it
        ctx.batch_retune_enqueue()                                # (no inventory workspace: none is needed)
        blob = check_rows(ctx, want, "no inventory")
        # the level of the other stages is neither raised ...
        ctx.batch_plan_inventory(8)                               # (does not drop the retune workspace)
        ctx.batch_plan_tracks()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)               # (the retune stage is not an inventory)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_retune_enqueue()
        ctx.batch_tracks_enqueue()                                # ... nor lowered: the inventory is still this pass's
        assert check_rows(ctx, want, "behind the tracks") == blob
        # a caller's array that is too small loses nothing
        row = np.zeros(len(want[0]) - 1, dtype=rfid.capi.RETUNE_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_window_retunes(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not row.tobytes().strip(b"\0")
        assert "EPC windows" in ctx._lib.rfid_last_error(ctx._h).decode()
        full = np.zeros(n.value, dtype=rfid.capi.RETUNE_DTYPE)
        assert ctx._lib.rfid_batch_get_window_retunes(ctx._h, 0, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        for s in (2, -1):
            assert ctx._lib.rfid_batch_get_window_retunes(ctx._h, s, None, 0, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_retunes(ctx._h, 0, None, 0, None) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_retunes(ctx._h, 0, None, 4, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_retune_ms(ctx._h, None) == ERR_INVALID
        for fn in ("rfid_batch_plan_retune", "rfid_batch_retune"):
            assert getattr(ctx._lib, fn)(None) == ERR_INVALID
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_retune_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_retunes(0), ERR_STATE)
    finally:
        ctx.close()


# ---- rfid_retune_window on crafted, noise-free spans ----------------------------------------------------------------------------
def crafted_y(oracle_mod, synth_mod, frame, delta, lead=100):
    """the matched filter's output of one noise-free, leak-free EPC reply whose half-bits last 25 (1 + delta) raw samples, `lead` raw
    samples into the trace"""
    lv = synth_mod.fm0_levels(frame)
    half = 25 * (1.0 + delta)
    at = np.floor(np.arange(int(np.ceil(len(lv) * half))) / half).astype(np.int64)
    wave = lv[at[at < len(lv)]]
    raw = np.zeros(5 * 1700, dtype=np.complex64)
    raw[lead:lead + len(wave)] = H * wave
    return oracle_mod.fir(raw)


def crafted_frame(synth_mod):
    return synth_mod.epc_frame(synth_mod.epc_for_id(0x27, np.random.default_rng(5)))


def result_for(oracle_mod, span):
    """the decoder's own result for the span's first 1 370 samples (the oracle's), as the library's record"""
    return repair_ref.result_of_dump(oracle_mod.decode_window(np.ascontiguousarray(span[: ref.EPC_WIN]), 1))


def test_retune_window_over_all_sync_offsets(oracle_mod, synth_mod, call_ctx):
    """delta = - 4 % and + 4 %, the span cut so that the decoder's sync offset takes every value 0 .. 14: each is retuned with the
    frame that was sent, t* at the grid's ends, the record the reference's (the literal loop on the first and the last)"""
    frame = crafted_frame(synth_mod)
    for delta in (-0.04, 0.04):
        y = crafted_y(oracle_mod, synth_mod, frame, delta)
        seen = {}
        for a in range(0, 40):
            span = y[a:a + ref.SPAN]
            res = result_for(oracle_mod, span)
            m = int(res["index"]) - 65
            if m in seen or res["crc_ok"]:
                continue
            want = ref.expected_window(oracle_mod, span, res, literal=m in (0, 14))
            if not (want["flags"] & 2 and list(ref.frame_bits(want)) == list(frame)):
                continue                                           # (the reply has left the span, or the sync is an alias)
            seen[m] = int(want["t_index"])
            got = call_ctx.retune_window(span, res)
            ref.assert_equal(got, want, (delta, m))
            assert got["flags"] == 2 and abs(5.0 * (1 + delta) - float(got["T"])) < 0.011
        assert sorted(seen) == list(range(15)), (delta, sorted(seen))
        assert all(t <= 2 for t in seen.values()) if delta < 0 else all(t >= 78 for t in seen.values()), seen


def test_retune_window_on_crafted_spans(oracle_mod, synth_mod, call_ctx):
    frame = crafted_frame(synth_mod)
    F = np.float32
    # delta = 0 with one frame bit flipped: t* is the middle of the grid, T = 5 exactly, and the frame still fails
    bad = list(frame)
    bad[40] ^= 1
    span = crafted_y(oracle_mod, synth_mod, bad, 0.0)[12:12 + ref.SPAN]
    res = result_for(oracle_mod, span)
    assert res["crc_ok"] == 0 and res["index"] == 78
    want = ref.expected_window(oracle_mod, span, res, literal=True)
    assert want["t_index"] == 40 and want["T"] == F(5.0) and want["flags"] == 0 and list(ref.frame_bits(want)) == bad
    ref.assert_equal(call_ctx.retune_window(span, res), want, "flipped")
    assert (want["frame"] == res["bits"]).all()                    # (at T = 5 the decoder's own bits)
    # ... and a result that says the CRC held: nothing is searched
    held = res.copy()
    held["crc_ok"] = 1
    got = call_ctx.retune_window(span, held)
    assert got["flags"] == 1 and not got.tobytes()[16:].strip(b"\0")
    ref.assert_equal(got, ref.expected_window(oracle_mod, span, held), "held")
    # all zero: t* = 0, every sum + 0.0; a constant span: every candidate has the same energy, the first wins
    for what, span in (("zero", np.zeros(ref.SPAN, dtype=np.complex64)), ("constant", np.full(ref.SPAN, 0.25 - 0.5j, dtype=np.complex64))):
        want = ref.expected_window(oracle_mod, span, res, literal=True)
        assert want["t_index"] == 0 and want["T"] == F(4.8) and not want["flags"] & 2
        if what == "zero":
            assert all(want[f].tobytes() == b"\0\0\0\0" for f in ("h_re", "h_im", "energy"))
        ref.assert_equal(call_ctx.retune_window(span, res), want, what)
    # n = 1370 with a + 4 % reply: the search runs behind the span's end -- held at n - 1, flags bit 2 -- and so does every n up to 1407
    y = crafted_y(oracle_mod, synth_mod, frame, 0.04)
    a4 = next(a for a in range(40) if ref.expected_window(oracle_mod, y[a:a + ref.SPAN], result_for(oracle_mod, y[a:]))["flags"] == 2)
    res4 = result_for(oracle_mod, y[a4:])
    for n in (1370, 1389, 1407, 1408):
        span = y[a4:a4 + n]
        want = ref.expected_window(oracle_mod, span, res4, literal=n == 1370)
        assert bool(want["flags"] & 4) == (n < 1408) and (n > 1370 or not want["flags"] & 2), (n, want)
        ref.assert_equal(call_ctx.retune_window(span, res4), want, n)
    # two equal maxima: one sample alone carries energy, and several candidates gather it exactly once -- the first of them wins
    m = int(res["index"]) - 65
    span = np.zeros(ref.SPAN, dtype=np.complex64)
    span[m + 64] = 3 - 4j
    s_re, s_im = ref.span_of(span, 0, 0, ref.SPAN - 1)
    e, _ = ref.energies(s_re, s_im, m)
    top = np.flatnonzero(e == e.max())
    assert len(top) >= 2 and top[0] > 0 and e.max() == F(25.0) and e[0] == 0
    want = ref.expected_window(oracle_mod, span, res, literal=True)
    assert want["t_index"] == top[0]
    ref.assert_equal(call_ctx.retune_window(span, res), want, "equal maxima")


def test_retune_window_refuses(oracle_mod, synth_mod, call_ctx):
    import rfid
    span = crafted_y(oracle_mod, synth_mod, crafted_frame(synth_mod), 0.04)[10:10 + ref.SPAN]
    res = result_for(oracle_mod, span)
    for n in (1369, 1409, 0):
        with pytest.raises(ValueError):
            call_ctx.retune_window(np.zeros(n, dtype=np.complex64), res)
    with pytest.raises(ValueError):
        call_ctx.retune_window(np.zeros((2, 1400), dtype=np.complex64), res)
    lib, h, INVALID = call_ctx._lib, call_ctx._h, rfid.capi.ERR_INVALID
    r = np.zeros(1, dtype=rfid.capi.RESULT_DTYPE)
    out = np.zeros(1, dtype=rfid.capi.RETUNE_DTYPE)
    r[0] = res
    args = lambda n=ref.SPAN, s=span.ctypes.data, rr=r.ctypes.data, o=out.ctypes.data: (h, s, n, rr, o)
    assert lib.rfid_retune_window(*args()) == rfid.capi.OK
    ref.assert_equal(out[0], ref.expected_window(oracle_mod, span, res), "accepted")
    for n in (1369, 1409, -1):
        assert lib.rfid_retune_window(*args(n=n)) == INVALID
    assert lib.rfid_retune_window(*args(s=None)) == INVALID and lib.rfid_retune_window(*args(rr=None)) == INVALID
    assert lib.rfid_retune_window(*args(o=None)) == INVALID and lib.rfid_retune_window(None, *args()[1:]) == INVALID
    for field, value in (("type", 0), ("index", 64), ("index", 80)):
        r[0] = res
        r[0][field] = value
        assert lib.rfid_retune_window(*args()) == INVALID, (field, value)
        assert "rfid_retune_window" in lib.rfid_last_error(h).decode()

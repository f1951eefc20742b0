"""The cases of the diversity stage that run on both sides, written once: tests/test_diversity_emu.py (the kernels on the wave emulator) and
tests/test_gpu_diversity.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches the
library) and `call_ctx` (the context of the per-call cases).  Pytest collects the imported functions in the importing module, resolves
their fixtures there and applies that module's marks.  Every expected record is worked out in numpy from the ORACLE alone
(tests/diversity_ref.py) and every comparison is exact, the floats by bit pattern.

The batch: six traces, M = 3, FIXED_Q = 2, tags (1, 2, 3), sigma = 0.03, t1_jitter_raw = 3, odd row stride.  Antenna m has the leak
(1 - 0.15 m) e^{j (0.7 + 1.3 m)}, h = 0.026 (1 - 0.1 m) e^{j (2.1 + 0.8 m)} and the noise seed 1000 S + m (group 0) or 1000 S + 500 + m
(group 1), S = 22.  Group 0 is 6 rounds of the session with seed 22, its third member cut behind its tenth EPC window; group 1 is 4
rounds of the session with seed 72, its second member delayed by 30 raw samples -- 6 filtered samples, more than the slack: never
present.  What is asserted of it before anything runs (on the reference alone): per group at least 3 recovered rows, at least 3 rows
read by some member, at least 10 member-rows left out, and more than one block of eight rows."""
import ctypes as C

import numpy as np
import pytest

import repair_ref
import diversity_ref as ref
from stage_backend import lay_out

__all__ = ["batch", "batch_rows", "small", "test_abi_version_is_7", "test_batch_equals_the_reference_in_both_front_end_modes",
           "test_truth_every_recovered_frame_was_sent_and_no_empty_or_collided_slot_is_recovered",
           "test_pairs_of_the_same_traces_with_two_sessions_paired", "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero",
           "test_plan_larger_than_the_batch_a_small_grid_stray_traces_and_a_new_plan", "test_overlap_each_pass_gets_its_own_records",
           "test_other_stages_results_and_statistics_are_untouched", "test_protocol_capacity_state_and_null_pointer_errors",
           "test_diversity_window_two_and_eight_members_over_all_sync_offsets", "test_diversity_window_on_crafted_spans",
           "test_diversity_window_refuses"]

SIGMA, S, M = 0.03, 22, 3
ROUNDS, SEEDS = (6, 4), (22, 72)
CUT_ROWS, DELAY_RAW = 10, 30
H = np.complex64(0.1 * np.exp(2.1j))         # the crafted spans' channel


def antennas_of(synth_mod, g, sigma=SIGMA, **kw):
    """group g's three antennas -> (Traces, the slot truth they share)"""
    m = np.arange(M)
    return synth_mod.make_antennas(leaks=list((1 - 0.15 * m) * np.exp(1j * (0.7 + 1.3 * m))),
                                   hs=list(0.026 * (1 - 0.1 * m) * np.exp(1j * (2.1 + 0.8 * m))), sigma=sigma,
                                   noise_seeds=[1000 * S + 500 * g + int(k) for k in m],
                                   n_rounds=ROUNDS[g], fixed_q=2, tag_ids=(1, 2, 3), seed=SEEDS[g], t1_jitter_raw=3, **kw)


def oracle_of(oracle_mod, host, lens, members=M, **cfg):
    """-> (oracle Results, expected rows per group, member-rows left out per group)"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return (refs,) + ref.expected_batch(oracle_mod, refs, ys, members)


def counts(rows):
    """-> (read by some, combined, recovered, lone)"""
    f = rows["flags"]
    return int((f & 1).sum()), int(((f & 5) == 0).sum()), int(((f & 2) != 0).sum()), int(((f & 4) != 0).sum())


def check_rows(ctx, want, what="", extra=3):
    """every group's row of the last batch_diversity_enqueue against the reference's, the rows behind it zero, nrows == the anchor's
    n_windows_used / 2 -> the bytes of all rows"""
    st = ctx.batch_stats()
    members = len(st) // len(want)
    blob = b""
    for g, w in enumerate(want):
        r = ctx.batch_window_diversity(g, extra=extra)
        assert int(st[g * members]["n_windows_used"]) // 2 == len(w), (what, g, int(st[g * members]["n_windows_used"]), len(w))
        assert len(r) >= len(w) and (extra > 1000 or len(r) == len(w) + extra), (what, g, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, g)
        ref.assert_equal(r[: len(w)], w, (what, g))
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_window_diversity(ctx._h, g, None, 0, C.byref(n)) in (0, -5) and n.value == len(w)
        blob += r[: len(w) + 3].tobytes()
    return blob


@pytest.fixture(scope="module")
def batch(backend, oracle_mod, synth_mod):
    groups = [antennas_of(synth_mod, g) for g in range(2)]
    samples = [t.samples for ts, _ in groups for t in ts]
    samples[4] = np.concatenate([samples[4][:DELAY_RAW], samples[4]])           # group 1's second member: the same carrier 30 samples longer
    host, lens, L, stride = lay_out(samples, odd_stride=True)
    assert stride & 1
    full = oracle_mod.run_trace(host[2, : lens[2]], oracle_mod.config(fixed_q=2))
    lens[2] = 5 * int(full.open_idx[2 * (CUT_ROWS - 1) + 1] + ref.EPC_WIN + 60)   # group 0's third member: ten EPC windows
    refs, want, left_out = oracle_of(oracle_mod, host, lens)
    for g, w in enumerate(want):                                                  # (on the reference alone, before anything runs)
        reads, combined, recovered, lone = counts(w)
        print("group %d: %d rows, %d read by some, %d combined, %d recovered, %d lone, %d member-rows left out" %
              (g, len(w), reads, combined, recovered, lone, left_out[g]))
        assert len(w) == len(groups[g][1]) == 4 * ROUNDS[g] and len(w) > 8
        assert recovered >= 3 and reads >= 3 and left_out[g] >= 10, (g, reads, combined, recovered, left_out[g])
    assert len(refs[2].dumps) // 2 == CUT_ROWS and left_out[1] == len(want[1])
    assert all(abs(int(a) - int(b)) > ref.SLACK for a, b in zip(refs[3].open_idx, refs[4].open_idx))
    return dict(host=host, lens=lens, L=L, stride=stride, refs=refs, want=want, slots=[sl for _, sl in groups], dev=backend.put(host, lens))


@pytest.fixture(scope="module")
def batch_rows(backend, batch):
    """one pass over the batch through the fused front end -> (the rows per group, their bytes, diversity ms, decode ms)"""
    import rfid
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(6, batch["L"])
        ctx.batch_plan_diversity(M)
        backend.run_pass(ctx, batch["dev"], batch["L"], batch["stride"])
        ctx.batch_diversity_enqueue()
        blob = check_rows(ctx, batch["want"], "fixture")
        assert ctx.batch_ls_report()["pieces"] == 0
        return [ctx.batch_window_diversity(g) for g in range(2)], blob, ctx.batch_diversity_ms(), ctx.batch_timing()["decode_ms"]
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def small(backend, batch):
    """group 1 of the batch (16 EPC windows, its second member never present) as a batch of its own: what the protocol cases run on"""
    h, l = np.ascontiguousarray(batch["host"][3:]), batch["lens"][3:].copy()
    w = batch["want"][1].copy()
    w["stream"] = 0
    return h, l, batch["L"], batch["stride"], [w], backend.put(h, l), batch["refs"][3:]


def test_abi_version_is_7():
    import rfid
    assert rfid.capi.load().rfid_abi_version() == 7


def test_batch_equals_the_reference_in_both_front_end_modes(backend, batch, batch_rows):
    """the batch, backend.reps passes through the fused front end and one through the long-stream front end (modes 0 and 2): the
    reference's records and the same table bytes every time"""
    import rfid
    want, L = batch["want"], batch["L"]
    rows, blob, ms, decode_ms = batch_rows
    print("%s: diversity of the batch (%d EPC windows of 2 groups of %d, %d combined): %.4f ms; decode of the same pass %.4f ms" %
          (backend.name, sum(map(len, want)), M, sum(counts(w)[1] for w in want), ms, decode_ms))
    assert ms >= 0.0
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(6, L)
        ctx.batch_plan_diversity(M)
        for mode in [0] * (backend.reps - 1) + [2]:
            ctx.batch_set_long_stream(mode)
            backend.run_pass(ctx, batch["dev"], L, batch["stride"])
            ctx.batch_diversity_enqueue()
            assert check_rows(ctx, want, mode) == blob
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        many = ctx.batch_window_diversity(1, extra=10_000)         # (more than the table has: the whole row of the group)
        ref.assert_equal(many[: len(want[1])], want[1])
        assert len(many) > len(want[1]) and not many[len(want[1]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_truth_every_recovered_frame_was_sent_and_no_empty_or_collided_slot_is_recovered(batch, batch_rows):
    """Against SlotTruth: every recovered frame is the frame of a single-responder slot, and no row of an empty or collided slot has
    bit 1.  A condition, not a measurement: the seeds are such that the reference alone meets it.  And a row read by some member
    holds that member's frame, which is the frame that was sent"""
    rows = batch_rows[0]
    recovered = 0
    for g in range(2):
        assert len(rows[g]) == len(batch["slots"][g])
        for rec, sl in zip(rows[g], batch["slots"][g]):
            single = sl.n_tags == 1 and sl.epc_valid
            if rec["flags"] & 2:
                recovered += 1
                assert single and list(ref.frame_bits(rec)) == list(sl.epc) and rec["crc_rcvd"] == rec["crc_calc"], (g, rec, sl)
                assert bin(int(rec["present"])).count("1") >= 2 and rec["reads"] == 0 and rec["h_sq"] > 0
            if not single:
                assert not rec["flags"] & 3 and sl.epc is None, (g, rec, sl)
            if rec["flags"] & 1:
                assert single and list(ref.frame_bits(rec)) == list(sl.epc) and rec["reads"] & rec["present"] == rec["reads"] != 0
                assert not rec.tobytes()[40:].strip(b"\0")
            if rec["flags"] & 4:
                assert rec["present"] == 1 and not rec.tobytes()[24:].strip(b"\0")
    assert recovered >= 6


def test_pairs_of_the_same_traces_with_two_sessions_paired(backend, oracle_mod, batch):
    """the same six traces under M = 2: three groups, the middle one pairing the cut member of one session with the anchor of the
    other -- behind the first slot their gates no longer open together, so the rows no member read are lone; and the last one's second
    member is the delayed trace.  The reference holds at least 3 lone rows in the middle group; the records are exact"""
    import rfid
    refs, want, left_out = oracle_of(oracle_mod, batch["host"], batch["lens"], members=2)
    assert len(want) == 3 and [len(w) for w in want] == [24, CUT_ROWS, 16]
    assert counts(want[1])[3] >= 3 and counts(want[2])[3] >= 3 and counts(want[0])[1] >= 3, [counts(w) for w in want]
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(6, batch["L"])
        ctx.batch_plan_diversity(2)
        backend.run_pass(ctx, batch["dev"], batch["L"], batch["stride"])
        ctx.batch_diversity_enqueue()
        check_rows(ctx, want, "pairs")
        assert [int(r["stream"]) for r in (ctx.batch_window_diversity(g)[0] for g in range(3))] == [0, 2, 4]
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, batch):
    """MAX_NUM_QUERIES = 5 reached inside the first block of eight rows: nrows == the anchor's n_windows_used / 2 = 5, the rows behind it
    zero, also when more rows are asked for than the table has.  Then in one context: rows an earlier pass had filled are zeroed
    again by a pass over shorter traces"""
    import rfid
    host, lens, L, stride, dev = batch["host"], batch["lens"], batch["L"], batch["stride"], batch["dev"]
    refs, want, _ = oracle_of(oracle_mod, host, lens, max_num_queries=5)
    assert [o.state.status for o in refs] == [1] * 6 and [len(w) for w in want] == [5, 5]
    assert sum(counts(w)[1] for w in want) >= 3
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=5)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(6, L)
        ctx.batch_plan_diversity(M)
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_diversity_enqueue()
        check_rows(ctx, want, "cut")
        check_rows(ctx, want, "cut, all rows", extra=10_000)
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(6, L)
        ctx.batch_plan_diversity(M)
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_diversity_enqueue()
        check_rows(ctx, batch["want"], "full")
        cut = lens.copy()
        for b in range(6):                                         # (4 EPC windows in group 0, 6 in group 1 but 5 in its last member)
            rows = (4, 4, 4, 6, 6, 5)[b]
            cut[b] = 5 * int(batch["refs"][b].open_idx[2 * (rows - 1) + 1] + ref.EPC_WIN + 60)
        short_refs, short, _ = oracle_of(oracle_mod, host, cut)
        assert [len(o.dumps) // 2 for o in short_refs] == [4, 4, 4, 6, 6, 5] and [len(r) for r in short] == [4, 6]
        assert short[1][5]["present"] == 1
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ctx.batch_diversity_enqueue()
        check_rows(ctx, short, "short", extra=10_000)
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_a_small_grid_stray_traces_and_a_new_plan(backend, small):
    """A plan of eight traces, one group of three of them processed: two passes give the same table bytes, the second with
    diversity_wgs = 3 (the table's blocks of rows, more than three, on three workgroups: a workgroup goes round its loop again); the
    groups not covered are not fetched; a stream count that is no multiple of M is refused with a message; a new plan drops the
    workspace"""
    import rfid
    host, lens, L, stride, want, dev, _ = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(8, L)
        ctx.batch_plan_diversity(M)
        ctx.batch_set_streams(3)
        blobs = []
        for rep in range(2):
            if rep:
                ctx.set_knob("diversity_wgs", 3)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_diversity_enqueue()
            blobs.append(check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1] and ctx.get_knob("diversity_wgs") == 3
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_diversity(ctx._h, 1, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID     # (not covered)
        assert ctx.batch_window_diversity(0, extra=10_000).shape[0] > 8 * 3      # (more blocks of rows than workgroups)
        ctx.batch_set_streams(2)
        backend.run_pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_diversity_enqueue()
        assert e.value.status == rfid.capi.ERR_INVALID and "groups of 3" in str(e.value)
        ctx.batch_plan(3, L)
        for fn in (ctx.batch_diversity_enqueue, lambda: ctx.batch_window_diversity(0), ctx.batch_diversity_ms):
            with pytest.raises(rfid.capi.RfidError) as e:
                fn()
            assert e.value.status == rfid.capi.ERR_STATE
        backend.run_pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_diversity_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_diversity" in str(e.value)
        ctx.batch_plan_diversity(M)
        ctx.batch_diversity_enqueue()                            # (the pass before the workspace: its statistics are current)
        assert check_rows(ctx, want, "planned again") == blobs[0]
    finally:
        ctx.close()


@pytest.mark.parametrize("overlap", [1, 2])
def test_overlap_each_pass_gets_its_own_records(backend, oracle_mod, small, overlap):
    """RFID_OVERLAP 1 and 2 (two result sets where the plan has them): the next pass -- the group's second and third member exchanged:
    other masks, another order of the sums -- enqueued BEFORE this pass's records are fetched leaves them this pass's, then gets its own"""
    import rfid
    host, lens, L, stride, want_a, dev_a, refs = small
    order = [0, 2, 1]
    dev_b = backend.put(np.ascontiguousarray(host[order]), lens[order].copy())
    want_b = [ref.expected_group(oracle_mod, [refs[k] for k in order], [oracle_mod.fir(host[k, : lens[k]]) for k in order])[0]]
    assert set(want_a[0]["present"]) == {5} and set(want_b[0]["present"]) == {3} and counts(want_b[0])[2] >= 3
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.set_knob("overlap", overlap)
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_diversity(M)
        for rep in range(2):
            backend.run_pass(ctx, dev_a, L, stride)
            ctx.batch_diversity_enqueue()
            backend.run_pass(ctx, dev_b, L, stride)
            ref.assert_equal(ctx.batch_window_diversity(0), want_a[0], ("a", rep))
            ctx.batch_diversity_enqueue()
            check_rows(ctx, want_b, ("b", rep))
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
    ctx.batch_lengths_enqueue()
    w, r, _ = ctx.batch_windows()
    parts = [ent, counts_, reads, off, q, rep, fine, ctx.batch_stats(), w, r]
    for b in range(n):
        parts += [ctx.batch_window_quality(b, extra=2), ctx.batch_window_repairs(b, extra=2), ctx.batch_window_fine(b, extra=2),
                  ctx.batch_window_moments(b, extra=2), ctx.batch_window_commands(b, extra=2), ctx.batch_window_retunes(b, extra=2),
                  ctx.batch_window_collisions(b, extra=2), ctx.batch_window_lengths(b, extra=2)]
    return [np.ascontiguousarray(p).tobytes() for p in parts]


@pytest.mark.parametrize("order", ["diversity-first", "diversity-last"])
def test_other_stages_results_and_statistics_are_untouched(backend, small, order):
    """inventory, tracks, quality, repair, fine, slots, commands, retune, collisions and lengths on the same pass, with the diversity
    stage enqueued before or behind them and without it: every other fetched array -- results and statistics among them -- is
    byte-identical"""
    import rfid
    host, lens, L, stride, want, dev, _ = small
    outs = []
    for diversity in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(3, L)
            ctx.batch_plan_inventory(8)
            ctx.batch_plan_tracks()
            for plan in (ctx.batch_plan_quality, ctx.batch_plan_repair, ctx.batch_plan_fine, ctx.batch_plan_slots, ctx.batch_plan_commands,
                         ctx.batch_plan_retune, ctx.batch_plan_collisions, ctx.batch_plan_lengths):
                plan()
            if diversity:
                ctx.batch_plan_diversity(M)
            backend.run_pass(ctx, dev, L, stride)
            if diversity and order == "diversity-first":
                ctx.batch_diversity_enqueue()
            outs.append(other_outputs(ctx, 3))
            if diversity and order == "diversity-last":
                ctx.batch_diversity_enqueue()
            if diversity:
                check_rows(ctx, want, order)
                assert other_outputs(ctx, 3) == outs[-1]         # (and the stage lowered nothing: the others run again behind it)
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs)), [a == b for a, b in zip(*outs)]
    assert sum(map(len, outs[0])) > 5_000


def test_protocol_capacity_state_and_null_pointer_errors(backend, small):
    import rfid
    host, lens, L, stride, want, dev, _ = small
    ctx = rfid.Context(device=0, fixed_q=2)
    ERR_STATE, ERR_CAPACITY, ERR_INVALID = rfid.capi.ERR_STATE, rfid.capi.ERR_CAPACITY, rfid.capi.ERR_INVALID

    def raises(fn, status):
        with pytest.raises(rfid.capi.RfidError) as e:
            fn()
        assert e.value.status == status, e.value

    try:
        raises(lambda: ctx.batch_plan_diversity(M), ERR_STATE)      # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        raises(ctx.batch_diversity_enqueue, ERR_STATE)              # no workspace
        for members in (1, 9, 0, -3):
            raises(lambda: ctx.batch_plan_diversity(members), ERR_INVALID)
            assert "rfid_batch_plan_diversity" in ctx._lib.rfid_last_error(ctx._h).decode()
        raises(ctx.batch_diversity_enqueue, ERR_STATE)              # (a refused plan call left none)
        ctx.batch_plan_diversity(M)
        raises(ctx.batch_diversity_enqueue, ERR_STATE)              # no pass
        raises(lambda: ctx.batch_window_diversity(0), ERR_STATE)    # nothing enqueued
        raises(ctx.batch_diversity_ms, ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_diversity(0), ERR_STATE)    # a pass, but nothing enqueued behind it
        ctx.batch_diversity_enqueue()                               # (no inventory workspace: none is needed)
        blob = check_rows(ctx, want, "no inventory")
        # the level of the other stages is neither raised ...
        ctx.batch_plan_inventory(8)                                 # (does not drop the diversity workspace)
        ctx.batch_plan_tracks()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)                 # (the diversity stage is not an inventory)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_diversity_enqueue()
        ctx.batch_tracks_enqueue()                                  # ... nor lowered: the inventory is still this pass's
        assert check_rows(ctx, want, "behind the tracks") == blob
        # a caller's array that is too small loses nothing
        row = np.zeros(len(want[0]) - 1, dtype=rfid.capi.DIVERSITY_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_window_diversity(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not row.tobytes().strip(b"\0")
        assert "EPC windows" in ctx._lib.rfid_last_error(ctx._h).decode()
        full = np.zeros(n.value, dtype=rfid.capi.DIVERSITY_DTYPE)
        assert ctx._lib.rfid_batch_get_window_diversity(ctx._h, 0, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        for g in (1, -1):                                           # (groups, not traces: three traces are one group)
            assert ctx._lib.rfid_batch_get_window_diversity(ctx._h, g, None, 0, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_diversity(ctx._h, 0, None, 0, None) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_diversity(ctx._h, 0, None, 4, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_diversity_ms(ctx._h, None) == ERR_INVALID
        assert ctx._lib.rfid_batch_plan_diversity(None, M) == ERR_INVALID and ctx._lib.rfid_batch_diversity(None) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_diversity(None, 0, None, 0, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_diversity_ms(None, C.byref(C.c_float(0))) == ERR_INVALID
        # a plan for another group size takes the place of this one
        ctx.batch_plan_diversity(2)
        raises(lambda: ctx.batch_window_diversity(0), ERR_STATE)
        raises(ctx.batch_diversity_enqueue, ERR_INVALID)            # (three traces are no pairs)
        assert "groups of 2" in ctx._lib.rfid_last_error(ctx._h).decode()
        # a new plan drops the workspace
        ctx.batch_plan(3, L)
        raises(ctx.batch_diversity_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_diversity(0), ERR_STATE)
    finally:
        ctx.close()


# ---- rfid_diversity_window on crafted, noise-free spans -------------------------------------------------------------------------
def crafted_y(oracle_mod, synth_mod, frame, h=H, lead=100):
    """the matched filter's output of one noise-free, leak-free EPC reply with the channel h, `lead` raw samples into the trace"""
    wave = np.repeat(synth_mod.fm0_levels(frame), 25)
    raw = np.zeros(5 * 1500, dtype=np.complex64)
    assert lead + len(wave) < len(raw)
    raw[lead:lead + len(wave)] = np.complex64(h) * wave
    return oracle_mod.fir(raw)


def crafted_frame(synth_mod, tag_id=0x27, seed=5):
    return synth_mod.epc_frame(synth_mod.epc_for_id(tag_id, np.random.default_rng(seed)))


def result_for(oracle_mod, span, crc_ok=None):
    """the decoder's own result for a span (the oracle's), as the library's record; crc_ok: overwritten (a noise-free span is read by
    the decoder itself: with 0 the stage takes it for a failed window)"""
    r = repair_ref.result_of_dump(oracle_mod.decode_window(np.ascontiguousarray(span), 1))
    if crc_ok is not None:
        r["crc_ok"] = crc_ok
        r["tag_id"] = -1 if not crc_ok else r["tag_id"]
    return r


def by_sync_offset(oracle_mod, synth_mod, frame):
    """the reply cut so that the decoder's sync offset takes every value 0 .. 14, each with a channel of its own -> {offset: (span,
    its result with crc_ok = 0)}"""
    import rfid
    found = {}
    for a in range(0, 40):
        h = H * np.complex64((0.5 + 0.05 * a) * np.exp(0.37j * a))
        span = crafted_y(oracle_mod, synth_mod, frame, h)[a:a + ref.EPC_WIN]
        res = result_for(oracle_mod, span)
        m = int(res["index"]) - 65
        if m in found or not res["crc_ok"] or list(rfid.unpack_bits(res["bits"], 128)) != list(frame):
            continue                                               # (the reply has left the span, or the sync is an alias)
        res["crc_ok"], res["tag_id"] = 0, -1
        found[m] = (span, res)
    assert sorted(found) == list(range(15)), sorted(found)
    return found


def test_diversity_window_two_and_eight_members_over_all_sync_offsets(oracle_mod, synth_mod, call_ctx):
    """M = 2 and M = 8, members whose sync offsets cover 0 .. 14 between them, each with its own channel: the frame that was sent,
    the record the reference's (the literal loop on each)"""
    frame = crafted_frame(synth_mod)
    found = by_sync_offset(oracle_mod, synth_mod, frame)
    for offsets in ((0, 14), tuple(range(8)), tuple(range(7, 15)), (14, 3)):
        spans = np.stack([found[m][0] for m in offsets])
        results = [found[m][1] for m in offsets]
        want = ref.expected_window(oracle_mod, spans, results, literal=True)
        got = call_ctx.diversity_window(spans, results)
        ref.assert_equal(got, want, offsets)
        assert got["flags"] == 2 and list(ref.frame_bits(got)) == list(frame) and got["present"] == (1 << len(offsets)) - 1
        assert got["reads"] == 0 and got["crc_rcvd"] == got["crc_calc"] and got["margin_min"] > 0 and got["stream"] == got["seq"] == got["start"] == 0


def test_diversity_window_on_crafted_spans(oracle_mod, synth_mod, call_ctx):
    frame, other = crafted_frame(synth_mod), crafted_frame(synth_mod, tag_id=0x31, seed=6)
    assert sum(a != b for a, b in zip(frame, other)) > 20
    span = crafted_y(oracle_mod, synth_mod, frame)[10:10 + ref.EPC_WIN]
    res = result_for(oracle_mod, span, crc_ok=0)
    # a member whose tag part is negated under the same result record: acc is exactly 0 -- no decision is positive, frame bit 0 alone is
    # set, the frame fails, and decision 0 is the weakest at margin 0
    spans = np.stack([span, -span])
    want = ref.expected_window(oracle_mod, spans, [res, res], literal=True)
    assert want["flags"] == 0 and list(want["frame"]) == [1, 0, 0, 0] and want["margin_min"] == 0 and want["weakest"] == 0
    assert want["crc_rcvd"] != want["crc_calc"] and want["h_sq"] > 0
    ref.assert_equal(call_ctx.diversity_window(spans, [res, res]), want, "negated")
    # a strong wrong member outvotes a weak right one, and the reverse: the combined frame is the strong member's
    for strong, weak, name in ((other, frame, "wrong wins"), (frame, other, "right wins")):
        s_hi = crafted_y(oracle_mod, synth_mod, strong, 3 * H)[10:10 + ref.EPC_WIN]
        s_lo = crafted_y(oracle_mod, synth_mod, weak, H * np.complex64(np.exp(1.1j)))[10:10 + ref.EPC_WIN]
        for spans in (np.stack([s_lo, s_hi]), np.stack([s_hi, s_lo])):
            results = [result_for(oracle_mod, s, crc_ok=0) for s in spans]
            want = ref.expected_window(oracle_mod, spans, results, literal=True)
            assert want["flags"] == 2 and list(ref.frame_bits(want)) == list(strong), name
            ref.assert_equal(call_ctx.diversity_window(spans, results), want, name)
    # one member whose own CRC held: bit 0, that member's frame copied, nothing combined -- the lowest such member's
    s_other = crafted_y(oracle_mod, synth_mod, other)[10:10 + ref.EPC_WIN]
    spans = np.stack([span, s_other, span])
    results = [res, result_for(oracle_mod, s_other), result_for(oracle_mod, span)]
    assert results[1]["crc_ok"] == 1 and results[2]["crc_ok"] == 1
    want = ref.expected_window(oracle_mod, spans, results)
    assert want["flags"] == 1 and want["reads"] == 6 and want["present"] == 7 and list(ref.frame_bits(want)) == list(other)
    got = call_ctx.diversity_window(spans, results)
    ref.assert_equal(got, want, "read by some")
    assert not got.tobytes()[40:].strip(b"\0")
    # all zero: no decision is positive
    zero = np.zeros((2, ref.EPC_WIN), dtype=np.complex64)
    want = ref.expected_window(oracle_mod, zero, [res, res], literal=True)
    assert want["flags"] == 0 and list(want["frame"]) == [1, 0, 0, 0]
    ref.assert_equal(call_ctx.diversity_window(zero, [res, res]), want, "zero")


def test_diversity_window_refuses(oracle_mod, synth_mod, call_ctx):
    import rfid
    span = crafted_y(oracle_mod, synth_mod, crafted_frame(synth_mod))[10:10 + ref.EPC_WIN]
    res = result_for(oracle_mod, span, crc_ok=0)
    for shape in ((1, 1370), (9, 1370), (2, 1369), (2, 1371), (1370,)):
        with pytest.raises(ValueError):
            call_ctx.diversity_window(np.zeros(shape, dtype=np.complex64), [res] * shape[0])
    with pytest.raises(ValueError):
        call_ctx.diversity_window(np.zeros((3, 1370), dtype=np.complex64), [res] * 2)
    lib, h, INVALID = call_ctx._lib, call_ctx._h, rfid.capi.ERR_INVALID
    spans = np.ascontiguousarray(np.stack([span] * 8))
    r = np.zeros(8, dtype=rfid.capi.RESULT_DTYPE)
    out = np.zeros(1, dtype=rfid.capi.DIVERSITY_DTYPE)
    r[:] = res
    args = lambda n=3, s=spans.ctypes.data, rr=r.ctypes.data, o=out.ctypes.data: (h, s, n, rr, o)
    assert lib.rfid_diversity_window(*args()) == rfid.capi.OK
    ref.assert_equal(out[0], ref.expected_window(oracle_mod, spans[:3], list(r[:3])), "accepted")
    for n in (1, 9, 0, -1):
        assert lib.rfid_diversity_window(*args(n=n)) == INVALID
        assert "rfid_diversity_window" in lib.rfid_last_error(h).decode()
    assert lib.rfid_diversity_window(*args(s=None)) == INVALID and lib.rfid_diversity_window(*args(rr=None)) == INVALID
    assert lib.rfid_diversity_window(*args(o=None)) == INVALID and lib.rfid_diversity_window(None, *args()[1:]) == INVALID
    F = np.float32
    for member in (0, 2):
        for field, value in (("type", 0), ("index", 64), ("index", 80), ("T", np.nextafter(F(4.95), F(0))), ("T", np.nextafter(F(5.05), F(9))),
                             ("T", F(0)), ("T", F(np.nan))):
            r[:] = res
            r[member][field] = value
            assert lib.rfid_diversity_window(*args()) == INVALID, (member, field, value)
            assert "rfid_diversity_window: member %d" % member in lib.rfid_last_error(h).decode()
            assert lib.rfid_diversity_window(*args(n=2)) == (INVALID if member == 0 else rfid.capi.OK)   # (a member behind the group is not looked at)
    for value in (F(4.95), F(5.05)):                               # (the ends of the decoder's own range are accepted)
        r[:] = res
        r[1]["T"] = value
        assert lib.rfid_diversity_window(*args()) == rfid.capi.OK

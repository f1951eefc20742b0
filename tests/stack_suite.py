"""The cases of the stack stage that run on both sides, written once: tests/test_stack_emu.py (the kernels on the wave emulator) and
tests/test_gpu_stack.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches the
library) and `call_ctx` (the context of the per-call cases).  Pytest collects the imported functions in the importing module, resolves
their fixtures there and applies that module's marks.  Every expected record is worked out in numpy from the ORACLE alone
(tests/stack_ref.py) and every comparison is exact, the floats by bit pattern.

The batch: four traces, FIXED_Q = 2, tags (1, 2, 3), sigma = 0.03, t1_jitter_raw = 3, h = |h| e^{j 2.1}, odd row stride: (|h|, seed,
rounds) = (0.026, 22, 6), (0.018, 72, 12), (0.015, 72, 20), (0.012, 22, 6), rho_min = 0.5.  What is asserted of it before anything runs
(on the reference alone): 18, 46, 80 and 24 failed windows; at least 8, 22, 30 and 0 combinations that pass the CRC, of at least 2, 3, 3
and 0 distinct EPCs; every combination that passes the CRC is, by the synthesiser's SlotTruth, the frame its own single-responder slot
sent -- none wrong, none from an empty or collided slot; the third trace has two blocks of failed rows, 64 + 16; the third and the
fourth have an empty decoder inventory; member_mask is symmetric."""
import ctypes as C

import numpy as np
import pytest

import inventory_ref
import stack_ref as ref
from diversity_suite import crafted_frame, crafted_y, result_for
from stage_backend import lay_out

__all__ = ["batch", "batch_rows", "small", "test_abi_version_is_7", "test_batch_equals_the_reference_in_both_front_end_modes",
           "test_truth_every_combination_that_passes_the_crc_is_the_frame_its_slot_sent",
           "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero", "test_plan_larger_than_the_batch_and_one_workgroup",
           "test_overlap_each_pass_gets_its_own_records", "test_other_stages_results_and_statistics_are_untouched",
           "test_protocol_capacity_state_and_null_pointer_errors", "test_rho_min_outside_its_range_is_refused",
           "test_rho_min_one_finds_partners_only_among_identical_sign_patterns", "test_stack_windows_on_replies_of_one_frame",
           "test_stack_windows_on_crafted_decision_values", "test_stack_windows_refuses"]

SIGMA = 0.03
SPEC = ((0.026, 22, 6), (0.018, 72, 12), (0.015, 72, 20), (0.012, 22, 6))       # |h|, seed, rounds
FAILED = (18, 46, 80, 24)
PASS_AT_LEAST, DISTINCT_AT_LEAST = (8, 22, 30, 0), (2, 3, 3, 0)
RHO = 0.5
N = len(SPEC)


def trace_of(synth_mod, b):
    a, seed, rounds = SPEC[b]
    return synth_mod.make_trace(n_rounds=rounds, fixed_q=2, tag_ids=(1, 2, 3), sigma=SIGMA, seed=seed, t1_jitter_raw=3, h=a * np.exp(2.1j))


def oracle_of(oracle_mod, host, lens, rho=RHO, **cfg):
    """-> (oracle Results, the reference's rows per trace)"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2, **cfg)) for b in range(len(lens))]
    rows = [ref.expected_rows(oracle_mod, o, oracle_mod.fir(host[b, : lens[b]]), b, rho) for b, o in enumerate(refs)]
    return refs, rows


def passed(rows):
    return rows[(rows["flags"] & ref.PASS) != 0]


def check_truth(rows, slots):
    """-> (combinations that pass the CRC, their distinct frames) of one trace, each the frame its own single-responder slot sent"""
    assert len(rows) == len(slots)
    for rec, sl in zip(rows, slots):
        if rec["flags"] & ref.PASS:
            assert sl.n_tags == 1 and sl.epc_valid and list(ref.frame_bits(rec)) == list(sl.epc), (rec, sl)
            assert rec["flags"] == (ref.FORMED | ref.PASS) and rec["n_partners"] >= 1 and rec["ordinal"] >= 0 and rec["sig_abs"] > 0
    ok = passed(rows)
    return len(ok), {bytes(np.ascontiguousarray(r["frame"])) for r in ok}


def check_rows(ctx, want, what="", extra=3):
    """every trace's row of the last batch_stack_enqueue against the reference's, the rows behind it zero, nrows == n_windows_used / 2
    -> the bytes of all rows"""
    st = ctx.batch_stats()
    blob = b""
    for b, w in enumerate(want):
        r = ctx.batch_window_stacks(b, extra=extra)
        assert int(st[b]["n_windows_used"]) // 2 == len(w), (what, b, int(st[b]["n_windows_used"]), len(w))
        assert len(r) >= len(w) and (extra > 1000 or len(r) == len(w) + extra), (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, b)
        ref.assert_equal(r[: len(w)], w, (what, b))
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_window_stacks(ctx._h, b, None, 0, C.byref(n)) in (0, -5) and n.value == len(w)
        blob += r[: len(w) + 3].tobytes()
    return blob


def stack_pass(backend, ctx, dev, L, stride, rho=RHO):
    backend.run_pass(ctx, dev, L, stride)
    ctx.batch_stack_enqueue(rho)


@pytest.fixture(scope="module")
def batch(backend, oracle_mod, synth_mod):
    traces = [trace_of(synth_mod, b) for b in range(N)]
    host, lens, L, stride = lay_out([t.samples for t in traces], odd_stride=True)
    assert stride & 1
    slots = [t.slots for t in traces]
    refs, rows = oracle_of(oracle_mod, host, lens)
    for b in range(N):                                                            # (on the reference alone, before anything runs)
        w = rows[b]
        failed = w[(w["flags"] & ref.READ) == 0]
        n_ok, frames = check_truth(w, slots[b])
        print("trace %d: %d EPC windows, %d failed, %d reads, %d combinations formed, %d pass the CRC, %d distinct EPCs" %
              (b, len(w), len(failed), len(w) - len(failed), int(((w["flags"] & ref.FORMED) != 0).sum()), n_ok, len(frames)))
        assert len(w) == 4 * SPEC[b][2] and len(failed) == FAILED[b], (b, len(w), len(failed))
        assert n_ok >= PASS_AT_LEAST[b] and len(frames) >= DISTINCT_AT_LEAST[b], (b, n_ok, len(frames))
        ref.assert_symmetric(w)
        assert all(not r.tobytes()[20:].strip(b"\0") and r["ordinal"] == -1 for r in w[(w["flags"] & ref.READ) != 0])
    assert list(rows[2]["ordinal"]) == list(range(80)) and {o // ref.BLOCK for o in rows[2]["ordinal"]} == {0, 1}      # 64 + 16
    assert any(r["ordinal"] >= 64 and r["flags"] & ref.PASS for r in rows[2]) and all(r["member_mask"] < (1 << 16) for r in rows[2][64:])
    assert len(inventory_ref.expected(refs[2].dumps, 2)) == 0 and len(inventory_ref.expected(refs[3].dumps, 3)) == 0
    assert ((rows[3]["flags"] & ref.FORMED) != 0).any()                           # (combinations that fail the CRC: reported, not accepted)
    return dict(host=host, lens=lens, L=L, stride=stride, refs=refs, rows=rows, slots=slots, dev=backend.put(host, lens))


@pytest.fixture(scope="module")
def batch_rows(backend, batch):
    """one pass over the batch through the fused front end -> (the library's rows, their bytes, stack ms, decode ms)"""
    import rfid
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(N, batch["L"])
        ctx.batch_plan_stack()
        stack_pass(backend, ctx, batch["dev"], batch["L"], batch["stride"])
        blob = check_rows(ctx, batch["rows"], "fixture")
        assert ctx.batch_ls_report()["pieces"] == 0
        return [ctx.batch_window_stacks(b) for b in range(N)], blob, ctx.batch_stack_ms(), ctx.batch_timing()["decode_ms"]
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def small(backend, batch):
    """traces 0 and 3 of the batch (24 EPC windows each; 8 combinations that pass, and 11 that are formed and fail) as a batch of its
    own: what the protocol cases run on -> (host, lens, L, stride, rows, device handle)"""
    pick = [0, 3]
    h, l = np.ascontiguousarray(batch["host"][pick]), batch["lens"][pick].copy()
    rows = [batch["rows"][b].copy() for b in pick]
    for b in range(2):
        rows[b]["stream"] = b
    L = int(l.max())
    return h, l, L, batch["stride"], rows, backend.put(h, l)


def test_abi_version_is_7():
    import rfid
    assert rfid.capi.load().rfid_abi_version() == 7


def test_batch_equals_the_reference_in_both_front_end_modes(backend, batch, batch_rows):
    """the batch, backend.reps passes through the fused front end and one through the long-stream front end (modes 0 and 2): the
    reference's records and the same table bytes every time"""
    import rfid
    L = batch["L"]
    _, blob, ms, decode_ms = batch_rows
    print("%s: stack of the batch (%d EPC windows of %d traces, %d failed): stack_ms %.4f; decode_ms of the same pass %.4f" %
          (backend.name, sum(map(len, batch["rows"])), N, sum(FAILED), ms, decode_ms))
    assert ms >= 0.0
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(N, L)
        ctx.batch_plan_stack()
        for mode in [0] * (backend.reps - 1) + [2]:
            ctx.batch_set_long_stream(mode)
            stack_pass(backend, ctx, batch["dev"], L, batch["stride"])
            assert check_rows(ctx, batch["rows"], mode) == blob
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        many = ctx.batch_window_stacks(2, extra=10_000)             # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(batch["rows"][2])], batch["rows"][2])
        assert len(many) > len(batch["rows"][2]) and not many[len(batch["rows"][2]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_truth_every_combination_that_passes_the_crc_is_the_frame_its_slot_sent(batch, batch_rows):
    """Against SlotTruth, on the records the library gave: every combination that passes the CRC is the frame its own
    single-responder slot sent; the counts are the reference's; the third trace, in which the decoder read nothing, yields all three
    tags; the masks are symmetric"""
    got = batch_rows[0]
    for b in range(N):
        n_ok, frames = check_truth(got[b], batch["slots"][b])
        assert n_ok >= PASS_AT_LEAST[b] and len(frames) >= DISTINCT_AT_LEAST[b] and n_ok == len(passed(batch["rows"][b]))
        ref.assert_symmetric(got[b])
    assert len(check_truth(got[2], batch["slots"][2])[1]) == 3 and not (got[2]["flags"] & ref.READ).any()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, small):
    """MAX_NUM_QUERIES = 9 reached inside the table: nrows == n_windows_used / 2 = 9, the rows behind it zero, also when more rows are
    asked for than the table has; the failed rows behind the cut-off are no partners of those before it.  Then in one context: rows an
    earlier pass had filled are zeroed again by a pass over shorter traces"""
    import rfid
    host, lens, L, stride, rows, dev = small
    refs, cut_rows = oracle_of(oracle_mod, host, lens, max_num_queries=9)
    assert [o.state.status for o in refs] == [1, 1] and [len(w) for w in cut_rows] == [9, 9]
    assert any(((w["flags"] & ref.FORMED) != 0).any() for w in cut_rows) and cut_rows[0].tobytes() != rows[0][:9].tobytes()
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=9)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_stack()
        stack_pass(backend, ctx, dev, L, stride)
        check_rows(ctx, cut_rows, "cut")
        check_rows(ctx, cut_rows, "cut, all rows", extra=10_000)
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_stack()
        stack_pass(backend, ctx, dev, L, stride)
        check_rows(ctx, rows, "full")
        full_refs, _ = oracle_of(oracle_mod, host, lens)
        cut = lens.copy()
        keep = (7, 3)
        for b in range(2):
            cut[b] = 5 * int(full_refs[b].open_idx[2 * (keep[b] - 1) + 1] + ref.EPC_WIN + 60)
        short_refs, short = oracle_of(oracle_mod, host, cut)
        assert [len(o.dumps) // 2 for o in short_refs] == list(keep) and [len(r) for r in short] == list(keep)
        dcut = backend.put(host, cut)
        stack_pass(backend, ctx, dcut, L, stride)
        check_rows(ctx, short, "short", extra=10_000)
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_one_workgroup(backend, small):
    """A plan of eight traces, two of them processed: two passes give the same table bytes, the second with stack_wgs = 1 (one
    workgroup walks every trace of the index kernel and every block of the block kernel); a trace not covered is not fetched; a new
    plan drops the workspace"""
    import rfid
    host, lens, L, stride, rows, dev = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(8, L)
        ctx.batch_plan_stack()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            if rep:
                ctx.set_knob("stack_wgs", 1)
            stack_pass(backend, ctx, dev, L, stride)
            blobs.append(check_rows(ctx, rows, rep))
        assert blobs[0] == blobs[1] and ctx.get_knob("stack_wgs") == 1
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_stacks(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID     # (not covered)
        ctx.batch_plan(2, L)
        for fn in (ctx.batch_stack_enqueue, lambda: ctx.batch_window_stacks(0), ctx.batch_stack_ms):
            with pytest.raises(rfid.capi.RfidError) as e:
                fn()
            assert e.value.status == rfid.capi.ERR_STATE
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_plan_stack()
        ctx.batch_stack_enqueue(RHO)                                 # (the pass before the workspace: its statistics are current)
        assert check_rows(ctx, rows, "planned again") == blobs[0]
    finally:
        ctx.close()


@pytest.mark.parametrize("overlap", [1, 2])
def test_overlap_each_pass_gets_its_own_records(backend, small, overlap):
    """RFID_OVERLAP 1 and 2 (two result sets where the plan has them): the next pass -- the two traces exchanged, so every row holds
    another trace's records -- enqueued BEFORE this pass's records are fetched leaves them this pass's, then gets its own"""
    import rfid
    host, lens, L, stride, rows_a, dev_a = small
    order = [1, 0]
    dev_b = backend.put(np.ascontiguousarray(host[order]), lens[order].copy())
    rows_b = [rows_a[k].copy() for k in order]
    for b in range(2):
        rows_b[b]["stream"] = b
    assert rows_a[0].tobytes() != rows_b[0].tobytes()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.set_knob("overlap", overlap)
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_stack()
        for rep in range(2):
            stack_pass(backend, ctx, dev_a, L, stride)
            backend.run_pass(ctx, dev_b, L, stride)
            for b in range(2):
                ref.assert_equal(ctx.batch_window_stacks(b), rows_a[b], ("a", rep, b))
            ctx.batch_stack_enqueue(RHO)
            check_rows(ctx, rows_b, ("b", rep))
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
    ctx.batch_diversity_enqueue()
    ctx.batch_match_enqueue()
    w, r, _ = ctx.batch_windows()
    parts = [ent, counts_, reads, off, q, rep, fine, ctx.batch_stats(), w, r, ctx.batch_window_diversity(0, extra=2)]
    for b in range(n):
        parts += [ctx.batch_window_quality(b, extra=2), ctx.batch_window_repairs(b, extra=2), ctx.batch_window_fine(b, extra=2),
                  ctx.batch_window_moments(b, extra=2), ctx.batch_window_commands(b, extra=2), ctx.batch_window_retunes(b, extra=2),
                  ctx.batch_window_collisions(b, extra=2), ctx.batch_window_lengths(b, extra=2), ctx.batch_window_matches(b, extra=2)]
    return [np.ascontiguousarray(p).tobytes() for p in parts]


@pytest.mark.parametrize("order", ["stack-first", "stack-last"])
def test_other_stages_results_and_statistics_are_untouched(backend, small, order):
    """inventory, tracks, quality, repair, fine, slots, commands, retune, collisions, lengths, diversity (the two traces as one pair)
    and match on the same pass, without the stack stage and with it -- enqueued before all of them or behind all of them: every other
    fetched array -- results and statistics among them -- is byte-identical"""
    import rfid
    host, lens, L, stride, rows, dev = small
    outs = []
    for stack in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_inventory(8)
            ctx.batch_plan_tracks()
            for plan in (ctx.batch_plan_quality, ctx.batch_plan_repair, ctx.batch_plan_fine, ctx.batch_plan_slots, ctx.batch_plan_commands,
                         ctx.batch_plan_retune, ctx.batch_plan_collisions, ctx.batch_plan_lengths, lambda: ctx.batch_plan_diversity(2),
                         ctx.batch_plan_match):
                plan()
            if stack:
                ctx.batch_plan_stack()
            backend.run_pass(ctx, dev, L, stride)
            if stack and order == "stack-first":
                ctx.batch_stack_enqueue(RHO)
            outs.append(other_outputs(ctx, 2))
            if stack and order == "stack-last":
                ctx.batch_stack_enqueue(RHO)
            if stack:
                check_rows(ctx, rows, order)
                assert other_outputs(ctx, 2) == outs[-1]           # (and the stage lowered nothing: the others run again behind it)
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs)), [a == b for a, b in zip(*outs)]
    assert sum(map(len, outs[0])) > 5_000


def test_protocol_capacity_state_and_null_pointer_errors(backend, small):
    import rfid
    host, lens, L, stride, rows, dev = small
    ctx = rfid.Context(device=0, fixed_q=2)
    ERR_STATE, ERR_CAPACITY, ERR_INVALID, OK = rfid.capi.ERR_STATE, rfid.capi.ERR_CAPACITY, rfid.capi.ERR_INVALID, rfid.capi.OK
    lib, h = ctx._lib, ctx._h
    last = lambda: lib.rfid_last_error(h).decode()

    def raises(fn, status, text=None):
        with pytest.raises(rfid.capi.RfidError) as e:
            fn()
        assert e.value.status == status, e.value
        assert text is None or text in str(e.value), e.value

    try:
        raises(ctx.batch_plan_stack, ERR_STATE, "rfid_batch_plan_stack: no plan")
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_stack_enqueue, ERR_STATE, "rfid_batch_plan_stack")              # no workspace
        ctx.batch_plan_stack()
        raises(ctx.batch_stack_enqueue, ERR_STATE, "no pass with statistics yet")
        raises(lambda: ctx.batch_window_stacks(0), ERR_STATE)                            # nothing enqueued
        raises(ctx.batch_stack_ms, ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_stacks(0), ERR_STATE)                            # a pass, but nothing enqueued behind it
        ctx.batch_stack_enqueue(RHO)                                                     # (no inventory workspace: none is needed)
        blob = check_rows(ctx, rows, "no inventory")
        # the level of the other stages is neither raised ...
        ctx.batch_plan_inventory(8)                                                      # (does not drop the stack workspace)
        ctx.batch_plan_tracks()
        ctx.batch_stack_enqueue(RHO)
        raises(ctx.batch_tracks_enqueue, ERR_STATE)                                      # (the stack stage is not an inventory)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_stack_enqueue(RHO)
        ctx.batch_tracks_enqueue()                                                       # ... nor lowered: the inventory is still this pass's
        assert check_rows(ctx, rows, "behind the tracks") == blob
        # a caller's array that is too small loses nothing
        row = np.zeros(len(rows[0]) - 1, dtype=rfid.capi.STACK_DTYPE)
        n = C.c_int64(0)
        rc = lib.rfid_batch_get_window_stacks(h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(rows[0]) and not row.tobytes().strip(b"\0") and "EPC windows" in last()
        full = np.zeros(n.value, dtype=rfid.capi.STACK_DTYPE)
        assert lib.rfid_batch_get_window_stacks(h, 0, full.ctypes.data, len(full), C.byref(n)) == OK
        ref.assert_equal(full, rows[0])
        for b in (2, -1):
            assert lib.rfid_batch_get_window_stacks(h, b, None, 0, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_get_window_stacks(h, 0, None, 0, None) == ERR_INVALID
        assert lib.rfid_batch_get_window_stacks(h, 0, None, 4, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_stack_ms(h, None) == ERR_INVALID
        assert lib.rfid_batch_plan_stack(None) == ERR_INVALID and lib.rfid_batch_stack(None, RHO) == ERR_INVALID
        assert lib.rfid_batch_get_window_stacks(None, 0, None, 0, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_stack_ms(None, C.byref(C.c_float(0))) == ERR_INVALID
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_stack_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_stacks(0), ERR_STATE)
    finally:
        ctx.close()


def test_rho_min_outside_its_range_is_refused(backend, small):
    """rho_min = 0, 1.5, NaN (and a negative and an infinite one) are refused with RFID_ERR_INVALID and a message, whatever the
    context's state, and a refused call leaves the table as it was; the smallest positive value and 1.0 are taken"""
    import rfid
    host, lens, L, stride, rows, dev = small
    bad = (0.0, 1.5, float("nan"), -0.5, float("inf"), float(np.nextafter(np.float32(1.0), np.float32(2.0))))
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        for rho in bad:                                              # (before any plan: the value is looked at first)
            assert ctx._lib.rfid_batch_stack(ctx._h, rho) == rfid.capi.ERR_INVALID, rho
            assert "rfid_batch_stack: rho_min" in ctx._lib.rfid_last_error(ctx._h).decode()
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_stack()
        stack_pass(backend, ctx, dev, L, stride)
        blob = check_rows(ctx, rows, "before")
        for rho in bad:
            with pytest.raises(rfid.capi.RfidError) as e:
                ctx.batch_stack_enqueue(rho)
            assert e.value.status == rfid.capi.ERR_INVALID, rho
        assert check_rows(ctx, rows, "after the refused calls") == blob
        for rho in (float(np.finfo(np.float32).smallest_subnormal), 1.0):
            ctx.batch_stack_enqueue(rho)
            ctx.batch_window_stacks(0)
    finally:
        ctx.close()


def sign_patterns_agree(y, result, rec_f, rec_g):
    """no decision of the two rows' windows has opposite signs (a zero agrees with both)"""
    from match_ref import decision_values, window_of
    r = []
    for rec in (rec_f, rec_g):
        k = int(rec["seq"])
        d = result.dumps[k]
        r.append(decision_values(*window_of(y, int(result.open_idx[k]), result.dc[k]), d["T"], int(d["index"]), d["h_est"][0], d["h_est"][1]))
    return not ((r[0] * r[1]) < 0).any()


def test_rho_min_one_finds_partners_only_among_identical_sign_patterns(backend, oracle_mod, synth_mod, small, call_ctx):
    """rho_min = 1.0: s >= a needs every product to be non-negative.  On the two noisy traces the library gives the reference's records,
    and every pair the reference calls partners has no decision of opposite signs.  On crafted replies: two replies of one frame at
    different strengths are partners, a reply of the same frame with one decision turned is not, nor is another frame's"""
    import rfid
    host, lens, L, stride, _, dev = small
    refs, rows = oracle_of(oracle_mod, host, lens, rho=1.0)
    for b, w in enumerate(rows):
        ref.assert_symmetric(w)
        y = oracle_mod.fir(host[b, : lens[b]])
        failed = w[(w["flags"] & ref.READ) == 0]
        for rec in failed[failed["n_partners"] > 0]:
            for g in ref.members_of(rec):
                assert sign_patterns_agree(y, refs[b], rec, failed[g])
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_stack()
        stack_pass(backend, ctx, dev, L, stride, rho=1.0)
        check_rows(ctx, rows, "rho_min = 1")
    finally:
        ctx.close()
    frame, other = crafted_frame(synth_mod), crafted_frame(synth_mod, tag_id=0x31, seed=6)
    span = crafted_y(oracle_mod, synth_mod, frame)[10:10 + ref.EPC_WIN]
    res = result_for(oracle_mod, span, crc_ok=0)
    turned = span.copy()
    j = 40                                                            # (decision 40: its first half-bit sample negated about the second)
    ia = int(np.float32(j) * (np.float32(2.0) * np.float32(res["T"])) + np.float32(res["index"]))
    ib = int((np.float32(2 * j) * np.float32(res["T"]) + np.float32(res["T"])) + np.float32(res["index"]))
    turned[ia] = np.complex64(2) * span[ib] - span[ia]
    s_other = crafted_y(oracle_mod, synth_mod, other)[10:10 + ref.EPC_WIN]
    spans = np.stack([span, turned, s_other, np.complex64(0.25) * span])
    results = [res, res, result_for(oracle_mod, s_other, crc_ok=0), res]
    want = ref.expected_windows(oracle_mod, spans, results, 1.0)
    assert [int(m) for m in want["member_mask"]] == [0b1001, 0b0010, 0b0100, 0b1001] and list(want["flags"]) == [6, 0, 0, 6]
    assert list(ref.frame_bits(want[0])) == list(frame)
    ref.assert_equal(call_ctx.stack_windows(spans, results, 1.0), want, "crafted, rho_min = 1")
    at_half = ref.expected_windows(oracle_mod, spans, results, 0.5)  # (at 0.5 the turned one is a partner again)
    assert [int(m) for m in at_half["member_mask"]] == [0b1011, 0b1011, 0b0100, 0b1011]
    ref.assert_equal(call_ctx.stack_windows(spans, results, 0.5), at_half, "crafted, rho_min = 0.5")


# ---- rfid_stack_windows on crafted, noise-free spans ----------------------------------------------------------------------------
def test_stack_windows_on_replies_of_one_frame(oracle_mod, synth_mod, call_ctx):
    """n = 1: nothing to combine.  Two identical windows: each the other's partner, the combination the frame that was sent, sig_abs
    twice a window's own.  64 identical windows: every mask all ones, 63 partners.  A window whose own CRC held takes no ordinal"""
    import quality_ref  # noqa: F401  (the reference's r_j are the quality stage's: tests/match_ref.py asserts it on every trace)
    frame = crafted_frame(synth_mod)
    span = crafted_y(oracle_mod, synth_mod, frame)[10:10 + ref.EPC_WIN]
    res = result_for(oracle_mod, span, crc_ok=0)
    check = lambda s, r, what, rho=RHO: (ref.assert_equal(call_ctx.stack_windows(s, r, rho), ref.expected_windows(oracle_mod, s, r, rho), what),
                                         call_ctx.stack_windows(s, r, rho))[1]
    got = check(span[None], [res], "n = 1")
    assert got[0]["flags"] == 0 and got[0]["ordinal"] == 0 and got[0]["member_mask"] == 1 and not got[0].tobytes()[32:].strip(b"\0")
    got = check(np.stack([span, span]), [res, res], "two identical")
    assert list(got["flags"]) == [6, 6] and list(got["member_mask"]) == [3, 3] and list(got["n_partners"]) == [1, 1]
    assert got[0].tobytes()[24:] == got[1].tobytes()[24:] and list(ref.frame_bits(got[0])) == list(frame) and got[0]["margin_min"] > 0
    assert list(got["ordinal"]) == [0, 1] and not got["stream"].any() and not got["seq"].any() and not got["start"].any()
    got = check(np.stack([span] * 64), [res] * 64, "64 identical")
    assert (got["member_mask"] == np.uint64(2 ** 64 - 1)).all() and (got["n_partners"] == 63).all() and (got["flags"] == 6).all()
    assert list(got["ordinal"]) == list(range(64)) and all(list(ref.frame_bits(r)) == list(frame) for r in got[[0, 63]])
    # a read among them: bit 0, ordinal -1, nothing behind; the others' ordinals skip it
    read = result_for(oracle_mod, span)
    assert read["crc_ok"] == 1
    got = check(np.stack([span, span, span]), [res, read, res], "a read between two")
    assert list(got["flags"]) == [6, 1, 6] and list(got["ordinal"]) == [0, -1, 1] and list(got["member_mask"]) == [3, 0, 3]
    assert not got[1].tobytes()[20:].strip(b"\0")
    got = check(np.stack([span, span]), [read, read], "reads only")
    assert list(got["flags"]) == [1, 1]


def crafted_r(r):
    """-> (a DC-free span, a result record) whose decision values are exactly r: T = 5, index = 65, h = 1 -- decision j is the real part
    of sample 10 j + 65 minus that of sample 10 j + 70, which stays 0"""
    import rfid
    span = np.zeros(ref.EPC_WIN, dtype=np.complex64)
    span[10 * np.arange(128) + 65] = np.asarray(r, dtype=np.float32)
    res = np.zeros(1, dtype=rfid.capi.RESULT_DTYPE)[0]
    res["type"], res["index"], res["T"], res["h_re"], res["h_im"], res["n_bits"], res["tag_id"] = 1, 65, 5.0, 1.0, 0.0, 128, -1
    return span, res


def test_stack_windows_on_crafted_decision_values(oracle_mod, synth_mod, call_ctx):
    """decision values set one by one (powers of two: every sum is exact).  An exact tie s == rho_min * a is a partner; one step
    below it is not.  An all-zero window has s = 0 and is nobody's partner.  Members whose R_j cancels to zero: the decision is
    `not positive`, as the decoder's result > 0 has it"""
    from match_ref import decision_values, window_of
    frame = crafted_frame(synth_mod)
    c = np.where(np.bitwise_xor.accumulate(np.asarray(frame, dtype=np.uint8)) ^ 1, 1.0, -1.0).astype(np.float32)     # the frame's sign pattern
    sp, rs = crafted_r(c)
    assert decision_values(*window_of(sp, 0, 0), rs["T"], 65, rs["h_re"], rs["h_im"]).tobytes() == c.tobytes()
    check = lambda spans, rho, what: (ref.assert_equal(call_ctx.stack_windows(spans, [rs] * len(spans), rho),
                                                       ref.expected_windows(oracle_mod, spans, [rs] * len(spans), rho), what),
                                      call_ctx.stack_windows(spans, [rs] * len(spans), rho))[1]
    # ---- the tie: 96 decisions agree, 32 are opposed, all products of magnitude 2: s = 128, a = 256, rho_min * a = 128 ----
    opposed = c.copy()
    opposed[5::4] *= -1                                              # (j = 5, 9, ..., 125: 31) ...
    opposed[0] *= -1                                                 # ... and j = 0: 32
    assert int((opposed != c).sum()) == 32
    spans = np.stack([crafted_r(2 * c)[0], crafted_r(opposed)[0]])
    got = check(spans, 0.5, "tie")
    assert list(got["member_mask"]) == [3, 3] and list(got["flags"] & 2) == [2, 2]
    # R = 2 c + opposed: 3 c or c -- the signs are c's, the frame is the sent one and its CRC holds
    assert list(got["flags"]) == [6, 6] and list(ref.frame_bits(got[0])) == list(frame) and got[0]["margin_min"] == 1 and got[0]["weakest"] == 0
    assert got[0]["sig_abs"] == 96 * 3 + 32 * 1
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    got = check(spans, above, "just above the tie")
    assert list(got["member_mask"]) == [1, 2] and list(got["flags"]) == [0, 0]
    one_more = opposed.copy()
    one_more[1] *= -1                                                # 33 opposed: s = 124 < 128
    got = check(np.stack([spans[0], crafted_r(one_more)[0]]), 0.5, "one below the tie")
    assert list(got["member_mask"]) == [1, 2]
    # ---- an all-zero window between two partners ----
    zero = np.zeros(ref.EPC_WIN, dtype=np.complex64)
    got = check(np.stack([sp, zero, crafted_r(4 * c)[0]]), 0.5, "zero")
    assert list(got["member_mask"]) == [0b101, 0b010, 0b101] and list(got["flags"]) == [6, 0, 6] and got[0]["sig_abs"] == 5 * 128
    got = check(np.stack([zero, zero]), 0.5, "zeros only")
    assert list(got["member_mask"]) == [1, 2] and list(got["flags"]) == [0, 0]
    # ---- R_j cancels to zero on j = 7, 64 and 127: not positive ----
    cancel = c.copy()
    cancel[[7, 64, 127]] *= -1
    got = check(np.stack([sp, crafted_r(cancel)[0]]), 0.5, "cancel")
    R = c + cancel
    cur = R > 0
    bits = (cur != np.concatenate([[True], cur[:-1]])).astype(np.uint8)
    assert list(got["flags"] & 2) == [2, 2] and got[0]["margin_min"] == 0 and got[0]["weakest"] == 7 and got[0]["sig_abs"] == 2 * 125
    assert list(ref.frame_bits(got[0])) == list(bits) and (list(bits) != list(frame)) and not (c[[7, 64, 127]] < 0).all()
    # three members, the anchor in its place: the sum runs in ascending ordinal whichever row asks
    big = np.float32(2 ** 24)
    a, b, d = c * big, c.copy(), c.copy()                            # (big + 1) + 1 = big, 1 + 1 + big = big + 2: the order shows
    for order in ((a, b, d), (b, d, a), (b, a, d)):
        got = check(np.stack([crafted_r(v)[0] for v in order]), 0.5, "order")
        assert list(got["member_mask"]) == [7, 7, 7] and len({q.tobytes()[24:] for q in got}) == 1
    assert check(np.stack([crafted_r(v)[0] for v in (a, b, d)]), 0.5, "order")[0]["sig_abs"] != \
        check(np.stack([crafted_r(v)[0] for v in (b, d, a)]), 0.5, "order")[0]["sig_abs"]


def test_stack_windows_refuses(oracle_mod, synth_mod, call_ctx):
    import rfid
    frame = crafted_frame(synth_mod)
    span = np.ascontiguousarray(crafted_y(oracle_mod, synth_mod, frame)[10:10 + ref.EPC_WIN])
    res = result_for(oracle_mod, span, crc_ok=0)
    for shape in ((0, 1370), (65, 1370), (2, 1369), (2, 1371), (1370,)):
        with pytest.raises(ValueError):
            call_ctx.stack_windows(np.zeros(shape, dtype=np.complex64), [res] * shape[0])
    with pytest.raises(ValueError):
        call_ctx.stack_windows(np.zeros((3, 1370), dtype=np.complex64), [res] * 2)
    lib, h, INVALID = call_ctx._lib, call_ctx._h, rfid.capi.ERR_INVALID
    spans = np.ascontiguousarray(np.stack([span] * 65))
    r = np.zeros(65, dtype=rfid.capi.RESULT_DTYPE)
    out = np.zeros(65, dtype=rfid.capi.STACK_DTYPE)
    r[:] = res
    args = lambda n=3, s=spans.ctypes.data, rr=r.ctypes.data, rho=RHO, o=out.ctypes.data: (h, s, rr, n, rho, o)
    assert lib.rfid_stack_windows(*args()) == rfid.capi.OK
    ref.assert_equal(out[:3], ref.expected_windows(oracle_mod, spans[:3], list(r[:3])), "accepted")
    assert not out[3:].tobytes().strip(b"\0")
    for n in (0, -1, 65):
        assert lib.rfid_stack_windows(*args(n=n)) == INVALID and "rfid_stack_windows" in lib.rfid_last_error(h).decode()
    assert lib.rfid_stack_windows(*args(n=64)) == rfid.capi.OK
    for rho in (0.0, 1.5, float("nan")):
        assert lib.rfid_stack_windows(*args(rho=rho)) == INVALID and "rho_min" in lib.rfid_last_error(h).decode()
    for kw in (dict(s=None), dict(rr=None), dict(o=None)):
        assert lib.rfid_stack_windows(*args(**kw)) == INVALID
    assert lib.rfid_stack_windows(None, *args()[1:]) == INVALID
    F = np.float32
    for member in (0, 2):
        for field, value in (("type", 0), ("index", 64), ("index", 80), ("T", np.nextafter(F(4.95), F(0))), ("T", np.nextafter(F(5.05), F(9))),
                             ("T", F(0)), ("T", F(np.nan))):
            r[:] = res
            r[member][field] = value
            assert lib.rfid_stack_windows(*args()) == INVALID, (member, field, value)
            assert "rfid_stack_windows: window %d" % member in lib.rfid_last_error(h).decode()
            assert lib.rfid_stack_windows(*args(n=2)) == (INVALID if member == 0 else rfid.capi.OK)   # (a window behind the n given is not looked at)
    for value in (F(4.95), F(5.05)):                               # (the ends of the decoder's own range are accepted)
        r[:] = res
        r[1]["T"] = value
        assert lib.rfid_stack_windows(*args()) == rfid.capi.OK

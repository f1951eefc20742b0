"""The cases of the collisions stage that run on both sides, written once: tests/test_collide_emu.py (the kernels on the wave emulator)
and tests/test_gpu_collide.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches
the library) and `call_ctx` (the context of the per-call cases).  Pytest collects the imported functions in the importing module,
resolves their fixtures there and applies that module's marks.  Every expected record is worked out in numpy from the ORACLE alone
(tests/collide_ref.py) and every comparison is exact.

The ragged batch: four traces of 6, 5, 4 and 3 rounds, sigma = 0.03, t1_jitter_raw = 3, no link-frequency offsets, odd row stride --
FIXED_Q = 1 with three tags, FIXED_Q = 2 with four, FIXED_Q = 0 with one (no collision at all) and FIXED_Q = 1 with four.  The
reader's own FIXED_Q (the context's and the oracle's: 2 for all four) only counts slots; what was on the air is the synthesiser's.
What is asserted of the batch before anything runs (on the reference alone) is listed at the `ragged` fixture."""
import ctypes as C

import numpy as np
import pytest

import collide_ref as ref
from stage_backend import lay_out

__all__ = ["ragged", "ragged_rows", "small", "test_collisions_abi_version_is_7",
           "test_ragged_batch_equals_the_reference_in_every_front_end_mode", "test_truth_both_handles_of_every_two_tag_slot",
           "test_row_counts_at_the_tails_of_a_wave_and_of_a_block_on_small_grids",
           "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero", "test_plan_larger_than_the_batch_and_a_new_plan",
           "test_overlap_each_pass_gets_its_own_records", "test_other_stages_results_and_statistics_are_untouched",
           "test_protocol_capacity_and_state_errors", "test_collisions_of_crafted_windows", "test_collisions_of_all_sync_offsets",
           "test_collisions_of_refuses"]

SIGMA = 0.03
SPEC = ((6, 1, (1, 2, 3)), (5, 2, (1, 2, 3, 4)), (4, 0, (1,)), (3, 1, (1, 2, 3, 4)))     # rounds, FIXED_Q on the air, tags
SEED = 40                                    # trace b: seed 40 + b (chosen so that collide_ref alone meets the fixture's conditions)
CTX_Q = 2
WIN = ref.WIN


def trace_of(synth_mod, b, **kw):
    rounds, q, tags = SPEC[b]
    return synth_mod.make_trace(n_rounds=rounds, fixed_q=q, tag_ids=tags, seed=SEED + b, sigma=SIGMA, t1_jitter_raw=3, **kw)


def oracle_of(oracle_mod, host, lens, **cfg):
    """-> (oracle Results, expected collision rows per trace)"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=CTX_Q, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ref.expected_batch(oracle_mod, refs, ys)


def check_rows(ctx, want, what="", extra=3):
    """every trace's row of the last batch_collisions_enqueue against the reference's, the rows behind it zero,
    nrows == (n_windows_used + 1) // 2 -> the bytes of all rows"""
    st = ctx.batch_stats()
    blob = b""
    for b, w in enumerate(want):
        r = ctx.batch_window_collisions(b, extra=extra)
        assert (int(st[b]["n_windows_used"]) + 1) // 2 == len(w), (what, b, int(st[b]["n_windows_used"]), len(w))
        assert len(r) >= len(w) and (extra > 1000 or len(r) == len(w) + extra), (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, b)
        ref.assert_equal(r[: len(w)], w, (what, b))
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_window_collisions(ctx._h, b, None, 0, C.byref(n)) in (0, -5) and n.value == len(w)
        blob += r[: len(w) + 3].tobytes()
    return blob


@pytest.fixture(scope="module")
def ragged(backend, oracle_mod, synth_mod):
    """On the reference alone, before anything runs: the batch holds at least 8 two-tag slots and at least 2 with three or more tags;
    collide_ref resolves every two-tag slot ({rn16_a, rn16_b} is the pair that was sent); the decoder's own RN16 is one of the pair
    in fewer than all of them; the largest fit of the single and two-tag slots lies below the smallest fit of the slots with three or
    more tags; in every single-tag slot rn16_a or rn16_b is the handle that was sent"""
    ts = [trace_of(synth_mod, b) for b in range(4)]
    host, lens, L, stride = lay_out([t.samples for t in ts], odd_stride=True)
    refs, want = oracle_of(oracle_mod, host, lens)
    truth = [ref.sent(t.plan.slots) for t in ts]
    assert stride & 1
    two = three = captured = 0
    low, high = [], []
    for b, (w, tr) in enumerate(zip(want, truth)):
        assert len(w) == len(tr) == SPEC[b][0] << SPEC[b][1]
        for rec, (n_tags, handles), f in zip(w, tr, ref.fit(w)):
            if n_tags == 2:
                two += 1
                assert ref.pair(rec) == set(handles) and len(set(handles)) == 2, (b, rec, handles)
                captured += bool(rec["flags"] & 3)
            if n_tags == 1:
                assert handles[0] in ref.pair(rec), (b, rec, handles)
            if n_tags in (1, 2):
                low.append(f)
            if n_tags >= 3:
                three += 1
                high.append(f)
    assert two >= 8 and three >= 2 and captured < two and max(low) < min(high), (two, three, captured, max(low), min(high))
    assert not any(n for n, _ in truth[2] if n != 1)                  # (the third trace: no collision at all)
    return host, lens, L, stride, refs, want, truth, backend.put(host, lens)


@pytest.fixture(scope="module")
def ragged_rows(backend, ragged):
    """one pass over the ragged batch through the fused front end -> (the rows per trace, their bytes, collisions ms, decode ms)"""
    import rfid
    host, lens, L, stride, refs, want, truth, dev = ragged
    ctx = rfid.Context(device=0, fixed_q=CTX_Q)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(4, L)
        ctx.batch_plan_collisions()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_collisions_enqueue()
        blob = check_rows(ctx, want, "fixture")
        assert ctx.batch_ls_report()["pieces"] == 0
        rows = [ctx.batch_window_collisions(b) for b in range(4)]
        return rows, blob, ctx.batch_collisions_ms(), ctx.batch_timing()["decode_ms"]
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def small(backend, ragged):
    """the second and the fourth trace of the ragged batch (20 and 6 RN16 windows) as a batch of their own: what the protocol cases
    run on"""
    host, lens, L, stride, refs, want, truth, _ = ragged
    pick = [1, 3]
    w = [want[k].copy() for k in pick]
    for b, r in enumerate(w):
        r["stream"] = b
    h, l = np.ascontiguousarray(host[pick]), lens[pick].copy()
    return h, l, L, stride, [refs[k] for k in pick], w, backend.put(h, l)


def test_collisions_abi_version_is_7():
    import rfid
    lib = rfid.capi.load()
    assert lib.rfid_abi_version() == 7 and rfid.capi.COLLISION_DTYPE.itemsize == 64
    assert all(hasattr(lib, n) for n in ("rfid_batch_plan_collisions", "rfid_batch_collisions", "rfid_batch_get_window_collisions",
                                         "rfid_batch_collisions_ms", "rfid_collisions_of"))


def test_ragged_batch_equals_the_reference_in_every_front_end_mode(backend, ragged, ragged_rows):
    """the ragged batch, backend.reps passes with batch_set_long_stream(0), then one each with (1) -- on the device -- and (2): the
    reference's records and the same table bytes every time"""
    import rfid
    host, lens, L, stride, refs, want, truth, dev = ragged
    rows, blob, ms, decode_ms = ragged_rows
    print("%s: collisions of the ragged batch (%d RN16 windows): %.4f ms; decode of the same pass %.4f ms" %
          (backend.name, sum(map(len, want)), ms, decode_ms))
    assert ms >= 0.0
    ctx = rfid.Context(device=0, fixed_q=CTX_Q)
    try:
        ctx.batch_plan(4, L)
        ctx.batch_plan_collisions()
        # (mode 1, "automatic", sizes its choice by the device: on the wave emulator its pass over this batch does not come to an
        # end within minutes, with or without this stage, so that side runs the modes tests/retune_suite.py runs)
        for mode in [0] * (backend.reps - 1) + ([2] if backend.name == "emulator" else [1, 2]):
            ctx.batch_set_long_stream(mode)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_collisions_enqueue()
            assert check_rows(ctx, want, mode) == blob
            rep = ctx.batch_ls_report()
            assert mode == 1 or ((rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0), rep
        many = ctx.batch_window_collisions(3, extra=10_000)       # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(want[3])], want[3])
        assert len(many) > len(want[3]) and not many[len(want[3]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_truth_both_handles_of_every_two_tag_slot(ragged, ragged_rows):
    """Against the slot table of the synthesiser: the rows that came back name both handles of every two-tag slot and the handle of
    every single-tag slot.  A condition, not a measurement: the seeds are such that the reference alone meets it"""
    host, lens, L, stride, refs, want, truth, _ = ragged
    rows = ragged_rows[0]
    two = 0
    for b in range(4):
        assert len(rows[b]) == len(truth[b])
        for rec, (n_tags, handles) in zip(rows[b], truth[b]):
            if n_tags == 2:
                two += 1
                assert ref.pair(rec) == set(handles) and rec["n_diff"] > 0 and not rec["flags"] & 4, (b, rec, handles)
            if n_tags == 1:
                assert handles[0] in ref.pair(rec), (b, rec, handles)
    assert two >= 8


# ---- the shapes at which the kernel can go wrong -----------------------------------------------------------------------------------
ROW_COUNTS = (17, 1, 3, 4, 5, 17)            # the tails of a wave's four windows and of a block's sixteen rows; two traces of two blocks


def test_row_counts_at_the_tails_of_a_wave_and_of_a_block_on_small_grids(backend, oracle_mod, synth_mod):
    """Six traces cut behind their 17th, 1st, 3rd, 4th, 5th and 17th RN16 window (the last RN16 without its EPC window: n_windows_used
    is odd): one row more than a block in two traces, a full step, one window more and one less.  With the default grid, with
    collide_wgs = 1 and with 2 (fewer workgroups than blocks: a workgroup goes round its loop again, across traces): the reference's
    records and the same bytes"""
    import rfid
    ts = [synth_mod.make_trace(n_rounds=(n + 1) // 2 + 1, fixed_q=1, tag_ids=(1, 2, 3), seed=60 + b, sigma=SIGMA, t1_jitter_raw=3)
          for b, n in enumerate(ROW_COUNTS)]
    host, lens, L, stride = lay_out([t.samples for t in ts], odd_stride=True)
    full = [oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=CTX_Q)) for t in ts]
    for b, n in enumerate(ROW_COUNTS):
        lens[b] = 5 * int(full[b].open_idx[2 * (n - 1)] + WIN + 60)
    refs, want = oracle_of(oracle_mod, host, lens)
    assert [len(w) for w in want] == list(ROW_COUNTS) and all(o.n_windows == 2 * n - 1 for o, n in zip(refs, ROW_COUNTS))
    assert sum(int((w["n_diff"] > 0).sum()) for w in want) >= 20
    L = int(lens.max())
    dev = backend.put(host, lens)
    ctx = rfid.Context(device=0, fixed_q=CTX_Q)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(len(ts), L)
        ctx.batch_plan_collisions()
        blobs = []
        for wgs in (0, 1, 2):
            ctx.set_knob("collide_wgs", wgs)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_collisions_enqueue()
            blobs.append(check_rows(ctx, want, wgs))
        assert blobs[0] == blobs[1] == blobs[2] and ctx.get_knob("collide_wgs") == 2
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, ragged):
    """MAX_NUM_QUERIES = 3 reached inside the first step of every trace: nrows == (n_windows_used + 1) // 2, the rows behind it
    zero, also when more rows are asked for than the table has.  Then in one context: rows an earlier pass had filled are zeroed
    again"""
    import rfid
    host, lens, L, stride, full_refs, full_want, truth, dev = ragged
    refs, want = oracle_of(oracle_mod, host, lens, max_num_queries=3)
    assert [o.state.status for o in refs] == [1, 1, 1, 1] and [len(w) for w in want] == [3, 3, 3, 3]
    assert all(len(w) < len(f) for w, f in zip(want, full_want))
    ctx = rfid.Context(device=0, fixed_q=CTX_Q, max_num_queries=3)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(4, L)
        ctx.batch_plan_collisions()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_collisions_enqueue()
        check_rows(ctx, want, "cut")
        check_rows(ctx, want, "cut, all rows", extra=10_000)
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=CTX_Q)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(4, L)
        ctx.batch_plan_collisions()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_collisions_enqueue()
        check_rows(ctx, full_want, "full")
        cut = lens.copy()
        for b in range(4):
            cut[b] = 5 * int(full_refs[b].open_idx[2 * (1 + b)] + WIN + 60)           # (2, 3, 4 and 5 RN16 windows)
        short_refs, short = oracle_of(oracle_mod, host, cut)
        assert [len(r) for r in short] == [2, 3, 4, 5]
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ctx.batch_collisions_enqueue()
        check_rows(ctx, short, "short", extra=10_000)
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_a_new_plan(backend, small):
    """A plan of five traces, two of them processed: two passes give the same table bytes; the traces not covered are not fetched; a new
    plan drops the workspace"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    ctx = rfid.Context(device=0, fixed_q=CTX_Q)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(5, L)
        ctx.batch_plan_collisions()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_collisions_enqueue()
            blobs.append(check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1]
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_collisions(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID     # (not covered)
        ctx.batch_plan(2, L)
        for fn in (ctx.batch_collisions_enqueue, lambda: ctx.batch_window_collisions(0), ctx.batch_collisions_ms):
            with pytest.raises(rfid.capi.RfidError) as e:
                fn()
            assert e.value.status == rfid.capi.ERR_STATE
        backend.run_pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_collisions_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_collisions" in str(e.value)
        ctx.batch_plan_collisions()
        ctx.batch_collisions_enqueue()                           # (the pass before the workspace: its statistics are current)
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

    ctx = rfid.Context(device=0, fixed_q=CTX_Q)
    try:
        ctx.set_knob("overlap", overlap)
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_collisions()
        for rep in range(2):
            backend.run_pass(ctx, dev_a, L, stride)
            ctx.batch_collisions_enqueue()
            backend.run_pass(ctx, dev_b, L, stride)
            for b, w in enumerate(stamped((0, 1))):
                ref.assert_equal(ctx.batch_window_collisions(b), w, ("a", rep, b))
            ctx.batch_collisions_enqueue()
            check_rows(ctx, stamped((1, 0)), ("b", rep))
    finally:
        ctx.close()


def other_outputs(ctx, n):
    """everything else a pass and its stages report, as bytes (the other stages of the last pass are enqueued here)"""
    ctx.batch_slots_enqueue()
    ctx.batch_commands_enqueue()
    ctx.batch_retune_enqueue()
    w, r, _ = ctx.batch_windows()
    parts = [ctx.batch_stats(), w, r]
    for b in range(n):
        parts += [ctx.batch_window_moments(b, extra=2), ctx.batch_window_commands(b, extra=2), ctx.batch_window_retunes(b, extra=2)]
    return [np.ascontiguousarray(p).tobytes() for p in parts]


@pytest.mark.parametrize("order", ["collisions-first", "collisions-last"])
def test_other_stages_results_and_statistics_are_untouched(backend, small, order):
    """slots, commands and retune on the same pass, with the collisions stage enqueued before or behind them and without it: windows,
    results, statistics and the moments, commands and retune rows are byte-identical"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    outs = []
    for collide in (False, True):
        ctx = rfid.Context(device=0, fixed_q=CTX_Q)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            for plan in (ctx.batch_plan_slots, ctx.batch_plan_commands, ctx.batch_plan_retune):
                plan()
            if collide:
                ctx.batch_plan_collisions()
            backend.run_pass(ctx, dev, L, stride)
            if collide and order == "collisions-first":
                ctx.batch_collisions_enqueue()
            outs.append(other_outputs(ctx, 2))
            if collide and order == "collisions-last":
                ctx.batch_collisions_enqueue()
            if collide:
                check_rows(ctx, want, order)
                assert other_outputs(ctx, 2) == outs[-1]         # (and the stage lowered nothing: the others run again behind it)
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs)), [a == b for a, b in zip(*outs)]
    assert sum(map(len, outs[0])) > 5_000


def test_protocol_capacity_and_state_errors(backend, small):
    import rfid
    host, lens, L, stride, refs, want, dev = small
    ctx = rfid.Context(device=0, fixed_q=CTX_Q)
    ERR_STATE, ERR_CAPACITY, ERR_INVALID = rfid.capi.ERR_STATE, rfid.capi.ERR_CAPACITY, rfid.capi.ERR_INVALID

    def raises(fn, status):
        with pytest.raises(rfid.capi.RfidError) as e:
            fn()
        assert e.value.status == status, e.value

    try:
        raises(ctx.batch_plan_collisions, ERR_STATE)              # no plan
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_collisions_enqueue, ERR_STATE)           # no workspace
        ctx.batch_plan_collisions()
        raises(ctx.batch_collisions_enqueue, ERR_STATE)           # no pass
        raises(lambda: ctx.batch_window_collisions(0), ERR_STATE)  # nothing enqueued
        raises(ctx.batch_collisions_ms, ERR_STATE)
        backend.run_pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_collisions(0), ERR_STATE)  # a pass, but nothing enqueued behind it
        ctx.batch_collisions_enqueue()                            # (no inventory workspace: none is needed)
        blob = check_rows(ctx, want, "no inventory")
        # the level of the other stages is neither raised ...
        ctx.batch_plan_inventory(8)                               # (does not drop the collisions workspace)
        ctx.batch_plan_tracks()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)               # (the collisions stage is not an inventory)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_collisions_enqueue()
        ctx.batch_tracks_enqueue()                                # ... nor lowered: the inventory is still this pass's
        assert check_rows(ctx, want, "behind the tracks") == blob
        # a caller's array that is too small loses nothing
        row = np.zeros(len(want[0]) - 1, dtype=rfid.capi.COLLISION_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_window_collisions(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not row.tobytes().strip(b"\0")
        assert "RN16 windows" in ctx._lib.rfid_last_error(ctx._h).decode()
        full = np.zeros(n.value, dtype=rfid.capi.COLLISION_DTYPE)
        assert ctx._lib.rfid_batch_get_window_collisions(ctx._h, 0, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        for s in (2, -1):
            assert ctx._lib.rfid_batch_get_window_collisions(ctx._h, s, None, 0, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_collisions(ctx._h, 0, None, 0, None) == ERR_INVALID
        assert ctx._lib.rfid_batch_get_window_collisions(ctx._h, 0, None, 4, C.byref(n)) == ERR_INVALID
        assert ctx._lib.rfid_batch_collisions_ms(ctx._h, None) == ERR_INVALID
        for fn in ("rfid_batch_plan_collisions", "rfid_batch_collisions"):
            assert getattr(ctx._lib, fn)(None) == ERR_INVALID
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_collisions_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_collisions(0), ERR_STATE)
    finally:
        ctx.close()


# ---- rfid_collisions_of on crafted windows -----------------------------------------------------------------------------------------
def crafted(d, hs, m=7, bits=0):
    """one DC-free RN16 window whose decisions are exactly d (16 complex values: z_2j = d_j, z_2j+1 = 0) at sync offset m, and the
    result record a decoder with channel hs and the 16 bits `bits` (the first decided in bit 0) would hand over"""
    import rfid
    w = np.zeros(WIN, dtype=np.complex64)
    w[m + 65 + 10 * np.arange(16)] = np.asarray(d, dtype=np.complex64)
    r = np.zeros(1, dtype=rfid.capi.RESULT_DTYPE)[0]
    r["type"], r["index"], r["h_re"], r["h_im"], r["n_bits"], r["tag_id"] = 0, m + 65, np.float32(hs.real), np.float32(hs.imag), 16, -1
    r["bits"][0] = bits
    return w, r


def chain(handle):
    """the signs (+1 / -1) of the 16 decisions of a reply whose handle is `handle` (bit 15 first): sign_j = sign_j-1 unless bit_j"""
    s, out = 1, []
    for j in range(16):
        if (handle >> (15 - j)) & 1:
            s = -s
        out.append(s)
    return np.array(out)


def two_tags(h1, h2, a, b):
    return chain(a) * np.complex64(h1) + chain(b) * np.complex64(h2)


def crafted_cases():
    """-> {name: (window, result)}; what each must show is asserted on the reference's record in the test"""
    one = np.ones(16)
    cases = {}
    cases["all equal"] = crafted(one * (0.25 + 0.5j), 0.25 + 0.5j)
    cases["all members"] = crafted(chain(0x5A3C) * (0.5 - 0.25j), 1 + 1j)
    d = np.where(np.arange(16) % 2 == 0, chain(0x0F0F) * (0.5 + 0j), chain(0x3333) * 0.5j)
    cases["equal strength"] = crafted(d, 0.5 + 0j)
    d = np.where(np.arange(16) % 2 == 0, chain(0x0F0F) * (1 + 0j), chain(0x3333) * (-0.5 + 0j))
    cases["weaker first"] = crafted(d, 1 + 0j)
    cases["stronger first"] = crafted(np.where(np.arange(16) % 2 == 0, d, -d), 1 + 0j)
    d = one * (1 + 0j)
    d[3], d[7] = 1 + 1j, 1 - 1j
    cases["two farthest"] = crafted(d, 1 + 0j)
    d = two_tags(0.5 + 0.25j, -0.25 + 0.5j, 0xBEEF, 0x1234)
    d[5] = 0
    cases["equidistant"] = crafted(d, (0.5 + 0.25j) + (-0.25 + 0.5j), bits=0x1234)
    cases["all zero"] = crafted(np.zeros(16), 0j)
    cases["all zero, a channel"] = crafted(np.zeros(16), 0.1 - 0.2j)
    d = np.zeros(16, dtype=np.complex64)
    d.real[:] = -0.0
    d.imag[:] = -0.0
    cases["minus zero"] = crafted(d, complex(-0.0, 0.25))
    d = two_tags(0.5 + 0.25j, -0.25 + 0.5j, 0xBEEF, 0x1234)
    d.real[0] = -0.0
    cases["minus zero first term"] = crafted(d, (0.5 + 0.25j) + (-0.25 + 0.5j))
    rng = np.random.default_rng(9)
    h = (0.1 * np.exp(2.1j), 0.08 * np.exp(0.4j), 0.09 * np.exp(-1.3j))
    s = rng.choice([-1, 1], size=(3, 16))
    cases["three tags"] = crafted(s[0] * h[0] + s[1] * h[1] + s[2] * h[2], sum(h))
    cases["two tags"] = crafted(two_tags(h[0], h[1], 0xC0DE, 0x0A55), h[0] + h[1], m=0, bits=0x0001)
    return cases


def test_collisions_of_crafted_windows(call_ctx):
    """Windows built from chosen d_j and hs, all in ONE call (13 windows: three full steps of four and a tail of one).  What each case
    is there for is asserted on the reference's record -- whose two restatements must agree on every window -- then the library's
    records must be the reference's"""
    cases = crafted_cases()
    names = list(cases)
    wins = np.stack([cases[n][0] for n in names])
    res = np.stack([cases[n][1] for n in names])
    want = ref.expected_of(wins, res)
    rec = dict(zip(names, want))
    r = rec["all equal"]
    assert r["n_diff"] == 0 and r["flags"] & 4 and r["rn16_a"] == r["rn16_b"] == 0
    assert (r["ha_re"], r["ha_im"], r["hb_re"], r["hb_im"]) == (0.125, 0.25, 0.125, 0.25)        # (hd = 0: both are hs' / 2)
    r = rec["all members"]
    assert r["n_same"] == 0 and r["n_diff"] == 16 and (r["ha_re"] + r["hb_re"], r["ha_im"] + r["hb_im"]) == (1, 1)   # (hs' = hs)
    r = rec["equal strength"]
    assert r["n_diff"] == 8 and not r["flags"] & 8 and (r["ha_re"], r["ha_im"], r["hb_re"], r["hb_im"]) == (0.25, 0.25, 0.25, -0.25)
    r = rec["weaker first"]
    assert r["flags"] & 8 and (r["ha_re"], r["hb_re"]) == (0.75, 0.25)
    r = rec["stronger first"]
    assert not r["flags"] & 8 and (r["ha_re"], r["hb_re"]) == (0.75, 0.25)
    r = rec["two farthest"]
    assert r["n_diff"] == 1 and (r["c_re"], r["c_im"]) == (0, 2)                   # (the first of the two: w_3, not w_7 = (0, -2))
    r = rec["equidistant"]                         # (d_5 = 0 lies as far from P0 as from P1, and from P2 as from P3)
    assert r["n_diff"] > 0 and r["sum_sq"] > 0
    for name in ("all zero", "all zero, a channel", "minus zero"):
        r = rec[name]                              # (with a channel every square lies nearer to c = w_0 = 0 than to A: all are members)
        assert (r["n_diff"], r["flags"] & 4) == ((0, 4) if name == "all zero" else (16, 0)), name
        assert all(r[f].tobytes() == b"\0\0\0\0" for f in ("resid", "sum_sq", "c_re", "c_im")), name
    assert ref.fit(want[names.index("three tags")])[()] > 10 * ref.fit(want[names.index("two tags")])[()]
    r = rec["two tags"]
    assert ref.pair(r) == {0xC0DE, 0x0A55} and r["rn16_a"] == 0xC0DE and not r["flags"] & 3 and r["seq"] == len(names) - 1
    assert len(names) == 13
    got = call_ctx.collisions_of(wins, res)
    ref.assert_equal(got, want, names)
    assert len(call_ctx.collisions_of(wins[:0], res[:0])) == 0


def test_collisions_of_all_sync_offsets(call_ctx):
    """a two-tag window at every sync offset 0 .. 14, 1 to 15 windows per call (every tail of a step): both handles, and the
    reference's records"""
    rng = np.random.default_rng(11)
    wins, res, sent = [], [], []
    for m in range(15):
        a, b = (int(v) for v in rng.integers(0, 65536, 2))
        h1, h2 = 0.1 * np.exp(1j * rng.uniform(0, 6.28)), 0.06 * np.exp(1j * rng.uniform(0, 6.28))
        noise = 0.002 * (rng.standard_normal(16) + 1j * rng.standard_normal(16))
        w, r = crafted(two_tags(h1, h2, a, b) + noise, h1 + h2, m=m, bits=int(rng.integers(0, 65536)))
        w += (0.001 * (rng.standard_normal(WIN) + 1j * rng.standard_normal(WIN))).astype(np.complex64)    # (z_2j+1 is no zero)
        wins.append(w), res.append(r), sent.append((a, b))
    wins, res = np.stack(wins), np.stack(res)
    want = ref.expected_of(wins, res)
    for k, (a, b) in enumerate(sent):
        assert (int(want[k]["rn16_a"]), int(want[k]["rn16_b"])) == (a, b), (k, want[k])
    for n in range(1, 16):
        ref.assert_equal(call_ctx.collisions_of(wins[15 - n:], res[15 - n:]), _renumbered(want[15 - n:]), n)


def _renumbered(rows):
    rows = rows.copy()
    rows["seq"] = np.arange(len(rows))
    return rows


def test_collisions_of_refuses(call_ctx):
    import rfid
    w, r = crafted(np.ones(16) * (0.5 + 0j), 0.5 + 0j)
    with pytest.raises(ValueError):
        call_ctx.collisions_of(np.zeros(249, dtype=np.complex64), r)
    with pytest.raises(ValueError):
        call_ctx.collisions_of(np.zeros((2, 240), dtype=np.complex64), [r, r])
    lib, h, INVALID = call_ctx._lib, call_ctx._h, rfid.capi.ERR_INVALID
    wins = np.stack([w, w])
    res = np.stack([r, r])
    out = np.zeros(2, dtype=rfid.capi.COLLISION_DTYPE)
    args = lambda g=wins.ctypes.data, rr=res.ctypes.data, n=2, o=out.ctypes.data: (h, g, rr, n, o)
    assert lib.rfid_collisions_of(*args()) == rfid.capi.OK
    ref.assert_equal(out, ref.expected_of(wins, res), "accepted")
    assert lib.rfid_collisions_of(*args(n=-1)) == INVALID and lib.rfid_collisions_of(*args(n=0)) == rfid.capi.OK
    assert lib.rfid_collisions_of(*args(g=None)) == INVALID and lib.rfid_collisions_of(*args(rr=None)) == INVALID
    assert lib.rfid_collisions_of(*args(o=None)) == INVALID and lib.rfid_collisions_of(None, *args()[1:]) == INVALID
    before = out.copy()
    for field, value in (("type", 1), ("index", 64), ("index", 80)):
        res[1] = r
        res[1][field] = value
        assert lib.rfid_collisions_of(*args()) == INVALID, (field, value)
        assert "rfid_collisions_of" in lib.rfid_last_error(h).decode()
    assert out.tobytes() == before.tobytes()                     # (nothing was launched)

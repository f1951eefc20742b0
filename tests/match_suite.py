"""The cases of the match stage that run on both sides, written once: tests/test_match_emu.py (the kernels on the wave emulator) and
tests/test_gpu_match.py (on the device) import everything here and define `backend` (tests/stage_backend.py: how a pass reaches the
library) and `call_ctx` (the context of the per-call cases).  Pytest collects the imported functions in the importing module, resolves
their fixtures there and applies that module's marks.  Every expected record is worked out in numpy from the ORACLE alone
(tests/match_ref.py) and every comparison is exact, the floats by bit pattern.

The batch: four traces, FIXED_Q = 2, tags (1, 2, 3), sigma = 0.03, t1_jitter_raw = 3, h = |h| e^{j 2.1}, odd row stride: (|h|, seed,
rounds) = (0.026, 22, 6), (0.026, 72, 4), (0.022, 22, 6), (0.018, 72, 6).  The last one's decoder reads nothing: its inventory is
empty.  What is asserted of it before anything runs (on the reference alone, with the host's rule restated in match_ref.policy): own
mode attributes at least 8, 2 and 2 windows of the first three traces, list mode at least 8, 2, 10 and 8 -- the list is the six
frames the two sessions (seeds 22 and 72) sent, three each, so every trace also meets three frames nobody sent in it;
every attributed window is a single-responder slot whose sent frame is best's; no window of an empty or collided slot is attributed;
in own mode no reply of a tag the trace's inventory lacks is attributed; the table has more than one block of eight rows."""
import ctypes as C

import numpy as np
import pytest

import inventory_ref
import match_ref as ref
from diversity_suite import by_sync_offset, crafted_frame, crafted_y, result_for
from stage_backend import lay_out

__all__ = ["batch", "batch_rows", "small", "test_abi_version_is_7", "test_batch_equals_the_reference_in_own_and_list_mode_and_both_front_end_modes",
           "test_truth_every_attributed_window_holds_the_reply_of_its_tag", "test_a_list_set_and_cleared_gives_the_own_mode_bytes_back",
           "test_windows_behind_the_cut_off_are_absent_and_their_rows_zero", "test_plan_larger_than_the_batch_and_a_small_grid",
           "test_overlap_each_pass_gets_its_own_records", "test_other_stages_results_and_statistics_are_untouched",
           "test_protocol_capacity_state_and_null_pointer_errors", "test_a_list_of_1025_frames_is_refused",
           "test_match_window_finds_the_sent_frame_over_all_sync_offsets", "test_match_window_on_crafted_spans",
           "test_match_window_many_candidates_merge_in_index_order", "test_match_window_refuses"]

SIGMA = 0.03
SPEC = ((0.026, 22, 6), (0.026, 72, 4), (0.022, 22, 6), (0.018, 72, 6))       # |h|, seed, rounds
OWN_AT_LEAST, LIST_AT_LEAST = (8, 2, 2, 0), (8, 2, 10, 8)
MAX_TAGS = 8
N = len(SPEC)


def trace_of(synth_mod, b):
    a, seed, rounds = SPEC[b]
    return synth_mod.make_trace(n_rounds=rounds, fixed_q=2, tag_ids=(1, 2, 3), sigma=SIGMA, seed=seed, t1_jitter_raw=3, h=a * np.exp(2.1j))


def sent_frames(slots_per_trace) -> np.ndarray:
    """the distinct frames single responders sent, ordered by their words -> [n][4]"""
    frames = sorted({bytes(ref.pack(sl.epc)) for slots in slots_per_trace for sl in slots if sl.n_tags == 1 and sl.epc_valid})
    return np.array([np.frombuffer(f, dtype=np.uint32) for f in frames], dtype=np.uint32).reshape(-1, 4)


def oracle_of(oracle_mod, host, lens, frames=None, **cfg):
    """-> (oracle Results, own-mode rows per trace, list-mode rows per trace or None)"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    own = [ref.expected_rows(o, y, b, None, MAX_TAGS) for b, (o, y) in enumerate(zip(refs, ys))]
    lst = [ref.expected_rows(o, y, b, frames) for b, (o, y) in enumerate(zip(refs, ys))] if frames is not None else None
    return refs, own, lst


def check_truth(rows, slots, own: bool):
    """-> the attributed rows of one trace, each of them the reply of best's tag in a single-responder slot"""
    assert len(rows) == len(slots)
    att = ref.policy(rows)
    had = {bytes(np.ascontiguousarray(r["frame"])) for r in rows[att]}
    for rec, sl, a in zip(rows, slots, att):
        single = sl.n_tags == 1 and sl.epc_valid
        if a:
            assert single and list(ref.frame_bits(rec)) == list(sl.epc), (rec, sl)
            assert not rec["flags"] & ref.READ and rec["n_cand"] >= 1 and 0 <= rec["best"] < rec["n_cand"] and rec["sig_abs"] > 0
        if not single:
            assert not a and sl.epc is None, (rec, sl)
    return int(att.sum()), had


def check_rows(ctx, want, what="", extra=3):
    """every trace's row of the last batch_match_enqueue against the reference's, the rows behind it zero, nrows == n_windows_used / 2
    -> the bytes of all rows"""
    st = ctx.batch_stats()
    blob = b""
    for b, w in enumerate(want):
        r = ctx.batch_window_matches(b, extra=extra)
        assert int(st[b]["n_windows_used"]) // 2 == len(w), (what, b, int(st[b]["n_windows_used"]), len(w))
        assert len(r) >= len(w) and (extra > 1000 or len(r) == len(w) + extra), (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, b)
        ref.assert_equal(r[: len(w)], w, (what, b))
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_window_matches(ctx._h, b, None, 0, C.byref(n)) in (0, -5) and n.value == len(w)
        blob += r[: len(w) + 3].tobytes()
    return blob


def own_pass(backend, ctx, dev, L, stride):
    """a pass, its inventory and the match stage behind it"""
    backend.run_pass(ctx, dev, L, stride)
    ctx.batch_inventory_enqueue()
    ctx.batch_match_enqueue()


@pytest.fixture(scope="module")
def batch(backend, oracle_mod, synth_mod):
    traces = [trace_of(synth_mod, b) for b in range(N)]
    host, lens, L, stride = lay_out([t.samples for t in traces], odd_stride=True)
    assert stride & 1
    slots = [t.slots for t in traces]
    frames = sent_frames(slots)
    assert len(frames) == 6                                                       # (three per session: seeds 22 and 72)
    refs, own, lst = oracle_of(oracle_mod, host, lens, frames)
    for b in range(N):                                                            # (on the reference alone, before anything runs)
        entries = inventory_ref.expected(refs[b].dumps, b)
        n_own, had_own = check_truth(own[b], slots[b], True)
        n_lst, had_lst = check_truth(lst[b], slots[b], False)
        print("trace %d: %d EPC windows, %d failed, inventory %d; attributed: own mode %d, list mode %d" %
              (b, len(own[b]), int(((own[b]["flags"] & 1) == 0).sum()), len(entries), n_own, n_lst))
        assert n_own >= OWN_AT_LEAST[b] and n_lst >= LIST_AT_LEAST[b], (b, n_own, n_lst)
        assert had_own <= {bytes(np.ascontiguousarray(e["frame"])) for e in entries}        # no tag the trace's inventory lacks
        assert len(own[b]) == 4 * SPEC[b][2] and len(own[b]) > 8                              # more than one block of eight rows
        assert set(lst[b]["flags"]) <= {ref.LIST, ref.LIST | ref.READ} and set(lst[b]["n_cand"]) <= {0, 6}
    assert len(inventory_ref.expected(refs[3].dumps, 3)) == 0 and set(own[3]["flags"]) == {ref.NO_CANDIDATES}
    assert all(not r.tobytes()[16:].strip(b"\0") for r in own[3]) and 1 <= len(inventory_ref.expected(refs[2].dumps, 2)) < 3
    return dict(host=host, lens=lens, L=L, stride=stride, refs=refs, own=own, lst=lst, frames=frames, slots=slots, dev=backend.put(host, lens))


@pytest.fixture(scope="module")
def batch_rows(backend, batch):
    """one pass over the batch through the fused front end, own mode then list mode -> (own rows, list rows, own bytes, list bytes, match ms
    of the list pass, decode ms)"""
    import rfid
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(N, batch["L"])
        ctx.batch_plan_inventory(MAX_TAGS)
        ctx.batch_plan_match()
        own_pass(backend, ctx, batch["dev"], batch["L"], batch["stride"])
        own_blob = check_rows(ctx, batch["own"], "fixture, own")
        own_rows = [ctx.batch_window_matches(b) for b in range(N)]
        assert ctx.batch_ls_report()["pieces"] == 0
        ctx.batch_match_set_list(batch["frames"])
        ctx.batch_match_enqueue()                                   # (the same pass again: its statistics are current)
        lst_blob = check_rows(ctx, batch["lst"], "fixture, list")
        return (own_rows, [ctx.batch_window_matches(b) for b in range(N)], own_blob, lst_blob, ctx.batch_match_ms(),
                ctx.batch_timing()["decode_ms"])
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def small(backend, batch):
    """traces 1 and 2 of the batch (16 and 24 EPC windows, inventories of three and of one tag) as a batch of its own: what the protocol
    cases run on -> (host, lens, L, stride, own rows, list rows, device handle, refs, the list of six frames)"""
    h, l = np.ascontiguousarray(batch["host"][1:3]), batch["lens"][1:3].copy()
    own, lst = [w.copy() for w in batch["own"][1:3]], [w.copy() for w in batch["lst"][1:3]]
    for b in range(2):
        own[b]["stream"], lst[b]["stream"] = b, b
    return h, l, batch["L"], batch["stride"], own, lst, backend.put(h, l), batch["refs"][1:3], batch["frames"]


def test_abi_version_is_7():
    import rfid
    assert rfid.capi.load().rfid_abi_version() == 7


def test_batch_equals_the_reference_in_own_and_list_mode_and_both_front_end_modes(backend, batch, batch_rows):
    """the batch, backend.reps passes through the fused front end and one through the long-stream front end (modes 0 and 2), each in own
    mode and in list mode: the reference's records and the same table bytes every time"""
    import rfid
    L = batch["L"]
    own_blob, lst_blob, ms, decode_ms = batch_rows[2:]
    failed = sum(int(((w["flags"] & 1) == 0).sum()) for w in batch["lst"])
    print("%s: match of the batch (%d EPC windows of %d traces, %d failed, 6 candidates each): %.4f ms; decode of the same pass %.4f ms" %
          (backend.name, sum(map(len, batch["lst"])), N, failed, ms, decode_ms))
    assert ms >= 0.0
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(N, L)
        ctx.batch_plan_inventory(MAX_TAGS)
        ctx.batch_plan_match()
        for mode in [0] * (backend.reps - 1) + [2]:
            ctx.batch_set_long_stream(mode)
            ctx.batch_match_set_list(None)
            own_pass(backend, ctx, batch["dev"], L, batch["stride"])
            assert check_rows(ctx, batch["own"], ("own", mode)) == own_blob
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
            ctx.batch_match_set_list(batch["frames"])
            ctx.batch_match_enqueue()
            assert check_rows(ctx, batch["lst"], ("list", mode)) == lst_blob
        many = ctx.batch_window_matches(1, extra=10_000)            # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(batch["lst"][1])], batch["lst"][1])
        assert len(many) > len(batch["lst"][1]) and not many[len(batch["lst"][1]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_truth_every_attributed_window_holds_the_reply_of_its_tag(batch, batch_rows):
    """Against SlotTruth, on the records the library gave: every attributed window is a single-responder slot whose sent frame is
    best's, none is an empty or collided slot; the counts are the reference's.  In list mode the third trace -- whose decoder read one
    tag, twice -- gains ten sightings of all three tags, and the fourth, whose decoder read nothing, at least eight"""
    own_rows, lst_rows = batch_rows[:2]
    for b in range(N):
        n_own, _ = check_truth(own_rows[b], batch["slots"][b], True)
        n_lst, had = check_truth(lst_rows[b], batch["slots"][b], False)
        assert n_own >= OWN_AT_LEAST[b] and n_lst >= LIST_AT_LEAST[b]
        assert n_own == int(ref.policy(batch["own"][b]).sum()) and n_lst == int(ref.policy(batch["lst"][b]).sum())
    assert len(had) >= 2


def test_a_list_set_and_cleared_gives_the_own_mode_bytes_back(backend, small):
    """own, list, own on the same pass: the first and the last table are the same bytes; the list survives a new pass and a new
    inventory plan; NULL with a count and a count of 0 both clear it"""
    import rfid
    host, lens, L, stride, own, lst, dev, refs, frames = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(MAX_TAGS)
        ctx.batch_plan_match()
        own_pass(backend, ctx, dev, L, stride)
        first = check_rows(ctx, own, "own")
        ctx.batch_match_set_list(frames)
        ctx.batch_match_enqueue()
        listed = check_rows(ctx, lst, "list")
        assert listed != first
        assert ctx._lib.rfid_batch_match_set_list(ctx._h, None, 3) == rfid.capi.OK       # (NULL: the inventory again)
        ctx.batch_match_enqueue()
        assert check_rows(ctx, own, "own again") == first
        ctx.batch_match_set_list(frames)
        ctx.batch_plan_inventory(MAX_TAGS)                           # (drops neither the workspace nor the list)
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_match_enqueue()                                    # (no inventory behind this pass: none is needed)
        assert check_rows(ctx, lst, "list, next pass") == listed
        ctx.batch_match_set_list(np.zeros((0, 4), dtype=np.uint32))
        ctx.batch_inventory_enqueue()
        ctx.batch_match_enqueue()
        assert check_rows(ctx, own, "own, cleared with n = 0") == first
    finally:
        ctx.close()


def test_windows_behind_the_cut_off_are_absent_and_their_rows_zero(backend, oracle_mod, batch):
    """MAX_NUM_QUERIES = 5 reached inside the first block of eight rows: nrows == n_windows_used / 2 = 5, the rows behind it zero, also
    when more rows are asked for than the table has -- the inventories end at the cut-off too.  Then in one context: rows an earlier
    pass had filled are zeroed again by a pass over shorter traces"""
    import rfid
    host, lens, L, stride, dev, frames = batch["host"], batch["lens"], batch["L"], batch["stride"], batch["dev"], batch["frames"]
    refs, own, lst = oracle_of(oracle_mod, host, lens, frames, max_num_queries=5)
    assert [o.state.status for o in refs] == [1] * N and [len(w) for w in own] == [5] * N
    assert sum(int(ref.policy(w).sum()) for w in lst) >= 3
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=5)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(N, L)
        ctx.batch_plan_inventory(MAX_TAGS)
        ctx.batch_plan_match()
        own_pass(backend, ctx, dev, L, stride)
        check_rows(ctx, own, "cut, own")
        ctx.batch_match_set_list(frames)
        ctx.batch_match_enqueue()
        check_rows(ctx, lst, "cut, list")
        check_rows(ctx, lst, "cut, all rows", extra=10_000)
    finally:
        ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(N, L)
        ctx.batch_plan_match()
        ctx.batch_match_set_list(frames)
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_match_enqueue()
        check_rows(ctx, batch["lst"], "full")
        cut = lens.copy()
        keep = (4, 6, 9, 3)
        for b in range(N):
            cut[b] = 5 * int(batch["refs"][b].open_idx[2 * (keep[b] - 1) + 1] + ref.EPC_WIN + 60)
        short_refs, _, short = oracle_of(oracle_mod, host, cut, frames)
        assert [len(o.dumps) // 2 for o in short_refs] == list(keep) and [len(r) for r in short] == list(keep)
        dcut = backend.put(host, cut)
        backend.run_pass(ctx, dcut, L, stride)
        ctx.batch_match_enqueue()
        check_rows(ctx, short, "short", extra=10_000)
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_a_small_grid(backend, small):
    """A plan of eight traces, two of them processed: two passes give the same table bytes, the second with match_wgs = 3 (the
    table's blocks of rows, more than three, on three workgroups: a workgroup goes round its loop again); a trace not covered is not
    fetched; a new plan drops the workspace and the list"""
    import rfid
    host, lens, L, stride, own, lst, dev, refs, frames = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(8, L)
        ctx.batch_plan_inventory(MAX_TAGS)
        ctx.batch_plan_match()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            if rep:
                ctx.set_knob("match_wgs", 3)
            own_pass(backend, ctx, dev, L, stride)
            blobs.append(check_rows(ctx, own, rep))
        assert blobs[0] == blobs[1] and ctx.get_knob("match_wgs") == 3
        ctx.batch_match_set_list(frames)
        ctx.batch_match_enqueue()
        check_rows(ctx, lst, "list, three workgroups")
        n = C.c_int64(0)
        assert ctx._lib.rfid_batch_get_window_matches(ctx._h, 2, None, 0, C.byref(n)) == rfid.capi.ERR_INVALID     # (not covered)
        assert ctx.batch_window_matches(0, extra=10_000).shape[0] > 8 * 3      # (more blocks of rows than workgroups)
        ctx.batch_plan(2, L)
        for fn in (ctx.batch_match_enqueue, lambda: ctx.batch_window_matches(0), ctx.batch_match_ms, lambda: ctx.batch_match_set_list(None)):
            with pytest.raises(rfid.capi.RfidError) as e:
                fn()
            assert e.value.status == rfid.capi.ERR_STATE
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_plan_match()
        ctx.batch_plan_inventory(MAX_TAGS)
        ctx.batch_inventory_enqueue()                                # (the pass before the workspaces: its statistics are current)
        ctx.batch_match_enqueue()                                    # (and the list went with the old workspace: own mode)
        assert check_rows(ctx, own, "planned again") == blobs[0]
    finally:
        ctx.close()


@pytest.mark.parametrize("overlap", [1, 2])
def test_overlap_each_pass_gets_its_own_records(backend, small, overlap):
    """RFID_OVERLAP 1 and 2 (two result sets where the plan has them): the next pass -- the two traces exchanged, so every row holds
    another trace's records and candidates -- enqueued BEFORE this pass's records are fetched leaves them this pass's, then gets its own"""
    import rfid
    host, lens, L, stride, own_a, _, dev_a, refs, _ = small
    order = [1, 0]
    dev_b = backend.put(np.ascontiguousarray(host[order]), lens[order].copy())
    own_b = [own_a[k].copy() for k in order]
    for b in range(2):
        own_b[b]["stream"] = b
    assert own_a[0].tobytes() != own_b[0].tobytes()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.set_knob("overlap", overlap)
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(MAX_TAGS)
        ctx.batch_plan_match()
        for rep in range(2):
            own_pass(backend, ctx, dev_a, L, stride)
            backend.run_pass(ctx, dev_b, L, stride)
            for b in range(2):
                ref.assert_equal(ctx.batch_window_matches(b), own_a[b], ("a", rep, b))
            ctx.batch_inventory_enqueue()
            ctx.batch_match_enqueue()
            check_rows(ctx, own_b, ("b", rep))
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
    w, r, _ = ctx.batch_windows()
    parts = [ent, counts_, reads, off, q, rep, fine, ctx.batch_stats(), w, r, ctx.batch_window_diversity(0, extra=2)]
    for b in range(n):
        parts += [ctx.batch_window_quality(b, extra=2), ctx.batch_window_repairs(b, extra=2), ctx.batch_window_fine(b, extra=2),
                  ctx.batch_window_moments(b, extra=2), ctx.batch_window_commands(b, extra=2), ctx.batch_window_retunes(b, extra=2),
                  ctx.batch_window_collisions(b, extra=2), ctx.batch_window_lengths(b, extra=2)]
    return [np.ascontiguousarray(p).tobytes() for p in parts]


@pytest.mark.parametrize("order", ["match-first", "match-last"])
def test_other_stages_results_and_statistics_are_untouched(backend, small, order):
    """inventory, tracks, quality, repair, fine, slots, commands, retune, collisions, lengths and diversity (the two traces as one pair)
    on the same pass, without the match stage and with it -- enqueued before all of them (with a list: it needs no inventory) or
    behind all of them (on the trace's own inventories): every other fetched array -- results and statistics among them -- is
    byte-identical"""
    import rfid
    host, lens, L, stride, own, lst, dev, refs, frames = small
    outs = []
    for match in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_inventory(MAX_TAGS)
            ctx.batch_plan_tracks()
            for plan in (ctx.batch_plan_quality, ctx.batch_plan_repair, ctx.batch_plan_fine, ctx.batch_plan_slots, ctx.batch_plan_commands,
                         ctx.batch_plan_retune, ctx.batch_plan_collisions, ctx.batch_plan_lengths, lambda: ctx.batch_plan_diversity(2)):
                plan()
            if match:
                ctx.batch_plan_match()
            backend.run_pass(ctx, dev, L, stride)
            if match and order == "match-first":
                ctx.batch_match_set_list(frames)
                ctx.batch_match_enqueue()
            outs.append(other_outputs(ctx, 2))
            if match and order == "match-last":
                ctx.batch_match_enqueue()
            if match:
                check_rows(ctx, lst if order == "match-first" else own, order)
                assert other_outputs(ctx, 2) == outs[-1]           # (and the stage lowered nothing: the others run again behind it)
        finally:
            ctx.close()
    assert len(outs[0]) == len(outs[1]) and all(a == b for a, b in zip(*outs)), [a == b for a, b in zip(*outs)]
    assert sum(map(len, outs[0])) > 5_000


def test_protocol_capacity_state_and_null_pointer_errors(backend, small):
    import rfid
    host, lens, L, stride, own, lst, dev, refs, frames = small
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
        raises(ctx.batch_plan_match, ERR_STATE, "rfid_batch_plan_match: no plan")
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        raises(ctx.batch_match_enqueue, ERR_STATE, "rfid_batch_plan_match")             # no workspace
        raises(lambda: ctx.batch_match_set_list(frames), ERR_STATE, "rfid_batch_plan_match")
        ctx.batch_plan_match()
        raises(ctx.batch_match_enqueue, ERR_STATE)                                       # own mode: no inventory workspace
        raises(lambda: ctx.batch_window_matches(0), ERR_STATE)                           # nothing enqueued
        raises(ctx.batch_match_ms, ERR_STATE)
        ctx.batch_match_set_list(frames)
        raises(ctx.batch_match_enqueue, ERR_STATE, "no pass with statistics yet")        # list mode: no pass
        backend.run_pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_matches(0), ERR_STATE)                           # a pass, but nothing enqueued behind it
        ctx.batch_match_enqueue()                                                        # (no inventory workspace: none is needed with a list)
        blob = check_rows(ctx, lst, "list, no inventory")
        # own mode asks what rfid_batch_repair asks
        ctx.batch_match_set_list(None)
        raises(ctx.batch_match_enqueue, ERR_STATE)                                       # no inventory workspace
        ctx.batch_plan_inventory(MAX_TAGS)                                               # (does not drop the match workspace)
        ctx.batch_plan_repair()
        raises(ctx.batch_match_enqueue, ERR_STATE, "no rfid_batch_inventory behind the last pass")
        raises(ctx.batch_repair_enqueue, ERR_STATE, "no rfid_batch_inventory behind the last pass")
        assert check_rows(ctx, lst, "a refused call changes nothing") == blob
        # the level of the other stages is neither raised ...
        ctx.batch_plan_tracks()
        ctx.batch_match_set_list(frames)
        ctx.batch_match_enqueue()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)                                      # (the match stage is not an inventory)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_match_set_list(None)
        ctx.batch_match_enqueue()
        ctx.batch_tracks_enqueue()                                                       # ... nor lowered: the inventory is still this pass's
        check_rows(ctx, own, "behind the tracks")
        # a caller's array that is too small loses nothing
        row = np.zeros(len(own[0]) - 1, dtype=rfid.capi.MATCH_DTYPE)
        n = C.c_int64(0)
        rc = lib.rfid_batch_get_window_matches(h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(own[0]) and not row.tobytes().strip(b"\0") and "EPC windows" in last()
        full = np.zeros(n.value, dtype=rfid.capi.MATCH_DTYPE)
        assert lib.rfid_batch_get_window_matches(h, 0, full.ctypes.data, len(full), C.byref(n)) == OK
        ref.assert_equal(full, own[0])
        for b in (2, -1):
            assert lib.rfid_batch_get_window_matches(h, b, None, 0, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_get_window_matches(h, 0, None, 0, None) == ERR_INVALID
        assert lib.rfid_batch_get_window_matches(h, 0, None, 4, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_match_ms(h, None) == ERR_INVALID
        assert lib.rfid_batch_plan_match(None) == ERR_INVALID and lib.rfid_batch_match(None) == ERR_INVALID
        assert lib.rfid_batch_match_set_list(None, frames.ctypes.data, 3) == ERR_INVALID
        assert lib.rfid_batch_get_window_matches(None, 0, None, 0, C.byref(n)) == ERR_INVALID
        assert lib.rfid_batch_match_ms(None, C.byref(C.c_float(0))) == ERR_INVALID
        assert lib.rfid_batch_match_set_list(h, frames.ctypes.data, -1) == ERR_INVALID and "rfid_batch_match_set_list" in last()
        check_rows(ctx, own, "a refused list changes nothing")
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        raises(ctx.batch_match_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_matches(0), ERR_STATE)
    finally:
        ctx.close()


def test_a_list_of_1025_frames_is_refused(backend, oracle_mod, small):
    """RFID_MATCH_MAX_LIST = 1024 frames are taken -- the six sent frames at the end of the last chunk of 64 -- and 1025 are refused with
    RFID_ERR_INVALID and a message; the refused call leaves the list as it was"""
    import rfid
    host, lens, L, stride, own, lst, dev, refs, sent = small
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 2 ** 32, size=(1025, 4), dtype=np.uint64).astype(np.uint32)
    frames[1018:1024] = sent
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_match()
        with pytest.raises(ValueError):
            ctx.batch_match_set_list(frames)
        assert ctx._lib.rfid_batch_match_set_list(ctx._h, frames.ctypes.data, 1025) == rfid.capi.ERR_INVALID
        assert "1024" in ctx._lib.rfid_last_error(ctx._h).decode()
        ctx.batch_match_set_list(frames[:1024])
        assert ctx._lib.rfid_batch_match_set_list(ctx._h, frames.ctypes.data, 1025) == rfid.capi.ERR_INVALID
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_match_enqueue()
        want = [ref.expected_rows(o, oracle_mod.fir(host[b, : lens[b]]), b, frames[:1024]) for b, o in enumerate(refs)]
        check_rows(ctx, want, "1024 frames")
        for b in range(2):
            att = ref.policy(want[b])
            assert att.sum() == ref.policy(lst[b]).sum() and set(want[b]["best"][att]) <= set(range(1018, 1024)) and set(want[b]["n_cand"]) <= {0, 1024}
    finally:
        ctx.close()


# ---- rfid_match_window on crafted, noise-free spans ----------------------------------------------------------------------------
def others(synth_mod, n, seed=40):
    """n frames of other tags, valid CRCs"""
    return [crafted_frame(synth_mod, tag_id=0x31 + i, seed=seed + i) for i in range(n)]


def words(frames) -> np.ndarray:
    return np.array([ref.pack(f) for f in frames], dtype=np.uint32).reshape(-1, 4)


def bits_of(x) -> bytes:
    return np.float32(x).tobytes()


def test_match_window_finds_the_sent_frame_over_all_sync_offsets(oracle_mod, synth_mod, call_ctx):
    """the sent frame among others, the reply cut so that the decoder's sync offset takes every value 0 .. 14, each with a channel of
    its own: best is the sent frame at the full score, the record the reference's (the literal loop on each)"""
    frame = crafted_frame(synth_mod)
    found = by_sync_offset(oracle_mod, synth_mod, frame)
    wrong = others(synth_mod, 4)
    for m in range(15):
        span, res = found[m]
        cands = words(wrong[:m % 4] + [frame] + wrong[m % 4:])
        want = ref.expected_window(span, res, cands, literal=True)
        got = call_ctx.match_window(span, res, cands)
        ref.assert_equal(got, want, m)
        assert got["flags"] == ref.LIST and got["best"] == m % 4 and got["n_cand"] == 5 and list(ref.frame_bits(got)) == list(frame)
        assert got["dist_best"] == 0 and bits_of(got["score_best"]) == bits_of(got["sig_abs"]) and got["sig_abs"] > 0
        assert ref.policy(got).all() and got["score_second"] < 0.5 * got["sig_abs"] and got["diff"] > 20
        assert got["stream"] == got["seq"] == got["start"] == 0


def test_match_window_on_crafted_spans(oracle_mod, synth_mod, call_ctx):
    frame, other = crafted_frame(synth_mod), crafted_frame(synth_mod, tag_id=0x31, seed=6)
    span = crafted_y(oracle_mod, synth_mod, frame)[10:10 + ref.EPC_WIN]
    res = result_for(oracle_mod, span, crc_ok=0)
    check = lambda s, r, c, what: (ref.assert_equal(call_ctx.match_window(s, r, c), ref.expected_window(s, r, c, literal=True), what),
                                   call_ctx.match_window(s, r, c))[1]
    # the decoded frame as a candidate scores sig_abs, bit for bit
    got = check(span, res, words([other, frame]), "decoded frame")
    assert got["best"] == 1 and got["second"] == 0 and got["dist_best"] == 0 and bits_of(got["score_best"]) == bits_of(got["sig_abs"])
    # the span negated under the same result record scores -sig_abs
    got = check(-span, res, words([frame]), "negated")
    assert got["best"] == 0 and bits_of(got["score_best"]) == bits_of(-got["sig_abs"]) and got["sig_abs"] > 0 and not ref.policy(got).any()
    assert got["dist_best"] == 0                                    # (against the RECORD's bits, which the caller left as they were)
    # two identical candidates: the lower index is best, diff = 0; the host's rule attributes (the gap needed is 0)
    got = check(span, res, words([frame, frame, other]), "duplicates")
    assert (got["best"], got["second"], got["diff"]) == (0, 1, 0) and bits_of(got["score_best"]) == bits_of(got["score_second"])
    assert ref.policy(got).all()
    # an all-zero span: every score is +0
    zero = np.zeros(ref.EPC_WIN, dtype=np.complex64)
    got = check(zero, res, words([other, frame, other]), "zero")
    assert (got["best"], got["second"]) == (0, 1) and bits_of(got["score_best"]) == bits_of(got["score_second"]) == bits_of(0.0)
    assert bits_of(got["sig_abs"]) == bits_of(0.0) and not ref.policy(got).any()
    # one candidate: no second
    got = check(span, res, words([frame]), "one candidate")
    assert (got["best"], got["second"], got["diff"], got["n_cand"]) == (0, -1, -1, 1) and bits_of(got["score_second"]) == bits_of(0.0)
    assert ref.policy(got).all()
    # two frames that differ in the last EPC bit only, and hence in the CRC: few decisions tell them apart, and the gap rule still
    # attributes the sent one, in either order
    epc = synth_mod.epc_for_id(0x27, np.random.default_rng(5))
    assert synth_mod.epc_frame(epc) == frame
    twin = synth_mod.epc_frame(epc[:-1] + [epc[-1] ^ 1])
    assert [j for j in range(112) if twin[j] != frame[j]] == [111]
    for cands, best in ((words([frame, twin]), 0), (words([twin, frame]), 1)):
        got = check(span, res, cands, "twins")
        assert got["best"] == best and got["second"] == 1 - best and 1 <= got["diff"] <= 17 and ref.policy(got).all()
        assert got["score_second"] > 0.5 * got["sig_abs"]           # (the threshold alone would take either)
        twin_span = crafted_y(oracle_mod, synth_mod, twin)[10:10 + ref.EPC_WIN]
        other_way = check(twin_span, result_for(oracle_mod, twin_span, crc_ok=0), cands, "twins, the other one sent")
        assert other_way["best"] == 1 - best and ref.policy(other_way).all()
    # crc_ok = 1: bit 0, nothing is searched, the rest is zero
    got = check(span, result_for(oracle_mod, span), words([frame, other]), "a read")
    assert got["flags"] == (ref.READ | ref.LIST) and not got.tobytes()[16:].strip(b"\0") and not ref.policy(got).any()


@pytest.mark.parametrize("n", [65, 130])
def test_match_window_many_candidates_merge_in_index_order(oracle_mod, synth_mod, call_ctx, n):
    """65 and 130 candidates: the sent frame in the last chunk of 64 and a duplicate of it in the first -- the duplicate, with the
    lower index, is best and the one in the last chunk second, at equal scores"""
    frame = crafted_frame(synth_mod)
    span = crafted_y(oracle_mod, synth_mod, frame)[10:10 + ref.EPC_WIN]
    res = result_for(oracle_mod, span, crc_ok=0)
    rng = np.random.default_rng(n)
    cands = rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    cands[n - 1] = cands[5] = ref.pack(frame)
    want = ref.expected_window(span, res, cands, literal=True)
    got = call_ctx.match_window(span, res, cands)
    ref.assert_equal(got, want, n)
    assert (got["best"], got["second"], got["diff"], got["n_cand"], got["dist_best"]) == (5, n - 1, 0, n, 0)
    assert bits_of(got["score_best"]) == bits_of(got["score_second"]) == bits_of(got["sig_abs"])
    # without the duplicate: the last candidate of the last chunk is best, the runner-up is somewhere else and far behind
    cands[5] = cands[6]
    got = call_ctx.match_window(span, res, cands)
    ref.assert_equal(got, ref.expected_window(span, res, cands), (n, "single"))
    assert got["best"] == n - 1 and got["second"] not in (-1, n - 1) and ref.policy(got).all()


def test_match_window_refuses(oracle_mod, synth_mod, call_ctx):
    import rfid
    frame = crafted_frame(synth_mod)
    span = np.ascontiguousarray(crafted_y(oracle_mod, synth_mod, frame)[10:10 + ref.EPC_WIN])
    res = result_for(oracle_mod, span, crc_ok=0)
    cands = words([frame] * 3)
    for bad in (np.zeros(1369, dtype=np.complex64), np.zeros(1371, dtype=np.complex64), np.zeros((2, 1370), dtype=np.complex64)):
        with pytest.raises(ValueError):
            call_ctx.match_window(bad, res, cands)
    for bad in (np.zeros((0, 4), dtype=np.uint32), np.zeros((1025, 4), dtype=np.uint32), np.zeros((3, 5), dtype=np.uint32)):
        with pytest.raises(ValueError):
            call_ctx.match_window(span, res, bad)
    lib, h, INVALID = call_ctx._lib, call_ctx._h, rfid.capi.ERR_INVALID
    r = np.zeros(1, dtype=rfid.capi.RESULT_DTYPE)
    out = np.zeros(1, dtype=rfid.capi.MATCH_DTYPE)
    big = np.zeros((1025, 4), dtype=np.uint32)
    r[0] = res
    args = lambda s=span.ctypes.data, rr=r.ctypes.data, f=cands.ctypes.data, n=3, o=out.ctypes.data: (h, s, rr, f, n, o)
    assert lib.rfid_match_window(*args()) == rfid.capi.OK
    ref.assert_equal(out[0], ref.expected_window(span, r[0], cands), "accepted")
    for n in (0, -1, 1025):
        assert lib.rfid_match_window(*args(f=big.ctypes.data, n=n)) == INVALID and "rfid_match_window" in lib.rfid_last_error(h).decode()
    assert lib.rfid_match_window(*args(f=big.ctypes.data, n=1024)) == rfid.capi.OK
    for kw in (dict(s=None), dict(rr=None), dict(f=None), dict(o=None)):
        assert lib.rfid_match_window(*args(**kw)) == INVALID
    assert lib.rfid_match_window(None, *args()[1:]) == INVALID
    F = np.float32
    for field, value in (("type", 0), ("index", 64), ("index", 80), ("T", np.nextafter(F(4.95), F(0))), ("T", np.nextafter(F(5.05), F(9))),
                         ("T", F(0)), ("T", F(np.nan))):
        r[0] = res
        r[0][field] = value
        assert lib.rfid_match_window(*args()) == INVALID, (field, value)
        assert "rfid_match_window" in lib.rfid_last_error(h).decode()
    for value in (F(4.95), F(5.05)):                               # (the ends of the decoder's own range are accepted)
        r[0] = res
        r[0]["T"] = value
        assert lib.rfid_match_window(*args()) == rfid.capi.OK

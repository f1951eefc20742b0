"""The slots stage on the device (rfid_batch_plan_slots / rfid_batch_slots / rfid_batch_get_window_moments / rfid_batch_slots_ms, and
the per-call rfid_window_moments_of): the second-order moments of every window's gated samples.  Every expected record is worked out
in numpy from the ORACLE alone (tests/slots_ref.py); every comparison is exact -- integers equal, floats by bit pattern, then the bytes
of the whole arrays.  The inputs and the checks are those of tests/test_slots_emu.py (tests/slots_cases.py): the smallest shapes at
which the kernel can still go wrong -- pack tails, odd counts, more than one trace, rows behind a cut-off."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import slots_ref as ref
import slots_cases as cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _dev(host, lens):
    """-> (device tensor of the traces, device tensor of their lengths); the caller keeps both alive"""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(host).view(np.float32)).to("cuda:0")
    dlens = torch.from_numpy(np.ascontiguousarray(lens)).to("cuda:0")
    torch.cuda.synchronize()
    return dev, dlens


@pytest.fixture(scope="module")
def ragged(oracle_mod, synth_mod):
    host, lens, L, stride, refs, want = cases.ragged_batch(oracle_mod, synth_mod)
    return host, lens, L, stride, refs, want, _dev(host, lens)


@pytest.fixture(scope="module")
def small(ragged):
    """the two short traces of the ragged batch (30 and 7 windows) as a batch of their own"""
    host, lens, L, stride, refs, want, _ = ragged
    w = [r.copy() for r in want[1:]]
    for r in w:
        r["stream"] -= 1
    h, l = np.ascontiguousarray(host[1:]), lens[1:].copy()
    return h, l, L, stride, refs[1:], w, _dev(h, l)


def _pass(ctx, dev, L, stride):
    ctx.batch_process_ptr(dev[0].data_ptr(), stride, L, dev[1].data_ptr())


def test_abi_version_is_7():
    import rfid
    assert rfid.capi.load().rfid_abi_version() == 7


def test_moments_of_a_ragged_multi_tag_batch_equal_the_oracles(ragged):
    """Three traces of 93, 30 and 7 windows, odd row stride; the pass three times: the same table bytes every time"""
    import rfid
    host, lens, L, stride, refs, want, dev = ragged
    assert all(len(w) % 8 for w in want) and sum((w["flags"] == 3).sum() for w in want) >= 10
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_slots()
        blobs = []
        for rep in range(3):
            _pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep))
        assert blobs[0] == blobs[1] == blobs[2]
        assert ctx.batch_ls_report()["pieces"] == 0
        print("slots of 3 traces (%d windows): %.4f ms; decode of the same pass %.4f ms" %
              (sum(map(len, want)), ctx.batch_slots_ms(), ctx.batch_timing()["decode_ms"]))
        many = ctx.batch_window_moments(2, extra=10_000)         # (more than the table has: the whole row of the trace)
        ref.assert_equal(many[: len(want[2])], want[2])
        assert not many[len(want[2]):].tobytes().strip(b"\0")
    finally:
        ctx.close()


def test_long_stream_front_end_gives_the_same_records(ragged):
    """rfid_batch_set_long_stream mode 2 on one trace (the 93-window one): the records of the fused front end, the oracle's"""
    import rfid
    host, lens, L, stride, refs, want, _ = ragged
    dev = _dev(host[:1], lens[:1])
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(1, L)
        ctx.batch_plan_slots()
        blobs = []
        for mode in (2, 0, 2):
            ctx.batch_set_long_stream(mode)
            _pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            blobs.append(cases.check_rows(ctx, want[:1], mode))
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        assert blobs[0] == blobs[1] == blobs[2]
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
    dev = _dev(host, lens)
    ctx = rfid.Context(device=0, fixed_q=0)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(1, L)
        ctx.batch_plan_slots()
        _pass(ctx, dev, L, stride)
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
    host, lens, L, stride, full_refs, full_want, dev = small
    refs, want = cases.oracle_of(oracle_mod, host, lens, 2, max_num_queries=5)
    assert [o.state.status for o in refs] == [1, 0] and [len(w) for w in want] == [10, 7]
    for mq, w in ((1000, full_want), (5, want)):
        ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=mq)
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(2, L)
            ctx.batch_plan_slots()
            _pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            cases.check_rows(ctx, w, mq, extra=len(full_want[0]))
            assert [int(s["n_windows_used"]) for s in ctx.batch_stats()] == [len(r) for r in w]
        finally:
            ctx.close()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_slots()
        _pass(ctx, dev, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, full_want, "full")
        cut = lens.copy()
        cut[0] = cases.cut_behind(oracle_mod, host[0, : lens[0]], 2, 13)
        cut[1] = cases.cut_behind(oracle_mod, host[1, : lens[1]], 2, 4)
        short_refs, short = cases.oracle_of(oracle_mod, host, cut, 2)
        assert [len(r) for r in short] == [13, 4]
        dcut = _dev(host, cut)
        _pass(ctx, dcut, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, short, "short", extra=len(full_want[0]))
    finally:
        ctx.close()


def test_plan_larger_than_the_batch_and_a_new_plan(small):
    """A plan of five traces, two of them processed (rfid_batch_set_streams): two passes give the same table bytes; the traces not
    covered are not fetched; a new plan drops the workspace"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(5, L)
        ctx.batch_plan_slots()
        ctx.batch_set_streams(2)
        blobs = []
        for rep in range(2):
            _pass(ctx, dev, L, stride)
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
        _pass(ctx, dev, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_slots_enqueue()
        assert e.value.status == rfid.capi.ERR_STATE and "rfid_batch_plan_slots" in str(e.value)
        ctx.batch_plan_slots()
        ctx.batch_slots_enqueue()                                # (the pass before the workspace: its statistics are current)
        cases.check_rows(ctx, want, "planned again")
    finally:
        ctx.close()


def test_two_result_sets_each_pass_gets_its_own_records(small):
    """44 traces (the two short ones, 22 times: 2 200 packs of rows against the 2 048 workgroups of a 256-CU launch, so a workgroup
    goes round its loop again), two result sets alternating (RFID_OVERLAP=2): the next pass -- the traces in the other order -- enqueued
    BEFORE this pass's records are fetched leaves them this pass's, then gets its own"""
    import rfid
    host, lens, L, stride, refs, want, _ = small
    order = np.arange(44) % 2
    dev_a = _dev(host[order], lens[order])
    dev_b = _dev(host[1 - order], lens[1 - order])

    def stamped(which):
        out = []
        for b, k in enumerate(which):
            r = want[k].copy()
            r["stream"] = b
            out.append(r)
        return out

    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.set_knob("overlap", 2)
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(44, L)
        ctx.batch_plan_slots()
        for rep in range(2):
            _pass(ctx, dev_a, L, stride)
            ctx.batch_slots_enqueue()
            _pass(ctx, dev_b, L, stride)
            for b, w in enumerate(stamped(order)):
                ref.assert_equal(ctx.batch_window_moments(b), w, ("a", rep, b))
            ctx.batch_slots_enqueue()
            cases.check_rows(ctx, stamped(1 - order), ("b", rep))
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["slots-first", "slots-last"])
def test_other_stages_are_untouched(small, order):
    """inventory + tracks + quality + repair on the same pass, with the slots stage enqueued before or behind them and without it:
    every other fetched array is byte-identical"""
    import rfid
    host, lens, L, stride, refs, want, dev = small
    outs = []
    for slots in (False, True):
        ctx = rfid.Context(device=0, fixed_q=2)
        try:
            ctx.batch_set_long_stream(0)
            cases.plan_all(ctx, 2, L, slots=slots)
            _pass(ctx, dev, L, stride)
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


def test_per_call_path_on_crafted_windows(oracle_mod, ragged, gpu_ctx):
    import rfid
    host, lens, L, stride, refs, want, _ = ragged
    g = cases.crafted_windows(oracle_mod, host, lens, refs, stream=0, seq=5)
    cases.check_crafted(gpu_ctx, g, want[0][5])
    with pytest.raises(ValueError):
        gpu_ctx.window_moments(np.zeros((2, 239), dtype=np.complex64))
    assert gpu_ctx._lib.rfid_window_moments_of(gpu_ctx._h, None, 1, None) == rfid.capi.ERR_INVALID
    assert gpu_ctx._lib.rfid_window_moments_of(gpu_ctx._h, g.ctypes.data, -1, None) == rfid.capi.ERR_INVALID
    # more packs than the launch has workgroups (at most eight per compute unit): a workgroup goes round its loop again
    big = np.ascontiguousarray(np.tile(g, (1546, 1))[:17_001])
    ref.assert_equal(gpu_ctx.window_moments(big), ref.expected_of(big), "17 001 windows")


def test_protocol_capacity_and_state_errors(small):
    import rfid
    host, lens, L, stride, refs, want, dev = small
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
        _pass(ctx, dev, L, stride)
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)    # a pass, but nothing enqueued behind it
        ctx.batch_slots_enqueue()                                 # (no inventory workspace: none is needed)
        cases.check_rows(ctx, want, "no inventory")
        ctx.batch_plan_inventory(8)                               # (does not drop the slots workspace)
        ctx.batch_plan_tracks()
        ctx.batch_plan_quality()
        raises(ctx.batch_tracks_enqueue, ERR_STATE)               # (the slots stage is not an inventory: the level is not raised ...)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_slots_enqueue()
        ctx.batch_quality_enqueue()                               # (... nor lowered: the tracks are still this pass's)
        cases.check_rows(ctx, want, "behind the tracks")
        row = np.zeros(len(want[0]) - 1, dtype=rfid.capi.MOMENTS_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_window_moments(ctx._h, 0, row.ctypes.data, len(row), C.byref(n))
        assert rc == ERR_CAPACITY and n.value == len(want[0]) and not row.tobytes().strip(b"\0")
        full = np.zeros(n.value, dtype=rfid.capi.MOMENTS_DTYPE)
        assert ctx._lib.rfid_batch_get_window_moments(ctx._h, 0, full.ctypes.data, len(full), C.byref(n)) == rfid.capi.OK
        ref.assert_equal(full, want[0])
        for s in (2, -1):
            assert ctx._lib.rfid_batch_get_window_moments(ctx._h, s, None, 0, C.byref(n)) == ERR_INVALID
        ctx.batch_plan(2, L)                                      # a new plan drops the workspace
        raises(ctx.batch_slots_enqueue, ERR_STATE)
        raises(lambda: ctx.batch_window_moments(0), ERR_STATE)
        ctx.batch_plan_slots()
        _pass(ctx, dev, L, stride)
        ctx.batch_slots_enqueue()
        cases.check_rows(ctx, want, "new plan")
    finally:
        ctx.close()


def test_classification_agrees_with_the_truth_on_the_five_shapes(oracle_mod, synth_mod):
    """The five shapes at sigma = 0.01: the device's records are the oracle's, classify_slots == SlotTruth for EVERY slot (no slot may
    be left out) and == the restatement of slots_ref; Schoute's estimate on the five-tag shape is 4.82 per round, the suggested Q 2"""
    import rfid
    from rfid import batch as rb
    kept = {}
    for shape in ref.SHAPES:
        t = ref.shape_trace(synth_mod, shape, cases.SIGMA)
        host, lens, L, stride = cases.lay_out([t.samples], odd_stride=False)
        dev = _dev(host, lens)
        ctx = rfid.Context(device=0, fixed_q=shape[0])
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(1, L)
            ctx.batch_plan_slots()
            _pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            rows = ctx.batch_window_moments(0)
        finally:
            ctx.close()
        o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=shape[0]))
        ref.assert_equal(rows, ref.expected(o, oracle_mod.fir(t.samples)), shape)
        got = cases.check_classification(rb, rows, t.slots, shape)
        assert len(got) == shape[2] << shape[0]
        kept[shape] = got
    est = rb.estimate_population(kept[ref.SHAPES[0]]["cls"], 12)
    assert "%.2f" % est == "4.82" and rb.suggest_q(est) == 2


def test_command_line_writes_the_slots_csv_and_a_line_per_file(oracle_mod, synth_mod, tmp_path):
    """python -m rfid.batch --slots OUT.csv on two trace files, in a fresh child process: exit status 0, one slots line per file
    behind its results block, the CSV's classes are the truth; no inventory is printed (--slots does not imply it)"""
    from rfid import batch as rb
    paths, slots, starts, truth = [], [], [], []
    for k, shape in enumerate((ref.SHAPES[4], (2, (1, 2, 3), 3, 21))):
        t = ref.shape_trace(synth_mod, shape, cases.SIGMA)
        p = str(tmp_path / ("trace%d.bin" % k))
        rb.write_trace_file(p, t.samples)
        paths.append(p)
        o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=2))
        rows = ref.expected(o, oracle_mod.fir(t.samples), k)
        slots.append(rb.classify_slots(rows))
        starts.append(np.asarray(o.open_idx))
        truth.append(ref.truth(t.slots))
        assert [(int(s["cls"]), int(s["answered"])) for s in slots[-1]] == truth[-1]
    csv = str(tmp_path / "slots.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    r = subprocess.run([sys.executable, "-m", "rfid.batch", "--fixed-q", "2", "--slots", csv] + paths, env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert " tags\n" not in out and "EPC windows :" not in out
    rule = " --------------------------\n"
    for k, p in enumerate(paths):
        line = rb.format_slots(slots[k], 2)
        assert out.count(line) == 1, (line, out)
        at = out.index(line)
        assert out[at - len(rule):at] == rule and out.index(p + "\n") < at
        assert k + 1 == len(paths) or at < out.index(paths[k + 1] + "\n")
        f = dict(zip(line.split()[1::3], line.split()[3::3]))
        n_true = [sum(c == v for c, _ in truth[k]) for v in (0, 1, 2)]
        assert [int(f[n]) for n in ("slots", "empty", "single", "collided")] == [len(truth[k])] + n_true, (line, f)
    text = open(csv).read()
    assert text == rb.format_slots_csv(slots, starts, paths)
    lines = text.splitlines()
    assert lines[0] == rb.SLOTS_HEADER and len(lines) == 1 + sum(map(len, truth))
    names = ("empty", "single", "collided")
    i = 1
    for k, p in enumerate(paths):
        for j, (cls, answered) in enumerate(truth[k]):
            f = lines[i].split(",")
            assert f[:3] == [p, str(j), str(2 * j)] and f[4] == names[cls] and int(f[8]) == answered, (lines[i], cls, answered)
            assert abs(float(f[3]) - starts[k][2 * j] / 400e3) <= 1e-9 and float(f[5]) >= float(f[6])
            i += 1

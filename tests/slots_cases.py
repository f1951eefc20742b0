"""What the slots stage's cases (tests/slots_suite.py, on both sides; tests/test_slots_emu.py and tests/test_gpu_slots.py, on one) are
built from: their inputs, cut and laid out by the ORACLE alone, and the checks that are the same wherever the records come from.
Expected records come from tests/slots_ref.py."""
import ctypes as C

import numpy as np

import slots_ref as ref
from stage_backend import lay_out, oracle_pass

SIGMA = 0.01


def cut_behind(oracle_mod, x, fixed_q, keep):
    """the raw length at which trace x ends 40 decimated samples behind the close of its window keep - 1"""
    o = oracle_mod.run_trace(x, oracle_mod.config(fixed_q=fixed_q))
    assert o.n_windows >= keep
    k = keep - 1
    return 5 * int(o.open_idx[k] + (1370 if k & 1 else 250) + 40)


def oracle_of(oracle_mod, host, lens, fixed_q, **cfg):
    """-> (oracle Results, expected moments per trace)"""
    refs, ys = oracle_pass(oracle_mod, host, lens, fixed_q, **cfg)
    return refs, ref.expected_batch(refs, ys)


def ragged_batch(oracle_mod, synth_mod):
    """FIXED_Q = 2, three traces: five tags / 12 rounds / seed 1, four tags / 4 rounds / seed 11 and a 1-round trace, sigma = 0.01,
    cut behind their windows 93, 30 and 7 (no count a multiple of 8, two of them odd: a last RN16 without its EPC), odd row stride"""
    ts = [ref.shape_trace(synth_mod, ref.SHAPES[0], SIGMA).samples, ref.shape_trace(synth_mod, ref.SHAPES[4], SIGMA).samples,
          synth_mod.make_trace(n_rounds=1, fixed_q=2, tag_ids=(1, 2, 3, 4), seed=5, sigma=SIGMA).samples]
    host, lens, L, stride = lay_out(ts, odd_stride=True)
    for b, keep in enumerate((93, 30, 7)):
        lens[b] = cut_behind(oracle_mod, ts[b], 2, keep)
    refs, want = oracle_of(oracle_mod, host, lens, 2)
    assert [o.n_windows for o in refs] == [93, 30, 7] and stride & 1
    return host, lens, L, stride, refs, want


def check_rows(ctx, want, what="", extra=3):
    """every trace's row of the last batch_slots_enqueue against the oracle's, the rows behind it zero, nrows == n_windows_used
    -> the bytes of all rows"""
    st = ctx.batch_stats()
    blob = b""
    for b, w in enumerate(want):
        r = ctx.batch_window_moments(b, extra=extra)
        assert len(r) == int(st[b]["n_windows_used"]) + extra == len(w) + extra, (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, b)
        ref.assert_equal(r[: len(w)], w, (what, b))
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_window_moments(ctx._h, b, None, 0, C.byref(n)) in (0, -5) and n.value == len(w)
        blob += r.tobytes()
    return blob


def crafted_windows(oracle_mod, host, lens, refs, stream=0, seq=5, seed=3):
    """eleven windows of 240 samples for the per-call path: all zero; a first sample of (-0.0, -0.0); one huge sample among small
    ones (the order of summation matters); window `seq` of a batch trace, gated by the oracle alone; seven of noise"""
    F = np.float32
    rng = np.random.default_rng(seed)
    g = np.zeros((11, ref.N), dtype=np.complex64)
    g[1, 0] = complex(-0.0, -0.0)
    gv = g.view(F).reshape(11, ref.N, 2)
    gv[1, 0, 0] = F(-0.0); gv[1, 0, 1] = F(-0.0)
    small = (rng.standard_normal((ref.N, 2)) * 1e-3).astype(F)
    gv[2] = small
    gv[2, 100] = (F(1000.0), F(-300.0))
    y = oracle_mod.fir(host[stream, : lens[stream]])
    o = refs[stream]
    a = int(o.open_idx[seq])
    dc = np.complex64(o.dc[seq])
    gv[3, :, 0] = np.ascontiguousarray(y.real[a:a + ref.N]).astype(F) - F(dc.real)
    gv[3, :, 1] = np.ascontiguousarray(y.imag[a:a + ref.N]).astype(F) - F(dc.imag)
    gv[4:] = (rng.standard_normal((7, ref.N, 2)) * 0.05).astype(F)
    assert np.signbit(gv[1, 0]).all()
    return g


def check_crafted(ctx, g, batch_record):
    """the per-call records of crafted_windows() against the definition; the window cut from a batch trace equals the batch stage's
    record apart from stream / seq / flags"""
    got = ctx.window_moments(g)
    want = ref.expected_of(g)
    ref.assert_equal(got, want, "per call")
    sums = ("sx", "sy", "sxx", "sxy", "syy")
    for k in (0, 1):
        assert all(got[f][k].tobytes() == b"\0\0\0\0" for f in sums), (k, got[k])          # (+0.0, not -0.0)
    # the huge sample makes the order matter (by the definition alone): the same terms from the far end give another sum
    x = np.ascontiguousarray(g[2].real).astype(np.float32)
    assert ref.in_order(x[None, :])[0].tobytes() != ref.in_order(np.ascontiguousarray(x[None, ::-1]))[0].tobytes()
    for f in sums:
        assert got[f][3].tobytes() == batch_record[f].tobytes(), (f, got[3], batch_record)
    assert (got["stream"] == 0).all() and np.array_equal(got["seq"], np.arange(len(g))) and (got["flags"] == 0).all()
    # fewer windows than a pack, one window, none
    ref.assert_equal(ctx.window_moments(g[:3]), want[:3], "three")
    ref.assert_equal(ctx.window_moments(g[2]), ref.expected_of(g[2:3]), "one")
    assert len(ctx.window_moments(g[:0])) == 0


def other_stage_outputs(ctx, n):
    """everything else a pass and its stages report, as bytes (inventory, tracks, quality and repair of the last pass are enqueued here)"""
    ent, counts = ctx.batch_inventory()
    reads, off = ctx.batch_tracks()
    q = ctx.batch_quality()
    rep = ctx.batch_repair()
    w, r, _ = ctx.batch_windows()
    parts = [ent, counts, reads, off, q, rep, ctx.batch_stats(), w, r]
    for b in range(n):
        parts += [ctx.batch_window_quality(b, extra=2), ctx.batch_window_repairs(b, extra=2)]
    return [np.ascontiguousarray(p).tobytes() for p in parts]


def plan_all(ctx, n, L, max_tags=8, slots=True):
    ctx.batch_plan(n, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_tracks()
    ctx.batch_plan_quality()
    ctx.batch_plan_repair()
    if slots:
        ctx.batch_plan_slots()


def check_classification(rb, rows, truth_slots, shape):
    """classify_slots of one trace's device (or emulator) records against SlotTruth and against the restatement of slots_ref"""
    got = rb.classify_slots(rows)
    want = ref.classify(rows)
    true = ref.truth(truth_slots)
    assert len(got) == len(want) == len(true) == len(truth_slots), (shape, len(got), len(true))
    # the two hypot()s may differ in the last place of d; l1, l2 and the floor are (tr +- d) / 2 / n: within a few ulp of the largest l1
    tol = 1e-15 * max(ref.eig(r)[0] for r in rows)
    for k, (g, w, t) in enumerate(zip(got, want, true)):
        assert (int(g["cls"]), int(g["answered"]), int(g["crc_ok"])) == w[:3], (shape, k, g, w)
        assert all(abs(float(g[f]) - v) <= tol for f, v in zip(("l1", "l2", "floor"), w[3:])), (shape, k, g, w)
        assert (int(g["cls"]), int(g["answered"])) == t, (shape, k, g, t, truth_slots[k])
        assert int(g["seq"]) == 2 * k
    return got


def five_shapes(backend, oracle_mod, synth_mod):
    """the five shapes at sigma = 0.01, each through a pass of its own context; the records are the oracle's
    -> per shape (trace, records)"""
    import rfid
    out = []
    for shape in ref.SHAPES:
        t = ref.shape_trace(synth_mod, shape, SIGMA)
        host, lens, L, stride = lay_out([t.samples])
        dev = backend.put(host, lens)
        ctx = rfid.Context(device=0, fixed_q=shape[0])
        try:
            ctx.batch_set_long_stream(0)
            ctx.batch_plan(1, L)
            ctx.batch_plan_slots()
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            rows = ctx.batch_window_moments(0)
        finally:
            ctx.close()
        o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=shape[0]))
        ref.assert_equal(rows, ref.expected(o, oracle_mod.fir(t.samples)), shape)
        out.append((t, rows))
    return out


def check_five_shapes(rb, classified):
    """classify_slots == SlotTruth for EVERY slot of every shape of five_shapes() (no slot may be left out) and == the restatement
    of slots_ref; Schoute's estimate on the five-tag shape is 4.82 per round, the suggested Q 2"""
    for shape, (t, rows) in zip(ref.SHAPES, classified):
        got = check_classification(rb, rows, t.slots, shape)
        assert len(got) == shape[2] << shape[0]
    est = rb.estimate_population(rb.classify_slots(classified[0][1])["cls"], 12)
    assert "%.2f" % est == "4.82" and rb.suggest_q(est) == 2

"""What the commands stage's cases (tests/commands_suite.py, on both sides; tests/test_commands_emu.py and tests/test_gpu_commands.py,
on one) are built from: their inputs, cut and laid out by the ORACLE alone, and the checks that are the same wherever the records come
from.  Expected records come from tests/commands_ref.py; what every window's command must BE comes from the synthesiser's slot table."""
import ctypes as C

import numpy as np

import commands_ref as ref
import slots_cases
import slots_ref
from stage_backend import lay_out

SIGMA = slots_cases.SIGMA
SPAN = ref.SPAN


def oracle_of(oracle_mod, host, lens, fixed_q, **cfg):
    """-> (oracle Results, expected commands per trace)"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=fixed_q, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ref.expected_batch(refs, ys)


def ragged_batch(oracle_mod, synth_mod):
    """slots_cases.ragged_batch (three traces cut behind their windows 93, 30 and 7, odd row stride) with the commands the oracle's
    openings give, and the three traces' plans (the truth)
    -> (host, lens, L, stride, oracle Results, expected records per trace, plans per trace)"""
    host, lens, L, stride, refs, _ = slots_cases.ragged_batch(oracle_mod, synth_mod)
    want = ref.expected_batch(refs, [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))])
    plans = [synth_mod.make_trace(n_rounds=s[2], fixed_q=s[0], tag_ids=s[1], seed=s[3], sigma=SIGMA, render=False)
             for s in (slots_ref.SHAPES[0], slots_ref.SHAPES[4], (2, (1, 2, 3, 4), 1, 5))]
    assert [len(w) for w in want] == [93, 30, 7]
    return host, lens, L, stride, refs, want, plans


def check_rows(ctx, want, what="", extra=3):
    """every trace's row of the last batch_commands_enqueue against the oracle's, the rows behind it zero, nrows == n_windows_used
    -> the bytes of all rows"""
    st = ctx.batch_stats()
    blob = b""
    for b, w in enumerate(want):
        r = ctx.batch_window_commands(b, extra=extra)
        assert len(r) == int(st[b]["n_windows_used"]) + extra == len(w) + extra, (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, b)
        ref.assert_equal(r[: len(w)], w, (what, b))
        n = C.c_int64(-1)
        assert ctx._lib.rfid_batch_get_window_commands(ctx._h, b, None, 0, C.byref(n)) in (0, -5) and n.value == len(w)
        blob += r.tobytes()
    return blob


def table_rows(ctx, L_plan, stream=0):
    """the rows the table has per trace (wmax of a plan for traces of L_plan raw samples: the closest the gate can open windows is
    250 + 96 + 1 decimated samples), checked against the library: a fetch copies min(cap, wmax) rows and leaves the rest alone"""
    from rfid import _capi as capi
    wmax = (L_plan // 5) // 347 + 2
    out = np.zeros(wmax + 1, dtype=capi.COMMAND_DTYPE)
    out.view(np.uint8)[:] = 0xFF
    n = C.c_int64(0)
    assert ctx._lib.rfid_batch_get_window_commands(ctx._h, stream, out.ctypes.data, len(out), C.byref(n)) == 0
    assert out[-1:].tobytes() == b"\xff" * 48 and out[-2:-1].tobytes() == b"\0" * 48 and n.value < wmax, (wmax, n.value)
    return wmax


def plan_all(ctx, n, L, commands=True):
    slots_cases.plan_all(ctx, n, L, slots=True)
    if commands:
        ctx.batch_plan_commands()


def other_stage_outputs(ctx, n):
    """everything else a pass and its stages report, the slots stage's moments included, as bytes"""
    parts = slots_cases.other_stage_outputs(ctx, n)
    ctx.batch_slots_enqueue()
    return parts + [ctx.batch_window_moments(b, extra=2).tobytes() for b in range(n)]


# ---- a clipped span: a trace whose first window opens less than 704 samples behind the trace's start ------------------------
def clipped_batches(oracle_mod, synth_mod, start=660):
    """The 1-round FIXED_Q = 2 trace with its leading carrier cut so that the oracle still finds the first window, at `start`
    (500..703): its span is clipped at the trace's start.  With it a neighbour (the same trace, uncut: the longest of the batch,
    so the END of its row lies right below the clipped trace's row when that is at index 1) in two forms -- as it is (its row
    ends in carrier: high) and with its last 4 000 raw samples zeroed (low).
    -> list of (host, lens, L, stride, expected records per trace, index of the clipped trace)"""
    full = synth_mod.make_trace(n_rounds=1, fixed_q=2, tag_ids=(1, 2, 3, 4), seed=5, sigma=SIGMA).samples
    o = oracle_mod.run_trace(full, oracle_mod.config(fixed_q=2))
    cut = full[5 * (int(o.open_idx[0]) - start):]
    oc = oracle_mod.run_trace(cut, oracle_mod.config(fixed_q=2))
    assert oc.n_windows == o.n_windows == 8 and int(oc.open_idx[0]) == start and 500 <= start < SPAN          # (checked on the CPU)
    dark = full.copy()
    dark[-4000:] = 0
    out = []
    for order in ((cut, full), (full, cut), (dark, cut)):
        host, lens, L, stride = lay_out(list(order))
        assert L == len(full)
        refs, want = oracle_of(oracle_mod, host, lens, 2)
        k = 0 if order[0] is cut else 1
        w = want[k]
        assert int(w["flags"][0]) & 16 and not (w["flags"][1:] & 16).any() and int(w["cmd"][0]) == ref.QUERY and int(w["flags"][0]) & 2
        out.append((host, lens, L, stride, want, k))
    a, b, c = (o[4][o[5]].copy() for o in out)
    for r in (a, b, c):
        r["stream"] = 0
    assert a.tobytes() == b.tobytes() == c.tobytes()      # (by the definition, the record does not depend on the neighbour)
    return out


# ---- crafted spans for the per-call path ---------------------------------------------------------------------------------------
def span_of(low, hi=1.0, lo=0.1):
    """low[704] (bool) -> a span whose samples are lo where low and hi elsewhere (against a level of 1 + 0j: thr = 0.25)"""
    s = np.full(SPAN, hi, dtype=np.complex64)
    s[np.asarray(low, dtype=bool)] = lo
    return s


def low_from_edges(edges, width=2):
    """rising edges at the given positions: `width` low samples in front of each (fewer at the span's start)"""
    low = np.zeros(SPAN, dtype=bool)
    for p in edges:
        assert 1 <= p < SPAN
        low[max(p - width, 0):p] = True
    return low


def pie_edges(first, d0, rtcal, trcal, bits, zero=10, one=20):
    """the rising edges of a PIE command whose delimiter's edge is at `first`"""
    e = [first, first + d0, first + d0 + rtcal]
    if trcal:
        e.append(e[-1] + trcal)
    for b in bits:
        e.append(e[-1] + (one if b else zero))
    return e


def crafted_spans(synth_mod, seed=4):
    """-> (spans [n][704], levels [n], names [n]): the smallest shapes at which the kernel can go wrong"""
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, low=None, span=None, level=1.0 + 0.0j):
        cases.append((name, span_of(low) if span is None else np.asarray(span, dtype=np.complex64), np.complex64(level)))

    # the carry between ballots: edges at p = 1, at every multiple of 64 and at 703 (low only at the sample before each)
    low = np.zeros(SPAN, dtype=bool)
    low[[0, 702] + [64 * k - 1 for k in range(1, 11)]] = True
    add("edges at 1, 64 k, 703", low)
    add("edge at every multiple of 64 alone", low_from_edges([64 * k for k in range(1, 11)], 1))
    add("low at 63 and 64: no edge at 64", low_from_edges([65, 129], 2))
    low = low_from_edges(pie_edges(300, 10, 28, 0, [0, 0, 0, 0]))
    low[690:] = True
    add("a span that ends low", low)
    low = np.zeros(SPAN, dtype=bool)
    low[0] = True
    add("low only at 0", low)
    add("all low", np.ones(SPAN, dtype=bool))
    add("all high", np.zeros(SPAN, dtype=bool))
    for n in (64, 65, 80):
        add("%d edges" % n, low_from_edges([40 + 8 * k for k in range(n)], 3))
    add("65 edges, a long gap behind the first", low_from_edges([5] + [150 + 8 * k for k in range(64)], 3))
    add("gap of 120", low_from_edges([100, 220, 230, 258, 268, 278]))
    add("gap of 121", low_from_edges([100, 221, 231, 259, 269, 279]))
    add("gaps of 121 twice", low_from_edges([100, 221, 231, 352, 362, 390, 400]))
    add("2 d == rtcal", low_from_edges(pie_edges(200, 10, 28, 0, [0, 1, 0], zero=14, one=15)))
    add("d3 == rtcal", low_from_edges(pie_edges(200, 10, 28, 0, [1, 0, 0, 1], zero=10, one=28)))
    add("d3 == rtcal + 1", low_from_edges(pie_edges(200, 10, 28, 0, [1, 0, 0, 1], zero=10, one=29)))
    for m in (1, 2, 3):
        add("m = %d" % m, low_from_edges([400, 410, 438][:m]))
    add("m = 4 with a trcal", low_from_edges([400, 410, 438, 518]))
    add("not a frame-sync: 2 d0 > rtcal", low_from_edges(pie_edges(200, 20, 28, 0, [0, 0, 0, 0])))
    bits40 = rng.integers(0, 2, 40).tolist()
    add("40 data symbols", low_from_edges(pie_edges(60, 5, 14, 0, bits40, zero=5, one=9)))
    add("58 data symbols behind a trcal", low_from_edges(pie_edges(20, 5, 14, 40, rng.integers(0, 2, 58).tolist(), zero=5, one=9)))
    add("nak", low_from_edges(pie_edges(300, 10, 28, 0, [1, 1, 0, 0, 0, 0, 0, 0])))
    add("nak with a wrong bit", low_from_edges(pie_edges(300, 10, 28, 0, [1, 1, 0, 0, 0, 1, 0, 0])))
    add("query adjust", low_from_edges(pie_edges(300, 10, 28, 0, [1, 0, 0, 1, 0, 1, 1, 1, 0])))
    add("query rep", low_from_edges(pie_edges(300, 10, 28, 0, [0, 0, 1, 0])))
    add("ack", low_from_edges(pie_edges(200, 10, 28, 0, [0, 1] + rng.integers(0, 2, 16).tolist())))
    q = [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1]
    add("query, Q = 11", low_from_edges(pie_edges(60, 10, 28, 80, q + synth_mod.crc5(q))))
    bad = synth_mod.crc5(q)
    bad[2] ^= 1
    add("query with a wrong CRC-5", low_from_edges(pie_edges(60, 10, 28, 80, q + bad)))
    add("query bits without a trcal", low_from_edges(pie_edges(60, 10, 28, 0, [0] + q + synth_mod.crc5(q))))
    # a sample exactly at thr is high: level (2, 0) -> thr = 1.0f; |(1, 0)|^2 == 1.0f, the float below it gives less
    low = low_from_edges(pie_edges(300, 10, 28, 0, [0, 0, 0, 0]))
    add("samples exactly at thr", span=span_of(low, hi=2.0, lo=1.0), level=2.0)
    add("samples one ulp below thr", span=span_of(low, hi=2.0, lo=float(np.nextafter(np.float32(1.0), np.float32(0.0)))), level=2.0)
    add("a level of 0", span=span_of(low, hi=1.0, lo=0.0), level=0.0)
    add("a level of 0, all samples 0", span=np.zeros(SPAN, dtype=np.complex64), level=0.0)
    # samples within a few ulp of thr on both sides: a fused multiply-add would decide some of them differently
    ang = rng.uniform(0, 2 * np.pi, SPAN)
    near = (np.sqrt(0.5) * (1.0 + rng.integers(-4, 5, SPAN) * 6e-8) * np.exp(1j * ang)).astype(np.complex64)
    add("samples within ulps of thr", span=near, level=1.0 + 1.0j)
    names = [c[0] for c in cases]
    return np.stack([c[1] for c in cases]), np.array([c[2] for c in cases], dtype=np.complex64), names


def check_crafted(ctx, synth_mod):
    """the per-call records of crafted_spans() against the definition, and that the cases ARE what their names say
    -> (spans, levels, records)"""
    spans, levels, names = crafted_spans(synth_mod)
    want = ref.expected_of(spans, levels)
    by = dict(zip(names, want))
    f = lambda name, *fields: tuple(int(by[name][x]) for x in fields)
    # the reference itself on the cases whose answer is plain
    assert f("edges at 1, 64 k, 703", "n_edges", "n_syms", "end", "cmd") == (12, 12, 703, ref.UNKNOWN)
    assert f("edge at every multiple of 64 alone", "n_edges", "n_syms", "end") == (10, 10, 640)
    assert f("low at 63 and 64: no edge at 64", "n_edges", "end") == (2, 129)
    assert f("a span that ends low", "n_edges", "cmd", "end") == (7, ref.QUERY_REP, 300 + 38 + 40)
    assert f("low only at 0", "n_edges", "n_syms", "end", "cmd") == (1, 1, 1, ref.NONE)
    assert f("all low", "n_edges", "n_syms") == f("all high", "n_edges", "n_syms") == (0, 0)
    assert [f("%d edges" % n, "n_edges", "n_syms", "flags") for n in (64, 65, 80)] == [(64, 64, 32), (65, 64, 40), (80, 64, 40)]
    assert f("65 edges, a long gap behind the first", "n_edges", "n_syms") == (65, 64)
    assert f("gap of 120", "n_syms", "d0", "rtcal") == (6, 120, 10) and f("gap of 121", "n_syms", "d0", "rtcal") == (5, 10, 28)
    assert f("gaps of 121 twice", "n_syms", "n_edges") == (4, 7)
    assert f("2 d == rtcal", "n_bits", "bits") == (3, 0b010) and f("d3 == rtcal", "trcal", "n_bits", "bits") == (0, 4, 0b1001)
    assert f("d3 == rtcal + 1", "trcal", "n_bits") == (29, 3)
    assert [f("m = %d" % m, "n_syms", "cmd", "d0", "rtcal") for m in (1, 2, 3)] == [(1, 0, 0, 0), (2, 0, 10, 0), (3, ref.UNKNOWN, 10, 28)]
    assert f("m = 4 with a trcal", "trcal", "n_bits", "cmd") == (80, 0, ref.UNKNOWN)
    assert f("not a frame-sync: 2 d0 > rtcal", "cmd", "flags") == (ref.QUERY_REP, 32)
    assert f("40 data symbols", "n_bits", "n_syms") == (40, 43) and f("58 data symbols behind a trcal", "n_bits", "n_syms", "trcal") == (58, 62, 40)
    assert f("nak", "cmd") == (ref.NAK,) and f("nak with a wrong bit", "cmd") == (ref.UNKNOWN,) and f("query adjust", "cmd") == (ref.QUERY_ADJUST,)
    assert f("query rep", "cmd", "n_bits") == (ref.QUERY_REP, 4) and f("ack", "cmd", "flags") == (ref.ACK, 0)
    assert f("query, Q = 11", "cmd", "flags") == (ref.QUERY, 2) and ref.fields_of(by["query, Q = 11"])[1] == 11
    assert f("query with a wrong CRC-5", "cmd", "flags") == (ref.QUERY, 0) and f("query bits without a trcal", "cmd") == (ref.UNKNOWN,)
    assert f("samples exactly at thr", "n_edges") == (0,) and f("samples one ulp below thr", "n_edges", "cmd") == (7, ref.QUERY_REP)
    assert f("a level of 0", "n_edges") == f("a level of 0, all samples 0", "n_edges") == (0,)
    assert f("samples within ulps of thr", "n_edges")[0] > 64
    got = ctx.commands_of(spans, levels)
    for k, name in enumerate(names):
        ref.assert_equal(got[k:k + 1], want[k:k + 1], name)
    ref.assert_equal(got, want, "per call")
    assert (got["stream"] == 0).all() and np.array_equal(got["seq"], np.arange(len(spans))) and not (got["flags"] & (1 | 4 | 16)).any()
    # fewer, one, none
    ref.assert_equal(ctx.commands_of(spans[:3], levels[:3]), want[:3], "three")
    ref.assert_equal(ctx.commands_of(spans[5:6], levels[5:6]), ref.expected_of(spans[5:6], levels[5:6]), "one")
    assert len(ctx.commands_of(spans[:0], levels[:0])) == 0
    return spans, levels, want


def check_span_of_a_batch_window(ctx, oracle_mod, host, lens, refs, batch_rows, stream=0, seq=5):
    """window `seq` of a batch trace, its span cut by the oracle alone, through the per-call path: the batch stage's record apart
    from stream, seq and the flag bits 0, 2 and 4"""
    y = oracle_mod.fir(host[stream, : lens[stream]])
    a = int(refs[stream].open_idx[seq])
    assert a >= SPAN
    got = ctx.commands_of(y[a - SPAN:a][None, :], np.array([refs[stream].dc[seq]], dtype=np.complex64))[0]
    want = batch_rows[seq].copy()
    assert int(want["cmd"]) == ref.ACK and int(want["flags"]) & 1
    want["stream"], want["seq"] = 0, 0
    want["flags"] &= ~(1 | 4 | 16)
    assert got.tobytes() == want.tobytes(), (got, want)

"""What the repair stage's cases (tests/repair_suite.py, on both sides; tests/test_repair_emu.py and tests/test_gpu_repair.py, on one)
are built from: their small inputs, with what the ORACLE alone says about them, and the plan and the check that are the same wherever
the records come from.  Expected records come from tests/repair_ref.py, the crafted windows from tests/repair_windows.py.

The traces are at the sensitivity edge: sigma = 0.02, T1 jitter of 3 raw samples, tag amplitude A = 0.014 .. 0.018."""
import numpy as np

import repair_ref as ref
from stage_backend import lay_out, oracle_pass

TRACES = dict(      # name -> (A, make_trace arguments)
    edge=(0.016, dict(fixed_q=0, tag_ids=(0x27,), seed=1, n_rounds=24)),
    lost=(0.014, dict(fixed_q=0, tag_ids=(0x27,), seed=15, n_rounds=3)),
    mixed=(0.018, dict(fixed_q=2, tag_ids=(0x27, 0x27, 0x31), seed=2, n_rounds=8)),
)


def make(synth_mod, name):
    A, kw = TRACES[name]
    return synth_mod.make_trace(sigma=0.02, t1_jitter_raw=3, h=A * np.exp(2.1j), **kw).samples


def single_traces(oracle_mod, synth_mod):
    """name -> (host, lens, L, stride, fixed_q, oracle result, (packed, [rows]), y) of the three traces, each on its own"""
    out = {}
    for name, (A, kw) in TRACES.items():
        host, lens, L, stride = lay_out([make(synth_mod, name)])
        refs, ys = oracle_pass(oracle_mod, host, lens, kw["fixed_q"])
        out[name] = (host, lens, L, stride, kw["fixed_q"], refs[0], ref.expected_batch(oracle_mod, refs, ys), ys[0])
    return out


def ragged_batch(oracle_mod, synth_mod):
    """the three traces and a pure-carrier trace in the middle as one ragged batch, FIXED_Q = 2 for all of them
    -> (host, lens, L, stride, oracle Results, matched-filter outputs, (packed, rows))"""
    ts = [make(synth_mod, "mixed"), make(synth_mod, "edge"), None, make(synth_mod, "lost")]
    ts[2] = np.full(len(ts[0]) // 2, np.complex64(0.8 + 0.1j))
    host, lens, L, stride = lay_out(ts)
    refs, ys = oracle_pass(oracle_mod, host, lens, 2)
    want = ref.expected_batch(oracle_mod, refs, ys)
    assert [len(r) for r in want[1]] == [32, 24, 0, 3] and [int((r["n_flips"] > 0).sum()) for r in want[1]] == [6, 14, 0, 3]
    assert np.array_equal(want[0]["stream"], np.repeat([0, 1, 3], [6, 14, 3])) and (np.diff(want[0]["seq"])[np.diff(want[0]["stream"]) == 0] > 0).all()
    return host, lens, L, stride, refs, ys, want


def frame_sent_wrong(oracle_mod, synth_mod):
    """FIXED_Q = 0, one tag, five rounds, one bit of round 3's EPC frame flipped by the TAG -> (host, lens, L, stride, (packed, [rows])):
    by the reference the window stays unrepaired"""
    x = synth_mod.make_trace(n_rounds=5, fixed_q=0, tag_ids=(0x27,), seed=7, sigma=0.02, corrupt_rounds=(3,)).samples
    host, lens, L, stride = lay_out([x])
    want = ref.expected_batch(oracle_mod, *oracle_pass(oracle_mod, host, lens, 0))
    rows = want[1][0]
    assert (rows["flags"] & 1).tolist() == [1, 1, 0, 1, 1] and not rows["n_flips"].any() and len(want[0]) == 0
    return host, lens, L, stride, want


def summary(rows):
    """-> (EPC windows, verified, failed, [repaired by 1, 2, 3 flips])"""
    ok = (rows["flags"] & 1) == 1
    return len(rows), int(ok.sum()), int((~ok).sum()), np.bincount(rows["n_flips"], minlength=4)[1:].tolist()


def plan(ctx, n, L, max_tags=8):
    ctx.batch_plan(n, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_repair()


def check(ctx, want, what="", extra=3):
    """inventory + repair of the last pass; the packed records and every trace's row against the oracle's, the `extra` rows behind a
    row zero, nrows == n_windows_used // 2 -> all the bytes"""
    w_packed, w_rows = want
    ctx.batch_inventory_enqueue()
    got = ctx.batch_repair()
    ref.assert_equal(got, w_packed, what)
    st = ctx.batch_stats()
    blob = got.tobytes()
    for b, w in enumerate(w_rows):
        r = ctx.batch_window_repairs(b, extra=extra)
        assert len(r) == int(st[b]["n_windows_used"]) // 2 + extra == len(w) + extra, (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, "rows behind the trace's", b)
        ref.assert_equal(r[: len(w)], w, (what, "row", b))
        blob += r.tobytes()
    return blob

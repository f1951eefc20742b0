"""What the quality stage's cases (tests/quality_suite.py, on both sides; tests/test_quality_emu.py and tests/test_gpu_quality.py, on
one) are built from: their small inputs, with what the ORACLE alone says about them, and the plan and the check that are the same
wherever the records come from.  Expected records come from tests/quality_ref.py.

The traces are those of tests/test_inventory_emu.py: seeds 104 (4 rounds) and 112 (3 rounds), FIXED_Q = 2, tags (0x27, 0x27, 0x31),
sigma = 0.02: a third of the slots are empty or collided, and the reference ACKs every one of them."""
import numpy as np

import quality_ref as ref
from stage_backend import lay_out, oracle_pass

TAGS = (0x27, 0x27, 0x31)
SEEDS = ((104, 4), (112, 3))       # (seed, inventory rounds) per trace


def ragged_batch(oracle_mod, synth_mod):
    """-> (host, lens, L, stride, oracle Results, matched-filter outputs, (packed, rows)) of the two traces, the first cut short"""
    ts = [synth_mod.make_trace(n_rounds=n, fixed_q=2, tag_ids=TAGS, seed=seed, sigma=0.02, t1_jitter_raw=3).samples for seed, n in SEEDS]
    host, lens, L, stride = lay_out(ts, shorten=777)
    refs, ys = oracle_pass(oracle_mod, host, lens, 2)
    packed, rows = ref.expected_batch(refs, ys)
    # the input does what the case is about, by the oracle alone: every trace holds failed EPC windows next to its reads, and the
    # measure tells the two apart with room to spare
    for b, r in enumerate(rows):
        ok = r["flags"] == 1
        snr = ref.snr_db(r)
        assert len(r) == refs[b].n_windows // 2 and (~ok).sum() >= 2 and ok.sum() >= 6, (b, len(r), ok.sum())
        assert snr[ok].min() - snr[~ok].max() > 6.0, (b, snr[ok].min(), snr[~ok].max())
    assert len(packed) == sum(o.state.n_epc_correct for o in refs)
    return host, lens, L, stride, refs, ys, (packed, rows)


def corrupted_trace(oracle_mod, synth_mod):
    """FIXED_Q = 0, one tag, five rounds, one bit of round 3's EPC frame flipped by the tag -> (host, lens, L, stride, (packed, [rows])):
    by the oracle alone that window fails its CRC with an SNR above 15 dB -- a weak or damaged reply, not an empty or collided slot
    (those stay near 0 dB)"""
    x = synth_mod.make_trace(n_rounds=5, fixed_q=0, tag_ids=(0x27,), seed=7, sigma=0.02, corrupt_rounds=(3,)).samples
    host, lens, L, stride = lay_out([x])
    (o,), (y,) = oracle_pass(oracle_mod, host, lens, 0)
    packed, rows = ref.expected(o, y, 0)
    failed = np.flatnonzero(rows["flags"] == 0)
    assert len(rows) == 5 and failed.tolist() == [2], rows["flags"]
    snr = ref.snr_db(rows)
    assert snr[failed[0]] > 15.0, snr
    return host, lens, L, stride, (packed, [rows])


def plan(ctx, n, L, max_tags=8):
    ctx.batch_plan(n, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_tracks()
    ctx.batch_plan_quality()


def stages(ctx):
    """inventory, tracks and quality of the last pass -> (reads, packed quality records), the records aligned with the tracks"""
    ctx.batch_inventory()
    reads, off = ctx.batch_tracks()
    q = ctx.batch_quality()
    assert np.array_equal(q["stream"], reads["stream"]) and np.array_equal(q["seq"], reads["seq"])
    return reads, q


def check(ctx, want, what="", extra=3):
    """inventory + tracks + quality of the last pass; the packed records and every trace's row against the oracle's, the `extra` rows
    behind a row zero, nrows == n_windows_used // 2 -> all the bytes"""
    w_packed, w_rows = want
    reads, q = stages(ctx)
    ref.assert_equal(q, w_packed, what)
    st = ctx.batch_stats()
    blob = q.tobytes()
    for b, w in enumerate(w_rows):
        r = ctx.batch_window_quality(b, extra=extra)
        assert len(r) == int(st[b]["n_windows_used"]) // 2 + extra == len(w) + extra, (what, b, len(r), len(w))
        assert not r[len(w):].tobytes().strip(b"\0"), (what, "rows behind the trace's", b)
        ref.assert_equal(r[: len(w)], w, (what, "row", b))
        blob += r.tobytes()
    return blob

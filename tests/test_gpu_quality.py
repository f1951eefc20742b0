"""The read-quality stage on the device (rfid_batch_plan_quality / rfid_batch_quality / rfid_batch_get_quality /
rfid_batch_get_window_quality): SNR and decision margin of every EPC window of a pass.  Every expected record is worked out in numpy
from the ORACLE alone (tests/quality_ref.py: oracle.fir, the oracle's openings, dc_est and per-window dumps); every comparison is
exact -- integers equal, floats by bit pattern, then the bytes of the whole arrays.  The cases that also run on the wave emulator are
written once, in tests/quality_suite.py, and run here through stage_backend.Device: the smallest shapes at which the kernel can still go
wrong -- a ragged batch, rows behind a cut-off, a plan larger than the batch, a trace without windows, the protocol.  Below them, what
only the device runs, in the shapes of tests/test_gpu_tracks.py: eight traces, 1 024 replicas, one long trace and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stage_backend
from stage_backend import lay_out, oracle_pass
import quality_cases as cases
import quality_ref as ref
import tracks_ref as tref
from quality_suite import *

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIG = (1 << 31) - 2

# six tags, two pairs share the byte tag_reads[] is keyed by
TAGS6 = (0x27, 0x27, 0x31, 0x31, 0x4C, 0x5A)


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Device()


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_ragged_batch_of_eight_traces(backend, oracle_mod, synth_mod, mode):
    """40 rounds, FIXED_Q = 3, six tags, sigma = 0.03; eight traces of different lengths.  The pass three times: byte-identical
    records, packed and per trace; reads and failed windows alike against the oracle."""
    import rfid
    ts = [synth_mod.make_trace(n_rounds=40 - 3 * k, fixed_q=3, tag_ids=TAGS6, seed=900 + k, sigma=0.03, t1_jitter_raw=3).samples for k in range(8)]
    host, lens, L, stride = lay_out(ts)
    dev = backend.put(host, lens)
    packed, rows = ref.expected_batch(*oracle_pass(oracle_mod, host, lens, 3, max_num_queries=BIG))
    # the input does what the case is about, by the oracle alone: every trace holds many failed windows next to its reads
    for b, r in enumerate(rows):
        ok = r["flags"] == 1
        assert ok.sum() >= 12 and (~ok).sum() >= 12, (b, ok.sum(), (~ok).sum())
    ctx = rfid.Context(device=0, fixed_q=3, max_num_queries=BIG)
    try:
        ctx.batch_set_long_stream(mode)
        cases.plan(ctx, 8, L, 16)
        blobs = []
        for rep in range(3):
            backend.run_pass(ctx, dev, L, stride)
            blobs.append(cases.check(ctx, (packed, rows), (mode, rep)))
        assert blobs[0] == blobs[1] == blobs[2]
        print("quality of 8 traces: %.4f ms, %d reads, %d EPC windows; decode %.4f ms" %
              (ctx.batch_quality_ms(), len(packed), sum(map(len, rows)), ctx.batch_timing()["decode_ms"]))
    finally:
        ctx.close()


@pytest.mark.parametrize("overlap", [1, 2], ids=["one-result-set", "two-result-sets"])
def test_1024_replicas_one_failed_window_each(oracle_mod, synth_mod, overlap):
    """The 1 024-trace shape (noise replicas of the 71-round trace, one EPC corrupted): 70 reads and ONE failed window per trace, the
    corrupted round; replicas 0 and 1023 against the oracle.  With two result sets alternating (RFID_OVERLAP=2) the quality of
    every pass is that pass's -- also when the next pass, over other samples, is enqueued before the records are fetched.  The stage
    takes no longer than the decoder of the same pass, which reads the same windows in full and searches them."""
    import rfid
    import torch
    B = 1024
    t = synth_mod.make_trace(n_rounds=71, fixed_q=0, tag_ids=(0x27,), sigma=0.0, seed=7, corrupt_rounds=(36,), noise=False, render=False)
    ctx = rfid.Context(device=0)
    data = other = None
    try:
        ctx.set_knob("overlap", overlap)
        L = ctx.synth_gen2_size(t.plan)
        stride = (L + 1) & ~1
        base = torch.zeros(2 * stride, dtype=torch.float32, device="cuda:0")
        data = torch.empty((B, 2 * stride), dtype=torch.float32, device="cuda:0")
        other = torch.empty((B, 2 * stride), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.synth_gen2_ptr(t.plan, base.data_ptr(), stride)
        ctx.synth_replicas_ptr(base.data_ptr(), L, data.data_ptr(), stride, B, 0.002, 777, first_replica=0)
        ctx.synth_replicas_ptr(base.data_ptr(), L, other.data_ptr(), stride, B, 0.004, 4242, first_replica=0)
        ctx.batch_sync()
        cases.plan(ctx, B, L, 4)
        blobs = []
        for rep in range(3):
            ctx.batch_process_ptr(data.data_ptr(), stride, L, 0)
            reads, q = cases.stages(ctx)
            blobs.append(q.tobytes())
        assert blobs[0] == blobs[1] == blobs[2]
        quality_ms, decode_ms = ctx.batch_quality_ms(), ctx.batch_timing()["decode_ms"]
        print("quality of 1024 traces: %.4f ms; decode of the same pass %.4f ms (ratio %.3f); tracks %.4f ms; inventory %.4f ms" %
              (quality_ms, decode_ms, quality_ms / decode_ms, ctx.batch_tracks_ms(), ctx.batch_inventory_ms()))
        st = ctx.batch_stats()
        assert len(q) == 70 * B and np.array_equal(q["stream"], reads["stream"]) and np.array_equal(q["seq"], reads["seq"])
        assert (q["flags"] == 1).all()
        # every trace's row: 71 EPC windows, exactly one of them failed -- the corrupted round, with the SNR of a read
        table, per = [], q.reshape(B, 70)           # (one tag per trace: a trace's reads are contiguous, in seq order)
        assert (per["stream"] == np.arange(B)[:, None]).all()
        for b in range(B):
            r = ctx.batch_window_quality(b)
            assert len(r) == int(st[b]["n_windows_used"]) // 2 == 71, (b, len(r))
            bad = np.flatnonzero((r["flags"] & 1) == 0)
            assert bad.tolist() == [35] and (r["stream"] == b).all() and np.array_equal(r["seq"], 2 * np.arange(71) + 1), (b, bad)
            assert r[(r["flags"] & 1) == 1].tobytes() == per[b].tobytes(), b
            table.append(r)
        snr = ref.snr_db(np.concatenate(table))
        assert snr.min() > 15.0, snr.min()
        for b in (0, B - 1):
            x = data[b, : 2 * L].cpu().numpy().view(np.complex64)
            o = oracle_mod.run_trace(x)
            w_packed, w_rows = ref.expected(o, oracle_mod.fir(x), b)
            ref.assert_equal(per[b], w_packed, b)
            ref.assert_equal(table[b], w_rows, b)
        # the next pass -- other samples -- enqueued BEFORE this pass's records are fetched: they are still this pass's
        ctx.batch_process_ptr(data.data_ptr(), stride, L, 0)
        ctx.batch_inventory_enqueue()
        ctx.batch_tracks_enqueue()
        ctx.batch_quality_enqueue()
        ctx.batch_process_ptr(other.data_ptr(), stride, L, 0)
        assert ctx.batch_quality_fetch().tobytes() == blobs[0]
        assert ctx.batch_window_quality(B - 1).tobytes() == table[B - 1].tobytes()
        reads2, q2 = cases.stages(ctx)                       # ... and the pass over the other samples gets its own
        assert len(q2) == len(reads2) and q2.tobytes() != blobs[0]
        x = other[3, : 2 * L].cpu().numpy().view(np.complex64)
        o = oracle_mod.run_trace(x)
        w_packed, w_rows = ref.expected(o, oracle_mod.fir(x), 3)
        ref.assert_equal(q2[reads2["stream"] == 3], w_packed, "other")
        ref.assert_equal(ctx.batch_window_quality(3), w_rows, "other")
        assert quality_ms <= decode_ms, (quality_ms, decode_ms)
    finally:
        ctx.close()
        del data, other
        torch.cuda.empty_cache()


def test_one_long_trace(oracle_mod, synth_mod):
    """One trace, FIXED_Q = 4, 2 000 rounds, 8 tags, generated on the device from its slot table: 32 000 EPC windows, half of them
    empty or collided slots, against the oracle over the same samples."""
    import rfid
    import torch
    t = synth_mod.make_trace(n_rounds=2000, fixed_q=4, tag_ids=tuple(0x11 + 0x10 * k for k in range(8)), sigma=0.0, seed=2024,
                             noise=False, render=False)
    ctx = rfid.Context(device=0, fixed_q=4, max_num_queries=BIG)
    try:
        L = ctx.synth_gen2_size(t.plan)
        stride = (L + 1) & ~1
        data = torch.zeros(2 * stride, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.synth_gen2_ptr(t.plan, data.data_ptr(), stride, sigma=0.002, seed=99)
        ctx.batch_sync()
        cases.plan(ctx, 1, L, 64)
        blobs = []
        for rep in range(3):
            ctx.batch_process_ptr(data.data_ptr(), stride, L, 0)
            reads, q = cases.stages(ctx)
            rows = ctx.batch_window_quality(0)
            blobs.append(q.tobytes() + rows.tobytes())
        assert blobs[0] == blobs[1] == blobs[2]
        quality_ms, decode_ms = ctx.batch_quality_ms(), ctx.batch_timing()["decode_ms"]
        st = ctx.batch_stats()
        assert st[0]["n_windows"] == 2 * len(t.slots) > 2048
        get_raw = lambda lo, hi: data[2 * lo: 2 * hi].cpu().numpy().view(np.complex64)
        cfg = oracle_mod.config(fixed_q=4, max_num_queries=BIG)
        s = oracle_mod.Stream(cfg)
        piece = 48_000_000
        for pos in range(0, L, piece):
            s.feed_raw(get_raw(pos, min(pos + piece, L)))
        o = s.result()
        s.close()
        w_packed, w_rows = ref.expected(o, ref.fir_pieces(get_raw, L, oracle_mod), 0)
        assert len(w_packed) > 10000 and (w_rows["flags"] == 0).sum() > 10000
        assert len(rows) == int(st[0]["n_windows_used"]) // 2
        ref.assert_equal(q, w_packed)
        ref.assert_equal(rows, w_rows)
        assert np.array_equal(q["seq"], reads["seq"])
        print("quality of one trace of %d windows: %.4f ms, %d reads, %d failed windows; decode of the same pass %.4f ms (ratio %.3f)" %
              (st[0]["n_windows"], quality_ms, len(q), (rows["flags"] == 0).sum(), decode_ms, quality_ms / decode_ms))
    finally:
        ctx.close()


def test_command_line_prints_the_quality_and_extends_the_csv(oracle_mod, synth_mod, tmp_path):
    """python -m rfid.batch --tracks OUT.csv --quality on two trace files, in a fresh child process: the CSV's two new columns parse back
    to quality_fields of the oracle-derived records, one quality line per file stands behind its results block, and a run without
    --quality prints what it printed before (up to the closing line of the pass, which carries wall times) and writes the CSV it wrote."""
    from rfid import batch as rb
    paths, results, ys = [], [], []
    for k in range(2):
        x = synth_mod.make_trace(n_rounds=6 + k, fixed_q=2, tag_ids=(0x27, 0x27, 0x31), seed=104 + 8 * k, sigma=0.02).samples
        p = str(tmp_path / ("trace%d.bin" % k))
        rb.write_trace_file(p, x)
        paths.append(p)
        results.append(oracle_mod.run_trace(x, oracle_mod.config(fixed_q=2)))
        ys.append(oracle_mod.fir(x))
    ent, counts, reads, off = tref.expected_batch(results)
    packed, rows = ref.expected_batch(results, ys)
    assert len(ent) == 6 and len(reads) >= 12 and all((r["flags"] == 0).sum() >= 2 for r in rows)
    csv, csvq = str(tmp_path / "tracks.csv"), str(tmp_path / "tracks_quality.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    outs = []
    for extra in (["--tracks", csv, "--max-tags", "8"], ["--tracks", csvq, "--quality", "--max-tags", "8"]):
        r = subprocess.run([sys.executable, "-m", "rfid.batch", "--fixed-q", "2"] + extra + paths, env=env, capture_output=True,
                           text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    plain, qual = outs
    # without --quality: the CSV of the tracks stage, byte for byte
    assert open(csv).read() == rb.format_tracks(ent, reads, off, paths)
    # with it: the same text plus one line per file behind its results block
    want_lines = [rb.format_quality(r) for r in rows]
    for line in want_lines:
        assert qual.count(line) == 1 and line not in plain
    stripped = qual
    for line in want_lines:
        stripped = stripped.replace(line, "")
    n_old = plain.rindex("2 traces, ")                       # (the closing line of the pass carries wall times)
    assert stripped[:n_old] == plain[:n_old] and stripped[n_old:].startswith("2 traces, ")
    assert stripped[n_old:].split("\n", 1)[1] == plain[n_old:].split("\n", 1)[1]
    rule = " --------------------------\n"
    for k, (p, line) in enumerate(zip(paths, want_lines)):
        at = qual.index(line)
        assert qual[at - len(rule):at] == rule and qual.index(p + "\n") < at                 # (right behind the file's results block)
        assert k + 1 == len(paths) or at < qual.index(paths[k + 1] + "\n")
    lines = open(csvq).read().splitlines()
    assert lines[0] == rb.TRACKS_QUALITY_HEADER and len(lines) == 1 + len(reads)
    assert "\n".join(lines) + "\n" == rb.format_tracks(ent, reads, off, paths, packed)
    snr, margin = rb.quality_fields(packed)
    old = open(csv).read().splitlines()
    for k, line in enumerate(lines[1:]):
        f = line.split(",")
        assert ",".join(f[:-2]) == old[1 + k]
        assert f[-2] == "%.9g" % snr[k] and f[-1] == "%.9g" % margin[k]
        assert abs(float(f[-2]) - snr[k]) <= 5e-9 * abs(snr[k]) and abs(float(f[-1]) - margin[k]) <= 5e-9 * margin[k]    # (%.9g)

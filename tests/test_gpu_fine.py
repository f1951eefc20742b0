"""The fine-channel stage on the device (rfid_batch_plan_fine / rfid_batch_fine / rfid_batch_get_fine / rfid_batch_get_window_fine and the
per-call rfid_fine_window): the data-aided channel estimate of every EPC window of a pass and of its eight 16-bit segments.  Every
expected record is worked out in numpy from the ORACLE alone (tests/fine_ref.py: oracle.fir, the oracle's openings, dc_est and per-window
dumps); every comparison is exact -- integers equal, floats by bit pattern, then the bytes of the whole arrays."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stage_backend
from stage_backend import lay_out
import fine_cases as cases
import fine_ref as ref
import tracks_ref as tref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIG = (1 << 31) - 2

# six tags, two pairs share the byte tag_reads[] is keyed by
TAGS6 = (0x27, 0x27, 0x31, 0x31, 0x4C, 0x5A)
TAGS3 = (0x27, 0x27, 0x31)


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Device()


def _oracle(oracle_mod, host, lens, fixed_q, **cfg):
    cfg.setdefault("max_num_queries", BIG)
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=fixed_q, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ys


def _plan(ctx, n, L, max_tags):
    ctx.batch_plan(n, L)
    ctx.batch_plan_inventory(max_tags)
    ctx.batch_plan_tracks()
    ctx.batch_plan_fine()


def _enqueue(ctx):
    ctx.batch_inventory_enqueue()
    ctx.batch_tracks_enqueue()
    ctx.batch_fine_enqueue()


def _check(ctx, want, what=""):
    """the stages of the last pass; packed records (aligned with the tracks) and every trace's row against the oracle's -> the bytes"""
    _enqueue(ctx)
    reads, off = ctx.batch_tracks_fetch()
    f = ctx.batch_fine_fetch()
    assert np.array_equal(f["stream"], reads["stream"]) and np.array_equal(f["seq"], reads["seq"]) and np.array_equal(f["start"], reads["start"])
    return cases.check_rows(ctx, want, what)


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_ragged_batch_of_eight_traces(backend, oracle_mod, synth_mod, mode):
    """14 .. 7 rounds, FIXED_Q = 3, six tags, sigma = 0.03; eight traces of different lengths.  The pass three times: byte-identical
    records, packed and per trace; reads and failed windows alike against the oracle."""
    import rfid
    ts = [synth_mod.make_trace(n_rounds=14 - k, fixed_q=3, tag_ids=TAGS6, seed=900 + k, sigma=0.03, t1_jitter_raw=3).samples for k in range(8)]
    host, lens, L, stride = lay_out(ts)
    dev = backend.put(host, lens)
    refs, ys = _oracle(oracle_mod, host, lens, 3)
    want = ref.expected_batch(refs, ys)
    for b, r in enumerate(want[1]):
        ok = r["flags"] == 1
        assert ok.sum() >= 4 and (~ok).sum() >= 4 and len(r) == 8 * (14 - b), (b, ok.sum(), (~ok).sum())
    ctx = rfid.Context(device=0, fixed_q=3, max_num_queries=BIG)
    try:
        ctx.batch_set_long_stream(mode)
        _plan(ctx, 8, L, 16)
        blobs = []
        for rep in range(3):
            backend.run_pass(ctx, dev, L, stride)
            blobs.append(_check(ctx, want, (mode, rep)))
        assert blobs[0] == blobs[1] == blobs[2]
        print("fine of 8 traces: %.4f ms, %d reads, %d EPC windows; decode %.4f ms" %
              (ctx.batch_fine_ms(), len(want[0]), sum(map(len, want[1])), ctx.batch_timing()["decode_ms"]))
    finally:
        ctx.close()


@pytest.mark.parametrize("overlap", [1, 2], ids=["one-result-set", "two-result-sets"])
def test_64_traces_two_passes_back_to_back(backend, oracle_mod, synth_mod, overlap):
    """64 traces of three rounds (FIXED_Q = 1), and the same traces in the opposite order as a second batch.  With two result sets
    alternating (RFID_OVERLAP=2) the records of every pass are that pass's -- also when the next pass, over other samples, is
    enqueued before they are fetched."""
    import rfid
    ts = [synth_mod.make_trace(n_rounds=3, fixed_q=1, tag_ids=TAGS3, seed=500 + k, sigma=0.02, t1_jitter_raw=3).samples for k in range(64)]
    host, lens, L, stride = lay_out(ts)
    dev = backend.put(host, lens)
    host2, lens2, L2, stride2 = lay_out(ts[::-1])
    dev2 = backend.put(host2, lens2)
    assert (L2, stride2) == (L, stride)
    refs, ys = _oracle(oracle_mod, host, lens, 1)
    want = ref.expected_batch(refs, ys)
    want2 = ref.expected_batch(refs[::-1], ys[::-1])
    assert len(want[0]) >= 64 and sum(int((r["flags"] == 0).sum()) for r in want[1]) >= 16 and want[0].tobytes() != want2[0].tobytes()
    ctx = rfid.Context(device=0, fixed_q=1, max_num_queries=BIG)
    try:
        ctx.set_knob("overlap", overlap)
        _plan(ctx, 64, L, 8)
        for rep in range(2):
            backend.run_pass(ctx, dev, L, stride)
            _enqueue(ctx)
            backend.run_pass(ctx, dev2, L, stride)      # (the next pass, before anything is fetched)
            first = cases.check_rows(ctx, want, (overlap, rep, "first"), stats=False)
            second = _check(ctx, want2, (overlap, rep, "second"))
            assert first != second
    finally:
        ctx.close()


def test_crafted_windows_through_fine_window(oracle_mod):
    """rfid_fine_window: 15 noise-free frames at every sync offset, each turning by 0, 0.3 and 0.6 rad over its window -- the segments
    see the turn -- the degenerate windows (all zero, constant, period 7, 38 samples), and a frame whose bits the caller changed"""
    import rfid
    ctx = rfid.Context(device=0)
    try:
        cases.check_crafted_windows(ctx, oracle_mod, rfid)
    finally:
        ctx.close()


def test_per_call_forms_share_one_buffer(oracle_mod, synth_mod):
    """repair_window, window_moments, fine_window and commands_of interleaved in one context, the buffer growing twice: every
    result is what a context of its own returns"""
    import rfid
    cases.check_per_call_forms_share_one_buffer(rfid, oracle_mod, synth_mod)


@pytest.fixture(scope="module")
def small(backend, oracle_mod, synth_mod):
    """the four traces of tests/test_fine_emu.py: 16, 12, 8 and 12 EPC windows"""
    ts = [synth_mod.make_trace(n_rounds=n, fixed_q=2, tag_ids=TAGS3, seed=seed, sigma=0.02, t1_jitter_raw=3).samples
          for seed, n in ((104, 4), (112, 3), (120, 2), (128, 3))]
    host, lens, L, stride = lay_out(ts)
    return host, lens, L, stride, backend.put(host, lens)


def test_windows_behind_the_cut_off(backend, oracle_mod, small):
    """MAX_NUM_QUERIES = 7 reached inside the traces: seven EPC windows each -- a pack that is cut off inside -- behind a pass of the
    same context's twin without the limit; the rows behind the cut-off are zero and the packed array holds no read from there"""
    import rfid
    host, lens, L, stride, dev = small
    refs, ys = _oracle(oracle_mod, host, lens, 2, max_num_queries=7)
    want = ref.expected_batch(refs, ys)
    full = ref.expected_batch(*_oracle(oracle_mod, host, lens, 2))
    assert [len(r) for r in want[1]] == [7, 7, 7, 7] and [len(r) for r in full[1]] == [16, 12, 8, 12] and len(want[0]) < len(full[0])
    for mq, w in ((BIG, full), (7, want)):
        ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=mq)
        try:
            _plan(ctx, 4, L, 8)
            backend.run_pass(ctx, dev, L, stride)
            _check(ctx, w, mq)
            for b in range(4):
                many = ctx.batch_window_fine(b, extra=10_000)
                assert not many[len(w[1][b]):].tobytes().strip(b"\0")
        finally:
            ctx.close()


@pytest.mark.parametrize("wgs", [0, 3])
def test_a_later_trace_whose_rows_cross_a_pack_boundary(backend, oracle_mod, small, wgs):
    """Traces 1 and 3 of the batch have twelve EPC windows: a pack and a half.  With the launch's default grid and with three
    workgroups for everything (the knob fine_wgs: every workgroup walks many packs, of several traces)"""
    import rfid
    host, lens, L, stride, dev = small
    want = ref.expected_batch(*_oracle(oracle_mod, host, lens, 2))
    assert len(want[1][1]) == 12 and len(want[1][3]) == 12
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=BIG)
    try:
        _plan(ctx, 4, L, 8)
        ctx.set_knob("fine_wgs", wgs)
        backend.run_pass(ctx, dev, L, stride)
        _check(ctx, want, wgs)
    finally:
        ctx.close()


def test_command_line_prints_the_line_and_extends_the_csv(oracle_mod, synth_mod, tmp_path):
    """python -m rfid.batch --tracks OUT.csv --fine on two trace files, in a fresh child process: the CSV's six new columns are
    fine_fields of the oracle-derived records, one line per file stands behind its results block, and a run without --fine prints what
    it printed before (up to the closing line of the pass, which carries wall times) and writes the CSV it wrote."""
    from rfid import batch as rb
    paths, results, ys = [], [], []
    for k in range(2):
        x = synth_mod.make_trace(n_rounds=6 + k, fixed_q=2, tag_ids=TAGS3, seed=104 + 8 * k, sigma=0.02).samples
        p = str(tmp_path / ("trace%d.bin" % k))
        rb.write_trace_file(p, x)
        paths.append(p)
        results.append(oracle_mod.run_trace(x, oracle_mod.config(fixed_q=2)))
        ys.append(oracle_mod.fir(x))
    ent, counts, reads, off = tref.expected_batch(results)
    packed, rows = ref.expected_batch(results, ys)
    assert len(ent) == 6 and len(reads) >= 12
    csv, csvf = str(tmp_path / "tracks.csv"), str(tmp_path / "tracks_fine.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    outs = []
    for extra in (["--tracks", csv, "--max-tags", "8"], ["--tracks", csvf, "--fine", "--max-tags", "8"]):
        r = subprocess.run([sys.executable, "-m", "rfid.batch", "--fixed-q", "2"] + extra + paths, env=env, capture_output=True,
                           text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    plain, fine = outs
    assert open(csv).read() == rb.format_tracks(ent, reads, off, paths)
    want_lines = [rb.format_fine(r) for r in rows]
    stripped = fine
    for line in want_lines:
        assert fine.count(line) == 1 and line not in plain
        stripped = stripped.replace(line, "")
    n_old = plain.rindex("2 traces, ")                       # (the closing line of the pass carries wall times)
    assert stripped[:n_old] == plain[:n_old] and stripped[n_old:].startswith("2 traces, ")
    assert stripped[n_old:].split("\n", 1)[1] == plain[n_old:].split("\n", 1)[1]
    lines = open(csvf).read().splitlines()
    assert lines[0] == rb.TRACKS_HEADER + rb.TRACKS_FINE_COLUMNS and len(lines) == 1 + len(reads)
    assert "\n".join(lines) + "\n" == rb.format_tracks(ent, reads, off, paths, None, packed)
    old = open(csv).read().splitlines()
    for k, line in enumerate(lines[1:]):
        assert ",".join(line.split(",")[:-6]) == old[1 + k]

"""The fine-channel stage on the device (rfid_batch_plan_fine / rfid_batch_fine / rfid_batch_get_fine / rfid_batch_get_window_fine and the
per-call rfid_fine_window): the data-aided channel estimate of every EPC window of a pass and of its eight 16-bit segments.  Every
expected record is worked out in numpy from the ORACLE alone (tests/fine_ref.py: oracle.fir, the oracle's openings, dc_est and per-window
dumps); every comparison is exact -- integers equal, floats by bit pattern, then the bytes of the whole arrays.  The cases that also run
on the wave emulator are written once, in tests/fine_suite.py, and run here through stage_backend.Device: the smallest shapes at which
the kernel can still go wrong -- pack tails, a cut-off inside a pack, a workgroup that walks many packs, a trace without windows, the
per-call forms, the protocol.  Below them, what only the device runs: eight traces, 64 traces back to back and the command line."""
import os
import subprocess
import sys

import pytest

import stage_backend
from stage_backend import lay_out, oracle_pass
import fine_cases as cases
import fine_ref as ref
import tracks_ref as tref
from fine_suite import *

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
    """14 .. 7 rounds, FIXED_Q = 3, six tags, sigma = 0.03; eight traces of different lengths.  The pass three times: byte-identical
    records, packed and per trace; reads and failed windows alike against the oracle."""
    import rfid
    ts = [synth_mod.make_trace(n_rounds=14 - k, fixed_q=3, tag_ids=TAGS6, seed=900 + k, sigma=0.03, t1_jitter_raw=3).samples for k in range(8)]
    host, lens, L, stride = lay_out(ts)
    dev = backend.put(host, lens)
    refs, ys = oracle_pass(oracle_mod, host, lens, 3, max_num_queries=BIG)
    want = ref.expected_batch(refs, ys)
    for b, r in enumerate(want[1]):
        ok = r["flags"] == 1
        assert ok.sum() >= 4 and (~ok).sum() >= 4 and len(r) == 8 * (14 - b), (b, ok.sum(), (~ok).sum())
    ctx = rfid.Context(device=0, fixed_q=3, max_num_queries=BIG)
    try:
        ctx.batch_set_long_stream(mode)
        cases.plan(ctx, 8, L, 16)
        blobs = []
        for rep in range(3):
            backend.run_pass(ctx, dev, L, stride)
            blobs.append(cases.check(ctx, want, (mode, rep)))
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
    ts = [synth_mod.make_trace(n_rounds=3, fixed_q=1, tag_ids=cases.TAGS, seed=500 + k, sigma=0.02, t1_jitter_raw=3).samples for k in range(64)]
    host, lens, L, stride = lay_out(ts)
    dev = backend.put(host, lens)
    host2, lens2, L2, stride2 = lay_out(ts[::-1])
    dev2 = backend.put(host2, lens2)
    assert (L2, stride2) == (L, stride)
    refs, ys = oracle_pass(oracle_mod, host, lens, 1, max_num_queries=BIG)
    want = ref.expected_batch(refs, ys)
    want2 = ref.expected_batch(refs[::-1], ys[::-1])
    assert len(want[0]) >= 64 and sum(int((r["flags"] == 0).sum()) for r in want[1]) >= 16 and want[0].tobytes() != want2[0].tobytes()
    ctx = rfid.Context(device=0, fixed_q=1, max_num_queries=BIG)
    try:
        ctx.set_knob("overlap", overlap)
        cases.plan(ctx, 64, L, 8)
        for rep in range(2):
            backend.run_pass(ctx, dev, L, stride)
            cases.enqueue(ctx)
            backend.run_pass(ctx, dev2, L, stride)      # (the next pass, before anything is fetched)
            first = cases.check_rows(ctx, want, (overlap, rep, "first"), stats=False)
            second = cases.check(ctx, want2, (overlap, rep, "second"))
            assert first != second
    finally:
        ctx.close()


def test_command_line_prints_the_line_and_extends_the_csv(oracle_mod, synth_mod, tmp_path):
    """python -m rfid.batch --tracks OUT.csv --fine on two trace files, in a fresh child process: the CSV's six new columns are
    fine_fields of the oracle-derived records, one line per file stands behind its results block, and a run without --fine prints what
    it printed before (up to the closing line of the pass, which carries wall times) and writes the CSV it wrote."""
    from rfid import batch as rb
    paths, results, ys = [], [], []
    for k in range(2):
        x = synth_mod.make_trace(n_rounds=6 + k, fixed_q=2, tag_ids=cases.TAGS, seed=104 + 8 * k, sigma=0.02).samples
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

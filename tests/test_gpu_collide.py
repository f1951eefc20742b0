"""The collisions stage on the device (rfid_batch_plan_collisions / rfid_batch_collisions / rfid_batch_get_window_collisions /
rfid_batch_collisions_ms, and the per-call rfid_collisions_of): both RN16s and both channels of every RN16 window, as of two tags
replying at once.  Every expected record is worked out in numpy from the ORACLE alone (tests/collide_ref.py); every comparison is exact
-- integers equal, floats by bit pattern, then the bytes of the whole arrays.  The cases that also run on the wave emulator are written
once, in tests/collide_suite.py, and run here through stage_backend.Device: the smallest shapes at which the kernel can still go wrong
-- the tails of a wave's four windows and of a block, more than one block and trace, rows behind a cut-off, fewer workgroups than
blocks.  Below them, what only the device runs: a crowded trace (its cost is printed beside the decoder's) and the command line."""
import os
import subprocess
import sys

import pytest

import collide_ref as ref
import collide_suite as suite
import slots_ref
import stage_backend
from collide_suite import *

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Device()


@pytest.fixture
def call_ctx(gpu_ctx):
    return gpu_ctx


def test_crowded_trace(backend, oracle_mod, synth_mod):
    """FIXED_Q = 4, eight tags, ten rounds: 160 RN16 windows, ten blocks of rows -- the records are the reference's on two repeats.
    The stage's time is printed beside the decoder's"""
    import rfid
    t = synth_mod.make_trace(n_rounds=10, fixed_q=4, tag_ids=tuple(range(1, 9)), seed=8, sigma=suite.SIGMA, t1_jitter_raw=3)
    host, lens, L, stride = stage_backend.lay_out([t.samples])
    o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=4))
    want = ref.expected(oracle_mod, o, oracle_mod.fir(t.samples))
    truth = ref.sent(t.plan.slots)
    two = [k for k, (n, _) in enumerate(truth) if n == 2]
    assert len(want) == 160 == len(truth) and len(two) >= 10
    dev = backend.put(host, lens)
    ctx = rfid.Context(device=0, fixed_q=4)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(1, L)
        ctx.batch_plan_collisions()
        for rep in range(2):
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_collisions_enqueue()
            suite.check_rows(ctx, [want], rep)
        print("device: collisions of one crowded trace (160 RN16 windows, %d two-tag slots): %.4f ms; decode of the same pass %.4f ms" %
              (len(two), ctx.batch_collisions_ms(), ctx.batch_timing()["decode_ms"]))
    finally:
        ctx.close()


def test_command_line_writes_the_collisions_csv_and_a_line_per_file(oracle_mod, synth_mod, tmp_path):
    """python -m rfid.batch --collisions OUT.csv on two trace files, in a fresh child process: exit status 0, one collisions line per
    file behind its results block and the CSV, both format_collisions / format_collisions_csv of the reference's rows; a run without
    the flag prints what --slots alone printed, line for line"""
    from rfid import batch as rb
    paths, collided, starts = [], [], []
    for k, b in enumerate((0, 1)):
        t = suite.trace_of(synth_mod, b)
        p = str(tmp_path / ("trace%d.bin" % k))
        rb.write_trace_file(p, t.samples)
        paths.append(p)
        o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=2))
        y = oracle_mod.fir(t.samples)
        slots = rb.classify_slots(slots_ref.expected(o, y, k))
        collided.append(rb.classify_collisions(ref.expected(oracle_mod, o, y, k), slots))
        starts.append(o.open_idx)
    assert all(len(c) >= 4 for c in collided) and sum(int((c["order"] == 2).sum()) for c in collided) >= 6
    csv, slots_csv = str(tmp_path / "collisions.csv"), str(tmp_path / "slots.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    base = [sys.executable, "-m", "rfid.batch", "--fixed-q", "2", "--slots", slots_csv]
    r = subprocess.run(base + ["--collisions", csv] + paths, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    for k, p in enumerate(paths):
        line = rb.format_collisions(collided[k])
        assert out.count(line) == 1, (line, out)
        at = out.index(line)
        assert out.index(p + "\n") < at and (k + 1 == len(paths) or at < out.index(paths[k + 1] + "\n"))
    assert open(csv).read() == rb.format_collisions_csv(collided, starts, paths)
    with_flag_slots = open(slots_csv).read()
    # without the flag: what --slots alone printed, line for line, and the same slots CSV
    plain = subprocess.run(base + paths, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    timing = lambda s: " raw samples: " in s
    keep = [s for s in out.splitlines() if not s.startswith("| collided slots :") and not timing(s)]
    assert keep == [s for s in plain.stdout.splitlines() if not timing(s)]
    assert "collided slots" not in plain.stdout and len(out.splitlines()) == len(plain.stdout.splitlines()) + 2
    assert open(slots_csv).read() == with_flag_slots
    # --collisions alone classifies the slots but prints neither their line nor their CSV
    alone = subprocess.run(base[:-2] + ["--collisions", csv] + paths, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert alone.returncode == 0 and "| slots :" not in alone.stdout and alone.stdout.count("| collided slots :") == 2

"""The diversity stage on the device (rfid_batch_plan_diversity / rfid_batch_diversity / rfid_batch_get_window_diversity /
rfid_batch_diversity_ms, and the per-call rfid_diversity_window): the EPC windows of traces recorded together -- the receive antennas of
one session -- combined before the sign is taken.  Every expected record is worked out in numpy from the ORACLE alone
(tests/diversity_ref.py); every comparison is exact -- integers equal, the floats by bit pattern, then the bytes of the whole arrays.
The cases that also run on the wave emulator are written once, in tests/diversity_suite.py, and run here through stage_backend.Device:
the smallest shapes at which the kernel can still go wrong -- block tails, more than one block and group, a member cut short, a member
outside the slack, two sessions paired, rows behind a cut-off, fewer workgroups than blocks, two and eight members.  Below them, what
only the device runs: a crowded group (its cost is printed beside the decoder's) and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import diversity_ref as ref
import diversity_suite as suite
import inventory_ref
import stage_backend
from diversity_suite import *

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Device()


@pytest.fixture
def call_ctx(gpu_ctx):
    return gpu_ctx


def test_crowded_group(backend, oracle_mod, synth_mod):
    """FIXED_Q = 4, eight tags, three antennas, six rounds: 96 EPC windows per antenna, most of them of empty or collided slots; the
    records are the reference's.  The stage's time is printed beside the decoder's"""
    import rfid
    m = np.arange(3)
    traces, slots = synth_mod.make_antennas(leaks=list((1 - 0.15 * m) * np.exp(1j * (0.7 + 1.3 * m))),
                                            hs=list(0.026 * (1 - 0.1 * m) * np.exp(1j * (2.1 + 0.8 * m))), sigma=suite.SIGMA,
                                            noise_seeds=[9000 + int(k) for k in m], n_rounds=6, fixed_q=4, tag_ids=tuple(range(1, 9)),
                                            seed=8, t1_jitter_raw=3)
    host, lens, L, stride = stage_backend.lay_out([t.samples for t in traces])
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=4)) for b in range(3)]
    want, left_out = ref.expected_group(oracle_mod, refs, [oracle_mod.fir(host[b, : lens[b]]) for b in range(3)])
    reads, combined, recovered, lone = suite.counts(want)
    assert len(want) == 96 == len(slots) and reads >= 3 and combined > reads and recovered >= 3, (reads, combined, recovered, lone)
    dev = backend.put(host, lens)
    ctx = rfid.Context(device=0, fixed_q=4)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_diversity(3)
        for rep in range(2):
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_diversity_enqueue()
            suite.check_rows(ctx, [want], rep)
        print("device: diversity of one crowded group (96 EPC windows of 3 antennas, %d combined, %d recovered): %.4f ms; decode of the "
              "same pass %.4f ms" % (combined, recovered, ctx.batch_diversity_ms(), ctx.batch_timing()["decode_ms"]))
    finally:
        ctx.close()


def test_command_line_writes_the_diversity_csv_and_a_line_per_group(batch, tmp_path):
    """python -m rfid.batch --antennas 3 --diversity OUT.csv on the batch's six trace files, in a fresh child process: exit status 0, one
    diversity line per group behind its anchor's results block and the CSV, both the host functions on the reference's records; a run
    without the flags prints what it printed before"""
    from rfid import batch as rb
    paths = []
    for b in range(6):
        p = str(tmp_path / ("capture%d_antenna%d.bin" % (b // 3, b % 3)))
        rb.write_trace_file(p, batch["host"][b, : batch["lens"][b]])
        paths.append(p)
    want = batch["want"]
    entries = [inventory_ref.expected(o.dumps, b) for b, o in enumerate(batch["refs"])]
    of_members = [entries[0:3], entries[3:6]]
    csv = str(tmp_path / "diversity.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    base = [sys.executable, "-m", "rfid.batch", "--fixed-q", "2"]
    r = subprocess.run(base + ["--antennas", "3", "--diversity", csv] + paths, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    rule = " --------------------------\n"
    for g in range(2):
        line = rb.format_diversity(want[g], of_members[g])
        assert out.count(line) == 1, (line, out)
        at = out.index(line)
        assert out[at - len(rule):at] == rule and out.index(paths[3 * g] + "\n") < at < out.index(paths[3 * g + 1] + "\n")
    text = open(csv).read()
    assert text == rb.format_diversity_csv(want, of_members, [paths[0], paths[3]])
    assert len(text.splitlines()) == 1 + sum(suite.counts(w)[2] for w in want)
    # without the flags (--diversity implies --inventory): what it printed before, line for line
    plain = subprocess.run(base + ["--inventory"] + paths, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    timing = lambda s: " raw samples: " in s
    keep = [s for s in out.splitlines() if not s.startswith("| EPC windows :") and not timing(s)]
    assert keep == [s for s in plain.stdout.splitlines() if not timing(s)]
    assert "recovered by combining" not in plain.stdout and len(out.splitlines()) == len(plain.stdout.splitlines()) + 2
    # files that are no whole captures are refused before anything is decoded
    bad = subprocess.run(base + ["--antennas", "3", "--diversity", csv] + paths[:5], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert bad.returncode == 2 and "whole captures" in bad.stderr

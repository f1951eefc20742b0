"""The slots stage on the device (rfid_batch_plan_slots / rfid_batch_slots / rfid_batch_get_window_moments / rfid_batch_slots_ms, and
the per-call rfid_window_moments_of): the second-order moments of every window's gated samples.  Every expected record is worked out
in numpy from the ORACLE alone (tests/slots_ref.py); every comparison is exact -- integers equal, floats by bit pattern, then the bytes
of the whole arrays.  The cases that also run on the wave emulator are written once, in tests/slots_suite.py, and run here through
stage_backend.Device: the smallest shapes at which the kernel can still go wrong -- pack tails, odd counts, more than one trace, rows
behind a cut-off.  Below them, what only the device runs: the long-stream front end, two result sets, more packs than workgroups,
and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import slots_ref as ref
import slots_cases as cases
import slots_suite as suite
import stage_backend
from slots_suite import *

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Device()


@pytest.fixture
def call_ctx(gpu_ctx):
    return gpu_ctx


def test_long_stream_front_end_gives_the_same_records(backend, ragged):
    """rfid_batch_set_long_stream mode 2 on one trace (the 93-window one): the records of the fused front end, the oracle's"""
    import rfid
    host, lens, L, stride, refs, want, _ = ragged
    dev = backend.put(host[:1], lens[:1])
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(1, L)
        ctx.batch_plan_slots()
        blobs = []
        for mode in (2, 0, 2):
            ctx.batch_set_long_stream(mode)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_slots_enqueue()
            blobs.append(cases.check_rows(ctx, want[:1], mode))
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        assert blobs[0] == blobs[1] == blobs[2]
    finally:
        ctx.close()


def test_two_result_sets_each_pass_gets_its_own_records(backend, small):
    """44 traces (the two short ones, 22 times: 2 200 packs of rows against the 2 048 workgroups of a 256-CU launch, so a workgroup
    goes round its loop again), two result sets alternating (RFID_OVERLAP=2): the next pass -- the traces in the other order -- enqueued
    BEFORE this pass's records are fetched leaves them this pass's, then gets its own"""
    import rfid
    host, lens, L, stride, refs, want, _ = small
    order = np.arange(44) % 2
    dev_a = backend.put(host[order], lens[order])
    dev_b = backend.put(host[1 - order], lens[1 - order])

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
            backend.run_pass(ctx, dev_a, L, stride)
            ctx.batch_slots_enqueue()
            backend.run_pass(ctx, dev_b, L, stride)
            for b, w in enumerate(stamped(order)):
                ref.assert_equal(ctx.batch_window_moments(b), w, ("a", rep, b))
            ctx.batch_slots_enqueue()
            cases.check_rows(ctx, stamped(1 - order), ("b", rep))
    finally:
        ctx.close()


def test_per_call_path_on_crafted_windows(oracle_mod, ragged, call_ctx):
    """the shared case, then more packs than the launch has workgroups (at most eight per compute unit): a workgroup goes round its
    loop again (too many windows for the emulator)"""
    suite.test_per_call_path_on_crafted_windows(oracle_mod, ragged, call_ctx)
    host, lens, L, stride, refs, want, _ = ragged
    g = cases.crafted_windows(oracle_mod, host, lens, refs, stream=0, seq=5)
    big = np.ascontiguousarray(np.tile(g, (1546, 1))[:17_001])
    ref.assert_equal(call_ctx.window_moments(big), ref.expected_of(big), "17 001 windows")


def test_classification_agrees_with_the_truth_on_the_five_shapes(backend, oracle_mod, synth_mod):
    """The five shapes at sigma = 0.01: the device's records are the oracle's, classify_slots == SlotTruth for EVERY slot (no slot may
    be left out) and == the restatement of slots_ref; Schoute's estimate on the five-tag shape is 4.82 per round, the suggested Q 2"""
    from rfid import batch as rb
    cases.check_five_shapes(rb, cases.five_shapes(backend, oracle_mod, synth_mod))


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

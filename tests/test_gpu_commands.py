"""The commands stage on the device (rfid_batch_plan_commands / rfid_batch_commands / rfid_batch_get_window_commands /
rfid_batch_commands_ms, and the per-call rfid_commands_of): the reader's own PIE command in front of every window.  Every expected
record is worked out in numpy from the ORACLE alone (tests/commands_ref.py) and compared by bytes; what every window's command must BE
comes from the synthesiser's slot table.  The cases that also run on the wave emulator are written once, in tests/commands_suite.py,
and run here through stage_backend.Device: the smallest shapes at which the kernel can still go wrong -- edges at the seams of the
ballots, 64 / 65 edges, gaps of 120 / 121, ties, odd counts, more than one trace, rows behind a cut-off, a span clipped at the
trace's start.  Below them, what only the device runs: the long-stream front end, two result sets, more blocks than workgroups, and
the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import commands_ref as ref
import commands_cases as cases
import commands_suite as suite
import stage_backend
from commands_suite import *

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
    host, lens, L, stride, refs, want, plans, _ = ragged
    dev = backend.put(host[:1], lens[:1])
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(1, L)
        ctx.batch_plan_commands()
        blobs = []
        for mode in (2, 0, 2):
            ctx.batch_set_long_stream(mode)
            backend.run_pass(ctx, dev, L, stride)
            ctx.batch_commands_enqueue()
            blobs.append(cases.check_rows(ctx, want[:1], mode))
            rep = ctx.batch_ls_report()
            assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        assert blobs[0] == blobs[1] == blobs[2]
    finally:
        ctx.close()


def test_two_result_sets_each_pass_gets_its_own_records(backend, small):
    """44 traces (the two short ones, 22 times) at one row per block (the knob commands_rows: the stage would pack four): more
    (trace, row) items than the launch has workgroups, so a workgroup of commands_kernel goes round its loop again -- past blocks
    behind the cut-off and blocks with work alike.  Two result sets alternating (RFID_OVERLAP=2): the next pass -- the traces in
    the other order -- enqueued BEFORE this pass's records are fetched leaves them this pass's, then gets its own"""
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
        ctx.batch_plan_commands()
        ctx.set_knob("commands_rows", 1)
        looped = False
        for rep in range(2):
            backend.run_pass(ctx, dev_a, L, stride)
            ctx.batch_commands_enqueue()
            backend.run_pass(ctx, dev_b, L, stride)
            for b, w in enumerate(stamped(order)):
                ref.assert_equal(ctx.batch_window_commands(b), w, ("a", rep, b))
            ctx.batch_commands_enqueue()
            cases.check_rows(ctx, stamped(1 - order), ("b", rep))
            if not looped:       # (the launch has at most 20 workgroups per compute unit)
                import torch
                wmax = cases.table_rows(ctx, L)
                assert 44 * wmax > 2 * 20 * torch.cuda.get_device_properties(0).multi_processor_count, wmax
                looped = True
    finally:
        ctx.close()


def test_per_call_path_on_crafted_spans(synth_mod, call_ctx):
    """the shared case, then more blocks of sixteen spans (1 063) than the launch has workgroups (two per compute unit): a workgroup
    goes round its loop again (too many spans for the emulator)"""
    suite.test_per_call_path_on_crafted_spans(synth_mod, call_ctx)
    spans, levels, names = cases.crafted_spans(synth_mod)
    want = ref.expected_of(spans, levels)
    reps = -(-17_001 // len(spans))
    big = np.ascontiguousarray(np.tile(spans, (reps, 1))[:17_001])
    big_levels = np.ascontiguousarray(np.tile(levels, reps)[:17_001])
    big_want = np.tile(want, reps)[:17_001]
    big_want["seq"] = np.arange(17_001)
    got = call_ctx.commands_of(big, big_levels)
    assert len(got) == 17_001 and int(got["seq"][-1]) == 17_000
    ref.assert_equal(got, big_want, "17 001 spans")


def test_command_line_writes_the_commands_csv_and_a_line_per_file(oracle_mod, synth_mod, tmp_path):
    """python -m rfid.batch --commands OUT.csv on two trace files, in a fresh child process: exit status 0, one commands line per file
    behind its results block, the CSV's commands, Q and ACKed RN16 are the truth; nothing else is printed (--commands implies nothing)"""
    from rfid import batch as rb
    import slots_ref
    paths, rows, starts, truth = [], [], [], []
    for k, shape in enumerate((slots_ref.SHAPES[4], (2, (1, 2, 3), 3, 21))):
        t = slots_ref.shape_trace(synth_mod, shape, cases.SIGMA)
        p = str(tmp_path / ("trace%d.bin" % k))
        rb.write_trace_file(p, t.samples)
        paths.append(p)
        o = oracle_mod.run_trace(t.samples, oracle_mod.config(fixed_q=2))
        rows.append(ref.expected(o, oracle_mod.fir(t.samples), k))
        starts.append(np.asarray(o.open_idx))
        truth.append(ref.plan_truth(t))
        ref.check_truth(rows[-1], t, k)
        assert len(rows[-1]) == len(truth[-1]) == 2 * shape[2] << 2
    csv = str(tmp_path / "commands.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    r = subprocess.run([sys.executable, "-m", "rfid.batch", "--fixed-q", "2", "--commands", csv] + paths, env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert " tags\n" not in out and "EPC windows :" not in out and "| slots :" not in out
    rule = " --------------------------\n"
    for k, p in enumerate(paths):
        line = rb.format_commands(rows[k])
        assert out.count(line) == 1, (line, out)
        at = out.index(line)
        assert out[at - len(rule):at] == rule and out.index(p + "\n") < at
        assert k + 1 == len(paths) or at < out.index(paths[k + 1] + "\n")
        n_q = sum(t[0] == ref.QUERY for t in truth[k])
        n_w = len(truth[k])
        singles = sum(t[4] for t in truth[k])
        assert line.startswith("| commands : %d  query : %d  queryrep : %d  ack : %d  other : 0  none : 0  Q : {2}  failed CRC-5 : 0  " %
                               (n_w, n_q, n_w // 2 - n_q, n_w // 2)), line
        assert int(line.split("RN16 : ")[1].split(" of ")[0]) >= singles > 0 and (" of %d  median" % (n_w // 2)) in line
    text = open(csv).read()
    assert text == rb.format_commands_csv(rows, starts, paths)
    lines = text.splitlines()
    assert lines[0] == rb.COMMANDS_HEADER and len(lines) == 1 + sum(map(len, truth))
    names = {ref.QUERY: "query", ref.QUERY_REP: "queryrep", ref.ACK: "ack"}
    i = 1
    for k, p in enumerate(paths):
        for j, t in enumerate(truth[k]):
            f = lines[i].split(",")
            assert f[:2] == [p, str(j)] and f[3] == names[t[0]] and abs(float(f[2]) - starts[k][j] / 400e3) <= 1e-9, (lines[i], t)
            assert f[6] == (str(t[1]) if t[0] == ref.QUERY else "") and f[7] == ("%04x" % t[3] if t[0] == ref.ACK else ""), (lines[i], t)
            assert f[8] == ("1" if t[0] == ref.QUERY else "") and (not t[4] or f[9] == "1"), (lines[i], t)
            i += 1

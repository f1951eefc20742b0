"""The stack stage on the device (rfid_batch_plan_stack / rfid_batch_stack / rfid_batch_get_window_stacks / rfid_batch_stack_ms, and the
per-call rfid_stack_windows): an unknown tag's repeated EPC frames combined over the rounds of a session.  Every expected record is
worked out in numpy from the ORACLE alone (tests/stack_ref.py); every comparison is exact -- integers equal, the floats by bit pattern,
then the bytes of the whole arrays.  The cases that also run on the wave emulator are written once, in tests/stack_suite.py, and run
here through stage_backend.Device: the smallest shapes at which the kernels can still go wrong -- one, two and 64 rows in a block, a
second block of sixteen, reads between the failed rows, rows behind a cut-off, one workgroup for every block, ties, zeros and sums
that cancel.  The stage's time is printed beside the decoder's; no timing is claimed or asserted: these are single passes far below
the device's width.  Below them, what only the device runs: the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import inventory_ref
import stack_ref as ref
import stack_suite as suite
import stage_backend
from stack_suite import *

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Device()


@pytest.fixture
def call_ctx(gpu_ctx):
    return gpu_ctx


def test_command_line_writes_the_stack_csv_and_the_line_per_file(batch, tmp_path):
    """python -m rfid.batch --stack OUT.csv [--stack-min RHO] on the batch's four trace files, in a fresh child process: exit status 0,
    the stack line behind every file's results block and the CSV, both the host functions on the reference's records and the
    inventories the oracle's results give"""
    from rfid import batch as rb
    paths = []
    for b in range(suite.N):
        p = str(tmp_path / ("trace%d.bin" % b))
        rb.write_trace_file(p, batch["host"][b, : batch["lens"][b]])
        paths.append(p)
    ents = [inventory_ref.expected(o.dumps, b) for b, o in enumerate(batch["refs"])]
    csv = str(tmp_path / "stack.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    base = [sys.executable, "-m", "rfid.batch", "--fixed-q", "2"]
    for flags in (["--stack", csv], ["--stack", csv, "--stack-min", "0.5"]):
        r = subprocess.run(base + flags + paths, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        for b in range(suite.N):
            line = rb.format_stack(batch["rows"][b], ents[b])
            at = r.stdout.index(paths[b] + "\n")
            assert r.stdout.index(line, at) > at, (line, r.stdout)
        assert open(csv).read() == rb.format_stack_csv(batch["rows"], ents, paths)
        assert "all traces:" in r.stdout                               # (--stack implies --inventory)
    bad = subprocess.run(base + ["--stack", csv, "--stack-min", "1.5"] + paths[:1], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert bad.returncode == 2 and "--stack-min" in bad.stderr

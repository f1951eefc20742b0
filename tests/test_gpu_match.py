"""The match stage on the device (rfid_batch_plan_match / rfid_batch_match_set_list / rfid_batch_match / rfid_batch_get_window_matches /
rfid_batch_match_ms, and the per-call rfid_match_window): known tags' frames found in CRC-failed EPC windows.  Every expected record is
worked out in numpy from the ORACLE alone (tests/match_ref.py); every comparison is exact -- integers equal, the floats by bit pattern,
then the bytes of the whole arrays.  The cases that also run on the wave emulator are written once, in tests/match_suite.py, and run
here through stage_backend.Device: the smallest shapes at which the kernel can still go wrong -- block tails, more than one block and
trace, an empty inventory, rows behind a cut-off, fewer workgroups than blocks, one, 65, 130 and 1024 candidates.  The stage's time is
printed beside the decoder's; no timing is claimed or asserted: these are single passes far below the device's width.  Below them, what
only the device runs: the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import inventory_ref
import match_ref as ref
import match_suite as suite
import stage_backend
from match_suite import *

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Device()


@pytest.fixture
def call_ctx(gpu_ctx):
    return gpu_ctx


def test_command_line_writes_the_match_csv_and_the_lines_per_file(batch, tmp_path):
    """python -m rfid.batch --match OUT.csv [--match-list EPCS.txt] on the batch's four trace files, in a fresh child process each: exit
    status 0, the match lines behind every file's results block and the CSV, both the host functions on the reference's records"""
    import rfid
    from rfid import batch as rb
    paths = []
    for b in range(suite.N):
        p = str(tmp_path / ("trace%d.bin" % b))
        rb.write_trace_file(p, batch["host"][b, : batch["lens"][b]])
        paths.append(p)
    results = []
    for o in batch["refs"]:
        r = np.zeros(len(o.dumps), dtype=rfid.capi.RESULT_DTYPE)
        r["h_re"], r["h_im"] = o.dumps["h_est"][:, 0], o.dumps["h_est"][:, 1]
        r["bits"] = inventory_ref.pack_frames(o.dumps["bits"])
        results.append(r)
    epcs = str(tmp_path / "epcs.txt")
    with open(epcs, "w") as f:
        f.write("".join("%04x:%s\n" % rb.frame_fields(fr) for fr in batch["frames"]))
    csv = str(tmp_path / "match.csv")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    base = [sys.executable, "-m", "rfid.batch", "--fixed-q", "2"]
    for flags, want in ((["--match", csv], batch["own"]), (["--match", csv, "--match-list", epcs], batch["lst"])):
        r = subprocess.run(base + flags + paths, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        for b in range(suite.N):
            block = rb.format_match(want[b], results[b])
            assert r.stdout.count(block) >= 1, (block, r.stdout)
            assert r.stdout.index(paths[b] + "\n") < r.stdout.index(block, r.stdout.index(paths[b] + "\n"))
        assert open(csv).read() == rb.format_match_csv(want, paths, results)
        assert ("all traces:" in r.stdout) == (len(flags) == 2)        # (without a list --match implies --inventory)
    bad = subprocess.run(base + ["--match-list", epcs] + paths[:1], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert bad.returncode == 2 and "--match" in bad.stderr

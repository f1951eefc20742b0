"""The pin hooks that need more than this image has.  The oracle (oracle/rfid_oracle.c) IS pinned to the reference's own
gate / tag_decoder / reader blocks, compiled untouched against stand-in headers and run under the oracle's schedule
(tests/test_reference_blocks.py).  What that leaves unpinned -- a real GNU Radio scheduler and VOLK's filter, and the
reference's one known answer, whose trace file is missing from the checkout -- these tests take up where the
environment allows it:

  * with a real GNU Radio 3.7 (gnuradio-config-info on PATH): `make -C oracle ref` compiles the reference's OWN sources
    against the real headers together with oracle/ref_harness.cc; the harness is run (single-threaded scheduler) on the
    committed fixtures' traces and its matched-filter output, gated samples and print_results() text are compared with
    the oracle's;
  * with the reference's bundled trace misc/data/file_source_test: tests/test_gpu_round2.py replays it (README.md:48-53).

Both skip here."""
import os
import shutil
import subprocess
import glob

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
HAVE_GR = shutil.which("gnuradio-config-info") is not None and os.path.isdir("/root/reference/gr-rfid/lib")


def test_the_hook_is_wired():
    """(runs everywhere) the recipe and the harness exist, and without GNU Radio the recipe says so instead of faking a build"""
    assert os.path.isfile(os.path.join(ROOT, "oracle", "ref_harness.cc"))
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    if not HAVE_GR:
        assert "unbuildable" in out.stdout and not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "ref_harness"))


@pytest.mark.skipif(not HAVE_GR, reason="no GNU Radio in this image: the real-scheduler harness cannot be compiled (tests/test_reference_blocks.py pins the blocks)")
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_reference_blocks_against_the_oracle(tmp_path, oracle_mod, path):
    g = np.load(path)
    if int(g["fixed_q"]) != 0:
        pytest.skip("FIXED_Q is a compile-time constant of the reference (global_vars.h:72): rebuild it to pin this fixture")
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
    assert os.path.isfile(exe)
    trace = tmp_path / "trace.bin"
    g["raw"].astype(np.complex64).tofile(str(trace))
    out = subprocess.run([exe, str(trace), str(tmp_path / "ref")], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, GR_SCHEDULER="STS"))
    assert out.returncode == 0, out.stderr
    o = oracle_mod.run_trace(g["raw"])
    # the report (lib/reader_impl.cc:173-192)
    assert o.print_results().strip() in out.stdout
    # the matched filter: VOLK's summation order is the machine's -- rounding-level agreement (tests/test_fir_boundary.py)
    y_ref = np.fromfile(str(tmp_path / "ref.mf"), dtype=np.complex64)
    y = oracle_mod.fir(g["raw"])
    n = min(len(y), len(y_ref))
    assert n > 0 and np.abs(y_ref[:n] - y[:n]).max() <= 1e-6 * np.abs(y).max()
    # the gate's output: in[i] - dc_est over every window (lib/gate_impl.cc:176,187), bit for bit when the filter
    # outputs agree bit for bit, else to the filter's rounding level
    gated_ref = np.fromfile(str(tmp_path / "ref.gate"), dtype=np.complex64)
    want = np.concatenate([(y[s:s + (1370 if t else 250)] - np.complex64(dc)).astype(np.complex64)
                           for s, t, dc in zip(o.open_idx, o.dumps["type"], o.dc)])
    m = min(len(want), len(gated_ref))
    assert m >= len(want) - 1370
    if np.array_equal(y_ref[:n].view(np.uint32), y[:n].view(np.uint32)):
        assert np.array_equal(gated_ref[:m].view(np.uint32), want[:m].view(np.uint32))
    else:
        assert np.abs(gated_ref[:m] - want[:m]).max() <= 1e-5 * np.abs(y).max()

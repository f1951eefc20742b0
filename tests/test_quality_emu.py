"""The read-quality stage (rfid_batch_plan_quality / rfid_batch_quality / rfid_batch_get_quality / rfid_batch_get_window_quality:
SNR and decision margin of every EPC window, built on the device behind the tracks) on the CPU: csrc/rfid_capi.hip and
csrc/rfid_quality.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave emulator.  Every expected record is
worked out in numpy from the ORACLE alone (tests/quality_ref.py: oracle.fir, the oracle's openings, dc_est and per-window dumps), never
from the library's own windows or results, and every comparison is exact: by bit pattern, then by the bytes of the whole arrays.
The cases that also run on the device are written once, in tests/quality_suite.py, and run here through stage_backend.Emulated; below
them, what only this side runs: the host functions.  The traces are in tests/quality_cases.py."""
import numpy as np
import pytest

import quality_ref as ref
import tracks_ref as tref
import emu_lib
import stage_backend
from quality_suite import *


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Emulated()


def test_quality_fields_and_the_csv_columns(batch):
    """rfid.batch.quality_fields / format_tracks(..., quality) / format_quality (host side) on the oracle-derived records"""
    from rfid import batch as rb
    from rfid import _capi as capi
    host, lens, L, stride, refs, ys, (packed, rows), _ = batch
    snr, margin = rb.quality_fields(packed)
    assert snr.dtype == np.float64 and margin.dtype == np.float64
    for i, q in enumerate(packed):
        assert snr[i] == 10.0 * np.log10(float(q["sig_sq"]) / float(q["quad_sq"]))
        assert margin[i] == float(q["margin_min"]) / (float(q["sig_abs"]) / 128.0)
    assert np.array_equal(snr, ref.snr_db(packed)) and (margin > 0).all() and (margin <= 1.0).all()
    edge = np.zeros(2, dtype=capi.QUALITY_DTYPE)
    edge["sig_sq"][0] = 1.0
    s, m = rb.quality_fields(edge)
    assert s[0] == np.inf and np.isnan(s[1]) and np.isnan(m[1])
    ent, counts, reads, off = tref.expected_batch(refs)
    names = ["a.bin", "b.bin"]
    plain = rb.format_tracks(ent, reads, off, names)
    assert plain.splitlines()[0] == rb.TRACKS_HEADER == "file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T"
    lines = rb.format_tracks(ent, reads, off, names, packed).splitlines()
    assert lines[0] == rb.TRACKS_QUALITY_HEADER == rb.TRACKS_HEADER + ",snr_db,margin" and len(lines) == 1 + len(reads)
    for line, old, k in zip(lines[1:], plain.splitlines()[1:], range(len(reads))):
        f = line.split(",")
        assert ",".join(f[:-2]) == old                      # (the columns there were are untouched)
        assert f[-2] == "%.9g" % snr[k] and f[-1] == "%.9g" % margin[k]
    text = rb.format_quality(rows[0])
    ok = rows[0]["flags"] == 1
    assert text.startswith("| EPC windows : %d  failed : %d  " % (len(rows[0]), (~ok).sum())) and text.endswith("\n") and text.count("\n") == 1
    assert "%.2f" % np.median(ref.snr_db(rows[0])[ok]) in text and "%.2f" % np.median(ref.snr_db(rows[0])[~ok]) in text

"""The fine-channel stage (rfid_batch_plan_fine / rfid_batch_fine / rfid_batch_get_fine / rfid_batch_get_window_fine and the per-call
rfid_fine_window: the data-aided channel estimate of every EPC window and of its eight 16-bit segments, built on the device behind the
tracks) on the CPU: csrc/rfid_capi.hip and csrc/rfid_fine.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the
wave emulator.  Every expected record is worked out in numpy from the ORACLE alone (tests/fine_ref.py: oracle.fir, the oracle's
openings, dc_est and per-window dumps), never from the library's own windows or results, and every comparison of records is exact: by
bit pattern, then by the bytes of the whole arrays.  The cases that also run on the device are written once, in tests/fine_suite.py,
and run here through stage_backend.Emulated; below them, what only this side runs: the host functions.  The traces are in
tests/fine_cases.py."""
import numpy as np
import pytest

import fine_ref as ref
import tracks_ref as tref
import emu_lib
import stage_backend
from fine_suite import *


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Emulated()


def test_fine_fields_and_the_csv_columns(batch):
    """rfid.batch.fine_fields / format_tracks(..., fine) / format_fine (host side) on the oracle-derived records"""
    from rfid import batch as rb
    from rfid import _capi as capi
    host, lens, L, stride, refs, ys, (packed, rows), _ = batch
    ff = rb.fine_fields(packed)
    assert ff["h"].dtype == np.complex128 and ff["h_seg"].shape == (len(packed), 8)
    for i, r in enumerate(packed):
        re, im = np.float64(r["sum_re"]), np.float64(r["sum_im"])
        sq = re * re + im * im
        mag = np.sqrt(sq) / 128.0
        assert ff["h"][i].real == re / 128.0 and ff["h"][i].imag == im / 128.0
        assert ff["noise"][i] == (np.float64(r["pow"]) - sq / 128.0) / 127.0 > 0
        assert ff["mag_db"][i] == 20.0 * np.log10(mag) and ff["phase_rad"][i] == np.arctan2(im, re)
        assert ff["snr_db"][i] == 10.0 * np.log10(mag ** 2 / ff["noise"][i])
        hk = (r["seg_re"].astype(np.float64) + 1j * r["seg_im"].astype(np.float64)) / 16.0
        assert np.array_equal(ff["h_seg"][i], hk)
        ph = np.angle(hk * np.conj(ff["h"][i]))
        slope = np.polyfit(400e-6 * np.arange(8), ph, 1)[0]
        assert abs(ff["drift_rad_s"][i] - slope) <= 1e-9 * max(1.0, abs(slope)), (i, ff["drift_rad_s"][i], slope)
    assert ref.h_of(packed).tobytes() == ff["h"].tobytes() and (ff["snr_db"] > 10.0).all()
    # a turning channel has the drift it was given: 0.6 rad over 1370 samples at 400 ksps
    edge = np.zeros(3, dtype=capi.FINE_DTYPE)
    turn = np.exp(1j * 0.6 * 160.0 / 1370.0 * np.arange(8))
    edge["seg_re"][0], edge["seg_im"][0] = 16.0 * turn.real, 16.0 * turn.imag
    edge["sum_re"][0], edge["sum_im"][0], edge["pow"][0] = edge["seg_re"][0].sum(), edge["seg_im"][0].sum(), 128.0
    edge["sum_re"][1], edge["pow"][1] = 128.0, 128.0
    e = rb.fine_fields(edge)
    assert abs(e["drift_rad_s"][0] - 0.6 * 400e3 / 1370.0) < 1e-3 and e["drift_rad_s"][1] == 0.0
    assert e["snr_db"][1] == np.inf and np.isnan(e["snr_db"][2]) and e["mag_db"][2] == -np.inf
    ent, counts, reads, off = tref.expected_batch(refs)
    names = ["a.bin", "b.bin", "c.bin", "d.bin"]
    plain = rb.format_tracks(ent, reads, off, names)
    assert plain.splitlines()[0] == rb.TRACKS_HEADER == "file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T"
    assert rb.TRACKS_FINE_COLUMNS == ",hd_re,hd_im,hd_mag_db,hd_phase_rad,hd_snr_db,drift_rad_s"
    lines = rb.format_tracks(ent, reads, off, names, None, packed).splitlines()
    assert lines[0] == rb.TRACKS_HEADER + rb.TRACKS_FINE_COLUMNS and len(lines) == 1 + len(reads)
    for line, old, k in zip(lines[1:], plain.splitlines()[1:], range(len(reads))):
        f = line.split(",")
        assert ",".join(f[:-6]) == old                      # (the columns there were are untouched)
        assert f[-6:] == ["%.9g" % v for v in (ff["h"][k].real, ff["h"][k].imag, ff["mag_db"][k], ff["phase_rad"][k], ff["snr_db"][k],
                                               ff["drift_rad_s"][k])]
    text = rb.format_fine(rows[0])
    ok = rows[0]["flags"] == 1
    assert text.startswith("| EPC windows : %d  failed : %d  " % (len(rows[0]), (~ok).sum())) and text.endswith("\n") and text.count("\n") == 1
    assert "%.2f" % np.median(rb.fine_fields(rows[0])["snr_db"][ok]) in text
    assert rb.format_fine(rows[0][:0]).startswith("| EPC windows : 0  failed : 0  ")

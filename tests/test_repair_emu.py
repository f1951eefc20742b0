"""The repair stage (rfid_batch_plan_repair / rfid_batch_repair / rfid_batch_get_repairs / rfid_batch_get_window_repairs and the
per-call rfid_repair_window: CRC-failed EPC frames recovered from their weakest decisions, built on the device behind the inventory) on
the CPU: csrc/rfid_capi.hip and csrc/rfid_repair.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave
emulator.  Every expected record is worked out from the ORACLE alone (tests/repair_ref.py: the definition of include/rfid_mi355x.h run
literally, the oracle's check_crc for the CRC), never from the library's own windows or results, and every comparison is exact: by bit
pattern, then by the bytes of the whole arrays.  Each test asserts from the reference that its input has the properties it is there
for before a kernel sees it.  The cases that also run on the device are written once, in tests/repair_suite.py, and run here through
stage_backend.Emulated; below them, what only this side runs: the host functions.  The traces are in tests/repair_cases.py."""
import numpy as np
import pytest

import repair_ref as ref
import emu_lib
import stage_backend
from repair_suite import *


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Emulated()


def test_format_helpers_and_the_csv_columns(single):
    """rfid.batch.repair_flips / format_repair_summary / format_repairs (host side) on the reference-made records"""
    from rfid import batch as rb
    packed, (rows,) = single["mixed"][6]
    assert [rb.repair_flips(r) for r in packed] == [ref.flip_list(r) for r in packed]
    assert rb.format_repair_summary(rows) == "| failed EPC windows : 26  repaired : 6  of a tag in the inventory : 3\n"
    assert rb.format_repair_summary(rows[:0]) == "| failed EPC windows : 0  repaired : 0  of a tag in the inventory : 0\n"
    lines = rb.format_repairs(packed, ["a.bin"]).splitlines()
    assert lines[0] == rb.REPAIRS_HEADER == "file,epc,pc,seq,t_s,n_flips,flips,cost,known" and len(lines) == 1 + len(packed)
    for line, r in zip(lines[1:], packed):
        f = line.split(",")
        pc, epc = rb.frame_fields(r["frame"])
        assert f[0] == "a.bin" and f[1] == epc and f[2] == "%04x" % pc and int(f[3]) == r["seq"]
        assert f[4] == "%.9g" % (int(r["start"]) / rb.TRACKS_RATE) and int(f[5]) == r["n_flips"]
        assert [int(v) for v in f[6].split("+")] == ref.flip_list(r)
        assert np.float32(f[7]).tobytes() == r["cost"].tobytes() and f[8] == ("1" if r["entry"] >= 0 else "0")
    # the formats that were there are what they were: no new column, no new line
    assert rb.TRACKS_HEADER == "file,epc,pc,seq,t_s,h_re,h_im,mag_db,phase_rad,T" and rb.TRACKS_QUALITY_HEADER == rb.TRACKS_HEADER + ",snr_db,margin"

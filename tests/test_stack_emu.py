"""The stack stage (rfid_batch_plan_stack / rfid_batch_stack / rfid_batch_get_window_stacks / rfid_batch_stack_ms, and the per-call
rfid_stack_windows: an unknown tag's repeated EPC frames combined over the rounds of a session, built on the device behind a pass) on the
CPU: csrc/rfid_capi.hip and csrc/rfid_stack.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave emulator.
The cases that also run on the device are written once, in tests/stack_suite.py, and run here through stage_backend.Emulated; below
them, what only this side runs: the host functions of rfid.batch."""
import numpy as np
import pytest

import emu_lib
import inventory_ref
import stack_ref as ref
import stack_suite as suite
import stage_backend
from stack_suite import *


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Emulated()


@pytest.fixture
def call_ctx():
    import rfid
    ctx = rfid.Context(device=0, fixed_q=2)
    yield ctx
    ctx.close()


def test_host_functions(batch):
    """stack_fields, stack_known, format_stack and format_stack_csv on the reference's records of the batch and the inventories the
    oracle's results give"""
    from rfid import batch as rb
    rows_of, names = batch["rows"], ["a.bin", "b.bin", "c.bin", "d.bin"]
    ents = [inventory_ref.expected(o.dumps, b) for b, o in enumerate(batch["refs"])]
    assert [len(e) for e in ents][2:] == [0, 0] and len(ents[0]) >= 1
    for b, rows in enumerate(rows_of):
        f = rb.stack_fields(rows)
        failed = np.flatnonzero((rows["flags"] & 1) == 0)
        assert f["read"].tolist() == ((rows["flags"] & 1) != 0).tolist() and f["failed"].tolist() == (~f["read"]).tolist()
        assert f["stacked"].tolist() == ((rows["flags"] & 2) != 0).tolist() and f["passed"].tolist() == ((rows["flags"] & 4) != 0).tolist()
        for k, r in enumerate(rows):
            want = [] if r["flags"] & 1 else [int(failed[g]) for g in ref.members_of(r)]
            assert f["members"][k] == want and f["member_seqs"][k] == [2 * i + 1 for i in want], (b, k)
            assert (k in f["members"][k]) == (not r["flags"] & 1) and (len(want) > 1) == bool(r["flags"] & 2)
        have = {e["frame"].tobytes() for e in ents[b]}
        known = rb.stack_known(rows, ents[b])
        assert known.tolist() == [bool(r["flags"] & 4) and r["frame"].tobytes() in have for r in rows]
        ok = rows[f["passed"]]
        frames = {r["frame"].tobytes() for r in ok}
        assert rb.format_stack(rows, ents[b]) == (
            "| EPC windows : %d  failed : %d  stacked : %d  combinations that pass the CRC : %d  distinct EPCs : %d  not in the inventory : %d\n"
            % (len(rows), len(failed), int(f["stacked"].sum()), len(ok), len(frames), len(frames - have)))
    assert "distinct EPCs : 3  not in the inventory : 3\n" in rb.format_stack(rows_of[2], ents[2])      # (the decoder read nothing there)
    assert "combinations that pass the CRC : 0  distinct EPCs : 0  not in the inventory : 0\n" in rb.format_stack(rows_of[3], ents[3])
    text = rb.format_stack_csv(rows_of, ents, names)
    lines = text.splitlines()
    assert lines[0] == rb.STACK_HEADER == "file,epc,pc,seq,t_s,n_members,member_seqs,margin_min,weakest,known"
    assert len(lines) == 1 + sum(len(suite.passed(w)) for w in rows_of) and text.endswith("\n")
    i = 1
    for b, w in enumerate(rows_of):
        f = rb.stack_fields(w)
        known = rb.stack_known(w, ents[b])
        for k in np.flatnonzero((w["flags"] & 4) != 0):
            r, c = w[k], lines[i].split(",")
            pc, epc = rb.frame_fields(r["frame"])
            assert c[:4] == [names[b], epc, "%04x" % pc, str(int(r["seq"]))] and c[4] == "%.9g" % (int(r["start"]) / 400e3) and len(c) == 10
            assert c[5] == str(int(r["n_partners"]) + 1) and c[6].split("+") == [str(s) for s in f["member_seqs"][k]] and str(int(r["seq"])) in c[6].split("+")
            assert np.float32(c[7]) == r["margin_min"] and c[8] == str(int(r["weakest"])) and c[9] == str(int(known[k]))
            i += 1
    assert {ln.split(",")[0] for ln in lines[1:]} == set(names[:3])
    assert rb.format_stack_csv([], [], []) == rb.STACK_HEADER + "\n"

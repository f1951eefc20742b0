"""The commands stage (rfid_batch_plan_commands / rfid_batch_commands / rfid_batch_get_window_commands / rfid_batch_commands_ms, and the
per-call rfid_commands_of: the reader's own PIE command in front of every window, decoded on the device behind a pass) on the CPU:
csrc/rfid_capi.hip and csrc/rfid_commands.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave emulator.
The cases that also run on the device are written once, in tests/commands_suite.py, and run here through stage_backend.Emulated;
below them, what only this side runs: a launch with fewer workgroups than items, and the host functions."""
import numpy as np
import pytest

import commands_ref as ref
import commands_cases as cases
import emu_lib
import stage_backend
from commands_suite import *


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


def test_workgroups_go_round_their_loop_again(backend, ragged):
    """The ragged batch under a plan for traces seven times as long, at one row per block (the knob commands_rows): more (trace,
    row) items than the launch has workgroups (20 per compute unit, 256 of them), so a workgroup of commands_kernel takes a second
    item.  The third trace's rows lie behind the first 5 120 items: its seven windows are second items with work, behind first
    items behind a cut-off, and the rows behind them second items behind a cut-off.  The stage twice: the same table bytes"""
    import rfid
    host, lens, L, stride, refs, want, plans, dev = ragged
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, 7 * L)
        ctx.batch_plan_commands()
        ctx.set_knob("commands_rows", 1)
        backend.run_pass(ctx, dev, L, stride)
        blobs = []
        for rep in range(2):
            ctx.batch_commands_enqueue()
            blobs.append(cases.check_rows(ctx, want, rep, extra=4000))       # (every row of the table)
        assert blobs[0] == blobs[1]
        wmax = cases.table_rows(ctx, 7 * L)
        assert 5120 < 2 * wmax and 3 * wmax < 2 * 5120 and wmax < 4000, wmax
    finally:
        ctx.close()


def test_host_functions(backend, ragged):
    """command_fields, command_bits, format_commands and format_commands_csv on emulator records and crafted ones"""
    import rfid
    from rfid import batch as rb
    host, lens, L, stride, refs, want, plans, dev = ragged
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(3, L)
        ctx.batch_plan_commands()
        backend.run_pass(ctx, dev, L, stride)
        ctx.batch_commands_enqueue()
        rows = [ctx.batch_window_commands(b) for b in range(3)]
    finally:
        ctx.close()
    r, truth = rows[1], ref.plan_truth(plans[1])[:30]
    f = rb.command_fields(r)
    assert len(f) == 30 and np.array_equal(f["seq"], np.arange(30))
    names = {ref.QUERY: "query", ref.QUERY_REP: "queryrep", ref.ACK: "ack"}
    for k, (g, t) in enumerate(zip(f, truth)):
        assert (g["name"], int(g["q"]), int(g["crc5_ok"]), int(g["rn16"])) == (names[t[0]], t[1], t[2], t[3]), (k, g, t)
        assert int(g["ack_echo"]) == (-1 if t[0] != ref.ACK else (int(r["flags"][k]) >> 2) & 1) and (not t[4] or int(g["ack_echo"]) == 1)
        assert g["rtcal_us"] == 2.5 * int(r["rtcal"][k]) and g["t1_us"] == 2.5 * (704 - int(r["end"][k]))
        assert (g["trcal_us"] == 200.0) if t[0] == ref.QUERY else np.isnan(g["trcal_us"])
    assert rb.command_bits(r[1]) == "01" + format(truth[1][3], "016b") and rb.command_bits(r[0])[:4] == "1000" and len(rb.command_bits(r[0])) == 22
    n_q, n_a = sum(t[0] == ref.QUERY for t in truth), 15
    echo = int((r["flags"] & 4 != 0).sum())
    line = rb.format_commands(r)
    assert line == ("| commands : 30  query : %d  queryrep : %d  ack : %d  other : 0  none : 0  Q : {2}  failed CRC-5 : 0  "
                    "ACKs echoing the decoded RN16 : %d of %d  median RTcal us : %s  TRcal us : 200.0  T1 us : %s\n" %
                    (n_q, 15 - n_q, n_a, echo, n_a, "%.1f" % np.median(2.5 * r["rtcal"]), "%.1f" % np.median(2.5 * (704 - r["end"]))))
    assert echo >= sum(t[4] for t in truth) > 0 and line.count("\n") == 1
    # crafted records: a Query whose CRC-5 failed, an unknown command, nothing at all
    odd = np.zeros(4, dtype=rfid.capi.COMMAND_DTYPE)
    odd["seq"] = np.arange(4)
    odd[0] = r[0]
    odd[0]["flags"] &= ~2
    odd[1]["cmd"], odd[1]["n_bits"], odd[1]["bits"], odd[1]["n_syms"], odd[1]["end"], odd[1]["rtcal"] = ref.UNKNOWN, 40, 0x80000005, 43, 600, 30
    odd[2]["cmd"], odd[2]["n_bits"], odd[2]["bits"], odd[2]["n_syms"], odd[2]["end"], odd[2]["rtcal"], odd[2]["seq"] = ref.NAK, 8, 3, 11, 610, 28, 2
    line = rb.format_commands(odd)
    assert line.startswith("| commands : 4  query : 1  queryrep : 0  ack : 0  other : 2  none : 1  Q : {2}  failed CRC-5 : 1  "
                           "ACKs echoing the decoded RN16 : 0 of 0  median RTcal us : 72.5  TRcal us : 200.0  T1 us : ")
    assert rb.format_commands(odd[3:]).endswith("Q : -  failed CRC-5 : 0  ACKs echoing the decoded RN16 : 0 of 0  median RTcal us : -  TRcal us : -  T1 us : -\n")
    assert rb.command_bits(odd[1]) == "101" + "0" * 28 + "1"
    starts = [1000 + 400 * np.arange(30), np.arange(4)]
    text = rb.format_commands_csv([r, odd], starts, ["a.bin", "b.bin"])
    lines = text.splitlines()
    assert lines[0] == rb.COMMANDS_HEADER == "file,seq,t_s,cmd,n_bits,bits,q,rn16,crc5_ok,ack_echo,rtcal_us,trcal_us,t1_us" and len(lines) == 1 + 30 + 4
    for k, line in enumerate(lines[1:31]):
        c, t, g = line.split(","), truth[k], f[k]
        assert c[:2] == ["a.bin", str(k)] and c[2] == "%.9g" % (starts[0][k] / 400e3) and c[3] == names[t[0]]
        assert c[4] == str(int(r["n_bits"][k])) and c[5] == rb.command_bits(r[k])
        assert c[6] == (str(t[1]) if t[0] == ref.QUERY else "") and c[7] == ("%04x" % t[3] if t[0] == ref.ACK else "")
        assert c[8] == ("1" if t[0] == ref.QUERY else "") and c[9] == (str(int(g["ack_echo"])) if t[0] == ref.ACK else "")
        assert c[10] == "%.1f" % g["rtcal_us"] and c[11] == ("200.0" if t[0] == ref.QUERY else "") and c[12] == "%.1f" % g["t1_us"]
    assert lines[31].split(",")[8] == "0" and lines[32].startswith("b.bin,1,2.5e-06,unknown,40,101" + "0" * 28 + "1,,,,,75.0,,260.0")
    assert lines[33].startswith("b.bin,2,5e-06,nak,8,11000000,,,,,70.0,,235.0") and lines[34] == "b.bin,3,7.5e-06,none,0,,,,,,,,"

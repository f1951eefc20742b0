"""The match stage (rfid_batch_plan_match / rfid_batch_match_set_list / rfid_batch_match / rfid_batch_get_window_matches /
rfid_batch_match_ms, and the per-call rfid_match_window: known tags' frames found in CRC-failed EPC windows, built on the device behind a
pass) on the CPU: csrc/rfid_capi.hip and csrc/rfid_match.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave
emulator.  The cases that also run on the device are written once, in tests/match_suite.py, and run here through
stage_backend.Emulated; below them, what only this side runs: a trace whose inventory overflows, the host functions of rfid.batch and
frame_of_epc."""
import numpy as np
import pytest

import emu_lib
import inventory_ref
import match_ref as ref
import match_suite as suite
import stage_backend
from match_suite import *


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


def test_an_overflowed_inventory_sets_bit_1_and_searches_nothing(backend, oracle_mod, batch):
    """the batch with max_tags_per_trace = 2: the first two traces read three tags and overflow -- bit 1 in every row, nothing searched;
    the third read one tag and is searched as before; the fourth read none: bit 2"""
    import rfid
    refs = batch["refs"]
    want = [ref.expected_rows(o, oracle_mod.fir(batch["host"][b, : batch["lens"][b]]), b, None, 2) for b, o in enumerate(refs)]
    for b in (0, 1):
        assert set(want[b]["flags"]) == {ref.OVERFLOW, ref.OVERFLOW | ref.READ} and all(not r.tobytes()[16:].strip(b"\0") for r in want[b])
    assert want[2].tobytes() == batch["own"][2].tobytes() and want[3].tobytes() == batch["own"][3].tobytes()
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(suite.N, batch["L"])
        ctx.batch_plan_inventory(2)
        ctx.batch_plan_match()
        suite.own_pass(backend, ctx, batch["dev"], batch["L"], batch["stride"])
        suite.check_rows(ctx, want, "overflow")
        ctx.batch_match_set_list(batch["frames"])                     # (a list does not look at the inventory)
        ctx.batch_match_enqueue()
        suite.check_rows(ctx, batch["lst"], "overflow, list")
    finally:
        ctx.close()


def test_host_functions(batch, tmp_path):
    """match_fields against the rule restated in match_ref.policy, format_match and format_match_csv on the reference's records of the
    batch and the oracle's results; frame_of_epc and read_epc_list against the frames the synthesiser sent"""
    import rfid
    from rfid import batch as rb
    refs, names = batch["refs"], ["a.bin", "b.bin", "c.bin", "d.bin"]
    results = []
    for o in refs:
        r = np.zeros(len(o.dumps), dtype=rfid.capi.RESULT_DTYPE)
        r["h_re"], r["h_im"] = o.dumps["h_est"][:, 0], o.dumps["h_est"][:, 1]
        r["bits"] = inventory_ref.pack_frames(o.dumps["bits"])
        results.append(r)
    for rows_of in (batch["own"], batch["lst"]):
        for b, rows in enumerate(rows_of):
            f = rb.match_fields(rows)
            att = ref.policy(rows)
            assert f["attributed"].tolist() == att.tolist() and f["searched"].tolist() == (((rows["flags"] & 1) == 0) & (rows["n_cand"] > 0)).tolist()
            for k in np.flatnonzero(f["searched"]):
                r = rows[k]
                assert f["rho"][k] == np.float64(r["score_best"]) / np.float64(r["sig_abs"])
                assert f["gap_needed"][k] == (int(r["diff"]) * np.float64(r["sig_abs"]) / 128.0 if r["second"] >= 0 else 0.0)
            assert np.isnan(f["rho"][~f["searched"]]).all() and not f["attributed"][~f["searched"]].any()
            assert rb.match_fields(rows, 2.0)["attributed"].sum() == 0 and rb.match_fields(rows, -2.0)["attributed"].sum() >= att.sum()
            lines = rb.format_match(rows, results[b]).splitlines()
            got = rows[att]
            tags = sorted({r["frame"].tobytes() for r in got})
            assert lines[0] == "| EPC windows : %d  failed : %d  attributed to a known tag : %d  distinct tags : %d" % (
                len(rows), int(((rows["flags"] & 1) == 0).sum()), len(got), len(tags)) and len(lines) == 1 + len(tags)
            for ln, t in zip(lines[1:], tags):
                pc, epc = rb.frame_fields(np.frombuffer(t, dtype=np.uint32))
                reads = sum(1 for r in rows if r["flags"] & 1 and results[b][int(r["seq"])]["bits"].tobytes() == t)
                assert ln == "|   %s  %04x  reads : %d  attributed : %d" % (epc, pc, reads, sum(1 for r in got if r["frame"].tobytes() == t))
        text = rb.format_match_csv(rows_of, names, results)
        lines = text.splitlines()
        assert lines[0] == rb.MATCH_HEADER == "file,epc,pc,seq,t_s,rho,rho_second,diff,bit_errors,h_re,h_im,mag_db,phase_rad"
        assert len(lines) == 1 + sum(int(ref.policy(w).sum()) for w in rows_of) and text.endswith("\n")
        i = 1
        for b, w in enumerate(rows_of):
            f = rb.match_fields(w)
            for k in np.flatnonzero(ref.policy(w)):
                r, c, d = w[k], lines[i].split(","), results[b][int(w[k]["seq"])]
                pc, epc = rb.frame_fields(r["frame"])
                assert c[:4] == [names[b], epc, "%04x" % pc, str(int(r["seq"]))] and c[4] == "%.9g" % (int(r["start"]) / 400e3) and len(c) == 13
                assert c[5] == "%.6f" % f["rho"][k] and float(c[5]) >= 0.5 and c[7] == str(int(r["diff"])) and c[8] == str(int(r["dist_best"]))
                assert c[6] == ("" if r["second"] < 0 else "%.6f" % f["rho_second"][k])
                assert np.float32(c[9]) == d["h_re"] and np.float32(c[10]) == d["h_im"]
                h = complex(np.float64(d["h_re"]), np.float64(d["h_im"]))
                assert c[11] == "%.9g" % (20.0 * np.log10(abs(h))) and c[12] == "%.9g" % np.angle(h)
                i += 1
    assert {ln.split(",")[0] for ln in lines[1:]} == set(names)          # (list mode: every trace has sightings)
    assert rb.format_match_csv([], [], []) == rb.MATCH_HEADER + "\n"
    # frame_of_epc: PC + EPC + CRC-16, as the synthesiser sent them
    sent = batch["frames"]
    hexes = [rb.frame_fields(f) for f in sent]
    for f, (pc, epc) in zip(sent, hexes):
        assert pc == 0x3000 and rfid.frame_of_epc(epc).tobytes() == f.tobytes() == rfid.frame_of_epc(epc.upper(), pc=0x3000).tobytes()
        assert rfid.frame_of_epc(epc, pc=0x3400).tobytes() != f.tobytes()
    for bad in ("12", "g" * 24, "0" * 25):
        with pytest.raises(ValueError):
            rfid.frame_of_epc(bad)
    with pytest.raises(ValueError):
        rfid.frame_of_epc("0" * 24, pc=0x10000)
    path = tmp_path / "epcs.txt"
    forms = ("%s\n", "\n3000:%s\n", "  %s  \n")                          # (bare, PC:EPC, blanks around it)
    path.write_text("# known tags\n" + "".join(forms[i % 3] % (epc.upper() if i & 1 else epc) for i, (_, epc) in enumerate(hexes)))
    assert rb.read_epc_list(str(path)).tobytes() == sent.tobytes()

"""The diversity stage (rfid_batch_plan_diversity / rfid_batch_diversity / rfid_batch_get_window_diversity / rfid_batch_diversity_ms, and the
per-call rfid_diversity_window: the EPC windows of traces recorded together combined before the sign is taken, built on the device behind
a pass) on the CPU: csrc/rfid_capi.hip and csrc/rfid_diversity.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the
wave emulator.  The cases that also run on the device are written once, in tests/diversity_suite.py, and run here through
stage_backend.Emulated; below them, what only this side runs: the host functions of rfid.batch and the synthesiser's antennas."""
import numpy as np
import pytest

import emu_lib
import diversity_ref as ref
import diversity_suite as suite
import inventory_ref
import stage_backend
from diversity_suite import *


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
    """diversity_fields, format_diversity and format_diversity_csv on the reference's records of the batch and the members' reference
    inventories"""
    from rfid import batch as rb
    want, refs = batch["want"], batch["refs"]
    entries = [inventory_ref.expected(o.dumps, b) for b, o in enumerate(refs)]
    of_members = [entries[0:3], entries[3:6]]
    names = ["a0.bin", "b0.bin"]
    for g, rows in enumerate(want):
        f = rb.diversity_fields(rows)
        reads, combined, recovered, lone = suite.counts(rows)
        assert (int(f["read"].sum()), int(f["combined"].sum()), int(f["recovered"].sum()), int(f["lone"].sum())) == (reads, combined, recovered, lone)
        for k, r in enumerate(rows):
            assert f["members"][k] == [m for m in range(8) if int(r["present"]) >> m & 1] and f["members"][k][0] == 0
            assert f["readers"][k] == [m for m in range(8) if int(r["reads"]) >> m & 1]
            if f["combined"][k]:
                assert f["h_db"][k] == 10.0 * np.log10(np.float64(r["h_sq"])) and r["h_sq"] > 0
            else:
                assert np.isnan(f["h_db"][k])
        known = rb.diversity_known(rows, of_members[g])
        have = {e["frame"].tobytes() for ent in of_members[g] for e in ent}
        got = rows[f["recovered"]]
        assert [bool(k) for k in known[f["recovered"]]] == [r["frame"].tobytes() in have for r in got] and not known[~f["recovered"]].any()
        frames = {r["frame"].tobytes() for r in got}
        assert rb.format_diversity(rows, of_members[g]) == (
            "| EPC windows : %d  read by an antenna : %d  read by none : %d  recovered by combining : %d  distinct EPCs : %d  "
            "in no antenna's inventory : %d\n" % (len(rows), reads, len(rows) - reads, recovered, len(frames), len(frames - have)))
    assert 1 <= len({r["frame"].tobytes() for r in want[0][(want[0]["flags"] & 2) != 0]}) <= 3
    text = rb.format_diversity_csv(want, of_members, names)
    lines = text.splitlines()
    assert lines[0] == rb.DIVERSITY_HEADER == "file,epc,pc,seq,t_s,members,h_db,margin_min,weakest,known"
    assert len(lines) == 1 + sum(suite.counts(w)[2] for w in want) and text.endswith("\n")
    i = 1
    for g, w in enumerate(want):
        known = rb.diversity_known(w, of_members[g])
        for k in np.flatnonzero((w["flags"] & 2) != 0):
            r, c = w[k], lines[i].split(",")
            pc, epc = rb.frame_fields(r["frame"])
            assert c[:4] == [names[g], epc, "%04x" % pc, str(int(r["seq"]))] and c[4] == "%.9g" % (int(r["start"]) / 400e3)
            assert c[5] == "+".join(str(m) for m in range(8) if int(r["present"]) >> m & 1) and len(c) == 10
            assert c[6] == "%.4f" % (10.0 * np.log10(np.float64(r["h_sq"]))) and np.float32(c[7]) == r["margin_min"]
            assert c[8] == str(int(r["weakest"])) and c[9] == str(int(known[k]))
            i += 1
    assert {ln.split(",")[5] for ln in lines[1:]} >= {"0+1+2", "0+1", "0+2"}      # (the cut member, and the delayed one, left out)
    assert rb.format_diversity_csv([], [], []) == rb.DIVERSITY_HEADER + "\n"


def test_make_antennas_share_the_truth_and_antenna_0_without_noise_is_make_trace(synth_mod):
    """make_antennas: the truth and the slot table of make_trace with the same session arguments; antenna 0 with zero noise equals
    make_trace(noise=False) byte for byte, and with noise equals that plus add_noise_replicas' draw; every antenna's replies start at
    the same samples"""
    kw = dict(n_rounds=3, fixed_q=2, tag_ids=(1, 2, 3), seed=30, t1_jitter_raw=3)
    leak, h = 1.0 * np.exp(0.7j), 0.10 * np.exp(2.1j)                         # (make_trace's defaults)
    base = synth_mod.make_trace(noise=False, **kw)
    noisy = synth_mod.make_trace(sigma=0.03, **kw)
    traces, slots = synth_mod.make_antennas([leak, 0.5j], [h, 0.05], 0.0, [7, 8], **kw)
    assert len(traces) == 2 and traces[0].samples.tobytes() == base.samples.tobytes()
    assert traces[0].samples.dtype == np.complex64 and traces[0].samples.flags.c_contiguous
    for t in traces:
        assert t.slots == base.slots == noisy.slots == slots and t.plan.slots.tobytes() == base.plan.slots.tobytes() == noisy.plan.slots.tobytes()
        assert len(t.samples) == len(base.samples)
    assert traces[1].samples.tobytes() != base.samples.tobytes()
    with_noise, _ = synth_mod.make_antennas([leak, 0.5j], [h, 0.05], 0.03, [7, 8], **kw)
    for m, t in enumerate(with_noise):
        assert t.samples.tobytes() == synth_mod.add_noise_replicas(traces[m].samples, 1, 0.03, 7 + m)[0].tobytes()
    assert with_noise[0].samples.tobytes() != with_noise[1].samples.tobytes()
    for bad in (dict(leak=1.0), dict(h=0.1), dict(noise=False), dict(render=False)):
        with pytest.raises(ValueError):
            synth_mod.make_antennas([leak], [h], 0.0, [1], **dict(kw, **bad))
    for args in (([leak], [h, h], 0.0, [1]), ([leak], [h], 0.0, [1, 2]), ([], [], 0.0, [])):
        with pytest.raises(ValueError):
            synth_mod.make_antennas(*args, **kw)

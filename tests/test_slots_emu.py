"""The slots stage (rfid_batch_plan_slots / rfid_batch_slots / rfid_batch_get_window_moments / rfid_batch_slots_ms, and the per-call
rfid_window_moments_of: the second-order moments of every window's gated samples, built on the device behind a pass) on the CPU:
csrc/rfid_capi.hip and csrc/rfid_slots.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave emulator.
The cases that also run on the device are written once, in tests/slots_suite.py, and run here through stage_backend.Emulated; below
them, what only this side runs: the classification of the five shapes against the reference alone, and the host functions."""
import numpy as np
import pytest

import slots_ref as ref
import slots_cases as cases
import emu_lib
import stage_backend
from slots_suite import *


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


@pytest.fixture(scope="module")
def classified(backend, oracle_mod, synth_mod):
    """the five shapes at sigma = 0.01, each through a pass of its own context: -> per shape (trace, emulator records)"""
    return cases.five_shapes(backend, oracle_mod, synth_mod)


def test_classification_agrees_with_the_truth_on_the_five_shapes(classified):
    """classify_slots == SlotTruth for EVERY slot of every shape (no slot may be left out), == the restatement of slots_ref; the
    reference classification itself is within that on these inputs"""
    from rfid import batch as rb
    for shape, (t, rows) in zip(ref.SHAPES, classified):
        assert [c[:2] for c in ref.classify(rows)] == ref.truth(t.slots), shape        # (the reference alone)
    cases.check_five_shapes(rb, classified)
    t, rows = classified[2]
    assert sum(s.n_tags >= 2 for s in t.slots) == 22 and len(t.slots) == 24            # (most slots collide: the floor is the EPC windows')


def test_host_functions(classified):
    """moment_fields, estimate_population, suggest_q, format_slots and format_slots_csv on emulator records and crafted ones"""
    from rfid import batch as rb
    t, rows = classified[4]
    l1, l2 = rb.moment_fields(rows)
    assert l1.dtype == np.float64 and (l1 >= l2).all() and (l2 >= 0).all()
    for k in (0, len(rows) - 1):
        e = ref.eig(rows[k])
        assert abs(l1[k] - e[0]) <= 1e-15 * e[0] and abs(l2[k] - e[1]) <= 1e-15 * e[0]
    # a noise-free trace has no floor: nothing is classified
    flat = np.zeros(6, dtype=rows.dtype)
    flat["seq"] = np.arange(6)
    none = rb.classify_slots(flat)
    assert len(none) == 3 and (none["cls"] == -1).all() and (none["answered"] == 0).all()
    assert "not classified" in rb.format_slots(none, 2)
    assert len(rb.classify_slots(rows[:1])) == 0 and len(rb.classify_slots(rows[:5])) == 2          # (a last RN16 without its EPC)
    assert rb.estimate_population(np.array([1, 1, 2, 0, 2, -1]), 2) == (2 + 2.39 * 2) / 2 and rb.estimate_population([], 0) == 0.0
    assert [rb.suggest_q(n) for n in (0, 1, 1.4, 1.5, 3, 5.6, 5.7, 100, 1e9)] == [0, 0, 0, 1, 2, 2, 3, 7, 15]
    slots = rb.classify_slots(rows)
    line = rb.format_slots(slots, 2)
    cls = slots["cls"]
    assert line.startswith("| slots : 16  empty : %d  single : %d  collided : %d  answered : %d  read : %d  efficiency : %.3f  " %
                           ((cls == 0).sum(), (cls == 1).sum(), (cls == 2).sum(), slots["answered"].sum(), slots["crc_ok"].sum(),
                            slots["crc_ok"].sum() / 16.0))
    assert line.endswith("suggested Q : 2 (in use : 2)\n") and line.count("\n") == 1 and "tags per round : 4.14" in line
    starts = 1000 + 400 * np.arange(len(rows))
    text = rb.format_slots_csv([slots, none], [starts, np.arange(6)], ["a.bin", "b.bin"])
    lines = text.splitlines()
    assert lines[0] == rb.SLOTS_HEADER == "file,slot,seq,t_s,class,l1_db,l2_db,floor_db,answered,crc_ok" and len(lines) == 1 + 16 + 3
    names = {0: "empty", 1: "single", 2: "collided"}
    for k, line in enumerate(lines[1:17]):
        f = line.split(",")
        s = slots[k]
        assert f[:3] == ["a.bin", str(k), str(2 * k)] and f[3] == "%.9g" % (starts[2 * k] / 400e3) and f[4] == names[int(s["cls"])]
        assert [float(v) for v in f[5:8]] == [float("%.9g" % (10 * np.log10(s[n]))) for n in ("l1", "l2", "floor")]
        assert f[8:] == [str(int(s["answered"])), str(int(s["crc_ok"]))]
    assert lines[17].startswith("b.bin,0,0,0,unknown,-inf,-inf,-inf,0,0")

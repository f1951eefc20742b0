"""The collisions stage (rfid_batch_plan_collisions / rfid_batch_collisions / rfid_batch_get_window_collisions /
rfid_batch_collisions_ms, and the per-call rfid_collisions_of: both RN16s and both channels of every RN16 window, as of two tags
replying at once, built on the device behind a pass) on the CPU: csrc/rfid_capi.hip and csrc/rfid_collide.hpp, unmodified, through
tests/fake_hip's library -- the kernels run on the wave emulator.  The cases that also run on the device are written once, in
tests/collide_suite.py, and run here through stage_backend.Emulated; below them, what only this side runs: the host functions of
rfid.batch."""
import numpy as np
import pytest

import collide_ref as ref
import emu_lib
import stage_backend
from collide_suite import *


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


def test_host_functions(oracle_mod, ragged):
    """collision_fields, classify_collisions, format_collisions and format_collisions_csv on the reference's records of the ragged
    batch; the default order_k lies between the bounds measured on the two-tag slots and on the slots with three or more tags"""
    import slots_ref
    from rfid import batch as rb
    host, lens, L, stride, refs, want, truth, _ = ragged
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(4)]
    slots = [rb.classify_slots(slots_ref.expected(o, y, b)) for b, (o, y) in enumerate(zip(refs, ys))]
    rows = want[1]
    f = rb.collision_fields(rows)
    assert all(f[k].dtype == np.float64 for k in ("ha_db", "hb_db", "ratio_db", "phase_rad", "fit")) and (f["ratio_db"] <= 0).all()
    ha = rows["ha_re"].astype(np.float64) + 1j * rows["ha_im"].astype(np.float64)
    hb = rows["hb_re"].astype(np.float64) + 1j * rows["hb_im"].astype(np.float64)
    assert (f["ha_db"] == 20 * np.log10(np.abs(ha))).all() and (f["phase_rad"] == np.angle(hb * np.conj(ha))).all()
    assert (f["fit"] == ref.fit(rows)).all() and np.allclose(f["ratio_db"], 20 * np.log10(np.abs(hb) / np.abs(ha)), rtol=0, atol=1e-9)
    assert list(f["decoded"]) == ["a" if r["flags"] & 1 else ("b" if r["flags"] & 2 else "-") for r in rows]
    zero = np.zeros(1, dtype=rb.capi.COLLISION_DTYPE)
    assert np.isnan(rb.collision_fields(zero)["fit"][0])
    two_fit, more_fit, collided = [], [], []
    for b in range(4):
        col = rb.classify_collisions(want[b], slots[b])
        collided.append(col)
        cls = [k for k in range(len(slots[b])) if slots[b]["cls"][k] == rb.SLOT_COLLIDED]
        assert list(col["slot"]) == cls and list(col["seq"]) == [2 * k for k in cls]
        assert cls == [k for k, (n, _) in enumerate(truth[b]) if n >= 2]                 # (the slots stage sees every collision here)
        for c in col:
            n_tags, handles = truth[b][int(c["slot"])]
            assert int(c["order"]) == (2 if n_tags == 2 else 3), (b, c)
            (two_fit if n_tags == 2 else more_fit).append(float(c["fit"]))
            if n_tags == 2:
                assert {int(c["rn16_a"]), int(c["rn16_b"])} == set(handles)
    # (the bounds in classify_collisions' docstring are over these traces and the crowded one of tests/test_gpu_collide.py)
    assert len(collided[2]) == 0 and max(two_fit) <= 0.0151 < rb.COLLISION_ORDER_K < 0.150 <= min(more_fit)
    assert (rb.classify_collisions(want[1], slots[1], order_k=0.0)["order"] == 3).all()
    line = rb.format_collisions(collided[1])
    two = collided[1][collided[1]["order"] == 2]
    assert line == ("| collided slots : %d  two tags : %d  more : %d  decoder's RN16 the stronger tag's : %d  the weaker's : %d  neither's : %d  "
                    "median |hB|/|hA| dB : %.2f\n" % (len(collided[1]), len(two), len(collided[1]) - len(two), (two["decoded"] == "a").sum(),
                                                      (two["decoded"] == "b").sum(), (two["decoded"] == "-").sum(), np.median(two["ratio_db"])))
    assert rb.format_collisions(collided[2]).endswith("two tags : 0  more : 0  decoder's RN16 the stronger tag's : 0  the weaker's : 0  "
                                                      "neither's : 0  median |hB|/|hA| dB : -\n")
    names = ["a.bin", "b.bin", "c.bin", "d.bin"]
    starts = [o.open_idx for o in refs]
    text = rb.format_collisions_csv(collided, starts, names)
    lines = text.splitlines()
    assert lines[0] == rb.COLLISIONS_HEADER == "file,slot,seq,t_s,rn16_a,rn16_b,ha_re,ha_im,hb_re,hb_im,ratio_db,fit,order,decoded"
    assert len(lines) == 1 + sum(map(len, collided)) and text.endswith("\n")
    i = 1
    for b, col in enumerate(collided):
        for c in col:
            v = lines[i].split(",")
            r = want[b][int(c["slot"])]
            assert v[:3] == [names[b], str(int(c["slot"])), str(int(r["seq"]))] and v[3] == "%.9g" % (int(starts[b][int(r["seq"])]) / 400e3)
            assert v[4:6] == ["%04x" % r["rn16_a"], "%04x" % r["rn16_b"]] and v[12:] == [str(int(c["order"])), str(c["decoded"])]
            assert [np.float32(x) for x in v[6:10]] == [r["ha_re"], r["ha_im"], r["hb_re"], r["hb_im"]]
            assert v[10] == "%.9g" % c["ratio_db"] and v[11] == "%.9g" % c["fit"]
            i += 1
    assert rb.format_collisions_csv([], [], []) == rb.COLLISIONS_HEADER + "\n"

"""The retune stage (rfid_batch_plan_retune / rfid_batch_retune / rfid_batch_get_window_retunes / rfid_batch_retune_ms, and the per-call
rfid_retune_window: CRC-failed EPC windows decoded again with the half-bit period searched over the Gen2 BLF tolerance, built on the
device behind a pass) on the CPU: csrc/rfid_capi.hip and csrc/rfid_retune.hpp, unmodified, through tests/fake_hip's library -- the
kernels run on the wave emulator.  The cases that also run on the device are written once, in tests/retune_suite.py, and run here
through stage_backend.Emulated; below them, what only this side runs: the host functions of rfid.batch and the synthesiser's offsets."""
import hashlib

import numpy as np
import pytest

import emu_lib
import stage_backend
from retune_suite import *


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
    """retune_fields, retune_known, format_retune and format_retunes_csv on the reference's records of the ragged batch"""
    import inventory_ref as inv
    from rfid import batch as rb
    host, lens, L, stride, refs, want, slots, _ = ragged
    ents = [inv.expected(o.dumps, b) for b, o in enumerate(refs)]
    rows, ent = want[0], ents[0]
    f = rb.retune_fields(rows)
    got, read = (rows["flags"] & 2) != 0, (rows["flags"] & 1) != 0
    assert f["blf_khz"].dtype == np.float64 and (f["retuned"] == got).all() and not f["clamped"].any()
    assert np.isnan(f["blf_khz"][read]).all() and np.isnan(f["blf_off_pct"][read]).all() and not np.isnan(f["blf_khz"][~read]).any()
    T = rows["T"][~read].astype(np.float64)
    assert (f["blf_khz"][~read] == 200.0 / T).all() and np.allclose(f["blf_off_pct"][~read], 100.0 * (5.0 / T - 1.0), rtol=0, atol=1e-12)
    # the first trace's tags: -4 % and +4 % in half-bit length are +4.17 % and -3.85 % in frequency; the one on frequency is read
    off = f["blf_off_pct"][got]
    assert ((np.abs(off - 100 * (1 / 0.96 - 1)) < 0.45) | (np.abs(off - 100 * (1 / 1.04 - 1)) < 0.45)).all() and (off > 0).any() and (off < 0).any()
    known = rb.retune_known(rows, ent)
    assert known.dtype == bool and not known.any() and not rb.retune_known(rows, ent[:0]).any()      # (tags the pass never read)
    mine = ent[:1].copy()
    k = int(np.flatnonzero(got)[0])
    mine["frame"][0] = rows["frame"][k]
    same = (rows["frame"] == rows["frame"][k]).all(axis=1) & got
    assert (rb.retune_known(rows, mine) == same).all() and same.sum() >= 1
    line = rb.format_retune(rows, ent)
    frames = {bytes(np.ascontiguousarray(r["frame"])) for r in rows[got]}
    assert len(frames) == 2                                                                        # (the two tags off frequency)
    assert line == ("| failed EPC windows : %d  retuned : %d  distinct EPCs : 2  not in the inventory : 2  BLF offset median : %+.2f %%  "
                    "min : %+.2f %%  max : %+.2f %%\n" % ((~read).sum(), got.sum(), np.median(off), off.min(), off.max()))
    assert "not in the inventory : %d " % (2 - 1) in rb.format_retune(rows, mine)
    assert rb.format_retune(want[2], ents[2]).endswith("retuned : 0  distinct EPCs : 0  not in the inventory : 0  BLF offset median : -  min : -  max : -\n")
    names = ["a.bin", "b.bin", "c.bin", "d.bin"]
    text = rb.format_retunes_csv(want, ents, names)
    lines = text.splitlines()
    assert lines[0] == rb.RETUNES_HEADER == "file,epc,pc,seq,t_s,T,blf_khz,blf_off_pct,h_re,h_im,clamped,known"
    assert len(lines) == 1 + sum(int(((w["flags"] & 2) != 0).sum()) for w in want) and text.endswith("\n")
    i = 1
    for b, w in enumerate(want):
        for r in w[(w["flags"] & 2) != 0]:
            c = lines[i].split(",")
            pc, epc = rb.frame_fields(r["frame"])
            assert c[:4] == [names[b], epc, "%04x" % pc, str(int(r["seq"]))] and c[4] == "%.9g" % (int(r["start"]) / 400e3)
            assert np.float32(c[5]) == r["T"] and np.float32(c[8]) == r["h_re"] and np.float32(c[9]) == r["h_im"]
            assert abs(float(c[6]) - 200.0 / float(r["T"])) < 1e-6 and abs(float(c[7]) - 100 * (5 / float(r["T"]) - 1)) < 1e-4
            assert c[10:] == ["0", "0"]
            i += 1
    assert rb.format_retunes_csv([], [], []) == rb.RETUNES_HEADER + "\n"


def test_synthesiser_offsets_of_none_or_zero_change_no_byte(synth_mod):
    """make_trace with blf_offsets None or zeros gives the samples it gave before the argument existed (their SHA-256, recorded from
    the synthesiser as it was), with and without it the same draws; an offset stretches every reply of its tag and nothing else"""
    kw = dict(n_rounds=3, fixed_q=2, tag_ids=(1, 2, 3), seed=30, sigma=0.03, t1_jitter_raw=3)
    a = synth_mod.make_trace(**kw)
    assert len(a.samples) == 177886
    assert hashlib.sha256(a.samples.tobytes()).hexdigest() == "b1ac72dc8b12d713acaea140f0cb9e58a53e886b0ca1c574fa1fd69d96c8d933"
    for off in (None, (0, 0, 0), (0.0, -0.0, 0)):
        b = synth_mod.make_trace(blf_offsets=off, **kw)
        assert b.samples.tobytes() == a.samples.tobytes() and b.plan.slots.tobytes() == a.plan.slots.tobytes()
    c = synth_mod.make_trace(blf_offsets=(0.04, 0, 0), **kw)
    assert len(c.samples) == len(a.samples) and [s.epc for s in c.slots] == [s.epc for s in a.slots]
    assert [s.epc_raw_start for s in c.slots] == [s.epc_raw_start for s in a.slots]
    diff = np.flatnonzero(c.samples != a.samples)
    assert len(diff) > 1000
    mine = [(s.rn16_raw_start, s.epc_raw_start) for s in a.slots if s.n_tags == 1 and s.tag_id == 1]
    others = [s for s in a.slots if s.n_tags == 1 and s.tag_id != 1]
    assert mine and others
    for s in others:                                             # (another tag's replies: not a sample differs)
        assert not ((diff >= s.epc_raw_start) & (diff < s.epc_raw_start + 25 * 270)).any()
    # the level at raw sample n of a reply is levels[floor(n / (25 (1 + d)))]: noise-free, one tag, the reply's own samples
    d = 0.04
    t = synth_mod.make_trace(n_rounds=1, fixed_q=0, tag_ids=(7,), seed=2, noise=False, blf_offsets=(d,))
    base = synth_mod.make_trace(n_rounds=1, fixed_q=0, tag_ids=(7,), seed=2, noise=False)
    s = t.slots[0]
    lv = synth_mod.fm0_levels(s.epc)
    n = np.arange(int(np.ceil(len(lv) * 25 * (1 + d))))
    want = lv[np.floor(n / (25 * (1 + d))).astype(int)]
    leak = base.samples[s.epc_raw_start - 10]
    h = (base.samples[s.epc_raw_start] - leak)                   # (the first half-bit of the preamble is a 1)
    got = (t.samples[s.epc_raw_start: s.epc_raw_start + len(n)] - leak) / h
    assert np.abs(got - want).max() < 1e-4
    with pytest.raises(ValueError):
        synth_mod.make_trace(render=False, blf_offsets=(0.01,))
    with pytest.raises(ValueError):
        synth_mod.make_trace(blf_offsets=(0.01, 0.02))
    assert synth_mod.make_trace(n_rounds=1, render=False, blf_offsets=(0.0,)).samples is None

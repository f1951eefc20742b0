"""The lengths stage (rfid_batch_plan_lengths / rfid_batch_lengths / rfid_batch_get_window_lengths / rfid_batch_lengths_ms, and the per-call
rfid_length_window: CRC-failed EPC windows read again at the length their own PC word announces, built on the device behind a pass)
on the CPU: csrc/rfid_capi.hip and csrc/rfid_lengths.hpp, unmodified, through tests/fake_hip's library -- the kernels run on the wave
emulator.  The cases that also run on the device are written once, in tests/lengths_suite.py, and run here through
stage_backend.Emulated; below them, what only this side runs: the host functions of rfid.batch and the synthesiser's EPC lengths."""
import hashlib

import numpy as np
import pytest

import emu_lib
import lengths_ref as ref
import stage_backend
from lengths_suite import *


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


def test_host_functions(ragged):
    """sized_frame_fields, format_lengths and format_lengths_csv on the reference's records of the ragged batch"""
    import repair_ref
    from rfid import batch as rb
    host, lens, L, stride, refs, want, slots, _ = ragged
    rows = want[0]
    got = rows[(rows["flags"] & 2) != 0]
    for r in got:
        pc, epc, epc_bits = rb.sized_frame_fields(r)
        bits = "".join(map(str, ref.frame_bits(r)))
        assert epc_bits == int(r["n_bits"]) - 32 == 16 * int(r["words"]) and pc == int(bits[:16], 2) == int(r["words"]) << 11
        assert len(epc) == epc_bits // 4 and int(epc, 16) == int(bits[16:-16], 2)
    with pytest.raises(ValueError):
        rb.sized_frame_fields(rows[(rows["flags"] & 1) != 0][0])
    # the first trace's tags: a 128-, a 64- and a 96-bit EPC -- the last is read, the others are found here, one EPC each
    n128, n64 = int((got["n_bits"] == 160).sum()), int((got["n_bits"] == 96).sum())
    assert n128 >= 1 and n64 >= 1 and n128 + n64 == len(got)
    assert rb.format_lengths(rows) == ("| failed EPC windows : %d  pass at the PC's length : %d  distinct EPCs : 2  by EPC length : 64-bit : %d  "
                                       "128-bit : %d  longer than the slot : %d\n" %
                                       (((rows["flags"] & 1) == 0).sum(), len(got), n64, n128, ((rows["flags"] & 8) != 0).sum()))
    assert ((rows["flags"] & 8) != 0).sum() >= 1
    assert rb.format_lengths(want[2]).startswith("| failed EPC windows : %d  pass at the PC's length : 0  distinct EPCs : 0  by EPC length : -  "
                                                 "longer than the slot : " % ((want[2]["flags"] & 1) == 0).sum())
    # a PC alone: no EPC digits
    pc_only = [r for r in want[1] if r["flags"] & 2 and r["n_bits"] == 32]
    assert pc_only and rb.sized_frame_fields(pc_only[0]) == (0, "", 0)
    names = ["a.bin", "b.bin", "c.bin", "d.bin"]
    results = [np.array([repair_ref.result_of_dump(d) for d in o.dumps]) for o in refs]
    text = rb.format_lengths_csv(want, names, results)
    lines = text.splitlines()
    assert lines[0] == rb.LENGTHS_HEADER == "file,epc,pc,epc_bits,seq,t_s,T,h_re,h_im,clamped"
    assert len(lines) == 1 + sum(int(((w["flags"] & 2) != 0).sum()) for w in want) and text.endswith("\n")
    i = 1
    for b, w in enumerate(want):
        for r in w[(w["flags"] & 2) != 0]:
            c = lines[i].split(",")
            pc, epc, epc_bits = rb.sized_frame_fields(r)
            d = refs[b].dumps[int(r["seq"])]
            assert c[:5] == [names[b], epc, "%04x" % pc, str(epc_bits), str(int(r["seq"]))] and c[5] == "%.9g" % (int(r["start"]) / 400e3)
            assert np.float32(c[6]) == d["T"] and np.float32(c[7]) == d["h_est"][0] and np.float32(c[8]) == d["h_est"][1]
            assert c[9:] == ["0"]
            i += 1
    assert rb.format_lengths_csv([], [], []) == rb.LENGTHS_HEADER + "\n"


def test_synthesiser_lengths_of_none_or_96_change_no_byte(synth_mod):
    """make_trace with epc_bits None or all 96 gives the samples and the slot table it gave before the argument existed (the samples'
    SHA-256, recorded from the synthesiser as it was); another length changes that tag's EPC replies and nothing else"""
    kw = dict(n_rounds=3, fixed_q=2, tag_ids=(1, 2, 3), seed=30, sigma=0.03, t1_jitter_raw=3)
    a = synth_mod.make_trace(**kw)
    assert len(a.samples) == 177886
    assert hashlib.sha256(a.samples.tobytes()).hexdigest() == "b1ac72dc8b12d713acaea140f0cb9e58a53e886b0ca1c574fa1fd69d96c8d933"
    for bits in (None, (96, 96, 96), [96.0, 96, 96]):
        b = synth_mod.make_trace(epc_bits=bits, **kw)
        assert b.samples.tobytes() == a.samples.tobytes() and b.plan.slots.tobytes() == a.plan.slots.tobytes()
        assert [s.epc for s in b.slots] == [s.epc for s in a.slots]
    plan = synth_mod.make_trace(render=False, epc_bits=(96, 96, 96), **kw)
    assert plan.samples is None and plan.plan.slots.tobytes() == a.plan.slots.tobytes()
    c = synth_mod.make_trace(epc_bits=(128, 96, 96), **kw)
    assert len(c.samples) == len(a.samples) and c.plan is None
    assert [s.epc_raw_start for s in c.slots] == [s.epc_raw_start for s in a.slots] and [s.rn16 for s in c.slots] == [s.rn16 for s in a.slots]
    diff = np.flatnonzero(c.samples != a.samples)
    mine = [s for s in c.slots if s.n_tags == 1 and s.tag_id == 1]
    others = [(s, t) for s, t in zip(c.slots, a.slots) if not (s.n_tags == 1 and s.tag_id == 1)]
    assert mine and others and len(diff) > 1000
    inside = np.zeros(len(diff), dtype=bool)
    for s in mine:                                               # (every changed sample lies in one of that tag's EPC replies)
        assert len(s.epc) == 160 and s.epc_valid and s.epc[:16] == synth_mod.pc_for_words(8) and s.epc[136:144] == [0, 0, 0, 0, 0, 0, 0, 1]
        assert s.epc[144:] == synth_mod.crc16(s.epc[:144])
        inside |= (diff >= s.epc_raw_start) & (diff < s.epc_raw_start + 25 * (12 + 2 * 161))
    assert inside.all()
    for s, t in others:
        assert s.epc == t.epc and (s.epc is None or len(s.epc) == 128)
    # the frame's levels: noise-free, one tag, the reply's own samples -- and it ends 150 us before the carrier does
    t = synth_mod.make_trace(n_rounds=1, fixed_q=0, tag_ids=(7,), seed=2, noise=False, epc_bits=(128,))
    base = synth_mod.make_trace(n_rounds=1, fixed_q=0, tag_ids=(7,), seed=2, noise=False)
    s = t.slots[0]
    lv = np.repeat(synth_mod.fm0_levels(s.epc), 25)
    leak = base.samples[s.epc_raw_start - 10]
    h = base.samples[s.epc_raw_start] - leak                     # (the first half-bit of the preamble is a 1)
    got = (t.samples[s.epc_raw_start: s.epc_raw_start + len(lv)] - leak) / h
    assert np.abs(got - lv).max() < 1e-4 and len(lv) == 2 * 4175
    assert 2 * (synth_mod.T1_US + 4175 + 150) == 2 * synth_mod.CW_ACK
    for bits, n in ((0, 32), (16, 48), (80, 112), (112, 144)):
        s = synth_mod.make_trace(n_rounds=1, fixed_q=0, tag_ids=(7,), seed=2, epc_bits=(bits,)).slots[0]
        assert len(s.epc) == n and s.epc[:5] == [(bits // 16 >> i) & 1 for i in (4, 3, 2, 1, 0)] and s.epc[-16:] == synth_mod.crc16(s.epc[:-16])
        assert bits == 0 or s.epc[n - 24:n - 16] == [0, 0, 0, 0, 0, 1, 1, 1]
    for bad in (dict(render=False, epc_bits=(128,)), dict(epc_bits=(96, 96)), dict(epc_bits=(100,)), dict(epc_bits=(144,)), dict(epc_bits=(-16,)),
                dict(epc_bits=(128,), blf_offsets=(0.04,))):
        with pytest.raises(ValueError):
            synth_mod.make_trace(**bad)
    assert synth_mod.make_trace(n_rounds=1, epc_bits=(128,), blf_offsets=(0.03,)).samples is not None
    assert synth_mod.make_trace(n_rounds=1, epc_bits=(96,), blf_offsets=(0.04,)).samples is not None     # (as before the argument existed)

"""The inventory stage (rfid_batch_plan_inventory / rfid_batch_inventory / rfid_batch_get_inventory: the distinct 128-bit EPC frames of
every trace, built on the device) on the CPU: csrc/rfid_capi.hip and csrc/rfid_inventory.hpp, unmodified, through tests/fake_hip's
library -- the kernels run on the wave emulator.  Every expected inventory is worked out in numpy from the ORACLE's per-window dumps
(tests/inventory_ref.py), never from the library's own results, and every comparison is exact.

The traces: rfid.synth.make_trace draws a random 88-bit head per tag, so tag_ids = (0x27, 0x27, 0x31) are three different EPCs of
which two share the byte tag_reads[] is keyed by.  Seeds 104 (4 rounds) and 112 (3 rounds), FIXED_Q = 2: the oracle alone reads all
three frames in each, the two 0x27 frames apart, every frame at least twice (asserted below before anything is compared)."""
import ctypes as C

import numpy as np
import pytest

import inventory_ref as ref
import emu_lib
from emu_lib import oracle_runs as _oracle, run_pass as _pass
from stage_backend import lay_out

TAGS = (0x27, 0x27, 0x31)
SEEDS = ((104, 4), (112, 3))       # (seed, inventory rounds) per trace


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


def _batch(synth_mod, **kw):
    ts = [synth_mod.make_trace(n_rounds=n, fixed_q=2, tag_ids=TAGS, seed=seed, sigma=0.02, t1_jitter_raw=3, **kw).samples
          for seed, n in SEEDS]
    return lay_out(ts, shorten=777)            # (ragged also where the longest trace is concerned)


@pytest.fixture(scope="module")
def batch(oracle_mod, synth_mod):
    host, lens, L, stride = _batch(synth_mod)
    refs = _oracle(oracle_mod, host, lens)
    want, want_counts = ref.expected_batch([o.dumps for o in refs])
    # the input does what the case is about, by the oracle alone: two different frames that end in the same byte, and repeated reads
    for b in range(len(lens)):
        e = want[want["stream"] == b]
        assert len(e) == 3 and (e["tag_id"] == 0x27).sum() == 2 and (e["reads"] >= 2).all(), (b, e)
        assert len({bytes(f) for f in e["frame"]}) == 3
    return host, lens, L, stride, refs, want, want_counts


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_inventory_of_a_ragged_batch_equals_the_oracles(batch, mode):
    """Two traces, both front ends; the pass run twice: the same inventory both times; then the same pass listed again through tables
    of 4 slots (three frames in four slots: probes collide, the later rounds run) and of 2 slots (more frames than slots: overflow)."""
    import rfid
    host, lens, L, stride, refs, want, want_counts = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(mode)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(8)
        first = None
        for rep in range(2):
            _pass(ctx, host, lens, L, stride)
            ent, counts = ctx.batch_inventory()
            st = ctx.batch_stats()
            ref.assert_equal(ent, counts, want, want_counts, (mode, rep))
            ref.cross_check(ent, counts, st)
            for b, o in enumerate(refs):
                assert st[b]["n_epc_correct"] == o.state.n_epc_correct and st[b]["n_unique_tags"] == 2     # (one byte: two "tags")
            first = first if first is not None else ent.tobytes()
            assert ent.tobytes() == first
        assert ctx.batch_inventory_ms() >= 0.0
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if mode == 2 else rep["pieces"] == 0, rep
        # forced collisions: the workspace is planned again, the pass stays
        ctx.set_knob("inventory_slots", 4)
        ctx.batch_plan_inventory(4)
        ent, counts = ctx.batch_inventory()
        ref.assert_equal(ent, counts, want, want_counts, "4 slots")
        ctx.batch_plan_inventory(3)
        ent, counts = ctx.batch_inventory()
        ref.assert_equal(ent, counts, want, want_counts, "4 slots, max_tags 3")
        ctx.set_knob("inventory_slots", 2)
        ctx.batch_plan_inventory(4)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory()
        assert e.value.status == rfid.capi.ERR_CAPACITY and "trace 0" in str(e.value)
        ctx.set_knob("inventory_slots", 0)
        with pytest.raises(rfid.capi.RfidError):
            ctx.set_knob("inventory_slots", 2048)
        ctx.set_knob("inventory_slots", 6)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_plan_inventory(4)                 # (not a power of two)
        assert e.value.status == rfid.capi.ERR_INVALID
    finally:
        ctx.close()


def test_only_one_trace_of_the_plan(batch):
    """rfid_batch_set_streams: the inventory covers the rows the pass covered"""
    import rfid
    host, lens, L, stride, refs, want, want_counts = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(8)
        ctx.batch_set_streams(1)
        _pass(ctx, host, lens, L, stride)
        ent, counts = ctx.batch_inventory()
        ref.assert_equal(ent, counts, want[want["stream"] == 0], want_counts[:1])
    finally:
        ctx.close()


def test_reads_behind_the_cut_off_are_not_counted(oracle_mod, batch):
    """MAX_NUM_QUERIES reached inside the traces (gate_impl.cc:101-109): the inventory stops where tag_reads[] stops"""
    import rfid
    host, lens, L, stride, full_refs, full_want, _ = batch
    refs = _oracle(oracle_mod, host, lens, max_num_queries=7)
    want, want_counts = ref.expected_batch([o.dumps for o in refs])
    assert all(o.state.status == 1 and o.n_windows < f.n_windows for o, f in zip(refs, full_refs))
    assert 0 < int(want["reads"].sum()) < int(full_want["reads"].sum())          # (the cut-off takes reads away, and leaves some)
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=7)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(8)
        _pass(ctx, host, lens, L, stride)
        ent, counts = ctx.batch_inventory()
        st = ctx.batch_stats()
        assert [int(s["n_windows_used"]) for s in st] == [o.n_windows for o in refs]
        ref.assert_equal(ent, counts, want, want_counts)
        ref.cross_check(ent, counts, st)
    finally:
        ctx.close()


def test_a_frame_whose_crc_fails_is_in_no_entry(oracle_mod, synth_mod):
    import rfid
    host, lens, L, stride = _batch(synth_mod, corrupt_rounds=(1, 2))
    refs = _oracle(oracle_mod, host, lens)
    bad = [o.dumps[(o.dumps["type"] == 1) & (o.dumps["crc_ok"] == 0)] for o in refs]
    assert all(len(b) >= 2 for b in bad)
    want, want_counts = ref.expected_batch([o.dumps for o in refs])
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        ctx.batch_plan_inventory(8)
        _pass(ctx, host, lens, L, stride)
        ent, counts = ctx.batch_inventory()
        ref.assert_equal(ent, counts, want, want_counts)
        ref.cross_check(ent, counts, ctx.batch_stats())
        listed = {bytes(f) for f in ent["frame"]}
        for s, b in enumerate(bad):
            # the input does what the case is about: the oracle decoded a frame one bit away from a listed one, and its CRC failed
            near = [int(np.unpackbits((x ^ y).view(np.uint8)).sum()) for x in ref.pack_frames(b["bits"]) for y in want["frame"][want["stream"] == s]]
            assert 1 in near, (s, sorted(near)[:4])
            # (a corrupted frame differs from its tag's frame in one bit: it must not appear as an entry of its own)
            assert not ({bytes(f) for f in ref.pack_frames(b["bits"])} & listed)
    finally:
        ctx.close()


def test_capacity_and_state_errors(batch):
    import rfid
    host, lens, L, stride, refs, want, want_counts = batch
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_plan_inventory(8)                  # no plan
        assert e.value.status == rfid.capi.ERR_STATE
        ctx.batch_set_long_stream(0)
        ctx.batch_plan(2, L)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory()                        # no inventory workspace
        assert e.value.status == rfid.capi.ERR_STATE
        for bad in (0, -3):
            with pytest.raises(rfid.capi.RfidError) as e:
                ctx.batch_plan_inventory(bad)
            assert e.value.status == rfid.capi.ERR_INVALID
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_plan_inventory(513)
        assert e.value.status == rfid.capi.ERR_UNSUPPORTED
        ctx.batch_plan_inventory(1)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory()                        # no pass yet
        assert e.value.status == rfid.capi.ERR_STATE
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory_fetch()                  # nothing enqueued
        assert e.value.status == rfid.capi.ERR_STATE
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory_ms()
        assert e.value.status == rfid.capi.ERR_STATE
        _pass(ctx, host, lens, L, stride)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory()                        # three frames, room for one
        assert e.value.status == rfid.capi.ERR_CAPACITY and "trace 0" in str(e.value)
        # the context stays usable: a larger inventory of the same pass, and a caller's array that is too small loses nothing
        ctx.batch_plan_inventory(8)
        ent, counts = ctx.batch_inventory()
        ref.assert_equal(ent, counts, want, want_counts)
        small = np.zeros(2, dtype=rfid.capi.TAG_ENTRY_DTYPE)
        n = C.c_int64(0)
        rc = ctx._lib.rfid_batch_get_inventory(ctx._h, small.ctypes.data, len(small), C.byref(n), None)
        assert rc == rfid.capi.ERR_CAPACITY and n.value == len(want) and not small.tobytes().strip(b"\0")
        ent2, _ = ctx.batch_inventory_fetch()
        assert ent2.tobytes() == want.tobytes()
        # a new plan drops the workspace
        ctx.batch_plan(2, L)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory()
        assert e.value.status == rfid.capi.ERR_STATE
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory_fetch()
        assert e.value.status == rfid.capi.ERR_STATE
        ctx.batch_plan_inventory(8)
        _pass(ctx, host, lens, L, stride)
        ent, counts = ctx.batch_inventory()
        ref.assert_equal(ent, counts, want, want_counts)
        # the stage calls one by one: results without their statistics are not listed
        ctx.batch_stage("decode", False)
        with pytest.raises(rfid.capi.RfidError) as e:
            ctx.batch_inventory()
        assert e.value.status == rfid.capi.ERR_STATE
        ctx.batch_stage("stats")
        ent, counts = ctx.batch_inventory()
        ref.assert_equal(ent, counts, want, want_counts)
    finally:
        ctx.close()


def test_merge_and_format(batch):
    """rfid.batch.merge_inventory / format_inventory (host side) on the oracle-derived entries, with one frame made common to both traces"""
    from rfid import batch as rb
    want = batch[5].copy()
    want["frame"][3] = want["frame"][0]
    m = rb.merge_inventory(want)
    assert len(m) == 5 and int(m["reads"].sum()) == int(want["reads"].sum())
    frames = [bytes(f) for f in m["frame"]]
    assert len(set(frames)) == 5 and frames == sorted(frames, key=lambda f: tuple(np.frombuffer(f, dtype=np.uint32)))
    g = m[[f == bytes(want["frame"][0]) for f in frames]][0]
    assert g["reads"] == want["reads"][0] + want["reads"][3]
    text = rb.format_inventory(want[:3])
    lines = text.splitlines()
    assert len(lines) == 5
    for e, line in zip(want[:3], lines[1:]):
        pc, epc = rb.frame_fields(e["frame"])
        assert pc == 0x3000 and len(epc) == 24 and epc[-2:] == "%02x" % e["tag_id"]
        db = 20 * np.log10(np.hypot(float(e["best_h_re"]), float(e["best_h_im"])))
        assert line.split() == ["|", epc, "3000", str(e["reads"]), str(e["first_seq"]), str(e["last_seq"]), "%.2f" % db]

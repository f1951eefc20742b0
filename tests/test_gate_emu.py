"""The gate's state machine on the crafted traces of tests/gate_cases.py, on the emulator (tests/test_gpu_gate.py: the same
on the device).  Three layers, each one's reference validated by the one above, ending at the oracle:
 1. tests/gate_ref.py (the gate on votes, sample by sample) == oracle.run_trace on every crafted trace: openings and types;
 2. what the crafted set reaches, counted by that replay over the oracle's filter output (conditions, not measurements);
 3. gate_fsm_step by itself (gate_fsm_selftest_kernel, both forms) == the replay over the same 64 votes from the same state;
 4. every front-end path on every crafted batch == the oracle (parity.compare_trace; the filter output bit for bit)."""
import numpy as np
import pytest

import gate_cases as gc
import gate_ref
import parity
from rfid import _capi as capi


@pytest.fixture(scope="module")
def crafted(oracle_mod, synth_mod):
    return gc.crafted(oracle_mod, synth_mod)


# ---- 1. the replay is the oracle's gate ------------------------------------------------------------------------------
def test_replay_equals_oracle_on_every_crafted_trace(crafted):
    """what licenses the replay as the reference of layer 3 and as the counter of layer 2.  (The oracle lists the windows
    that reached the decoder: the complete ones.)"""
    n = 0
    for batch in crafted:
        for row in batch["rows"]:
            r, o, nd = row["replay"], row["o"], len(row["y"])
            done = [(s, t) for s, t in r.openings if s + gate_ref.WINDOW_LEN[t] <= nd]
            assert [s for s, _ in done] == list(o.open_idx) and [t for _, t in done] == list(o.dumps["type"]), row["name"]
            assert o.n_windows == len(done) and o.state.status == 0, row["name"]     # (no termination inside: compare_trace's premise)
            n += len(done)
    assert n >= 200


# ---- 2. coverage -----------------------------------------------------------------------------------------------------
def test_directed_cases_show_what_they_are_named_for(crafted):
    seen = 0
    for batch in crafted:
        if batch["name"].startswith("directed"):
            for row in batch["rows"]:
                assert gc.directed_event(row["name"], row["head_replay"], row["head_n"]) is not None, row["name"]
                seen += 1
    assert seen == len(gc.DIRECTED_NAMES)


def test_open_lane0_trace_opens_on_the_first_closed_sample_of_a_step(crafted):
    """need == 0: the step of the open_lane0 trace in which the gate opens begins closed with n_samples = T1, and the
    opening is its lane 0"""
    row = next(r for b in crafted for r in b["rows"] if r["name"] == "open_lane0")
    recs = gc.fsm_records_of_trace(capi, row["below"], row["above"])
    want = gc.fsm_expected(capi, recs)
    k = row["head_replay"].openings[0][0] // 64
    assert recs[k]["gate_open"] == 0 and recs[k]["n_samples"] == gate_ref.T1 and recs[k]["num_pulses"] > gate_ref.NUM_PULSES
    assert want[k]["open_lane"] == 0 and want[k]["gate_open"] == 1


def test_coverage_conditions(crafted):
    total = {}
    for batch in crafted:
        for row in batch["rows"]:
            for k, v in row["cover"].items():
                total[k] = total.get(k, 0) + v
        if batch["name"].startswith("random"):
            assert sum(row["o"].n_windows for row in batch["rows"]) >= 20, batch["name"]
    short = {k: total.get(k, 0) for k in gc.COVERED if total.get(k, 0) < gc.MIN_EACH}
    assert not short, short
    assert total.get("tie_state0", 0) >= gc.MIN_TIES and total.get("tie_state1", 0) >= gc.MIN_TIES, total


def test_tie_traces_are_exact(crafted, oracle_mod):
    """the integer traces: the boxcar of the raw samples IS the stated y; avg_ampl returns to exactly 0 behind the long zero
    stretch and stays exactly 400 through the periodic one, whose 300s are then exact ties in both signal states"""
    batch = next(b for b in crafted if b["name"] == "ties")
    for row in batch["rows"]:
        want = np.asarray(gc.tie_y(row["name"]) + gc.IDLE_TAIL, dtype=np.float32).astype(np.complex64)
        assert np.array_equal(row["y"].view(np.uint32), want.view(np.uint32)), row["name"]
        amp, avg = gc.avg_ampl(row["y"])
        ties = [e for e in row["replay"].events if e[0] == "tie"]
        if row["name"] == "ties_leading_zeros":
            assert (avg[:37] == 0).all() and sum(1 for e in ties if e[1] < 37) == 37
        if row["name"] == "ties_zero_stretch_resets_avg":
            assert (avg[250:270] == 0).all() and (amp[250:270] == 0).all() and avg[200] > 0
            assert sum(1 for e in ties if 250 <= e[1] < 270) == 20
        if row["name"] == "ties_periodic":
            assert (avg[249:150 + 900] == 400).all()
            mid = [e for e in ties if 250 <= e[1] < 1050]
            assert all(amp[e[1]] == 300 for e in mid)
            assert sum(1 for e in mid if e[2] == 0) >= 50 and sum(1 for e in mid if e[2] == 1) >= 50
        assert row["o"].n_windows >= 1


# ---- 3. the step function by itself ----------------------------------------------------------------------------------
def test_step_function_on_the_emulator(emu_mod, crafted):
    gc.check_fsm(capi, emu_mod.gate_fsm_selftest, crafted)


# ---- 4. the whole front end ------------------------------------------------------------------------------------------
def _compare(batch, r, want_y=False):
    gc.compare_batch(parity, batch, r["windows"], r["results"], r["scores"], r["stats"], r["y"] if want_y else None)


@pytest.mark.parametrize("name", gc.BATCHES)
def test_fused_front_end(emu_mod, crafted, name):
    """front_end_fused_kernel (its pair body), rows 16-byte aligned and 8-byte aligned only"""
    batch = gc.batch_of(crafted, name)
    for unaligned in (False, True):
        _compare(batch, emu_mod.batch_process(batch["raw"], lens=batch["lens"], gate_chunk=-1, want_y=True, unaligned=unaligned), want_y=True)


@pytest.mark.parametrize("name", gc.BATCHES)
def test_stage_kernels_cut_along_time(emu_mod, crafted, name):
    """matched filter, gate scan (its state carried from chunk to chunk, 777 samples each), decoder, statistics"""
    batch = gc.batch_of(crafted, name)
    _compare(batch, emu_mod.batch_process(batch["raw"], lens=batch["lens"], gate_chunk=777, want_y=True), want_y=True)


_ls = {}


def _long_stream(emu_mod, crafted, name, fsm_lanes):
    batch = gc.batch_of(crafted, name)
    r = emu_mod.ls2_process(batch["raw"], lens=batch["lens"], min_piece=512, target=2048, fsm_lanes=fsm_lanes)
    _ls[(name, fsm_lanes)] = dict(ok=r["ok"], **{k: r["ctl"][k] for k in ("fail", "n_heads", "n_units", "fsm_rounds", "fsm_reruns")})
    print("long-stream pass", name, "per lane" if fsm_lanes else "per wave", _ls[(name, fsm_lanes)])
    _compare(batch, r)
    return _ls[(name, fsm_lanes)]


@pytest.mark.parametrize("fsm_lanes", [False, True], ids=["fsm-per-wave", "fsm-per-lane"])
@pytest.mark.parametrize("name", gc.BATCHES)
def test_long_stream_front_end(emu_mod, crafted, name, fsm_lanes):
    """The results whatever the pass reports (a pass that gives up runs the sequential scan).  A cut needs 1615 samples of
    carrier in front of it, which the commands' own carrier never has: the random envelopes (two in three), the directed traces
    (but those about the trace's end) and the tie traces hold IDLE_CARRIER for it, and every noise-free batch must complete
    without the sequential scan, with more units than traces -- else the long-stream state machine (its run-skipping, its
    per-lane twin, the idle cut's constant) was not the code under comparison.  (Threshold chatter may give up: no assertion.)"""
    rep = _long_stream(emu_mod, crafted, name, fsm_lanes)
    if gc.noise_free(name):
        assert rep["ok"] == 1 and rep["fail"] == 0 and rep["n_units"] > len(gc.batch_of(crafted, name)["rows"]), (name, rep)


@pytest.mark.parametrize("fsm_lanes", [False, True], ids=["fsm-per-wave", "fsm-per-lane"])
def test_long_stream_withdraws_cuts_that_are_not_idle(emu_mod, crafted, fsm_lanes):
    """carrier_pulses_pending_long, carrier_epc_pending_long: a cut's constant state is wrong there (pulses pending, an EPC
    due), the cut is withdrawn and the unit run again"""
    name = gc.BATCHES[-3]
    assert "carrier_epc_pending_long" in [r["name"] for r in gc.batch_of(crafted, name)["rows"]]
    rep = _ls.get((name, fsm_lanes)) or _long_stream(emu_mod, crafted, name, fsm_lanes)
    assert rep["ok"] == 1 and rep["fsm_reruns"] >= 2, rep


@pytest.mark.parametrize("name", gc.BATCHES)
def test_per_call_gate(emu_mod, oracle_mod, crafted, name):
    """gate_scan_kernel in per-call mode: the only path on which gate_fsm_step's stop is reached.  The tie traces' y is the
    stated one (test_tie_traces_are_exact)."""
    batch = gc.batch_of(crafted, name)
    n_closed = 0
    for row in batch["rows"]:
        gs = emu_mod.GateStream()
        try:
            n = gc.per_call_gate(oracle_mod, row["y"], lambda blk, seek: gs.work(blk, seek_type=seek))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (row["name"], e)) from e
        assert n == len(row["replay"].closings), row["name"]
        n_closed += n
    assert n_closed >= 3


# ---- the device tests of tests/test_gpu_gate.py on the stand-in runtime ("device" pointers are host pointers) ---------------
# csrc/rfid_capi.hip unmodified, its launches on the wave emulator: the C call of the step function's test entry, and the bodies
# of the device tests on the two batches the long-stream front end can cut.
@pytest.fixture(scope="module")
def capi_ctx():
    import emu_lib
    with emu_lib.emulated_library():
        import rfid
        c = rfid.Context(device=0)
        try:
            yield c
        finally:
            c.close()


def _host_upload(host):
    a = np.ascontiguousarray(host).copy()
    return a.ctypes.data, a


def _host_write(dst, arr):
    import ctypes as C
    arr = np.ascontiguousarray(arr)
    C.memmove(dst, arr.ctypes.data, arr.nbytes)


def test_step_function_through_the_c_call(capi_ctx, crafted):
    gc.check_fsm(capi, capi_ctx.selftest_gate_fsm, crafted)


@pytest.mark.parametrize("name", ["ties", gc.BATCHES[-3]])
def test_device_bodies_on_the_stand_in_runtime(capi_ctx, oracle_mod, crafted, name):
    import emu_lib
    import test_gpu_gate as g
    g.test_fused_front_end(capi_ctx, crafted, name, upload=_host_upload)
    g.test_stage_kernels(capi_ctx, crafted, name, upload=_host_upload, write=_host_write)
    for form in g.FORMS:
        g.test_long_stream_front_end(capi_ctx, crafted, name, form, upload=_host_upload)
        g.test_long_stream_withdraws_cuts_that_are_not_idle(capi_ctx, crafted, form, upload=_host_upload)
    with emu_lib.emulated_library():
        g.test_per_call_gate(oracle_mod, crafted, name)

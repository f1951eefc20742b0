"""The gate's state machine on the crafted traces of tests/gate_cases.py, on the device (tests/test_gate_emu.py: the same on
the emulator, with the validation of the reference and the coverage conditions).  gate_fsm_step by itself in both forms the
kernels call it in, against tests/gate_ref.py's replay; then every front-end path on every crafted batch against the oracle:
the fused front end (pair body and one-step body, even and odd row stride), the stage kernels (one launch each, and cut
along time), the gate stage on a filter output written by the test (the tie traces), the long-stream front end with its
state machine per wave and per lane, and the per-call gate in odd chunk sizes."""
import numpy as np
import pytest

import gate_cases as gc
import parity
from rfid import _capi as capi
from test_gpu_decoder_windows import gpu_upload, hip_write

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rfid
    c = rfid.Context(device=0)
    c.batch_set_long_stream(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def crafted(oracle_mod, synth_mod):
    return gc.crafted(oracle_mod, synth_mod)


def test_step_function_on_the_device(ctx, crafted):
    """gate_fsm_selftest_kernel: wave-uniform arguments (the consumer wave, ls2_fsm_kernel) and one record per lane
    (ls2_fsm_lanes_kernel), every output word of both against the replay over the same 64 votes from the same state"""
    gc.check_fsm(capi, ctx.selftest_gate_fsm, crafted)


def _upload(batch, upload, odd_stride=False):
    raw, lens = batch["raw"], batch["lens"]
    B, L = raw.shape
    stride = (L | 1) if odd_stride else (L + 1) & ~1     # odd stride: rows 8-byte aligned only, the filter wave's float2 loads
    host = np.zeros((B, stride), dtype=np.complex64)
    host[:, :L] = raw
    d_raw, keep_raw = upload(host.view(np.float32))
    d_lens, keep_lens = upload(np.asarray(lens, dtype=np.int64))
    return d_raw, d_lens, B, L, stride, (keep_raw, keep_lens)


def _fetch(ctx, batch, want_y=True):
    w, r, s = ctx.batch_windows(want_scores=True)
    st = ctx.batch_stats().copy()
    y = [ctx.batch_mf_output(b)[: int(batch["lens"][b]) // 5].copy() for b in range(len(batch["rows"]))] if want_y else None
    return w, r, s, st, y


def _process(ctx, batch, upload, odd_stride=False, long_stream=0, **knobs):
    d_raw, d_lens, B, L, stride, keep = _upload(batch, upload, odd_stride)
    ctx.batch_plan(B, L)
    ctx.batch_set_long_stream(long_stream)
    for k, v in knobs.items():
        ctx.set_knob(k, v[0])
    try:
        ctx.batch_process_ptr(d_raw, stride, L, d_lens, want_scores=True)
        ctx.batch_sync()
    finally:
        for k, v in knobs.items():
            ctx.set_knob(k, v[1])
        ctx.batch_set_long_stream(0)
    return _fetch(ctx, batch)


@pytest.mark.parametrize("name", gc.BATCHES)
def test_fused_front_end(ctx, crafted, name, upload=gpu_upload):
    """the pair body and the one-step body byte-equal to each other, with even and odd row stride, and equal to the oracle"""
    batch = gc.batch_of(crafted, name)
    for odd in (False, True):
        w0, r0, s0, st0, y0 = _process(ctx, batch, upload, odd, front_single_step=(0, 0))
        assert ctx.batch_timing()["fused_front"] == 1
        w1, r1, s1, st1, y1 = _process(ctx, batch, upload, odd, front_single_step=(1, 0))
        assert ctx.batch_timing()["fused_front"] == 1
        s0["pad_"] = s1["pad_"] = 0          # (padding: not an output, and not written)
        assert w0.tobytes() == w1.tobytes() and r0.tobytes() == r1.tobytes() and s0.tobytes() == s1.tobytes()
        assert st0.tobytes() == st1.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(y0, y1))
        gc.compare_batch(parity, batch, w0, r0, s0, st0, y0)


@pytest.mark.parametrize("name", gc.BATCHES)
def test_stage_kernels(ctx, crafted, name, upload=gpu_upload, write=hip_write):
    """rfid_batch_mf / _gate / _decode / _stats one launch each; then the pass cut along time in four (the gate's state
    carried from chunk to chunk); for the tie traces also the gate stage on the stated y, written over the filter's output"""
    batch = gc.batch_of(crafted, name)
    d_raw, d_lens, B, L, stride, keep = _upload(batch, upload)
    ctx.batch_plan(B, L)
    ctx.batch_set_long_stream(0)

    def stages(mf):
        if mf:
            ctx.batch_stage("mf", d_raw, stride, L, d_lens)
        ctx.batch_stage("gate")
        ctx.batch_stage("decode", True)
        ctx.batch_stage("stats")
        ctx.batch_sync()
        assert ctx.batch_timing()["fused_front"] == 0
        gc.compare_batch(parity, batch, *_fetch(ctx, batch))
    stages(True)
    if name == "ties":
        ptrs = ctx.batch_device_ptrs()
        for b, row in enumerate(batch["rows"]):
            want = np.asarray(gc.tie_y(row["name"]) + gc.IDLE_TAIL, dtype=np.float32).astype(np.complex64)
            write(ptrs["mf_out"] + 8 * b * ptrs["mf_stride"], want)
        stages(False)
    # (the library cuts along time only where every chunk holds four of the filter's 512-sample tiles)
    nch = min(4, ((L // 5 + 511) // 512) // 4)
    assert nch >= 2
    w, r, s, st, y = _process(ctx, batch, upload, front_chunks=(nch, 1))
    assert ctx.batch_timing()["front_chunks"] == nch and ctx.batch_timing()["fused_front"] == 0
    gc.compare_batch(parity, batch, w, r, s, st, y)


_reports = {}      # (context, batch, form) -> the reports of its passes, in order
FORMS = {"fsm-per-wave": 1 << 30, "fsm-per-lane": 0}      # the knob fsm_lanes_min: from how many heads on a lane takes a unit


def _long_stream(ctx, crafted, name, form, upload):
    """-> the reports of the passes run.  A small pass enqueues ONE re-run round of the state machine (the library has no
    knob for that count); where cuts are withdrawn one behind the other that does not settle it, the pass says gave_up 3, the
    sequential scan takes over and the context enqueues the full count from then on.  Such a pass is run once more; both
    passes' results are compared with the oracle and both reports are kept."""
    batch = gc.batch_of(crafted, name)
    reps = _reports[(id(ctx), name, form)] = []
    for attempt in range(2):
        w, r, s, st, y = _process(ctx, batch, upload, long_stream=2, fsm_lanes_min=(FORMS[form], -1))
        reps.append(ctx.batch_ls_report())
        print("long-stream report", name, form, reps[-1])
        gc.compare_batch(parity, batch, w, r, s, st, y)
        if reps[-1]["gave_up"] != 3:
            break
    return reps


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", gc.BATCHES)
def test_long_stream_front_end(ctx, crafted, name, form, upload=gpu_upload):
    """The results whatever the pass reports (a pass that gives up runs the sequential scan).  Every noise-free batch holds
    traces with carrier to cut in (tests/gate_cases.py: IDLE_CARRIER) and must complete without the sequential scan, at the
    library's own piece size, with more units than traces: else the long-stream state machine was not the code under
    comparison.  (Threshold chatter may give up: no assertion.)"""
    reps = _long_stream(ctx, crafted, name, form, upload)
    if gc.noise_free(name):
        rep = reps[-1]
        assert rep["verified"] == 1 and rep["gave_up"] == 0, (name, reps)
        assert rep["units"] > len(gc.batch_of(crafted, name)["rows"]), (name, reps)
        assert all(q["gave_up"] == 3 for q in reps[:-1]), (name, reps)


@pytest.mark.parametrize("form", list(FORMS))
def test_long_stream_withdraws_cuts_that_are_not_idle(ctx, crafted, form, upload=gpu_upload):
    """carrier_pulses_pending_long, carrier_epc_pending_long: what an idle cut assumes is not the case"""
    name = gc.BATCHES[-3]
    assert "carrier_epc_pending_long" in [r["name"] for r in gc.batch_of(crafted, name)["rows"]]
    reps = _reports.get((id(ctx), name, form)) or _long_stream(ctx, crafted, name, form, upload)
    assert reps[-1]["verified"] == 1 and reps[-1]["cuts_dropped"] >= 2, reps


@pytest.mark.parametrize("name", gc.BATCHES)
def test_per_call_gate(oracle_mod, crafted, name):
    """rfid_gate_work on the oracle's filter output (the tie traces': the stated y) in odd chunk sizes, decoder and reader
    re-arming the gate behind every window: consumed, the samples written and the open flag, call by call, against
    orc_gate_work"""
    import rfid
    batch = gc.batch_of(crafted, name)
    c = rfid.Context(device=0)
    try:
        n_closed = 0
        for row in batch["rows"]:
            c.reset()
            acc = []

            def reader(n_bits):
                for _ in range(8):
                    if c.state().gen2_logic_status == capi.IDLE:
                        break
                    c.reader_work(n_bits)
                    n_bits = 0

            def work(blk, seek):
                if seek >= 0 and acc:      # a window closed in the call before: the decoder takes it, the reader re-arms the gate
                    win = np.concatenate(acc)
                    acc.clear()
                    cons, bits, _, _ = c.decoder_work(win)
                    assert cons == len(win)
                    reader(len(bits))
                    assert c.state().gate_status == (capi.GATE_SEEK_EPC if seek else capi.GATE_SEEK_RN16)
                cons, out = c.gate_work(blk)
                if len(out):
                    acc.append(out)
                return cons, out, int(c.state().gate_status == capi.GATE_OPEN)
            reader(0)
            try:
                n = gc.per_call_gate(oracle_mod, row["y"], work)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (row["name"], e)) from e
            assert n == len(row["replay"].closings), row["name"]
            n_closed += n
        assert n_closed >= 3
    finally:
        c.close()

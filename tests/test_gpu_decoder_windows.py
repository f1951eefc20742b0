"""The tag decoder on the device, on the windows where the reference's comparison operators decide (tests/decoder_windows.py:
tied sync maxima, tied energies, half-bit differences of exactly 0, valid frames at every sync offset) -- the per-call path
(decode_windows_kernel behind rfid_decoder_work), the batched decoder the library launches (decode_all_kernel: crafted
windows written over the matched filter's output inside the windows the gate found) and the whole chain on a noise-free
trace, whose empty and collided slots are constant windows: 15-way sync ties and 20-way energy ties.  Bit for bit against the
oracle.  tests/test_capi_decoder_windows.py runs the same functions on the stand-in runtime."""
import ctypes as C

import numpy as np
import pytest

import decoder_windows as dw
import parity

pytestmark = pytest.mark.gpu

_hip = None


def hip_write(dst: int, arr: np.ndarray) -> None:
    """hipMemcpy host -> device through the HIP runtime this process has already loaded"""
    global _hip
    if _hip is None:
        with open("/proc/self/maps") as f:
            paths = [ln.split()[-1] for ln in f if "libamdhip64" in ln]
        assert paths, "the HIP runtime is not loaded"
        _hip = C.CDLL(paths[0])
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    arr = np.ascontiguousarray(arr)
    rc = _hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(arr.ctypes.data), arr.nbytes, 1)      # hipMemcpyHostToDevice
    assert rc == 0, ("hipMemcpy", rc)


def gpu_upload(host: np.ndarray):
    """-> (pointer, what keeps the memory alive)"""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0")
    torch.cuda.synchronize()
    return dev.data_ptr(), dev


def test_decoder_work_on_every_crafted_window(oracle_mod):
    """the per-call path: rfid_decoder_work, one decode_windows_kernel launch per window"""
    import rfid
    s = dw.sets(oracle_mod)
    ctx = rfid.Context(device=0)
    try:
        n = len(s.wins[dw.EPC])
        assert dw.drive_decoder_work(ctx, oracle_mod, s, n) == 2 * n == 550
        assert ctx.state().n_epc_correct == 15            # the valid frames, and nothing else
    finally:
        ctx.close()


# traces cut behind their k-th window (24: whole): with the whole batches of 1..4 traces the EPC list takes every length
# mod 3 (the pack of decode_epc3_body) and the RN16 list every length mod 4 (decode_rn16x4_body)
CUTS = [(24, 24, 24, 23), (24, 24, 24, 21), (24, 24, 22, 19), (24, 24, 21, 21)]


def test_batched_decoder_on_crafted_windows(oracle_mod, synth_mod, upload=gpu_upload, write=hip_write, variants=None):
    """decode_all_kernel as rfid_batch_decode launches it, on windows the gate found in four copies of the clean trace: the
    matched filter's output inside every window is overwritten on the device with float32(dc_est + w), w a crafted window of
    the window's type -- which the decoder's own subtraction turns back into w bit for bit (asserted in numpy first: w is made
    of small integers and dc_est + w stays below the next binade) -- and every result and score equals the oracle's for w."""
    import rfid
    s = dw.sets(oracle_mod)
    t, o = dw.clean_trace(oracle_mod, synth_mod)
    B, L = 4, len(t)
    stride = (L + 1) & ~1
    host = np.zeros((B, stride), dtype=np.complex64)
    host[:, :L] = t
    d_raw, keep_raw = upload(host.view(np.float32))
    full = variants is None
    if full:
        variants = [(n, None) for n in (1, 2, 3, 4)] + [(4, c) for c in CUTS]
    used = {dw.RN16: set(), dw.EPC: set()}
    mods = {dw.RN16: set(), dw.EPC: set()}
    first = {dw.RN16: 0, dw.EPC: 0}
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_plan(B, L)
        for n_streams, cut in variants:
            ctx.batch_set_streams(n_streams)
            d_lens, keep_lens = 0, None
            if cut is not None:   # the trace ends ten samples into its k-th window, which is then never handed out
                lens = np.array([L if k >= o.n_windows else 5 * (int(o.open_idx[k]) + 10) for k in cut], dtype=np.int64)
                d_lens, keep_lens = upload(lens)
            ctx.batch_stage("mf", d_raw, stride, L, d_lens)
            ctx.batch_stage("gate")
            ctx.batch_sync()
            w, _, _ = ctx.batch_windows()
            for b in range(n_streams):
                k = o.n_windows if cut is None else min(cut[b], o.n_windows)
                assert np.array_equal(w["start"][w["stream"] == b], o.open_idx[:k]), (n_streams, cut, b)
            ptrs = ctx.batch_device_ptrs()
            want = []
            for rec in w:
                type_ = int(rec["type"])
                i = first[type_] % len(s.wins[type_])
                first[type_] += 1
                used[type_].add(i)
                dc = np.complex64(complex(rec["dc_re"], rec["dc_im"]))
                y = dw.shifted(s.wins[type_][i], dc)              # (asserts that (dc + w) - dc == w for every sample)
                assert len(y) == dw.WLEN[type_]
                write(ptrs["mf_out"] + 8 * (int(rec["stream"]) * ptrs["mf_stride"] + int(rec["start"])), y)
                want.append((s.dumps[type_][i], s.names[type_][i]))
            for type_ in mods:
                mods[type_].add(int((w["type"] == type_).sum()) % (3 if type_ == dw.EPC else 4))
            ctx.batch_stage("decode", True)
            ctx.batch_sync()
            w2, r, sc = ctx.batch_windows(want_scores=True)
            assert w2.tobytes() == w.tobytes()
            for k, (dump, name) in enumerate(want):
                dw.compare_window(r[k], sc[k], dump, (name, "streams %d" % n_streams, "cut", cut, "window %d" % k))
    finally:
        ctx.close()
    if full:
        assert mods[dw.EPC] == {0, 1, 2} and mods[dw.RN16] == {0, 1, 2, 3}, mods
        for type_ in used:
            assert len(used[type_]) == len(s.wins[type_]), "not every crafted window was decoded"


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_clean_trace_through_the_batch_pass(oracle_mod, synth_mod, mode, upload=gpu_upload):
    import rfid
    t, o = dw.clean_trace(oracle_mod, synth_mod)
    L = len(t)
    stride = (L + 1) & ~1
    host = np.zeros((2, stride), dtype=np.complex64)
    host[:, :L] = t
    d_raw, keep = upload(host.view(np.float32))
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.batch_set_long_stream(mode)
        ctx.batch_plan(2, L)
        ctx.batch_process_ptr(d_raw, stride, L, 0, want_scores=True)
        ctx.batch_sync()
        w, r, sc = ctx.batch_windows(want_scores=True)
        st = ctx.batch_stats()
        for b, (wb, rb, sb) in enumerate(parity.split_by_stream(w, r, sc, 2)):
            parity.compare_trace(wb, rb, sb, st[b], o)
    finally:
        ctx.close()


def test_clean_trace_through_the_whole_chain_stream(oracle_mod, synth_mod):
    """rfid_stream_work in chunks that cut windows apart"""
    import rfid
    t, o = dw.clean_trace(oracle_mod, synth_mod)
    ctx = rfid.Context(device=0, fixed_q=2)
    try:
        ctx.stream_begin(60_000)
        ws, rs = [], []
        for pos in range(0, len(t), 52_345):
            w, r = ctx.stream_work(t[pos:pos + 52_345])
            ws.append(w); rs.append(r)
        w, r = ctx.stream_work(flush=True)
        ws.append(w); rs.append(r)
        w, r = np.concatenate(ws), np.concatenate(rs)
        parity.compare_trace(w, r, None, None, o)
        assert ctx.stats() == o.stats() and ctx.print_results() == o.print_results()
        ctx.stream_end()
    finally:
        ctx.close()


def test_clean_trace_through_the_per_block_flowgraph(oracle_mod, synth_mod):
    """matched filter, gate, tag_decoder and reader called block by block, scores included"""
    import rfid
    t, o = dw.clean_trace(oracle_mod, synth_mod)
    tb = rfid.reader_top_block(samples=t, device=0, chunk=2777, fixed_q=2)
    try:
        tb.run()
        assert len(tb.decoded) == o.n_windows
        for k, ((res, sc), dump) in enumerate(zip(tb.decoded, o.dumps)):
            dw.compare_window(res, sc, dump, "window %d" % k)
        assert tb.ctx.stats() == o.stats() and tb.ctx.print_results() == o.print_results()
    finally:
        tb.ctx.close()

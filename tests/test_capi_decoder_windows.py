"""rfid_decoder_work on the stand-in runtime (tests/fake_hip: csrc/rfid_capi.hip unmodified, its launches on the wave
emulator), driven with the crafted windows of tests/decoder_windows.py -- tied sync maxima, tied energies, half-bit
differences of exactly 0, valid frames at every sync offset: the CPU check of the C-ABI path into decode_windows_kernel.
RN16 and EPC windows alternate as the reader state demands; the oracle's decoder and reader are stepped alongside and
results, scores, port-0 bits and the reader state compared after every call.  tests/test_gpu_decoder_windows.py runs the
same driver against the real library."""
import ctypes as C

import pytest

import decoder_windows as dw
import emu_lib


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    with emu_lib.emulated_library() as lib:
        yield lib


def test_decoder_work_on_every_crafted_window(oracle_mod):
    import rfid
    s = dw.sets(oracle_mod)
    ctx = rfid.Context(device=0)
    try:
        n = len(s.wins[dw.EPC])
        assert dw.drive_decoder_work(ctx, oracle_mod, s, n) == 2 * n == 550
        assert ctx.state().n_epc_correct == 15            # the valid frames, and nothing else
    finally:
        ctx.close()


# ---- the device tests of tests/test_gpu_decoder_windows.py on the stand-in runtime ("device" pointers are host pointers) ----

def _host_upload(host):
    import numpy as np
    a = np.ascontiguousarray(host).copy()
    return a.ctypes.data, a


def _host_write(dst, arr):
    import numpy as np
    arr = np.ascontiguousarray(arr)
    C.memmove(dst, arr.ctypes.data, arr.nbytes)


def test_batched_decoder_on_crafted_windows(oracle_mod, synth_mod):
    """rfid_batch_mf / rfid_batch_gate / rfid_batch_decode with crafted windows written into the windows the gate found: one
    whole trace, and two traces of which the second is cut (the device test runs every batch size and every pack remainder)"""
    import test_gpu_decoder_windows as g
    g.test_batched_decoder_on_crafted_windows(oracle_mod, synth_mod, upload=_host_upload, write=_host_write,
                                              variants=[(1, None), (2, (24, 21))])


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_clean_trace_through_the_batch_pass(oracle_mod, synth_mod, mode):
    import test_gpu_decoder_windows as g
    g.test_clean_trace_through_the_batch_pass(oracle_mod, synth_mod, mode, upload=_host_upload)


def test_clean_trace_through_the_whole_chain_stream(oracle_mod, synth_mod):
    import test_gpu_decoder_windows as g
    g.test_clean_trace_through_the_whole_chain_stream(oracle_mod, synth_mod)


def test_clean_trace_through_the_per_block_flowgraph(oracle_mod, synth_mod):
    import test_gpu_decoder_windows as g
    g.test_clean_trace_through_the_per_block_flowgraph(oracle_mod, synth_mod)

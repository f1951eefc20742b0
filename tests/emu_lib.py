"""What the modules that run csrc/rfid_capi.hip on the CPU share: tests/fake_hip's library (the kernels on the wave emulator) in
place of librfid_mi355x.so, and the helpers of the four stage modules (test_inventory_emu, test_tracks_emu, test_quality_emu,
test_repair_emu) that are the same in each."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "fake_hip"))


@contextlib.contextmanager
def emulated_library():
    """librfid_capi_emu.so in place of librfid_mi355x.so -- in this process, and put back afterwards"""
    import build_capi_emu as fake_build
    import rfid
    from rfid import _capi
    lib = C.CDLL(fake_build.build())
    for name, (res, args) in _capi.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    saved = _capi._lib
    _capi._lib = lib
    try:
        yield lib
    finally:
        _capi._lib = saved


def pack(ts, shorten=777):
    """traces -> (host array [n][stride], lengths, longest length, stride), the first trace cut short"""
    L = max(map(len, ts))
    stride = (L + 1) & ~1
    host = np.zeros((len(ts), stride), dtype=np.complex64)
    lens = np.array([len(t) for t in ts], dtype=np.int64)
    lens[0] -= shorten            # (ragged also where the longest trace is concerned)
    for i, t in enumerate(ts):
        host[i, : len(t)] = t
    return host, lens, L, stride


def oracle_runs(oracle_mod, host, lens, **cfg):
    return [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2, **cfg)) for b in range(len(lens))]


def run_pass(ctx, host, lens, L, stride):
    ctx.batch_process_ptr(host.ctypes.data, stride, L, lens.ctypes.data)

"""What the modules that run csrc/rfid_capi.hip on the CPU share: tests/fake_hip's library (the kernels on the wave emulator) in
place of librfid_mi355x.so, and the helpers of the stage modules (test_<stage>_emu) that are the same in each.  Traces are laid
out by tests/stage_backend.py, whose Emulated is how a pass reaches this library."""
import contextlib
import ctypes as C
import os
import sys

from stage_backend import Emulated

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


def oracle_runs(oracle_mod, host, lens, **cfg):
    return [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=2, **cfg)) for b in range(len(lens))]


def run_pass(ctx, host, lens, L, stride):
    """a pass over arrays the caller holds, for the narratives that only this side runs"""
    backend = Emulated()
    backend.run_pass(ctx, backend.put(host, lens), L, stride)

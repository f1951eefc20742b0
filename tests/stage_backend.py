"""The seam between a stage's cases and the library they run on.  A case lays its traces out once (lay_out), hands them to its
module's `backend` (put: the handle keeps alive what a pass reads, so the case holds it until the pass's results are fetched) and
runs every pass through it (run_pass): Emulated passes host pointers to csrc/rfid_capi.hip on tests/fake_hip's stand-in runtime,
Device passes device tensors to librfid_mi355x.so on the MI355X.  A case that is meant for both sides is written once, in
tests/<stage>_suite.py, against this interface; the module that imports it picks the side with its `backend` fixture."""
import numpy as np


def lay_out(traces, odd_stride=False, shorten=0):
    """traces -> (host [n][stride] complex64, lens int64, L = the longest length, stride).  The row stride is the next even number,
    or an odd one (rows 8-byte aligned only) when asked; `shorten` cuts the first trace's length, so that a batch is ragged also
    where its longest trace is concerned"""
    L = max(map(len, traces))
    stride = ((L + 2) | 1) if odd_stride else ((L + 1) & ~1)
    host = np.zeros((len(traces), stride), dtype=np.complex64)
    lens = np.array([len(t) for t in traces], dtype=np.int64)
    lens[0] -= shorten
    for i, t in enumerate(traces):
        host[i, : len(t)] = t
    return host, lens, L, stride


def carrier_between(host, lens, L):
    """traces 0 and 1 of a laid-out batch with a pure-carrier trace of half the length between them (no window, no row, no read)
    -> (host [3][stride], lens)"""
    three = np.zeros((3, host.shape[1]), dtype=np.complex64)
    three[0], three[2] = host[0], host[1]
    three[1, : L // 2] = 0.8 + 0.1j
    return three, np.array([lens[0], L // 2, lens[1]], dtype=np.int64)


def oracle_pass(oracle_mod, host, lens, fixed_q, **cfg):
    """-> (oracle Results, the oracle's matched-filter outputs) of the traces of a laid-out batch; cfg goes to oracle.config as it is"""
    refs = [oracle_mod.run_trace(host[b, : lens[b]], oracle_mod.config(fixed_q=fixed_q, **cfg)) for b in range(len(lens))]
    ys = [oracle_mod.fir(host[b, : lens[b]]) for b in range(len(lens))]
    return refs, ys


class Emulated:
    """host pointers: the stand-in runtime reads the arrays themselves"""
    name = "emulator"
    reps = 2          # how often a "same bytes every time" case repeats its pass

    def put(self, host, lens):
        assert host.flags.c_contiguous and host.dtype == np.complex64 and lens.flags.c_contiguous and lens.dtype == np.int64
        return host, lens

    def run_pass(self, ctx, handle, L, stride):
        ctx.batch_process_ptr(handle[0].ctypes.data, stride, L, handle[1].ctypes.data)


class Device:
    """device tensors; torch is imported only where a pass is prepared, so that collecting a device module needs no GPU"""
    name = "device"
    reps = 3

    def put(self, host, lens):
        import torch
        dev = torch.from_numpy(np.ascontiguousarray(host).view(np.float32)).to("cuda:0")
        dlens = torch.from_numpy(np.ascontiguousarray(lens)).to("cuda:0")
        torch.cuda.synchronize()
        return dev, dlens

    def run_pass(self, ctx, handle, L, stride):
        ctx.batch_process_ptr(handle[0].data_ptr(), stride, L, handle[1].data_ptr())

"""front_end_fused_kernel's pair body (gate_pairs_body: every role works on two steps per loop trip) on the emulator,
bit for bit against the oracle: matched-filter output, window table, decisions, scores and statistics -- under every
workgroup schedule the emulator offers (its deadlock detector is the check on the ring protocol)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import front_pairs_cases as cases
import parity

SCHEDULES = ["seq", "in-order", "reversed", "random", "late"]


@contextlib.contextmanager
def _schedule(emu_mod, name):
    L = emu_mod.lib()
    L.emu_schedule(emu_mod.SCHEDULES[name], C.c_ulonglong(7))
    try:
        yield
    finally:
        L.emu_schedule(0, C.c_ulonglong(0))


_oracle_cache = {}


def _oracle(oracle_mod, key, raw, lens):
    """(run_trace, fir) of every row, computed once per batch and shared by the schedules"""
    if key not in _oracle_cache:
        _oracle_cache[key] = [(oracle_mod.run_trace(raw[b][: lens[b]]), oracle_mod.fir(raw[b][: lens[b]])) for b in range(len(raw))]
    return _oracle_cache[key]


def _check(emu_mod, oracle_mod, key, raw, lens, schedule, unaligned=False):
    ref = _oracle(oracle_mod, key, raw, lens)
    with _schedule(emu_mod, schedule):
        r = emu_mod.batch_process(raw, lens=lens, gate_chunk=-1, want_y=True, unaligned=unaligned)
    B = len(raw)
    for b, (wb, rb, sb) in enumerate(parity.split_by_stream(r["windows"], r["results"], r["scores"], B)):
        o, yo = ref[b]
        n = int(lens[b]) // 5
        assert np.array_equal(r["y"][b][:n].view(np.uint32), yo[:n].view(np.uint32)), (b, "y")
        parity.compare_trace(wb, rb, sb, r["stats"][b], o)
    return ref


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_step_counts_around_pairs_and_ring_wrap(emu_mod, oracle_mod, synth_mod, schedule):
    raw, lens = cases.step_count_batch(synth_mod)
    _check(emu_mod, oracle_mod, "steps", raw, lens, schedule)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_windows_against_pair_boundaries(emu_mod, oracle_mod, synth_mod, schedule):
    raw, lens = cases.shifted_batch(synth_mod)
    ref = _check(emu_mod, oracle_mod, "shift", raw, lens, schedule)
    # the shifts do move the openings through a pair: both halves and both kinds of boundary occur
    starts = np.concatenate([o.open_idx for o, _ in ref]) % 128
    assert (starts < 64).any() and (starts >= 64).any()
    assert all(o.n_windows == 4 for o, _ in ref)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_both_paths_of_the_sum(emu_mod, oracle_mod, synth_mod, schedule):
    raw, lens = cases.sum_paths_batch(synth_mod)
    ref = _check(emu_mod, oracle_mod, "sum", raw, lens, schedule)
    # the chain fallback was taken inside pairs of row 0 (and the scan in most others): from the oracle's avg_ampl trajectory
    left = cases.avg_ampl_pairs_leaving_binade(ref[0][1])
    npairs = (int(lens[0]) // 5 // 64) // 2
    assert 1 <= len(left) < npairs // 2, (len(left), npairs)
    assert all(o.n_windows == 4 for o, _ in ref)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("B,unaligned", [(1, False), (4, True), (5, False), (5, True)])
def test_workgroup_shapes(emu_mod, oracle_mod, synth_mod, schedule, B, unaligned):
    raw, lens = cases.ragged_batch(synth_mod, B)
    _check(emu_mod, oracle_mod, ("ragged", B), raw, lens, schedule, unaligned=unaligned)
    if B > 1:
        assert lens[B - 2] == 0


@pytest.fixture(scope="module")
def pairs_lib(tmp_path_factory):
    """the emulator driver with tests/wave_emu/emu_front_pairs.cpp's extra entry points, built outside the tree.  The flags
    are those of tests/wave_emu/build.py (whose build() only knows its own two outputs) but for -O1: half the compile time,
    and with -ffp-contract=off the arithmetic is the same at every level."""
    import os
    import subprocess
    import build as emu_build
    out = str(tmp_path_factory.mktemp("emu_pairs") / "librfid_wave_emu_pairs.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-fno-strict-aliasing",
                           "-DLS2_FIN_WPB=16", "-I", emu_build.HERE, "-I", os.path.join(emu_build.ROOT, "include"),
                           "-iquote", emu_build.HERE, "-o", out, os.path.join(emu_build.HERE, "emu_front_pairs.cpp"),
                           "-I", emu_build.CSRC])
    return C.CDLL(out)


def test_pair_scan_is_exact(pairs_lib):
    """chain_add_scan_pair (avg_ampl over two steps as one integer scan from the one carry, the ties' parity chain running on
    across the boundary) equals the in-order chain bit for bit whenever it says so -- random addends of the receive path's
    magnitudes, exact rounding ties in the first step, the second, both and at the boundary lanes, negative carries, sums
    that cross a power of two in either step -- and does apply in the common case, with ties in either step."""
    rng = np.random.default_rng(23)
    cases_ = []
    for _ in range(400):
        carry = float(rng.choice([23.456789, -19.12345, 31.99999, 16.000002, 0.0, 1e-30, -15.99999, 3.0e5, 25.0, 8.5, -0.75]))
        scale = float(rng.choice([1e-4, 1e-3, 1e-2, 0.3, 1e-8, 1e3]))
        x = (rng.standard_normal(128) * scale).astype(np.float32)
        kind = int(rng.integers(0, 6))
        tie = lambda n: np.ldexp(rng.integers(-7, 8, n).astype(np.float32) + 0.5, -19)   # half an ulp at 16..32
        if kind == 1:
            x[:64:3] = tie(len(x[:64:3]))
        if kind == 2:
            x[64::3] = tie(len(x[64::3]))
        if kind == 3:
            x[::5] = tie(len(x[::5]))
        if kind == 4:
            x[[0, 63, 64, 127]] = tie(4)
        if kind == 5:
            x[int(rng.integers(0, 128))] = 0.0
            x[69] = -0.0
        cases_.append((x, carry, kind))
    cases_.append((np.zeros(128, np.float32), 25.0, 0))
    cases_.append((np.full(128, 2.0 ** -19, np.float32), 31.9999, 0))       # walks up to and across 32 in the second step
    cases_.append((np.full(128, 2.0 ** -18, np.float32), 31.9999, 0))       # ... in the first
    cases_.append((np.full(128, -2.0 ** -20, np.float32), 16.00001, 0))     # walks down across 16: ties and a binade edge
    n_ok = {k: 0 for k in range(6)}
    for x, carry, kind in cases_:
        x0, x1 = np.ascontiguousarray(x[:64]), np.ascontiguousarray(x[64:])
        o0, o1, r0, r1 = (np.zeros(64, np.float32) for _ in range(4))
        ok = C.c_int(0)
        rc = pairs_lib.emu_chain_scan_pair(C.c_void_p(x0.ctypes.data), C.c_void_p(x1.ctypes.data), C.c_float(carry),
                                           *(C.c_void_p(a.ctypes.data) for a in (o0, o1, r0, r1)), C.byref(ok))
        assert rc == 0
        acc = np.float32(carry)
        want = np.zeros(128, np.float32)
        for i in range(128):
            acc = np.float32(acc + x[i])
            want[i] = acc
        assert np.array_equal(np.concatenate([r0, r1]).view(np.uint32), want.view(np.uint32))
        if ok.value:
            assert np.array_equal(np.concatenate([o0, o1]).view(np.uint32), want.view(np.uint32)), (carry, kind)
            n_ok[kind] += 1
    assert all(n_ok[k] > 5 for k in range(5)), n_ok

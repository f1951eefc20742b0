"""Shapes for the pair body of front_end_fused_kernel (tests/test_emu_front_pairs.py on the emulator,
tests/test_gpu_front_pairs.py on the device): step counts around the pair logic and the ring's wrap, windows shifted
against the pair boundaries, both paths of the avg_ampl sum, ragged workgroups."""
import numpy as np

LEAK = np.complex64(1.0 * np.exp(0.7j))

# decimated samples per trace: around one step, one pair, one pair and a half; around the 16-slot ring's wrap; an odd number
# of full steps plus a partial one
N_DEC = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 16 * 64 - 1, 16 * 64, 16 * 64 + 1, 17 * 64, 35 * 64 + 17]
SHIFTS = [0, 1, 63, 64, 65, 127]


def step_count_batch(synth_mod):
    """one trace of one round, cut to every length of N_DEC (+ a few raw samples that make no further output)"""
    t = synth_mod.make_trace(n_rounds=1, seed=401, sigma=0.01).samples
    assert len(t) // 5 > max(N_DEC)
    lens = np.array([5 * n + (i % 5) for i, n in enumerate(N_DEC)], dtype=np.int64)
    raw = np.zeros((len(N_DEC), int(lens.max())), dtype=np.complex64)
    for i, n in enumerate(lens):
        raw[i, :n] = t[:n]
    return raw, lens


def shifted_batch(synth_mod):
    """one trace of two rounds behind 0..127 decimated samples of carrier: the RN16 / EPC openings and closings fall into the
    first step of a pair, the second, on the boundary between them and on the boundary between pairs"""
    t = synth_mod.make_trace(n_rounds=2, seed=402, sigma=0.01, t1_jitter_raw=3).samples
    L = len(t) + 5 * max(SHIFTS)
    raw = np.zeros((len(SHIFTS), L), dtype=np.complex64)
    lens = np.zeros(len(SHIFTS), dtype=np.int64)
    for i, sh in enumerate(SHIFTS):
        raw[i, : 5 * sh] = LEAK
        raw[i, 5 * sh: 5 * sh + len(t)] = t
        lens[i] = 5 * sh + len(t)
    return raw, lens


def sum_paths_batch(synth_mod):
    """row 0: a carrier whose filtered level (25 x 0.6444) lies just above 16, so that every reader command pulls avg_ampl
    down through the power of two and the carrier behind it back up -- the integer scan gives way to the chain inside pairs;
    row 1: sigma 0.06"""
    a = synth_mod.make_trace(n_rounds=2, seed=403, sigma=0.004, leak=0.6444 * np.exp(0.7j)).samples
    b = synth_mod.make_trace(n_rounds=2, seed=404, sigma=0.06).samples
    L = max(len(a), len(b))
    raw = np.zeros((2, L), dtype=np.complex64)
    raw[0, : len(a)] = a
    raw[1, : len(b)] = b
    return raw, np.array([len(a), len(b)], dtype=np.int64)


def ragged_batch(synth_mod, B):
    """B traces of 1..3 rounds with ragged lengths, one of them empty (B > 1)"""
    ts = [synth_mod.make_trace(n_rounds=1 + i % 3, seed=410 + i, sigma=0.02, t1_jitter_raw=5).samples for i in range(B)]
    cuts = [0, 1237, 0, 20001, 333]
    lens = np.array([max(len(t) - cuts[i], 0) for i, t in enumerate(ts)], dtype=np.int64)
    if B > 1:
        lens[B - 2] = 0
    raw = np.zeros((B, int(max(map(len, ts)))), dtype=np.complex64)
    for i, t in enumerate(ts):
        raw[i, : len(t)] = t
    return raw, lens


def avg_ampl(y):
    """The oracle's |x| and avg_ampl after every sample of its matched-filter output y (gate_impl.cc:130-134: the in-order
    binary32 sum of (|x| - |x[i-100]|) / 100) -> (amp, avg), binary32"""
    y = np.asarray(y, dtype=np.complex64)
    amp = np.sqrt(y.real.astype(np.float64) ** 2 + y.imag.astype(np.float64) ** 2).astype(np.float32)
    old = np.concatenate([np.zeros(100, np.float32), amp])[: len(amp)]
    d = ((amp - old) / np.float32(100)).astype(np.float32)
    avg = np.zeros(len(d), np.float32)
    acc = np.float32(0)
    for i in range(len(d)):
        acc = np.float32(acc + d[i])
        avg[i] = acc
    return amp, avg


def avg_ampl_pairs_leaving_binade(y):
    """The oracle's avg_ampl trajectory over its matched-filter output y -> the pairs of full steps, past the first two, inside
    which some partial sum has another exponent than the sum the pair starts from: there chain_add_scan_pair cannot apply and
    the chain is taken."""
    _, avg = avg_ampl(y)
    expo = (avg.view(np.uint32) >> 23) & 0xff
    out = []
    for p in range(2, (len(y) // 64) // 2):
        e0 = expo[128 * p - 1]
        if (expo[128 * p: 128 * p + 128] != e0).any():
            out.append(p)
    return out

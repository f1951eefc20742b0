"""Crafted inputs for the gate's state machine (gate_fsm_step, csrc/rfid_kernels.hpp) and the shortcuts built round it: what
rfid/synth.py never makes -- low phases across the PW/2 rule, pulse counts on either side of a command's, carrier that stops
at T1 to the sample, dips on the opening sample, windows that end with the trace, exact ties and exact zeros, noise that
crosses the threshold.  tests/test_gate_emu.py (emulator) and tests/test_gpu_gate.py (device) run them; what they reach is
counted by tests/gate_ref.py's replay over the ORACLE's matched-filter output, never from the kernels' output.

Every generator is seeded and returns (raw [B][L] complex64, lens, names)."""
import numpy as np

import gate_ref
from front_pairs_cases import LEAK, avg_ampl

TAG_H = np.complex64(0.05 * np.exp(2.1j))     # the weak square "tag" term: windows are not flat
TAG_PERIOD = 50                               # raw samples (40 kHz at 2 Msps)


def _pack(traces, names):
    lens = np.array([len(t) for t in traces], dtype=np.int64)
    raw = np.zeros((len(traces), int(lens.max())), dtype=np.complex64)
    for i, t in enumerate(traces):
        raw[i, : len(t)] = t
    return raw, lens, list(names)


def envelope_trace(segments, origin=0, sigma=0.0, rng=None):
    """segments: [(level 0 / 1, raw samples)] -> leak x envelope, plus the square term (its phase counted from raw sample
    `origin`, so that a longer lead-in in front of `origin` shifts everything behind it unchanged), plus noise"""
    env = np.concatenate([np.full(int(n), float(lv), dtype=np.float32) for lv, n in segments]) if segments else np.zeros(0, np.float32)
    t = np.arange(len(env)) - int(origin)
    sq = ((t % TAG_PERIOD) < TAG_PERIOD // 2).astype(np.float32)
    x = (env * (LEAK + TAG_H * sq)).astype(np.complex64)
    if sigma > 0:
        nz = (rng.standard_normal((len(x), 2)).astype(np.float32) * np.float32(sigma)).view(np.complex64)[:, 0]
        x = (x + nz).astype(np.complex64)
    return x


# ---- (a) random envelopes -------------------------------------------------------------------------------------------
LOW_SHORT = list(range(4, 13))          # raw samples: below-threshold runs of none to three decimated samples (the PW/2 edge)
LOW_LONG = list(range(13, 41))          # ... of four to about eight
CARRIER_NEAR_T1 = list(range(470, 501))  # raw samples round T1 = 97 x 5, sample by sample


IDLE_CARRIER = 19000                     # raw samples: longer than LS_QUIET (1615 decimated samples) + the idle-cut grid's step at the
                                         # smallest piece size (4 x 512), so that the long-stream front end finds a place to cut


def random_envelope_segments(rng, idle=False):
    """idle: one stretch of IDLE_CARRIER behind the third command -- where the long-stream front end can cut the trace, so
    that its state machine runs over the commands on either side and not the sequential scan in its place"""
    segs = [(1, 600 + int(rng.integers(0, 700)))]        # lead-in: moves everything against the 64 / 128-sample step grid
    total = segs[0][1]
    goal = int(rng.integers(30000, 60000))
    n_cmd = 0
    while total < goal:
        if idle and n_cmd == 3:
            segs.append((1, IDLE_CARRIER))
        n_cmd += 1
        cmd = []
        for _ in range(int(rng.integers(4, 10))):
            low = int(rng.choice(LOW_SHORT)) if rng.random() < 0.3 else int(rng.choice(LOW_LONG))
            cmd += [(0, low), (1, int(rng.integers(3, 121)))]
        u = rng.random()
        cmd.append((1, int(rng.choice(CARRIER_NEAR_T1)) if u < 0.5 else int(rng.integers(300, 701))))
        if rng.random() < 0.35:
            cmd.append((0, int(rng.integers(5, 25))))
        v = rng.random()     # what follows: short carrier, an RN16 window's worth, an EPC window's worth
        cmd.append((1, int(rng.integers(100, 1200)) if v < 0.3 else (int(rng.integers(1200, 2500)) if v < 0.65 else int(rng.integers(2500, 7001)))))
        segs += cmd
        total += sum(n for _, n in cmd)
    return segs


N_RANDOM_BATCHES = 3


def random_envelopes(batch, B=12):
    rng = np.random.default_rng(7100 + batch)
    traces, names = [], []
    for i in range(B):
        segs = random_envelope_segments(rng, idle=(i % 3 != 2))
        sigma = 0.0 if i % 2 == 0 else 0.01
        x = envelope_trace(segs, sigma=sigma, rng=rng)
        x = x[: 80000 - int(rng.integers(0, 5))]
        if i % 4 == 3:      # ends wherever it ends: inside a command, inside a window
            x = x[: len(x) - int(rng.integers(0, 3000))]
        traces.append(x)
        names.append("random%d_%d_sigma%g" % (batch, i, sigma))
    return _pack(traces, names)


# ---- (b) directed cases ---------------------------------------------------------------------------------------------
# Found by `python tests/gate_cases.py` (search_directed below: the oracle's filter and the replay of gate_ref only) and
# kept as literals in DIRECTED_PARAMS: name -> the parameters of directed_template().  directed_event() says what each must
# show; tests/test_gate_emu.py re-derives it.

def _cmd(n, low=25, high=40):
    return [(0, low), (1, high)] * n


def directed_template(name, p):
    """name, parameters -> (segments, origin, cut).  p["lead"]: raw samples of lead-in carrier (the origin of the square
    term: everything behind it is the same whatever the lead-in), p["x"]: the parameter searched, p["cut"]: decimated length"""
    lead, x = p["lead"], p.get("x", 0)
    name = name.split("#")[0]          # ("#k": the same case once more, at another lead-in)
    kind = name.split("@")[0]
    if kind.startswith("low"):                 # six counted pulses, then a low phase of x raw samples, then T1 of carrier
        body = _cmd(6) + [(0, x), (1, 900)]
    elif kind == "pulses5":
        body = _cmd(5) + [(1, 1200)]
    elif kind == "pulses6":
        body = _cmd(6) + [(1, 2200)]
    elif kind == "short_after_four":           # the count restarts at the fifth low phase; three more do not make a command
        body = _cmd(4, low=40) + [(0, x), (1, 100)] + _cmd(3) + [(1, 1200)]
    elif kind.startswith("dip"):               # a dip x raw samples after the last rising edge's carrier began
        body = _cmd(6) + [(1, x), (0, 25), (1, 2500)]
    elif kind.startswith("open_lane") or kind.startswith("close_lane"):
        body = _cmd(6) + [(1, 2600)]
    elif kind == "fall_after_close":           # the next command begins x raw samples of carrier behind the command's end
        body = _cmd(6) + [(1, x)] + _cmd(6) + [(1, 1000)]
    elif kind.startswith("rn16_end"):
        body = _cmd(6) + [(1, 2600)]
    elif kind.startswith("epc_end"):
        body = _cmd(6) + [(1, 485 + 1250 + 700)] + _cmd(6) + [(1, 485 + 6850 + 700)]
    elif kind == "short_trace_ends_low":
        return [(1, 200), (0, 60)], 0, None
    elif kind == "carrier_pulses_pending_long":   # ... 1900 samples of carrier: room for an idle cut, whose state would be wrong
        body = _cmd(3) + [(1, 9500)] + _cmd(3) + [(1, 2200)]
    elif kind == "carrier_epc_pending_long":
        body = _cmd(6) + [(1, 485 + 1250 + 9500)] + _cmd(6) + [(1, 485 + 6850 + 500)]
    elif kind == "carrier_pulses_pending":     # three pulses, 200 decimated samples of carrier, three more: one command's count
        body = _cmd(3) + [(1, 1000)] + _cmd(3) + [(1, 2200)]
    elif kind == "carrier_epc_pending":        # 300 samples of carrier behind an RN16 window, the next window an EPC
        body = _cmd(6) + [(1, 485 + 1250 + 1500)] + _cmd(6) + [(1, 485 + 6850 + 500)]
    else:
        raise KeyError(name)
    cut = p.get("cut")
    return [(1, lead)] + body, lead, (None if cut is None else 5 * cut + p.get("cut_extra", 0))


def analyse(oracle_mod, x):
    """raw trace -> (the oracle's filter output, the replay over its votes)"""
    y = oracle_mod.fir(x)
    below, above = gate_ref.votes_from_y(y)
    return y, gate_ref.replay(below, above)


def _ev(r, kind, pred=lambda e: True):
    return [e for e in r.events if e[0] == kind and pred(e)]


def directed_event(name, r, n_dec):
    """-> the index (decimated sample) of what the case is named for, or None when the trace does not show it"""
    name = name.split("#")[0]
    kind = name.split("@")[0]
    spec = name.split("@")[1] if "@" in name else ""
    if kind.startswith("low"):
        k = int(kind[3])
        e = _ev(r, "rise", lambda e: e[2] == k and e[4] == 6 and e[3] is not None)
        if len(e) != 1:
            return None
        want_windows = 0 if k <= 2 else 1
        if len(r.openings) != want_windows or e[0][5] != (0 if k <= 2 else 7):
            return None
        if spec:      # fall lane, rise lane, boundary kind
            fl, rl, where = spec.split("_")
            i = e[0][1]
            if (i - k) % 64 != int(fl) or i % 64 != int(rl):
                return None
            if ((i // 64) % 2 == 1) != (where == "steps"):     # the boundary inside a pair: the rising edge in its second step
                return None
        return e[0][1]
    if kind in ("pulses5", "pulses6"):
        n = int(kind[-1])
        e = _ev(r, "t1", lambda e: e[2] == n)
        ok = len(e) >= 1 and len(r.openings) == (1 if n == 6 else 0) and not _ev(r, "t1", lambda e: e[2] > n)
        return e[0][1] if ok else None
    if kind == "short_after_four":
        e = _ev(r, "rise", lambda e: e[2] <= gate_ref.PW_HALF and e[4] == 4 and e[5] == 0)
        t = _ev(r, "t1", lambda e: e[2] == 3)
        return e[0][1] if len(e) == 1 and len(t) == 1 and not r.openings else None
    if kind.startswith("dip"):
        where = spec
        if where == "after":
            e = _ev(r, "below_after_open")
            return e[0][1] if len(e) == 1 and len(r.openings) == 1 else None
        n_at = gate_ref.T1 + (0 if where == "before" else 1)
        e = _ev(r, "fall", lambda e: e[2] == n_at and e[3] > gate_ref.NUM_PULSES)
        return e[0][1] if len(e) == 1 else None
    if kind.startswith("open_lane"):
        lane = int(kind[len("open_lane"):])
        return r.openings[0][0] if len(r.openings) == 1 and r.openings[0][0] % 64 == lane else None
    if kind.startswith("close_lane"):
        lane = int(kind[len("close_lane"):])
        return r.closings[0] if len(r.closings) == 1 and r.closings[0] % 64 == lane else None
    if kind == "fall_after_close":
        if len(r.closings) < 1:
            return None
        e = _ev(r, "fall", lambda e: e[1] == r.closings[0] + 1)
        return e[0][1] if len(e) == 1 else None
    if kind.startswith("rn16_end") or kind.startswith("epc_end"):
        wt = 0 if kind.startswith("rn16") else 1
        o = [s for s, t in r.openings if t == wt]
        if len(o) != 1 or len(r.openings) != wt + 1:
            return None
        end = o[0] + gate_ref.WINDOW_LEN[wt]
        want = dict(last=end, short=end - 1, inside=end - 100)[spec]
        return o[0] if n_dec == want else None
    if kind == "short_trace_ends_low":
        return 0 if n_dec < 64 and r.state["signal_state"] == 0 and _ev(r, "fall") else None
    if kind.startswith("carrier_pulses_pending"):
        e = _ev(r, "t1", lambda e: e[2] == 3)
        if len(e) != 1 or len(r.openings) != 1:
            return None
        nxt = min(f[1] for f in _ev(r, "fall") if f[1] > e[0][1])
        return e[0][1] if nxt - (e[0][1] - gate_ref.T1) > 147 and r.openings[0][0] > nxt else None
    if kind.startswith("carrier_epc_pending"):
        if len(r.openings) != 2 or r.openings[1][1] != 1 or len(r.closings) < 1:
            return None
        nxt = min(f[1] for f in _ev(r, "fall") if f[1] > r.closings[0])
        return nxt if nxt - r.closings[0] > 147 else None
    raise KeyError(name)


DIRECTED_NAMES = (
    ["low1", "low2", "low3"] +
    ["low%d@%d_%d_%s" % (k, fl, rl, w) for w in ("steps", "pairs") for k, fl, rl in ((1, 63, 0), (2, 63, 1), (2, 62, 0), (3, 62, 1))] +
    ["pulses5", "pulses6", "short_after_four", "dip@before", "dip@at", "dip@after", "open_lane0", "open_lane63",
     "close_lane63", "close_lane0", "fall_after_close"] +
    ["%s_end@%s" % (t, w) for t in ("rn16", "epc") for w in ("inside", "last", "short")] +
    ["short_trace_ends_low", "carrier_pulses_pending", "carrier_epc_pending"] +
    # once and twice more at other lead-ins: what the random envelopes rarely hit
    ["%s#%d" % (n, k) for n in ("dip@before", "dip@at", "dip@after", "rn16_end@last", "rn16_end@short", "epc_end@last", "epc_end@short")
     for k in (1, 2)] + ["low1@63_0_steps#1", "carrier_pulses_pending_long", "carrier_epc_pending_long"])
# (open_lane0 is also the opening that is due on the first closed sample of its step: the step begins with n_samples = T1)

SEARCH_X = {"low": range(4, 25), "short_after_four": range(4, 25), "dip": range(430, 520), "fall_after_close": range(1700, 1800)}


def search_directed(oracle_mod, name):
    """-> parameters under which directed_event() holds: the searched length x, the raw offset of the lead-in (0..4: the
    decimation phase), and the lead-in's length in decimated samples -- one trial per value, then, because everything behind
    the lead-in moves with it, the shift that puts the event on the wanted lane, verified by a second replay"""
    base = 800 + 335 * (int(name.split("#")[1]) if "#" in name else 0)
    name = name.split("#")[0]
    kind = name.split("@")[0]
    xs = next((v for k, v in SEARCH_X.items() if kind.startswith(k)), [0])
    for x in xs:
        for off in range(5):
            for shift in range(0, 128):
                p = dict(lead=base + off + 5 * shift, x=x)
                if kind.endswith("_end"):
                    # the cut depends on where the window opens: find that first on the whole trace
                    segs, origin, _ = directed_template(name, p)
                    _, r0 = analyse(oracle_mod, envelope_trace(segs, origin))
                    wt = 0 if kind.startswith("rn16") else 1
                    o = [s for s, t in r0.openings if t == wt]
                    if len(o) != 1:
                        break
                    end = o[0] + gate_ref.WINDOW_LEN[wt]
                    p["cut"] = dict(last=end, short=end - 1, inside=end - 100)[name.split("@")[1]]
                    p["cut_extra"] = (x + off + shift) % 5
                segs, origin, cut = directed_template(name, p)
                xr = envelope_trace(segs, origin)[:cut]
                y, r = analyse(oracle_mod, xr)
                if directed_event(name, r, len(y)) is not None:
                    return p
                if "@" not in name and not kind.startswith(("open_lane", "close_lane")):
                    break           # no lane asked for: the lead-in does not matter
    raise RuntimeError("no parameters found for " + name)


DIRECTED_PARAMS = {
    'low1': {'lead': 803, 'x': 12},
    'low2': {'lead': 800, 'x': 13},
    'low3': {'lead': 801, 'x': 13},
    'low1@63_0_steps': {'lead': 1193, 'x': 12},
    'low2@63_1_steps': {'lead': 1190, 'x': 13},
    'low2@62_0_steps': {'lead': 1185, 'x': 13},
    'low3@62_1_steps': {'lead': 1186, 'x': 13},
    'low1@63_0_pairs': {'lead': 873, 'x': 12},
    'low2@63_1_pairs': {'lead': 870, 'x': 13},
    'low2@62_0_pairs': {'lead': 865, 'x': 13},
    'low3@62_1_pairs': {'lead': 866, 'x': 13},
    'pulses5': {'lead': 800, 'x': 0},
    'pulses6': {'lead': 800, 'x': 0},
    'short_after_four': {'lead': 800, 'x': 13},
    'dip@before': {'lead': 802, 'x': 442},
    'dip@at': {'lead': 802, 'x': 448},
    'dip@after': {'lead': 802, 'x': 453},
    'open_lane0': {'lead': 1070, 'x': 0},
    'open_lane63': {'lead': 1065, 'x': 0},
    'close_lane63': {'lead': 1100, 'x': 0},
    'close_lane0': {'lead': 1105, 'x': 0},
    'fall_after_close': {'lead': 800, 'x': 1700},
    'rn16_end@inside': {'lead': 800, 'x': 0, 'cut': 480, 'cut_extra': 0},
    'rn16_end@last': {'lead': 800, 'x': 0, 'cut': 580, 'cut_extra': 3},
    'rn16_end@short': {'lead': 800, 'x': 0, 'cut': 579, 'cut_extra': 4},
    'epc_end@inside': {'lead': 800, 'x': 0, 'cut': 2165, 'cut_extra': 1},
    'epc_end@last': {'lead': 800, 'x': 0, 'cut': 2265, 'cut_extra': 0},
    'epc_end@short': {'lead': 800, 'x': 0, 'cut': 2264, 'cut_extra': 2},
    'short_trace_ends_low': {'lead': 0, 'x': 0},
    'carrier_pulses_pending': {'lead': 800, 'x': 0},
    'carrier_epc_pending': {'lead': 800, 'x': 0},
    'carrier_pulses_pending_long': {'lead': 800, 'x': 0},
    'carrier_epc_pending_long': {'lead': 800, 'x': 0},
    'dip@before#1': {'lead': 1137, 'x': 442},
    'dip@before#2': {'lead': 1472, 'x': 442},
    'dip@at#1': {'lead': 1137, 'x': 448},
    'dip@at#2': {'lead': 1472, 'x': 448},
    'dip@after#1': {'lead': 1137, 'x': 453},
    'dip@after#2': {'lead': 1472, 'x': 453},
    'rn16_end@last#1': {'lead': 1135, 'x': 0, 'cut': 647, 'cut_extra': 0},
    'rn16_end@last#2': {'lead': 1470, 'x': 0, 'cut': 714, 'cut_extra': 0},
    'rn16_end@short#1': {'lead': 1135, 'x': 0, 'cut': 646, 'cut_extra': 0},
    'rn16_end@short#2': {'lead': 1470, 'x': 0, 'cut': 713, 'cut_extra': 0},
    'epc_end@last#1': {'lead': 1135, 'x': 0, 'cut': 2332, 'cut_extra': 0},
    'epc_end@last#2': {'lead': 1470, 'x': 0, 'cut': 2399, 'cut_extra': 0},
    'epc_end@short#1': {'lead': 1135, 'x': 0, 'cut': 2331, 'cut_extra': 0},
    'epc_end@short#2': {'lead': 1470, 'x': 0, 'cut': 2398, 'cut_extra': 0},
    'low1@63_0_steps#1': {'lead': 1833, 'x': 12},
}


# behind every directed trace but those that are about where the trace ends: carrier the long-stream front end can cut in,
# then one more command and its window.  What a case is named for lies in front of that: directed_event() looks at the replay
# of the first HEAD_DEC[name] decimated samples, whose votes the tail cannot change.
ENV_IDLE_TAIL = [(1, IDLE_CARRIER)] + _cmd(6) + [(1, 485 + 1250 + 500)]
HEAD_DEC = {}


def has_idle_tail(name):
    return "_end@" not in name and not name.startswith("short_trace")


def directed():
    traces = []
    for name in DIRECTED_NAMES:
        segs, origin, cut = directed_template(name, DIRECTED_PARAMS[name])
        head = envelope_trace(segs, origin)[:cut]
        HEAD_DEC[name] = len(head) // 5
        traces.append(envelope_trace(segs + ENV_IDLE_TAIL, origin) if has_idle_tail(name) else head)
    return _pack(traces, DIRECTED_NAMES)


# ---- (c) exact ties and exact zeros ---------------------------------------------------------------------------------
# Samples that are small integers with zero imaginary part: every sum of the filter, |y|, the division by 100 and avg_ampl are
# exact in binary32 whatever the order.  The traces are stated as the filter output y (multiples of 100, so that every
# (|y| - |y[i-100]|) / 100 is an integer); raw_from_y() makes the raw samples whose boxcar IS that y.
def raw_from_y(y):
    """integer y (multiples of 5) -> raw samples, constant over each block of five, with y[k] = the sum of raw[5k-24 .. 5k] (the
    blocks end at the samples 5k): block value v[k] = v[k-5] + (y[k] - y[k-1]) / 5"""
    y = np.asarray(y, dtype=np.int64)
    y = np.concatenate([y, y[-1:]])        # (the samples behind 5(N-1) that make the length 5N + 1: no further output)
    assert (y % 5 == 0).all() and y[0] == 0       # (output 0 sums one sample only)
    v = np.zeros(len(y) + 5, dtype=np.int64)
    prev = 0
    for k in range(len(y)):
        v[k + 5] = v[k] + (y[k] - prev) // 5
        prev = y[k]
    v = v[5:]
    assert np.abs(v).max() < 4096
    return np.repeat(v, 5)[4:].astype(np.float32).astype(np.complex64)


C = 400                                   # carrier level of y
TAGGED = [400] * 5 + [500] * 5            # carrier with a square term in it: a window's content is not flat


def _ycmd(n=6, low=10, high=15):
    return ([0] * low + [C] * high) * n


PERIOD = [400] * 40 + [300] * 10 + [0] * 10 + [300] * 10 + [500] * 20 + [800] * 10     # mean 400: 300 = 0.75 x 400 exactly
assert len(PERIOD) == 100 and sum(PERIOD) == 100 * C


def tie_y(name):
    if name == "ties_leading_zeros":           # avg == amp == thresh == 0 in front: neither vote
        return [0] * 37 + [C] * 200 + _ycmd() + [C] * 95 + TAGGED * 60 + [C] * 300
    if name == "ties_zero_stretch_resets_avg":  # 120 zeros behind carrier: avg_ampl is exactly 0 again, then ties
        return [0] * 5 + [C] * 145 + [0] * 120 + [C] * 200 + _ycmd() + [C] * 95 + TAGGED * 60 + [C] * 200
    if name == "ties_zeros_in_carrier_command_window":
        return ([0] * 5 + [C] * 145 + [0] * 8 + [C] * 150 + _ycmd(3) + [0] * 30 + [C] * 15 + _ycmd(3) + [C] * 95 + TAGGED * 10 + [0] * 8 +
                TAGGED * 40 + [C] * 200 + _ycmd() + [C] * 95 + TAGGED * 150 + [C] * 50)
    if name == "ties_periodic":                # avg_ampl stays exactly 400: the 300s are ties, behind POS_EDGE and behind NEG_EDGE
        return [0] * 5 + [C] * 145 + PERIOD * 9 + [C] * 95 + TAGGED * 60 + [C] * 200
    raise KeyError(name)


# behind each: carrier for longer than LS_QUIET (1615 samples) + the idle-cut grid's step at the smallest piece size (4 x 512),
# so that the long-stream front end finds a place to cut whatever the grid's phase, then one more round
IDLE_TAIL = [C] * 3800 + _ycmd() + [C] * 95 + TAGGED * 150 + [C] * 100


TIE_NAMES = ["ties_leading_zeros", "ties_zero_stretch_resets_avg", "ties_zeros_in_carrier_command_window", "ties_periodic"]


def ties():
    """-> (raw, lens, names, ys): ys[b] the filter output the trace was built for (complex64)"""
    ys = [np.asarray(tie_y(n) + IDLE_TAIL, dtype=np.float32).astype(np.complex64) for n in TIE_NAMES]
    raw, lens, names = _pack([raw_from_y(np.asarray(tie_y(n) + IDLE_TAIL)) for n in TIE_NAMES], TIE_NAMES)
    return raw, lens, names, ys


# ---- (d) threshold chatter ------------------------------------------------------------------------------------------
CHATTER_SIGMA = [0.15, 0.25, 0.4]


def chatter(synth_mod):
    traces = [synth_mod.make_trace(n_rounds=2, seed=7300 + i, sigma=s).samples for i, s in enumerate(CHATTER_SIGMA)]
    return _pack(traces, ["chatter_sigma%g" % s for s in CHATTER_SIGMA])


def all_batches(synth_mod):
    """-> [(batch name, raw, lens, names)]: every crafted batch, at most 16 traces each"""
    out = [("random%d" % k,) + random_envelopes(k) for k in range(N_RANDOM_BATCHES)]
    raw, lens, names = directed()
    for b0 in range(0, len(names), 16):
        out.append(("directed%d" % (b0 // 16), raw[b0:b0 + 16], lens[b0:b0 + 16], names[b0:b0 + 16]))
    out.append(("ties",) + ties()[:3])
    out.append(("chatter",) + chatter(synth_mod))
    return out


NOISE_FREE = ("random", "directed", "ties")      # (the random batches' sigma 0.01 stays far below the threshold)


_crafted = []


def crafted(oracle_mod, synth_mod):
    """every crafted batch with its references, computed once per process and shared by the tests (which leave it unchanged):
    [dict(name, raw, lens, rows)]; rows[b]: name, x (the raw trace), o (oracle.run_trace), y (oracle.fir), below / above
    (gate_ref.votes_from_y), replay (gate_ref.replay in batch mode), cover (coverage()), head_n / head_replay (a directed trace
    without its idle tail)"""
    if not _crafted:
        for bname, raw, lens, names in all_batches(synth_mod):
            rows = []
            for b in range(len(raw)):
                x = raw[b][: lens[b]]
                y = oracle_mod.fir(x)
                below, above = gate_ref.votes_from_y(y)
                r = gate_ref.replay(below, above)
                hn = HEAD_DEC.get(names[b], len(y)) if bname.startswith("directed") else len(y)
                rows.append(dict(name=names[b], x=x, o=oracle_mod.run_trace(x), y=y, below=below, above=above, replay=r,
                                 cover=coverage(r, len(y)), head_n=hn,
                                 head_replay=r if hn == len(y) else gate_ref.replay(below[:hn], above[:hn])))
            _crafted.append(dict(name=bname, raw=raw, lens=lens, rows=rows))
    return _crafted


def noise_free(batch_name):
    return batch_name.startswith(NOISE_FREE)


# ---- coverage, from the replay alone --------------------------------------------------------------------------------
def coverage(r, n_dec):
    """the replay of one trace -> {event name: count}"""
    c = {}

    def add(k, n=1):
        c[k] = c.get(k, 0) + n
    for e in _ev(r, "rise"):
        _, i, low, fall, before, after = e
        if fall is None:
            continue
        k = "low%s" % (low if low < 4 else "4+")
        add("rise_" + k)
        if fall // 64 != i // 64:
            add("rise_%s_across_64" % k)
        if low <= gate_ref.PW_HALF and before > 0:
            add("restart_nonzero")
    for e in _ev(r, "t1"):
        if e[2] in (5, 6):
            add("t1_pulses%d" % e[2])
    for e in _ev(r, "fall"):
        if e[3] > gate_ref.NUM_PULSES and e[2] in (gate_ref.T1, gate_ref.T1 + 1):
            add("fall_at_popen" if e[2] == gate_ref.T1 + 1 else "fall_at_popen-1")
    add("fall_at_popen+1", len(_ev(r, "below_after_open")))
    for s, t in r.openings:
        if s % 64 in (0, 63):
            add("open_lane%d" % (s % 64))
        end = s + gate_ref.WINDOW_LEN[t]
        for nm, at in (("last", end), ("short", end - 1)):
            if n_dec == at:
                add("%s_end_%s" % ("epc" if t else "rn16", nm))
        if n_dec < end - 1:
            add("%s_end_inside" % ("epc" if t else "rn16"))
    for i in r.closings:
        if i % 64 in (0, 63):
            add("close_lane%d" % (i % 64))
    for e in _ev(r, "tie"):
        add("tie_state%d" % e[2])
    add("windows", len(r.openings))
    return c


COVERED = (["rise_low%s%s" % (k, x) for k in ("1", "2", "3", "4+") for x in ("", "_across_64")] +
           ["restart_nonzero", "t1_pulses5", "t1_pulses6", "fall_at_popen-1", "fall_at_popen", "fall_at_popen+1", "open_lane0",
            "open_lane63", "close_lane0", "close_lane63"] +
           ["%s_end_%s" % (t, w) for t in ("rn16", "epc") for w in ("inside", "last", "short")])
MIN_EACH, MIN_TIES = 3, 50


# ---- records for the step function by itself ------------------------------------------------------------------------
def _rec(mode, st, below, above, nvalid, pos):
    return (mode, st["n_samples"], st["signal_state"], st["num_pulses"], st["open"], st["n_to_ungate"], st["wtype"], nvalid, pos, 0,
            below, above)


def fsm_records_random(capi, n=4096, seed=5):
    """States from the corners x masks sparse, dense and alternating x every nvalid.
    What gate_fsm_step's contract excludes is left out here, never compared more loosely:
    - an open gate with n_samples >= n_to_ungate (the step that reaches n_to_ungate closes the gate itself), so the corner
      n_to_ungate - n_samples = 0 yields no record;
    - n_to_ungate other than the window length of wtype (it is set from wtype wherever the gate is armed);
    - votes that overlap, or lie at or past nvalid (the callers mask them: gate_consume, ls2_fsm_kernel)."""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    while len(out) < n:
        k += 1
        mode = int(rng.integers(0, 2))
        wtype = int(rng.integers(0, 2))
        ung = gate_ref.WINDOW_LEN[wtype]
        is_open = int(rng.random() < 0.3)
        if is_open:
            n_s = ung - int(rng.choice([0, 1, 63, 64, 65, 129]))
            if n_s >= ung:
                continue
        else:
            n_s = int(rng.choice([0, 1, 2, 3, 95, 96, 97, 98, 127, 128]))
        st = dict(n_samples=n_s, signal_state=int(rng.integers(0, 2)), num_pulses=int(rng.choice([0, 4, 5, 6, 7])), open=is_open,
                  n_to_ungate=ung, wtype=wtype)
        nvalid = (k % 65) if k % 3 == 0 else 64
        kind = k % 4
        if kind == 0:      # sparse: one to four marks
            marks = rng.integers(0, 64, int(rng.integers(1, 5)))
            below = above = 0
            for m in marks:
                if rng.random() < 0.5:
                    below |= 1 << int(m)
                else:
                    above |= 1 << int(m)
            above &= ~below
        elif kind == 1:    # dense
            a, b = int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(0, 2)), int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(0, 2))
            below, above = a & ~b, b & ~a
        elif kind == 2:    # strictly alternating, in either phase, with or without gaps
            base = 0x5555555555555555
            below, above = (base, base << 1) if rng.random() < 0.5 else (base << 1, base)
            if rng.random() < 0.5:
                keep = int(rng.integers(0, 1 << 63)) << 1 | 1
                below &= keep
                above &= keep
        else:              # runs: a low phase of one to five samples somewhere, the rest above or nothing
            s0, ln = int(rng.integers(0, 64)), int(rng.integers(1, 6))
            below = ((1 << ln) - 1) << s0
            above = ~below if rng.random() < 0.6 else (1 << int(rng.integers(0, 64)))
            above &= ~below
        vm = (1 << nvalid) - 1
        out.append(_rec(mode, st, below & vm & (2 ** 64 - 1), above & vm & (2 ** 64 - 1), nvalid, 64 * int(rng.integers(0, 40))))
    return np.array(out, dtype=capi.GATE_FSM_IN_DTYPE)


def fsm_records_of_trace(capi, below, above, mode=0):
    """every 64-sample step the replay passes through on one trace's votes, each from the state the replay had there (batch
    mode: the states gate_consume and the long-stream units see; with mode 1 the same states, stopping at a window's end)"""
    out = []
    st = gate_ref.fresh_state()
    N = len(below)
    for p in range(0, N, 64):
        nv = min(64, N - p)
        b, a = gate_ref.mask_of(below[p:p + nv]), gate_ref.mask_of(above[p:p + nv])
        out.append(_rec(mode, st, b, a, nv, p))
        st = gate_ref.replay(below[p:p + nv], above[p:p + nv], st, 0).state
    return np.array(out, dtype=capi.GATE_FSM_IN_DTYPE)


def fsm_expected(capi, recs):
    out = np.zeros(len(recs), dtype=capi.GATE_FSM_OUT_DTYPE)
    for i, rec in enumerate(recs):
        e = gate_ref.step64(rec)
        for k, v in e.items():
            out[i][k] = v
    return out


# ---- what tests/test_gate_emu.py and tests/test_gpu_gate.py share ---------------------------------------------------
BATCHES = (["random%d" % k for k in range(N_RANDOM_BATCHES)] + ["directed%d" % k for k in range((len(DIRECTED_NAMES) + 15) // 16)] +
           ["ties", "chatter"])


def batch_of(crafted_, name):
    return next(b for b in crafted_ if b["name"] == name)


def fsm_records(capi, crafted_):
    """corner states x crafted masks, and every step the replay passes through on the crafted traces (in per-call mode as
    well where the gate is open: only there the mode can matter) -- each record once (the traces' idle steps are all alike)"""
    recs = [fsm_records_random(capi)]
    for batch in crafted_:
        for row in batch["rows"]:
            t = fsm_records_of_trace(capi, row["below"], row["above"])
            recs.append(t)
            m1 = t[t["gate_open"] == 1].copy()
            m1["mode"] = 1
            recs.append(m1)
    return np.unique(np.concatenate(recs))


_fsm = []


def check_fsm(capi, run, crafted_):
    """run(records) -> (wave-uniform form, per-lane form): every output word of both against gate_ref.step64, a few thousand
    records per launch.  -> (records, expected)"""
    if not _fsm:
        recs = fsm_records(capi, crafted_)
        _fsm.append((recs, fsm_expected(capi, recs)))
    recs, want = _fsm[0]
    for lo in range(0, len(recs), 4096):
        ow, ol = run(recs[lo:lo + 4096])
        w = want[lo:lo + 4096]
        for name in capi.GATE_FSM_OUT_DTYPE.names:
            for form, got in (("wave-uniform form", ow), ("per-lane form", ol)):
                bad = np.nonzero(got[name] != w[name])[0]
                assert len(bad) == 0, (form, name, recs[lo + bad[0]], got[bad[0]], w[bad[0]])
        assert ow.tobytes() == ol.tobytes()
    # the records do reach what they are for
    assert len(recs) > 8000 and (want["open_lane"] != 0xff).sum() > 100 and want["stop"].sum() > 20
    assert set(np.unique(recs["nvalid"])) >= set(range(65))
    assert ((want["open_lane"] == 0) & (recs["n_samples"] >= gate_ref.T1)).any()      # need == 0
    return recs, want


def compare_batch(parity, batch, windows, results, scores, stats, ys=None):
    """one pass over a crafted batch against the oracle: parity.compare_trace per trace, the filter output bit for bit"""
    B = len(batch["rows"])
    for b, (wb, rb, sb) in enumerate(parity.split_by_stream(windows, results, scores, B)):
        row = batch["rows"][b]
        if ys is not None:
            n = len(row["y"])
            assert np.array_equal(np.asarray(ys[b][:n]).view(np.uint32), row["y"].view(np.uint32)), (row["name"], "y")
        try:
            parity.compare_trace(wb, rb, sb, stats[b], row["o"])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (row["name"], e)) from e


CHUNKS = [777, 64, 1, 63, 1500, 129]


def per_call_gate(oracle_mod, y, work):
    """the oracle's filter output through gate_impl::general_work call by call in odd chunk sizes: consumed, the samples
    written and the open flag of work(block, seek_type) -> (consumed, samples, open flag or None) against orc_gate_work's.
    seek_type: -1, or the type the decoder and reader re-arm the gate for before this call.  -> windows closed"""
    import ctypes as C
    L = oracle_mod.lib()
    g = (C.c_char * 8192)()
    rs = oracle_mod.ReaderState()
    cfg = oracle_mod.config()
    L.orc_gate_init(C.byref(g), 400000)
    L.orc_initialize_reader_state(C.byref(rs), C.byref(cfg))
    rs.gate_status = 2   # SEEK_RN16
    pos, seek, typ, k, n_closed = 0, 0, 0, 0, 0
    while pos < len(y):
        n = min(CHUNKS[k % len(CHUNKS)], len(y) - pos)
        k += 1
        blk = np.ascontiguousarray(y[pos:pos + n])
        out_o = np.zeros(n, dtype=np.complex64)
        cons_o = C.c_int(0)
        wr_o = L.orc_gate_work(C.byref(g), C.byref(rs), C.c_void_p(blk.ctypes.data), n, C.c_void_p(out_o.ctypes.data), C.byref(cons_o))
        cons_e, out_e, open_e = work(blk, seek)
        seek = -1
        assert cons_e == cons_o.value and len(out_e) == wr_o, (pos, cons_e, cons_o.value, len(out_e), wr_o)
        assert np.array_equal(out_e.view(np.uint32), out_o[:wr_o].view(np.uint32)), pos
        assert open_e is None or open_e == (1 if rs.gate_status == 0 else 0), pos
        pos += cons_o.value
        if wr_o and rs.gate_status == 1:      # window closed: decoder and reader re-arm the gate
            typ ^= 1
            rs.gate_status = 3 if typ else 2
            seek = typ
            n_closed += 1
    return n_closed


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle
    oracle.build()
    print("DIRECTED_PARAMS = {")
    for nm in (sys.argv[1:] or DIRECTED_NAMES):
        print("    %r: %r," % (nm, search_directed(oracle, nm)), flush=True)
    print("}")

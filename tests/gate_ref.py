"""The gate's edge / pulse / window state machine on threshold votes, one sample per iteration: a plain restatement of
gate_impl.cc:145-195 as the oracle states it (oracle/rfid_oracle.c, orc_gate_work) -- no masks, no tricks.  The reference of
gate_fsm_step (csrc/rfid_kernels.hpp) in tests/test_gate_emu.py and tests/test_gpu_gate.py, and the counter of what the crafted
traces of tests/gate_cases.py reach.  Validated there against oracle.run_trace: same openings, same types, on every trace."""
import numpy as np

from oracle.oracle import WINDOW_LEN          # 250 (RN16) / 1370 (EPC) samples per window

from front_pairs_cases import avg_ampl

T1 = 96             # n_samples_T1 (gate_impl.cc:48): the gate opens at the first sample with n_samples > T1, the 97th after an edge
PW_HALF = 2         # n_samples_PW / 2 (:157): a low phase counts as a pulse when it lasted more than this
NUM_PULSES = 5      # NUM_PULSES_COMMAND: a command has more pulses than this
GATE_N_SAT = 128    # the kernels keep n_samples of a closed gate clamped here (no comparison can tell); the
                    # clamp goes into the state this file REPORTS, never into the count it runs on
THRESH_FRACTION = np.float32(0.75)
FIELDS = ("n_samples", "signal_state", "num_pulses", "open", "n_to_ungate", "wtype")


def fresh_state():
    return dict(n_samples=0, signal_state=0, num_pulses=0, open=0, n_to_ungate=WINDOW_LEN[0], wtype=0)


def votes_from_y(y):
    """the oracle's matched-filter output -> (below, above): amp < thresh, amp > thresh with thresh = avg_ampl * 0.75f, all in
    binary32 (gate_impl.cc:130-136,147,155)"""
    amp, avg = avg_ampl(y)
    thresh = (avg * THRESH_FRACTION).astype(np.float32)
    return amp < thresh, amp > thresh


class Replay:
    """what replay() leaves: closed / inwin (bool per sample taken; the opening sample is both), openings [(index, type)],
    closings [index of a window's last sample], state (n_samples clamped while closed), n_taken, stop, events"""


def replay(below, above, state=None, mode=0):
    """mode 0 (batch): the gate re-arms behind a window -- the type alternates, the count restarts (what the decoder and
    reader blocks do between two calls, gate_impl.cc:112-123).  mode 1 (per call): the scan stops where a window closes and
    n_taken says how many samples went in (consume_each).
    events: ("rise", i, low, fall_index or None, pulses before, pulses after) -- low = n_samples at the rising edge, the length
    of the low phase; ("fall", i, n_samples it ended, pulses); ("t1", i, pulses): n_samples passes T1 at POS_EDGE, gate closed;
    ("below_after_open", i): a vote below the threshold on the sample behind an opening; ("tie", i, signal_state): neither
    vote, gate closed."""
    st = dict(state or fresh_state())
    n, sig, pulses, is_open, ung, wtype = (int(st[k]) for k in FIELDS)
    N = len(below)
    closed = np.zeros(N, dtype=bool)
    inwin = np.zeros(N, dtype=bool)
    openings, closings, events = [], [], []
    fall_at = None
    stop = False
    taken = 0
    for i in range(N):
        b, a = bool(below[i]), bool(above[i])
        taken = i + 1
        if not is_open:
            closed[i] = True
            n += 1
            if not b and not a:
                events.append(("tie", i, sig))
            if b and sig == 1:
                events.append(("fall", i, n, pulses))
                n = 0
                sig = 0
                fall_at = i
            elif a and sig == 0:
                sig = 1
                before = pulses
                pulses = pulses + 1 if n > PW_HALF else 0
                events.append(("rise", i, n, fall_at, before, pulses))
                n = 0
            if n == T1 + 1 and sig == 1:
                events.append(("t1", i, pulses))
            if n > T1 and sig == 1 and pulses > NUM_PULSES:
                is_open = 1
                inwin[i] = True
                openings.append((i, wtype))
                pulses = 0
                n = 1
                if i + 1 < N and below[i + 1]:
                    events.append(("below_after_open", i + 1))
        else:
            n += 1
            inwin[i] = True
            if n >= ung:
                is_open = 0
                closings.append(i)
                if mode == 0:
                    n = 0
                    wtype ^= 1
                    ung = WINDOW_LEN[wtype]
                else:
                    stop = True
                    break
    r = Replay()
    r.closed, r.inwin, r.openings, r.closings, r.events = closed[:taken], inwin[:taken], openings, closings, events
    r.n_taken, r.stop = taken, stop
    r.state = dict(n_samples=n if is_open or n <= GATE_N_SAT else GATE_N_SAT, signal_state=sig, num_pulses=pulses, open=is_open,
                   n_to_ungate=ung, wtype=wtype)
    r.state_unclamped = dict(r.state, n_samples=n)
    return r


def mask_of(bits):
    """bool per sample (at most 64) -> the 64-bit mask with sample i at bit i"""
    m = 0
    for i, v in enumerate(bits):
        if v:
            m |= 1 << i
    return m


def bits_of(mask, n=64):
    return [(int(mask) >> i) & 1 == 1 for i in range(n)]


def step64(rec):
    """One step of at most 64 votes from the record's own state: what gate_fsm_step must leave, word for word.
    rec: mode, the six state words (capi.GATE_FSM_IN_DTYPE names), nvalid, pos, below, above -> dict of GATE_FSM_OUT_DTYPE"""
    nvalid = int(rec["nvalid"])
    st = dict(n_samples=int(rec["n_samples"]), signal_state=int(rec["signal_state"]), num_pulses=int(rec["num_pulses"]),
              open=int(rec["gate_open"]), n_to_ungate=int(rec["n_to_ungate"]), wtype=int(rec["wtype"]))
    r = replay(bits_of(rec["below"], nvalid), bits_of(rec["above"], nvalid), st, int(rec["mode"]))
    assert len(r.openings) <= 1
    s = r.state
    return dict(n_samples=s["n_samples"], signal_state=s["signal_state"], num_pulses=s["num_pulses"], gate_open=s["open"],
                n_to_ungate=s["n_to_ungate"], wtype=s["wtype"], nvalid=r.n_taken if r.stop else nvalid, stop=int(r.stop),
                consumed=int(rec["pos"]) + r.n_taken if r.stop else 0,
                open_lane=r.openings[0][0] if r.openings else 0xff, open_type=r.openings[0][1] if r.openings else 0,
                reserved_=0, closedmask=mask_of(r.closed), openmask=mask_of(r.inwin))

"""CPU-only checks of the dc_est finishing walk (ls2_dcb_finish_kernel, csrc/rfid_ls2.hpp) in its DEVICE form: G one-wave
workgroups per trace that meet once per turn (wv::grid_meet), hand their tables to each other through two scratch sets used turn
about, and agree on the units each wave explores.  The emulator (tests/wave_emu) is built with LS2_FIN_WPB = 1, as the device is,
keeps every workgroup of a launch resident at once and interleaves them by a seeded schedule; a launch in which every live
workgroup waits is reported (EmuDeadlock), not hung.  The inputs put one component of dc_est next to a power of two (25 |sin phi|
or 25 |cos phi| within 1.2 % of 4, 8 or 16): the sums hover across a binade edge, nothing settles by rounds and the walk takes the
units.  Every case must be the oracle's sequential scan bit for bit.  (The emulator is sequentially consistent: fences and
acquire / release are checked on the MI355X only, tests/test_gpu_fin_walk.py.)"""
import numpy as np
import pytest

import parity

SCHEDULE_KINDS = ("in-order", "reversed", "random", "late")


def hover_traces(synth_mod, seed, edge, comp, sign, sigma, n_rounds, B=1, ragged=False, off=0.004):
    """B traces whose carrier puts dc_est's real (comp "cos") or imaginary (comp "sin") part at `edge` (1 + off), |off| <= 1.2 %
    -> (raw, lens)"""
    assert abs(off) <= 0.012
    rng = np.random.default_rng(seed)
    target = edge * (1.0 + off)
    phi = float(np.arcsin(target / 25.0)) if comp == "sin" else float(np.arccos(target / 25.0))
    leak = complex(np.exp(1j * sign * phi))
    ts = [synth_mod.make_trace(n_rounds=n_rounds, seed=int(rng.integers(1, 1 << 30)), sigma=sigma, tag_ids=(7, 91),
                               t1_jitter_raw=int(rng.integers(0, 6)), leak=leak).samples for _ in range(B)]
    L = max(map(len, ts))
    raw = np.zeros((B, L), dtype=np.complex64)
    for b, t in enumerate(ts):
        raw[b, :len(t)] = t
    lens = [len(t) - (int(rng.integers(1000, 30000)) if ragged and b % 2 == 1 else 0) for b, t in enumerate(ts)] if (ragged or B > 1) else None
    return raw, lens


_ORACLE = {}


def oracle_of(oracle_mod, key, raw, lens):
    if key not in _ORACLE:
        _ORACLE[key] = [oracle_mod.run_trace(raw[b, :(raw.shape[1] if lens is None else lens[b])], oracle_mod.config())
                        for b in range(raw.shape[0])]
    return _ORACLE[key]


def check_walk(emu_mod, refs, raw, lens, **kw):
    """the run against the oracle, every trace; the walk must have run and taken every unit the rounds left"""
    r = emu_mod.ls2_process(raw, lens=lens, **kw)
    for b, (wb, rb, sb) in enumerate(parity.split_by_stream(r["windows"], r["results"], r["scores"], raw.shape[0])):
        parity.compare_trace(wb, rb, sb, r["stats"][b], refs[b])
    c = r["ctl"]
    assert r["ok"] == 1 and c["dc_finished"] > 0, c             # (accepted: every unit settled, dc_count at the last round 0)
    if kw.get("dc_rounds") == 0:
        assert c["dc_count0"] == 0, c
    return r


# (G, edge, component, sign, sigma, dc_rounds, traces, ragged, fused, schedule, trace seed): every G of the device's range that changes
# what the walk does -- one wave (M = 1, nothing to meet), a few, G < 16 (one window per unit), 16 (M adapts from 4), G / M not
# whole.  (dc_rounds 1: a re-run round before the walk.  With the rounds as the library enqueues them, traces this short settle by
# rounds alone; tests/test_gpu_fin_walk.py runs that form.)  The seeds give traces on which the walk takes units
WPB1_CASES = [
    (1, 16.0, "sin", 1, 0.06, 0, 1, False, False, "random", 101),
    (2, 8.0, "cos", -1, 0.03, 0, 2, True, True, "random", 102),
    (3, 16.0, "cos", 1, 0.06, 1, 1, False, True, "late", 105),
    (7, 4.0, "sin", -1, 0.06, 0, 2, True, False, "random", 107),
    (15, 16.0, "sin", -1, 0.03, 0, 1, False, False, "reversed", 115),
    (16, 8.0, "sin", 1, 0.06, 0, 1, False, True, "random", 116),
    (17, 16.0, "cos", -1, 0.06, 1, 3, True, False, "random", 118),
    (31, 4.0, "cos", 1, 0.03, 0, 1, False, False, "late", 132),
    (64, 16.0, "sin", 1, 0.06, 0, 2, False, False, "in-order", 164),
]


@pytest.mark.parametrize("G,edge,comp,sign,sigma,dc_rounds,B,ragged,fused,schedule,seed", WPB1_CASES,
                         ids=[f"G{c[0]}-{c[2]}{'+' if c[3] > 0 else '-'}{c[1]:g}-s{c[4]}-r{c[5]}-B{c[6]}{'-fused' if c[8] else ''}-{c[9]}"
                              for c in WPB1_CASES])
def test_fin_walk_one_wave_workgroups_match_oracle(emu_mod, oracle_mod, synth_mod, G, edge, comp, sign, sigma, dc_rounds, B, ragged,
                                                   fused, schedule, seed):
    raw, lens = hover_traces(synth_mod, seed, edge, comp, sign, sigma, n_rounds=22 if B == 1 else 14, B=B, ragged=ragged, off=0.003)
    refs = oracle_of(oracle_mod, ("wpb1", G), raw, lens)
    check_walk(emu_mod, refs, raw, lens, dc_rounds=dc_rounds, fused=fused, fin_wpb=1, fin_waves=G, schedule=schedule, seed=G)


@pytest.mark.parametrize("schedule,dc_rounds,fused", [("random", 0, False), ("late", 1, True)])
def test_fin_walk_two_workgroups_of_sixteen_waves(emu_mod, oracle_mod, synth_mod, schedule, dc_rounds, fused):
    """G = 32 of the sixteen-wave build: two workgroups per trace, so that block_sync and grid_meet both order the turn"""
    raw, lens = hover_traces(synth_mod, 7, 16.0, "sin", 1, 0.06, n_rounds=14, B=2, ragged=True, off=0.003)
    refs = oracle_of(oracle_mod, ("wpb16", 32), raw, lens)
    check_walk(emu_mod, refs, raw, lens, dc_rounds=dc_rounds, fused=fused, fin_wpb=16, fin_waves=32, schedule=schedule, seed=5)


@pytest.mark.parametrize("G,B", [(7, 1), (16, 2)])
def test_fin_walk_is_independent_of_the_schedule(emu_mod, oracle_mod, synth_mod, G, B):
    """Every schedule kind, three seeds each (the seed picks the random interleaving, and which half of a trace's workgroups
    is dispatched late): windows, results, scores and the control words byte for byte the same, and never a deadlock"""
    raw, lens = hover_traces(synth_mod, 40 + G, 8.0, "sin", -1, 0.06, n_rounds=14, B=B, ragged=B > 1, off=0.003)
    refs = oracle_of(oracle_mod, ("sched", G, B), raw, lens)
    first = None
    for kind in SCHEDULE_KINDS:
        for seed in (1, 2, 3):
            r = check_walk(emu_mod, refs, raw, lens, dc_rounds=0, fin_wpb=1, fin_waves=G, schedule=kind, seed=seed)
            got = (r["windows"].tobytes(), r["results"].tobytes(), r["scores"].tobytes(), r["stats"].tobytes(), r["ctl"])
            if first is None:
                first = got
            else:
                assert got == first, (kind, seed)


@pytest.mark.parametrize("fused", [False, True], ids=["y-given", "fused-first-pass"])
def test_chain_hand_off_between_workgroups_waits_for_real(emu_mod, oracle_mod, synth_mod, fused):
    """test_emu_ls2.py's traces with 16 slots per chain workgroup, under the random schedule: a chain workgroup's await on the
    flags of the workgroups before it (ls2_chain_prefix) now waits while those run interleaved with it"""
    ts = [synth_mod.make_trace(n_rounds=16, sigma=sigma, seed=200 + k, leak=leak, t1_jitter_raw=4).samples
          for k, (sigma, leak) in enumerate([(0.01, 14.9 * np.exp(0.91j)), (0.03, 3.8 * np.exp(3.4j))])]
    L = min(map(len, ts))
    raw = np.stack([t[:L] for t in ts])
    refs = oracle_of(oracle_mod, ("chain",), raw, None)
    r = emu_mod.ls2_process(raw, chain_slots=16, fused=fused, schedule="random", seed=11)
    for b, (wb, rb, sb) in enumerate(parity.split_by_stream(r["windows"], r["results"], r["scores"], 2)):
        parity.compare_trace(wb, rb, sb, r["stats"][b], refs[b])
    assert r["ok"] == 1 and r["ctl"]["n_pieces"] >= 60, r["ctl"]


def test_chain_and_walk_on_the_hover_trace_under_late_dispatch(emu_mod, oracle_mod, synth_mod):
    """test_emu_ls2.py's hover trace (dc_est across 16.0) with small chain workgroups and the walk alone, the lower half of each
    launch's workgroups dispatched late: the higher ones wait at the chain's flags first"""
    t = synth_mod.make_trace(n_rounds=20, sigma=0.08, seed=9).samples
    refs = oracle_of(oracle_mod, ("hover9",), t[None, :], None)
    check_walk(emu_mod, refs, t[None, :], None, chain_slots=8, dc_rounds=0, fin_wpb=1, fin_waves=5, schedule="late", seed=2)


@pytest.mark.parametrize("schedule", SCHEDULE_KINDS)
def test_deadlock_is_reported_not_hung(emu_mod, schedule):
    """A workgroup that returns before a grid meeting the others wait at: the launch ends with a report naming the kernel and
    where the workgroups stand, and the process goes on"""
    assert emu_mod.grid_meet_selftest(5, 2, leave=False, schedule=schedule, seed=1).sum() == 10
    with pytest.raises(emu_mod.EmuDeadlock, match=r"deadlock in grid_meet_selftest .*at grid_meet"):
        emu_mod.grid_meet_selftest(5, 2, leave=True, schedule=schedule, seed=1)
    assert emu_mod.grid_meet_selftest(3, 1, leave=False, schedule=schedule, seed=2).sum() == 3   # (the emulator is usable after)


@pytest.mark.parametrize("schedule", SCHEDULE_KINDS)
def test_a_workgroup_that_never_ends_is_reported_not_hung(emu_mod, schedule):
    """The last workgroup of each row loops for ever on wave operations while the others wait at the meeting: never all waiting,
    so no deadlock -- the launch ends at the sweep limit with a report naming the workgroup, and the process goes on"""
    old = emu_mod.sweep_limit(20000)
    try:
        with pytest.raises(emu_mod.EmuDeadlock, match=r"no end in grid_meet_selftest .*workgroup \(3,[01]\) took"):
            emu_mod.grid_meet_selftest(4, 2, leave="loop", schedule=schedule, seed=1)
    finally:
        emu_mod.sweep_limit(old)
    assert emu_mod.grid_meet_selftest(4, 2, schedule=schedule, seed=1).sum() == 8


def test_an_earlier_failed_call_does_not_carry_over(emu_mod):
    """a deadlocked call leaves nothing behind: the next call of any entry point runs its launches"""
    with pytest.raises(emu_mod.EmuDeadlock):
        emu_mod.grid_meet_selftest(4, 1, schedule="seq")
    x = np.arange(64, dtype=np.float32)
    chain, _, _ = emu_mod.chain_scan(x, 0.5)
    assert chain[-1] != 0.0


def test_meeting_workgroups_under_the_sequential_schedule_are_a_deadlock(emu_mod):
    """one workgroup at a time (the default): the first waits at the meeting for ever -- a report, not an abort"""
    with pytest.raises(emu_mod.EmuDeadlock, match="grid 4 x 1"):
        emu_mod.grid_meet_selftest(4, 1, schedule="seq")
    assert emu_mod.grid_meet_selftest(1, 1, schedule="seq").sum() == 1

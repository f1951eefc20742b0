"""The tag decoder kernels on the lock-step emulator, on the windows where the reference's comparison operators decide
(tests/decoder_windows.py): tied sync maxima (the first wins; offset 0 when nothing exceeds 0), tied energies (the first
wins), half-bit differences of exactly 0 ("low"), and the pack edges of the batched decoders -- three EPC / four RN16 windows
per wave, a last pack that is not full, RN16 packs drawn eight at a time from a ticket counter.  Everything is compared bit
for bit with oracle.decode_window; the sets' tie counts are asserted from the oracle first."""
import ctypes as C

import numpy as np
import pytest

import decoder_windows as dw
import parity
from rfid import _capi as capi

RN16, EPC = dw.RN16, dw.EPC
EPC_LENGTHS = (0, 1, 2, 3, 4, 7)            # the remainders of a pack of three
RN16_LENGTHS = (0, 1, 3, 4, 5, 33, 70)      # ... of four; 33 and 70: past one draw of 8 packs, past one draw per workgroup


@pytest.fixture(scope="module")
def crafted(oracle_mod):
    return dw.sets(oracle_mod)


def _filled(arr, byte):
    return not (np.frombuffer(arr.tobytes(), dtype=np.uint8) != byte).any()


def _run_lists(emu_mod, crafted, which, n_wg, n_epc, n_rn16, first=0, schedule="seq", seed=0):
    """n_epc + n_rn16 crafted windows (from the first-th on) through emu.decode_lists, every result slot checked: those of
    the listed windows against the oracle, all the others for the prefill pattern"""
    picks = [(EPC, crafted.pick(EPC, first + k)) for k in range(n_epc)] + [(RN16, crafted.pick(RN16, first + k)) for k in range(n_rn16)]
    wmax = 2 * len(picks) + 3
    slots = [2 * k + 1 for k in range(len(picks))]                # (every other slot, and three at the end, belong to no window)
    y, recs = dw.layout([(t, p[0]) for t, p in picks], slots, capi.WINDOW_DTYPE)
    r = emu_mod.decode_lists(y, recs[:n_epc], recs[n_epc:], which=which, n_wg=n_wg, wmax=wmax, schedule=schedule, seed=seed)
    decoded = set()
    for (t, (w, dump, name)), slot in zip(picks, slots):
        if which == emu_mod.DECODE_ALL or which == (emu_mod.DECODE_EPC3 if t == EPC else emu_mod.DECODE_RN16X4):
            what = (name, "type %d" % t, "slot %d" % slot, "lists %d/%d on %d workgroups" % (n_epc, n_rn16, n_wg))
            dw.compare_window(r["results"][slot], r["scores"][slot], dump, what)
            res = r["results"][slot]
            assert r["sum"][slot] == (t | (int(res["crc_ok"]) << 1) | ((int(res["tag_id"]) & 255) << 2)), what
            assert _filled(r["scores"]["pad_"][slot], emu_mod.SCORE_FILL), what
            decoded.add(slot)
    rest = np.array([s not in decoded for s in range(wmax)])
    assert _filled(r["results"][rest], emu_mod.RES_FILL), "a result slot of no listed window was written"
    assert _filled(r["scores"][rest], emu_mod.SCORE_FILL), "a scores slot of no listed window was written"
    assert _filled(r["sum"][rest], emu_mod.SUM_FILL), "a summary slot of no listed window was written"
    if which == emu_mod.DECODE_ALL:
        n_packs = (n_rn16 + 3) // 4
        assert r["tickets"][1] == 0                                # the next launch's counter is zeroed
        assert r["tickets"][0] % 8 == 0 and r["tickets"][0] >= max(8 * n_wg, n_packs)   # every workgroup drew until nothing was left
    else:
        assert r["tickets"].tolist() == [0, 12345]
    return r


def test_crafted_sets_have_their_ties(crafted):
    """(the counts themselves are asserted where the sets are built, from the oracle's scores: decoder_windows.check_*)"""
    for t in (RN16, EPC):
        p = crafted.properties[t]
        print("lattice type %d: %d sync ties > 0, %d energy ties, %d with a zero decision, %d offsets, %d candidates" %
              (t, p["sync_tie"], p["energy_tie"], p["zero_decision"], len(p["offsets"]), len(p["candidates"])))
        assert len(crafted.wins[t]) == 256 + 4 + 15
    # the first-wins rule is visible: a tie whose first and last maximum differ, for both searches
    d = crafted.dumps[EPC]
    assert sum(1 for x in d if x["corr"].max() > 0 and np.ptp(np.flatnonzero(x["corr"] == x["corr"].max())) > 0) >= 20
    assert sum(1 for x in d if np.ptp(np.flatnonzero(x["energy"] == x["energy"].max())) > 0) >= 10


@pytest.mark.parametrize("type_", [RN16, EPC], ids=["rn16", "epc"])
def test_every_crafted_window_through_decode_windows_kernel(emu_mod, crafted, type_):
    """decode_windows_kernel, one window per launch (what rfid_decoder_work runs), via emu.decode_one"""
    for i, (w, dump, name) in enumerate(zip(crafted.wins[type_], crafted.dumps[type_], crafted.names[type_])):
        res, sc = emu_mod.decode_one(w, type_)
        dw.compare_window(res, sc, dump, name)
        if i in crafted.known[type_]:                              # the valid frames: known answers, not only the oracle's
            bits, tag_id = crafted.known[type_][i]
            assert np.array_equal(dw.unpack_bits(res["bits"], len(bits)), bits), name
            assert res["index"] == 65 + int(name[6:])
            if type_ == EPC:
                assert res["crc_ok"] == 1 and res["tag_id"] == tag_id, name


@pytest.mark.parametrize("which,n_wg,schedule", [(0, 5, "random"), (0, 2, "seq"), (1, 2, "seq"), (2, 1, "seq"), (2, 5, "reversed")],
                         ids=["all-5wg-random", "all-2wg", "epc3-2wg", "rn16x4-1wg", "rn16x4-5wg-reversed"])
def test_every_crafted_window_through_the_batched_decoders(emu_mod, crafted, which, n_wg, schedule):
    """all 275 windows of each type in one launch: decode_all_kernel, decode_epc3_kernel and decode_rn16x4_kernel"""
    n = len(crafted.wins[EPC])
    r = _run_lists(emu_mod, crafted, which, n_wg, n if which != 2 else 5, n if which != 1 else 5, schedule=schedule, seed=3)
    if which != 2:                                                 # the valid frames against their known answers
        for i, (bits, tag_id) in crafted.known[EPC].items():
            res = r["results"][2 * i + 1]                          # (the EPC windows come first, in the sets' order)
            assert res["crc_ok"] == 1 and res["tag_id"] == tag_id and np.array_equal(dw.unpack_bits(res["bits"], 128), bits), i


@pytest.mark.parametrize("n_wg", [1, 2, 5])
def test_pack_remainders_of_the_batched_decoders(emu_mod, crafted, n_wg):
    """list lengths around the packs (three EPC, four RN16 windows per wave; eight RN16 packs per ticket draw), empty lists
    (a null list pointer) included, in decode_all_kernel and in the two kernels on their own"""
    pairs = [(0, 0), (1, 1), (2, 3), (3, 4), (4, 5), (7, 33), (0, 70), (7, 0), (1, 70), (3, 33)]
    assert {e for e, _ in pairs} == set(EPC_LENGTHS) and {r for _, r in pairs} == set(RN16_LENGTHS)
    first = 250                                                    # (the last lattice windows, the degenerate ones, the frames, then the first lattice ones)
    for k, (n_epc, n_rn16) in enumerate(pairs):
        _run_lists(emu_mod, crafted, emu_mod.DECODE_ALL, n_wg, n_epc, n_rn16, first=first + k)
        if n_wg > 1:
            _run_lists(emu_mod, crafted, emu_mod.DECODE_ALL, n_wg, n_epc, n_rn16, first=first + k, schedule="random", seed=k)
    for n_epc in EPC_LENGTHS:
        _run_lists(emu_mod, crafted, emu_mod.DECODE_EPC3, n_wg, n_epc, 2, first=first)
    for n_rn16 in RN16_LENGTHS:
        _run_lists(emu_mod, crafted, emu_mod.DECODE_RN16X4, n_wg, 2, n_rn16, first=first)


# ---- a clean trace: its empty and collided slots are constant windows -------------------------------------------------

@pytest.fixture(scope="module")
def clean(oracle_mod, synth_mod):
    return dw.clean_trace(oracle_mod, synth_mod)


@pytest.mark.parametrize("path", ["fused", "unfused", "ls2"])
def test_clean_trace_through_the_batch_paths(emu_mod, clean, path):
    t, o = clean
    if path == "ls2":
        r = emu_mod.ls2_process(t[None, :], fixed_q=2)
    else:
        r = emu_mod.batch_process(t[None, :], fixed_q=2, gate_chunk=-1 if path == "fused" else 0)
    parity.compare_trace(r["windows"], r["results"], r["scores"], r["stats"][0], o)


def test_clean_trace_through_the_streaming_gate_and_decode_one(emu_mod, oracle_mod, clean):
    """gate_scan_kernel in streaming mode hands out the windows, decode_windows_kernel decodes them one by one (the per-call
    path).  The streaming gate reports no start and no dc_est: the gated samples must be the oracle's window, y[start ..] -
    dc_est, bit for bit, which pins both."""
    t, o = clean
    y = oracle_mod.fir(t)
    gs = emu_mod.GateStream()
    windows = np.zeros(o.n_windows, dtype=capi.WINDOW_DTYPE)
    results = np.zeros(o.n_windows, dtype=capi.RESULT_DTYPE)
    scores = np.zeros(o.n_windows, dtype=capi.SCORES_DTYPE)
    pos, seek, typ, k = 0, 0, 0, 0
    pending = np.zeros(0, dtype=np.complex64)
    while pos < len(y) and k < o.n_windows:
        blk = np.ascontiguousarray(y[pos:pos + 1500])
        cons, out, is_open = gs.work(blk, seek_type=seek)
        seek = -1
        pos += cons
        pending = np.concatenate([pending, out])
        if len(pending) == dw.WLEN[typ] and not is_open:
            start, dc = int(o.open_idx[k]), o.dc[k]
            want = np.empty(len(pending), dtype=np.complex64)
            want.real = y[start:start + len(pending)].real - dc.real
            want.imag = y[start:start + len(pending)].imag - dc.imag
            assert np.array_equal(pending.view(np.uint32), want.view(np.uint32)), ("gated samples of window", k)
            windows[k] = (0, k, start, typ, dc.real, dc.imag)
            results[k], scores[k] = emu_mod.decode_one(pending, typ)
            pending = np.zeros(0, dtype=np.complex64)
            k += 1
            typ ^= 1                                               # (the reader ACKs every slot: RN16 and EPC in turn)
            seek = typ
        else:
            assert cons > 0
    assert k == o.n_windows
    parity.compare_trace(windows, results, scores, None, o)


# ---- the streaming matched filter -----------------------------------------------------------------------------------

@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned16", "aligned8"])
def test_streaming_matched_filter(emu_mod, oracle_mod, unaligned):
    """mf_boxcar25_decim5_kernel as rfid_mf_work launches it: the staging buffer starts with the history, output k sums
    staging[in_off + 5 k + 0..24] with in_off 0..4 (the decimation phase the history leaves).  oracle.fir of the same staging
    behind 6 - in_off zeros has that sum at output k + 6 -- the same samples added in the same order."""
    rng = np.random.default_rng(12)
    for n_out in (1, 511, 512, 513):
        for in_off in range(5):
            n = in_off + 5 * n_out + 24 + 3
            staging = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
            got = emu_mod.mf_stream(staging, in_off, n_out, unaligned=unaligned)
            ref = oracle_mod.fir(np.concatenate([np.zeros(6 - in_off, dtype=np.complex64), staging]))[6:6 + n_out]
            assert len(got) == len(ref) == n_out
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (n_out, in_off, unaligned)

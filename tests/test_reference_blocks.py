"""The pin: the CPU oracle (oracle/rfid_oracle.c) against the reference's OWN gate, tag_decoder and reader blocks.

`make -C oracle refblocks` (run by build()) compiles the reference's lib/{gate,tag_decoder,reader}_impl.cc and
global_vars.cc untouched -- Release flags, against the stand-in headers of oracle/refshim -- together with
oracle/ref_blocks.cc, the single-threaded schedule the oracle models, into oracle/_ref/ref_blocks_<variant> (one per
set of the reference's compile-time constants FIXED_Q / MAX_NUM_QUERIES / NUMBER_UNIQUE_TAGS).  These tests run it
on decimated traces (the matched filter stays outside the pin: oracle.fir(raw) is the input, tests/test_fir_boundary.py
bounds the filter) and compare, bit for bit, window by window:

  * every gated sample with the oracle's y[open:open+L] - dc_est, the window starts and types;
  * the decoder's port-0 items (the RN16 bits), the 128 EPC bits it decided, h_est and T_global after each call;
  * reader_state after each window (status words, queries, round, slot, EPCs, tag count) and at the end (tag_reads,
    unique_tags_round, magn_squared_samples);
  * the reader's whole transmit stream, replayed call by call through oracle.ReaderTxSim;
  * the print_results() text (the gate's "| Execution time" line aside).

The GPU tests at the end hold the product (rfid.Context, bin/rfid_reader_offline --host-fir, rfid_reader_work_tx)
against the reference's blocks directly.  Everything here reads only oracle/_ref and tests/golden; the tests skip only
where the binaries are missing and cannot be built (no reference sources)."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
REF_DIR = os.path.join(ORACLE_DIR, "_ref")
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
# variant -> (FIXED_Q, MAX_NUM_QUERIES, NUMBER_UNIQUE_TAGS), as oracle/Makefile builds them
VARIANTS = {"q0": (0, 1000, 100), "q1": (1, 1000, 100), "q4": (4, 1000, 100), "term": (0, 12, 1)}
Q_VARIANT = {0: "q0", 1: "q1", 4: "q4"}
# gen2_logic_status (include/rfid/global_vars.h:32)
SEND_QUERY, SEND_ACK, SEND_QUERY_REP, IDLE, SEND_CW, START, SEND_QUERY_ADJUST, SEND_NAK_QR, SEND_NAK_Q, POWER_DOWN = range(10)
# windows.i32 record layout (oracle/ref_blocks.cc, WIN_*)
W_GATED, W_OPEN, W_TYPE, W_CONSUMED, W_NOUT0, W_BITS = 0, 1, 2, 3, 4, 5
W_STATE = 21   # status, gen2, gate, decoder, n_queries_sent, round, slot, n_epc_correct, tag_reads.size()
W_H, W_T, W_EPC = 30, 32, 33
STATE_FIELDS = ("status", "gen2_logic_status", "gate_status", "decoder_status", "n_queries_sent",
                "cur_inventory_round", "cur_slot_number", "n_epc_correct", "n_unique_tags")


def _exe(variant):
    return os.path.join(REF_DIR, "ref_blocks_" + variant)


@pytest.fixture(scope="module")
def ref_bins():
    """The binaries build() made; where they are missing, the recipe is asked once more (it builds them where the
    reference's sources are, and does nothing where they are not)."""
    if not all(os.path.isfile(_exe(v)) for v in VARIANTS):
        subprocess.run(["make", "-C", ORACLE_DIR, "refblocks"], capture_output=True, text=True, timeout=900)
    if not all(os.path.isfile(_exe(v)) for v in VARIANTS):
        pytest.skip("oracle/_ref/ref_blocks_* are missing and the reference's sources are not here to build them")
    return {v: _exe(v) for v in VARIANTS}


class RefRun:
    def __init__(self, d, stdout):
        self.res = json.load(open(os.path.join(d, "result.json")))
        self.gated = np.fromfile(os.path.join(d, "gated.c64"), dtype=np.complex64)
        self.tx = np.fromfile(os.path.join(d, "tx.f32"), dtype=np.float32)
        self.magn = np.fromfile(os.path.join(d, "magn.f32"), dtype=np.float32)
        self.win = np.fromfile(os.path.join(d, "windows.i32"), dtype=np.int32).reshape(-1, self.res["win_fields"])
        self.calls = np.fromfile(os.path.join(d, "reader.i32"), dtype=np.int32).reshape(-1, 4)
        self.stdout = stdout

    def report(self):
        """print_results() as printed, without the gate's timing line (gate_impl.cc:107)"""
        return "".join(l for l in self.stdout.splitlines(True) if not l.startswith("| Execution time"))


def run_ref(tmp_path, variant, y=None, chunk=4096, dac_rate=1000000, state=None, bits=None, tag="run"):
    """One driver process per run: the reference keeps its state in a global (global_vars.cc:31)."""
    d = tmp_path / f"{tag}_{variant}_{chunk}_{dac_rate}_{state}"
    d.mkdir()
    cmd = [_exe(variant), "--out", str(d), "--dac-rate", str(dac_rate)]
    if state is None:
        np.ascontiguousarray(y, dtype=np.complex64).tofile(str(d / "y.c64"))
        cmd += ["--in", str(d / "y.c64"), "--chunk", str(chunk)]
    else:
        cmd += ["--state", str(state)] + (["--bits", "".join(str(int(b)) for b in bits)] if bits is not None else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return RefRun(str(d), out.stdout)


def oracle_window_states(oracle_mod, cfg, y, ref):
    """reader_state after each of the reference's windows, from the oracle: its resumable harness fed up to the
    sample that closes that window (feeding in pieces is the same as one run, orc_stream_feed)."""
    s = oracle_mod.Stream(cfg, chunk=4096)
    pos, snaps = 0, []
    for open_idx, consumed in zip(ref.win[:, W_OPEN], ref.win[:, W_CONSUMED]):
        end = int(open_idx) + int(consumed)
        s.feed_decimated(y[pos:end], keep=False)
        pos = end
        st = s.result().state
        snaps.append([getattr(st, f) for f in STATE_FIELDS])
    s.close()
    return np.array(snaps, dtype=np.int64).reshape(-1, len(STATE_FIELDS))


def replay_tx(oracle_mod, cfg, ref, dac_rate):
    """The reader's transmit stream call by call: the oracle's reader (orc_reader_work_tx) started in the state the
    reference's reader was in, fed what the reference's reader was fed (its queue: the decoder's port-0 items)."""
    sim = oracle_mod.ReaderTxSim(dac_rate=dac_rate, cfg=cfg)
    port0 = np.concatenate([ref.win[k, W_BITS:W_BITS + ref.win[k, W_NOUT0]] for k in range(len(ref.win))] +
                           [np.zeros(0, np.int32)]).astype(np.float32)
    t = p = 0
    for before, nin, written, after in ref.calls:
        sim.state.gen2_logic_status = int(before)
        got = sim.work(port0[p:p + nin] if nin else None)
        p += nin
        assert np.array_equal(got.view(np.uint32), ref.tx[t:t + written].view(np.uint32)), ("tx", before, nin, t)
        assert sim.state.gen2_logic_status == after
        t += written
    assert t == len(ref.tx) and p == len(port0)


def compare_with_oracle(oracle_mod, y, ref, cfg, dac_rate=1000000, tx=True):
    y = np.ascontiguousarray(y, dtype=np.complex64)
    o = oracle_mod.run_decimated(y, cfg, max_dumps=max(16, len(y) // 100))
    n = len(ref.win)
    # windows: how many, where, which kind
    assert n == o.n_windows
    assert np.array_equal(ref.win[:, W_OPEN], o.open_idx)
    assert np.array_equal(ref.win[:, W_TYPE], o.dumps["type"])
    assert np.array_equal(ref.win[:, W_GATED], np.concatenate([[0], np.cumsum(ref.win[:, W_CONSUMED])[:-1]])[:n])
    # every gated sample: in[i] - dc_est (gate_impl.cc:176,187), the window consumed whole; what follows the last
    # consumed window is a window the trace cut short
    want = [(y[s:s + L] - np.complex64(dc)).astype(np.complex64)
            for s, L, dc in zip(o.open_idx, ref.win[:, W_CONSUMED], o.dc)]
    want = np.concatenate(want) if want else np.zeros(0, np.complex64)
    assert len(ref.gated) >= len(want) and len(ref.gated) - len(want) < 1370
    assert np.array_equal(ref.gated[:len(want)].view(np.uint32), want.view(np.uint32))
    assert all(len(w) == L for w, L in zip(np.split(want, np.cumsum(ref.win[:, W_CONSUMED])[:-1]), ref.win[:, W_CONSUMED]))
    # per window: what the decoder emitted and estimated
    for k in range(n):
        d = o.dumps[k]
        if d["type"] == 0:
            assert ref.win[k, W_NOUT0] == 16 == d["n_bits"]
            assert np.array_equal(ref.win[k, W_BITS:W_BITS + 16], d["bits"][:16]), k
        else:
            assert ref.win[k, W_NOUT0] == 0 and d["n_bits"] == 128
            assert np.array_equal(ref.win[k, W_T:W_T + 1].view(np.float32), np.array([d["T"]], np.float32)), k
            epc = np.unpackbits(ref.win[k, W_EPC:W_EPC + 4].astype(">u4").view(np.uint8))
            assert np.array_equal(epc, d["bits"][:128]), k
        assert np.array_equal(ref.win[k, W_H:W_H + 2].view(np.uint32), np.asarray(d["h_est"], np.float32).view(np.uint32)), k
    # reader_state after each window, then at the end
    if n:
        assert np.array_equal(ref.win[:, W_STATE:W_STATE + 9], oracle_window_states(oracle_mod, cfg, y, ref))
    s, r = o.state, ref.res
    assert (r["status"], r["gen2_logic_status"], r["gate_status"], r["decoder_status"]) == \
        (s.status, s.gen2_logic_status, s.gate_status, s.decoder_status)
    assert (r["n_queries_sent"], r["cur_inventory_round"], r["cur_slot_number"], r["max_slot_number"], r["n_epc_correct"]) == \
        (s.n_queries_sent, s.cur_inventory_round, s.cur_slot_number, s.max_slot_number, s.n_epc_correct)
    assert {int(k): v for k, v in r["tag_reads"].items()} == {i: s.tag_reads[i] for i in range(256) if s.tag_reads[i]}
    assert r["unique_tags_round"] == list(s.unique_tags_round[:s.n_rounds_logged])
    assert np.array_equal(ref.magn.view(np.uint32), np.array(s.magn_squared[:s.n_magn], np.float32).view(np.uint32))
    assert ref.report() == o.print_results()
    if tx:
        replay_tx(oracle_mod, cfg, ref, dac_rate)
    return o


def _cfg(oracle_mod, variant):
    q, m, u = VARIANTS[variant]
    return oracle_mod.config(fixed_q=q, max_num_queries=m, number_unique_tags=u)


# ---- the committed fixtures, each with the variant of its FIXED_Q --------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_golden_fixture_against_reference_blocks(tmp_path, ref_bins, oracle_mod, path):
    g = np.load(path)
    v = Q_VARIANT[int(g["fixed_q"])]
    y = oracle_mod.fir(g["raw"])
    ref = run_ref(tmp_path, v, y)
    o = compare_with_oracle(oracle_mod, y, ref, _cfg(oracle_mod, v))
    # ... and the fixture's own frozen arrays are the reference's
    assert np.array_equal(g["open_idx"], ref.win[:, W_OPEN]) and np.array_equal(g["type"], ref.win[:, W_TYPE])
    assert np.array_equal(g["print_results"].tobytes().decode(), ref.report())
    assert o.n_windows == len(g["type"])


# ---- synthetic traces: noise levels, Q, collisions, CRC failures, jitter, cuts, the carrier leak, extreme scales -----
SYNTH = {
    "s0p002_q0": (dict(n_rounds=3, sigma=0.002, seed=301), "q0"),
    "s0p03_q0_jitter": (dict(n_rounds=3, sigma=0.03, seed=302, t1_jitter_raw=7, tail_us=350), "q0"),
    "s0p06_q0_tail120": (dict(n_rounds=3, sigma=0.06, seed=303, tail_us=120), "q0"),
    "s0p002_q1_three_tags": (dict(n_rounds=4, fixed_q=1, tag_ids=(0x11, 0x22, 0x33), sigma=0.002, seed=304), "q1"),
    "s0p03_q1_two_tags_crc": (dict(n_rounds=4, fixed_q=1, tag_ids=(0x3C, 0xA5), sigma=0.03, seed=305,
                                   corrupt_rounds=(2, 3)), "q1"),
    "s0p03_q4_three_tags": (dict(n_rounds=2, fixed_q=4, tag_ids=(0x01, 0x80, 0xFE), sigma=0.03, seed=306,
                                 t1_jitter_raw=3), "q4"),
    "s0p06_q4_two_tags_jitter": (dict(n_rounds=1, fixed_q=4, tag_ids=(0x42, 0x43), sigma=0.06, seed=307,
                                      t1_jitter_raw=9, tail_us=500), "q4"),
    "s0p002_q0_crc": (dict(n_rounds=4, sigma=0.002, seed=308, corrupt_rounds=(1, 4)), "q0"),
    # carrier leak 25 e^{j0.7}: dc_est's imaginary part sits at 16.1, across the binade edge at 16 (README configs[2], [3])
    "s0p06_q0_leak25": (dict(n_rounds=4, sigma=0.06, seed=309, leak=25 * np.exp(0.7j)), "q0"),
    # low SNR: EPC bits decided on small margins, so every sampling position shows in the bits and CRC outcomes
    "s0p25_q1_two_tags": (dict(n_rounds=6, fixed_q=1, tag_ids=(0x5A, 0xC3), sigma=0.25, seed=311, t1_jitter_raw=2), "q1"),
    "s0p4_q0": (dict(n_rounds=8, sigma=0.4, seed=312), "q0"),
    "s0p06_q4_leak25": (dict(n_rounds=1, fixed_q=4, tag_ids=(0x27, 0x28, 0x29), sigma=0.06, seed=310,
                             leak=25 * np.exp(0.7j), t1_jitter_raw=5), "q4"),
}


@pytest.fixture(scope="module")
def synth_traces(synth_mod, oracle_mod):
    return {k: oracle_mod.fir(synth_mod.make_trace(**kw).samples) for k, (kw, _) in SYNTH.items()}


@pytest.mark.parametrize("case", list(SYNTH))
def test_synthetic_trace_against_reference_blocks(tmp_path, ref_bins, oracle_mod, synth_traces, case):
    v = SYNTH[case][1]
    y = synth_traces[case]
    o = compare_with_oracle(oracle_mod, y, run_ref(tmp_path, v, y), _cfg(oracle_mod, v))
    assert o.n_windows >= 2


@pytest.mark.parametrize("frac", [0.31, 0.5, 0.83, 0.97])
def test_trace_cut_mid_window(tmp_path, ref_bins, oracle_mod, synth_traces, frac):
    """A trace that ends inside a window: the window is gated but never decoded, on both sides."""
    y = synth_traces["s0p002_q0"]
    y = y[: int(len(y) * frac)]
    compare_with_oracle(oracle_mod, y, run_ref(tmp_path, "q0", y), _cfg(oracle_mod, "q0"))


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-36, 3e-39, 1e15, 1e18, 0.0])
def test_extreme_amplitudes(tmp_path, ref_bins, oracle_mod, synth_mod, scale):
    """The scales of test_gpu_parity.py::test_extreme_amplitudes_match_oracle: denormal products and increments,
    energies overflowing to +inf, an all-zero trace."""
    t = synth_mod.make_trace(n_rounds=3, seed=5, sigma=0.01).samples
    y = oracle_mod.fir((t * np.float32(scale)).astype(np.complex64))
    compare_with_oracle(oracle_mod, y, run_ref(tmp_path, "q0", y), _cfg(oracle_mod, "q0"))


@pytest.mark.parametrize("n", [0, 1, 2, 7, 250, 1370])
def test_empty_and_tiny_inputs(tmp_path, ref_bins, oracle_mod, n):
    rng = np.random.default_rng(n)
    y = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    ref = run_ref(tmp_path, "q0", y)
    compare_with_oracle(oracle_mod, y, ref, _cfg(oracle_mod, "q0"))
    # START carrier and the first Query go out before the gate sees a sample (reader_impl.cc:218-288)
    assert [tuple(c[[0, 3]]) for c in ref.calls] == [(START, SEND_QUERY), (SEND_QUERY, IDLE)]


@pytest.mark.parametrize("chunk", [1, 7, 250, 1370, 4096, 0])
@pytest.mark.parametrize("case", ["s0p03_q0_jitter", "s0p03_q4_three_tags"])
def test_reference_is_chunk_invariant(tmp_path, ref_bins, oracle_mod, synth_traces, case, chunk):
    """The gate breaks at every window close and checks termination / SEEK states only at the top of a call, and the
    decoder only acts once a whole window is queued, so under this schedule any chunking (0 = the whole trace in one
    call) gives the oracle's results -- run at its default chunking."""
    v = SYNTH[case][1]
    y = synth_traces[case]
    compare_with_oracle(oracle_mod, y, run_ref(tmp_path, v, y, chunk=chunk), _cfg(oracle_mod, v))


# ---- termination: MAX_NUM_QUERIES 12, NUMBER_UNIQUE_TAGS 1 ---------------------------------------------------------
def test_termination_by_query_count(tmp_path, ref_bins, oracle_mod, synth_mod):
    y = oracle_mod.fir(synth_mod.make_trace(n_rounds=16, sigma=0.01, seed=320).samples)
    ref = run_ref(tmp_path, "term", y)
    assert ref.res["status"] == 1 and "| Execution time" in ref.stdout
    o = compare_with_oracle(oracle_mod, y, ref, oracle_mod.config(max_num_queries=12, number_unique_tags=1))
    assert o.state.n_queries_sent == 13


@pytest.mark.parametrize("chunk", [1, 4096])
def test_termination_by_unique_tags(tmp_path, ref_bins, oracle_mod, synth_mod, chunk):
    """Three one-tag traces back to back, each its own tag: the second distinct tag ends the run (tag_reads.size() > 1)."""
    raw = np.concatenate([synth_mod.make_trace(n_rounds=2, tag_ids=(tid,), sigma=0.01, seed=321 + k).samples
                          for k, tid in enumerate((0x10, 0x20, 0x30))])
    y = oracle_mod.fir(raw)
    ref = run_ref(tmp_path, "term", y, chunk=chunk)
    assert ref.res["status"] == 1 and len(ref.res["tag_reads"]) == 2
    compare_with_oracle(oracle_mod, y, ref, oracle_mod.config(max_num_queries=12, number_unique_tags=1))


# ---- the reader's transmit stream, state by state (--state) and over whole traces at other DAC rates ---------------
RN16 = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1]


@pytest.mark.parametrize("dac", [1000000, 2000000, 800000])
def test_reader_every_state(tmp_path, ref_bins, oracle_mod, dac):
    """Every gen2_logic_status, POWER_DOWN / SEND_NAK_QR / SEND_NAK_Q / SEND_QUERY_ADJUST / SEND_CW among them (no trace
    reaches those), at 1 MHz, 2 MHz and 800 kHz (non-integer sample counts, reader_impl.h:35), for every FIXED_Q
    variant (the Query carries Q and its CRC-5)."""
    for v in ("q0", "q1", "q4"):
        cfg = _cfg(oracle_mod, v)
        for state in range(10):
            for bits in ([None, RN16, RN16[:15]] if state == SEND_ACK else [None]):
                ref = run_ref(tmp_path, v, dac_rate=dac, state=state, bits=bits, tag=f"b{0 if bits is None else len(bits)}")
                sim = oracle_mod.ReaderTxSim(dac_rate=dac, cfg=cfg)
                sim.state.gen2_logic_status = state
                want = sim.work(np.array(bits, np.float32) if bits is not None else None)
                assert np.array_equal(ref.tx.view(np.uint32), want.view(np.uint32)), (v, state, dac)
                r, s = ref.res, sim.state
                assert (r["gen2_logic_status"], r["gate_status"], r["decoder_status"], r["n_queries_sent"]) == \
                    (s.gen2_logic_status, s.gate_status, s.decoder_status, s.n_queries_sent), (v, state, dac)
                if state in (START, SEND_QUERY, SEND_CW, POWER_DOWN, SEND_NAK_Q) or (state == SEND_ACK and bits == RN16):
                    assert len(ref.tx) > 0


@pytest.mark.parametrize("dac", [2000000, 800000])
def test_reader_tx_stream_over_a_trace(tmp_path, ref_bins, oracle_mod, synth_traces, dac):
    y = synth_traces["s0p002_q1_three_tags"]
    ref = run_ref(tmp_path, "q1", y, dac_rate=dac)
    compare_with_oracle(oracle_mod, y, ref, _cfg(oracle_mod, "q1"), dac_rate=dac)
    assert len(ref.tx) > 10 * dac // 1000


# ---- GPU: the product against the reference's blocks directly ------------------------------------------------------
def _gpu_cases(synth_mod):
    cases = []
    for p in FIXTURES:
        g = np.load(p)
        cases.append((os.path.basename(p)[:-4], g["raw"].astype(np.complex64), Q_VARIANT[int(g["fixed_q"])]))
    for k in ("s0p03_q0_jitter", "s0p03_q1_two_tags_crc", "s0p03_q4_three_tags", "s0p06_q0_leak25"):
        kw, v = SYNTH[k]
        cases.append((k, synth_mod.make_trace(**kw).samples.astype(np.complex64), v))
    return cases


@pytest.mark.gpu
def test_gpu_batch_against_reference_blocks(tmp_path, ref_bins, oracle_mod, synth_mod):
    """rfid.Context's batched path, one batch per FIXED_Q: window starts / types / dc, bits, h_est, T, CRC and the
    statistics equal what the reference's blocks did on the same (host-filtered) trace."""
    import torch
    import rfid
    by_q = {}
    for name, raw, v in _gpu_cases(synth_mod):
        by_q.setdefault(v, []).append((name, raw))
    for v, items in by_q.items():
        q = VARIANTS[v][0]
        refs = [run_ref(tmp_path, v, oracle_mod.fir(raw), tag=name) for name, raw in items]
        L = max(len(raw) for _, raw in items)
        stride = (L + 1) & ~1
        host = np.zeros((len(items), stride), dtype=np.complex64)
        for b, (_, raw) in enumerate(items):
            host[b, :len(raw)] = raw
        lens = torch.tensor(np.array([len(raw) for _, raw in items], dtype=np.int64)).to("cuda:0")
        dev = torch.from_numpy(host.view(np.float32)).to("cuda:0")
        ctx = rfid.Context(device=0, fixed_q=q)
        try:
            ctx.batch_plan(len(items), L)
            ctx.batch_process_ptr(dev.data_ptr(), stride, L, lens.data_ptr(), want_scores=False)
            ctx.batch_sync()
            w, r, _ = ctx.batch_windows(want_scores=False)
            st = ctx.batch_stats()
        finally:
            ctx.close()
        for b, ((name, raw), ref) in enumerate(zip(items, refs)):
            sel = w["stream"] == b
            wb, rb = w[sel], r[sel]
            n = len(ref.win)
            assert st[b]["n_windows"] == n and len(wb) >= n, name
            assert np.array_equal(wb["start"][:n], ref.win[:, W_OPEN]), name
            assert np.array_equal(wb["type"][:n], ref.win[:, W_TYPE]), name
            h = np.stack([rb["h_re"][:n], rb["h_im"][:n]], axis=1).astype(np.float32)
            assert np.array_equal(h.view(np.uint32), ref.win[:, W_H:W_H + 2].view(np.uint32)), name
            y = oracle_mod.fir(raw)
            gated = np.concatenate([y[s:s + c] - np.complex64(complex(dr, di)) for s, c, dr, di in
                                    zip(wb["start"][:n], ref.win[:, W_CONSUMED], wb["dc_re"][:n], wb["dc_im"][:n])] +
                                   [np.zeros(0, np.complex64)]).astype(np.complex64)
            assert np.array_equal(gated.view(np.uint32), ref.gated[:len(gated)].view(np.uint32)), name
            for k in range(n):
                if ref.win[k, W_TYPE] == 0:
                    bits = rfid.unpack_bits(rb["bits"][k], int(rb["n_bits"][k]))
                    assert np.array_equal(bits, ref.win[k, W_BITS:W_BITS + 16]), (name, k)
                else:
                    assert np.float32(rb["T"][k]).view(np.uint32) == ref.win[k, W_T].view(np.uint32), (name, k)
            s = st[b]
            assert (s["n_queries_sent"], s["cur_inventory_round"], s["cur_slot_number"], s["n_epc_correct"],
                    s["n_unique_tags"], s["status"]) == \
                (ref.res["n_queries_sent"], ref.res["cur_inventory_round"], ref.res["cur_slot_number"],
                 ref.res["n_epc_correct"], len(ref.res["tag_reads"]), ref.res["status"]), name
            assert {i: int(c) for i, c in enumerate(s["tag_reads"]) if c} == \
                {int(k): c for k, c in ref.res["tag_reads"].items()}, name


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["q1_two_tags", "s0p03_q4_three_tags", "term_queries"])
def test_gpu_offline_binary_against_reference_blocks(tmp_path, ref_bins, oracle_mod, synth_mod, case):
    """bin/rfid_reader_offline --host-fir (gate, tag_decoder and reader made, fed a k-ascending host filter like
    oracle.fir): its report, gated samples and reader output are the reference blocks' byte for byte."""
    import rfid
    if case == "q1_two_tags":
        raw, v = np.load(os.path.join(ROOT, "tests", "golden", "q1_two_tags.npz"))["raw"], "q1"
    elif case == "term_queries":
        raw, v = synth_mod.make_trace(n_rounds=16, sigma=0.01, seed=320).samples, "term"
    else:
        kw, v = SYNTH[case]
        raw = synth_mod.make_trace(**kw).samples
    raw = raw.astype(np.complex64)
    q, m, u = VARIANTS[v]
    ref = run_ref(tmp_path, v, oracle_mod.fir(raw))
    exe = os.path.join(rfid.capi.PKG_ROOT, "bin", "rfid_reader_offline")
    path, gp, tp = tmp_path / "t.bin", tmp_path / "gate.c64", tmp_path / "tx.f32"
    rfid.batch.write_trace_file(str(path), raw)
    out = subprocess.run([exe, str(path), "--host-fir", "--fixed-q", str(q), "--max-queries", str(m), "--unique-tags", str(u),
                          "--gate-out", str(gp), "--tx-out", str(tp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    report = "".join(l for l in out.stdout.splitlines(True) if not l.startswith("| Execution time"))
    assert report.startswith(ref.report()), out.stdout[-800:]
    assert np.fromfile(str(gp), dtype=np.complex64).tobytes() == ref.gated.tobytes()
    assert np.fromfile(str(tp), dtype=np.float32).tobytes() == ref.tx.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dac", [1000000, 2000000, 800000])
def test_gpu_reader_work_tx_against_reference_reader(tmp_path, ref_bins, dac):
    """rfid_reader_work_tx from every gen2_logic_status the C-ABI can be walked into, against the reference's reader
    (--state): START, SEND_QUERY, IDLE, SEND_ACK (with and without 16 bits), SEND_CW, SEND_QUERY_REP via a trace-free
    walk, for each FIXED_Q variant."""
    import rfid
    for v in ("q0", "q1", "q4"):
        ctx = rfid.Context(device=0, fixed_q=VARIANTS[v][0])
        try:
            for state, bits in ((START, None), (SEND_QUERY, None), (IDLE, None)):
                assert ctx.state().gen2_logic_status == state
                _, got = ctx.reader_work_tx(None if bits is None else np.array(bits, np.float32), dac_rate=dac)
                ref = run_ref(tmp_path, v, dac_rate=dac, state=state, tag="gpu")
                assert got.tobytes() == ref.tx.tobytes(), (v, state, dac)
                assert ctx.state().gen2_logic_status == ref.res["gen2_logic_status"]
        finally:
            ctx.close()

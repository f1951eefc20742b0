"""Pins for the CPU oracle (oracle/rfid_oracle.c).  The reference ships no golden vectors for
this path; besides the bit-for-bit comparison with the reference's own blocks
(tests/test_reference_blocks.py, see oracle/rfid_oracle.h) the oracle is anchored on: published constants, the generator's ground truth, the README's
known-answer shape, self-consistency across scheduler chunk sizes, and committed fixtures."""
import ctypes as C

import numpy as np
import pytest


def test_crc16_published_check_value(oracle_mod):
    # CRC-16/GENIBUS (poly 0x1021, init 0xFFFF, xorout 0xFFFF, no reflection) check("123456789") = 0xD64E;
    # this is the EPC Gen2 CRC-16 that check_crc implements (tag_decoder_impl.cc:401-445)
    assert oracle_mod.lib().orc_crc16_bytes(b"123456789", 9) == 0xD64E


def test_check_crc_accepts_valid_and_rejects_flipped_frames(oracle_mod, synth_mod):
    frame = synth_mod.epc_frame(synth_mod.epc_for_id(0x27))
    s = "".join("1" if b else "0" for b in frame).encode()
    assert oracle_mod.lib().orc_check_crc(s, 128) == 1
    for pos in (0, 17, 111, 112, 127):
        f = list(frame)
        f[pos] ^= 1
        assert oracle_mod.lib().orc_check_crc("".join("1" if b else "0" for b in f).encode(), 128) == -1


def test_half_period_candidates_match_baseline_md(oracle_mod, synth_mod):
    # BASELINE.md section 5 lists the 20 float32 candidates of tag_decoder_impl.cc:151-166
    expected = [4.94999981, 4.95526314, 4.96052599, 4.96578932, 4.97105265, 4.97631550, 4.98157883, 4.98684216,
                4.99210501, 4.99736834, 5.00263166, 5.00789499, 5.01315784, 5.01842117, 5.02368450, 5.02894735,
                5.03421068, 5.03947401, 5.04473686, 5.05000019]
    mn, mx = np.float32(10.0 / 2.0 - 10.0 / 2.0 / 100), np.float32(10.0 / 2.0 + 10.0 / 2.0 / 100)
    cand = [np.float32(mn + np.float32(np.float32(t) * np.float32(mx - mn)) / np.float32(19)) for t in range(20)]
    assert np.allclose(cand, expected, rtol=0, atol=5e-8)
    # every T the oracle reports is one of them
    o = oracle_mod.run_trace(synth_mod.make_trace(n_rounds=3, seed=3).samples)
    for d in o.dumps[o.dumps["type"] == 1]:
        assert any(d["T"] == c for c in cand)


@pytest.mark.parametrize("sigma", [0.002, 0.03, 0.06])
def test_oracle_decodes_generator_truth(oracle_mod, synth_mod, sigma):
    t = synth_mod.make_trace(n_rounds=6, sigma=sigma, seed=int(sigma * 1000) + 5, t1_jitter_raw=8)
    o = oracle_mod.run_trace(t.samples)
    assert o.n_windows == 2 * len(t.slots)
    for k, s in enumerate(t.slots):
        assert list(o.dumps[2 * k]["bits"][:16]) == s.rn16
        assert list(o.dumps[2 * k + 1]["bits"]) == s.epc and o.dumps[2 * k + 1]["crc_ok"] == 1
        assert o.dumps[2 * k + 1]["tag_id"] == 0x27
    assert o.state.n_epc_correct == 6 and o.state.n_queries_sent == 7


def test_readme_known_answer_shape(oracle_mod, synth_mod):
    # README.md:48-53 on the stand-in for the missing misc/data/file_source_test
    o = oracle_mod.run_trace(synth_mod.fst_like_trace().samples)
    assert o.print_results() == ("\n --------------------------\n"
                                 "| Number of queries/queryreps sent : 71\n"
                                 "| Current Inventory round : 72\n"
                                 " --------------------------\n"
                                 "| Correctly decoded EPC : 70\n"
                                 "| Number of unique tags : 1\n"
                                 "| Tag ID : 27  Num of reads : 70\n"
                                 " --------------------------\n")


def test_scheduler_chunk_invariance(oracle_mod, synth_mod):
    t = synth_mod.make_trace(n_rounds=4, sigma=0.02, seed=9).samples
    ref = oracle_mod.run_trace(t, chunk=4096)
    for chunk in (1, 63, 512, 777, 1500, 8191):
        o = oracle_mod.run_trace(t, chunk=chunk)
        assert o.stats() == ref.stats()
        assert np.array_equal(o.dumps, ref.dumps) and np.array_equal(o.open_idx, ref.open_idx)
        assert np.array_equal(o.dc.view(np.uint32), ref.dc.view(np.uint32))


def test_streaming_fir_equals_batch_fir(oracle_mod, synth_mod):
    x = synth_mod.make_trace(n_rounds=1, seed=2).samples[:5003]
    L = oracle_mod.lib()
    L.orc_fir_stream.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.orc_fir_stream.restype = C.c_long
    hist = np.zeros(24, dtype=np.complex64)
    phase = C.c_int(0)
    out = []
    pos = 0
    for n in (1, 4, 5, 23, 24, 25, 1000, 3921):
        blk = np.ascontiguousarray(x[pos:pos + n])
        y = np.zeros(n // 5 + 2, dtype=np.complex64)
        k = L.orc_fir_stream(blk.ctypes.data, len(blk), y.ctypes.data, hist.ctypes.data, C.byref(phase))
        out.append(y[:k])
        pos += n
    got = np.concatenate(out)
    ref = oracle_mod.fir(x[:pos])
    assert np.array_equal(got[: len(ref)].view(np.uint32), ref.view(np.uint32))


def test_fixed_q_rounds_and_termination(oracle_mod, synth_mod):
    t = synth_mod.make_trace(n_rounds=3, fixed_q=2, tag_ids=(1, 2, 3), seed=4).samples
    o = oracle_mod.run_trace(t, oracle_mod.config(fixed_q=2))
    assert o.n_windows == 2 * 12 and o.state.cur_inventory_round == 4 and o.state.n_queries_sent == 13
    o2 = oracle_mod.run_trace(t, oracle_mod.config(fixed_q=2, max_num_queries=5))
    assert o2.state.status == 1 and o2.state.n_queries_sent == 6   # TERMINATED after the 6th query


def test_empty_and_tiny_inputs(oracle_mod):
    for n in (0, 1, 4, 5, 24):
        o = oracle_mod.run_trace(np.zeros(n, dtype=np.complex64))
        assert o.n_windows == 0 and o.state.n_queries_sent == 1


def test_multi_thread_timing_leg_decodes_the_same(oracle_mod, synth_mod):
    """bench.py's cpu_baseline leg on all host cores: every thread runs the single-thread chain on its own
    copy; the decode counts equal the single-thread run's."""
    t = synth_mod.make_trace(n_rounds=3, seed=4, sigma=0.01).samples
    one = oracle_mod.time_trace(t, reps=2)
    many = oracle_mod.time_trace_mt(t, reps=2, nthreads=3)
    assert many["windows"] == one["windows"] and many["n_epc_correct"] == one["n_epc_correct"]
    assert many["wall_s"] > 0.0


def test_reader_tx_waveforms_match_the_trace_generator(oracle_mod, synth_mod):
    """orc_reader_work_tx (restating reader_impl.cc:43-129,200-380,383-443) against rfid/synth.py, which was
    written separately to build the test traces: START carrier, Query (preamble + 22 PIE bits incl. CRC-5 for
    every Q) + 1295 us CW, ACK (frame sync + 01 + RN16), the 4575 us CW after it, QueryRep."""
    for q in range(16):
        sim = oracle_mod.ReaderTxSim(cfg=oracle_mod.config(fixed_q=q))
        assert sim.state.gen2_logic_status == 5                                   # START
        w = sim.work()
        assert len(w) == synth_mod.CW_ACK and (w == 1).all()                      # :218-224
        w = sim.work()                                                            # SEND_QUERY
        want = np.concatenate([synth_mod.query_cmd(q), np.ones(synth_mod.CW_QUERY, np.float32)])
        assert np.array_equal(w, want), q
        assert sim.state.gen2_logic_status == 3 and sim.state.n_queries_sent == 1  # IDLE
    sim = oracle_mod.ReaderTxSim()
    sim.work(); sim.work()
    assert len(sim.work()) == 0                                                   # IDLE writes nothing
    rn16 = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1]
    sim.state.gen2_logic_status = 1                                               # SEND_ACK (set by the decoder)
    assert len(sim.work(rn16[:5])) == 0 and sim.state.gen2_logic_status == 1      # needs exactly 16 items (:293)
    w = sim.work(rn16)
    assert np.array_equal(w, synth_mod.ack_cmd(rn16)) and sim.state.gen2_logic_status == 4   # SEND_CW
    w = sim.work()
    assert len(w) == synth_mod.CW_ACK and (w == 1).all() and sim.state.gen2_logic_status == 3
    sim.state.gen2_logic_status = 2                                               # SEND_QUERY_REP
    w = sim.work()
    assert np.array_equal(w, np.concatenate([synth_mod.query_rep_cmd(), np.ones(synth_mod.CW_QUERY, np.float32)]))
    assert sim.state.n_queries_sent == 2
    sim.state.gen2_logic_status = 7                                               # SEND_NAK_QR -> QueryRep next
    w = sim.work()
    nak = np.concatenate([synth_mod._FRAME_SYNC, synth_mod.pie([1, 1, 0, 0, 0, 0, 0, 0]), np.ones(250, np.float32)])
    assert np.array_equal(w, nak) and sim.state.gen2_logic_status == 2
    # a 2 MHz DAC doubles every duration
    sim2 = oracle_mod.ReaderTxSim(dac_rate=2000000)
    assert len(sim2.work()) == 2 * synth_mod.CW_ACK
    assert np.array_equal(sim2.work(), np.repeat(np.concatenate([synth_mod.query_cmd(0), np.ones(synth_mod.CW_QUERY, np.float32)]), 2))


def test_reader_tx_non_integer_sample_duration(oracle_mod):
    """dac_rate = 800 kHz (sample_d = 1.25 us): the reference keeps n_data0_s ... n_trcal_s as float members
    (reader_impl.h:35) and truncates at each use -- rtcal.resize(19.2f + 38.4f) = 57 samples,
    fill_n(57 - 9.6f) = 47 ones, not (19 + 38) - 9 = 48 (reader_impl.cc:84-96)."""
    sim = oracle_mod.ReaderTxSim(dac_rate=800000)
    tx = sim.tx
    assert (tx.n_data0, tx.n_data1, tx.n_pw, tx.n_delim, tx.n_trcal) == (19, 38, 9, 9, 160)
    assert (tx.n_rtcal, tx.n_rtcal_hi, tx.n_trcal_hi) == (57, 47, 150)
    assert len(sim.work()) == 3660                                  # START: (int)(4575 / 1.25)
    w = sim.work()                                                  # Query
    # delim(9 low) data_0(9 high, 10 low) rtcal(47 high, 10 low) trcal(150 high, 10 low)
    want = np.concatenate([np.zeros(9), np.ones(9), np.zeros(10), np.ones(47), np.zeros(10), np.ones(150), np.zeros(10)])
    assert np.array_equal(w[: len(want)], want.astype(np.float32))


def test_real_blob_hook_documents_the_missing_known_answer():
    """The reference's only known answer needs misc/data/file_source_test, which this checkout lacks; the GPU
    suite carries a skipped-if-absent replay (tests/test_gpu_round2.py) that pins parity where the blob exists."""
    import os
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_round2.py")).read()
    assert "RFID_FILE_SOURCE_TEST" in src and "Tag ID : 27  Num of reads : 70" in src


def test_oracle_stream_equals_one_shot(oracle_mod, synth_mod):
    """oracle.Stream (the harness fed in pieces -- how traces larger than host memory are checked) gives the
    same windows, dumps and reader state as run_trace() over the whole trace, whatever the piece sizes."""
    t = synth_mod.make_trace(n_rounds=4, fixed_q=1, tag_ids=(0x11, 0x22), seed=17, sigma=0.02, t1_jitter_raw=5).samples
    cfg = oracle_mod.config(fixed_q=1)
    o = oracle_mod.run_trace(t, cfg)
    for sizes in ([len(t)], [1, 7, 1000, 33333], [50001]):
        st = oracle_mod.Stream(cfg)
        pos, k = 0, 0
        while pos < len(t):
            n = sizes[k % len(sizes)] if k < len(sizes) - 1 or len(sizes) == 1 else sizes[-1]
            st.feed_raw(t[pos:pos + n])
            pos += n
            k += 1
        r = st.result()
        st.close()
        assert r.n_windows == o.n_windows and np.array_equal(r.open_idx, o.open_idx)
        assert r.dumps.tobytes() == o.dumps.tobytes() and r.dc.tobytes() == o.dc.tobytes()
        assert r.stats() == o.stats()

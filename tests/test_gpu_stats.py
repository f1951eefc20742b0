"""stream_stats_kernel by itself on the crafted and the random result tables of tests/stats_cases.py, on the device
(tests/test_stats_emu.py: the same on the emulator, with the pinning of the reference and the coverage conditions).  Every
table through rfid_selftest_stats in the product's two workgroup shapes, one wave and sixteen per trace, each from the 48-byte
records and from their one-word summaries, every word of every output row against tests/stats_ref.py's replay; then one pass
of a wide plan of three ragged traces, the statistics from what the decoder left, against the oracle."""
import numpy as np
import pytest

import stats_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rfid
    c = rfid.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def launches():
    return sc.groups(sc.crafted() + sc.random_tables())


@pytest.mark.parametrize("from_summaries", [False, True], ids=["records", "summaries"])
@pytest.mark.parametrize("waves", [1, 16])
def test_kernel_on_the_device(ctx, launches, waves, from_summaries):
    assert sum(len(g.names) for g in launches) >= 600
    for g in launches:
        sc.check(ctx.selftest_stats, g, waves, from_summaries)


def test_wide_plan_of_three_ragged_traces(oracle_mod, synth_mod):
    """The wiring: a plan whose traces can hold more than 2 048 windows (sixteen waves per trace, summaries left by the
    decoder), three traces of different lengths in rows of odd length, so the second and third row of summaries are not
    16-byte aligned, and a queries limit that cuts inside the second trace only.  rfid_batch_process's statistics, and
    rfid_batch_stats once more on what the decoder left, equal the oracle's."""
    import torch
    import rfid
    t = synth_mod.make_trace(n_rounds=260, sigma=0.01, seed=97, fixed_q=1, tag_ids=(0x31, 0x52), t1_jitter_raw=3).samples
    L = len(t)
    Lp = L
    while ((Lp // 5) // 348 + 2) % 2 == 0:           # (rfid_batch_plan: the windows a trace of max_raw samples can hold)
        Lp += 5 * 348
    wmax = (Lp // 5) // 348 + 2
    assert wmax > 2048 and wmax % 2 == 1
    lens = [L * 45 // 100, L, L * 7 // 10]
    free = [oracle_mod.run_trace(t[:n], oracle_mod.config(fixed_q=1, max_num_queries=1 << 30)) for n in lens]
    e = [o.state.n_queries_sent - 1 for o in free]
    q = (max(e[0], e[2]) + e[1]) // 2
    assert max(e[0], e[2]) + 1 < q < e[1] - 1
    want = [oracle_mod.run_trace(t[:n], oracle_mod.config(fixed_q=1, max_num_queries=q)) for n in lens]
    assert [o.state.status for o in want] == [0, 1, 0] and want[1].n_windows < free[1].n_windows
    stride = (Lp + 1) & ~1
    host = np.zeros((3, stride), dtype=np.complex64)
    for b, n in enumerate(lens):
        host[b, :n] = t[:n]
    dev = torch.from_numpy(host.view(np.float32)).to("cuda:0")
    d_lens = torch.tensor(lens, dtype=torch.int64, device="cuda:0")
    ctx = rfid.Context(device=0, fixed_q=1, max_num_queries=q)
    try:
        ctx.batch_plan(3, Lp)
        ctx.batch_process_ptr(dev.data_ptr(), stride, Lp, d_lens.data_ptr(), want_scores=False)
        ctx.batch_sync()
        first = ctx.batch_stats().copy()
        ctx.batch_stage("stats")
        ctx.batch_sync()
        again = ctx.batch_stats().copy()
        assert first.tobytes() == again.tobytes()
        for b, (o, f) in enumerate(zip(want, free)):
            st = first[b]
            assert st["n_windows_used"] == o.n_windows and st["n_windows"] == f.n_windows, b
            assert st["status"] == o.state.status, b
            for k in ("n_queries_sent", "cur_inventory_round", "cur_slot_number", "n_epc_correct", "n_unique_tags"):
                assert st[k] == getattr(o.state, k), (b, k)
            assert np.array_equal(st["tag_reads"], np.array(o.state.tag_reads[:], dtype=np.int32)), b
    finally:
        ctx.close()

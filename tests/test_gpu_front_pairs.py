"""front_end_fused_kernel on the device: its pair body (knob front_single_step = 0) against its one-step-at-a-time body
(front_single_step = 1) byte for byte, and both against the oracle, on the shapes of tests/front_pairs_cases.py -- the
ragged workgroups also with an odd row stride, where the filter wave loads two samples at a time --; then 260
traces -- more workgroups than CUs -- one body against the other."""
import numpy as np
import pytest

import front_pairs_cases as cases
import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rfid
    c = rfid.Context(device=0)
    c.batch_set_long_stream(0)      # (few short traces would otherwise be cut along time)
    yield c
    c.close()


def _run(ctx, raw, lens, knob, want_y=True, unaligned=False):
    import torch
    B, L = raw.shape
    stride = (L | 1) if unaligned else (L + 1) & ~1     # odd stride: rows 8-byte aligned only, the filter wave's float2 loads
    host = np.zeros((B, stride), dtype=np.complex64)
    host[:, :L] = raw
    dev = torch.from_numpy(host.view(np.float32)).to("cuda:0")
    d_lens = torch.tensor(np.asarray(lens, dtype=np.int64)).to("cuda:0")
    ctx.batch_plan(B, L)
    ctx.batch_set_long_stream(0)
    ctx.set_knob("front_single_step", knob)
    try:
        ctx.batch_process_ptr(dev.data_ptr(), stride, L, d_lens.data_ptr(), want_scores=True)
        ctx.batch_sync()
    finally:
        ctx.set_knob("front_single_step", 0)
    assert ctx.batch_timing()["fused_front"] == 1
    w, r, s = ctx.batch_windows(want_scores=True)
    st = ctx.batch_stats().copy()
    y = [ctx.batch_mf_output(b)[: int(lens[b]) // 5].copy() for b in range(B)] if want_y else None
    return w, r, s, st, y


def _both_and_oracle(ctx, oracle_mod, raw, lens, unaligned=False):
    for b0 in range(0, len(raw), 8):          # at most 8 traces per pass
        rw, ln = raw[b0:b0 + 8], lens[b0:b0 + 8]
        w0, r0, s0, st0, y0 = _run(ctx, rw, ln, 0, unaligned=unaligned)
        w1, r1, s1, st1, y1 = _run(ctx, rw, ln, 1, unaligned=unaligned)
        assert w0.tobytes() == w1.tobytes() and r0.tobytes() == r1.tobytes() and s0.tobytes() == s1.tobytes()
        assert st0.tobytes() == st1.tobytes()
        for b, (wb, rb, sb) in enumerate(parity.split_by_stream(w0, r0, s0, len(rw))):
            assert y0[b].tobytes() == y1[b].tobytes()
            x = rw[b][: ln[b]]
            assert np.array_equal(y0[b].view(np.uint32), oracle_mod.fir(x)[: len(y0[b])].view(np.uint32))
            parity.compare_trace(wb, rb, sb, st0[b], oracle_mod.run_trace(x))


def test_step_counts_around_pairs_and_ring_wrap(ctx, oracle_mod, synth_mod):
    _both_and_oracle(ctx, oracle_mod, *cases.step_count_batch(synth_mod))


def test_windows_against_pair_boundaries(ctx, oracle_mod, synth_mod):
    _both_and_oracle(ctx, oracle_mod, *cases.shifted_batch(synth_mod))


def test_both_paths_of_the_sum(ctx, oracle_mod, synth_mod):
    _both_and_oracle(ctx, oracle_mod, *cases.sum_paths_batch(synth_mod))


@pytest.mark.parametrize("B,unaligned", [(1, False), (4, True), (5, False), (5, True)])
def test_workgroup_shapes(ctx, oracle_mod, synth_mod, B, unaligned):
    _both_and_oracle(ctx, oracle_mod, *cases.ragged_batch(synth_mod, B), unaligned=unaligned)


def test_260_traces_pair_body_equals_single_step_body(ctx, synth_mod):
    """65 workgroups of four traces and more: workgroups retire and are followed by others on the same CU"""
    base = synth_mod.make_trace(n_rounds=2, seed=420, sigma=0.0, noise=False).samples
    B, L = 260, len(base)
    rng = np.random.default_rng(9)
    noise = (rng.standard_normal((B, L, 2)).astype(np.float32) * np.float32(0.01)).view(np.complex64)[..., 0]
    raw = (base[None, :] + noise).astype(np.complex64)
    lens = np.full(B, L, dtype=np.int64)
    lens[1::7] -= 5 * 64 * np.arange(len(lens[1::7]))     # ragged: other step counts, odd and even
    w0, r0, s0, st0, _ = _run(ctx, raw, lens, 0, want_y=False)
    w1, r1, s1, st1, _ = _run(ctx, raw, lens, 1, want_y=False)
    assert len(w0) >= 3 * B
    assert w0.tobytes() == w1.tobytes() and r0.tobytes() == r1.tobytes() and s0.tobytes() == s1.tobytes()
    assert st0.tobytes() == st1.tobytes()

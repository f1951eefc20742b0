"""The dc_est finishing walk (ls2_dcb_finish_kernel, csrc/rfid_ls2.hpp) on the MI355X at every trace count that changes its
shape: G = min(512, 1024 / B) one-wave workgroups per trace that meet once per turn -- B = 1, 3, 17, 64, 70, 130, 1024 give
G = 512, 341, 60, 16, 14, 7, 1 (G / M not whole at 341; one window per unit below 16; nothing to meet at 1).  The carrier puts
one component of dc_est within 1.2 % of 4, 8 or 16 (25 |sin phi| or 25 |cos phi|, both signs of phi): the sums hover across a
binade edge, the rounds settle little and the walk takes the units.  Every trace must be the oracle's, bit for bit.  Seeded and
deterministic; one context in one process.  (The emulator runs the same walk interleaved on the CPU: tests/test_emu_fin_walk.py;
what it cannot see -- fences, acquire / release, the device's caches -- is checked here.)"""
import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu


def hover_batch(synth_mod, seed, B, sigma, edge, comp, sign, n_rounds, ragged, distinct=16, off=0.003):
    """B traces (`distinct` different ones, repeated) with dc_est's real / imaginary part at edge (1 + off), |off| <= 1.2 %
    -> (host [B][stride] complex64, lens, L)"""
    assert abs(off) <= 0.012
    rng = np.random.default_rng(seed)
    target = edge * (1.0 + off)
    phi = float(np.arcsin(target / 25.0)) if comp == "sin" else float(np.arccos(target / 25.0))
    leak = complex(np.exp(1j * sign * phi))
    base = [synth_mod.make_trace(n_rounds=n_rounds, seed=int(rng.integers(1, 1 << 30)), sigma=sigma, tag_ids=(7, 91),
                                 t1_jitter_raw=int(rng.integers(0, 6)), leak=leak).samples for _ in range(min(B, distinct))]
    L = max(map(len, base))
    stride = (L + 1) & ~1
    host = np.zeros((B, stride), dtype=np.complex64)
    lens = np.zeros(B, dtype=np.int64)
    for b in range(B):
        t = base[b % len(base)]
        host[b, :len(t)] = t
        lens[b] = len(t) - (int(rng.integers(1000, 20000)) if ragged and b % 3 == 1 else 0)
    return host, lens, L


class Refs:
    """oracle results by (trace content, length): the repeated traces of a batch are run once"""
    def __init__(self, oracle_mod):
        self.o, self.cache = oracle_mod, {}

    def __call__(self, host, lens):
        out = []
        for b in range(host.shape[0]):
            x = host[b, :lens[b]]
            key = (hash(x.tobytes()), int(lens[b]))
            if key not in self.cache:
                self.cache[key] = self.o.run_trace(x, self.o.config())
            out.append(self.cache[key])
        return out


def to_device(host, lens):
    import torch
    return (torch.from_numpy(host.view(np.float32).copy()).to("cuda:0"),
            torch.from_numpy(lens.copy()).to("cuda:0"))


def check(ctx, refs, B):
    w, r, s = ctx.batch_windows(want_scores=True)
    st = ctx.batch_stats()
    for b, (wb, rb, sb) in enumerate(parity.split_by_stream(w, r, s, B)):
        parity.compare_trace(wb, rb, sb, st[b], refs[b])
    return ctx.batch_ls_report()


@pytest.fixture(scope="module")
def ctx():
    import rfid
    c = rfid.Context(device=0)
    c.batch_set_long_stream(2)
    yield c
    c.close()


# (traces, sigma, edge, component, sign, inventory rounds per trace, ragged lens)
CASES = [
    (1, 0.06, 16.0, "sin", 1, 24, False),
    (3, 0.03, 8.0, "cos", -1, 16, True),
    (17, 0.06, 4.0, "sin", -1, 6, True),
    (64, 0.06, 16.0, "cos", 1, 4, False),
    (70, 0.03, 16.0, "sin", -1, 4, True),
    (130, 0.06, 8.0, "sin", 1, 3, True),
    (1024, 0.06, 4.0, "sin", 1, 3, True),
]


@pytest.mark.parametrize("B,sigma,edge,comp,sign,n_rounds,ragged", CASES, ids=[f"B{c[0]}-{c[3]}{c[2]:g}-s{c[1]}" for c in CASES])
@pytest.mark.parametrize("dc_rounds", [-1, 0], ids=["rounds", "walk-alone"])
def test_fin_walk_matches_oracle(ctx, oracle_mod, synth_mod, B, sigma, edge, comp, sign, n_rounds, ragged, dc_rounds):
    host, lens, L = hover_batch(synth_mod, 1000 + B, B, sigma, edge, comp, sign, n_rounds, ragged)
    refs = Refs(oracle_mod)(host, lens)
    dev, d_lens = to_device(host, lens)
    ctx.set_knob("dc_rounds", dc_rounds)
    try:
        ctx.batch_plan(B, L)
        ctx.batch_process_ptr(dev.data_ptr(), host.shape[1], L, d_lens.data_ptr(), want_scores=True)
        ctx.batch_sync()
        rep = check(ctx, refs, B)
    finally:
        ctx.set_knob("dc_rounds", -1)
    print("long-stream report:", rep)
    assert rep["verified"] == 1 and rep["gave_up"] == 0, rep
    if dc_rounds == 0:
        assert rep["dc_finished"] > 0, rep        # (one round at a binade edge leaves units behind: the walk took them)


@pytest.mark.parametrize("B", [3, 130])
def test_fin_walk_passes_back_to_back(ctx, oracle_mod, synth_mod, B):
    """Batches A, B, A enqueued without a sync between them: the alternating work spaces, the meeting counters zeroed between
    passes and the walk of one pass beside the fused front end of the next.  The last result is A's; then B alone is B's."""
    ha, la, La = hover_batch(synth_mod, 77, B, 0.06, 16.0, "sin", 1, 12 if B <= 3 else 3, True)
    hb, lb, Lb = hover_batch(synth_mod, 78, B, 0.06, 8.0, "cos", -1, 12 if B <= 3 else 3, True)
    L = max(La, Lb)
    stride = (L + 1) & ~1
    pad = lambda h: np.pad(h, ((0, 0), (0, stride - h.shape[1])))
    ha, hb = pad(ha), pad(hb)
    refs = Refs(oracle_mod)
    ra, rb = refs(ha, la), refs(hb, lb)
    da, dla = to_device(ha, la)
    db, dlb = to_device(hb, lb)
    ctx.set_knob("dc_rounds", 0)
    try:
        ctx.batch_plan(B, L)
        ctx.batch_process_ptr(da.data_ptr(), stride, L, dla.data_ptr(), want_scores=True)
        ctx.batch_process_ptr(db.data_ptr(), stride, L, dlb.data_ptr(), want_scores=True)
        ctx.batch_process_ptr(da.data_ptr(), stride, L, dla.data_ptr(), want_scores=True)
        ctx.batch_sync()
        rep = check(ctx, ra, B)
        assert rep["verified"] == 1 and rep["gave_up"] == 0 and rep["dc_finished"] > 0, rep
        ctx.batch_process_ptr(db.data_ptr(), stride, L, dlb.data_ptr(), want_scores=True)
        ctx.batch_sync()
        rep = check(ctx, rb, B)
        assert rep["verified"] == 1 and rep["gave_up"] == 0, rep
    finally:
        ctx.set_knob("dc_rounds", -1)

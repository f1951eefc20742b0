"""The repair stage on the device (rfid_batch_plan_repair / rfid_batch_repair / rfid_batch_get_repairs / rfid_batch_get_window_repairs
and the per-call rfid_repair_window): CRC-failed EPC frames recovered from their weakest decisions.  Every expected record is worked
out from the ORACLE alone (tests/repair_ref.py: the definition of include/rfid_mi355x.h run literally, the oracle's check_crc); every
comparison is exact -- integers equal, floats by bit pattern, then the bytes of the whole arrays.  The cases that also run on the wave
emulator are written once, in tests/repair_suite.py, and run here through stage_backend.Device: the smallest shapes at which the kernel
can still go wrong -- single traces, a ragged batch with a trace without windows, rows behind a cut-off, crafted windows, the protocol.
Below them, what only the device runs: eight traces, 1 024 replicas and the command line.  The traces are those of
tests/repair_cases.py, at the sensitivity edge (sigma = 0.02, tag amplitude 0.014 .. 0.018)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stage_backend
from stage_backend import lay_out, oracle_pass
import repair_cases as cases
import repair_ref as ref
from repair_suite import *

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIG = (1 << 31) - 2
EDGE = dict(fixed_q=0, tag_ids=(0x27,), seed=1, n_rounds=24, sigma=0.02, t1_jitter_raw=3, h=0.016 * np.exp(2.1j))


@pytest.fixture(scope="module")
def backend():
    return stage_backend.Device()


def _eight(synth_mod):
    """the edge trace, the lost tag, the mixed slots and five more seeds at A = 0.016"""
    mk = lambda **kw: synth_mod.make_trace(sigma=0.02, t1_jitter_raw=3, h=0.016 * np.exp(2.1j), fixed_q=0, tag_ids=(0x27,), **kw).samples
    return [cases.make(synth_mod, n) for n in ("edge", "lost", "mixed")] + [mk(seed=3 + k, n_rounds=10 + 2 * k) for k in range(5)]


@pytest.mark.parametrize("mode", [0, 2], ids=["fused-front-end", "long-stream"])
def test_ragged_batch_of_eight_traces(backend, oracle_mod, synth_mod, mode):
    """The edge trace, the lost tag, the mixed slots and five more seeds at A = 0.016, eight traces of different lengths.  The pass
    three times: byte-identical records, packed and per trace, against the reference."""
    import rfid
    host, lens, L, stride = lay_out(_eight(synth_mod))
    dev = backend.put(host, lens)
    packed, rows = ref.expected_batch(oracle_mod, *oracle_pass(oracle_mod, host, lens, 2, max_num_queries=BIG))
    fixed = [int((r["n_flips"] > 0).sum()) for r in rows]
    assert fixed[:3] == [14, 3, 6] and min(fixed[3:]) >= 1 and (packed["entry"] >= 0).sum() >= 20 and (packed["entry"] < 0).sum() >= 6, fixed
    assert sorted(set(packed["n_flips"].tolist())) == [1, 2, 3]
    ctx = rfid.Context(device=0, fixed_q=2, max_num_queries=BIG)
    try:
        ctx.batch_set_long_stream(mode)
        cases.plan(ctx, 8, L, 8)
        blobs = []
        for rep in range(3):
            backend.run_pass(ctx, dev, L, stride)
            blobs.append(cases.check(ctx, (packed, rows), (mode, rep)))
        assert blobs[0] == blobs[1] == blobs[2]
        print("repair of 8 traces: %.4f ms, %d repaired of %d failed of %d EPC windows; decode %.4f ms" %
              (ctx.batch_repair_ms(), len(packed), sum(int(((r["flags"] & 1) == 0).sum()) for r in rows), sum(map(len, rows)),
               ctx.batch_timing()["decode_ms"]))
    finally:
        ctx.close()


@pytest.mark.parametrize("overlap", [1, 2], ids=["one-result-set", "two-result-sets"])
def test_1024_noise_replicas_of_the_edge_trace(oracle_mod, synth_mod, overlap):
    """1 024 noise replicas (sigma = 0.02) of the edge trace's noise-free base, made on the device.  Replicas 0 and 1023 are exact
    against the reference; on all replicas only what holds whatever the noise: every repaired frame passes check_crc and differs from
    the window's decoded bits exactly by the toggles of its flips, 1 <= n_flips <= 3, and the packed list is the table's rows with
    n_flips > 0 in (stream, seq) order.  (Not that every repair is "true": about one hopeless window in 700 passes by chance.)  With
    two result sets alternating the repairs of a pass are that pass's -- also when the next pass, over other samples, is enqueued
    before they are fetched."""
    import rfid
    import torch
    B = 1024
    t = synth_mod.make_trace(noise=False, render=False, **EDGE)
    ctx = rfid.Context(device=0)
    data = other = None
    try:
        ctx.set_knob("overlap", overlap)
        L = ctx.synth_gen2_size(t.plan)
        stride = (L + 1) & ~1
        base = torch.zeros(2 * stride, dtype=torch.float32, device="cuda:0")
        data = torch.empty((B, 2 * stride), dtype=torch.float32, device="cuda:0")
        other = torch.empty((B, 2 * stride), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.synth_gen2_ptr(t.plan, base.data_ptr(), stride)
        ctx.synth_replicas_ptr(base.data_ptr(), L, data.data_ptr(), stride, B, 0.02, 777, first_replica=0)
        ctx.synth_replicas_ptr(base.data_ptr(), L, other.data_ptr(), stride, B, 0.02, 4242, first_replica=0)
        ctx.batch_sync()
        cases.plan(ctx, B, L, 4)
        blobs = []
        for rep in range(3):
            ctx.batch_process_ptr(data.data_ptr(), stride, L, 0)
            ctx.batch_inventory_enqueue()
            got = ctx.batch_repair()
            blobs.append(got.tobytes())
        assert blobs[0] == blobs[1] == blobs[2]
        repair_ms, decode_ms = ctx.batch_repair_ms(), ctx.batch_timing()["decode_ms"]
        st = ctx.batch_stats()
        w, res, _ = ctx.batch_windows()
        table = [ctx.batch_window_repairs(b) for b in range(B)]
        for b in range(B):
            assert len(table[b]) == int(st[b]["n_windows_used"]) // 2, (b, len(table[b]))
        rows = np.concatenate(table)
        key, epc = w[w["type"] == 1], res[w["type"] == 1]                  # (ordered by (stream, seq), as the rows are)
        assert len(rows) >= 23 * B and np.array_equal(rows["seq"], key["seq"]) and np.array_equal(rows["stream"], key["stream"])
        assert np.array_equal(rows["start"], key["start"]) and np.array_equal(epc["crc_ok"], rows["flags"] & 1)
        ok, fixed = (rows["flags"] & 1) == 1, rows["n_flips"] > 0
        print("1024 replicas of the edge trace: %d EPC windows, %d verified, %d failed, %d repaired (%s by 1 / 2 / 3 flips), %d of them "
              "known to the trace's inventory; repair %.4f ms, decode of the same pass %.4f ms (ratio %.3f), inventory %.4f ms" %
              (len(rows), ok.sum(), (~ok).sum(), fixed.sum(), np.bincount(rows["n_flips"], minlength=4)[1:].tolist(),
               (rows["entry"] >= 0).sum(), repair_ms, decode_ms, repair_ms / decode_ms, ctx.batch_inventory_ms()))
        assert got.tobytes() == rows[fixed].tobytes()                      # the packed list: the repaired rows in (stream, seq) order
        assert not (ok & fixed).any() and ok.sum() == int(st["n_epc_correct"].sum())
        j = np.arange(128)
        unpack = lambda words: ((words[j >> 5] >> (j & 31)) & 1).astype(np.uint8)
        lookup = {(int(k["stream"]), int(k["seq"])): i for i, k in enumerate(key)}
        ref.structure_ok(oracle_mod, rows, lambda s, q: unpack(epc[lookup[(s, q)]]["bits"]))
        for b in (0, B - 1):
            x = data[b, : 2 * L].cpu().numpy().view(np.complex64)
            o = oracle_mod.run_trace(x)
            w_packed, w_rows = ref.expected(oracle_mod, o, oracle_mod.fir(x), b)
            ref.assert_equal(table[b], w_rows, b)
            ref.assert_equal(got[got["stream"] == b], w_packed, b)
        # the next pass -- other samples -- enqueued BEFORE this pass's records are fetched: they are still this pass's
        ctx.batch_process_ptr(data.data_ptr(), stride, L, 0)
        ctx.batch_inventory_enqueue()
        ctx.batch_repair_enqueue()
        ctx.batch_process_ptr(other.data_ptr(), stride, L, 0)
        assert ctx.batch_repair_fetch().tobytes() == blobs[0]
        assert ctx.batch_window_repairs(B - 1).tobytes() == table[B - 1].tobytes()
        ctx.batch_inventory_enqueue()                   # ... and the pass over the other samples gets its own
        got2 = ctx.batch_repair()
        assert got2.tobytes() != blobs[0]
        x = other[3, : 2 * L].cpu().numpy().view(np.complex64)
        o = oracle_mod.run_trace(x)
        w_packed, w_rows = ref.expected(oracle_mod, o, oracle_mod.fir(x), 3)
        ref.assert_equal(got2[got2["stream"] == 3], w_packed, "other")
        ref.assert_equal(ctx.batch_window_repairs(3), w_rows, "other")
        assert repair_ms <= decode_ms, (repair_ms, decode_ms)
    finally:
        ctx.close()
        del data, other
        torch.cuda.empty_cache()


def test_command_line_writes_the_repairs_and_leaves_the_rest_alone(oracle_mod, synth_mod, tmp_path):
    """python -m rfid.batch --repair OUT.csv on two trace files, in a fresh child process: the CSV parses back to the reference's
    records, one line per file stands behind its results block, and with --inventory --tracks --quality beside it everything those
    flags print and write is what they print and write without it (up to the closing line of the pass, which carries wall times)."""
    from rfid import batch as rb
    ts = _eight(synth_mod)
    paths, results, ys = [], [], []
    for k, x in enumerate((ts[2], ts[3])):
        p = str(tmp_path / ("trace%d.bin" % k))
        rb.write_trace_file(p, x)
        paths.append(p)
        results.append(oracle_mod.run_trace(x, oracle_mod.config(fixed_q=2)))
        ys.append(oracle_mod.fir(x))
    packed, rows = ref.expected_batch(oracle_mod, results, ys)
    assert (packed["stream"] == 0).sum() == 6 and (packed["stream"] == 1).sum() >= 1 and (packed["entry"] < 0).any()
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"))
    csv = [str(tmp_path / n) for n in ("tracks.csv", "tracks_r.csv", "repairs.csv", "repairs_only.csv")]
    outs = []
    for extra in (["--inventory", "--tracks", csv[0], "--quality"], ["--inventory", "--tracks", csv[1], "--quality", "--repair", csv[2]],
                  ["--repair", csv[3]]):
        r = subprocess.run([sys.executable, "-m", "rfid.batch", "--fixed-q", "2", "--max-tags", "8"] + extra + paths, env=env,
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    plain, both, only = outs
    want_lines = [rb.format_repair_summary(r) for r in rows]
    for k, (p, line) in enumerate(zip(paths, want_lines)):
        assert line not in plain
        at = both.index(line, both.index(p + "\n"))                       # (behind the file's results block, before the next file)
        assert k + 1 == len(paths) or at < both.index(paths[k + 1] + "\n")
        assert only.index(line, only.index(p + "\n")) > 0
    stripped = both
    for line in want_lines:
        stripped = stripped.replace(line, "", 1)
    n_old = plain.rindex("2 traces, ")
    assert stripped[:n_old] == plain[:n_old] and stripped[n_old:].startswith("2 traces, ")
    assert stripped[n_old:].split("\n", 1)[1] == plain[n_old:].split("\n", 1)[1]
    assert open(csv[0]).read() == open(csv[1]).read()
    # the CSV parses back to the records
    for path in (csv[2], csv[3]):
        text = open(path).read()
        assert text == rb.format_repairs(packed, paths)
        lines = text.splitlines()
        assert lines[0] == rb.REPAIRS_HEADER and len(lines) == 1 + len(packed)
        for line, r in zip(lines[1:], packed):
            f = line.split(",")
            pc, epc = rb.frame_fields(r["frame"])
            assert f[0] == paths[int(r["stream"])] and f[1] == epc and int(f[2], 16) == pc and int(f[3]) == r["seq"]
            assert round(float(f[4]) * rb.TRACKS_RATE) == r["start"] and int(f[5]) == r["n_flips"]
            assert [int(v) for v in f[6].split("+")] == ref.flip_list(r)
            assert np.float32(f[7]).tobytes() == r["cost"].tobytes() and int(f[8]) == (1 if r["entry"] >= 0 else 0)

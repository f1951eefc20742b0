"""What the host side of a batch pass enqueues, written down call by call: the scenarios below run on tests/fake_hip's library (the
kernels on the wave emulator) with FAKE_HIP_TRACE set, one log per scenario.  Two builds of csrc/ that enqueue the same launches,
event records / waits, copies and allocations in the same order on the same streams write the same bytes -- how a change of the
host code alone (csrc/rfid_capi.hip and what it includes) is shown to change nothing:

    python tests/tools/host_call_trace.py OUT_A [--csrc OLD_CSRC]
    python tests/tools/host_call_trace.py OUT_B
    diff -r -x '*.so' OUT_A OUT_B

A plain script: not collected by pytest.  Each scenario runs in a process of its own (the runtime numbers streams and events in creation
order per process).  The long-stream path's second stream ("ahead") needs a 16 MB filter output and is not reached here: the GPU
suite's tests/test_gpu_round4.py covers it."""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gen2-uhf-rfid-reader_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "fake_hip")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _two_ragged():
    from stage_backend import lay_out
    from rfid import synth
    return lay_out([synth.make_trace(n_rounds=4, seed=11, sigma=0.01).samples, synth.make_trace(n_rounds=3, seed=12, sigma=0.01).samples], shorten=777)


def _passes(ctx, data, n, want_scores=False):
    host, lens, L, stride = data
    for _ in range(n):
        ctx.batch_process_ptr(host.ctypes.data, stride, L, lens.ctypes.data, want_scores=want_scores)


def _finish(ctx, want):
    """what every scenario ends with; `want`: (fused_front, more than one chunk) of the last pass -- the path it is there for"""
    ctx.batch_sync()
    t = ctx.batch_timing()
    assert (t["fused_front"], t["front_chunks"] > 1) == want, t
    assert int(ctx.batch_stats()["n_windows"].sum()) > 0


def _front(knobs, want, want_scores=False, pieces=False):
    def run(ctx):
        data = _two_ragged()
        for k, v in knobs.items():
            ctx.set_knob(k, v)
        ctx.batch_plan(2, data[2])
        _passes(ctx, data, 2, want_scores)
        _finish(ctx, want)
        rep = ctx.batch_ls_report()
        assert (rep["pieces"] > 0 and rep["verified"] == 1) if pieces else rep["pieces"] == 0, rep
    return run


def _stage_calls(ctx):
    host, lens, L, stride = data = _two_ragged()
    ctx.set_knob("long_stream", 0)
    ctx.batch_plan(2, L)
    for _ in range(2):
        ctx.batch_stage("mf", host.ctypes.data, stride, L, lens.ctypes.data)
        ctx.batch_stage("gate")
        ctx.batch_stage("decode", False)
        ctx.batch_stage("stats")
    _finish(ctx, (0, False))


def _all_stages(mode):
    def run(ctx):
        data = _two_ragged()
        ctx.set_knob("long_stream", mode)
        ctx.batch_plan(2, data[2])
        ctx.batch_plan_inventory(8)
        ctx.batch_plan_tracks()
        ctx.batch_plan_quality()
        ctx.batch_plan_repair()
        ctx.batch_plan_slots()
        ctx.batch_plan_commands()
        ctx.batch_plan_fine()
        for _ in range(2):
            _passes(ctx, data, 1)
            ctx.batch_inventory()
            ctx.batch_tracks()
            ctx.batch_quality()
            ctx.batch_repair()
            ctx.batch_slots_enqueue()
            ctx.batch_commands_enqueue()
            ctx.batch_fine()
            assert len(ctx.batch_window_quality(1)) > 0 and len(ctx.batch_window_repairs(1)) > 0 and len(ctx.batch_window_fine(1)) > 0
            assert len(ctx.batch_window_moments(1)) > 0 and len(ctx.batch_window_commands(1)) > 0
        _finish(ctx, (2 if mode else 1, False))
    return run


def _per_call_forms(ctx):
    """the four calls that work on windows a caller holds, interleaved: what they allocate, copy and launch (the values do not matter)"""
    import numpy as np
    from rfid import capi
    win = np.zeros(1370, dtype=np.complex64)
    res = np.zeros(1, dtype=capi.RESULT_DTYPE)[0]
    res["type"] = 1
    for n_mom, n_cmd in ((9, 17), (1, 3)):
        ctx.repair_window(win, res)
        ctx.window_moments(np.zeros((n_mom, 240), dtype=np.complex64))
        ctx.fine_window(win, res)
        ctx.commands_of(np.ones((n_cmd, 704), dtype=np.complex64), np.ones(n_cmd, dtype=np.complex64))


def _second_set(ctx):
    from stage_backend import lay_out
    from rfid import synth
    data = lay_out([synth.make_trace(n_rounds=1, seed=100 + i, sigma=0.01).samples for i in range(64)], shorten=7)
    ctx.set_knob("long_stream", 0)
    ctx.set_knob("overlap", 2)
    ctx.batch_plan(64, data[2])
    _passes(ctx, data, 3)
    _finish(ctx, (1, False))


SCENARIOS = {
    "fused_scores0": _front({"long_stream": 0}, (1, False)),
    "fused_scores1": _front({"long_stream": 0}, (1, False), want_scores=True),
    "long_stream": _front({"long_stream": 2}, (2, False), pieces=True),
    "chunked": _front({"long_stream": 0, "front_chunks": 4}, (0, True)),
    "unfused": _front({"long_stream": 0, "front_unfused": 1}, (0, False)),
    "stage_calls": _stage_calls,
    "all_stages_mode0": _all_stages(0),
    "all_stages_mode2": _all_stages(2),
    "second_set": _second_set,
    "per_call_forms": _per_call_forms,
}


def _library(out_dir, csrc):
    """tests/fake_hip's build of `csrc` (default: this tree's), kept in out_dir"""
    import build_capi_emu
    if csrc:
        build_capi_emu.CSRC = os.path.abspath(csrc)
    build_capi_emu.OUT = os.path.join(out_dir, "librfid_capi_emu.so")
    return build_capi_emu


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir")
    ap.add_argument("--csrc", default=None, help="the csrc/ directory to build the host code from (default: this tree's)")
    ap.add_argument("--scenario", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    build = _library(a.out_dir, a.csrc)
    if a.scenario is None:
        build.build(force=True)
        for name in SCENARIOS:
            log = os.path.join(a.out_dir, name + ".log")
            if os.path.exists(log):
                os.remove(log)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), a.out_dir, "--scenario", name] + (["--csrc", a.csrc] if a.csrc else []),
                                  env=dict(os.environ, FAKE_HIP_TRACE=log, FAKE_HIP_LAG="0"))
            print(name, sum(1 for _ in open(log)), "calls")
        return
    import emu_lib
    import rfid
    with emu_lib.emulated_library():
        ctx = rfid.Context(device=0, fixed_q=0)
        try:
            SCENARIOS[a.scenario](ctx)
        finally:
            ctx.close()


if __name__ == "__main__":
    main()

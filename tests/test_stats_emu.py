"""stream_stats_kernel by itself on the crafted result tables of tests/stats_cases.py, on the emulator (tests/test_gpu_stats.py:
the same on the device).  Three layers, each one's reference validated by the one above, ending at the oracle:
 1. tests/stats_ref.py (the reader's statistics, window by window) over the oracle's decoded windows == the oracle's final
    reader state, for limits that cut before, on and behind the last window and a trace of seven tag ids;
 2. what every family of crafted tables reaches, asserted from that replay alone (conditions, not measurements);
 3. the kernel as rfid_selftest_stats launches it (1, 4 and 16 waves per trace; from the records and from their summaries)
    == the replay, every word of every output row; a handful of launches through the C call on the stand-in runtime."""
import numpy as np
import pytest

import stats_cases as sc
import stats_ref
from rfid import _capi as capi

STATE_FIELDS = ("n_queries_sent", "cur_inventory_round", "cur_slot_number", "n_epc_correct", "n_unique_tags", "status")
TERMINATION_LIMITS = [dict(max_num_queries=3), dict(number_unique_tags=1), dict(number_unique_tags=0),
                      dict(max_num_queries=1, number_unique_tags=2), dict(max_num_queries=0)]       # test_emu_parity's
SEVEN_IDS = (0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77)


@pytest.fixture(scope="module")
def crafted():
    return sc.crafted()


@pytest.fixture(scope="module")
def random_tables():
    return sc.random_tables()


def by_family(cases, family):
    return [c for c in cases if c.family == family]


# ---- 1. the replay is the oracle's bookkeeping -----------------------------------------------------------------------------
def _pin(oracle_mod, trace, fixed_q, limit_sets):
    """the replay over ALL windows the oracle decodes without limits, cut by the limits == the oracle run with those limits"""
    free = oracle_mod.run_trace(trace, oracle_mod.config(fixed_q=fixed_q, max_num_queries=10 ** 9, number_unique_tags=10 ** 6))
    assert free.state.status == stats_ref.RUNNING and free.n_windows == len(free.dumps)
    windows = stats_ref.windows_of(free.dumps)
    n_cut = 0
    for kw in limit_sets:
        o = oracle_mod.run_trace(trace, oracle_mod.config(fixed_q=fixed_q, **kw))
        full = dict(max_num_queries=1000, number_unique_tags=100)
        full.update(kw)
        st = stats_ref.replay(windows, 1 << fixed_q, full["max_num_queries"], full["number_unique_tags"])
        for f in STATE_FIELDS:
            assert getattr(st, f) == getattr(o.state, f), (kw, f, getattr(st, f), getattr(o.state, f))
        assert st.n_windows_used == o.n_windows, (kw, st.n_windows_used, o.n_windows)
        assert [st.tag_reads.get(i, 0) for i in range(256)] == list(o.state.tag_reads), kw
        assert st.n_windows == free.n_windows
        n_cut += st.n_windows_used < st.n_windows
    return free, n_cut


def test_replay_equals_oracle_around_the_last_window(oracle_mod, synth_mod):
    t = synth_mod.make_trace(n_rounds=2, fixed_q=3, tag_ids=(0x21, 0x43, 0x65), seed=78, sigma=0.01).samples
    free, _ = _pin(oracle_mod, t, 3, [dict()])
    e = free.state.n_queries_sent - 1
    assert e == int((free.dumps["type"] == 1).sum()) >= 4 and free.state.n_unique_tags == 3
    assert free.dumps["type"][-1] == 1            # the trace's last window is an EPC window: max_num_queries = E cuts nothing
    _, n_cut = _pin(oracle_mod, t, 3, TERMINATION_LIMITS + [dict(max_num_queries=q) for q in (e - 1, e, e + 1)])
    assert n_cut == len(TERMINATION_LIMITS) + 1
    on_last = oracle_mod.run_trace(t, oracle_mod.config(fixed_q=3, max_num_queries=e))
    assert on_last.state.status == stats_ref.TERMINATED and on_last.n_windows == free.n_windows
    assert oracle_mod.run_trace(t, oracle_mod.config(fixed_q=3, max_num_queries=e + 1)).state.status == stats_ref.RUNNING


def test_replay_equals_oracle_on_a_trace_of_seven_ids(oracle_mod, synth_mod):
    t = synth_mod.make_trace(n_rounds=3, fixed_q=4, tag_ids=SEVEN_IDS, seed=79, sigma=0.01).samples
    free, _ = _pin(oracle_mod, t, 4, [dict()])
    assert free.state.n_unique_tags >= 6
    assert int((free.dumps["type"] == 1).sum()) > free.state.n_epc_correct          # (collisions: CRC-failed EPC windows too)
    _, n_cut = _pin(oracle_mod, t, 4, [dict(number_unique_tags=n) for n in (0, 1, 4, 5, 6)] +
                    [dict(number_unique_tags=4, max_num_queries=q) for q in (2, 1000)])
    assert n_cut >= 6


# ---- 2. coverage: what the tables reach, from the replay alone -------------------------------------------------------------
def _first_reads(res):
    first = {}
    for k, (t, ok, i) in enumerate(stats_ref.windows_of(res)):
        if t == 1 and ok and i not in first:
            first[i] = k
    return first


def test_records_are_what_the_decoders_write(crafted, random_tables):
    n_free = 0
    for c in crafted + random_tables:
        r = c.res
        rn16, epc = r[r["type"] == 0], r[r["type"] == 1]
        assert len(rn16) + len(epc) == len(r)
        if c.family == "stale":            # (RN16 records with a CRC flag and an id: stats_cases' header)
            assert ((rn16["crc_ok"] == 1) & (rn16["tag_id"] >= 0)).sum() >= 100 and np.array_equal(r["type"], sc.alt(len(r)))
            rn16 = rn16[rn16["crc_ok"] == 0]
        assert (rn16["crc_ok"] == 0).all() and (rn16["tag_id"] == -1).all() and (rn16["n_bits"] == 16).all()
        ok = epc["crc_ok"] == 1
        assert ((epc["crc_ok"] == 0) | ok).all() and (epc["tag_id"][~ok] == -1).all()
        assert ((epc["tag_id"][ok] >= 0) & (epc["tag_id"][ok] < 256)).all()
        if not np.array_equal(r["type"], sc.alt(len(r))):
            n_free += 1
            assert c.family == "queries"           # (the inverted and the RN16-led tables: stats_cases' header)
    assert 0 < n_free < 80


def test_lengths_family(crafted):
    cs = {c.name: c for c in by_family(crafted, "lengths")}
    for nw in sc.LENGTHS + sc.LONG:
        plain, last, short = cs["len%d" % nw], cs["len%d_q_last" % nw], cs["len%d_q_short" % nw]
        assert plain.want.n_windows == nw == plain.want.n_windows_used and plain.want.status == stats_ref.RUNNING
        assert last.want.status == stats_ref.TERMINATED and last.want.n_windows_used == (nw if nw % 2 == 0 else nw - 1)
        assert short.want.status == stats_ref.RUNNING and short.want.n_windows_used == nw
    for nw in sc.LONG:
        assert sc.share(nw, 16) > 1024 and nw * capi.RESULT_DTYPE.itemsize < 1 << 20


def test_queries_family(crafted):
    cs = by_family(crafted, "queries")
    seen = set()
    for c in cs:
        if "deciding" in c.aim:
            t, nw = c.aim["deciding"], len(c.res)
            assert c.want.status == stats_ref.TERMINATED and c.want.n_windows_used == t + 1, c.name
            assert c.res["type"][t] == 1 and c.want.n_queries_sent - 1 == c.limits[1], c.name
            for w in c.aim["where"]:
                if w[0] in ("lane", "turn"):
                    assert t % 64 == w[1] % 64
                    seen.add((nw > 3000,) + w)
                else:
                    waves, wave, end = w
                    seg = sc.share(nw, waves)
                    assert t == (wave * seg if end == "first" else min(wave * seg + seg, nw) - 1)
                    busy = (nw + seg - 1) // seg
                    seen.add((nw > 3000, waves, "wave0" if wave == 0 else ("last" if wave == busy - 1 else "middle"), end))
            if t + 1 == nw:
                seen.add((nw > 3000, "k_term == nw"))
    for long in (False, True):
        for waves in sc.WAVE_COUNTS:
            for end in ("first", "last"):
                assert (long, waves, "wave0", end) in seen
                if waves > 1:
                    assert (long, waves, "middle", end) in seen and (long, waves, "last", end) in seen
        assert {(long, "lane", 0), (long, "lane", 63), (long, "turn", 255), (long, "turn", 1024), (long, "k_term == nw")} <= seen
    lim = {c.limits[1]: c.want for c in cs if c.name.startswith("q_limit_")}
    assert lim[0].status == 1 and lim[0].n_windows_used == 0 and lim[0].n_queries_sent == 1
    assert lim[1].status == 1 and lim[1].n_windows_used == 2 and lim[sc.NO_Q].status == 0
    for c in cs:
        if "lead" in c.aim:      # the deciding EPC window behind waves without any
            assert (c.res["type"][: c.aim["lead"]] == 0).all() and c.want.status == 1
            for waves in (4, 16):
                assert (c.want.n_windows_used - 1) // sc.share(len(c.res), waves) >= 1 and sc.share(len(c.res), waves) <= c.aim["lead"]


def test_unique_family(crafted):
    cs = by_family(crafted, "unique")
    tables = {}
    for c in cs:
        tables.setdefault(c.name.rsplit("_u", 1)[0], {})[c.limits[2]] = c
    assert {c.limits[2] for c in cs} == set(sc.UNIQUE_LIMITS)
    groups_hit = set()
    for name, per_limit in tables.items():
        res = per_limit[0].res
        first = _first_reads(res)
        order = sorted(first, key=first.get)
        m = len(first)
        assert per_limit[256].want.n_unique_tags == m and per_limit[256].want.status == 0
        for n, c in per_limit.items():
            if n < m:         # the cut right behind the first read of the (n + 1)-th id
                assert c.want.status == 1 and c.want.n_unique_tags == n + 1 and c.want.n_windows_used == first[order[n]] + 1, c.name
                assert c.want.n_windows_used < len(res) or (name == "second_on_last" and n == 1)
            else:
                assert c.want.status == 0 and c.want.n_windows_used == len(res), c.name
        if name.startswith("ids"):
            assert m == per_limit[0].aim["ids"]
            assert order != sorted(order) or m <= 2
            assert per_limit[256].want.n_epc_correct >= 3 * m                      # repeats are frequent
            if m >= 63:
                assert {first[i] // sc.share(len(res), 16) for i in order} == set(range(16))     # spread over every wave's share
            assert (255 in first) == (m >= 101)
            assert (res["crc_ok"][res["type"] == 1] == 0).sum() > 100
        if "lead_fail" in per_limit[0].aim:       # CRC-failed EPC windows in front of the first good read start no id
            k = first[order[0]]
            assert ((res["type"][:k] == 1) & (res["crc_ok"][:k] == 0) & (res["tag_id"][:k] == -1)).sum() >= per_limit[0].aim["lead_fail"]
            assert per_limit[0].want.n_windows_used == k + 1 and per_limit[0].want.n_epc_correct == 1
        if name == "fail_first":
            assert 255 not in first
        if name == "only255":
            assert per_limit[256].want.tag_reads == {255: per_limit[256].want.n_epc_correct} and 255 in first
        if name == "second_on_last":      # k_u == nw: nothing is cut, and only the count of ids says TERMINATED
            c = per_limit[1]
            assert c.want.status == 1 and c.want.n_windows_used == len(res) == first[c.aim["on_last"]] + 1
            assert c.want.n_queries_sent <= c.limits[1] and c.want.n_unique_tags == 2
        if "group" in per_limit[0].aim:
            c = per_limit[1]
            assert res["tag_id"][c.want.n_windows_used - 1] // 64 == c.aim["group"] and order[1] == c.aim["second"]
            groups_hit.add(c.aim["group"])
    assert {int(n[3:]) for n in tables if n.startswith("ids")} == set(sc.IDS_READ)
    assert groups_hit == {0, 1, 2, 3}


def test_stale_family(crafted):
    cs = {c.limits[2]: c for c in by_family(crafted, "stale")}
    res = cs[0].res
    first = _first_reads(res)
    stale_ids = set(res["tag_id"][(res["type"] == 0) & (res["crc_ok"] == 1)].tolist())
    assert len(first) == 6 and len(stale_ids) >= 20 and not stale_ids & set(first)
    assert cs[256].want.n_unique_tags == 6 and set(cs[256].want.tag_reads) == set(first) and cs[256].want.status == 0
    order = sorted(first, key=first.get)
    for n in (0, 1, 5):        # the cut behind the (n + 1)-th id read by an EPC window, stale records in front of it
        assert cs[n].want.status == 1 and cs[n].want.n_windows_used == first[order[n]] + 1
        assert ((res["type"][: first[order[n]]] == 0) & (res["crc_ok"][: first[order[n]]] == 1)).sum() > n + 1


def test_both_limits_family(crafted):
    rels = set()
    for c in by_family(crafted, "both"):
        k_q, k_u = sc.cuts(c)
        assert k_q is not None and k_u is not None and k_u < len(c.res)
        assert {"lt": k_q < k_u, "eq": k_q == k_u, "gt": k_q > k_u}[c.aim["rel"]], (c.name, k_q, k_u)
        assert c.want.n_windows_used == min(k_q, k_u) and c.want.status == 1
        rels.add((c.name.split("_")[0], c.aim["rel"]))
    assert len(rels) == 6


def test_slots_family(crafted):
    seen = {}
    for c in by_family(crafted, "slots"):
        ms, e = c.limits[0], c.want.n_queries_sent - 1
        assert c.want.status == 0 and e == len(c.res) // 2
        seen.setdefault(ms, {})[e] = (c.want.cur_inventory_round, c.want.cur_slot_number)
    assert set(seen) == {1, 2, 16, 32768}
    for ms, by_e in seen.items():
        m = [k for k in range(1, 3) if {k * ms - 1, k * ms, k * ms + 1} <= set(by_e)]
        assert m, ms
        for k in m:          # a round ends with the EPC window that takes the slot number past max_slot_number
            assert by_e[k * ms - 1][0] + 1 == by_e[k * ms][0] == by_e[k * ms + 1][0] - (ms == 1) and by_e[k * ms][1] == 1


def test_batch_family(crafted):
    gs = [g for g in sc.groups(crafted) if g.limits == sc.BATCH_LIMITS]
    assert len(gs) == 1
    g = gs[0]
    n, wmax = g.res.shape
    assert n >= 6 and wmax % 2 == 1 and 0 in g.wcount and len(set(g.wcount.tolist())) == n
    al = sc.row_alignments(g)
    assert set(al) == {0, 4, 8, 12}
    # both fetch paths: the 16-byte load on an aligned row, its scalar tail at the row's end and at a cut that is no multiple
    # of four, and the scalar fetch on every other row
    assert any(a == 0 and g.wcount[s] >= 8 and g.want[s]["n_windows_used"] % 4 and g.want[s]["n_windows_used"] < g.wcount[s]
               for s, a in enumerate(al))
    assert any(a != 0 and g.wcount[s] >= 8 for s, a in enumerate(al))
    assert {0, 1} <= set(g.want["status"].tolist())


def test_random_family(random_tables):
    assert len(random_tables) == sc.N_RANDOM and len({c.limits for c in random_tables}) <= 9
    kinds = {"q": 0, "u": 0, "none": 0}
    for c in random_tables:
        k_q, k_u = sc.cuts(c)
        cut = c.want.n_windows_used < len(c.res)
        kind = "none" if not cut else ("q" if k_q == c.want.n_windows_used else "u")
        assert kind == c.aim["kind"]
        kinds[kind] += 1
    assert min(kinds.values()) >= sc.N_RANDOM // 4, kinds
    lens = sorted(len(c.res) for c in random_tables)
    assert lens[0] == 0 and lens[len(lens) // 3] < 64 and lens[-1] > 2900
    ids = sorted(c.want.n_unique_tags for c in random_tables)
    assert ids[0] == 0 and ids[-1] > 128


# ---- 3. the kernel ------------------------------------------------------------------------------------------------------------
FAMILIES = ("lengths", "queries", "unique", "both", "slots", "batch", "stale", "random")


@pytest.fixture(scope="module")
def emu_groups(crafted, random_tables):
    """the emulator's launches, family by family: every crafted table (of the two long ones' launches a part) and a tenth of
    the random ones"""
    return {f: sc.groups([c for c in by_family(crafted + random_tables, f) if c.emu]) for f in FAMILIES}


def test_the_emulators_share_holds_every_table_and_a_long_one(crafted, emu_groups):
    names = {n for gs in emu_groups.values() for g in gs for n in g.names}
    assert {c.name for c in crafted if len(c.res) <= 3100} <= names          # every crafted table; not every launch of the long ones
    assert {"len%d" % n for n in sc.LONG} <= names and "slot32768_epc32768" in names
    assert len([n for n in names if n.startswith("random")]) >= 30
    assert any(g.wcount.max() > 16 * 1024 and g.limits[1] < sc.NO_Q for g in emu_groups["queries"])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("from_summaries", [False, True], ids=["records", "summaries"])
@pytest.mark.parametrize("waves", sc.WAVE_COUNTS)
def test_kernel_on_the_emulator(emu_mod, emu_groups, waves, from_summaries, family):
    for g in emu_groups[family]:
        sc.check(emu_mod.stats_selftest, g, waves, from_summaries)


@pytest.fixture(scope="module")
def capi_ctx():
    import emu_lib
    with emu_lib.emulated_library():
        import rfid
        c = rfid.Context(device=0)
        try:
            yield c
        finally:
            c.close()


def test_kernel_through_the_c_call(capi_ctx, crafted):
    """rfid_selftest_stats of csrc/rfid_capi.hip on the stand-in runtime: the entry's host code, a handful of launches"""
    gs = [g for g in sc.groups(by_family(crafted, "batch") + by_family(crafted, "both"))]
    assert len(gs) >= 4
    for g in gs[:5]:
        for waves, from_summaries in ((1, True), (16, False), (16, True)):
            sc.check(capi_ctx.selftest_stats, g, waves, from_summaries)
    g = gs[0]
    for bad in (dict(waves=0), dict(waves=17), dict(max_slot_number=0)):
        kw = dict(waves=1, from_summaries=False, max_slot_number=g.limits[0], max_num_queries=g.limits[1], number_unique_tags=g.limits[2])
        kw.update(bad)
        with pytest.raises(capi.RfidError):
            capi_ctx.selftest_stats(g.res, g.wcount, **kw)
    with pytest.raises(capi.RfidError):
        capi_ctx.selftest_stats(g.res, g.wcount + g.res.shape[1], 1, False, *g.limits)     # counts past the rows

"""The inventory and the tracks kernels by themselves on the crafted result tables of tests/inventory_cases.py, on the emulator
(tests/test_gpu_inventory_tables.py: the same on the device).  Three layers, each one's reference validated by the one above, ending at
the oracle:
 1. the builder that turns a row of a result table into the dumps-shaped array tests/inventory_ref.py and tests/tracks_ref.py take
    (inventory_ref.dumps_of_table): on the library's own results of a synthesised trace it gives the inventory and the tracks the
    oracle's dumps give;
 2. what every family of crafted tables reaches, asserted from those references alone (conditions, not measurements; where a condition
    is about the probe sequence, from inventory_cases.inv_hash, the restatement that built the input);
 3. the five kernels as rfid_selftest_inventory launches them (one wave and sixteen per trace) == the references, every word of every
    output array, the prefilled words the kernels must leave alone included; a handful of launches through the C call on the stand-in
    runtime, argument errors included."""
import numpy as np
import pytest

import inventory_cases as ic
import inventory_ref
import tracks_ref
from rfid import _capi as capi


@pytest.fixture(scope="module")
def launches():
    by = {}
    for g in ic.launches(emu_only=True):
        by.setdefault(g.family, []).append(g)
    return by


@pytest.fixture(scope="module")
def tables():
    return {t.name: t for t in ic.crafted() + ic.random_tables()}


def entries_of(t):
    """a table's entries and reads by the reference, without the kernels' limits"""
    return tracks_ref.expected(inventory_ref.dumps_of_table(t.res, t.wcount, t.used), t.start)


def norms_of(t, ent, reads, e):
    r = reads[reads["entry"] == e]
    with np.errstate(over="ignore", under="ignore"):
        return r["seq"], (r["h_re"] * r["h_re"] + r["h_im"] * r["h_im"]).astype(np.float32)


# ---- 1. the builder against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limits", [dict(), dict(max_num_queries=7)], ids=["whole", "cut"])
def test_table_builder_equals_the_oracles_dumps(oracle_mod, synth_mod, emu_mod, limits):
    t = synth_mod.make_trace(n_rounds=4, fixed_q=2, tag_ids=(0x27, 0x27, 0x31), seed=104, sigma=0.02, t1_jitter_raw=3).samples
    o = oracle_mod.run_trace(t, oracle_mod.config(fixed_q=2, **limits))
    got = emu_mod.batch_process(t, fixed_q=2, **limits)
    used = int(got["stats"][0]["n_windows_used"])
    assert used == o.n_windows == len(o.dumps) and (len(got["results"]) > used) == bool(limits)
    d = inventory_ref.dumps_of_table(got["results"], len(got["results"]), used)
    assert len(d) == len(o.dumps)
    for f in ("type", "crc_ok", "bits"):
        assert np.array_equal(d[f], o.dumps[f]), f
    ok = (d["type"] == 1) & (d["crc_ok"] == 1)
    assert np.array_equal(d["tag_id"][ok], o.dumps["tag_id"][ok]) and ok.sum() >= 5         # (the id of a read: the oracle keeps none of the others)
    want = tracks_ref.expected(o.dumps, o.open_idx)
    mine = tracks_ref.expected(d, got["windows"]["start"])
    n_ent = len(want[0])
    assert n_ent == 3 and len(want[1]) >= 5
    assert mine[0].tobytes() == want[0].tobytes() and mine[1].tobytes() == want[1].tobytes() and np.array_equal(mine[2], want[2])
    # and the launch-level expectation over it: one trace, within the limits and beyond them
    res = got["results"][None, :]
    for max_tags, slots, fits in ((n_ent, 4, True), (n_ent - 1, 4, False), (n_ent, n_ent - 1, False)):
        w = tracks_ref.expected_tables(res, [res.shape[1]], [used], got["windows"]["start"][None, :], max_tags, slots)
        assert w["overflow"][0] == (not fits) and w["head"][1] == (inventory_ref.NO_TRACE if fits else 0)
        assert (w["packed"].tobytes() == want[0].tobytes() and w["reads"].tobytes() == want[1].tobytes()) if fits else \
            (len(w["packed"]) == 0 and len(w["reads"]) == 0 and w["counts"][0] == 0)


# ---- 2. coverage: what the tables reach, from the references alone ------------------------------------------------------------------
def test_records_are_what_the_decoders_write(tables):
    n_all_epc = 0
    for t in tables.values():
        r = t.res
        if not np.array_equal(r["type"], ic.alt(len(r))):
            assert t.family == "lanes" and (r["type"] == 1).all()          # (the all-EPC tables: inventory_cases' header)
            n_all_epc += 1
        rn16, epc = r[r["type"] == 0], r[r["type"] == 1]
        assert (rn16["n_bits"] == 16).all() and (epc["n_bits"] == 128).all()
        ok = epc["crc_ok"] == 1
        assert ((epc["crc_ok"] == 0) | ok).all() and (epc["tag_id"][~ok] == -1).all()
        assert np.array_equal(epc["tag_id"][ok], ic.tag_id_of(epc["bits"][ok])) and not np.isnan(epc["h_re"][ok]).any() and not np.isnan(epc["h_im"][ok]).any()
        if ok.sum() >= 20 and len(rn16) >= 20:      # what stage_fetch must not act on: stale RN16 records and failed EPC records with the bits of frames read
            read = {bytes(f) for f in epc["bits"][ok]}
            assert sum(bytes(f) in read for f in rn16["bits"][rn16["crc_ok"] == 1]) >= 3
            assert sum(bytes(f) in read for f in epc["bits"][~ok]) >= 1 or (~ok).sum() < 8
    assert n_all_epc == 2


def test_counts_family(tables):
    seen = set()
    for t in tables.values():
        if t.family != "counts":
            continue
        ent, reads, _ = entries_of(t)
        d = len(ent)
        assert d == t.aim["d"] and len(reads) > d and t.slots >= 2 * d or t.name == "count64_rows65"
        assert (t.aim["over"] == "count") == (d > t.max_tags) and d <= t.slots
        seen.add((d, d - t.max_tags))
        seen.add(("inventory<128>" if t.slots <= 128 else "inventory<1024>", "tracks small" if t.slots <= 128 and t.max_tags <= 64 else "tracks large"))
    assert {(d, 0) for d in ic.COUNTS_D} | {(d, 1) for d in ic.COUNTS_D if d > 1} | {(64, -1)} <= seen
    assert {("inventory<128>", "tracks small"), ("inventory<128>", "tracks large"), ("inventory<1024>", "tracks large")} <= seen
    assert tables["count512_fits"].slots == 1024 and tables["count64_fits"].slots == 128 and tables["count65_fits"].slots == 256


def test_full_tables_family(tables):
    for d in ic.FULL_D:
        t = tables["full%d" % d]
        assert len(entries_of(t)[0]) == d == t.slots == t.max_tags              # every slot owned
    for d in ic.OVERFULL_D:
        t = tables["overfull%d" % d]
        assert len(entries_of(t)[0]) == d == t.slots + 1 and t.max_tags >= d    # overflow by `full`, not by the rows


def test_one_chain_family(tables):
    for slots, n in ((1024, 24), (128, 64)):
        plain, desc, blocked = (tables["chain%d%s" % (slots, k)] for k in ("", "_descending", "_blocked"))
        for t in (plain, desc, blocked):
            ent = entries_of(t)[0]
            h0, step = ic.inv_hash(ent["frame"], slots - 1)
            key = h0 * slots + step
            chain = key == np.bincount(key).argmax()
            assert chain.sum() == n == t.aim["chain"] and len(ent) <= t.max_tags and t.slots == slots
            # the k-th frame of the chain to be read first finds k slots of its probe sequence taken: n + 1 rounds at the least
            if t is blocked:
                on_chain = (h0[chain][0] + np.arange(n) * step[chain][0]) & (slots - 1)
                assert (~chain).sum() == t.aim["blockers"] and np.isin(h0[~chain], on_chain).all()
                assert ent["first_seq"][~chain].max() < ent["first_seq"][chain].min()           # they claim their slots first
        a, b = entries_of(plain)[0], entries_of(desc)[0]
        assert [bytes(f) for f in a["frame"]] == [bytes(f) for f in b["frame"]][::-1]


def test_near_frames_family(tables):
    ent = entries_of(tables["near_flips"])[0]
    f = ent["frame"]
    dist = np.array([[int(np.unpackbits((x ^ y).view(np.uint8)).sum()) for y in f] for x in f[:129]])
    assert len(ent) == 129 and sorted(dist.min(axis=1) + 0)[0] == 0 and (np.sort(dist, axis=1)[:, 1] == 1).all() and (dist.max(axis=1) <= 2).all()
    for name in ("near_perms", "near_perms_32slots"):
        f = entries_of(tables[name])[0]["frame"]
        assert len(f) == 24 and len({tuple(sorted(x.tolist())) for x in f}) == 1 and len({bytes(x) for x in f}) == 24
    for name in ("near_sparse", "near_sparse_16slots"):
        f = entries_of(tables[name])[0]["frame"]
        assert len(f) == 14 and (f == 0).all(axis=1).sum() == 1 and (f == 0xFFFFFFFF).all(axis=1).sum() == 1 and ((f == 0).sum(axis=1) == 3).sum() == 12


def test_first_reads_family(tables, launches):
    ent, reads, _ = entries_of(tables["firsts_in_front"])
    repeats = np.setdiff1d(reads["seq"], ent["first_seq"])
    assert len(ent) == 5 and len(repeats) >= 15 and ent["first_seq"].max() < repeats.min()
    ent, reads, _ = entries_of(tables["firsts_behind"])
    assert len(ent) == 5 and ent["reads"][0] == 20 and (ent["reads"][1:] == 1).all() and ent["first_seq"][1:].min() > ent["last_seq"][0]
    t = tables["only_read_is_last"]
    ent = entries_of(t)[0]
    assert ent["reads"][-1] == 1 and ent["first_seq"][-1] == len(t.res) - 1 == t.wcount - 1 and len(ent) == 5
    hows = set()
    for t in tables.values():
        if t.family != "firsts":
            continue
        if t.aim.get("kind") == "cut":
            cut, r = t.aim["cut"], t.res
            ent = entries_of(t)[0]
            hows.add((np.sign(t.used - t.wcount), cut < len(r)))
            if cut < len(r):         # the first window behind the cut is a verified read of a frame read nowhere else: absent, and no overflow
                assert r["type"][cut] == 1 and r["crc_ok"][cut] == 1 and bytes(r["bits"][cut]) not in {bytes(f) for f in ent["frame"]}
                assert len(ent) == t.max_tags == 5 and cut == min(t.wcount, t.used)
                whole = tracks_ref.expected(inventory_ref.dumps_of_table(r, len(r), len(r)), t.start)[0]
                assert len(whole) == t.max_tags + 1 and whole["first_seq"][-1] == cut and whole["reads"][-1] == 1
            else:
                assert len(ent) == 6 == t.max_tags
        if t.aim.get("kind") == "zero":
            assert len(entries_of(t)[0]) == 0 and min(t.wcount, t.used) <= 0 and (t.res["crc_ok"] == 1).sum() > 20
            hows.add(("zero", t.wcount == 0, t.used <= 0))
    assert {(-1, True), (1, True), (0, True), (1, False)} <= hows and {("zero", True, False), ("zero", False, True), ("zero", True, True)} <= hows
    g = [g for g in launches["firsts"] if "no_verified_read" in g.names][0]
    k = g.names.index("no_verified_read")
    assert g.want["counts"][k - 1] > 0 and g.want["counts"][k] == 0 and g.want["counts"][k + 1] > 0 and g.want["overflow"][k] == 0
    assert g.want["ent_off"][k] == g.want["ent_off"][k + 1] and g.want["base"][k] == g.want["base"][k + 1]


def test_strongest_read_family(tables):
    kinds = set()
    for t in tables.values():
        if t.family != "strongest":
            continue
        ent, reads, _ = entries_of(t)
        assert len(ent) == 2
        for e in range(2):
            seq, norm = norms_of(t, ent, reads, e)
            assert not np.isnan(norm).any()
            top = np.flatnonzero(norm == norm.max())
            assert ent["best_seq"][e] == seq[top[0]]
            where = "first" if top[0] == 0 else ("last" if top[0] == len(seq) - 1 else "middle")
            kinds.add((t.aim["kind"], where, "tie" if len(top) > 1 else "single"))
            if t.aim["kind"] == "tie":
                assert len(top) == 7 and len({(a, b) for a, b in zip(reads["h_re"][reads["entry"] == e][top].view(np.uint32).tolist(),
                                                                        reads["h_im"][reads["entry"] == e][top].view(np.uint32).tolist())}) == 7
                assert norm.max() == 25.0 and (ent["last_seq"][e] > seq[top[-1]] or t.name == "tie_all_equal" or e == 1)
            if t.aim["kind"] == "ulp":
                s = np.sort(np.unique(norm).view(np.int32))
                assert len(s) == 2 and s[1] - s[0] == 1
            if t.aim["kind"] == "zero":
                assert (norm == 0.0).all() and len(norm) == 4 and (reads["h_re"][reads["entry"] == e] != 0).any()
            if t.aim["kind"] == "inf":
                assert np.isposinf(norm.max()) and len(top) >= 2 and np.isfinite(norm).any()
    assert {("tie", "first", "tie"), ("tie", "middle", "tie"), ("max", "first", "single"), ("max", "middle", "single"), ("max", "last", "single"),
            ("ulp", "middle", "single"), ("ulp", "first", "tie"), ("zero", "first", "tie"), ("inf", "middle", "tie")} <= kinds, kinds


def share16(nw):
    """the windows per wave as tracks_kernel divides a trace among sixteen (to check the aims with)"""
    return (((nw + 15) // 16) + 63) & ~63


def test_lanes_and_waves_family(tables):
    for name, per in (("batch_of_32_entries", 32), ("batch_of_64_entries", 64)):
        reads = entries_of(tables[name])[1]
        b = reads[(reads["seq"] >= 64) & (reads["seq"] < 128)]
        assert len(b) == per == len(set(b["entry"].tolist())) and tables[name].max_tags == 64          # `per` turns of the ballot loop
        assert ((reads["seq"] < 64).sum()) == 5
    for name, per in (("batch_of_one_entry_32", 32), ("batch_of_one_entry_64", 64)):
        ent, reads, _ = entries_of(tables[name])
        b = reads[(reads["seq"] >= 64) & (reads["seq"] < 128)]
        assert len(b) == per and len(set(b["entry"].tolist())) == 1 and len(ent) == 3
        assert (per < 64) or set(b["seq"].tolist()) == set(range(64, 128))                             # a full mask: lane 63 counts 63 lanes
        assert ent["reads"][b["entry"][0]] > per and ent["first_seq"][b["entry"][0]] < 64              # (the cursor does not start at the batch)
    t = tables["every_wave_and_last_wave"]
    ent, reads, _ = entries_of(t)
    per = share16(len(t.res))
    assert per == 256 and len(t.res) == 16 * per
    in_waves = [set((reads["seq"][reads["entry"] == e] // per).tolist()) for e in range(len(ent))]
    assert set(range(16)) in in_waves and {15} in in_waves and {0} in in_waves and {7} in in_waves
    seen = set()
    for nw in ic.NW_LIST:
        t = tables["nw%d" % nw]
        ent, reads, _ = entries_of(t)
        assert len(t.res) == nw and len(ent) == min(6, nw // 2) and len(reads) >= 0.39 * nw
        per = share16(nw)
        lens = [max(0, min(nw, (w + 1) * per) - min(nw, w * per)) for w in range(16)]
        seen |= {"range empty" if n == 0 else ("range of one" if n == 1 else ("range full" if n == per else "range cut")) for n in lens}
        seen.add("one wave: %s" % ("one turn" if nw <= 64 * ic.INV_UNROLL else "more turns"))
        seen.add("sixteen, inventory: %s" % ("one turn" if nw <= 1024 * ic.INV_UNROLL else "more turns"))
        seen.add("sixteen, tracks: %s" % ("one turn" if per <= 64 * ic.INV_UNROLL else "more turns"))
    assert seen == {"range empty", "range of one", "range full", "range cut", "one wave: one turn", "one wave: more turns",
                    "sixteen, inventory: one turn", "sixteen, inventory: more turns", "sixteen, tracks: one turn", "sixteen, tracks: more turns"}


def test_capacity_family(launches):
    (g,) = launches["capacity"]
    total = int(g.want["reads_head"][0])
    assert 0 < g.cap < total < g.reads_len and len(g.names) == 2 and g.want["base"][1] < g.cap        # (the capacity ends inside the second trace)
    out = ic.expected_outputs(g)
    assert out["reads"][: g.cap].tobytes() == g.want["reads"][: g.cap].tobytes()
    assert (out["reads"][g.cap:].view(np.int32) == ic.PREFILL).all()


def test_batches_family(launches):
    gs = launches["batches"]
    assert {len(g.res) for g in gs} == set(ic.BATCH_SIZES)
    shares, places = set(), set()
    for g in gs:
        n = len(g.res)
        assert g.res.shape[1] == 8 and g.aim["n"] == n
        nthr = min(1024, (n + 63) & ~63)
        per = (n + nthr - 1) // nthr
        shares.add((per, "empty shares" if per * (nthr - 1) >= n else "all busy"))
        over = np.flatnonzero(g.want["overflow"]).tolist()
        assert over == sorted(g.aim["over"]) and g.want["head"][1] == (over[0] if over else inventory_ref.NO_TRACE)
        assert (g.want["counts"][over] == 0).all()
        if n >= 63:
            assert set(g.want["counts"].tolist()) == {0, 1, 2, 3, 4}
        for k in over:
            places.add("first" if k == 0 else ("last" if k == n - 1 else "middle"))
        if len(over) > 1:
            places.add("several")
        if not over:
            places.add("none")
        assert np.array_equal(g.want["ent_off"], np.cumsum(g.want["counts"]) - g.want["counts"])
        reads_per = np.array([sum(int(e["reads"].sum()) for e in [p]) for p in g.want["per"]])
        assert np.array_equal(g.want["base"], np.cumsum(reads_per) - reads_per) and g.want["reads_head"][0] == reads_per.sum()
    assert {(1, "all busy"), (1, "empty shares"), (2, "empty shares"), (3, "empty shares")} <= shares, shares
    assert places == {"first", "last", "middle", "several", "none"}


def test_random_family(tables):
    ts = [t for t in tables.values() if t.family == "random"]
    assert len(ts) == ic.N_RANDOM
    kinds = {"fits": 0, "count": 0}
    ds = []
    for t in ts:
        d = len(entries_of(t)[0])
        ds.append(d)
        assert d <= t.slots
        kinds["count" if d > t.max_tags else "fits"] += 1
    assert min(ds) == 0 and max(ds) == 40 and kinds["fits"] > 100 and kinds["count"] >= 15, kinds
    assert len({t.slots for t in ts}) >= 6 and 1024 in {t.slots for t in ts}


# ---- 3. the kernels ------------------------------------------------------------------------------------------------------------
def test_the_emulators_share(launches):
    names = {n for gs in launches.values() for g in gs for n in g.names}
    every = {t.name for t in ic.crafted()}
    assert {n for n in every if not n.startswith("nw")} <= names and {"nw%d" % n for n in ic.NW_EMU} <= names
    assert len([n for n in names if n.startswith("random")]) == ic.N_RANDOM // ic.RANDOM_EMU_EVERY and set(launches) == set(ic.FAMILIES)


@pytest.mark.parametrize("family", ic.FAMILIES)
@pytest.mark.parametrize("waves", ic.WAVES)
def test_kernels_on_the_emulator(emu_mod, launches, waves, family):
    for g in launches[family]:
        if waves in ic.emu_waves(g):
            ic.check(emu_mod.inventory_selftest, g, waves)


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


def test_kernels_through_the_c_call(capi_ctx, launches):
    """rfid_selftest_inventory of csrc/rfid_capi.hip on the stand-in runtime: the entry's host code and its choice of instantiation"""
    gs = launches["firsts"] + launches["strongest"] + launches["capacity"] + [g for g in launches["counts"] if g.max_tags in (64, 65)]
    gs += [g for g in launches["batches"] if len(g.res) == 65]
    assert len(gs) >= 8
    for g in gs:
        for waves in ic.WAVES:
            ic.check(capi_ctx.selftest_inventory, g, waves)
    g = launches["strongest"][0]
    ok = dict(waves=1, max_tags=g.max_tags, slots=g.slots, reads_cap=g.cap, reads_len=g.reads_len)
    for bad, status in ((dict(waves=0), capi.ERR_INVALID), (dict(waves=4), capi.ERR_INVALID), (dict(waves=17), capi.ERR_INVALID),
                        (dict(slots=1), capi.ERR_INVALID), (dict(slots=6), capi.ERR_INVALID), (dict(slots=2048), capi.ERR_INVALID),
                        (dict(max_tags=0), capi.ERR_INVALID), (dict(max_tags=513), capi.ERR_UNSUPPORTED),
                        (dict(reads_cap=-1), capi.ERR_INVALID), (dict(reads_len=g.cap - 1), capi.ERR_INVALID)):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(capi.RfidError) as e:
            capi_ctx.selftest_inventory(g.res, g.wcount, g.used, g.start, **kw)
        assert e.value.status == status, (bad, e.value.status)
    for wc in (g.wcount + g.res.shape[1], -1 - g.wcount):           # counts past the rows, negative counts
        with pytest.raises(capi.RfidError) as e:
            capi_ctx.selftest_inventory(g.res, wc, g.used, g.start, **ok)
        assert e.value.status == capi.ERR_INVALID
    lib = capi_ctx._lib
    assert lib.rfid_selftest_inventory(capi_ctx._h, *([None] * 4), 1, 8, 1, 4, 8, 8, 8, *([None] * 10)) == capi.ERR_INVALID

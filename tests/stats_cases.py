"""Crafted result tables for stream_stats_kernel by itself (TEST INFRASTRUCTURE; tests/test_stats_emu.py runs them on the
emulator and asserts what each family reaches, tests/test_gpu_stats.py runs them on the device).  A table holds
rfid_decode_result records as the decoders write them -- type = seq & 1, an RN16 record with crc_ok 0 and tag_id -1, an EPC
record with tag_id 0..255 when its CRC holds and -1 when not -- with seeded noise (any bit pattern, NaNs included) in every
field the kernel has no business reading.  The expected statistics are tests/stats_ref.py's window-by-window replay, nothing
else: where this module counts or locates windows itself it only AIMS a limit at a window, and test_stats_emu.py then asserts
from the replay that the cut fell there.

Three kinds of table step outside what a decoder writes, because the kernel takes a window's type from its record and not
from its index: `inv` tables (type = (seq + 1) & 1) put an EPC window on even indices -- the first window of a wave's share and lane 0
of a 64-window batch are even -- and `lead` tables begin with RN16 records only, so that the deciding EPC window lies in a wave
behind waves that hold none; `stale` tables carry a good CRC and a tag id on RN16 records, which only the type keeps from
counting.  The replay is defined on any sequence of records.

Cases that share a limit triple (max_slot_number, max_num_queries, number_unique_tags) are stacked into one launch, one table
per workgroup, ragged, the row length odd; the records of a row behind its count are good reads of tag 0xAB, which must not
be looked at."""
from collections import namedtuple

import numpy as np

import stats_ref
from rfid import _capi as capi

NO_Q = 2 ** 31 - 2          # a queries limit no table reaches
NO_U = 256                  # a distinct-id limit no table exceeds: there are 256 ids
SLOTS = 16                  # max_slot_number where the family is not about it
WAVE_COUNTS = (1, 4, 16)    # the emulator's; the device runs 1 and 16, the product's two shapes
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1087, 1088, 2047, 2049)
LONG = (17413, 16 * 1088)   # a sixteenth exceeds 1024: more than one turn of either loop per wave
IDS_READ = (1, 2, 63, 64, 65, 100, 101, 255, 256)
UNIQUE_LIMITS = (0, 1, 63, 64, 65, 100, 255, 256)
POISON_ID = 0xAB
PREFILL = -0x12345679       # every word of the output rows in front of a launch

Case = namedtuple("Case", "name family res limits want aim emu")
Group = namedtuple("Group", "limits names res wcount want families")


def share(nw, waves):
    """the windows per wave as the kernel divides a trace (to aim with: first and last window of a wave's share)"""
    return (((nw + waves - 1) // waves) + 63) & ~63


# ---- records ----------------------------------------------------------------------------------------------------------
def records(rng, types, crc_ok, tag_id):
    n = len(types)
    r = np.zeros(n, dtype=capi.RESULT_DTYPE)
    types = np.asarray(types, dtype=np.int32)
    r["type"] = types
    r["index"] = rng.integers(-2 ** 31, 2 ** 31, n)
    for f in ("h_re", "h_im", "T"):
        r[f] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r["bits"] = rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    r["n_bits"] = np.where(types == 1, 128, 16)
    r["crc_ok"] = crc_ok
    r["tag_id"] = tag_id
    return r


def alt(nw):
    return np.arange(nw, dtype=np.int32) & 1


def inv(nw):
    return (np.arange(nw, dtype=np.int32) + 1) & 1


def id_table(rng, types, ids, p_fail=0.3, lead_fail=0):
    """A table whose EPC windows read exactly `ids`, first reads in the order given, one in each of len(ids) equal stretches of
    the EPC windows (so they spread over every wave's share), behind `lead_fail` CRC-failed EPC windows; every other EPC window
    fails with p_fail or else repeats an id already read"""
    types = np.asarray(types, dtype=np.int32)
    nw = len(types)
    crc = np.zeros(nw, dtype=np.int32)
    tid = np.full(nw, -1, dtype=np.int32)
    epc = np.flatnonzero(types == 1)[lead_fail:]
    assert len(epc) >= len(ids), (len(epc), len(ids))
    firsts = {}
    if len(ids):
        edges = np.linspace(0, len(epc), len(ids) + 1).astype(int)
        for j, i in enumerate(ids):
            firsts[int(epc[rng.integers(edges[j], edges[j + 1])])] = int(i)
    seen = []
    for k in epc.tolist():
        if k in firsts:
            crc[k], tid[k] = 1, firsts[k]
            seen.append(firsts[k])
        elif seen and rng.random() >= p_fail:
            crc[k], tid[k] = 1, seen[int(rng.integers(0, len(seen)))]
    return records(rng, types, crc, tid)


def pick_ids(rng, m, must=(), never=()):
    pool = [i for i in range(256) if i not in must and i not in never]
    ids = list(must) + [int(i) for i in rng.permutation(pool)[: m - len(must)]]
    return [int(i) for i in rng.permutation(ids)]


def epc_through(res, t):
    """EPC windows among res[0 .. t]: the queries limit that makes window t the deciding one (to aim with)"""
    return int((res["type"][: t + 1] & 1).sum())


# ---- expected rows ----------------------------------------------------------------------------------------------------
def want_row(st):
    row = np.zeros(1, dtype=capi.STATS_DTYPE)
    for f in ("n_queries_sent", "cur_inventory_round", "cur_slot_number", "n_epc_correct", "n_unique_tags", "n_windows",
              "n_windows_used", "status"):
        row[f] = getattr(st, f)
    for i, n in st.tag_reads.items():
        assert 0 <= i < 256
        row["tag_reads"][0, i] = n
    return row[0]


def case(name, family, res, limits, aim=None, emu=True):
    st = stats_ref.replay(stats_ref.windows_of(res), *limits)
    return Case(name, family, res, tuple(int(v) for v in limits), st, aim or {}, emu)


def cuts(c):
    """(k_q, k_u) of a case from the replay with one limit at a time: the index of the first window not decoded, None where
    that limit does not end the run inside or at the end of the trace"""
    w = stats_ref.windows_of(c.res)
    q = stats_ref.replay(w, c.limits[0], c.limits[1], 1 << 40)
    u = stats_ref.replay(w, c.limits[0], 1 << 40, c.limits[2])
    return (q.n_windows_used if q.status else None), (u.n_windows_used if u.status else None)


# ---- the families -----------------------------------------------------------------------------------------------------
def lengths(rng):
    out = []
    for nw in LENGTHS + LONG:
        e = nw // 2
        res = id_table(rng, alt(nw), pick_ids(rng, min(5, e)))
        out.append(case("len%d" % nw, "lengths", res, (SLOTS, NO_Q, NO_U)))
        # the last EPC window decides: on an even length it is the trace's last window (no cut, yet TERMINATED), on an odd one
        # the cut leaves the RN16 window behind it out; and one EPC window short of the limit: RUNNING
        out.append(case("len%d_q_last" % nw, "lengths", res, (SLOTS, e, NO_U), emu=nw in LENGTHS or nw == LONG[0]))
        out.append(case("len%d_q_short" % nw, "lengths", res, (SLOTS, e + 1, NO_U), emu=nw in LENGTHS))
    return out


def query_targets(nw):
    """window indices to aim the queries limit at -> {index: [(waves, wave, 'first' | 'last')] + [('lane', 0 | 63)]}"""
    t = {}
    for waves in WAVE_COUNTS:
        seg = share(nw, waves)
        busy = [w for w in range(waves) if w * seg < nw]
        for w in sorted({busy[0], busy[len(busy) // 2], busy[-1]}):
            k0, k1 = w * seg, min(w * seg + seg, nw)
            t.setdefault(k0, []).append((waves, w, "first"))
            t.setdefault(k1 - 1, []).append((waves, w, "last"))
    for b in (0, 7, (nw - 64) // 64):
        t.setdefault(64 * b, []).append(("lane", 0))
        t.setdefault(64 * b + 63, []).append(("lane", 63))
    for k in (255, 256, 1023, 1024):                      # the turns of the result loop and of the summary loop
        if k < nw:
            t.setdefault(k, []).append(("turn", k))
    return t


def queries(rng):
    out = []
    for nw, emu_every in ((2500, 1), (LONG[0], 6), (LONG[1], 6)):
        tabs = {1: id_table(rng, alt(nw), pick_ids(rng, 7)), 0: id_table(rng, inv(nw), pick_ids(rng, 7))}
        for n, (t, where) in enumerate(sorted(query_targets(nw).items())):
            res = tabs[t & 1]                             # the table in which window t is an EPC window
            out.append(case("q%d_at%d" % (nw, t), "queries", res, (SLOTS, epc_through(res, t), NO_U),
                            aim=dict(deciding=t, where=where), emu=(n % emu_every == 0)))
    res = id_table(rng, alt(300), pick_ids(rng, 4))
    for q in (0, 1, NO_Q):
        out.append(case("q_limit_%d" % q, "queries", res, (SLOTS, q, NO_U)))
    # the deciding EPC window in a wave behind waves that hold none: RN16 records only up to window 1000
    types = alt(2500)
    types[:1000] = 0
    res = id_table(rng, types, pick_ids(rng, 6))
    for q in (1, 5, 300):
        out.append(case("q_lead_%d" % q, "queries", res, (SLOTS, q, NO_U), aim=dict(lead=1000)))
    return out


def unique_tables(rng):
    tabs = []
    for m in IDS_READ:
        # (id 255 is in the tables of 101 ids and more, not in those below: a failed read's tag_id -1 must not count for it)
        ids = pick_ids(rng, m, must=(255,) if m >= 101 else (), never=() if m >= 101 else (255,))
        tabs.append(("ids%d" % m, id_table(rng, alt(3001), ids), dict(ids=m)))
    tabs.append(("fail_first", id_table(rng, alt(801), pick_ids(rng, 12, never=(255,)), p_fail=0.5, lead_fail=40), dict(lead_fail=40)))
    tabs.append(("only255", id_table(rng, alt(401), [255], p_fail=0.5, lead_fail=3), dict(lead_fail=3)))
    for q in range(4):        # the second id read lies in the kernel's group q of ids (lane + 64 q)
        ids = [int(rng.integers(0, 256)), 64 * q + int(rng.integers(0, 64))]
        while ids[0] == ids[1]:
            ids[0] = int(rng.integers(0, 256))
        rest = [i for i in pick_ids(rng, 10) if i not in ids][:6]
        tabs.append(("second_in_group%d" % q, id_table(rng, alt(401), ids + rest), dict(group=q, second=ids[1])))
    # the second id's first read on the trace's last window: with a limit of one id the count passes it behind the last window
    # (no cut, yet TERMINATED)
    head = id_table(rng, alt(398), [17])
    tail = records(rng, [0, 1], [0, 1], [-1, 201])
    tabs.append(("second_on_last", np.concatenate([head, tail]), dict(on_last=201)))
    return tabs


def unique(rng):
    out = []
    for name, res, aim in unique_tables(rng):
        for n in UNIQUE_LIMITS:
            out.append(case("%s_u%d" % (name, n), "unique", res, (SLOTS, NO_Q, n), aim=aim))
    return out


def both(rng):
    """the queries limit in front of, behind and on the window of the (N + 1)-th id's first read"""
    out = []
    for m, n in ((65, 10), (256, 100)):
        res = id_table(rng, alt(3001), pick_ids(rng, m))
        k_u = stats_ref.replay(stats_ref.windows_of(res), SLOTS, 1 << 40, n).n_windows_used
        at = epc_through(res, k_u - 1)
        for rel, q in (("lt", at - 7), ("eq", at), ("gt", at + 7)):
            out.append(case("both%d_%s" % (m, rel), "both", res, (SLOTS, q, n), aim=dict(rel=rel)))
    return out


def slots(rng):
    out = []
    small = list(range(0, 8)) + list(range(30, 36))                                # EPC counts 0..3 and 15..17
    tabs = [(nw, id_table(rng, alt(nw), pick_ids(rng, min(3, nw // 2)))) for nw in small]
    for ms in (1, 2, SLOTS, 32768):
        for nw, res in tabs:
            out.append(case("slot%d_len%d" % (ms, nw), "slots", res, (ms, NO_Q, NO_U)))
    big = id_table(rng, alt(2 * 32769 + 1), pick_ids(rng, 9))
    for e in (32767, 32768, 32769):
        out.append(case("slot32768_epc%d" % e, "slots", big[: 2 * e + 1], (32768, NO_Q, NO_U), emu=(e == 32768)))
    return out


def stale(rng):
    """Outside what a decoder writes, as `inv` and `lead` are: RN16 records that carry crc_ok = 1 and a tag id, as a record slot
    reused without being cleared would.  The CRC flag and the id count on an EPC record only (tag_decoder_impl.cc:291,327): the
    ids of those RN16 records are never read, none of them starts an id or moves the cut"""
    out = []
    res = id_table(rng, alt(1201), [i for i in pick_ids(rng, 30) if i >= 32][:6])
    rn16 = np.flatnonzero(res["type"] == 0)
    hit = rn16[rng.random(len(rn16)) < 0.5]
    res["crc_ok"][hit] = 1
    res["tag_id"][hit] = rng.integers(0, 32, len(hit))
    for n in (0, 1, 5, 256):
        out.append(case("stale_rn16_u%d" % n, "stale", res, (SLOTS, NO_Q, n)))
    return out


BATCH_LIMITS = (4, 51, 6)
BATCH_LENGTHS = (0, 333, 5, 131, 1029, 64, 777, 1500)


def batch(rng):
    """eight ragged traces under one triple of their own: with the odd row length the summary rows start at every alignment"""
    out = []
    for s, nw in enumerate(BATCH_LENGTHS):
        res = id_table(rng, alt(nw), pick_ids(rng, min(3 + 2 * s, nw // 2)))
        out.append(case("batch%d_len%d" % (s, nw), "batch", res, BATCH_LIMITS))
    return out


N_RANDOM = 300
RANDOM_Q = (0, 3, 40, 300)
RANDOM_U = (0, 2, 20, 100)
RANDOM_SLOTS = (1, 2, SLOTS, 32768)


def random_tables(seed=20240611):
    """nw log-uniform in 0..3000, 0..256 ids; a table's limits come from a menu of nine triples, so that about a third of
    the tables are cut by the queries limit, a third by the distinct-id limit and a third not at all (a table too short for the
    kind it was drawn for takes the next kind)"""
    rng = np.random.default_rng(seed)
    out = []
    for n in range(N_RANDOM):
        nw = int(np.exp(rng.uniform(0.0, np.log(3001.0)))) - 1 if n % 10 else int(rng.integers(1500, 3001))
        e = nw // 2
        m = min(int(rng.integers(0, 257)), e)
        res = id_table(rng, alt(nw), pick_ids(rng, m), p_fail=float(rng.uniform(0.0, 0.6)))
        w = stats_ref.windows_of(res)
        menu = {"q": [(RANDOM_SLOTS[i], q, NO_U) for i, q in enumerate(RANDOM_Q)],
                "u": [(RANDOM_SLOTS[i], NO_Q, u) for i, u in enumerate(RANDOM_U)],
                "none": [(SLOTS, NO_Q, NO_U)]}
        chosen = None
        for kind in (("q", "u", "none"), ("u", "q", "none"), ("none",))[n % 3]:
            fits = [lim for lim in menu[kind] if kind == "none" or stats_ref.replay(w, *lim).n_windows_used < nw]
            if fits:
                chosen = (kind, fits[int(rng.integers(0, len(fits)))])
                break
        out.append(case("random%d_%s_len%d" % (n, chosen[0], nw), "random", res, chosen[1], aim=dict(kind=chosen[0]), emu=(n % 10 == 0)))
    return out


def crafted(seed=20240610):
    rng = np.random.default_rng(seed)
    out = []
    for fam in (lengths, queries, unique, both, slots, batch, stale):
        out += fam(rng)
    return out


# ---- launches ---------------------------------------------------------------------------------------------------------
def groups(cases):
    """cases of one limit triple (and one size class) -> one launch: [n][wmax] records, wmax odd, rows padded with poison"""
    by = {}
    for c in cases:
        size = 0 if len(c.res) <= 3100 else (1 if len(c.res) <= 20000 else 2)
        by.setdefault((c.limits, size), []).append(c)
    out = []
    for (limits, _), cs in by.items():
        wmax = max(1, max(len(c.res) for c in cs)) | 1
        res = np.zeros((len(cs), wmax), dtype=capi.RESULT_DTYPE)
        res["type"], res["crc_ok"], res["tag_id"], res["n_bits"] = 1, 1, POISON_ID, 128
        for s, c in enumerate(cs):
            res[s, : len(c.res)] = c.res
        out.append(Group(limits, [c.name for c in cs], res, np.array([len(c.res) for c in cs], dtype=np.int32),
                         np.array([want_row(c.want) for c in cs], dtype=capi.STATS_DTYPE), sorted({c.family for c in cs})))
    return out


def row_alignments(g):
    """byte offset modulo 16 of each row of the group's summary array (the array itself is 256-byte aligned)"""
    return [(4 * s * g.res.shape[1]) % 16 for s in range(len(g.names))]


def check(run, g, waves, from_summaries):
    """run(results, wcount, waves, from_summaries, max_slot_number, max_num_queries, number_unique_tags, out) -> rows.  The output
    starts from PREFILL words with a guard row behind the traces: every word of every trace's row must come back as the
    replay's, the guard as it was."""
    n = len(g.names)
    pre = np.full((n + 1) * capi.STATS_DTYPE.itemsize // 4, PREFILL, dtype=np.int32).view(capi.STATS_DTYPE)
    got = run(g.res, g.wcount, waves, from_summaries, *g.limits, out=pre)
    assert len(got) == n + 1
    for s in range(n):
        if got[s].tobytes() != g.want[s].tobytes():
            diff = {f: (got[s][f].tolist(), g.want[s][f].tolist()) for f in capi.STATS_DTYPE.names
                    if f != "tag_reads" and got[s][f] != g.want[s][f]}
            ids = np.flatnonzero(got[s]["tag_reads"] != g.want[s]["tag_reads"])
            raise AssertionError("%s, limits %s, %d waves, %s: (got, want) %s; tag_reads differ at ids %s" % (
                g.names[s], g.limits, waves, "summaries" if from_summaries else "records", diff, ids[:8].tolist()))
    assert got[n].tobytes() == pre[n].tobytes(), "the row behind the last trace was written"

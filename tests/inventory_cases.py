"""Crafted result tables for the inventory and the tracks kernels by themselves (TEST INFRASTRUCTURE; tests/test_inventory_tables_emu.py
runs them on the emulator and asserts what each family reaches, tests/test_gpu_inventory_tables.py runs them on the device).  A table
holds rfid_decode_result records as the decoders write them -- type = seq & 1, tag_id = frame bits 104..111 when the CRC holds and -1
when not -- and around the verified reads everything stage_fetch must not act on: seeded noise of any bit pattern (NaNs included) in
the other fields of every record that is no verified read, CRC-failed EPC records that carry the bits of frames read elsewhere in the
table, RN16 records with a stale crc_ok = 1, an id and the bits of a real frame.  A verified read carries finite h_est (the header
leaves NaN undefined), any T and any index.

Two kinds of table step outside what a decoder writes: `all-EPC` tables (type = 1 on every seq), because only they put 64 reads into
one 64-window batch of the tracks kernel, and the rows of a launch behind their wcount, which hold verified reads of a frame of their
own that must not be looked at.

The expected entries and reads are tests/inventory_ref.py's and tests/tracks_ref.py's, from the records alone (tracks_ref.expected_tables);
they never use the kernels' hash.  inv_hash below RESTATES the kernels' hash to BUILD inputs only: frames that share a probe sequence,
frames that start on it.  Where this module counts rounds or probes it only aims; test_inventory_tables_emu.py asserts what was reached.

Tables that share (max_tags, slots, size class) are stacked into one launch, one table per workgroup, ragged; every launch runs in both
workgroup shapes, one wave and sixteen per trace.  The device runs everything.  The emulator runs NW_EMU of the lengths, every fifth
random table, and of the batches of a thousand traces and more one launch per size, with one wave per trace only (emu_waves): sixteen
waves are 1 024 fibers per trace there, and the offsets scans those batches are about do not depend on the shape."""
import functools
from collections import namedtuple

import numpy as np

import tracks_ref
from rfid import _capi as capi

PREFILL = -0x12345679       # every word of every output array in front of a launch
WAVES = (1, 16)             # the product's two workgroup shapes
COUNTS_D = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512)
FULL_D = (2, 4, 64, 128, 512)
OVERFULL_D = (3, 5, 129)
NW_LIST = (63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8193)
NW_EMU = (63, 64, 65, 255, 256, 257, 1023, 1025, 4097)          # the emulator's share of NW_LIST
BATCH_SIZES = (1, 63, 64, 65, 1024, 1025, 2049)
N_RANDOM = 200
RANDOM_EMU_EVERY = 5        # the emulator's share of the random tables: every fifth
INV_UNROLL = 4              # (the kernels': 64-window batches in flight per wave -- to aim the lengths with)

Table = namedtuple("Table", "name family res wcount used start max_tags slots aim emu")
Launch = namedtuple("Launch", "names family res wcount used start max_tags slots cap reads_len want aim emu")
POISON_FRAME = np.array([0xDEADBEEF, 0x0BADF00D, 0xFEEDFACE, 0x8BADF00D], dtype=np.uint32)


# ---- the kernels' hash, restated to build inputs (never to form an expectation) -------------------------------------
def inv_hash(frames, mask):
    """[n][4] uint32 frames -> (h0, step) of their probe sequences slot_i = (h0 + i * step) & mask"""
    f = np.asarray(frames, dtype=np.uint32).reshape(-1, 4)
    h = (f[:, 0] * np.uint32(0x9E3779B1)) ^ (f[:, 1] * np.uint32(0x85EBCA77)) ^ (f[:, 2] * np.uint32(0xC2B2AE3D)) ^ (f[:, 3] * np.uint32(0x27D4EB2F))
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x2C1B3C6D)
    h = h ^ (h >> np.uint32(12))
    return (h & np.uint32(mask)).astype(np.int64), (((h >> np.uint32(16)) & np.uint32(mask)) | np.uint32(1)).astype(np.int64)


def default_slots(max_tags):
    """the table a plan gives max_tags: the smallest power of two >= 2 max_tags"""
    s = 2
    while s < 2 * max_tags:
        s *= 2
    return s


@functools.lru_cache(maxsize=None)
def _chain(seed, mask, n, n_block):
    """a seeded search: n frames that share h0 and step under `mask`, and n_block other frames whose h0 lies on the first n slots of
    that probe sequence (with another step)"""
    rng = np.random.default_rng(seed)
    chunk = 1 << 21
    f = rng.integers(0, 2 ** 32, (chunk, 4), dtype=np.uint64).astype(np.uint32)
    h0, st = inv_hash(f, mask)
    key = h0 * (mask + 1) + st
    target = np.bincount(key).argmax()                    # (the fullest bucket of the first draw: a head start)
    found = [f[key == target]]
    while sum(len(x) for x in found) < n:
        f = rng.integers(0, 2 ** 32, (chunk, 4), dtype=np.uint64).astype(np.uint32)
        h0, st = inv_hash(f, mask)
        found.append(f[h0 * (mask + 1) + st == target])
    chain = np.concatenate(found)[:n]
    c0, cs = int(target // (mask + 1)), int(target % (mask + 1))
    on_chain = (c0 + np.arange(n) * cs) & mask
    f = rng.integers(0, 2 ** 32, (1 << 18, 4), dtype=np.uint64).astype(np.uint32)
    h0, st = inv_hash(f, mask)
    block = f[np.isin(h0, on_chain) & (st != cs)][:n_block]
    assert len(chain) == n and len(block) == n_block
    return chain, block


def chain_frames(mask, n, n_block=0):
    chain, block = _chain(20240915 + mask, mask, n, n_block)
    return chain.copy(), block.copy()


# ---- records ---------------------------------------------------------------------------------------------------------
def alt(nw):
    return np.arange(nw, dtype=np.int32) & 1


def tag_id_of(frames):
    """frame bits 104..111, MSB first (rfid_decode_result::tag_id)"""
    w3 = np.asarray(frames, dtype=np.uint32).reshape(-1, 4)[:, 3].astype(np.int64)
    return sum(((w3 >> (8 + i)) & 1) << (7 - i) for i in range(8)).astype(np.int32)


def rand_frames(rng, d):
    while True:
        f = rng.integers(0, 2 ** 32, (d, 4), dtype=np.uint64).astype(np.uint32)
        if len({bytes(x) for x in f}) == d:
            return f


def finite_h(rng, n):
    """finite h_est over thirty binades, both signs"""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 4, n)).astype(np.float32)


def records(rng, frames, on, types=None, h=None):
    """on[k]: the frame (index into frames) window k reads with a verified CRC, -1: none.  Everything else is filled as the header says"""
    on = np.asarray(on, dtype=np.int64)
    nw = len(on)
    types = alt(nw) if types is None else np.asarray(types, dtype=np.int32)
    frames = np.asarray(frames, dtype=np.uint32).reshape(-1, 4)
    r = rng.integers(0, 2 ** 32, (nw, 12), dtype=np.uint64).astype(np.uint32).view(capi.RESULT_DTYPE).reshape(nw)
    assert (types[on >= 0] == 1).all()
    r["type"] = types
    r["n_bits"] = np.where(types == 1, 128, 16)
    hit = on >= 0
    r["crc_ok"] = hit
    r["tag_id"] = -1
    if len(frames):
        lend = rng.integers(0, len(frames), nw)
        borrowed = ~hit & (rng.random(nw) < 0.6)                        # failed EPC and RN16 records with the bits of a real frame
        r["bits"][borrowed] = frames[lend[borrowed]]
        stale = borrowed & (types == 0)
        r["crc_ok"][stale] = 1
        r["tag_id"][stale] = tag_id_of(frames[lend[stale]])
        r["bits"][hit] = frames[on[hit]]
        r["tag_id"][hit] = tag_id_of(frames[on[hit]])
    n = int(hit.sum())
    r["h_re"][hit], r["h_im"][hit] = finite_h(rng, n), finite_h(rng, n)
    if h is not None:
        hh = np.asarray(h, dtype=np.float32).reshape(-1, 2)
        assert len(hh) == n
        r["h_re"][hit], r["h_im"][hit] = hh[:, 0], hh[:, 1]
    return r


def starts(rng, nw):
    return np.cumsum(rng.integers(347, 3000, nw)).astype(np.int32)


def spread(rng, nw, d, n_reads, types=None, skew=1.5):
    """on[] of nw windows: n_reads verified reads of d frames on random EPC windows, every frame at least once, read counts skewed"""
    types = alt(nw) if types is None else types
    epc = np.flatnonzero(types == 1)
    assert d <= n_reads <= len(epc), (d, n_reads, len(epc))
    on = np.full(nw, -1, dtype=np.int64)
    if n_reads:
        w = 1.0 / (1.0 + np.arange(d)) ** skew
        ids = np.concatenate([np.arange(d), rng.choice(d, n_reads - d, p=w / w.sum())])
        on[np.sort(rng.choice(epc, n_reads, replace=False))] = rng.permutation(ids)
    return on


def table(rng, name, family, frames, on, max_tags, slots, types=None, h=None, wcount=None, used=None, aim=None, emu=True):
    res = records(rng, frames, on, types, h)
    nw = len(res)
    return Table(name, family, res, nw if wcount is None else wcount, nw if used is None else used, starts(rng, nw), int(max_tags),
                 int(slots), aim or {}, emu)


def simple(rng, name, family, d, max_tags, slots, frames=None, nw=None, n_reads=None, **kw):
    """d frames (random ones unless given) read 1.5 d + 2 times in all, on 0.8 of the EPC windows"""
    frames = rand_frames(rng, d) if frames is None else frames
    n_reads = d + d // 2 + 2 if n_reads is None else n_reads
    nw = 2 * (n_reads + n_reads // 4 + 1) if nw is None else nw
    return table(rng, name, family, frames, spread(rng, nw, d, n_reads), max_tags, slots, **kw)


# ---- the families ------------------------------------------------------------------------------------------------------
def counts(rng):
    out = []
    for d in COUNTS_D:
        slots = default_slots(d)
        frames = rand_frames(rng, d)
        out.append(simple(rng, "count%d_fits" % d, "counts", d, d, slots, frames, aim=dict(d=d, over=None)))
        if d > 1:
            out.append(simple(rng, "count%d_over" % d, "counts", d, d - 1, slots, frames, aim=dict(d=d, over="count")))
    # 64 frames: the small tracks instantiation with rows of 64, the large one with rows of 65 (the table of 128 slots in both, and the
    # table a plan gives rows of 65)
    out.append(simple(rng, "count64_rows65", "counts", 64, 65, 128, aim=dict(d=64, over=None)))
    out.append(simple(rng, "count64_rows65_slots256", "counts", 64, 65, 256, aim=dict(d=64, over=None)))
    return out


def full_tables(rng):
    out = []
    for d in FULL_D:
        out.append(simple(rng, "full%d" % d, "full", d, d, d, aim=dict(d=d, over=None)))
    for d in OVERFULL_D:
        out.append(simple(rng, "overfull%d" % d, "full", d, d + 1, d - 1, aim=dict(d=d, over="full")))
    return out


def one_chain(rng):
    out = []
    for mask, n, n_block in ((1023, 24, 8), (127, 64, 16)):
        chain, block = chain_frames(mask, n, n_block)
        slots = mask + 1
        aim = dict(mask=mask, chain=n)

        def firsts_then_repeats(order, extra):
            """first reads in `order`, one EPC window each, then `extra` repeats of random frames"""
            seqs = list(order) + [int(x) for x in rng.choice(order, extra)]
            on = np.full(2 * len(seqs) + 1, -1, dtype=np.int64)
            on[1::2] = seqs
            return on

        ids = list(range(n))
        out.append(table(rng, "chain%d" % slots, "chain", chain, firsts_then_repeats(ids, n), n, slots, aim=dict(aim, kind="plain")))
        out.append(table(rng, "chain%d_descending" % slots, "chain", chain, firsts_then_repeats(ids[::-1], n), n, slots,
                         aim=dict(aim, kind="descending")))
        both = np.concatenate([chain, block])
        order = list(range(n, n + n_block)) + ids         # the frames that start on the chain claim their slots first
        out.append(table(rng, "chain%d_blocked" % slots, "chain", both, firsts_then_repeats(order, n), n + n_block, slots,
                         aim=dict(aim, kind="blocked", blockers=n_block)))
    return out


def near_frames(rng):
    out = []
    base = rand_frames(rng, 1)[0]
    flips = np.array([base] + [base ^ (np.uint32(1 << (j & 31)) * (np.arange(4) == (j >> 5)).astype(np.uint32)) for j in range(128)], dtype=np.uint32)
    out.append(simple(rng, "near_flips", "near", 129, 129, default_slots(129), flips, aim=dict(d=129, kind="flips")))
    import itertools
    words = rand_frames(rng, 1)[0]
    perms = np.array([words[list(p)] for p in itertools.permutations(range(4))], dtype=np.uint32)
    out.append(simple(rng, "near_perms", "near", 24, 24, default_slots(24), perms, aim=dict(d=24, kind="perms")))
    out.append(simple(rng, "near_perms_32slots", "near", 24, 24, 32, perms, aim=dict(d=24, kind="perms")))
    sparse = [[0, 0, 0, 0], [0xFFFFFFFF] * 4]
    for k in range(4):
        for v in (1, 0x80000000, int(rng.integers(2, 2 ** 31))):
            sparse.append([v if j == k else 0 for j in range(4)])
    sparse = np.array(sparse, dtype=np.uint32)
    out.append(simple(rng, "near_sparse", "near", len(sparse), len(sparse), default_slots(len(sparse)), sparse,
                      aim=dict(d=len(sparse), kind="sparse")))
    out.append(simple(rng, "near_sparse_16slots", "near", len(sparse), 16, 16, sparse[:14], n_reads=30, aim=dict(d=14, kind="sparse")))
    return out


def first_reads(rng):
    out = []
    d, mt, slots = 5, 5, 16
    frames = rand_frames(rng, d + 1)

    def on_of(seq_ids, nw=None):
        on = np.full(2 * len(seq_ids) + 1 if nw is None else nw, -1, dtype=np.int64)
        on[1:2 * len(seq_ids):2] = seq_ids
        return on

    rep = [int(x) for x in rng.integers(0, d, 20)]
    out.append(table(rng, "firsts_in_front", "firsts", frames[:d], on_of(list(range(d)) + rep), mt, slots, aim=dict(kind="front")))
    out.append(table(rng, "firsts_behind", "firsts", frames[:d], on_of([0] * 20 + list(range(1, d))), mt, slots, aim=dict(kind="behind")))
    # a frame whose only read is the last counted window (nw even: the last window is an EPC window)
    on = on_of(rep + [0, 1, 2, 3], nw=2 * 24 + 2)
    on[on == 4] = 0
    on[-1] = 4
    out.append(table(rng, "only_read_is_last", "firsts", frames[:d], on, mt, slots, aim=dict(kind="last", frame=4)))
    # a frame whose only read is the first window behind the cut, as frame number max_tags + 1: by n_windows_used, by wcount, by both
    ids = list(range(d)) + rep
    on = on_of(ids + [d] + rep)
    cut = 2 * len(ids) + 1
    assert on[cut] == d
    for how, wc, used in (("used", len(on), cut), ("wcount", cut, len(on)), ("both", cut, cut), ("used_far_behind", len(on), 10 ** 9)):
        out.append(table(rng, "behind_cut_by_%s" % how, "firsts", frames, on, mt if how != "used_far_behind" else d + 1, slots, wcount=wc, used=used,
                         aim=dict(kind="cut", how=how, frame=d, cut=min(wc, used))))
    for how, wc, used in (("wcount0", 0, len(on)), ("used0", len(on), 0), ("both0", 0, 0), ("used_negative", len(on), -5)):
        out.append(table(rng, "nothing_counts_%s" % how, "firsts", frames, on, mt, slots, wcount=wc, used=used, aim=dict(kind="zero")))
    # a trace without a verified read between two that have some (the launch stacks the family's tables in this order)
    out.append(table(rng, "some_a", "firsts", frames[:d], on_of(ids), mt, slots, aim=dict(kind="some")))
    out.append(table(rng, "no_verified_read", "firsts", frames[:d], np.full(41, -1, dtype=np.int64), mt, slots, aim=dict(kind="none")))
    out.append(table(rng, "some_b", "firsts", frames[:d], on_of(ids[::-1]), mt, slots, aim=dict(kind="some")))
    return out


def ulp_pair():
    """two h_re (h_im = 0) whose binary32 squares are neighbours"""
    x = (np.float32(1.5) + np.arange(1, 4096, dtype=np.float32) * np.float32(2.0 ** -23)).astype(np.float32)      # (x * x in [2, 4): 1.5 to 2 ulps a step)
    n = (x * x).astype(np.float32).view(np.int32)
    k = int(np.flatnonzero(np.diff(n) == 1)[0])
    return float(x[k]), float(x[k + 1])


def strongest(rng):
    out = []
    frames = rand_frames(rng, 3)
    tie = [(3, 4), (5, 0), (-5, 0), (0, -5), (4, -3), (-0.0, 5), (-5, -0.0)]
    lo, hi = ulp_pair()

    def one(name, hs, aim):
        """every h list is one frame's reads in order; a second frame's reads lie between them with norms of their own"""
        hs = [np.asarray(h, dtype=np.float32).reshape(-1, 2) for h in hs]
        ids, hh = [], []
        for j in range(max(len(h) for h in hs)):
            for f, h in enumerate(hs):
                if j < len(h):
                    ids.append(f)
                    hh.append(h[j])
        on = np.full(2 * len(ids) + 1, -1, dtype=np.int64)
        on[1::2] = ids
        out.append(table(rng, name, "strongest", frames[:len(hs)], on, 4, 8, h=np.array(hh, dtype=np.float32), aim=aim))

    weak = [(1, 1), (0.5, -2)]
    one("tie_all_equal", [tie, tie[::-1]], dict(kind="tie"))
    one("tie_behind_weaker", [weak + tie + weak, weak[:1] + tie[::-1]], dict(kind="tie"))
    one("max_first", [[(9, 9)] + weak * 3, weak * 2], dict(kind="max"))
    one("max_middle", [weak * 2 + [(9, 9)] + weak * 2, weak + [(0, -7)] + weak], dict(kind="max"))
    one("max_last", [weak * 3 + [(-9, 9)], weak * 2 + [(7, 0)]], dict(kind="max"))
    one("ulp_apart_up", [[(lo, 0), (hi, 0), (lo, 0)], [(0, hi), (0, lo)]], dict(kind="ulp"))
    one("ulp_apart_down", [[(hi, 0), (lo, 0), (hi, 0)], [(0, -lo), (0, -hi), (0, hi)]], dict(kind="ulp"))
    tiny = [(1e-30, 1e-30), (-3e-25, 1e-38), (1e-23, 0), (0.0, -0.0)]
    one("norms_underflow", [tiny, tiny[::-1]], dict(kind="zero"))
    huge = [(1, 1), (3e38, 0), (2e19, 2e19), (np.inf, 0), (-3e38, 3e38)]
    one("norm_inf", [huge, huge[::-1][:4] + [(1, 2)]], dict(kind="inf"))
    return out


def lanes_and_waves(rng):
    out = []
    # a 64-window batch whose reads are 32 different entries (decoder order), and 64 (an all-EPC table): the second batch of the table
    for name, types, per in (("batch_of_32_entries", alt(192), 32), ("batch_of_64_entries", np.ones(192, dtype=np.int32), 64)):
        frames = rand_frames(rng, per)
        on = np.full(192, -1, dtype=np.int64)
        k = np.flatnonzero(types[64:128] == 1) + 64
        on[k] = rng.permutation(per)
        on[np.flatnonzero(types[:64] == 1)[:5]] = rng.integers(0, per, 5)
        out.append(table(rng, name, "lanes", frames, on, 64, 128, types=types, aim=dict(kind="distinct", per=per, batch=1)))
    # a batch whose reads are all one entry: 32 lanes, and all 64 (lane 63 counts 63 lanes below it)
    for name, types, per in (("batch_of_one_entry_32", alt(192), 32), ("batch_of_one_entry_64", np.ones(192, dtype=np.int32), 64)):
        frames = rand_frames(rng, 3)
        on = np.full(192, -1, dtype=np.int64)
        on[np.flatnonzero(types[64:128] == 1) + 64] = 1
        on[[1, 3, 131, 191]] = [0, 1, 2, 1]
        out.append(table(rng, name, "lanes", frames, on, 64, 128, types=types, aim=dict(kind="same", per=per, batch=1)))
    # one entry's reads in every one of the sixteen waves' ranges, another's in the last only
    nw = 4096
    frames = rand_frames(rng, 4)
    on = np.full(nw, -1, dtype=np.int64)
    on[5] = 2
    on[256 * 7 + 255] = 3
    on[256 * 15 + 2 * rng.choice(128, 40, replace=False) + 1] = 1
    for w in range(16):
        free = np.flatnonzero(on[256 * w: 256 * w + 256] < 0)
        on[256 * w + rng.choice(free[free % 2 == 1], 3 + w % 3, replace=False)] = 0
    out.append(table(rng, "every_wave_and_last_wave", "lanes", frames, on, 8, 16, aim=dict(kind="waves")))
    for nw in NW_LIST:
        d = 6
        n_reads = max(min(nw // 2, d), int(0.4 * nw))
        out.append(table(rng, "nw%d" % nw, "lanes", rand_frames(rng, d), spread(rng, nw, min(d, n_reads), n_reads), 8, 16,
                         aim=dict(kind="nw", nw=nw), emu=nw in NW_EMU))
    return out


def capacity(rng):
    """more EPC reads than the reads capacity given (a launch of its own: the capacity is the launch's)"""
    out = [simple(rng, "cap_a", "capacity", 7, 8, 16, nw=700, n_reads=300, aim=dict(kind="cap")),
           simple(rng, "cap_b", "capacity", 5, 8, 16, nw=600, n_reads=101, aim=dict(kind="cap"))]
    return out


BATCH_MAX_TAGS, BATCH_SLOTS, BATCH_WMAX = 4, 8, 8
BATCH_OVER = {1: [[], [0]], 63: [[62]], 64: [[0]], 65: [[31, 32, 64]], 1024: [[1023], []], 1025: [[1024], [512, 513, 1000]], 2049: [[2048], [5, 700, 2047]]}


def batches(rng):
    """whole launches: n traces of 8 windows, 0..4 distinct frames per trace (EPC windows 1, 3, 5, 7), the traces listed in BATCH_OVER
    all-EPC with more than four (overflow by count)"""
    out = []
    pool = rand_frames(rng, 24)
    for n in BATCH_SIZES:
        for v, over in enumerate(BATCH_OVER[n]):
            res = np.zeros((n, BATCH_WMAX), dtype=capi.RESULT_DTYPE)
            st = np.zeros((n, BATCH_WMAX), dtype=np.int32)
            for s in range(n):
                if s in over:
                    types = np.ones(BATCH_WMAX, dtype=np.int32)
                    on = rng.permutation(24)[:BATCH_WMAX].astype(np.int64)
                    on[rng.integers(0, 8)] = on[0] if rng.random() < 0.5 else -1          # (5 .. 8 distinct frames)
                    on[int(rng.integers(1, 8))] = on[0]
                else:
                    types = alt(BATCH_WMAX)
                    c = int(rng.integers(0, 5))
                    on = np.full(BATCH_WMAX, -1, dtype=np.int64)
                    if c:
                        ids = rng.permutation(24)[:c]
                        reads = np.concatenate([ids, rng.choice(ids, 4 - c)]) if rng.random() < 0.6 else np.concatenate([ids, np.full(4 - c, -1)])
                        on[1::2] = rng.permutation(reads)
                res[s] = records(rng, pool, on, types)
                st[s] = starts(rng, BATCH_WMAX)
            wc = np.full(n, BATCH_WMAX, dtype=np.int32)
            used = np.full(n, BATCH_WMAX, dtype=np.int32)
            short = rng.random(n) < 0.2
            short[list(over)] = False
            used[short] = rng.integers(0, BATCH_WMAX + 3, int(short.sum()))
            out.append(launch(["batch%d_%d" % (n, v)], "batches", res, wc, used, st, BATCH_MAX_TAGS, BATCH_SLOTS,
                              aim=dict(n=n, over=list(over)), emu=(n < 1024 or v == 0)))
    return out


def random_tables(seed=20240916):
    """D up to 40 with skewed read counts, random limits, slots from {the plan's, D rounded up, 1024}"""
    rng = np.random.default_rng(seed)
    out = []
    for n in range(N_RANDOM):
        d = int(rng.integers(0, 41))
        n_reads = d + int(rng.integers(0, 3 * d + 2)) if d else 0
        nw = 2 * n_reads + int(rng.integers(1, 40))
        max_tags = max(1, int(rng.choice([d - 1, d, d, d + 1, d + 7, 64, 65])))
        up = 2
        while up < d:
            up *= 2
        slots = int(rng.choice([default_slots(max_tags), up, 1024]))
        out.append(table(rng, "random%d_d%d_mt%d_s%d" % (n, d, max_tags, slots), "random", rand_frames(rng, max(d, 1))[:d],
                         spread(rng, nw, d, n_reads, skew=float(rng.uniform(0.0, 2.5))), max_tags, slots,
                         used=nw if n % 4 else int(rng.integers(0, nw + 1)), aim=dict(d=d), emu=(n % RANDOM_EMU_EVERY == 0)))
    return out


def crafted(seed=20240917):
    rng = np.random.default_rng(seed)
    out = []
    for fam in (counts, full_tables, one_chain, near_frames, first_reads, strongest, lanes_and_waves, capacity):
        out += fam(rng)
    return out


FAMILIES = ("counts", "full", "chain", "near", "firsts", "strongest", "lanes", "capacity", "batches", "random")


# ---- launches ---------------------------------------------------------------------------------------------------------
def launch(names, family, res, wcount, used, start, max_tags, slots, cap=None, reads_len=None, aim=None, emu=True):
    n, wmax = res.shape
    want = tracks_ref.expected_tables(res, wcount, used, start, max_tags, slots)
    total = int(want["reads_head"][0])
    if cap is None:                     # every window of the launch could be a read
        cap = max(1, n * wmax)
    reads_len = max(cap, total) + 8 if reads_len is None else reads_len
    return Launch(list(names), family, res, np.asarray(wcount, dtype=np.int32), np.asarray(used, dtype=np.int32),
                  np.ascontiguousarray(start, dtype=np.int32), int(max_tags), int(slots), int(cap), int(reads_len), want, aim or {}, emu)


def groups(tables):
    """tables of one family, one (max_tags, slots) and one size class -> one launch: [n][wmax] records, the rows behind their own
    records filled with verified reads of POISON_FRAME (and the windows' starts there with -1)"""
    by = {}
    for t in tables:
        size = 0 if len(t.res) <= 512 else (1 if len(t.res) <= 2100 else 2)
        by.setdefault((t.family, t.max_tags, t.slots, size), []).append(t)
    out = []
    for (family, max_tags, slots, _), ts in by.items():
        wmax = max(1, max(len(t.res) for t in ts))
        res = np.zeros((len(ts), wmax), dtype=capi.RESULT_DTYPE)
        res["type"], res["crc_ok"], res["n_bits"], res["bits"] = 1, 1, 128, POISON_FRAME
        res["h_re"], res["tag_id"] = 1e30, tag_id_of(POISON_FRAME)[0]
        st = np.full((len(ts), wmax), -1, dtype=np.int32)
        for s, t in enumerate(ts):
            res[s, : len(t.res)] = t.res
            st[s, : len(t.res)] = t.start
        g = launch([t.name for t in ts], family, res, [t.wcount for t in ts], [t.used for t in ts], st, max_tags, slots,
                   aim=dict(tables=[t.aim for t in ts]), emu=all(t.emu for t in ts))
        if family == "capacity":        # the capacity ends inside the last trace; the caller's array holds all reads, and a guard
            total, last = int(g.want["reads_head"][0]), int(g.want["base"][-1])
            g = g._replace(cap=last + (total - last) // 2, reads_len=total + 8)
        out.append(g)
    return out


def launches(emu_only=False):
    """every launch of the suite; emu_only: the emulator's share (NW_EMU of the lengths, a fifth of the random tables)"""
    ts = crafted() + random_tables()
    if emu_only:
        ts = [t for t in ts if t.emu]
    rng = np.random.default_rng(20240918)
    return groups(ts) + [g for g in batches(rng) if g.emu or not emu_only]


def emu_waves(g):
    """the workgroup shapes the emulator runs a launch in: both, but a batch of a thousand traces and more in one wave per trace only
    (sixteen are 1 024 fibers per trace there; the offsets scans such a batch is about do not depend on the shape)"""
    return WAVES if len(g.res) < 1024 else WAVES[:1]


# ---- the comparison ----------------------------------------------------------------------------------------------------
def prefilled(dtype, n):
    return np.full(n * np.dtype(dtype).itemsize // 4, PREFILL, dtype=np.int32).view(dtype)


def expected_outputs(g):
    """every output array as a launch must leave it: PREFILL words wherever the kernels have no business writing"""
    n = len(g.res)
    w = g.want
    rows = prefilled(capi.TAG_ENTRY_DTYPE, n * g.max_tags).reshape(n, g.max_tags)
    for s, e in enumerate(w["per"]):
        rows[s, : len(e)] = e
    packed = prefilled(capi.TAG_ENTRY_DTYPE, n * g.max_tags)
    packed[: len(w["packed"])] = w["packed"]
    offsets = prefilled(np.int64, n * g.max_tags + 1)
    offsets[: len(w["offsets"])] = w["offsets"]
    reads = prefilled(capi.TAG_READ_DTYPE, g.reads_len)
    k = min(len(w["reads"]), g.cap)
    reads[:k] = w["reads"][:k]
    return dict(rows=rows, counts=w["counts"], overflow=w["overflow"], head=w["head"], ent_off=w["ent_off"], packed=packed,
                base=w["base"], reads_head=w["reads_head"], offsets=offsets, reads=reads)


OUTPUTS = ("counts", "overflow", "head", "rows", "ent_off", "packed", "base", "reads_head", "offsets", "reads")


def check(run, g, waves):
    """run(results, wcount, n_windows_used, start, waves, max_tags, slots, reads_cap, reads_len, prefill) -> dict of the output arrays.
    Every array starts from PREFILL words; every word of every array must come back as expected_outputs() says."""
    got = run(g.res, g.wcount, g.used, g.start, waves, g.max_tags, g.slots, g.cap, g.reads_len, PREFILL)
    want = expected_outputs(g)
    for name in OUTPUTS:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() == b.tobytes():
            continue
        aw, bw = a.reshape(-1).view(np.int32), b.reshape(-1).view(np.int32)
        per = a.dtype.itemsize // 4
        bad = np.flatnonzero(aw != bw)
        rec = int(bad[0]) // per
        where = ""
        if name == "rows":
            where = " (trace %d = %s, row %d)" % (rec // g.max_tags, g.names[min(rec // g.max_tags, len(g.names) - 1)], rec % g.max_tags)
        elif name in ("counts", "overflow", "ent_off", "base"):
            where = " (trace %s)" % g.names[min(rec, len(g.names) - 1)]
        raise AssertionError("%s %s, %d waves, max_tags %d, slots %d: `%s` differs in %d words, first in record %d%s: got %s, want %s" % (
            g.family, g.names[:3], waves, g.max_tags, g.slots, name, len(bad), rec, where, a.reshape(-1)[rec], b.reshape(-1)[rec]))

"""The bodies that tests/test_arith_emu.py (the kernels on the emulator) and tests/test_gpu_arith.py (on the device) share: the
reference is pinned and the reach of every family of tests/arith_cases.py asserted from tests/arith_ref.py alone (check_reference,
no kernel involved), then one call of rfid_selftest_arith per group of records is compared field by field (check_outputs)."""
from fractions import Fraction

import numpy as np

import arith_cases as ac
import arith_ref as ref

F32 = np.float32

# floors: the two of the near-midpoint family are the issue's (722 pairs and 204 double-rounding cases measured); the others were measured on the
# committed seeds (1 016 scanned records, 425 of them with ties; 835 scanned pairs, 193 with ties in both halves; 988 shared scans; 368 refusals;
# 168 / 34 division records on the fast path / the fallback) and are set a little below
FLOOR_MID_PAIRS = 500
FLOOR_MID_DOUBLE_ROUNDING = 150
FLOOR_SCANNED = 900           # records whose chain_add_scan flag is due
FLOOR_SCANNED_WITH_TIES = 350
FLOOR_PAIR_SCANNED = 700
FLOOR_PAIR_WITH_TIES = 150
FLOOR_SCAN2 = 850
FLOOR_REFUSED = 300           # records where a partial sum leaves, the size limit is hit or the carry is of the wrong kind
FLOOR_FAST_WAVES = 150        # division records whose every lane is admitted / that take the fallback
FLOOR_FALLBACK_WAVES = 30


# ---- the reference, pinned; the reach of the cases --------------------------------------------------------------------------
def facts_of(cases):
    return [ac.sum_facts(r) for r in cases.recs]


def check_additions_pinned(cases):
    """numpy's binary32 addition is the exact sum rounded to nearest-even on the sample, subnormal and overflowing sums included"""
    rng = np.random.default_rng(7)
    recs = cases.recs
    n = ref.pin_additions(recs["carry"], recs["x0"], rng, 1500)
    n += ref.pin_additions(ref.seq_sum(recs["carry"], recs["x0"])[:, 63], recs["x1"], rng, 1000)
    assert n >= 2000
    # and where it matters most: subnormal sums, overflow, ties
    for a, b, want in ((1.0, 2.0 ** -24, 1.0), (1.0 + 2.0 ** -23, 2.0 ** -24, 1.0 + 2.0 ** -22), (ac.FLT_MAX, 2.0 ** 103, np.inf),
                       (ac.FLT_MAX, 2.0 ** 102, ac.FLT_MAX), (ac.SUBNORMAL_MIN, ac.SUBNORMAL_MIN, 2 * ac.SUBNORMAL_MIN), (-0.0, -0.0, -0.0), (-0.0, 0.0, 0.0)):
        got = ref.add_exact(a, b)
        with np.errstate(over="ignore"):
            assert ref.bits(got) == ref.bits(F32(want)) == ref.bits(F32(F32(a) + F32(b))), (a, b)


def check_sum_reach(cases, facts):
    fam, name = cases.family, cases.name

    def rows(family, part=""):
        k = [i for i in range(len(fam)) if fam[i] == family and part in name[i]]
        assert k, (family, part)
        return k

    lanes = lambda m: set(np.flatnonzero(m).tolist())     # noqa: E731
    for i in rows("exponent", "e22"):
        assert not facts[i]["pred"] and not facts[i]["pred_pair"]
    for e in (23, 24, 253, 254):
        assert any(facts[i]["pred"] for i in rows("exponent", f"e{e}")), e
        assert any(facts[i]["pred"] and facts[i]["tie"][:64].any() for i in rows("exponent", f"e{e}")), e
    assert all(np.isinf(ref.from_bits(facts[i]["part"])).any() for i in rows("overflow", "alone"))
    for i in rows("zero_carry") + rows("subnormal_carry"):
        assert not facts[i]["pred"] and not facts[i]["pred2"]
    i = rows("zero_carry", "neg/negzeros")[0]
    assert np.all(facts[i]["part"][:64] == 0x80000000)     # a sum that is -0 on every lane: the one operand on which the chains are not the sequential sum
    seq, chain = ref.bits(ref.seq_sum(cases.recs["carry"], cases.recs["x0"])), ref.bits(ref.chain_sum(cases.recs["carry"], cases.recs["x0"]))
    differ = np.flatnonzero((seq != chain).any(axis=1))
    assert len(differ) >= 1 and all(fam[k] == "zero_carry" and ref.bits(cases.recs["carry"][k]) == 0x80000000 for k in differ)
    i = rows("power_of_two", "p16_up/pos/alone")[0]
    assert facts[i]["pred"] and cases.recs[i]["carry"] == 16.0
    for i in rows("power_of_two", "p16_down") + rows("power_of_two", "p16_stay"):
        assert not facts[i]["pred"]
    for sg in ("pos", "neg"):
        i = rows("edge", f"lower_from_above/{sg}/alone")[0]
        cb = int(ref.bits(cases.recs[i]["carry"]))
        assert int(facts[i]["part"][7]) == (cb & 0xff800000) and not facts[i]["pred"]       # exactly the binade's lower edge
        for nm in ("upper_plain", "upper_tie_from_top/"):
            i = rows("edge", f"{nm}")[0 if sg == "pos" else 2]
            cb = int(ref.bits(cases.recs[i]["carry"]))
            assert int(facts[i]["part"][7]) == (cb & 0xff800000) + 0x00800000 and not facts[i]["pred"], nm      # exactly the next power of two
        i = rows("edge", f"upper_tie_from_top/{sg}/alone")[0]
        assert facts[i]["tie"][7] and (int(ref.bits(cases.recs[i]["carry"])) & 0x7fffff) == 0x7fffff
        assert lanes(facts[rows("edge", f"leave_lane0_only/{sg}/alone")[0]]["out"][:64]) == {0}
        assert lanes(facts[rows("edge", f"leave_lane63_only/{sg}/alone")[0]]["out"][:64]) == {63}
        assert lanes(facts[rows("edge", f"leave_and_return/{sg}/alone")[0]]["out"][:64]) == {20}
        assert lanes(facts[rows("edge", f"leave_and_return_low/{sg}/alone")[0]]["out"][:64]) == {20}
        assert lanes(facts[rows("edge", f"leave_and_return/{sg}/split")[0]]["out"][:64]) == {52}
        i = rows("edge_pair", f"second_leaves_lane0/{sg}")[0]
        assert facts[i]["pred"] and not facts[i]["pred_pair"] and not facts[i]["out"][:64].any() and facts[i]["out"][64]
        i = rows("edge_pair", f"first_leaves_lane63_second_returns/{sg}")[0]
        assert lanes(facts[i]["out"]) == {63} and not facts[i]["pred"] and not facts[i]["pred_pair"]
    for i in rows("limit", "t_2p22/") + rows("limit", "t_2p22_odd/"):
        assert facts[i]["tmax"] == 2.0 ** 22 and not facts[i]["pred_pair"]
    for i in rows("limit", "t_2p22_minus_half"):
        assert facts[i]["tmax"] == 2.0 ** 22 - 0.5 and facts[i]["tie"].any()
    for i in rows("limit", "t_2p22_minus_1"):
        assert facts[i]["tmax"] == 2.0 ** 22 - 1
    assert all(facts[i]["pred"] for i in rows("limit", "minus_half/pos/alone") + rows("limit", "minus_1/pos/alone") + rows("limit", "minus_half/neg/alone"))
    for i in rows("ties", "alone"):
        assert facts[i]["tie"].all() and facts[i]["pred_pair"]
    for i in rows("ties_lane0", "alone"):
        assert lanes(facts[i]["tie"]) == {0} and facts[i]["pred"]
    seen = set()
    for i in rows("ties_boundary"):
        assert facts[i]["pred_pair"] and facts[i]["tie"][:64].any() and facts[i]["tie"][64:].any()
        seen.add((bool(facts[i]["tie"][63]), int(facts[i]["part"][63]) & 1))
    assert seen == {(True, 0), (False, 0), (False, 1)}      # (a tie leaves an even sum)
    seen = set()
    for i in rows("ties_popc"):
        assert facts[i]["pred_pair"] and not facts[i]["tie"][:64].any() and facts[i]["tie"][64:].any()
        r = np.rint(ref.scaled(cases.recs[i]["carry"], cases.recs[i]["x0"])).astype(np.int64)
        seen.add(int(np.sum(r & 1)) & 1)
    assert seen == {0, 1}
    for i in rows("ties_negative") + rows("ties_runs") + rows("ties_zeros"):
        t = ref.scaled(cases.recs[i]["carry"], cases.recs[i]["x0"])
        fr = t - np.rint(t)
        assert (fr == -0.5).any() or (fr == 0.5).any()
    assert any(((lambda fr: (fr == -0.5).any() and (fr == 0.5).any())((lambda t: t - np.rint(t))(ref.scaled(cases.recs[i]["carry"], cases.recs[i]["x0"]))))
               for i in rows("ties_negative"))
    assert all(facts[i]["pred"] for i in rows("ties_runs", "alone") + rows("ties_zeros"))
    bulk = rows("bulk")
    assert len(bulk) == 400 and sum(facts[i]["pred"] for i in bulk) > 200 and sum(facts[i]["pred_pair"] for i in bulk) > 200
    assert sum(facts[i]["pred2"] for i in bulk) > 200
    # the two-carry sum
    for i in rows("two_carry"):
        rec = cases.recs[i]
        dm = (int(ref.bits(rec["carry_b"])) & 0x7fffffff) - (int(ref.bits(rec["carry"])) & 0x7fffffff)
        assert f"dm{dm}/" in name[i] and facts[i]["pred2"], name[i]
    assert sum(1 for i in rows("two_carry", "/ties/") if "dm1/" in name[i] or "dm-1/" in name[i] or "dm3/" in name[i]) == 6       # odd dm with ties: the dual scan
    for i in rows("two_carry_edge"):
        rec = cases.recs[i]
        pa, pb = facts[i]["pred"], ref.scan_predicate(rec["carry_b"], rec["x0"])
        if "dm8/" in name[i] or "dm-8/" in name[i]:
            assert pa and pb and facts[i]["pred2"], name[i]
        elif name[i].startswith("b_leaves"):
            assert pa and not pb and not facts[i]["pred2"], name[i]
        else:
            assert not pa and pb and not facts[i]["pred2"], name[i]
    for i in rows("two_carry_refused"):
        assert facts[i]["pred"] and not facts[i]["pred2"], name[i]
    # the condition as chain_add_scan2's comment writes it (m + dm in [1, 2^23 - 1]) is the same wherever both take the same integers
    n = 0
    for i in range(len(fam)):
        rec = cases.recs[i]
        dm = (int(ref.bits(rec["carry_b"])) & 0x7fffffff) - (int(ref.bits(rec["carry"])) & 0x7fffffff)
        if (dm & 1) == 0 or not facts[i]["tie"][:64].any():
            assert ref.scan2_shared_form(rec["carry"], rec["carry_b"], rec["x0"]) == facts[i]["pred2"], name[i]
            n += 1
    assert n >= 800
    # floors over everything
    count = lambda f: sum(1 for x in facts if f(x))     # noqa: E731
    assert count(lambda x: x["pred"]) >= FLOOR_SCANNED
    assert count(lambda x: x["pred"] and x["tie"][:64].any()) >= FLOOR_SCANNED_WITH_TIES
    assert count(lambda x: x["pred_pair"]) >= FLOOR_PAIR_SCANNED
    assert count(lambda x: x["pred_pair"] and x["tie"][:64].any() and x["tie"][64:].any()) >= FLOOR_PAIR_WITH_TIES
    assert count(lambda x: x["pred2"]) >= FLOOR_SCAN2
    assert count(lambda x: not x["pred"]) >= FLOOR_REFUSED


def check_division_reach(cases):
    """numpy's binary32 division is the exact quotient rounded once on every operand of the division families (the result grid
    includes subnormals); what the families reach"""
    fam, name, recs = cases.family, cases.name, cases.recs
    div = [i for i in range(len(fam)) if fam[i].startswith("div_")]
    for i in div:
        x0, x1 = recs[i]["x0"], recs[i]["x1"]
        for d, got in ((F32(100.0), ref.quotient_np(x0, F32(100.0))), (F32(48.0), ref.quotient_np(x0, F32(48.0)))):
            want = np.array([ref.quotient_exact(v, d) for v in x0], dtype=F32)
            assert ref.same(want, got).all(), name[i]
        want = np.array([ref.quotient_exact(a, b) for a, b in zip(x0, x1)], dtype=F32)
        assert ref.same(want, ref.quotient_np(x0, x1)).all(), name[i]
    adm = ref.div_admitted(recs["x0"])
    not_admitted = {"below_2m100", "neg_below_2m100", "p2m120", "subnormal_max", "subnormal_min", "nzero", "pinf", "ninf", "nan"}
    for i in div:
        if fam[i] == "div_one_lane":
            special, lane = name[i].rsplit("_lane", 1)
            assert adm[i].sum() == (63 if special in not_admitted else 64) and adm[i, int(lane)] == (special not in not_admitted), name[i]
        if fam[i] == "div_all_lanes":
            assert adm[i].all() == (name[i][:-4] not in not_admitted) and adm[i].any() == adm[i].all(), name[i]
    assert sum(1 for i in div if adm[i].all()) >= FLOOR_FAST_WAVES and sum(1 for i in div if not adm[i].all()) >= FLOOR_FALLBACK_WAVES
    sw = recs["x0"][[i for i in div if fam[i] == "div_sweep"]]
    assert sw.size == 8192 and len(set(((ref.bits(sw) >> 23) & 0xff).ravel().tolist())) == 255      # every binade, the subnormals' included
    # subnormal quotients and subnormal results of fdiv occur
    q = ref.quotient_np(recs["x0"][div], recs["x1"][div])
    assert np.sum((q != 0) & (np.abs(q) < F32(2.0 ** -126))) >= 200
    q = ref.quotient_np(recs["x0"][div], F32(100.0))
    assert np.sum((q != 0) & (np.abs(q) < F32(2.0 ** -126))) >= 200
    for i in div:
        if fam[i] == "div_exact" and not name[i].endswith(("_up", "_down")):
            d = int(name[i][5:].split("_")[0])
            assert all((ref.frac(v) / d) == ref.frac(qq) for v, qq in zip(recs[i]["x0"], ref.quotient_np(recs[i]["x0"], F32(d)))), name[i]
        if fam[i] == "div_halfway":
            d = int(name[i][7:])
            half = sum(1 for v in recs[i]["x0"] if (ref.frac(v) / d * 2 ** 149) % 1 == Fraction(1, 2))
            assert half >= 40, (name[i], half)


def check_hypot_reach(pairs):
    """the exact-integer formula and numpy's double formula agree on every pair of the hypot families; what the families reach"""
    x, y, fam = pairs
    want = np.array([ref.hypot_exact(a, b) for a, b in zip(x, y)], dtype=F32)
    assert np.array_equal(ref.bits(want), ref.bits(ref.hypot_np(x, y)))
    mid = np.flatnonzero(fam == "mid")
    assert len(mid) >= FLOOR_MID_PAIRS
    X = x[mid].astype(np.int64)
    got = want[mid].astype(np.int64)
    assert set((got - X).tolist()) == {0, 1}                         # either neighbour of the midpoint X + 1/2
    single = np.array([ref.hypot_single_rounding(a, b) for a, b in zip(x[mid], y[mid])], dtype=F32)
    n_double = int(np.sum(single != want[mid]))
    assert n_double >= FLOOR_MID_DOUBLE_ROUNDING
    for f, scale in (("mid_2m60", -60), ("mid_2m100", -100), ("mid_2p60", 60)):
        k = np.flatnonzero(fam == f)
        assert len(k) == len(mid) and np.array_equal(want[k].astype(np.float64), np.ldexp(want[mid].astype(np.float64), scale))
    k = np.flatnonzero(fam == "pythagorean")
    assert np.array_equal(want[k].astype(np.float64) ** 2, x[k].astype(np.float64) ** 2 + y[k].astype(np.float64) ** 2)
    k = np.flatnonzero(fam == "pythagorean_tie")[::2]
    h = np.array([int(a) ** 2 + int(b) ** 2 for a, b in zip(x[k], y[k])])
    r = np.array([int(np.sqrt(float(v))) for v in h])
    assert np.array_equal(r * r, h) and np.all(r & 1) and np.all(r > 1 << 24) and np.all(want[k].astype(np.int64) % 4 == 0) and np.all(np.abs(want[k].astype(np.int64) - r) == 1)
    assert np.isinf(want[fam == "range"]).sum() >= 2 and np.sum((want != 0) & (want < F32(2.0 ** -126))) >= 10
    k = np.flatnonzero(fam == "range_apart")
    big = np.maximum(np.abs(x[k]), np.abs(y[k])).astype(np.float64)
    ssum = x[k].astype(np.float64) ** 2 + y[k].astype(np.float64) ** 2
    assert np.sum(ssum == big * big) >= 8 and np.sum(ssum != big * big) >= 8      # the small operand vanishes in the double sum / does not
    assert np.sum(fam == "bulk") == 4096
    return dict(mid_pairs=len(mid), mid_double_rounding=n_double)


def check_tile_reach(cases):
    fam, name, recs = cases.family, cases.name, cases.recs
    want = ref.sum25(recs["tile"])
    t = recs["tile"].reshape(len(recs), 340, 2)
    lanes = 5 * np.arange(64)
    rev = np.zeros((len(recs), 64, 2), dtype=F32)
    pairwise = np.zeros((len(recs), 64, 2), dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(24, -1, -1):
            rev = (rev + t[:, lanes + k, :]).astype(F32)
        for k in range(0, 24, 2):       # two partial sums, as a packed or split accumulation would form them
            pairwise = (pairwise + (t[:, lanes + k, :] + t[:, lanes + k + 1, :]).astype(F32)).astype(F32)
        pairwise = (pairwise + t[:, lanes + 24, :]).astype(F32)
    rev, pairwise = rev.reshape(len(recs), 128), pairwise.reshape(len(recs), 128)
    differs = lambda a, i: int(np.sum(ref.bits(a[i]) != ref.bits(want[i])))     # noqa: E731
    for i in range(len(fam)):
        if fam[i] in ("tile_cancel", "tile_binades"):
            assert differs(rev, i) >= 16 and differs(pairwise, i) >= 8, (name[i], differs(rev, i), differs(pairwise, i))
        if fam[i] == "tile_subnormal":
            assert np.sum((want[i] != 0) & (np.abs(want[i]) < F32(2.0 ** -126))) >= (8 if "to_normal" in name[i] else 100), name[i]
        if name[i] == "index":
            assert np.array_equal(want[i][0::2], 125.0 * np.arange(64) + 300.0) and np.array_equal(want[i][1::2], -(250.0 * np.arange(64) + 600.0))
        if name[i] == "all_negzero":
            assert np.all(ref.bits(want[i]) == 0)        # (0 + -0 = +0: the sum starts from +0)
    seeded = [i for i in range(len(fam)) if not fam[i].startswith("tile_")]
    assert len(seeded) >= 200 and np.mean([differs(rev, i) for i in seeded[:200]]) >= 32


def check_scan_reach(cases):
    fam, recs = cases.family, cases.recs
    wraps = np.abs(np.cumsum(recs["iv"].astype(np.int64), axis=1)).max(axis=1) >= 2 ** 31
    assert wraps[fam == "scan_wrap"].all() and np.sum(fam == "scan_single") == 64
    assert set(recs["fill"][fam == "scan_ones"].tolist()) == set(ac.FILLS)


# ---- the expected outputs -----------------------------------------------------------------------------------------------------
def expected(recs, facts):
    c, cb, x0, x1 = recs["carry"], recs["carry_b"], recs["x0"], recs["x1"]
    # the DPP chains: the sequential sum, but for the -0 partial sums of a -0 carry (ref.chain_sum); the end sums keep those
    s0 = ref.chain_sum(c, x0)
    w = dict(chain=s0, autosum=s0, pair_fb0=s0, pair_fb1=ref.chain_sum(s0[:, 63], x1), auto2_a=s0, auto2_b=ref.chain_sum(cb, x0),
             chain2_a=s0, chain2_b=ref.chain_sum(cb, x1),
             ends_a=ref.seq_sum(c, x0)[:, 63], ends_b=ref.seq_sum(cb, x1)[:, 63], div100=ref.quotient_np(x0, F32(100.0)), div48=ref.quotient_np(x0, F32(48.0)),
             fdiv=ref.quotient_np(x0, x1), hypot=ref.hypot_np(x0, x1), shr1=ref.shr1(x0), rint=ref.rint(x0), sum25=ref.sum25(recs["tile"]),
             scan_add=ref.scan_add(recs["iv"]), row_shr1=ref.row_shr(recs["iv"], recs["fill"], 1), row_shr2=ref.row_shr(recs["iv"], recs["fill"], 2),
             row_shr4=ref.row_shr(recs["iv"], recs["fill"], 4), row_shr8=ref.row_shr(recs["iv"], recs["fill"], 8),
             row_bcast15=ref.row_bcast15(recs["iv"], recs["fill"]), row_bcast31=ref.row_bcast31(recs["iv"], recs["fill"]),
             wave_shr1=ref.wave_shr1(recs["iv"], recs["fill"]))
    w["mf"] = w["sum25"]
    w["admitted"] = ref.div_admitted(x0)
    w["scan_flag"] = np.array([f["pred"] for f in facts], dtype=np.int32)
    w["pair_flag"] = np.array([f["pred_pair"] for f in facts], dtype=np.int32)
    w["auto2_flag"] = np.array([f["pred2"] for f in facts], dtype=np.int32)
    return w


def _report(cases, field, bad, got, want):
    k, lane = np.argwhere(bad)[0] if bad.ndim == 2 else (np.flatnonzero(bad)[0], -1)
    r = cases.recs[k]
    g, w = (got[k, lane], want[k, lane]) if lane >= 0 else (got[k], want[k])
    hexof = lambda v: hex(int(np.asarray(v).view(np.uint32 if np.asarray(v).itemsize == 4 else np.uint64)))     # noqa: E731
    return (f"{field}: {int(bad.sum())} mismatches in {len(set(np.argwhere(bad)[:, 0].tolist()))} records; first: record {k} "
            f"({cases.family[k]}: {cases.name[k]}) lane {lane}: got {g!r} ({hexof(g)}), want {w!r} ({hexof(w)}); carry {r['carry']!r} "
            f"({hexof(r['carry'])}), carry_b {r['carry_b']!r}, x0 {r['x0'][max(lane, 0)]!r} ({hexof(r['x0'][max(lane, 0)])}), x1 {r['x1'][max(lane, 0)]!r} "
            f"({hexof(r['x1'][max(lane, 0)])}), fill {r['fill']}")


def check_outputs(cases, facts, out):
    """out: what Context.selftest_arith(cases.recs, prefill=ac.PREFILL) returned.  Every mismatching field is reported, with the
    operands and the bits of the first mismatch of each."""
    recs = cases.recs
    n = len(recs)
    assert len(out) == n + 1
    guard = out[n:].view(np.uint8)
    assert np.all(guard == ac.PREFILL), "the guard record behind the last one was written"
    o = out[:n]
    w = expected(recs, facts)
    errors = []

    def floats(field, want, where=None):
        bad = ~ref.same(o[field], want)
        if where is not None:
            bad &= where
        if bad.any():
            errors.append(_report(cases, field, bad, o[field], want))

    def ints(field, want):
        bad = o[field] != want
        if bad.any():
            errors.append(_report(cases, field, bad, o[field], want))

    for f in ("chain", "autosum", "pair_fb0", "pair_fb1", "auto2_a", "auto2_b", "chain2_a", "chain2_b", "div100", "div48", "fdiv", "shr1", "rint", "sum25", "mf"):
        floats(f, w[f])
    if not np.array_equal(ref.bits(o["sum25"]), ref.bits(o["mf"])):
        errors.append("sum25 and mf differ from each other")
    finite = np.isfinite(recs["x0"]) & np.isfinite(recs["x1"])
    floats("hypot", w["hypot"], finite)
    floats("ends_a", w["ends_a"])
    floats("ends_b", w["ends_b"])
    # the flags are the predicates of the comments; a flag that is set vouches for the bits, whatever the predicate says
    for f in ("scan_flag", "pair_flag", "auto2_flag"):
        if not np.all((o[f] == 0) | (o[f] == 1)):
            errors.append(f"{f} is neither 0 nor 1 somewhere")
        ints(f, w[f])
    floats("scan", w["chain"], (o["scan_flag"] != 0)[:, None])
    floats("pair0", w["pair_fb0"], (o["pair_flag"] != 0)[:, None])
    floats("pair1", w["pair_fb1"], (o["pair_flag"] != 0)[:, None])
    # divisions: the votes are complementary and what the comment admits; the fast form is the quotient wherever it is admitted
    ints("div_ok", ref.mask_of(w["admitted"]))
    ints("div_bad", ~ref.mask_of(w["admitted"]))
    if not np.all((o["div_ok"] ^ o["div_bad"]) == np.uint64(0xffffffffffffffff)):
        errors.append("div_const_bad and div_const_ok are not complementary somewhere")
    floats("fast100", w["div100"], w["admitted"])
    floats("fast48", w["div48"], w["admitted"])
    # f2i: stored where |x0| < 2^31, the prefill kept elsewhere
    with np.errstate(all="ignore"):
        small = np.abs(recs["x0"]) < F32(2.0 ** 31)
        want_i = np.where(small, np.where(small, w["rint"], 0).astype(np.int64), np.int64(ac.PREFILL_WORD)).astype(np.int32)
    ints("f2i", want_i)
    for f in ("scan_add", "row_shr1", "row_shr2", "row_shr4", "row_shr8", "row_bcast15", "row_bcast31", "wave_shr1"):
        ints(f, w[f])
    if not np.all(o["reserved_"] == ac.PREFILL_WORD):
        errors.append("reserved_ was written")
    assert not errors, "\n".join(errors)


def check_rint_pinned(cases):
    """numpy's rint on binary32 is the exact value rounded to the nearest integer, ties to even (a sample, the ties included)"""
    x = cases.recs["x0"].ravel()
    x = x[np.isfinite(x) & (np.abs(x) < 2.0 ** 40)]
    pick = np.concatenate([x[:: max(1, len(x) // 1500)], np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 8388607.5, -8388606.5, 4194303.5], dtype=F32)])
    got = ref.rint(pick)
    assert all(ref.rint_exact(v) == int(g) for v, g in zip(pick, got))
    assert ref.bits(ref.rint(F32(-0.25))) == 0x80000000


def run(ctx, cases, facts, group):
    """one launch: the records of `group` (arith_cases.GROUPS) with a guard record behind them"""
    k = np.array([i for i in range(len(cases.recs)) if ac.group_of(cases.family[i]) == group])
    assert len(k)
    part = ac.Set(cases.recs[k], cases.family[k], cases.name[k])
    check_outputs(part, [facts[i] for i in k], ctx.selftest_arith(part.recs, prefill=ac.PREFILL))

"""Crafted operands for the arithmetic primitives (TEST INFRASTRUCTURE; tests/arith_suite.py runs them through
rfid_selftest_arith on the emulator and on the device).  A record is one wave's operands (capi.ARITH_IN_DTYPE); every routine
runs on every record, so a record made for one family is a bystander case for all the others, and every record carries a
seeded filter tile and seeded scan words unless its family is about those.  The expected values are tests/arith_ref.py's,
nothing else; what a family is meant to reach is asserted from that reference alone (tests/arith_suite.py), before any kernel runs.

The in-order sums are written in the units of the carry's binade: an addend of t ulps is t * 2^(e - 23), negated under a
negative carry (the kernels fold the sign the same way), so that `S` -- the carry's 24-bit integer image 2^23 + mantissa --
moves by RNE(t) wherever the integer scan is the same arithmetic."""
import math
from collections import namedtuple

import numpy as np

import arith_ref as ref
from rfid import _capi as capi

F32 = np.float32
PREFILL = 0xA5                     # every byte of the output records in front of a launch
PREFILL_WORD = int(np.array([PREFILL * 0x01010101], dtype=np.uint32).view(np.int32)[0])
FILLS = (0, -1, 0x5A5A1234)
E_ORD = 120                        # the biased exponent of an ordinary carry: 2^-7, where avg_ampl and dc_est live
FLT_MAX = float(np.finfo(F32).max)
SUBNORMAL_MAX = float(ref.from_bits(0x007fffff))
SUBNORMAL_MIN = float(ref.from_bits(1))
TIE_I = tuple(range(-8, 9))

Set = namedtuple("Set", "recs family name")


def carry_of(e_b, mant, negative=False):
    return ref.from_bits(np.uint32((0x80000000 if negative else 0) | (e_b << 23) | (mant & 0x7fffff)))[()]


def ulps(carry, t):
    """addends of t units of the carry's binade, in the direction of its sign; exact or an assertion fails"""
    cb = int(ref.bits(F32(carry)))
    e_b = max((cb >> 23) & 0xff, 1)
    t = np.asarray(t, dtype=np.float64)
    v = t * math.ldexp(1.0, e_b - 150) * (-1.0 if cb >> 31 else 1.0)
    x = v.astype(F32)
    assert np.array_equal(x.astype(np.float64), v), "addend not representable"
    return x


class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rows, self.family, self.name = [], [], []

    def ordinary(self, n):
        """increments of the receive path's size: differences of amplitudes ~1e-2 over 100"""
        return (self.rng.normal(0.0, 1e-4, n)).astype(F32)

    def add(self, family, name, carry=None, carry_b=None, x0=None, x1=None, tile=None, iv=None, fill=None):
        r = np.zeros((), dtype=capi.ARITH_IN_DTYPE)
        k = len(self.rows)
        r["carry"] = F32(0.0123) if carry is None else carry
        r["carry_b"] = ref.from_bits(ref.bits(r["carry"]) + np.uint32(2))[()] if carry_b is None else carry_b
        r["fill"] = FILLS[k % 3] if fill is None else fill
        r["x0"] = self.ordinary(64) if x0 is None else x0
        r["x1"] = self.ordinary(64) if x1 is None else x1
        r["tile"] = self.rng.normal(0.0, 0.02, 680).astype(F32) if tile is None else tile
        r["iv"] = self.rng.integers(-2 ** 31, 2 ** 31, 64).astype(np.int32) if iv is None else iv
        self.rows.append(r)
        self.family.append(family)
        self.name.append(name)

    def done(self):
        return Set(np.array(self.rows, dtype=capi.ARITH_IN_DTYPE), np.array(self.family), np.array(self.name))


# =========================================================================================================================
# in-order sums
# =========================================================================================================================
DM = (2, 0, 1, -1, -2, 3, 4)      # carry_b - carry of the sum families' records, in turn: the two-carry sum rides along


def emit_sum(b, family, name, e_b, mant, t, t1=None):
    """the four forms of one family member.  t: 64 addends in ulps (t1: 64 more, default t reversed).  `alone`: x0 = t, x1 = t1;
    `split`: the same 64 addends shifted by 32 lanes, so that they straddle the boundary of the pair, zeros around them."""
    t = np.asarray(t, dtype=np.float64)
    assert t.shape == (64,)
    t1 = t[::-1].copy() if t1 is None else np.asarray(t1, dtype=np.float64)
    z = np.zeros(32)
    for neg in (False, True):
        c = carry_of(e_b, mant, neg)
        k = len(b.rows)
        dm = DM[k % len(DM)]
        cb_bits = int(ref.bits(c)) + dm
        cb2 = ref.from_bits(np.uint32(cb_bits))[()] if ((cb_bits ^ int(ref.bits(c))) & 0xff800000) == 0 else c
        sgn = "neg" if neg else "pos"
        b.add(family, f"{name}/{sgn}/alone", carry=c, carry_b=cb2, x0=ulps(c, t), x1=ulps(c, t1))
        b.add(family, f"{name}/{sgn}/split", carry=c, carry_b=cb2, x0=ulps(c, np.concatenate([z, t[:32]])),
              x1=ulps(c, np.concatenate([t[32:], z])))


def lane_only(lanes_values, base=0.0):
    t = np.full(64, base)
    for lane, v in lanes_values.items():
        t[lane] = v
    return t


def sums(seed=20250101):
    b = Builder(seed)
    rng = b.rng
    halves = lambda n: rng.integers(-16, 17, n) / 2.0     # noqa: E731  (multiples of half an ulp, ties among them)

    # ---- carries by exponent -------------------------------------------------------------------------------------------
    for e_b in (22, 23, 24, 253, 254):
        emit_sum(b, "exponent", f"e{e_b}", e_b, 0x2aaaab, halves(64))
        emit_sum(b, "exponent", f"e{e_b}_int", e_b, 0x400001, rng.integers(-9, 10, 64).astype(np.float64))
    emit_sum(b, "overflow", "flt_max", 254, 0x7fffff, lane_only({3: 1.0, 4: 1.0, 9: -1.0}, 0.0))
    emit_sum(b, "overflow", "flt_max_tie", 254, 0x7fffff, lane_only({0: 0.5, 1: -0.5}, 0.0))
    for neg in (False, True):
        zero = F32(-0.0) if neg else F32(0.0)
        sg = "neg" if neg else "pos"
        b.add("zero_carry", f"zero/{sg}/zeros", carry=zero, carry_b=zero, x0=np.where(np.arange(64) % 3 == 0, F32(0.0), F32(-0.0)).astype(F32),
              x1=np.full(64, -0.0, dtype=F32))
        b.add("zero_carry", f"zero/{sg}/negzeros", carry=zero, carry_b=F32(-0.0), x0=np.full(64, -0.0, dtype=F32), x1=np.full(64, -0.0, dtype=F32))
        b.add("zero_carry", f"zero/{sg}/ordinary", carry=zero, carry_b=zero)
        sub = ref.from_bits(np.uint32((0x80000000 if neg else 0) | 0x00012345))[()]
        b.add("subnormal_carry", f"subnormal/{sg}", carry=sub, carry_b=sub,
              x0=ref.from_bits(rng.integers(0, 0x200, 64).astype(np.uint32) | (rng.integers(0, 2, 64).astype(np.uint32) << 31)),
              x1=ref.from_bits(rng.integers(0, 0x00400000, 64).astype(np.uint32)))
    # exact powers of two: 16.0 and -16.0 (biased exponent 131, mantissa 0) -- upwards the sums enter the binade, downwards they leave it
    emit_sum(b, "power_of_two", "p16_up", 131, 0, np.abs(halves(64)) + 1.0)
    emit_sum(b, "power_of_two", "p16_down", 131, 0, lane_only({0: -0.25, 1: 3.0}))
    emit_sum(b, "power_of_two", "p16_stay", 131, 0, np.zeros(64))

    # ---- binade edges --------------------------------------------------------------------------------------------------
    emit_sum(b, "edge", "lower_from_above", E_ORD, 5, lane_only({7: -5.0, 8: 3.0}))
    emit_sum(b, "edge", "upper_plain", E_ORD, 0x7ffffd, lane_only({7: 3.0}))
    emit_sum(b, "edge", "upper_tie_from_top", E_ORD, 0x7fffff, lane_only({7: 0.5}))
    emit_sum(b, "edge", "upper_tie_from_top_lane0", E_ORD, 0x7fffff, lane_only({0: 0.5, 1: -1.0}))
    emit_sum(b, "edge", "leave_lane0_only", E_ORD, 0x7ffffe, lane_only({0: 4.0, 1: -6.0}))
    emit_sum(b, "edge", "leave_lane63_only", E_ORD, 0x7ffff0, lane_only({63: 32.0}), t1=np.zeros(64))
    emit_sum(b, "edge", "leave_and_return", E_ORD, 0x7ffffe, lane_only({20: 4.0, 21: -6.0}))
    emit_sum(b, "edge", "leave_and_return_low", E_ORD, 2, lane_only({20: -3.0, 21: 4.0}))
    # the pair's own: inside through the first step, out on the second's lane 0; out on lane 63 of the first, back on the second's lane 0
    for neg in (False, True):
        c = carry_of(E_ORD, 0x7ffff0, neg)
        sg = "neg" if neg else "pos"
        b.add("edge_pair", f"second_leaves_lane0/{sg}", carry=c, x0=ulps(c, lane_only({5: 3.0})), x1=ulps(c, lane_only({0: 32.0})))
        b.add("edge_pair", f"first_leaves_lane63_second_returns/{sg}", carry=c, x0=ulps(c, lane_only({63: 16.0})),
              x1=ulps(c, lane_only({0: -18.0, 9: 1.0})))

    # ---- size limits ---------------------------------------------------------------------------------------------------
    for name, big in (("t_2p22", 4194304.0), ("t_2p22_minus_half", 4194303.5), ("t_2p22_minus_1", 4194303.0)):
        emit_sum(b, "limit", name, E_ORD, 100, lane_only({4: big, 5: -big, 30: big}))
        emit_sum(b, "limit", name + "_odd", E_ORD, 101, lane_only({0: big, 63: -big}))

    # ---- ties ----------------------------------------------------------------------------------------------------------
    all_ties = np.array([TIE_I[k % 17] + 0.5 for k in range(64)])
    emit_sum(b, "ties", "all_lanes", E_ORD, 0x2aaaaa, all_ties)
    emit_sum(b, "ties", "all_lanes_odd", E_ORD, 0x2aaaab, all_ties[::-1])
    emit_sum(b, "ties", "all_lanes_shuffled", E_ORD, 0x155555, rng.permutation(all_ties))
    for i in TIE_I:
        emit_sum(b, "ties_lane0", f"lane0_I{i}_even", E_ORD, 0x300000, lane_only({0: i + 0.5}), t1=np.zeros(64))
        emit_sum(b, "ties_lane0", f"lane0_I{i}_odd", E_ORD, 0x300001, lane_only({0: i + 0.5}), t1=np.zeros(64))
    # parity handed across the boundary of the pair (these are built for the pair: x0's last lanes, x1's first)
    for neg in (False, True):
        sg = "neg" if neg else "pos"
        for mant in (0x300000, 0x300001):
            c = carry_of(E_ORD, mant, neg)
            for i in (-3, -2, 0, 1, 4):
                for pattern, l0, l1 in (("tie63", {63: i + 0.5}, {0: 1.5, 1: -0.5}),
                                        ("tie62_63", {62: i + 0.5, 63: 2.5}, {0: -1.5, 1: 0.5}),
                                        ("tie62_odd63", {62: i + 0.5, 63: 3.0}, {0: 0.5, 1: 2.5}),
                                        ("tie62_even63", {62: i + 0.5, 63: 2.0}, {0: 0.5, 1: 2.5})):
                    b.add("ties_boundary", f"{pattern}_I{i}_m{mant & 1}/{sg}", carry=c, x0=ulps(c, lane_only(l0)), x1=ulps(c, lane_only(l1)))
            # no tie in x0; an odd and an even number of odd R there; ties in x1 (the popc branch)
            for n_odd in (0, 1, 2, 7, 63, 64):
                t0 = np.zeros(64)
                t0[rng.permutation(64)[:n_odd]] = rng.choice([-3.0, -1.0, 1.0, 5.0, 0.75, 1.25], n_odd)
                t0[t0 == 0.0] = rng.choice([0.0, 2.0, -4.0, 0.25], int(np.sum(t0 == 0.0)))
                b.add("ties_popc", f"odd{n_odd}_m{mant & 1}/{sg}", carry=c, x0=ulps(c, t0),
                      x1=ulps(c, lane_only({0: 0.5, 5: -2.5, 6: 1.0, 7: 3.5, 63: 0.5})))
    # ties separated by odd and by even runs of odd non-tie addends; negative fractions; signed zeros between ties
    for run in (0, 1, 2, 3, 4, 5, 8, 15):
        t = np.zeros(64)
        pos = 1
        while pos + run + 1 < 64:
            t[pos] = rng.choice([-3.5, -0.5, 0.5, 2.5, 5.5])
            t[pos + 1: pos + 1 + run] = rng.choice([-3.0, -1.0, 1.0, 7.0], run)
            pos += run + 1
        emit_sum(b, "ties_runs", f"run{run}", E_ORD, 0x2aaaaa + run, t)
    emit_sum(b, "ties_negative", "minus_half", E_ORD, 0x400000, np.where(np.arange(64) % 2 == 0, -0.5, 0.0))
    emit_sum(b, "ties_negative", "minus_half_odd", E_ORD, 0x400001, np.where(np.arange(64) % 3 == 0, -0.5, 1.0))
    emit_sum(b, "ties_negative", "mixed", E_ORD, 0x400001, np.array([(-1) ** k * (k % 5 + 0.5) for k in range(64)]))
    for neg in (False, True):
        c = carry_of(E_ORD, 0x2aaaab, neg)
        x = ulps(c, np.where(np.arange(64) % 4 == 0, 1.5, 0.0))
        x[1::4] = -0.0
        x[2::4] = 0.0
        x[3::4] = -0.0
        b.add("ties_zeros", f"signed_zeros/{'neg' if neg else 'pos'}", carry=c, x0=x, x1=x[::-1].copy())

    # ---- random bulk: the receive path's magnitudes --------------------------------------------------------------------
    for k in range(400):
        c = F32(abs(rng.normal(0.02, 0.01)) + 1e-3) if k % 4 else F32(rng.normal(0.0, 0.01))
        b.add("bulk", f"bulk{k}", carry=c, carry_b=ref.from_bits(ref.bits(c) + np.uint32(k % 3))[()],
              x0=(rng.integers(-2000, 2000, 64) * 2.0 ** -17 / 100.0).astype(F32), x1=(rng.integers(-2000, 2000, 64) * 2.0 ** -17 / 48.0).astype(F32))
    return b.done()


def two_carry(seed=20250102):
    """chain_add_auto2: dm = carry_b - carry in the integer image, crossed with steps without and with ties, with one variant
    leaving the binade while the other stays, and with carries the shared scan must refuse outright"""
    b = Builder(seed)
    rng = b.rng
    no_tie = rng.integers(-6, 7, 64).astype(np.float64) + rng.choice([0.0, 0.25, -0.25], 64)
    ties = np.where(rng.integers(0, 3, 64) == 0, rng.integers(-4, 5, 64) + 0.5, rng.integers(-5, 6, 64).astype(np.float64))
    one_tie = lane_only({17: 2.5}, 1.0)
    mant = 0x200010
    for neg in (False, True):
        sg = "neg" if neg else "pos"
        for dm in (0, 1, -1, 2, -2, 3, 0x3fffff, 0x3ffffe, -0x1fffff, -0x1ffffe, -7, -8):
            for tname, t in (("no_tie", no_tie), ("ties", ties), ("one_tie", one_tie)):
                ca = carry_of(E_ORD, mant + (1 if tname == "ties" else 0), neg)
                cb = ref.from_bits(ref.bits(ca) + np.uint32(dm & 0xffffffff))[()]
                b.add("two_carry", f"dm{dm}/{tname}/{sg}", carry=ca, carry_b=cb, x0=ulps(ca, t))
        # A inside while B's partial sums leave, and the other way round (B above: top edge; B below: bottom edge)
        for tname, t in (("no_tie", lane_only({9: 6.0, 10: -6.0})), ("ties", lane_only({3: 0.5, 9: 6.0, 10: -6.0}))):
            ca = carry_of(E_ORD, 0x7ffff0, neg)
            for dm in (10, 11, 8):        # B reaches 2^24 exactly, crosses it, stops short
                b.add("two_carry_edge", f"b_leaves_top_dm{dm}/{tname}/{sg}", carry=ca, carry_b=ref.from_bits(ref.bits(ca) + np.uint32(dm))[()], x0=ulps(ca, t))
                b.add("two_carry_edge", f"a_leaves_top_dm{dm}/{tname}/{sg}", carry=ref.from_bits(ref.bits(ca) + np.uint32(dm))[()], carry_b=ca, x0=ulps(ca, t))
            ca = carry_of(E_ORD, 0x10, neg)
            tl = -t
            for dm in (-10, -11, -8):     # B's mantissa reaches 0, crosses below, stops short
                b.add("two_carry_edge", f"b_leaves_bottom_dm{dm}/{tname}/{sg}", carry=ca, carry_b=ref.from_bits(ref.bits(ca) + np.uint32(dm & 0xffffffff))[()], x0=ulps(ca, tl))
                b.add("two_carry_edge", f"a_leaves_bottom_dm{dm}/{tname}/{sg}", carry=ref.from_bits(ref.bits(ca) + np.uint32(dm & 0xffffffff))[()], carry_b=ca, x0=ulps(ca, tl))
        ca = carry_of(E_ORD, mant, neg)
        for tname, t in (("no_tie", no_tie), ("ties", ties)):
            b.add("two_carry_refused", f"opposite_sign/{tname}/{sg}", carry=ca, carry_b=F32(-ca), x0=ulps(ca, t))
            b.add("two_carry_refused", f"binade_above/{tname}/{sg}", carry=ca, carry_b=carry_of(E_ORD + 1, mant, neg), x0=ulps(ca, t))
            b.add("two_carry_refused", f"binade_below/{tname}/{sg}", carry=ca, carry_b=carry_of(E_ORD - 1, mant + 5, neg), x0=ulps(ca, t))
    return b.done()


# =========================================================================================================================
# constant divisions and fdiv
# =========================================================================================================================
DENOMINATORS = np.array([100.0, 48.0, 6.0, 3.0, 7.0, 2.0 ** 100, 1e38, 2.0 ** -100, SUBNORMAL_MAX, SUBNORMAL_MIN, -3.0, 1.0,
                         2.0 ** 126, 0.1, -2.0 ** -126, 1.0000001], dtype=F32)
EDGE = 2.0 ** -100


def special_numerators():
    e = F32(EDGE)
    return [("p2m100", e), ("m2m100", -e), ("below_2m100", np.nextafter(e, F32(0.0))), ("above_2m100", np.nextafter(e, F32(1.0))),
            ("neg_below_2m100", -np.nextafter(e, F32(0.0))), ("neg_above_2m100", -np.nextafter(e, F32(1.0))), ("p2m120", F32(2.0 ** -120)),
            ("subnormal_max", F32(SUBNORMAL_MAX)), ("subnormal_min", F32(SUBNORMAL_MIN)), ("pzero", F32(0.0)), ("nzero", F32(-0.0)),
            ("flt_max", F32(FLT_MAX)), ("neg_flt_max", F32(-FLT_MAX)), ("pinf", F32(np.inf)), ("ninf", F32(-np.inf)), ("nan", F32(np.nan))]


def sweep(rng, n):
    """uniform bits per binade over the whole exponent range (biased 0 .. 254), either sign"""
    u = (rng.integers(0, 255, n).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)
    return ref.from_bits(u)


def divisions(seed=20250103):
    b = Builder(seed)
    rng = b.rng
    den = np.resize(DENOMINATORS, 64)
    for k, (name, v) in enumerate(special_numerators()):
        x = b.ordinary(64)
        lane = (7 * k + 3) % 64 if k % 4 else (0 if k % 8 else 63)
        x[lane] = v
        b.add("div_one_lane", f"{name}_lane{lane}", x0=x, x1=np.roll(den, k))
        b.add("div_all_lanes", f"{name}_all", x0=np.full(64, v, dtype=F32), x1=np.roll(den, k))
    # ordinary numerators in every lane: the fast path as div_const takes it
    for k in range(4):
        b.add("div_ordinary", f"ordinary{k}", x0=(b.ordinary(64) * F32(100.0 if k % 2 else 48.0)), x1=np.roll(den, k))
    # the exponent sweep: 4096 numerators per divisor; sorted by magnitude, so that waves wholly above 2^-100 (the fast path) and waves
    # with lanes below it (the fallback) both occur
    for d in (100, 48):
        v = sweep(rng, 4096)
        v = v[np.argsort(np.abs(v), kind="stable")]
        for k in range(64):
            b.add("div_sweep", f"sweep{d}_{k}", x0=v[64 * k: 64 * k + 64], x1=np.full(64, float(d), dtype=F32) if k % 2 else np.roll(den, k))
    # quotients that are exact (k * C * 2^e) and the numerators one ulp either side
    for d in (100, 48):
        for k in range(6):
            q = (rng.integers(1, 1 << 17, 64) * 2.0 ** rng.integers(-110, 100, 64))
            x = (q * d).astype(F32)
            assert np.array_equal(x.astype(np.float64), q * d)
            b.add("div_exact", f"exact{d}_{k}", x0=x, x1=np.full(64, float(d), dtype=F32))
            b.add("div_exact", f"exact{d}_{k}_up", x0=ref.from_bits(ref.bits(x) + np.uint32(1)), x1=np.full(64, float(d), dtype=F32))
            b.add("div_exact", f"exact{d}_{k}_down", x0=ref.from_bits(ref.bits(x) - np.uint32(1)), x1=np.full(64, float(d), dtype=F32))
    # quotients half-way between two binary32 numbers cannot come from a binary32 numerator over 100 or 48 in the normal range (the
    # quotient would need more than 24 bits times an odd factor), but they do on the subnormal grid: numerators (2 j + 1) * C * 2^-150
    for d in (100, 48):
        j = rng.integers(0, 1 << 16, 64)
        x = ((2 * j + 1) * d * 2.0 ** -150)
        xf = x.astype(F32)
        keep = xf.astype(np.float64) == x
        b.add("div_halfway", f"halfway{d}", x0=np.where(keep, xf, F32(d * 2.0 ** -150)), x1=np.full(64, float(d), dtype=F32))
    return b.done()


# =========================================================================================================================
# hypot_f
# =========================================================================================================================
def near_midpoints(seed=20250104, n=20000):
    """integer X in [2^23, 2^24), y = Y / 2^12 with Y^2 within 2^19 of X * 2^24 + 2^22: x^2 + y^2 = (X + 1/2)^2 + (Y^2 - X 2^24 - 2^22) / 2^24,
    so the square root lies within 2^-5 / (2 X) < 2^-28 of the binary32 midpoint X + 1/2 -- about an ulp of its binary64 value (2^-29)"""
    rng = np.random.default_rng(seed)
    out = []
    for X in rng.integers(1 << 23, 1 << 24, n).tolist():
        T = X * (1 << 24) + (1 << 22)
        y0 = math.isqrt(T)
        for Y in (y0 - 1, y0, y0 + 1):
            if abs(Y * Y - T) < (1 << 19) and Y < (1 << 24):
                out.append((X, Y))
    return out


def hypot_pairs(seed=20250105):
    """-> (x [n], y [n], family [n]) of the hypot families, in pairs (the records are cut from them 64 at a time)"""
    rng = np.random.default_rng(seed)
    xs, ys, fam = [], [], []

    def put(f, x, y):
        xs.append(F32(x)); ys.append(F32(y)); fam.append(f)      # noqa: E702

    mid = near_midpoints()
    for scale, f in ((0, "mid"), (-60, "mid_2m60"), (-100, "mid_2m100"), (60, "mid_2p60")):
        for X, Y in mid:
            put(f, math.ldexp(X, scale), math.ldexp(Y, scale - 12))
    # Pythagorean pairs: the hypotenuse representable, and a 25-bit odd hypotenuse (an exact binary32 tie) from p^2 - q^2, 2 p q
    for a, bb in ((3, 4), (5, 12), (8, 15), (20, 21), (119, 120), (696, 697)):
        put("pythagorean", a, bb); put("pythagorean", -bb, a); put("pythagorean", a * 2.0 ** -70, bb * 2.0 ** -70)      # noqa: E702
    n_tie = 0
    while n_tie < 40:
        p, q = int(rng.integers(2900, 5792)), int(rng.integers(1, 2900))
        h, a, bb = p * p + q * q, p * p - q * q, 2 * p * q
        if (1 << 24) < h < (1 << 25) and (h & 1) and a < (1 << 24) and bb < (1 << 24) and a > 0:
            put("pythagorean_tie", a, bb); put("pythagorean_tie", -a * 2.0 ** 30, bb * 2.0 ** 30)      # noqa: E702
            n_tie += 1
    for v in (0.0, 1.5, -2.75e-3, SUBNORMAL_MIN, FLT_MAX):
        for z in (0.0, -0.0):
            put("zero_operand", v, z); put("zero_operand", z, v)      # noqa: E702
    for z0 in (0.0, -0.0):
        for z1 in (0.0, -0.0):
            put("zero_operand", z0, z1)
    for v in (1.0, 3.0, 0.0123, 1e-30, 2.0 ** -140, 1e30, float(ref.from_bits(0x3f8ccccd)), SUBNORMAL_MAX, 2.0 ** 127):
        put("equal", v, v); put("equal", v, -v)      # noqa: E702
    put("range", SUBNORMAL_MIN, 0.0); put("range", SUBNORMAL_MIN, SUBNORMAL_MIN); put("range", SUBNORMAL_MIN, -2 * SUBNORMAL_MIN)      # noqa: E702
    put("range", SUBNORMAL_MAX, 0.0); put("range", SUBNORMAL_MAX, SUBNORMAL_MAX); put("range", SUBNORMAL_MAX, 2.0 ** -126)      # noqa: E702
    for k in (3, 5, 1000, 0x3fffff):
        put("range", k * SUBNORMAL_MIN, (k + 1) * SUBNORMAL_MIN)
    put("range", FLT_MAX, 0.0); put("range", FLT_MAX, FLT_MAX); put("range", -FLT_MAX, 2.0 ** 127); put("range", 2.0 ** 127, 2.0 ** 127)      # noqa: E702
    for base in (1.0, 1.2345678, 2.0 ** -60, 3.0e20):
        m = float(F32(base))
        put("range_apart", m, m * 2.0 ** -40); put("range_apart", m * 2.0 ** -40, -m)      # noqa: E702
        put("range_apart", m, m * 2.0 ** -26 * 1.5); put("range_apart", m * 2.0 ** -26, m)      # noqa: E702
        put("range_apart", float(ref.from_bits(ref.bits(F32(m)) | np.uint32(1))), m * 2.0 ** -13)
    bulk_x, bulk_y = sweep(rng, 4096), sweep(rng, 4096)
    for x, y in zip(bulk_x, bulk_y):
        put("bulk", x, y)
    return np.array(xs, dtype=F32), np.array(ys, dtype=F32), np.array(fam)


def hypot_records(pairs, seed=20250106):
    b = Builder(seed)
    x, y, fam = pairs
    n = len(x)
    pad = (-n) % 64
    x = np.concatenate([x, np.full(pad, 3.0, dtype=F32)])
    y = np.concatenate([y, np.full(pad, 4.0, dtype=F32)])
    for k in range(len(x) // 64):
        b.add("hypot", f"hypot{k}:{fam[min(64 * k, n - 1)]}", x0=x[64 * k: 64 * k + 64], x1=y[64 * k: 64 * k + 64])
    return b.done()


# =========================================================================================================================
# the filter sum, the integer scan and the DPP building blocks
# =========================================================================================================================
def tiles(seed=20250107):
    b = Builder(seed)
    rng = b.rng

    def tile(re, im):
        t = np.empty(680, dtype=F32)
        t[0::2] = re
        t[1::2] = im
        return t

    i = np.arange(340)
    # every window has its own sum: 125 L + 300 and -(250 L + 600) -- a lane that reads 5 (L +- 1), or a term too few, shows
    b.add("tile_index", "index", tile=tile(i.astype(F32), (-2.0 * i).astype(F32)))
    b.add("tile_index", "index_sq", tile=tile((i * i).astype(F32), (i % 7 - 3).astype(F32)))
    # cancellation of 2^24 : 1 -- +-2^24 a few samples apart among ones; the window slides by 5, so the pair sits at every position
    for k, (gap, period) in enumerate(((1, 25), (3, 25), (7, 27), (12, 31), (24, 50), (2, 11))):
        re = np.ones(340)
        im = rng.choice([1.0, -1.0, 0.5], 340)
        re[k::period] = 2.0 ** 24
        re[k + gap::period] = -2.0 ** 24
        im[(k + 5)::period] = -2.0 ** 24
        im[(k + 5 + gap)::period] = 2.0 ** 24
        b.add("tile_cancel", f"cancel_gap{gap}_period{period}", tile=tile(re, im))
    # running sums that cross binades both ways
    for k in range(6):
        mag = 2.0 ** rng.integers(-6, 7, 680) * (1.0 + rng.integers(0, 1 << 23, 680) * 2.0 ** -23)
        b.add("tile_binades", f"binades{k}", tile=(mag * rng.choice([-1.0, 1.0], 680)).astype(F32))
    # subnormal terms and sums
    for k in range(4):
        u = rng.integers(0, 1 << (8 + 3 * k), 680).astype(np.uint32) | (rng.integers(0, 2, 680).astype(np.uint32) << 31)
        b.add("tile_subnormal", f"subnormal{k}", tile=ref.from_bits(u))
    b.add("tile_subnormal", "subnormal_to_normal", tile=ref.from_bits(rng.integers(0x00700000, 0x00900000, 680).astype(np.uint32) | (rng.integers(0, 2, 680).astype(np.uint32) << 31)))
    # -0.0 terms: all of them, and among zeros and cancelling pairs
    b.add("tile_negzero", "all_negzero", tile=np.full(680, -0.0, dtype=F32))
    t = np.where(rng.integers(0, 2, 680) == 0, F32(-0.0), F32(0.0)).astype(F32)
    b.add("tile_negzero", "signed_zeros", tile=t)
    t = t.copy()
    t[10::50] = 1.5
    t[12::50] = -1.5
    b.add("tile_negzero", "zeros_and_pairs", tile=t)
    return b.done()


def scans(seed=20250108):
    b = Builder(seed)
    rng = b.rng
    for fill in FILLS:
        b.add("scan_ones", f"ones_fill{fill}", iv=np.ones(64, dtype=np.int32), fill=fill)
        b.add("scan_ones", f"all_bits_fill{fill}", iv=np.full(64, -1, dtype=np.int32), fill=fill)
        b.add("scan_wrap", f"int_max_fill{fill}", iv=np.full(64, 2 ** 31 - 1, dtype=np.int32), fill=fill)
        b.add("scan_wrap", f"int_min_fill{fill}", iv=np.full(64, -2 ** 31, dtype=np.int32), fill=fill)
        b.add("scan_wrap", f"min_max_fill{fill}", iv=np.where(np.arange(64) % 2 == 0, -2 ** 31, 2 ** 31 - 1).astype(np.int32), fill=fill)
        b.add("scan_index", f"lane_index_fill{fill}", iv=(np.arange(64) * 0x01010101 + 1).astype(np.int64).astype(np.int32), fill=fill)
    for lane in range(64):
        iv = np.zeros(64, dtype=np.int32)
        iv[lane] = 1
        b.add("scan_single", f"single{lane}", iv=iv, fill=FILLS[(lane + 1) % 3] if lane % 2 else 0x7e7e0000 + lane)
    for k in range(8):
        b.add("scan_random", f"random{k}", fill=int(rng.integers(-2 ** 31, 2 ** 31)))
    return b.done()


# =========================================================================================================================
# everything, and what it reaches
# =========================================================================================================================
def concat(sets):
    return Set(np.concatenate([s.recs for s in sets]), np.concatenate([s.family for s in sets]), np.concatenate([s.name for s in sets]))


GROUPS = ("sums", "bulk_sums", "two_carry", "divisions", "hypot", "tiles_scans")     # what one launch of the suites takes


def group_of(family):
    """the launch a record goes with (the emulator spends ~15 ms on a record: a group stays within a few seconds)"""
    if family == "bulk":
        return "bulk_sums"
    if family.startswith("two_carry"):
        return "two_carry"
    if family.startswith("div_"):
        return "divisions"
    if family == "hypot":
        return "hypot"
    if family.startswith(("tile_", "scan_")):
        return "tiles_scans"
    return "sums"


def build():
    pairs = hypot_pairs()
    return concat([sums(), two_carry(), divisions(), hypot_records(pairs), tiles(), scans()]), pairs


def sum_facts(rec):
    """what the reference says about one record's sums: the flags' predicates, where the 128 partial sums from `carry` are outside
    the carry's binade (or on its edge), the ties of either half, the largest |t|"""
    c = rec["carry"]
    xs = np.concatenate([rec["x0"], rec["x1"]])
    cb = np.uint32(ref.bits(c))
    part = ref.bits(ref.seq_sum(np.array([c], dtype=F32), xs[None, :])[0])
    out = (((part ^ cb) & np.uint32(0xff800000)) != 0) | ((part & np.uint32(0x007fffff)) == 0)
    e_b = (int(cb) >> 23) & 0xff
    if 1 <= e_b <= 254:
        t = ref.scaled(c, xs)
        fin = np.isfinite(t)
        tie = fin & (np.abs(t) < ref.TWO22) & (np.abs(t - np.rint(np.where(fin, t, 0.0))) == 0.5)
        tmax = float(np.max(np.abs(t[fin]))) if fin.any() else 0.0
    else:
        tie, tmax = np.zeros(128, dtype=bool), 0.0
    return dict(pred=ref.scan_predicate(c, rec["x0"]), pred_pair=ref.scan_predicate(c, xs), pred2=ref.scan2_predicate(c, rec["carry_b"], rec["x0"]),
                out=out, tie=tie, tmax=tmax, part=part)
